"""pf_encode_jpeg, CPU tier: the numpy restatement (tests/jpeg_enc_ref.py) is libjpeg(-turbo) through Pillow byte for byte, and the
engine -- here the SIMT-emulator build of the same kernels -- is the restatement, whole file, byte for byte.  The check_* functions
take an engine; tests/test_gpu_jpeg_encode.py runs them on the HIP library.  Exact bytes throughout: no tolerance anywhere."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd._native import PeppaHipError
from tests import jpeg_enc_ref as ref
from tests.test_jpeg_decode import _image

# H x W: the smallest image; a narrow partly covered block; an exact MCU; a one-pixel overhang (dummy luma blocks on both edges in
# 4:2:0); an even overhang (the down-sampled-row rule); partial blocks on both edges; another block multiple; more blocks per interval
# than a wave has lanes (102 in 4:2:0, 99 in 4:4:4); 9 / 17 intervals, so RSTm wraps past 7
SHAPES = [(1, 1), (8, 5), (16, 16), (17, 17), (18, 23), (33, 47), (40, 24), (72, 264), (136, 40)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
SAMPLINGS = (444, 422, 420)
# (content, quality): texture; noise at 100 (long codes, many 0xFF to stuff); constant 0xFF (EOB-only blocks, zero DC differences,
# intervals of a few bytes, a pad byte that needs stuffing or not); a 0 / 255 checkerboard at 100 and 1 (largest magnitudes, both
# clamps of the table scaling); a smooth ramp at 30 (zero runs beyond 15: ZRL)
CONTENTS = [("texture", 75), ("texture", 90), ("noise", 100), ("white", 75), ("checker", 100), ("checker", 1), ("ramp", 30)]


def make_image(kind, H, W, seed=0):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "texture":
        return _image(H, W, seed=7 * H + W + seed)
    if kind == "noise":
        return np.random.default_rng(1000 * H + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((H, W, 3), 255, np.uint8)
    if kind == "checker":
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    if kind == "ramp":
        return np.stack([(xx * 255) // max(W - 1, 1), (yy * 255) // max(H - 1, 1), ((xx + yy) * 255) // max(H + W - 2, 1)], -1).astype(np.uint8)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, H, W, quality, sampling, seed=0):
    return ref.encode(make_image(kind, H, W, seed), quality, sampling)


def pillow_encode(bgr, quality, sampling):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, format="JPEG", quality=quality, subsampling={444: 0, 422: 1, 420: 2}[sampling],
                                                                restart_marker_rows=1)
    return buf.getvalue()


def pillow_decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return "lengths %d / %d, first differing byte %s" % (len(a), len(b), d[0] if len(d) else None)


def raw_encode(engine, images, mem, n, H, W, stride, quality, sampling, out, capacity, sizes, out_mem):
    rc = engine.lib.pf_encode_jpeg(engine.h, _native._ptr(images), mem, n, H, W, stride, quality, sampling, _native._ptr(out), capacity,
                                   _native._ptr(sizes), out_mem)
    engine._check(rc, "pf_encode_jpeg")


# ---- test 1: the restatement is libjpeg -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_restatement_is_pillow(shape):
    H, W = shape
    for kind in ("texture", "noise"):
        img = make_image(kind, H, W)
        for sampling in SAMPLINGS:
            for quality in (30, 75, 90, 100):
                want = pillow_encode(img, quality, sampling)
                got = ref.encode(img, quality, sampling)
                assert got == want, (kind, sampling, quality, first_difference(got, want))


def test_restatement_is_pillow_on_the_edge_contents():
    for kind, quality in CONTENTS[3:]:
        for H, W in ((17, 17), (18, 23), (40, 24)):
            for sampling in SAMPLINGS:
                assert reference(kind, H, W, quality, sampling) == pillow_encode(make_image(kind, H, W), quality, sampling), (kind, quality, H, W)


# ---- test 2: the engine is the restatement ----------------------------------------------------------------------------------------

def check_shape(engine, shape):
    H, W = shape
    for kind, quality in CONTENTS:
        img = make_image(kind, H, W)
        for sampling in SAMPLINGS:
            want = reference(kind, H, W, quality, sampling)
            got = engine.encode_jpeg(img, quality=quality, subsampling=sampling)
            assert len(got) == 1
            assert got[0] == want, (kind, quality, sampling, first_difference(got[0], want))
            # with the bound as capacity no case reports a negative size
            bound = engine.encode_jpeg_bound(H, W, sampling)
            assert bound >= len(want)
            out, sizes = np.full((bound + 8,), 0xAB, np.uint8), np.zeros((1,), np.int32)
            raw_encode(engine, img, _native.PF_MEM_HOST, 1, H, W, 3 * W, quality, sampling, out, bound, sizes, _native.PF_MEM_HOST)
            assert sizes[0] == len(want) and out[:sizes[0]].tobytes() == want and (out[sizes[0]:] == 0xAB).all()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_engine_is_the_restatement(emu_engine, shape):
    check_shape(emu_engine, shape)


# ---- test 3: batches and memory ---------------------------------------------------------------------------------------------------

BATCH = dict(H=33, W=47, n=5)


def batch_images():
    H, W, n = BATCH["H"], BATCH["W"], BATCH["n"]
    kinds = ["texture", "noise", "ramp", "white", "texture"]
    return np.stack([make_image(k, H, W, seed=i) for i, k in enumerate(kinds)])


def check_batches(engine, dev_bytes, sync):
    """dev_bytes(array or (n, fill)) -> (device pointer, read() -> uint8 [n])"""
    H, W, n = BATCH["H"], BATCH["W"], BATCH["n"]
    imgs = batch_images()
    for quality, sampling in ((90, 420), (100, 444), (60, 422)):
        want = [ref.encode(im, quality, sampling) for im in imgs]
        assert len(set(want)) == n
        assert engine.encode_jpeg(imgs, quality=quality, subsampling=sampling) == want
        # strided host rows
        stride = 3 * W + 5
        padded = np.full((n, H, stride), 0xCD, np.uint8)
        padded[:, :, :3 * W] = imgs.reshape(n, H, 3 * W)
        view = padded[:, :, :3 * W].reshape(n, H, W, 3)
        assert engine.encode_jpeg(view, quality=quality, subsampling=sampling) == want
        # device memory at odd byte offsets, strided rows, device output and device sizes, canaries everywhere
        cap = max(len(w) for w in want) + 7
        for in_off, out_off in ((1, 0), (2, 3), (3, 1)):
            src = np.concatenate([np.zeros(in_off, np.uint8), padded.reshape(-1)])
            d_src, _ = dev_bytes(src)
            d_out, r_out = dev_bytes((n * cap + 16, 0xAB))
            d_sizes, r_sizes = dev_bytes((4 * n + 8, 0xAB))
            engine.encode_jpeg_device(d_src + in_off, n, H, W, d_out + out_off, cap, d_sizes + 4, quality=quality, subsampling=sampling,
                                      row_stride=stride)
            sync()
            out, sz = r_out(), r_sizes()
            sizes = sz[4:4 + 4 * n].copy().view(np.int32)
            assert sizes.tolist() == [len(w) for w in want]
            assert (sz[:4] == 0xAB).all() and (sz[4 + 4 * n:] == 0xAB).all()
            assert (out[:out_off] == 0xAB).all() and (out[out_off + n * cap:] == 0xAB).all()
            for i in range(n):
                slot = out[out_off + i * cap: out_off + (i + 1) * cap]
                assert slot[:sizes[i]].tobytes() == want[i], (i, in_off, out_off)
                assert (slot[sizes[i]:] == 0xAB).all(), i


def _host_bytes(spec):
    a = np.array(spec, np.uint8) if isinstance(spec, np.ndarray) else np.full((spec[0],), spec[1], np.uint8)
    return a.ctypes.data, lambda: a.copy()


def test_batches_and_memory(emu_engine):
    check_batches(emu_engine, _host_bytes, emu_engine.sync)          # the emulator's device memory is host memory


# ---- test 4: capacity -------------------------------------------------------------------------------------------------------------

def check_capacity(engine):
    H, W = 40, 56
    kinds = ["ramp", "noise", "white", "texture"]
    imgs = np.stack([make_image(k, H, W) for k in kinds])
    for sampling in (420, 444):
        want = [ref.encode(im, 75, sampling) for im in imgs]
        lens = sorted(len(w) for w in want)
        assert len(want[1]) == lens[-1] > lens[-2] + 8
        cap = (lens[-1] + lens[-2]) // 2                     # the noise image does not fit, the others do
        out, sizes = np.full((8 + 4 * cap + 8,), 0xAB, np.uint8), np.zeros((4,), np.int32)
        raw_encode(engine, imgs, _native.PF_MEM_HOST, 4, H, W, 3 * W, 75, sampling, out[8:], cap, sizes, _native.PF_MEM_HOST)
        assert sizes.tolist() == [len(want[0]), -len(want[1]), len(want[2]), len(want[3])]
        assert (out[:8] == 0xAB).all() and (out[8 + 4 * cap:] == 0xAB).all()
        for i in (0, 2, 3):
            slot = out[8 + i * cap: 8 + (i + 1) * cap]
            assert slot[:sizes[i]].tobytes() == want[i] and (slot[sizes[i]:] == 0xAB).all(), i
        # the Python call repeats with the bound
        assert engine.encode_jpeg(imgs, quality=75, subsampling=sampling, capacity=cap) == want
        assert engine.encode_jpeg_bound(H, W, sampling) >= lens[-1]
    assert engine.encode_jpeg_bound(0, 8, 420) == 0 and engine.encode_jpeg_bound(8, 8, 411) == 0 and engine.encode_jpeg_bound(8, 65536, 444) == 0
    assert engine.encode_jpeg_bound(65535, 65535, 444) == 0          # its bound does not fit the int of sizes[]: refused


def test_capacity(emu_engine):
    check_capacity(emu_engine)


# ---- test 5: round trip through the project's own decoder -------------------------------------------------------------------------

def check_round_trip(engine):
    cases = [(make_image("texture", 72, 104), 85, 420), (make_image("texture", 67, 101), 92, 444)]
    files = [engine.encode_jpeg(im, quality=q, subsampling=s)[0] for im, q, s in cases]
    try:
        for entropy in (2, 1):
            engine.set_option(_native.PF_OPT_JPEG_ENTROPY, entropy)
            engine.profile_enable(True)
            for data, (im, q, s) in zip(files, cases):
                assert engine.jpeg_info(data) == (im.shape[0], im.shape[1], 3, s)
                got = engine.decode_jpeg(data)[3]
                assert np.array_equal(got, pillow_decode(data)), (entropy, s)
            names = list(engine.profile_fetch())
            engine.profile_enable(False)
            assert ("jpeg_huffman" in names) == (entropy == 2), names
    finally:
        engine.profile_enable(False)
        engine.set_option(_native.PF_OPT_JPEG_ENTROPY, 0)


def test_round_trip_through_the_decoder(emu_engine):
    check_round_trip(emu_engine)


# ---- test 6: repeatability and dispatch -------------------------------------------------------------------------------------------

def check_repeatability(engine):
    img = make_image("noise", 72, 264)
    engine.profile_enable(True)
    a = engine.encode_jpeg(img, quality=95, subsampling=420)
    log = engine.launch_log()
    names = list(engine.profile_fetch())
    engine.profile_enable(False)
    b = engine.encode_jpeg(img, quality=95, subsampling=420)
    assert a == b and a[0] == reference("noise", 72, 264, 95, 420)
    for kernel in ("jpeg_enc_blocks", "jpeg_enc_entropy", "jpeg_enc_pack"):
        assert any(kernel in entry for entry in log), (kernel, log)
        assert kernel in names, names
    # other tables in between: the handle rebuilds them
    assert engine.encode_jpeg(img, quality=40, subsampling=444)[0] == reference("noise", 72, 264, 40, 444)
    assert engine.encode_jpeg(img, quality=95, subsampling=420) == a


def test_repeatability_and_dispatch(emu_engine):
    check_repeatability(emu_engine)


# ---- test 7: refusals -------------------------------------------------------------------------------------------------------------

def check_refusals(engine):
    H, W = 16, 24
    img = make_image("texture", H, W)
    out, sizes = np.full((4096,), 0xAB, np.uint8), np.full((1,), -7, np.int32)
    ok = dict(images=img, mem=_native.PF_MEM_HOST, n=1, H=H, W=W, stride=3 * W, quality=90, sampling=420, out=out, capacity=4096, sizes=sizes,
              out_mem=_native.PF_MEM_HOST)
    for change, why in ((dict(quality=0), r"quality must lie in \[1, 100\] \(got 0\)"), (dict(quality=101), "quality must lie"),
                        (dict(sampling=411), r"subsampling must be 444, 422 or 420 \(got 411\)"),
                        (dict(H=0), r"height and width must lie in \[1, 65535\]"), (dict(W=65536, stride=3 * 65536), "height and width must lie"),
                        (dict(H=65535, W=65535, stride=3 * 65535), "too large"),
                        (dict(images=None), "images must not be NULL"), (dict(out=None), "out and sizes must not be NULL"),
                        (dict(sizes=None), "out and sizes must not be NULL"), (dict(n=0), r"n must be at least 1 \(got 0\)"),
                        (dict(stride=3 * W - 1), "row_stride 71 is below 3 \\* width = 72"), (dict(capacity=628), "capacity 628 is below the header's 629 bytes"),
                        (dict(mem=7), "mem must be"), (dict(out_mem=3), "out_mem must be"),
                        (dict(mem=_native.PF_MEM_RESIDENT, n=2), "PF_MEM_RESIDENT is one frame, n = 2"),
                        (dict(mem=_native.PF_MEM_RESIDENT, images=None), "no resident frame of this size")):
        with pytest.raises(PeppaHipError, match="pf_encode_jpeg: .*" + why):
            raw_encode(engine, **dict(ok, **change))
    assert (out == 0xAB).all() and sizes[0] == -7             # refused calls write nothing
    with pytest.raises(ValueError, match="uint8"):
        engine.encode_jpeg(img.astype(np.float32))
    # afterwards the handle still works, the resident frame included
    assert engine.encode_jpeg(img, quality=90, subsampling=420)[0] == ref.encode(img, 90, 420)
    engine.set_frame(img)
    raw_encode(engine, **dict(ok, mem=_native.PF_MEM_RESIDENT, images=None))
    assert out[:sizes[0]].tobytes() == ref.encode(img, 90, 420)
    with pytest.raises(PeppaHipError, match="no resident frame of this size"):
        raw_encode(engine, **dict(ok, mem=_native.PF_MEM_RESIDENT, images=None, H=8))


def test_refusals(emu_engine):
    check_refusals(emu_engine)

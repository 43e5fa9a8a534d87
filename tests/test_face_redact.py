"""Face redaction (pf_redact_faces / pf_face_redact, csrc/k_redact.h) on the CPU tier, through the SIMT emulator: every output byte
against the integer restatement tests/redact_ref.py -- the masks' case table under every mode and mask, frames smaller than a tile, a
cell and a window, overlap with select, dead and invalid slots, device outputs through unaligned pointers, the ABI's refusals and the
last-call accessor after the entry points the emulator can run.  Nothing here has a tolerance.  Input frames are uniform random bytes
(a smooth frame would hide wrong sums) and every output buffer starts as 0xAB, so a byte left unwritten shows.  The same checks run on
a real MI355X from tests/test_gpu_face_redact.py, which imports the ``check_*`` functions from here."""
import ctypes as C

import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd._native import PeppaHipError
from peppa_pig_face_landmark_amd.synth import make_frame as synth_frame, plant_rows
from tests import align_ref as ar
from tests import mask_ref as mr
from tests import redact_ref as rr
from tests.test_face_masks import _load_small_student

# (mode, strength): fill; mosaic 4, 8, 16; blur 1, 7, 32 (32 exceeds the tile height and reaches the border from every pixel of 120 rows)
MODES = [("fill", 0), ("mosaic", 4), ("mosaic", 8), ("mosaic", 16), ("blur", 1), ("blur", 7), ("blur", 32)]
MODE_NO = {"fill": rr.FILL, "mosaic": rr.MOSAIC, "blur": rr.BLUR}
# (label_mask, pad): all face labels, the eyes only, the background, the boxes bare and grown by 9
MASKS = [(0x1FE, 0), (0x030, 0), (0x001, 0), (0x200, 0), (0x200, 9)]
COLOUR = 0x0A1B2C          # channel 0 = 0x2C, 1 = 0x1B, 2 = 0x0A
# the restatement's selected-pixel counts per MASKS entry: a case must not pass vacuously
COUNTS = {
    "upright_io40_odd": [5776, 153, 13705, 7905, 11433],
    "rect_integer": [6400, 0, 12800, 6400, 9604],
    "outside": [0, 0, 19200, 0, 0],
    "huge": [19200, 0, 0, 19200, 19200],
}


def random_frame(H, W, seed, F=None):
    shape = (H, W, 3) if F is None else (F, H, W, 3)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def sentinel(*shape):
    return np.full(shape, 0xAB, np.uint8)


def assert_frames_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d bytes differ, first at %s" % (what, int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad)))


def check_one(engine, frame, kps, maps, mode, strength, label_mask, pad, select=None, count=None, kps_dtype=np.float32):
    """One stage-level call on one frame against the restatement; returns (out, number of selected pixels)."""
    H, W = frame.shape[:2]
    want, valid, n_sel = rr.frame_reference(frame, kps, count, select, MODE_NO[mode], label_mask, strength, pad, COLOUR, maps=maps)
    got, got_valid = engine.redact_faces(frame, np.asarray(kps, kps_dtype)[None], counts=None if count is None else [count],
                                         select=None if select is None else np.asarray(select)[None], mode=mode, labels=label_mask,
                                         strength=strength, pad=pad, colour=COLOUR, out=sentinel(1, H, W, 3))
    what = "%s %d mask 0x%x pad %d" % (mode, strength, label_mask, pad)
    assert_frames_equal(got[0], want, what)
    assert np.array_equal(got_valid[0], valid), what
    if n_sel and mode != "fill":
        assert (got[0] != frame).any(), what
    if n_sel == 0:
        assert np.array_equal(got[0], frame), what
    return got[0], n_sel


# ---- test 1: the restatement over the masks' case table -------------------------------------------------------------------------

def check_restatement(engine, case):
    name, H, W, faces = case
    kps = np.stack(faces)
    maps = mr.case_reference(case)
    frame = random_frame(H, W, seed=1000 + mr.CASE_IDS.index(name))
    engine.profile_enable(True)
    counts = []
    for label_mask, pad in MASKS:
        for mode, strength in MODES:
            out, n_sel = check_one(engine, frame, kps, maps, mode, strength, label_mask, pad)
        counts.append(n_sel)
    log = engine.launch_log()
    engine.profile_enable(False)
    assert any("redact_kernel" in k for k in log) and any("mask_fill_kernel" in k for k in log), log
    if name in COUNTS:
        assert counts == COUNTS[name], counts
    # float64 landmarks of the same values: the same bytes
    a, _ = check_one(engine, frame, kps, maps, "blur", 7, 0x1FE, 0)
    b, _ = check_one(engine, frame, kps, maps, "blur", 7, 0x1FE, 0, kps_dtype=np.float64)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("case", mr.CASES, ids=mr.CASE_IDS)
def test_restatement(emu_engine, case):
    check_restatement(emu_engine, case)


# ---- test 2: a frame smaller than a tile, a cell and a window ---------------------------------------------------------------------

def _round_mean(a):
    """(sum + (n >> 1)) // n per channel of pixels a [..., 3]."""
    a = np.asarray(a, np.int64).reshape(-1, 3)
    return (a.sum(0) + (len(a) >> 1)) // len(a)


def check_small_frames(engine):
    H, W = 10, 13
    kps = ar.make_landmarks(6, 5, 600, 5, seed=6)[None]
    maps = mr.frame_maps(kps, None, H, W)
    assert maps[3].all() and maps[2][0].tolist() == [0, 0, W, H] and int((maps[0] != 0).sum()) == 130
    frame = random_frame(H, W, seed=77)
    out, n = check_one(engine, frame, kps, maps, "blur", 32, 0x200, 0)          # every window is the whole frame
    assert n == 130 and (out == _round_mean(frame)).all()
    out, _ = check_one(engine, frame, kps, maps, "mosaic", 16, 0x200, 0)        # one 10 x 13 cell
    assert (out == _round_mean(frame)).all()
    out, _ = check_one(engine, frame, kps, maps, "mosaic", 4, 0x200, 0)         # clipped cells of 4, 8 and 2 pixels
    assert (out[8:, 12] == _round_mean(frame[8:, 12])).all() and (out[8:, :4] == _round_mean(frame[8:, :4])).all()
    assert (out[4:8, 12] == _round_mean(frame[4:8, 12])).all()
    for mode, strength in MODES:
        for label_mask in (0x1FE, 0x001, 0x200):
            check_one(engine, frame, kps, maps, mode, strength, label_mask, 0)
    # one row of five pixels
    kps1 = ar.make_landmarks(2, 0, 600, 5, seed=6)[None]
    maps1 = mr.frame_maps(kps1, None, 1, 5)
    frame1 = random_frame(1, 5, seed=78)
    for mode, strength in MODES:
        for label_mask in (0x1FE, 0x001, 0x200):
            check_one(engine, frame1, kps1, maps1, mode, strength, label_mask, 2)
    out, n = check_one(engine, frame1, kps1, maps1, "blur", 1, 0x200, 2)
    assert n == 5 and (out[0, 0] == _round_mean(frame1[0, :2])).all() and (out[0, 2] == _round_mean(frame1[0, 1:4])).all()
    # a 4 x 4 cell whose sum is 2: 2 / 16 = 0.125 -> (2 + 8) // 16 = 0; the half itself, 8 / 16, rounds up to 1
    kps4 = ar.make_landmarks(2, 2, 600, 5, seed=6)[None]
    maps4 = mr.frame_maps(kps4, None, 4, 4)
    frame4 = np.zeros((4, 4, 3), np.uint8)
    frame4[0, 0] = (2, 1, 0)
    frame4[1, 1] = (0, 7, 0)
    frame4[3, 3] = (0, 0, 7)
    out, n = check_one(engine, frame4, kps4, maps4, "mosaic", 4, 0x200, 0)
    assert n == 16 and (out == (0, 1, 0)).all()           # sums 2, 8, 7 -> 0, 1 (a half rounds up), 0
    frame2 = np.zeros((2, 2, 3), np.uint8)               # a clipped cell of n = 4 whose sum is 2: 2 / 4 is the half as well
    frame2[0, 0] = (2, 1, 3)
    kps2 = ar.make_landmarks(1, 1, 600, 5, seed=6)[None]
    out, n = check_one(engine, frame2, kps2, mr.frame_maps(kps2, None, 2, 2), "mosaic", 4, 0x200, 0)
    assert n == 4 and (out == (1, 0, 1)).all()


def test_small_frames(emu_engine):
    check_small_frames(emu_engine)


# ---- test 3: overlap, order and select --------------------------------------------------------------------------------------------

OVERLAP_COUNTS = {(1, 1): (8353, 12424, 10847), (0, 1): (2646, 8800, 10847), (1, 0): (5707, 9064, 10847), (0, 0): (0, 0, 10847)}


def check_overlap_select(engine):
    H, W = 120, 160
    kps = np.stack([ar.make_landmarks(70, 60, 40, 10, seed=30), ar.make_landmarks(100, 70, 40, -10, seed=31)])
    maps = mr.frame_maps(kps, None, H, W)
    frame = random_frame(H, W, seed=33)
    for select, want in OVERLAP_COUNTS.items():
        got = []
        for label_mask, pad in ((0x1FE, 0), (0x200, 3), (0x001, 0)):
            for mode, strength in (("mosaic", 8), ("blur", 7), ("fill", 0)):
                out, n = check_one(engine, frame, kps, maps, mode, strength, label_mask, pad, select=select)
            got.append(n)
            if select == (0, 1) and label_mask == 0x1FE:          # the unselected face protects every pixel it owns
                own0 = maps[1] == 1
                assert own0.any() and np.array_equal(out[own0], frame[own0])
        assert tuple(got) == want, (select, got)
    # select = all ones is select = None
    a, _ = check_one(engine, frame, kps, maps, "blur", 7, 0x3FE, 3, select=(1, 1))
    b, _ = check_one(engine, frame, kps, maps, "blur", 7, 0x3FE, 3)
    assert np.array_equal(a, b)


def test_overlap_order_and_select(emu_engine):
    check_overlap_select(emu_engine)


# ---- test 4: dead and invalid slots -----------------------------------------------------------------------------------------------

def check_dead_slots(engine):
    H, W, F, K = 120, 160, 2, 3
    kps = np.stack([np.stack([ar.make_landmarks(50 + 25 * k, 60, 22, 10 * k, seed=30 + 3 * f + k) for k in range(K)]) for f in range(F)])
    counts = np.array([2, 0])
    frames = random_frame(H, W, seed=44, F=F)
    for mode, strength, label_mask in (("mosaic", 16, 0x1FE), ("blur", 7, 0x3FE), ("fill", 0, 0x200)):
        got, valid = engine.redact_faces(frames, kps, counts=counts, mode=mode, labels=label_mask, strength=strength, pad=2, colour=COLOUR,
                                         out=sentinel(F, H, W, 3))
        assert np.array_equal(valid, engine.mask_faces(kps, H, W, counts=counts)[3]) and valid.tolist() == [[True, True, False], [False] * 3]
        for f in range(F):
            want, v, n = rr.frame_reference(frames[f], kps[f], counts[f], None, MODE_NO[mode], label_mask, strength, 2, COLOUR)
            assert_frames_equal(got[f], want, mode)
            assert (n > 0) == (f == 0)
        assert np.array_equal(got[1], frames[1]) and (got[0] != frames[0]).any()          # no live face: the input, not the sentinel
    # a NaN in a used landmark kills the slot, one in a pupil does not
    nan54, nan97 = kps[0, 0].copy(), kps[0, 1].copy()
    nan54[54, 0] = np.nan
    nan97[97, 1] = np.nan
    k3 = np.stack([nan54, nan97, kps[0, 2]])
    got, valid = engine.redact_faces(frames[0], k3[None], mode="mosaic", labels=0x3FE, strength=8, pad=1, out=sentinel(1, H, W, 3))
    assert valid.tolist() == [[False, True, True]] and np.array_equal(valid, engine.mask_faces(k3[None], H, W)[3])
    want, _, n = rr.frame_reference(frames[0], k3, None, None, rr.MOSAIC, 0x3FE, 8, 1)
    assert n > 0
    assert_frames_equal(got[0], want, "nan")
    # the background mask with no live face selects the whole frame
    got, _ = engine.redact_faces(frames[1], kps[1][None], counts=[0], mode="fill", labels=0x001, colour=COLOUR, out=sentinel(1, H, W, 3))
    assert (got[0] == (0x2C, 0x1B, 0x0A)).all()


def test_dead_slots(emu_engine):
    check_dead_slots(emu_engine)


# ---- test 5: device outputs through unaligned pointers; repeatability ----------------------------------------------------------------

def raw_redact(engine, frames_ptr, F, H, W, kps, counts, select, K, mode, label_mask, strength, pad, colour, out_ptr, valid_ptr, frames_mem,
               out_mem):
    """frames / out / valid as integer pointers (0 = NULL); landmarks, counts and select from host memory."""
    p = lambda v: C.c_void_p(v) if v else None
    rc = engine.lib.pf_redact_faces(engine.h, p(frames_ptr), frames_mem, F, H, W, _native._ptr(kps), 1 if kps.dtype == np.float64 else 0,
                                    _native.PF_MEM_HOST, _native._ptr(counts), _native._ptr(select), K, mode, label_mask, strength, pad,
                                    C.c_uint(colour), p(out_ptr), p(valid_ptr), out_mem)
    engine._check(rc, "pf_redact_faces")


def _scene_3x4(H, W):
    F, K = 3, 4
    kps = np.stack([np.stack([ar.make_landmarks(30 + 35 * k, 50 + 12 * f, 18 + 4 * k, 40 * k - 70 + 7 * f, seed=190 + 4 * f + k)
                              for k in range(K)]) for f in range(F)]).astype(np.float32)
    return kps, np.array([4, 2, 0], np.int32), random_frame(H, W, seed=55, F=F)


def check_device_outputs(engine, dev_bytes, sync):
    """dev_bytes(array or (n, fill)) -> (device pointer, read() -> uint8 [n]).  The frame base is offset by 0 .. 3 bytes, out by 0 and
    1, W * 3 is odd, so no row of either is word-aligned alike: every copy, staging and store path gives the same bytes, and the
    guard bytes around out stay."""
    H, W = 60, 161
    kps, counts, frames = _scene_3x4(H, W)
    F, K = kps.shape[:2]
    nb = F * H * W * 3
    select = np.array([[1, 0, 1, 1]] * F, np.int32)
    for mode, strength, label_mask in ((rr.MOSAIC, 8, 0x1FE), (rr.BLUR, 9, 0x3FE), (rr.FILL, 0, 0x200)):
        want = np.stack([rr.frame_reference(frames[f], kps[f], counts[f], select[f], mode, label_mask, strength, 3, COLOUR)[0] for f in range(F)])
        assert (want[:2] != frames[:2]).any() and np.array_equal(want[2], frames[2])
        for in_off, out_off in ((0, 0), (1, 1), (2, 0), (3, 1), (0, 1)):
            src = np.full((nb + 8,), 0xCD, np.uint8)
            src[in_off:in_off + nb] = frames.reshape(-1)
            d_src, _ = dev_bytes(src)
            d_out, r_out = dev_bytes((nb + 8, 0xAB))
            d_val, r_val = dev_bytes((F * K * 4, 0xAB))
            raw_redact(engine, d_src + in_off, F, H, W, kps, counts, select, K, mode, label_mask, strength, 3, COLOUR, d_out + out_off, d_val,
                       _native.PF_MEM_DEVICE, _native.PF_MEM_DEVICE)
            sync()
            o = r_out()
            assert_frames_equal(o[out_off:out_off + nb].reshape(F, H, W, 3), want, "mode %d offsets %d %d" % (mode, in_off, out_off))
            assert (o[:out_off] == 0xAB).all() and (o[out_off + nb:] == 0xAB).all()          # nothing outside out is written
            assert r_val().view(np.int32).reshape(F, K).astype(bool).tolist() == [[True] * 4, [True, True, False, False], [False] * 4]


def check_repeatability(engine):
    H, W = 60, 161
    kps, counts, frames = _scene_3x4(H, W)
    for mode, strength in (("mosaic", 4), ("blur", 32)):
        a = engine.redact_faces(frames, kps, counts=counts, mode=mode, labels=0x3FF, strength=strength, pad=5, out=sentinel(3, H, W, 3))
        b = engine.redact_faces(frames, kps, counts=counts, mode=mode, labels=0x3FF, strength=strength, pad=5, out=sentinel(3, H, W, 3))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[0] != frames).any()


def _host_bytes(spec):
    a = np.array(spec, np.uint8) if isinstance(spec, np.ndarray) else np.full((spec[0],), spec[1], np.uint8)
    return a.ctypes.data, lambda: a.copy()


def test_device_outputs_and_unaligned_pointers(emu_engine):
    check_device_outputs(emu_engine, _host_bytes, emu_engine.sync)          # the emulator's device memory is host memory


def test_repeatability(emu_engine):
    check_repeatability(emu_engine)


# ---- test 7: refusals -------------------------------------------------------------------------------------------------------------

def raw_face_redact(engine, rows, out, mode="mosaic", labels=0x1FE, strength=8, pad=0, colour=0, select=None):
    """pf_face_redact without the shape query Engine.face_redact makes first."""
    m, lm, st, pd, col = _native._redact_args(mode, labels, strength, pad, colour)
    rc = engine.lib.pf_face_redact(engine.h, rows, _native._ptr(select), m, lm, st, pd, col, _native._ptr(out), None, _native.PF_MEM_HOST)
    engine._check(rc, "pf_face_redact")


def check_rejections(engine, weights):
    H, W = 24, 40
    kps = ar.make_landmarks(20, 12, 10, 0, seed=60)[None, None]
    frame = random_frame(H, W, seed=66)
    out = sentinel(1, H, W, 3)
    ok = dict(mode="mosaic", labels=0x1FE, strength=8, pad=0)
    bad = [(dict(mode=3), "mode must be"), (dict(mode=-1), "mode must be"), (dict(labels=0), "label_mask"), (dict(labels=0x400), "label_mask"),
           (dict(labels=0x7FE), "label_mask"), (dict(strength=5), "cell size"), (dict(strength=32), "cell size"), (dict(strength=0), "cell size"),
           (dict(mode="blur", strength=0), "radius"), (dict(mode="blur", strength=33), "radius"), (dict(pad=-1), "pad"), (dict(pad=4097), "pad")]
    for change, why in bad:
        with pytest.raises(PeppaHipError, match="pf_redact_faces.*" + why):
            engine.redact_faces(frame, kps, out=out, **dict(ok, **change))
        with pytest.raises(PeppaHipError, match="pf_face_redact.*" + why):          # the arguments are judged before the record
            raw_face_redact(engine, 1, out, **dict(ok, **change))
    many = np.zeros((1, 256, 98, 2), np.float32)
    with pytest.raises(PeppaHipError, match="pf_redact_faces.*select.*top_k <= 255"):
        engine.redact_faces(frame, many, select=np.ones((1, 256), np.int32), out=out, **ok)
    assert np.array_equal(engine.redact_faces(frame, many, out=out.copy(), **ok)[0][0], frame)          # without select 256 slots are fine
    with pytest.raises(PeppaHipError, match="pf_redact_faces.*out must not be NULL"):
        raw_redact(engine, frame.ctypes.data, 1, H, W, kps, None, None, 1, rr.MOSAIC, 0x1FE, 8, 0, 0, 0, 0, _native.PF_MEM_HOST,
                   _native.PF_MEM_HOST)
    with pytest.raises(PeppaHipError, match="pf_redact_faces.*face slots are too many"):
        raw_redact(engine, frame.ctypes.data, 1 << 11, H, W, kps, None, None, 1 << 10, rr.MOSAIC, 0x1FE, 8, 0, 0, out.ctypes.data, 0,
                   _native.PF_MEM_HOST, _native.PF_MEM_HOST)
    with pytest.raises(PeppaHipError, match="pf_redact_faces: bad arguments"):
        raw_redact(engine, frame.ctypes.data, 1, 32769, W, kps, None, None, 1, rr.MOSAIC, 0x1FE, 8, 0, 0, out.ctypes.data, 0,
                   _native.PF_MEM_HOST, _native.PF_MEM_HOST)
    with pytest.raises(PeppaHipError, match="pf_face_redact.*out must not be NULL"):
        raw_face_redact(engine, 1, None, **ok)
    assert (out == 0xAB).all()                            # refused calls write nothing
    # the last-call refusals are those of pf_face_chips
    with pytest.raises(PeppaHipError, match="pf_face_redact.*left no face rows"):          # fresh handle: no pipeline call yet
        engine.face_redact(1, **ok)
    _load_small_student(engine, weights, 2)
    engine.landmark_forward(np.zeros((1, 64, 64, 3), np.uint8))
    with pytest.raises(PeppaHipError, match="pf_face_redact.*pf_landmark_forward.*no frame"):
        engine.face_redact(1, **ok)
    big, boxes = synth_frame(270, 480, 2, seed=11)
    engine.landmarks(big, boxes)
    with pytest.raises(PeppaHipError, match="3 rows asked, the last call left 2"):
        engine.face_redact(3, **ok)
    with pytest.raises(PeppaHipError, match="pf_face_redact: 3 rows asked, the last call left 2"):
        raw_face_redact(engine, 3, out, **ok)
    raw_face_redact(engine, 0, out, **ok)                 # rows == 0 succeeds and writes nothing
    assert (out == 0xAB).all()
    assert engine.face_redact(2, **ok)[0].shape == (1, 270, 480, 3)
    rc = engine.lib.pf_landmarks(engine.h, _native._ptr(big), _native.PF_MEM_HOST, big.shape[0], big.shape[1], big.strides[0], None, 0,
                                 None, None, None)
    assert rc == 0
    with pytest.raises(PeppaHipError, match="left no face rows"):          # a call without boxes leaves no rows either
        engine.face_redact(1, **ok)


def test_rejections(emu_engine, student_weights):
    check_rejections(emu_engine, student_weights)


# ---- test 8: the last-call accessor (the entry points the emulator runs; the rest in the GPU file) ------------------------------------

ACCESSOR_MODES = (("mosaic", 16, 0x1FE, 0), ("blur", 8, 0x3FE, 4))


def check_accessor(engine, rows, frames, kps, counts, select=None):
    """pf_face_redact over the last call's `rows` rows == pf_redact_faces on the frames [F,H,W,3], landmarks [F,K,98,2] and counts of
    that call == the restatement.  Returns the outputs per ACCESSOR_MODES entry."""
    F, K = kps.shape[:2]
    H, W = frames.shape[1:3]
    sel = None if select is None else np.asarray(select).reshape(F, K)
    maps = [mr.frame_maps(kps[f], None if counts is None else counts[f], H, W) for f in range(F)]      # once per frame, shared by the modes
    outs = []
    for mode, strength, label_mask, pad in ACCESSOR_MODES:
        got, valid = engine.face_redact(rows, select=select, mode=mode, labels=label_mask, strength=strength, pad=pad)
        want, want_valid = engine.redact_faces(frames, kps, counts=counts, select=sel, mode=mode, labels=label_mask, strength=strength, pad=pad)
        assert_frames_equal(got, want, mode)
        assert np.array_equal(valid, want_valid.reshape(-1)[:rows])
        for f in range(F):
            ref = rr.frame_reference(frames[f], kps[f], None, None if sel is None else sel[f], MODE_NO[mode], label_mask, strength, pad, maps=maps[f])[0]
            assert_frames_equal(got[f], ref, "%s frame %d" % (mode, f))
        outs.append(got)
    return outs


def check_after_landmarks(engine, frame, boxes):
    """pf_landmarks on a resident frame with one rejected box: the rejected row is dead, select speaks of the call's rows."""
    bad = np.array([[10.0, 10.0, 25.0, 60.0]], np.float32)
    b = np.concatenate([boxes[:1], bad, boxes[1:]], 0)
    engine.set_frame(frame)
    kps, _, valid = engine.landmarks(None, b)
    assert valid.tolist() == [True, False] + [True] * (len(boxes) - 1)
    n = len(b)
    k = kps.copy()
    k[~valid] = np.nan                                  # what the dead row holds does not matter: it is dead by its flag
    outs = check_accessor(engine, n, frame[None], k[None], None)
    assert all((o[0] != frame).any() for o in outs)
    select = np.ones((n,), np.int32)
    select[0] = 0
    outs_sel = check_accessor(engine, n, frame[None], k[None], None, select=select)
    assert (outs_sel[0] != outs[0]).any()
    return outs


def check_after_run_frames(engine, frames, rows, top_k, min_face):
    counts, _, kps, _ = engine.run_frames(frames, 0.5, 0.3, min_face, top_k, planted_rows=rows)
    F = frames.shape[0]
    outs = check_accessor(engine, F * top_k, frames, kps, counts)
    assert all((outs[0][f] != frames[f]).any() == (counts[f] > 0) for f in range(F))
    return counts, kps, outs


def test_face_redact_after_landmarks_and_run_frames(emu_engine, student_weights):
    _load_small_student(emu_engine, student_weights, 8)
    boxes = synth_frame(270, 480, 2, seed=11)[1]
    frame = random_frame(270, 480, seed=12)             # the landmarks of noise are still landmarks: only the bytes matter here
    check_after_landmarks(emu_engine, frame, boxes)
    F, K = 2, 4
    frames, rows = random_frame(270, 480, seed=13, F=F), []
    for f in range(F):
        bx = synth_frame(270, 480, 4 - f, seed=20 + f, face_w=300, face_h=400)[1]
        bx[:, 2] += np.arange(len(bx)) * 6
        rows.append(plant_rows(bx, (270, 480), n_rows=1260, input_hw=(384, 640), per_box=6, seed=f))
    counts, kps, outs = check_after_run_frames(emu_engine, frames, np.stack(rows), K, 100.0)
    assert counts.tolist() == [4, 3]
    part, valid = emu_engine.face_redact(K + 2, mode="mosaic", labels=0x1FE, strength=16)      # rows that end inside the second frame
    assert part.shape[0] == 2 and np.array_equal(part[0], outs[0][0]) and valid.sum() == 6
    want = rr.frame_reference(frames[1], kps[1], 2, None, rr.MOSAIC, 0x1FE, 16)[0]
    assert_frames_equal(part[1], want, "two slots of the second frame")

"""Face overlay (pf_draw_faces / pf_face_draw, csrc/k_draw.h) on the CPU tier, through the SIMT emulator: every output byte against
the integer restatement tests/draw_ref.py -- the masks' case table under every `what`, radius, width and alpha, hand-derived pixel
counts, frames smaller than a tile, a strided frame, unaligned device pointers, priority and overlap, scores, dead and invalid slots,
the ABI's refusals and the last-call accessor after the entry points the emulator can run.  Nothing here has a tolerance.  Input
frames are uniform random bytes and every output buffer starts as 0xAB, so a byte left unwritten shows.  The same checks run on a real
MI355X from tests/test_gpu_face_draw.py, which imports the ``check_*`` functions from here."""
import ctypes as C

import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd._native import PeppaHipError
from peppa_pig_face_landmark_amd.synth import make_frame as synth_frame, plant_rows
from tests import align_ref as ar
from tests import draw_ref as dr
from tests import mask_ref as mr
from tests.test_face_masks import _load_small_student
from tests.test_face_redact import assert_frames_equal, random_frame, sentinel

WHAT_NAMES = {1: ("points",), 2: ("contours",), 4: ("box",), 3: ("points", "contours"), 5: ("points", "box"), 6: ("contours", "box"),
              7: ("points", "contours", "box")}
# (what, r, w, alpha): every non-empty what; r in {1, 2, 16}, w in {1, 2, 3, 16}, alpha in {256, 128, 1} each where it matters and
# each with every other value at least once; r = 16 and w = 16 reach across a tile row of 16 pixels
COMBOS = [(1, 1, 1, 256), (1, 2, 1, 128), (1, 16, 1, 1), (2, 2, 1, 256), (2, 2, 2, 128), (2, 2, 3, 1), (2, 2, 16, 256), (4, 2, 1, 128),
          (4, 2, 2, 256), (4, 2, 3, 256), (4, 2, 16, 1), (3, 16, 16, 256), (5, 1, 3, 128), (6, 2, 2, 1), (7, 2, 1, 256), (7, 16, 16, 128),
          (7, 1, 2, 1)]
# the restatement's covered-pixel counts per COMBOS entry: a case must not pass vacuously
COUNTS = {
    "upright_io40_odd": [309, 1130, 10845, 583, 1123, 1645, 7130, 360, 728, 1104, 6220, 10865, 1400, 1830, 1673, 13884, 1844],
    "rect_integer": [179, 535, 9306, 320, 956, 960, 5348, 324, 656, 996, 5472, 9306, 1079, 1127, 737, 9512, 1127],
    "outside": [0] * len(COMBOS),
    "huge": [12, 53, 2890, 214, 427, 645, 3438, 0, 0, 0, 0, 4862, 12, 427, 255, 4862, 430],      # its box is the frame: the outline lies outside
}
COLOURS = ((0x2C, 0x1B, 0x0A), (1, 2, 250), (9, 240, 17), (250, 251, 3))          # hi, lo, contour, box: all different in every channel
STYLE = dict(colour_hi=COLOURS[0], colour_lo=COLOURS[1], colour_contour=COLOURS[2], colour_box=COLOURS[3])


def check_one(engine, frame, kps, what, r, w, alpha, scores=None, count=None, thres=0.8, kps_dtype=np.float32):
    """One stage-level call on one frame against the restatement; returns (out, number of covered pixels)."""
    H, W = frame.shape[:2]
    want, valid, n = dr.frame_reference(frame, kps, count, scores, what, r, w, alpha, thres, COLOURS)
    got, got_valid = engine.draw_faces(frame, np.asarray(kps, kps_dtype)[None], counts=None if count is None else [count],
                                       scores=None if scores is None else np.asarray(scores, np.float32)[None], what=WHAT_NAMES[what],
                                       point_radius=r, line_width=w, alpha=alpha, score_thres=thres, out=sentinel(1, H, W, 3), **STYLE)
    tag = "what %d r %d w %d alpha %d" % (what, r, w, alpha)
    assert_frames_equal(got[0], want, tag)
    assert np.array_equal(got_valid[0], valid), tag
    if n == 0:
        assert np.array_equal(got[0], frame), tag
    return got[0], n


# ---- test 1: the restatement over the masks' case table -------------------------------------------------------------------------

def check_restatement(engine, case):
    name, H, W, faces = case
    kps = np.stack(faces)
    frame = random_frame(H, W, seed=2000 + mr.CASE_IDS.index(name))
    scores = np.random.default_rng(7).uniform(0.6, 1.0, (1, 98)).astype(np.float32)          # hi and lo points mixed
    engine.profile_enable(True)
    counts = []
    for what, r, w, alpha in COMBOS:
        out, n = check_one(engine, frame, kps, what, r, w, alpha, scores=scores)
        if n and alpha == 256:
            assert (out != frame).any()
        counts.append(n)
    log = engine.launch_log()
    engine.profile_enable(False)
    assert any("draw_kernel" in k for k in log) and any("draw_prims_kernel" in k for k in log), log
    if name in COUNTS:
        assert counts == COUNTS[name], counts
    # float64 landmarks of the same values: the same bytes
    a, _ = check_one(engine, frame, kps, 7, 2, 2, 128, scores=scores)
    b, _ = check_one(engine, frame, kps, 7, 2, 2, 128, scores=scores, kps_dtype=np.float64)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("case", mr.CASES, ids=mr.CASE_IDS)
def test_restatement(emu_engine, case):
    check_restatement(emu_engine, case)


# ---- test 2: hand-derived pins on a 64 x 64 frame ---------------------------------------------------------------------------------

def _changed(engine, frame, kps, what, r=2, w=1):
    """pixels the overlay changes on a frame whose every byte differs from every colour byte"""
    out, n = check_one(engine, frame, kps, what, r, w, 256)
    changed = (out != frame).any(2)
    assert int(changed.sum()) == n
    return changed


def check_hand_pins(engine):
    frame = np.full((64, 64, 3), 100, np.uint8)          # no colour of COLOURS has a byte 100
    at = lambda x, y: np.full((1, 98, 2), (x, y), np.float32)
    assert _changed(engine, frame, at(50, 40), 1, r=1).sum() == 5            # the centre and its four neighbours
    assert _changed(engine, frame, at(50, 40), 1, r=2).sum() == 13
    assert _changed(engine, frame, at(50.5, 40.5), 1, r=1).sum() == 4       # the four pixels around the corner
    k = at(10, 20)
    k[0, 64:68] = (30, 20)
    ch = _changed(engine, frame, k, 2, w=1)
    assert ch.sum() == 21 and ch[20, 10:31].all()                            # one row from x = 10 to x = 30
    ch = _changed(engine, frame, k, 2, w=2)
    assert ch.sum() == 65 and ch[19:22, 10:31].all() and ch[20, 9] and ch[20, 31]          # three rows and the two cap pixels
    rect = np.stack(dict((c[0], c[3]) for c in mr.CASES)["rect_integer"])
    frame2 = np.full((120, 160, 3), 100, np.uint8)
    ch = _changed(engine, frame2, rect, 4, w=2)
    assert ch.sum() == 84 * 84 - 80 * 80 == 656 and not ch[10:90, 20:100].any() and ch[8:92, 18:102].sum() == 656


def test_hand_pins(emu_engine):
    check_hand_pins(emu_engine)


# ---- test 3: small frames and borders ---------------------------------------------------------------------------------------------

def check_small_frames(engine):
    H, W = 10, 13
    kps = ar.make_landmarks(6, 5, 8, 5, seed=6)[None]
    frame = random_frame(H, W, seed=77)
    total = 0
    for what, r, w, alpha in COMBOS:
        total += check_one(engine, frame, kps, what, r, w, alpha)[1]
    assert total > 0
    _, n = check_one(engine, frame, kps, 1, 16, 1, 256)              # a radius larger than the frame: every pixel
    assert n == H * W
    frame1 = random_frame(1, 5, seed=78)                             # one row of five pixels
    for what, r, w, alpha in COMBOS:
        check_one(engine, frame1, ar.make_landmarks(2, 0, 3, 5, seed=6)[None], what, r, w, alpha)


def test_small_frames(emu_engine):
    check_small_frames(emu_engine)


def raw_draw(engine, frames_ptr, F, H, W, kps, counts, scores, K, style, out_ptr, valid_ptr, frames_mem, out_mem):
    """frames / out / valid as integer pointers (0 = NULL); landmarks, counts and scores from host memory."""
    p = lambda v: C.c_void_p(v) if v else None
    rc = engine.lib.pf_draw_faces(engine.h, p(frames_ptr), frames_mem, F, H, W, _native._ptr(kps), 1 if kps.dtype == np.float64 else 0,
                                  _native.PF_MEM_HOST, _native._ptr(counts), _native._ptr(scores), K, C.byref(style) if style is not None else None,
                                  p(out_ptr), p(valid_ptr), out_mem)
    engine._check(rc, "pf_draw_faces")


def _scene_3x4(H, W):
    F, K = 3, 4
    kps = np.stack([np.stack([ar.make_landmarks(30 + 35 * k, 30 + 6 * f, 18 + 4 * k, 40 * k - 70 + 7 * f, seed=190 + 4 * f + k)
                              for k in range(K)]) for f in range(F)]).astype(np.float32)
    scores = np.random.default_rng(5).uniform(0.5, 1.0, (F, K, 98)).astype(np.float32)
    return kps, np.array([4, 2, 0], np.int32), scores, random_frame(H, W, seed=55, F=F)


def _scene_reference(frames, kps, counts, scores, what, r, w, alpha):
    return np.stack([dr.frame_reference(frames[f], kps[f], counts[f], None if scores is None else scores[f], what, r, w, alpha, 0.8, COLOURS)[0]
                     for f in range(len(frames))])


def check_device_outputs(engine, dev_bytes, sync):
    """dev_bytes(array or (n, fill)) -> (device pointer, read() -> uint8 [n]).  Frame base and out are offset by 0 .. 3 bytes and W * 3
    is odd, so no row of either is word-aligned alike: every copy, staging and store path gives the same bytes, and the guard bytes
    around out stay."""
    H, W = 60, 161
    kps, counts, scores, frames = _scene_3x4(H, W)
    F, K = kps.shape[:2]
    nb = F * H * W * 3
    style = _native._draw_style(what=7, point_radius=2, line_width=3, alpha=128, **STYLE)
    want = _scene_reference(frames, kps, counts, scores, 7, 2, 3, 128)
    assert (want[:2] != frames[:2]).any() and np.array_equal(want[2], frames[2])
    for in_off, out_off in ((0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (2, 0), (1, 3)):
        src = np.full((nb + 8,), 0xCD, np.uint8)
        src[in_off:in_off + nb] = frames.reshape(-1)
        d_src, _ = dev_bytes(src)
        d_out, r_out = dev_bytes((nb + 8, 0xAB))
        d_val, r_val = dev_bytes((F * K * 4, 0xAB))
        raw_draw(engine, d_src + in_off, F, H, W, kps, counts, scores, K, style, d_out + out_off, d_val, _native.PF_MEM_DEVICE,
                 _native.PF_MEM_DEVICE)
        sync()
        o = r_out()
        assert_frames_equal(o[out_off:out_off + nb].reshape(F, H, W, 3), want, "offsets %d %d" % (in_off, out_off))
        assert (o[:out_off] == 0xAB).all() and (o[out_off + nb:] == 0xAB).all()          # nothing outside out is written
        assert r_val().view(np.int32).reshape(F, K).astype(bool).tolist() == [[True] * 4, [True, True, False, False], [False] * 4]


def test_device_outputs_and_unaligned_pointers(emu_engine):
    check_device_outputs(emu_engine, lambda spec: _host_bytes(spec), emu_engine.sync)          # the emulator's device memory is host memory


def _host_bytes(spec):
    a = np.array(spec, np.uint8) if isinstance(spec, np.ndarray) else np.full((spec[0],), spec[1], np.uint8)
    return a.ctypes.data, lambda: a.copy()


def check_row_stride(engine, dev_bytes, H=270, W=480):
    """pf_landmarks on a device frame whose rows are 3 W + 5 bytes apart: pf_face_draw reads the rows where they are."""
    boxes = synth_frame(H, W, 2, seed=11)[1]
    frame = random_frame(H, W, seed=14)
    stride = 3 * W + 5
    buf = np.full((H * stride,), 0xCD, np.uint8)
    buf.reshape(H, stride)[:, :3 * W] = frame.reshape(H, 3 * W)
    d_src, _ = dev_bytes(buf)
    b = np.ascontiguousarray(boxes[:, :4], np.float32)
    kps, sc, valid = np.zeros((len(b), 98, 2), np.float32), np.zeros((len(b), 98), np.float32), np.zeros((len(b),), np.int32)
    rc = engine.lib.pf_landmarks(engine.h, C.c_void_p(d_src), _native.PF_MEM_DEVICE, H, W, stride, b.ctypes.data_as(C.POINTER(C.c_float)), len(b),
                                 kps.ctypes.data_as(C.POINTER(C.c_float)), sc.ctypes.data_as(C.POINTER(C.c_float)),
                                 valid.ctypes.data_as(C.POINTER(C.c_int)))
    engine._check(rc, "pf_landmarks")
    assert valid.all()
    got, gv = engine.face_draw(len(b), scores=sc, what=7, point_radius=2, line_width=2, alpha=256, **STYLE)
    want, wv, n = dr.frame_reference(frame, kps, None, sc, 7, 2, 2, 256, 0.8, COLOURS)
    assert n > 0 and np.array_equal(gv, wv)
    assert_frames_equal(got[0], want, "strided frame")


# ---- test 4: priority and overlap -------------------------------------------------------------------------------------------------

def check_priority(engine):
    H, W = 120, 160
    kps = np.stack([ar.make_landmarks(70, 60, 40, 10, seed=30), ar.make_landmarks(85, 64, 40, -10, seed=31)])
    frame = random_frame(H, W, seed=33)
    scores = np.random.default_rng(8).uniform(0.6, 1.0, (2, 98)).astype(np.float32)
    for alpha in (256, 128):
        out, n = check_one(engine, frame, kps, 7, 3, 3, alpha, scores=scores)
        both, _ = dr.frame_cover(kps, None, scores, H, W, 7, 3, 3)
        first = dr.slot_cover(kps[0], scores[0], H, W, 7, 3, 3, 0.8)
        second = dr.slot_cover(kps[1], scores[1], H, W, 7, 3, 3, 0.8)
        fight = (first >= 0) & (second >= 0) & (first != second)
        assert fight.sum() > 100 and np.array_equal(both[fight], first[fight])          # the lowest slot wins
        # within a slot: a point over a contour over the box
        pts, con, box = (dr.slot_cover(kps[0], scores[0], H, W, b, 3, 3, 0.8) for b in (1, 2, 4))
        assert ((pts >= 0) & (con >= 0)).sum() > 100 and ((con >= 0) & (box >= 0)).sum() > 20
        assert np.array_equal(first[pts >= 0], pts[pts >= 0]) and (first[(con >= 0) & (pts < 0)] == dr.CONTOUR).all()
        assert (first[(box >= 0) & (con < 0) & (pts < 0)] == dr.BOXC).all()
    # a lo point (index 10) and a hi point (index 11) that overlap, and the other way round: the higher index wins
    k = np.full((1, 98, 2), (-500.0, -500.0), np.float32)
    k[0, 10], k[0, 11] = (40, 30), (43, 30)
    base = np.full((64, 64, 3), 100, np.uint8)
    for s10, s11, idx in ((0.1, 0.9, 0), (0.9, 0.1, 1)):
        sc = np.full((1, 98), 0.5, np.float32)
        sc[0, 10], sc[0, 11] = s10, s11
        out, n = check_one(engine, base, k, 1, 4, 1, 256, scores=sc)
        assert n > 60 and (out[30, 41] == COLOURS[idx]).all() and (out[30, 37] == COLOURS[1 - idx]).all()
    # alpha = 128 blends once, not once per covering primitive: every point of a face at one place
    k = np.full((1, 98, 2), (20.0, 20.0), np.float32)
    out, n = check_one(engine, base, k, 7, 2, 2, 128)
    c = np.array(COLOURS[0], np.int64)
    assert (out[20, 20] == (100 * 128 + c * 128 + 128) >> 8).all()


def test_priority_and_overlap(emu_engine):
    check_priority(emu_engine)


# ---- test 5: scores ---------------------------------------------------------------------------------------------------------------

def check_scores(engine):
    H, W = 64, 96
    kps = ar.make_landmarks(48, 32, 30, 0, seed=40)[None]
    frame = np.full((H, W, 3), 100, np.uint8)
    thres = np.float32(0.8)
    seen = {}
    for name, sc in (("null", None), ("above", np.full((1, 98), np.nextafter(thres, np.float32(1))), ), ("below", np.full((1, 98), 0.1)),
                     ("equal", np.full((1, 98), thres)), ("nan", np.full((1, 98), np.nan))):
        out, n = check_one(engine, frame, kps, 1, 2, 1, 256, scores=None if sc is None else sc.astype(np.float32), thres=float(thres))
        hi, lo = (out == COLOURS[0]).all(2).sum(), (out == COLOURS[1]).all(2).sum()
        assert n > 300 and hi + lo == n
        seen[name] = (int(hi > 0), int(lo > 0))
    assert seen == {"null": (1, 0), "above": (1, 0), "below": (0, 1), "equal": (0, 1), "nan": (0, 1)}


def test_scores(emu_engine):
    check_scores(emu_engine)


# ---- test 6: dead and invalid slots -----------------------------------------------------------------------------------------------

def check_dead_slots(engine):
    H, W, F, K = 120, 160, 2, 3
    kps = np.stack([np.stack([ar.make_landmarks(50 + 25 * k, 60, 22, 10 * k, seed=30 + 3 * f + k) for k in range(K)]) for f in range(F)])
    counts = np.array([2, 0])
    frames = random_frame(H, W, seed=44, F=F)
    got, valid = engine.draw_faces(frames, kps, counts=counts, what=7, point_radius=2, line_width=2, out=sentinel(F, H, W, 3), **STYLE)
    assert np.array_equal(valid, engine.mask_faces(kps, H, W, counts=counts)[3]) and valid.tolist() == [[True, True, False], [False] * 3]
    for f in range(F):
        want, v, n = dr.frame_reference(frames[f], kps[f], counts[f], None, 7, 2, 2, 256, 0.8, COLOURS)
        assert_frames_equal(got[f], want, "frame %d" % f)
        assert (n > 0) == (f == 0)
    assert np.array_equal(got[1], frames[1]) and (got[0] != frames[0]).any()          # no live face: the input, not the sentinel
    # a NaN in a used landmark kills the slot; a NaN pupil alone does not, and that pupil is not drawn
    nan54, moved = kps[0, 0].copy(), kps[0, 1].copy()
    moved[97] = (150, 10)                                 # a pupil away from every other point, so that its disc counts
    nan97 = moved.copy()
    nan54[54, 0] = np.nan
    nan97[97, 1] = np.nan
    k3 = np.stack([nan54, nan97, kps[0, 2]])
    got, valid = engine.draw_faces(frames[0], k3[None], what=("points",), point_radius=3, out=sentinel(1, H, W, 3), **STYLE)
    assert valid.tolist() == [[False, True, True]] and np.array_equal(valid, engine.mask_faces(k3[None], H, W)[3])
    want, _, n = dr.frame_reference(frames[0], k3, None, None, 1, 3, 1, 256, 0.8, COLOURS)
    assert n > 0
    assert_frames_equal(got[0], want, "nan")
    whole, _, n_whole = dr.frame_reference(frames[0], np.stack([nan54, moved, kps[0, 2]]), None, None, 1, 3, 1, 256, 0.8, COLOURS)
    assert n_whole == n + 29                              # the pupil's disc of radius 3 is what is missing


def test_dead_slots(emu_engine):
    check_dead_slots(emu_engine)


# ---- test 7: refusals -------------------------------------------------------------------------------------------------------------

def raw_face_draw(engine, rows, out, style, scores=None, base=0):
    """pf_face_draw without the shape query Engine.face_draw makes first."""
    rc = engine.lib.pf_face_draw(engine.h, rows, _native._ptr(scores), C.byref(style) if style is not None else None,
                                 C.c_void_p(base) if base else None, _native._ptr(out), None, _native.PF_MEM_HOST)
    engine._check(rc, "pf_face_draw")


def check_rejections(engine, weights):
    H, W = 24, 40
    kps = ar.make_landmarks(20, 12, 10, 0, seed=60)[None, None]
    frame = random_frame(H, W, seed=66)
    out = sentinel(1, H, W, 3)
    ok = dict(what=7, point_radius=2, line_width=1, alpha=256)
    bad = [(dict(what=0), "what must"), (dict(what=8), "what must"), (dict(what=15), "what must"), (dict(point_radius=0), "point_radius"),
           (dict(point_radius=17), "point_radius"), (dict(line_width=0), "line_width"), (dict(line_width=17), "line_width"),
           (dict(alpha=0), "alpha"), (dict(alpha=257), "alpha")]
    for change, why in bad:
        with pytest.raises(PeppaHipError, match="pf_draw_faces.*" + why):
            engine.draw_faces(frame, kps, out=out, **dict(ok, **change))
        with pytest.raises(PeppaHipError, match="pf_face_draw.*" + why):          # the arguments are judged before the record
            raw_face_draw(engine, 1, out, _native._draw_style(**dict(ok, **change)))
    style = _native._draw_style(**ok)
    with pytest.raises(PeppaHipError, match="pf_draw_faces.*style must not be NULL"):
        raw_draw(engine, frame.ctypes.data, 1, H, W, kps, None, None, 1, None, out.ctypes.data, 0, _native.PF_MEM_HOST, _native.PF_MEM_HOST)
    with pytest.raises(PeppaHipError, match="pf_face_draw.*style must not be NULL"):
        raw_face_draw(engine, 1, out, None)
    with pytest.raises(PeppaHipError, match="pf_draw_faces.*out must not be NULL"):
        raw_draw(engine, frame.ctypes.data, 1, H, W, kps, None, None, 1, style, 0, 0, _native.PF_MEM_HOST, _native.PF_MEM_HOST)
    with pytest.raises(PeppaHipError, match="pf_face_draw.*out must not be NULL"):
        raw_face_draw(engine, 1, None, style)
    with pytest.raises(PeppaHipError, match="pf_draw_faces.*face slots are too many"):          # the size limits of pf_mask_faces
        raw_draw(engine, frame.ctypes.data, 1 << 11, H, W, kps, None, None, 1 << 10, style, out.ctypes.data, 0, _native.PF_MEM_HOST,
                 _native.PF_MEM_HOST)
    with pytest.raises(PeppaHipError, match="pf_draw_faces: bad arguments"):
        raw_draw(engine, frame.ctypes.data, 1, 32769, W, kps, None, None, 1, style, out.ctypes.data, 0, _native.PF_MEM_HOST, _native.PF_MEM_HOST)
    assert (out == 0xAB).all()                            # refused calls write nothing
    # the last-call refusals are those of pf_face_redact
    with pytest.raises(PeppaHipError, match="pf_face_draw.*left no face rows"):          # fresh handle: no pipeline call yet
        raw_face_draw(engine, 1, out, style)
    _load_small_student(engine, weights, 2)
    engine.landmark_forward(np.zeros((1, 64, 64, 3), np.uint8))
    with pytest.raises(PeppaHipError, match="pf_face_draw.*pf_landmark_forward.*no frame"):
        raw_face_draw(engine, 1, out, style)
    big, boxes = synth_frame(270, 480, 2, seed=11)
    engine.landmarks(big, boxes)
    with pytest.raises(PeppaHipError, match="3 rows asked, the last call left 2"):
        engine.face_draw(3, **ok)
    with pytest.raises(PeppaHipError, match="pf_face_draw: 3 rows asked, the last call left 2"):
        raw_face_draw(engine, 3, out, style)
    raw_face_draw(engine, 0, out, style)                  # rows == 0 succeeds and writes nothing
    assert (out == 0xAB).all()
    assert engine.face_draw(2, **ok)[0].shape == (1, 270, 480, 3)


def test_rejections(emu_engine, student_weights):
    check_rejections(emu_engine, student_weights)


# ---- test 8: repeatability --------------------------------------------------------------------------------------------------------

def check_repeatability(engine):
    H, W = 60, 161
    kps, counts, scores, frames = _scene_3x4(H, W)
    kw = dict(counts=counts, scores=scores, what=7, point_radius=3, line_width=2, alpha=77, **STYLE)
    a = engine.draw_faces(frames, kps, out=sentinel(3, H, W, 3), **kw)
    b = engine.draw_faces(frames, kps, out=sentinel(3, H, W, 3), **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[0] != frames).any()


def test_repeatability(emu_engine):
    check_repeatability(emu_engine)


# ---- test 9 (the entry points the emulator runs; the rest in the GPU file): the last-call accessor ------------------------------------

ACCESSOR_STYLES = (dict(what=1, point_radius=2, line_width=1, alpha=256), dict(what=7, point_radius=3, line_width=2, alpha=128))


def check_accessor(engine, rows, frames, kps, counts, scores):
    """pf_face_draw over the last call's `rows` rows == pf_draw_faces on the frames [F,H,W,3], landmarks [F,K,98,2], counts and scores
    [F,K,98] of that call == the restatement.  Returns the outputs per ACCESSOR_STYLES entry."""
    F, K = kps.shape[:2]
    outs = []
    for st in ACCESSOR_STYLES:
        got, valid = engine.face_draw(rows, scores=None if scores is None else scores.reshape(-1, 98)[:rows], **st, **STYLE)
        want, want_valid = engine.draw_faces(frames, kps, counts=counts, scores=scores, **st, **STYLE)
        assert_frames_equal(got, want, str(st))
        assert np.array_equal(valid, want_valid.reshape(-1)[:rows])
        ref = _scene_reference(frames, kps, [None] * F if counts is None else counts, scores, st["what"], st["point_radius"], st["line_width"],
                               st["alpha"])
        assert_frames_equal(got, ref, "restatement " + str(st))
        outs.append(got)
    return outs


def check_after_landmarks(engine, frame, boxes):
    """pf_landmarks on a resident frame with one rejected box: the rejected row is dead."""
    bad = np.array([[10.0, 10.0, 25.0, 60.0]], np.float32)
    b = np.concatenate([boxes[:1], bad, boxes[1:]], 0)
    engine.set_frame(frame)
    kps, scores, valid = engine.landmarks(None, b)
    assert valid.tolist() == [True, False] + [True] * (len(boxes) - 1)
    k = kps.copy()
    k[~valid] = np.nan                                  # what the dead row holds does not matter: it is dead by its flag
    outs = check_accessor(engine, len(b), frame[None], k[None], None, scores[None])
    assert all((o[0] != frame).any() for o in outs)
    return outs


def check_after_run_frames(engine, frames, rows, top_k, min_face):
    counts, _, kps, scores = engine.run_frames(frames, 0.5, 0.3, min_face, top_k, planted_rows=rows)
    F = frames.shape[0]
    outs = check_accessor(engine, F * top_k, frames, kps, counts, scores)
    assert all((outs[0][f] != frames[f]).any() == (counts[f] > 0) for f in range(F))
    return counts, kps, scores, outs


def test_face_draw_after_landmarks_and_run_frames(emu_engine, student_weights):
    _load_small_student(emu_engine, student_weights, 8)
    boxes = synth_frame(270, 480, 2, seed=11)[1]
    frame = random_frame(270, 480, seed=12)             # the landmarks of noise are still landmarks: only the bytes matter here
    check_after_landmarks(emu_engine, frame, boxes)
    check_row_stride(emu_engine, _host_bytes)
    F, K = 2, 4
    frames, rows = random_frame(270, 480, seed=13, F=F), []
    for f in range(F):
        bx = synth_frame(270, 480, 4 - f, seed=20 + f, face_w=300, face_h=400)[1]
        bx[:, 2] += np.arange(len(bx)) * 6
        rows.append(plant_rows(bx, (270, 480), n_rows=1260, input_hw=(384, 640), per_box=6, seed=f))
    counts, kps, scores, outs = check_after_run_frames(emu_engine, frames, np.stack(rows), K, 100.0)
    assert counts.tolist() == [4, 3]
    # base given: the frames to draw on come from elsewhere (the emulator's device memory is host memory)
    other = random_frame(270, 480, seed=17, F=F)
    got, _ = emu_engine.face_draw(F * K, scores=scores.reshape(-1, 98), base=other.ctypes.data, **ACCESSOR_STYLES[1], **STYLE)
    assert_frames_equal(got, _scene_reference(other, kps, counts, scores, 7, 3, 2, 128), "base")
    part, valid = emu_engine.face_draw(K + 2, **ACCESSOR_STYLES[0], **STYLE)      # rows that end inside the second frame, no scores
    assert part.shape[0] == 2 and valid.sum() == 6
    assert_frames_equal(part[1], dr.frame_reference(frames[1], kps[1], 2, None, 1, 2, 1, 256, 0.8, COLOURS)[0], "two slots of the second frame")

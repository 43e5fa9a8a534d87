"""Per-face region statistics (pf_measure_faces / pf_face_stats, csrc/k_stats.h) on the CPU tier, through the SIMT emulator: all 72
values of every slot against the integer restatement tests/stats_ref.py -- the masks' case table under two pairs of thresholds, closed
forms on a constant frame and a checkerboard, frames smaller than a tile, a band and a wave row, overlapping faces, dead and invalid
slots, device outputs through offset pointers, the ABI's refusals and the last-call accessor after the entry points the emulator can
run.  Nothing here has a tolerance: every comparison is array_equal on integers.  Input frames are uniform random bytes unless stated
and every output buffer starts as 0xAB bytes, so a row left unwritten or wrongly written shows.  The same checks run on a real MI355X
from tests/test_gpu_face_stats.py, which imports the ``check_*`` functions from here."""
import ctypes as C

import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd._native import PeppaHipError
from peppa_pig_face_landmark_amd.synth import make_frame as synth_frame, plant_rows
from tests import align_ref as ar
from tests import mask_ref as mr
from tests import stats_ref as sr
from tests.test_align_faces import emu_tool_library  # noqa: F401  (a fixture: the emulator build of the tool flavour)
from tests.test_face_masks import _load_small_student
from tests.test_face_redact import random_frame

THRESHOLDS = [(16, 240), (64, 192)]
SENTINEL = np.uint64(0xABABABABABABABAB)
# the restatement's pixel counts per label 0..8 (tests/mask_ref.py on the case's landmarks): a case must not pass vacuously
COUNTS = {
    "upright_io40_odd": [13705, 5123, 18, 22, 69, 84, 168, 228, 64],
    "huge": [0, 5808, 0, 0, 0, 0, 13392, 0, 0],
    "outside": [19200, 0, 0, 0, 0, 0, 0, 0, 0],
    "rect_integer": [12800, 6400, 0, 0, 0, 0, 0, 0, 0],
}


def sentinel(*shape):
    return np.full(shape, SENTINEL, np.uint64)


def assert_stats_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d values differ, first at %s: got %d, want %d" % (
        what, int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad)), int(got[bad][0]), int(want[bad][0]))


def check_one(engine, frame, kps, maps, dark, bright, count=None, kps_dtype=np.float32):
    """One stage-level call on one frame against the restatement; returns stats [K,8,9]."""
    K = len(kps)
    want = sr.frame_stats(frame, maps, dark, bright)
    got, got_valid = engine.measure_faces(frame, np.asarray(kps, kps_dtype)[None], counts=None if count is None else [count], dark=dark,
                                          bright=bright, out=sentinel(1, K, 8, 9))
    assert np.array_equal(got_valid[0], maps[3])
    want[~maps[3]] = SENTINEL                             # rows of invalid slots are left untouched
    assert_stats_equal(got[0], want, "dark %d bright %d" % (dark, bright))
    return got[0]


# ---- test 1: the restatement over the masks' case table -------------------------------------------------------------------------

def check_restatement(engine, case):
    name, H, W, faces = case
    kps = np.stack(faces)
    maps = mr.case_reference(case)
    per_label = np.bincount(maps[0].reshape(-1), minlength=9)
    if name in COUNTS:
        assert per_label.tolist() == COUNTS[name], per_label.tolist()
    if name == "scattered":
        assert per_label[1:].min() >= 399, per_label.tolist()
    frame = random_frame(H, W, seed=2000 + mr.CASE_IDS.index(name))
    engine.profile_enable(True)
    for dark, bright in THRESHOLDS:
        got = check_one(engine, frame, kps, maps, dark, bright)
        assert got[:, :, 0].sum(0).tolist() == per_label[1:].tolist(), (name, dark, bright)
        if (dark, bright) == (64, 192) and per_label[1:].sum() >= 1000:      # about a quarter of uniform bytes' lumas lie in each tail
            assert got[:, :, 7].sum() > 0 and got[:, :, 8].sum() > 0, name
    log = engine.launch_log()
    engine.profile_enable(False)
    assert any("face_stats_kernel" in k for k in log) and any("mask_fill_kernel" in k for k in log), log
    # float64 landmarks of the same values: the same values
    a = check_one(engine, frame, kps, maps, 16, 240)
    b = check_one(engine, frame, kps, maps, 16, 240, kps_dtype=np.float64)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("case", mr.CASES, ids=mr.CASE_IDS)
def test_restatement(emu_engine, case):
    check_restatement(emu_engine, case)


# ---- test 2: closed forms ---------------------------------------------------------------------------------------------------------

def _case(name):
    return mr.CASES[mr.CASE_IDS.index(name)]


def check_closed_forms(engine):
    """A constant frame (10, 20, 30): no Laplacian, every sum is n times the pixel's value; its luma by the specification's formula
    is 5728 >> 8 = 22 (the feature request's text says 24, which no ordering of the three weights gives: 22 is asserted).  Then the
    0 / 255 checkerboard, whose sum of Lap^2 has a closed form above 2^32."""
    for name in ("upright_io40_odd", "huge"):
        case = _case(name)
        _, H, W, faces = case
        maps = mr.case_reference(case)
        frame = np.empty((H, W, 3), np.uint8)
        frame[:] = (10, 20, 30)
        got = check_one(engine, frame, np.stack(faces), maps, 16, 240)[0]
        n = got[:, 0].astype(np.int64)
        assert n.sum() == int((maps[0] != 0).sum()) > 0
        Y0 = 22                                           # (29 * 10 + 150 * 20 + 77 * 30 + 128) >> 8 = 5728 >> 8
        assert int(sr.luma(frame)[0, 0]) == Y0 == (29 * 10 + 150 * 20 + 77 * 30 + 128) >> 8
        assert (got[:, 6] == 0).all()
        for field, per_pixel in ((1, 10), (2, 20), (3, 30), (4, Y0), (5, Y0 * Y0)):
            assert got[:, field].astype(np.int64).tolist() == (n * per_pixel).tolist(), field
        assert (got[:, 7] == 0).all() and (got[:, 8] == 0).all()
    # the checkerboard under the face that owns every pixel of 160 x 120: the total and label 6's share alone exceed 2^32
    case = _case("huge")
    _, H, W, faces = case
    maps = mr.case_reference(case)
    assert (maps[1] == 1).all()
    got = check_one(engine, sr.checkerboard(H, W), np.stack(faces), maps, 16, 240)[0]
    total = int(got[:, 6].astype(object).sum())
    assert total == 158 * 118 * 1020 ** 2 + 552 * 765 ** 2 + 4 * 510 ** 2 == 19721302200 == sr.checkerboard_lap2(H, W)
    assert total > 2 ** 32 and int(got[5, 6]) > 2 ** 32 and int(got[5, 0]) == 13392
    assert int(got[:, 7].sum()) + int(got[:, 8].sum()) == H * W          # every pixel is 0 or 255


def test_closed_forms(emu_engine):
    check_closed_forms(emu_engine)


# ---- test 3: frames smaller than a tile, a band and a wave row ----------------------------------------------------------------------

def check_small_frames(engine):
    H, W = 10, 13
    kps = ar.make_landmarks(6, 5, 600, 5, seed=6)[None]
    maps = mr.frame_maps(kps, None, H, W)
    assert maps[3].all() and maps[2][0].tolist() == [0, 0, W, H] and (maps[0] == 6).all() and maps[0].size == 130
    frame = random_frame(H, W, seed=77)
    for dark, bright in THRESHOLDS:
        got = check_one(engine, frame, kps, maps, dark, bright)
        assert int(got[0, 5, 0]) == 130 and int(got[0, :, 0].sum()) == 130
    # one row and one column: every vertical or every horizontal neighbour is a replica
    for H, W, centre in ((1, 40, (20, 0)), (40, 1, (0, 20))):
        kps = ar.make_landmarks(centre[0], centre[1], 600, 5, seed=6)[None]
        maps = mr.frame_maps(kps, None, H, W)
        assert int((maps[0] != 0).sum()) == H * W, (H, W)
        frame = random_frame(H, W, seed=78 + H)
        got = check_one(engine, frame, kps, maps, 64, 192)
        assert int(got[0, :, 0].sum()) == 40 and int(got[0, :, 6].sum()) > 0
        Y = sr.luma(frame).reshape(-1)                  # the Laplacian of a line: the replicas cancel two of the four terms
        p = np.pad(Y, 1, mode="edge")
        assert int(got[0, :, 6].sum()) == int(((2 * Y - p[:-2] - p[2:]) ** 2).sum())


def test_small_frames(emu_engine):
    check_small_frames(emu_engine)


# ---- test 4: overlap and ownership -------------------------------------------------------------------------------------------------

def check_overlap(engine):
    H, W = 120, 160
    kps = np.stack([ar.make_landmarks(70, 60, 40, 10, seed=1), ar.make_landmarks(95, 62, 40, -10, seed=2)])
    maps = mr.frame_maps(kps, None, H, W)
    owned = [int((maps[1] == k + 1).sum()) for k in range(2)]
    assert owned == [5772, 2065], owned
    b0, b1 = maps[2]
    assert b0[0] < b1[2] and b1[0] < b0[2] and b0[1] < b1[3] and b1[1] < b0[3]          # the boxes overlap
    frame = random_frame(H, W, seed=34)
    for dark, bright in THRESHOLDS:
        got = check_one(engine, frame, kps, maps, dark, bright)
        assert got[:, :, 0].sum(1).tolist() == owned
        assert int(got[:, :, 0].sum()) == int((maps[0] != 0).sum())


def test_overlap_and_ownership(emu_engine):
    check_overlap(emu_engine)


# ---- test 5: dead and invalid slots -----------------------------------------------------------------------------------------------

def check_dead_slots(engine):
    H, W, F, K = 120, 160, 2, 3
    kps = np.stack([np.stack([ar.make_landmarks(50 + 25 * k, 60, 22, 10 * k, seed=30 + 3 * f + k) for k in range(K)]) for f in range(F)])
    counts = np.array([2, 0])
    frames = random_frame(H, W, seed=44, F=F)
    got, valid = engine.measure_faces(frames, kps, counts=counts, out=sentinel(F, K, 8, 9))
    assert np.array_equal(valid, engine.mask_faces(kps, H, W, counts=counts)[3]) and valid.tolist() == [[True, True, False], [False] * 3]
    for f in range(F):
        want, v = sr.frame_reference(frames[f], kps[f], counts[f])
        assert_stats_equal(got[f][v], want[v], "frame %d" % f)
    assert (got[~valid] == SENTINEL).all() and int(got[0, :2, :, 0].sum()) > 0
    # a NaN in a used landmark kills the slot, one in a pupil does not; a valid slot outside the frame measures nothing
    nan54, nan97 = kps[0, 0].copy(), kps[0, 1].copy()
    nan54[54, 0] = np.nan
    nan97[97, 1] = np.nan
    k4 = np.stack([nan54, nan97, kps[0, 2], ar.make_landmarks(-400, 60, 40, 0, seed=5)])
    got, valid = engine.measure_faces(frames[0], k4[None], dark=64, bright=192, out=sentinel(1, 4, 8, 9))
    assert valid.tolist() == [[False, True, True, True]] and np.array_equal(valid, engine.mask_faces(k4[None], H, W)[3])
    want, _ = sr.frame_reference(frames[0], k4, None, 64, 192)
    assert (got[0, 0] == SENTINEL).all() and (got[0, 3] == 0).all()
    assert_stats_equal(got[0, 1:], want[1:], "nan")
    assert int(got[0, 1, :, 0].sum()) > 0 and int(got[0, 2, :, 0].sum()) > 0
    got, valid = engine.measure_faces(frames[0], k4[None], counts=[1], out=sentinel(1, 4, 8, 9))
    assert not valid.any() and (got == SENTINEL).all()


def test_dead_slots(emu_engine):
    check_dead_slots(emu_engine)


# ---- tests 6 and 7: several frames, device outputs through offset pointers; repeatability ------------------------------------------

def raw_measure(engine, frames_ptr, F, H, W, kps, counts, K, dark, bright, stats_ptr, valid_ptr, frames_mem, out_mem):
    """frames / stats / valid as integer pointers (0 = NULL); landmarks and counts from host memory."""
    p = lambda v: C.c_void_p(v) if v else None
    rc = engine.lib.pf_measure_faces(engine.h, p(frames_ptr), frames_mem, F, H, W, _native._ptr(kps), 1 if kps.dtype == np.float64 else 0,
                                     _native.PF_MEM_HOST, _native._ptr(counts), K, dark, bright, p(stats_ptr), p(valid_ptr), out_mem)
    engine._check(rc, "pf_measure_faces")


def _scene_3x4(H, W):
    F, K = 3, 4
    kps = np.stack([np.stack([ar.make_landmarks(30 + 35 * k, 50 + 12 * f, 18 + 4 * k, 40 * k - 70 + 7 * f, seed=190 + 4 * f + k)
                              for k in range(K)]) for f in range(F)]).astype(np.float32)
    return kps, np.array([4, 2, 0], np.int32), random_frame(H, W, seed=56, F=F)


def _scene_reference(kps, counts, frames, dark=16, bright=240):
    want = np.stack([sr.frame_reference(frames[f], kps[f], counts[f], dark, bright)[0] for f in range(len(frames))])
    valid = np.arange(kps.shape[1])[None, :] < counts[:, None]
    want[~valid] = SENTINEL
    return want, valid


def check_device_outputs(engine, dev_bytes, sync):
    """dev_bytes(array or (n, fill)) -> (device pointer, read() -> uint8 [n]).  Three frames of different content in one call; the
    frame base is offset by 0 .. 3 bytes and W * 3 is odd, so no row is word-aligned alike; stats and valid start 8 bytes into their
    allocations, and the guard bytes around them stay."""
    H, W = 60, 161
    kps, counts, frames = _scene_3x4(H, W)
    F, K = kps.shape[:2]
    nb, ns = F * H * W * 3, F * K * 72 * 8
    want, want_valid = _scene_reference(kps, counts, frames, 64, 192)
    assert all(int(want[f, :counts[f], :, 0].astype(np.int64).sum()) > 0 for f in range(2))
    assert not np.array_equal(want[0, 0], want[1, 0])
    for in_off in (0, 1, 2, 3):
        src = np.full((nb + 8,), 0xCD, np.uint8)
        src[in_off:in_off + nb] = frames.reshape(-1)
        d_src, _ = dev_bytes(src)
        d_out, r_out = dev_bytes((ns + 16, 0xAB))
        d_val, r_val = dev_bytes((F * K * 4 + 16, 0xAB))
        raw_measure(engine, d_src + in_off, F, H, W, kps, counts, K, 64, 192, d_out + 8, d_val + 8, _native.PF_MEM_DEVICE, _native.PF_MEM_DEVICE)
        sync()
        o, v = r_out(), r_val()
        assert_stats_equal(o[8:8 + ns].view(np.uint64).reshape(F, K, 8, 9), want, "frame offset %d" % in_off)
        assert (o[:8] == 0xAB).all() and (o[8 + ns:] == 0xAB).all()          # nothing outside stats is written
        assert np.array_equal(v[8:8 + F * K * 4].view(np.int32).reshape(F, K).astype(bool), want_valid)
        assert (v[:8] == 0xAB).all() and (v[8 + F * K * 4:] == 0xAB).all()
    # the same through the host path
    got, valid = engine.measure_faces(frames, kps, counts=counts, dark=64, bright=192, out=sentinel(F, K, 8, 9))
    assert_stats_equal(got, want, "host")
    assert np.array_equal(valid, want_valid)


def check_repeatability(engine):
    H, W = 60, 161
    kps, counts, frames = _scene_3x4(H, W)
    a = engine.measure_faces(frames, kps, counts=counts, out=sentinel(3, 4, 8, 9))
    b = engine.measure_faces(frames, kps, counts=counts, out=sentinel(3, 4, 8, 9))
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[1].any()


def _host_bytes(spec):
    a = np.array(spec, np.uint8) if isinstance(spec, np.ndarray) else np.full((spec[0],), spec[1], np.uint8)
    return a.ctypes.data, lambda: a.copy()


def test_device_outputs_and_offset_pointers(emu_engine):
    check_device_outputs(emu_engine, _host_bytes, emu_engine.sync)          # the emulator's device memory is host memory


def test_repeatability(emu_engine):
    check_repeatability(emu_engine)


# ---- the form that does not ship: the tool build's staged kernel gives the same values ------------------------------------------------

def test_staged_form_of_the_tool_build(emu_tool_library, monkeypatch):
    """face_stats_staged_kernel (LDS-staged pieces, packed 32-bit registers, shuffle reduction) is reachable in the tool flavour only,
    through PEPPA_STATS_STAGED, which is read when a handle is created.  The case table, the closed forms (the checkerboard's sum
    above 2^32 crosses its 32-bit registers), small frames, overlap and dead slots hold for it as they do for the kernel that ships."""
    from peppa_pig_face_landmark_amd._native import Engine
    monkeypatch.setenv("PEPPA_STATS_STAGED", "1")
    eng = Engine(0, emu_tool_library)
    try:
        eng.profile_enable(True)
        for case in mr.CASES:
            name, H, W, faces = case
            frame = random_frame(H, W, seed=2000 + mr.CASE_IDS.index(name))
            check_one(eng, frame, np.stack(faces), mr.case_reference(case), 64, 192)
        log = eng.launch_log()
        eng.profile_enable(False)
        assert any("face_stats_staged_kernel" in k for k in log) and not any("face_stats_kernel" in k for k in log), log
        check_closed_forms(eng)
        check_small_frames(eng)
        check_overlap(eng)
        check_dead_slots(eng)
        check_device_outputs(eng, _host_bytes, eng.sync)
    finally:
        eng.close()


# ---- test 8: refusals -------------------------------------------------------------------------------------------------------------

def raw_face_stats(engine, rows, out, dark=16, bright=240, out_mem=_native.PF_MEM_HOST):
    rc = engine.lib.pf_face_stats(engine.h, rows, dark, bright, _native._ptr(out), None, out_mem)
    engine._check(rc, "pf_face_stats")


def check_rejections(engine, weights):
    H, W = 24, 40
    kps = ar.make_landmarks(20, 12, 10, 0, seed=60)[None, None]
    frame = random_frame(H, W, seed=66)
    out = sentinel(1, 1, 8, 9)
    for dark, bright in ((-1, 240), (16, 256), (100, 100), (200, 100)):
        with pytest.raises(PeppaHipError, match="pf_measure_faces.*0 <= dark < bright <= 255"):
            engine.measure_faces(frame, kps, dark=dark, bright=bright, out=out)
        with pytest.raises(PeppaHipError, match="pf_face_stats.*0 <= dark < bright <= 255"):      # the arguments are judged before the record
            raw_face_stats(engine, 1, out, dark, bright)
    engine.measure_faces(frame, kps, dark=0, bright=255, out=out.copy())          # the widest pair is fine
    many = np.zeros((1, 256, 98, 2), np.float32)
    with pytest.raises(PeppaHipError, match="pf_measure_faces.*owners are bytes.*top_k <= 255.*got 256"):
        engine.measure_faces(frame, many)
    with pytest.raises(PeppaHipError, match="pf_measure_faces.*stats must not be NULL"):
        raw_measure(engine, frame.ctypes.data, 1, H, W, kps, None, 1, 16, 240, 0, 0, _native.PF_MEM_HOST, _native.PF_MEM_HOST)
    with pytest.raises(PeppaHipError, match="pf_face_stats.*stats must not be NULL"):
        raw_face_stats(engine, 1, None)
    for who, call in (("pf_measure_faces", lambda m: raw_measure(engine, frame.ctypes.data, 1, H, W, kps, None, 1, 16, 240, out.ctypes.data, 0,
                                                                  _native.PF_MEM_HOST, m)),
                      ("pf_face_stats", lambda m: raw_face_stats(engine, 1, out, out_mem=m))):
        with pytest.raises(PeppaHipError, match=who + ".*bad out_mem 7"):
            call(7)
    with pytest.raises(PeppaHipError, match="pf_measure_faces.*face slots are too many"):
        raw_measure(engine, frame.ctypes.data, 1 << 13, H, W, kps, None, 255, 16, 240, out.ctypes.data, 0, _native.PF_MEM_HOST, _native.PF_MEM_HOST)
    with pytest.raises(PeppaHipError, match="pf_measure_faces: bad arguments"):
        raw_measure(engine, frame.ctypes.data, 1, 32769, W, kps, None, 1, 16, 240, out.ctypes.data, 0, _native.PF_MEM_HOST, _native.PF_MEM_HOST)
    assert (out == SENTINEL).all()                        # refused calls write nothing
    # the last-call refusals are those of pf_face_redact
    with pytest.raises(PeppaHipError, match="pf_face_stats.*left no face rows"):          # fresh handle: no pipeline call yet
        engine.face_stats(1)
    _load_small_student(engine, weights, 2)
    engine.landmark_forward(np.zeros((1, 64, 64, 3), np.uint8))
    with pytest.raises(PeppaHipError, match="pf_face_stats.*pf_landmark_forward.*no frame"):
        engine.face_stats(1)
    big, boxes = synth_frame(270, 480, 2, seed=11)
    engine.landmarks(big, boxes)
    with pytest.raises(PeppaHipError, match="pf_face_stats: 3 rows asked, the last call left 2"):
        engine.face_stats(3)
    raw_face_stats(engine, 0, out)                        # rows == 0 succeeds and writes nothing
    assert (out == SENTINEL).all()
    stats, valid = engine.face_stats(2)
    assert stats.shape == (2, 8, 9) and valid.all()
    assert engine.face_stats(2)[0].tobytes() == stats.tobytes()          # the record of the last call is left alone
    engine.set_frame(big)
    with pytest.raises(PeppaHipError, match="pf_face_stats.*left no face rows"):          # pf_set_frame drops the record
        engine.face_stats(1)


def test_rejections(emu_engine, student_weights):
    check_rejections(emu_engine, student_weights)


# ---- test 9: the last-call accessor (the entry points the emulator runs; the rest in the GPU file) ------------------------------------

def check_accessor(engine, rows, frames, kps, counts, thresholds=((16, 240), (64, 192))):
    """pf_face_stats over the last call's `rows` rows == pf_measure_faces on the frames [F,H,W,3], landmarks [F,K,98,2] and counts of
    that call == the restatement.  Returns the stats [rows,8,9] of the first pair of thresholds."""
    F, K = kps.shape[:2]
    H, W = frames.shape[1:3]
    maps = [mr.frame_maps(kps[f], None if counts is None else counts[f], H, W) for f in range(F)]      # once per frame, shared by the pairs
    first = None
    for dark, bright in thresholds:
        got, valid = engine.face_stats(rows, dark=dark, bright=bright)
        want, want_valid = engine.measure_faces(frames, kps, counts=counts, dark=dark, bright=bright)
        want, want_valid = want.reshape(F * K, 8, 9)[:rows], want_valid.reshape(-1)[:rows]
        assert np.array_equal(valid, want_valid)
        assert_stats_equal(got[valid], want[valid], "accessor against the stage")
        assert (got[~valid] == 0).all()                   # untouched: the zeros the wrapper allocated
        ref = np.concatenate([sr.frame_stats(frames[f], maps[f], dark, bright) for f in range(F)])[:rows]
        assert np.array_equal(valid, np.concatenate([m[3] for m in maps])[:rows])
        assert_stats_equal(got[valid], ref[valid], "accessor against the restatement")
        first = got if first is None else first
    return first


def check_after_landmarks(engine, frame, boxes):
    """pf_landmarks on a resident frame with one rejected box: the rejected row is dead."""
    bad = np.array([[10.0, 10.0, 25.0, 60.0]], np.float32)
    b = np.concatenate([boxes[:1], bad, boxes[1:]], 0)
    engine.set_frame(frame)
    kps, _, valid = engine.landmarks(None, b)
    assert valid.tolist() == [True, False] + [True] * (len(boxes) - 1)
    k = kps.copy()
    k[~valid] = np.nan                                  # what the dead row holds does not matter: it is dead by its flag
    got = check_accessor(engine, len(b), frame[None], k[None], None)
    assert int(got[:, :, 0].sum()) > 0
    return got


def check_after_run_frames(engine, frames, rows, top_k, min_face):
    counts, _, kps, _ = engine.run_frames(frames, 0.5, 0.3, min_face, top_k, planted_rows=rows)
    F = frames.shape[0]
    got = check_accessor(engine, F * top_k, frames, kps, counts)
    per_frame = got.reshape(F, top_k, 8, 9)[:, :, :, 0].sum((1, 2))
    assert all((per_frame[f] > 0) == (counts[f] > 0) for f in range(F))
    return counts, kps, got


def test_face_stats_after_landmarks_and_run_frames(emu_engine, student_weights):
    _load_small_student(emu_engine, student_weights, 8)
    boxes = synth_frame(270, 480, 2, seed=11)[1]
    frame = random_frame(270, 480, seed=12)             # the landmarks of noise are still landmarks: only the values matter here
    check_after_landmarks(emu_engine, frame, boxes)
    F, K = 2, 4
    frames, rows = random_frame(270, 480, seed=13, F=F), []
    for f in range(F):
        bx = synth_frame(270, 480, 4 - f, seed=20 + f, face_w=300, face_h=400)[1]
        bx[:, 2] += np.arange(len(bx)) * 6
        rows.append(plant_rows(bx, (270, 480), n_rows=1260, input_hw=(384, 640), per_box=6, seed=f))
    counts, kps, got = check_after_run_frames(emu_engine, frames, np.stack(rows), K, 100.0)
    assert counts.tolist() == [4, 3]
    part, valid = emu_engine.face_stats(K + 2)          # rows that end inside the second frame
    assert part.shape == (K + 2, 8, 9) and valid.sum() == 6
    want = sr.frame_reference(frames[1], kps[1], 2)[0]
    assert_stats_equal(part[:K], got[:K], "the first frame")
    assert_stats_equal(part[K:], want[:2], "two slots of the second frame")

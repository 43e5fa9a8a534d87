"""Face-region label maps (pf_mask_faces / pf_face_masks, csrc/k_mask.h) on the CPU tier, through the SIMT emulator: every byte of
labels, owners, boxes and valid against the integer restatement tests/mask_ref.py -- the case table, overlap and slot order, dead and
invalid slots, chip space against the chips' own matrices, device outputs through unaligned pointers, the ABI's refusals and the
last-call accessor after the entry points the emulator can run.  Nothing here has a tolerance.  The same checks run on a real MI355X
from tests/test_gpu_face_masks.py, which imports the ``check_*`` functions from here."""
import ctypes as C

import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd._native import PeppaHipError
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.synth import make_frame as synth_frame, plant_rows
from tests import align_ref as ar
from tests import mask_ref as mr


def assert_maps_equal(got, want):
    """(labels, owners, boxes, valid) twice: every array equal (None == None)."""
    for name, g, w in zip(("labels", "owners", "boxes", "valid"), got, want):
        assert (g is None) == (w is None), name
        if g is not None:
            g, w = np.asarray(g), np.asarray(w)
            assert g.size == w.size and np.array_equal(g.reshape(w.shape), w), "%s: %d values differ" % (name, int((g.reshape(w.shape) != w).sum()))


# ---- test 1: the restatement, frame space ---------------------------------------------------------------------------------------

def check_restatement(engine, case):
    name, H, W, faces = case
    kps = np.stack(faces)[None]
    engine.profile_enable(True)
    got = engine.mask_faces(kps, H, W)
    log = engine.launch_log()
    engine.profile_enable(False)
    assert any("mask_edges_kernel" in k for k in log) and any("mask_fill_kernel" in k for k in log), log
    labels, owners, boxes, valid = mr.case_reference(case)
    assert_maps_equal(got, (labels[None], owners[None], boxes[None], valid[None]))
    assert_maps_equal(engine.mask_faces(kps.astype(np.float64), H, W), got)          # same values, either type
    assert valid.all()
    lab = got[0][0]
    if name == "upright_io40_odd":
        assert [int((lab == v).sum()) for v in range(1, 9)] == [5123, 18, 22, 69, 84, 168, 228, 64]
    if name == "outside":
        assert not lab.any() and boxes[0, 0] == boxes[0, 2] == 0
    if name == "huge":
        assert lab.all()                                  # every tile is interior to some polygon
    if name == "tile_corner":
        y, x = 4 * mr.TILE_H, mr.TILE_W                   # the four tiles meeting there all hold face pixels
        assert lab[y - 1, x - 1] and lab[y - 1, x] and lab[y, x - 1] and lab[y, x]
    if name.startswith("rect_"):
        lo = 0 if name == "rect_integer" else 1
        want = np.zeros((H, W), np.uint8)
        want[10 + lo:90 + lo, 20 + lo:100 + lo] = 1
        assert int((lab == 1).sum()) == 6400 and np.array_equal(lab, want)
    if name == "scattered":
        assert all((lab == v).sum() > 100 for v in range(1, 9))


@pytest.mark.parametrize("case", mr.CASES, ids=mr.CASE_IDS)
def test_restatement(emu_engine, case):
    check_restatement(emu_engine, case)


# ---- test 2: overlap and order --------------------------------------------------------------------------------------------------

def check_overlap(engine):
    H, W = 120, 160
    kps = np.stack([ar.make_landmarks(70, 60, 40, 10, seed=30), ar.make_landmarks(100, 70, 40, -10, seed=31)])
    ref = [mr.frame_maps(k, None, H, W) for k in (kps, kps[::-1])]
    assert int((ref[0][0] != ref[1][0]).sum()) == 765                 # the slot order decides who owns the overlap
    for k, (labels, owners, boxes, valid) in zip((kps, kps[::-1]), ref):
        got = engine.mask_faces(k[None], H, W)
        assert_maps_equal(got, (labels[None], owners[None], boxes[None], valid[None]))
        assert set(np.unique(got[1])) == {0, 1, 2}
        assert np.array_equal(got[0] != 0, got[1] != 0)
        for slot in (0, 1):                                           # every non-zero pixel lies in its owner's box
            ys, xs = np.nonzero(got[1][0] == slot + 1)
            x0, y0, x1, y1 = got[2][0, slot]
            assert xs.min() >= x0 and xs.max() < x1 and ys.min() >= y0 and ys.max() < y1


def test_overlap_and_order(emu_engine):
    check_overlap(emu_engine)


# ---- test 3: dead and invalid slots ---------------------------------------------------------------------------------------------

def check_dead_slots(engine):
    H, W, F, K, S = 120, 160, 2, 3, 32
    kps = np.stack([np.stack([ar.make_landmarks(50 + 25 * k, 60, 22, 10 * k, seed=30 + 3 * f + k) for k in range(K)]) for f in range(F)])
    counts = np.array([2, 0])
    out = (np.full((F, H, W), 0xAB, np.uint8), np.full((F, H, W), 0xAB, np.uint8), np.full((F, K, 4), -7, np.int32))
    got = engine.mask_faces(kps, H, W, counts=counts, out=out)
    assert got[3].tolist() == [[True, True, False], [False, False, False]]
    for f in range(F):
        labels, owners, boxes, valid = mr.frame_maps(kps[f], counts[f], H, W, boxes_init=np.full((K, 4), -7))
        assert_maps_equal((got[0][f], got[1][f], got[2][f], got[3][f]), (labels, owners, boxes, valid))
    assert (got[2][0, 2] == -7).all() and (got[2][1] == -7).all()          # box rows of dead slots are untouched
    assert not got[0][1].any() and not got[1][1].any()                    # no live face: all zero, not the sentinel
    assert got[0][0].any()
    # a NaN in a used landmark kills the slot, one in a pupil does not
    nan54, nan97 = kps[0, 0].copy(), kps[0, 1].copy()
    nan54[54, 0] = np.nan
    nan97[97, 1] = np.nan
    k3 = np.stack([nan54, nan97, kps[0, 2]])
    out = (np.full((1, H, W), 0xAB, np.uint8), np.full((1, H, W), 0xAB, np.uint8), np.full((1, K, 4), -7, np.int32))
    got = engine.mask_faces(k3[None], H, W, out=out)
    assert got[3].tolist() == [[False, True, True]]
    labels, owners, boxes, valid = mr.frame_maps(k3, None, H, W, boxes_init=np.full((K, 4), -7))
    assert_maps_equal(got, (labels[None], owners[None], boxes[None], valid[None]))
    assert set(np.unique(got[1])) == {0, 2, 3} and (got[2][0, 0] == -7).all()
    # chip space: the map of a dead slot keeps the sentinel
    maps = np.full((F, K, S, S), 0xAB, np.uint8)
    got = engine.mask_faces(kps, counts=counts, chip_size=S, out=(maps, None, None))
    assert got[1] is None and got[2] is None and got[3].tolist() == [[True, True, False], [False, False, False]]
    assert (maps[0, 2] == 0xAB).all() and (maps[1] == 0xAB).all()
    assert not (maps[0, :2] == 0xAB).any() and maps[0, 0].any() and maps[0, 1].any()


def test_dead_slots(emu_engine):
    check_dead_slots(emu_engine)


# ---- test 4: chip space ---------------------------------------------------------------------------------------------------------

CHIP_CASES = [c for c in ar.CASES if c[0] in ("scale04_roll30", "half_outside", "chip112")]


def check_chip_space(engine, case):
    frame, kps, S = ar.case_scene(case)
    tiny = ar.make_landmarks(80, 60, 2000.0 * S / 32, 0, seed=41)           # degenerate fit: scale 0.005, below 1/64
    kps = np.concatenate([kps, tiny[None, None]], 1)
    n = kps.shape[1]
    _, mats, fit_ok = engine.align_faces(frame, kps, chip_size=S)
    maps = np.full((1, n, S, S), 0xAB, np.uint8)
    got = engine.mask_faces(kps, chip_size=S, out=(maps, None, None))
    assert np.array_equal(got[3], fit_ok) and fit_ok[0, :-1].all() and not fit_ok[0, -1]
    assert (maps[0, -1] == 0xAB).all()
    for i in range(n - 1):       # the restatement through the matrix the chips use: mask and chip line up
        assert np.array_equal(maps[0, i], mr.chip_map(kps[0, i], mats[0, i], S)), case[0]
    assert_maps_equal(engine.mask_faces(kps.astype(np.float64), chip_size=S, out=(np.full_like(maps, 0xAB), None, None)), got)
    if case[0] == "chip112":     # the template's eye positions
        assert S == 112 and maps[0, 0][52, 38] == 4 and maps[0, 0][52, 74] == 5


@pytest.mark.parametrize("case", CHIP_CASES, ids=lambda c: c[0])
def test_chip_space(emu_engine, case):
    check_chip_space(emu_engine, case)


# ---- test 5: device outputs through unaligned pointers; repeatability --------------------------------------------------------------

def raw_mask(engine, F, H, W, kps, counts, K, S, labels, owners, boxes, valid, out_mem):
    """pointers as integers (0 = NULL)."""
    p = lambda v: C.c_void_p(v) if v else None
    rc = engine.lib.pf_mask_faces(engine.h, F, H, W, _native._ptr(kps), 1 if kps.dtype == np.float64 else 0, _native.PF_MEM_HOST,
                                  _native._ptr(counts), K, S, p(labels), p(owners), p(boxes), p(valid), out_mem)
    engine._check(rc, "pf_mask_faces")


def _scene_8x8():
    F, K = 8, 8
    kps = np.stack([np.stack([ar.make_landmarks(40 + 30 * k, 60 + 15 * f, 20 + 4 * k, 40 * k - 150 + 7 * f, seed=90 + 8 * f + k)
                              for k in range(K)]) for f in range(F)])
    return kps, np.array([8, 7, 6, 5, 4, 3, 0, 8], np.int32)


def check_device_outputs(engine, dev_bytes, sync):
    """dev_bytes(n, fill) -> (device pointer, read() -> uint8 [n]): the kernels write the caller's device buffers, enqueued only;
    label and owner pointers that are not 4-byte aligned take the byte stores and give the same bytes."""
    H, W, S = 240, 320, 32
    kps, counts = _scene_8x8()
    F, K = kps.shape[:2]
    want = engine.mask_faces(kps, H, W, counts=counts)
    want_chip = engine.mask_faces(kps, counts=counts, chip_size=S)
    assert want[3].sum() == counts.sum() and len(np.unique(want[1])) == 9
    for off in (0, 1):
        d_lab, r_lab = dev_bytes(F * H * W + 4, 0xAB)
        d_own, r_own = dev_bytes(F * H * W + 4, 0xAB)
        d_box, r_box = dev_bytes(F * K * 16, 0xAB)
        d_val, r_val = dev_bytes(F * K * 4, 0xAB)
        raw_mask(engine, F, H, W, kps, counts, K, 0, d_lab + off, d_own + off, d_box, d_val, _native.PF_MEM_DEVICE)
        sync()
        lab, own = r_lab(), r_own()
        assert np.array_equal(lab[off:off + F * H * W].reshape(F, H, W), want[0]) and np.array_equal(own[off:off + F * H * W].reshape(F, H, W), want[1])
        assert (lab[:off] == 0xAB).all() and (lab[off + F * H * W:] == 0xAB).all()       # nothing outside the maps is written
        valid = r_val().view(np.int32).reshape(F, K)
        assert np.array_equal(valid != 0, want[3])
        box = r_box().view(np.int32).reshape(F, K, 4)
        assert np.array_equal(box[want[3]], want[2][want[3]]) and (box[~want[3]] == np.int32(-0x54545455)).all()
        d_map, r_map = dev_bytes(F * K * S * S + 4, 0xAB)
        raw_mask(engine, F, 0, 0, kps, counts, K, S, d_map + off, 0, 0, 0, _native.PF_MEM_DEVICE)
        sync()
        m = r_map()[off:off + F * K * S * S].reshape(F, K, S, S)
        assert np.array_equal(m[want_chip[3]], want_chip[0][want_chip[3]]) and (m[~want_chip[3]] == 0xAB).all()


def check_repeatability(engine):
    kps, counts = _scene_8x8()
    a = engine.mask_faces(kps, 240, 320, counts=counts)
    b = engine.mask_faces(kps, 240, 320, counts=counts)
    assert a[0].any()
    assert_maps_equal(a, b)
    assert_maps_equal(engine.mask_faces(kps, counts=counts, chip_size=112), engine.mask_faces(kps, counts=counts, chip_size=112))


def _host_bytes(n, fill):
    a = np.full((n,), fill, np.uint8)
    return a.ctypes.data, lambda: a.copy()


def test_device_outputs_and_unaligned_pointers(emu_engine):
    check_device_outputs(emu_engine, _host_bytes, emu_engine.sync)          # the emulator's device memory is host memory


def test_repeatability(emu_engine):
    check_repeatability(emu_engine)


# ---- test 6: refusals -----------------------------------------------------------------------------------------------------------

def raw_face_masks(engine, rows, S, labels, owners=None, boxes=None, valid=None):
    rc = engine.lib.pf_face_masks(engine.h, rows, S, _native._ptr(labels), _native._ptr(owners), _native._ptr(boxes), _native._ptr(valid),
                                  _native.PF_MEM_HOST)
    engine._check(rc, "pf_face_masks")


def _load_small_student(engine, weights, batch):
    engine.load_program(0, build_student_program(weights, 64, "f32")[0], batch)


def check_rejections(engine, weights):
    H, W = 120, 160
    kps = ar.make_landmarks(80, 60, 22, 0, seed=60)[None, None]
    tiny = np.full((64,), 0xAB, np.uint8)               # refused calls write nothing
    for S in (100, 16, 272):
        maps = np.full((1, 1, S, S), 0xAB, np.uint8)
        with pytest.raises(PeppaHipError, match="multiple of 16"):
            engine.mask_faces(kps, chip_size=S, out=(maps, None, None))
        assert (maps == 0xAB).all()
        with pytest.raises(PeppaHipError, match="multiple of 16"):
            engine.face_masks(1, S)
    many = np.zeros((1, 256, 98, 2), np.float32)
    with pytest.raises(PeppaHipError, match="top_k <= 255"):
        engine.mask_faces(many, H, W)
    assert engine.mask_faces(many, H, W, owners=False)[1] is None                 # without owners 256 slots are fine
    for out in ((np.zeros((1, 1, 32, 32), np.uint8), tiny, None), (np.zeros((1, 1, 32, 32), np.uint8), None, np.zeros((1, 1, 4), np.int32))):
        with pytest.raises(PeppaHipError, match="must be NULL in chip space"):
            engine.mask_faces(kps, chip_size=32, out=out)
    with pytest.raises(PeppaHipError, match="must be NULL in chip space"):
        raw_face_masks(engine, 1, 32, tiny, owners=tiny)
    for S in (0, 32):
        with pytest.raises(PeppaHipError, match="left no face rows"):             # fresh handle: no pipeline call yet
            raw_face_masks(engine, 1, S, tiny)
    with pytest.raises(PeppaHipError, match="pf_face_masks_shape: the handle's last call left no face rows"):
        engine.face_masks_shape(1)
    _load_small_student(engine, weights, 2)
    engine.landmark_forward(np.zeros((1, 64, 64, 3), np.uint8))
    for S in (0, 32):
        with pytest.raises(PeppaHipError, match="pf_landmark_forward.*no frame"):
            raw_face_masks(engine, 1, S, tiny)
    with pytest.raises(PeppaHipError, match="pf_face_masks_shape.*pf_landmark_forward.*no frame"):
        engine.face_masks_shape(1)
    big, boxes = synth_frame(270, 480, 2, seed=11)
    engine.landmarks(big, boxes)
    with pytest.raises(PeppaHipError, match="pf_face_masks_shape: 3 rows asked, the last call left 2"):
        engine.face_masks_shape(3)
    for S in (0, 32):
        with pytest.raises(PeppaHipError, match="3 rows asked, the last call left 2"):
            raw_face_masks(engine, 3, S, tiny)
    with pytest.raises(PeppaHipError, match="3 rows asked, the last call left 2"):
        engine.face_masks(3)
    assert (tiny == 0xAB).all()
    assert engine.face_masks_shape(2) == (1, 270, 480)
    assert engine.face_masks(2)[0].shape == (1, 270, 480) and engine.face_masks(2, 32)[0].shape == (2, 32, 32)
    # a call without boxes leaves no rows either
    rc = engine.lib.pf_landmarks(engine.h, _native._ptr(big), _native.PF_MEM_HOST, big.shape[0], big.shape[1], big.strides[0], None, 0,
                                 None, None, None)
    assert rc == 0
    with pytest.raises(PeppaHipError, match="left no face rows"):
        engine.face_masks(1)


def test_rejections(emu_engine, student_weights):
    check_rejections(emu_engine, student_weights)


# ---- test 7: the last-call accessor (the entry points the emulator runs; the rest in the GPU file) ------------------------------------

def check_accessor(engine, rows, kps, counts, H, W, S=32):
    """pf_face_masks over the last call's `rows` rows == pf_mask_faces on the landmarks [F,K,98,2] and counts that call returned, in
    both spaces.  Returns the frame-space maps."""
    got = engine.face_masks(rows)
    want = engine.mask_faces(kps, H, W, counts=counts)
    assert_maps_equal(got, want)
    assert_maps_equal(engine.face_masks(rows, S), engine.mask_faces(kps, counts=counts, chip_size=S))
    return got


def check_after_landmarks(engine, frame, boxes, S=32):
    """pf_landmarks on a resident frame with one rejected box: the rejected row is dead, the others keep their slot numbers."""
    H, W = frame.shape[:2]
    bad = np.array([[10.0, 10.0, 25.0, 60.0]], np.float32)
    b = np.concatenate([boxes[:1], bad, boxes[1:]], 0)
    engine.set_frame(frame)
    kps, _, valid = engine.landmarks(None, b)
    assert valid.tolist() == [True, False] + [True] * (len(boxes) - 1)
    n, live = len(b), np.flatnonzero(valid)
    got = engine.face_masks(n)
    want = engine.mask_faces(kps[live][None], H, W)
    assert np.array_equal(got[3], valid) and np.array_equal(got[0], want[0]) and np.array_equal(got[2][live], want[2][0])
    assert np.array_equal(got[1], np.concatenate([[0], live + 1]).astype(np.uint8)[want[1]])        # owners are the call's row numbers
    assert not got[2][1].any()
    got_c, want_c = engine.face_masks(n, S), engine.mask_faces(kps[live][None], chip_size=S)
    assert np.array_equal(got_c[3][live], want_c[3][0]) and not got_c[3][1] and np.array_equal(got_c[0][live], want_c[0][0])
    return got


def check_after_run_frames(engine, frames, rows, top_k, min_face, S=32):
    counts, _, kps, _ = engine.run_frames(frames, 0.5, 0.3, min_face, top_k, planted_rows=rows)
    F, H, W = frames.shape[:3]
    got = check_accessor(engine, F * top_k, kps, counts, H, W, S)
    assert not got[3].reshape(F, top_k)[np.arange(top_k)[None] >= counts[:, None]].any()
    return counts, got


def test_face_masks_after_landmarks_and_run_frames(emu_engine, student_weights):
    _load_small_student(emu_engine, student_weights, 8)
    frame, boxes = synth_frame(270, 480, 2, seed=11)
    assert check_after_landmarks(emu_engine, frame, boxes)[3].any()
    F, K = 2, 4
    frames, rows = [], []
    for f in range(F):
        fr, bx = synth_frame(270, 480, 4 - f, seed=20 + f, face_w=300, face_h=400)
        bx[:, 2] += np.arange(len(bx)) * 6
        frames.append(fr)
        rows.append(plant_rows(bx, (270, 480), n_rows=1260, input_hw=(384, 640), per_box=6, seed=f))
    counts, got = check_after_run_frames(emu_engine, np.stack(frames), np.stack(rows), K, 100.0)
    assert counts.tolist() == [4, 3] and got[3].sum() == 7
    part = emu_engine.face_masks(K + 2)             # rows that end inside the second frame: two maps, the second from two slots
    assert part[0].shape[0] == 2 and np.array_equal(part[0][0], got[0][0]) and set(np.unique(part[1][1])) <= {0, 1, 2}

"""Aligned face chips (pf_align_faces / pf_face_chips, csrc/k_align.h) on the CPU tier, through the SIMT emulator: the fit against
the float64 restatement tests/align_ref.py, the warp bit for bit against its integer restatement, dead and degenerate slots, layout
independence, the ABI's refusals and the last-call accessor after the entry points the emulator can run.  The same checks run on a
real MI355X from tests/test_gpu_align_faces.py, which imports the ``check_*`` functions and the case table from here."""
import ctypes as C

import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd._native import PeppaHipError
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.synth import make_frame as synth_frame, plant_rows
from tests import align_ref as ar

# Test 1's tolerances: about 50 float64 operations on magnitudes <= 4096, error ~ 5e-11
TOL_AB, TOL_T = 1e-12, 1e-9
CASE_IDS = [c[0] for c in ar.CASES]


def assert_fit_close(M, ref):
    assert abs(M[0, 0] - ref[0, 0]) <= TOL_AB and abs(M[1, 0] - ref[1, 0]) <= TOL_AB
    assert M[0, 1] == -M[1, 0] and M[1, 1] == M[0, 0]
    assert abs(M[0, 2] - ref[0, 2]) <= TOL_T and abs(M[1, 2] - ref[1, 2]) <= TOL_T


def tile_bytes(M, S, H, W):
    """Per 16 x 16 tile: bytes of the source bounding box of its four corners (rows x 3 bytes per pixel), as the specification's
    coordinates give it; the kernel's LDS image is this plus at most 8 bytes of alignment per row."""
    a, b, tx, ty = M[0, 0], M[1, 0], M[0, 2], M[1, 2]
    det = a * a + b * b
    ia, ib = a / det, b / det
    itx, ity = -(ia * tx + ib * ty), -(ia * ty - ib * tx)
    out = []
    for y0 in range(0, S, 16):
        for x0 in range(0, S, 16):
            us, vs = [], []
            for y in (y0, y0 + 15):
                for x in (x0, x0 + 15):
                    us.append(int(np.floor(np.clip(ia * x + ib * y + itx, -2, W + 1))))
                    vs.append(int(np.floor(np.clip(ia * y - ib * x + ity, -2, H + 1))))
            bw, bh = max(us) - min(us) + 2, max(vs) - min(vs) + 2
            out.append((bh * bw * 3, bh * (bw * 3 + 8)))
    return out


# ---- tests 1 + 2: fit and warp ------------------------------------------------------------------------------------------------------

def check_fit_and_warp(engine, case):
    frame, kps, S = ar.case_scene(case)
    engine.profile_enable(True)
    chips, mats, valid = engine.align_faces(frame, kps, chip_size=S)
    log = engine.launch_log()
    engine.profile_enable(False)
    assert any("align_fit_kernel" in k for k in log) and any("align_warp_kernel" in k for k in log), log
    chips64, mats64, valid64 = engine.align_faces(frame, kps.astype(np.float64), chip_size=S)
    assert np.array_equal(mats, mats64) and np.array_equal(chips, chips64) and np.array_equal(valid, valid64)   # same values, either type
    for i in range(kps.shape[1]):
        ref, ok = ar.fit(kps[0, i], S)
        assert ok and valid[0, i]
        assert_fit_close(mats[0, i], ref)
        want = ar.warp(frame, mats[0, i], S)
        assert np.array_equal(chips[0, i], want), "%s: %d bytes differ" % (case[0], int((chips[0, i] != want).sum()))
        assert want.std() > 1.0                       # the chip shows the frame, not a constant
    # which path the tiles take, from the specification's own coordinates
    tb = tile_bytes(mats[0, 0], S, frame.shape[0], frame.shape[1])
    if case[0] == "huge_face":
        assert all(lo > 16384 for lo, _ in tb), tb
    elif case[0] == "roll45_scale02":
        assert any(lo > 16384 for lo, _ in tb) and any(hi <= 16384 for _, hi in tb), tb
    else:
        assert all(hi <= 16384 for _, hi in tb), tb
    if case[0] == "half_outside":
        assert (chips[0, 0] == 0).all(axis=2).mean() > 0.1       # border zeros
    if case[0] == "p0_on_integers":
        p0 = ar.five_points(kps[0, 0])[0]
        assert p0[0] == round(p0[0]) and p0[1] == round(p0[1])


@pytest.mark.parametrize("case", ar.CASES, ids=CASE_IDS)
def test_fit_and_warp(emu_engine, case):
    check_fit_and_warp(emu_engine, case)


# ---- test 3: dead and degenerate slots ----------------------------------------------------------------------------------------------

def _sentinel(F, K, S):
    return np.full((F, K, S, S, 3), 0xAB, np.uint8), np.frombuffer(b"\xab" * (F * K * 48), np.float64).reshape(F, K, 2, 3).copy()


def check_dead_slots(engine):
    S, F, K = 32, 2, 3
    frames = np.stack([ar.make_frame(120, 160, seed=1), ar.make_frame(120, 160, seed=2)])
    kps = np.stack([np.stack([ar.make_landmarks(50 + 25 * k, 60, 22, 10 * k, seed=30 + 3 * f + k) for k in range(K)]) for f in range(F)])
    chips, mats = _sentinel(F, K, S)
    s_chip, s_mat = chips[0, 0].copy(), mats[0, 0].copy()
    _, _, valid = engine.align_faces(frames, kps, counts=np.array([2, 0]), chip_size=S, out=(chips, mats))
    assert valid.tolist() == [[True, True, False], [False, False, False]]
    for f, k in ((0, 2), (1, 0), (1, 1), (1, 2)):
        assert np.array_equal(chips[f, k], s_chip) and mats[f, k].tobytes() == s_mat.tobytes()
    for k in range(2):
        assert np.array_equal(chips[0, k], ar.warp(frames[0], mats[0, k], S))
    # degenerate faces next to a good one
    good = ar.make_landmarks(80, 60, 22, 15, seed=40)
    same = np.full((98, 2), 37.5, np.float32)
    nan = good.copy(); nan[54, 0] = np.nan
    tiny = ar.make_landmarks(80, 60, 2000.0, 0, seed=41)            # scale 10.07 / 2000: det = 2.5e-5 < 2^-12
    for k4 in (same, nan, tiny):
        assert ar.fit(k4, S)[1] is False
    kps4 = np.stack([same, good, nan, tiny])[None]
    chips, mats = _sentinel(1, 4, S)
    _, _, valid = engine.align_faces(frames[0], kps4, chip_size=S, out=(chips, mats))
    assert valid.tolist() == [[False, True, False, False]]
    for k in (0, 2, 3):
        assert np.array_equal(chips[0, k], s_chip) and mats[0, k].tobytes() == s_mat.tobytes()
    alone = engine.align_faces(frames[0], good[None, None], chip_size=S)
    assert alone[2].all() and np.array_equal(alone[0][0, 0], chips[0, 1]) and np.array_equal(alone[1][0, 0], mats[0, 1])


def test_dead_slots(emu_engine):
    check_dead_slots(emu_engine)


# ---- test 4: layout -----------------------------------------------------------------------------------------------------------------

def raw_align(engine, frames_ptr, mem, F, H, W, kps_ptr, f64, kps_mem, counts_ptr, K, S, chips, mats, valid, out_mem=_native.PF_MEM_HOST):
    rc = engine.lib.pf_align_faces(engine.h, C.c_void_p(frames_ptr), mem, F, H, W, C.c_void_p(kps_ptr), f64, kps_mem,
                                   C.c_void_p(counts_ptr) if counts_ptr else None, K, S, _native._ptr(chips), _native._ptr(mats),
                                   _native._ptr(valid), out_mem)
    engine._check(rc, "pf_align_faces")


def check_layout(engine, to_device):
    """to_device(array) -> (device pointer, keep-alive): the emulator's device memory is host memory."""
    S, F, K = 32, 2, 2
    frames = np.stack([ar.make_frame(120, 160, seed=5), ar.make_frame(120, 160, seed=6)])
    kps = np.stack([np.stack([ar.make_landmarks(60 + 30 * k, 55 + 5 * f, 24, 20 * k - 10, seed=50 + 2 * f + k) for k in range(K)]) for f in range(F)])
    chips, mats, valid = engine.align_faces(frames, kps, chip_size=S)
    assert valid.all()
    for f in range(F):
        for k in range(K):            # a face's chip does not depend on its slot or on the batch
            c1, m1, v1 = engine.align_faces(frames[f], kps[f, k][None, None], chip_size=S)
            assert v1.all() and np.array_equal(c1[0, 0], chips[f, k]) and np.array_equal(m1[0, 0], mats[f, k])
    assert not np.array_equal(engine.align_faces(frames[1], kps[0], chip_size=S)[0][0], chips[0])     # the frames differ
    d_frames, keep1 = to_device(frames)
    d_kps, keep2 = to_device(kps)
    for fmem, kmem in ((_native.PF_MEM_DEVICE, _native.PF_MEM_HOST), (_native.PF_MEM_HOST, _native.PF_MEM_DEVICE),
                       (_native.PF_MEM_DEVICE, _native.PF_MEM_DEVICE)):
        c2, m2, v2 = np.zeros_like(chips), np.zeros_like(mats), np.zeros((F, K), np.int32)
        raw_align(engine, d_frames if fmem == _native.PF_MEM_DEVICE else frames.ctypes.data, fmem, F, 120, 160,
                  d_kps if kmem == _native.PF_MEM_DEVICE else kps.ctypes.data, 0, kmem, 0, K, S, c2, m2, v2)
        assert v2.all() and np.array_equal(c2, chips) and np.array_equal(m2, mats), (fmem, kmem)
    del keep1, keep2


def _host_as_device(a):
    a = np.ascontiguousarray(a)
    return a.ctypes.data, a


def test_layout(emu_engine):
    check_layout(emu_engine, _host_as_device)


# ---- test 5: rejections -------------------------------------------------------------------------------------------------------------

def _load_small_student(engine, weights, batch):
    engine.load_program(0, build_student_program(weights, 64, "f32")[0], batch)


def check_rejections(engine, weights):
    frame = ar.make_frame(120, 160, seed=9)
    kps = ar.make_landmarks(80, 60, 22, 0, seed=60)[None, None]
    for S in (100, 16, 272):
        chips, mats = np.full((1, 1, S, S, 3), 0xAB, np.uint8), np.zeros((1, 1, 2, 3))
        with pytest.raises(PeppaHipError, match="multiple of 16"):
            engine.align_faces(frame, kps, chip_size=S, out=(chips, mats))
        assert (chips == 0xAB).all() and (mats == 0).all()
        with pytest.raises(PeppaHipError, match="multiple of 16"):
            engine.face_chips(1, S)
    chips, mats, valid = np.full((2, 1, 32, 32, 3), 0xAB, np.uint8), np.zeros((2, 1, 2, 3)), np.zeros((2, 1), np.int32)
    k2 = np.concatenate([kps, kps])
    with pytest.raises(PeppaHipError, match="no resident frame"):
        raw_align(engine, 0, _native.PF_MEM_RESIDENT, 1, 120, 160, k2.ctypes.data, 0, _native.PF_MEM_HOST, 0, 1, 32, chips, mats, valid)
    engine.set_frame(frame)
    with pytest.raises(PeppaHipError, match="n_frames = 2"):
        raw_align(engine, 0, _native.PF_MEM_RESIDENT, 2, 120, 160, k2.ctypes.data, 0, _native.PF_MEM_HOST, 0, 1, 32, chips, mats, valid)
    assert (chips == 0xAB).all() and (mats == 0).all()
    got = engine.align_faces(None, kps, chip_size=32)                       # the resident frame itself is fine
    assert np.array_equal(got[0], engine.align_faces(frame, kps, chip_size=32)[0])
    with pytest.raises(PeppaHipError, match="left no face rows"):             # fresh handle: no pipeline call yet
        engine.face_chips(1, 32)
    _load_small_student(engine, weights, 2)
    with pytest.raises(PeppaHipError, match="left no face rows"):
        engine.face_chips(1, 32)
    engine.landmark_forward(np.zeros((1, 64, 64, 3), np.uint8))
    with pytest.raises(PeppaHipError, match="pf_landmark_forward.*no frame"):
        engine.face_chips(1, 32)
    big, boxes = synth_frame(270, 480, 2, seed=11)
    engine.landmarks(big, boxes)
    with pytest.raises(PeppaHipError, match="3 rows asked, the last call left 2"):
        engine.face_chips(3, 32)
    assert engine.face_chips(2, 32)[0].shape == (2, 32, 32, 3)


    # a call without boxes leaves no rows either
    rc = engine.lib.pf_landmarks(engine.h, _native._ptr(big), _native.PF_MEM_HOST, big.shape[0], big.shape[1], big.strides[0], None, 0,
                                 None, None, None)
    assert rc == 0
    with pytest.raises(PeppaHipError, match="left no face rows"):
        engine.face_chips(1, 32)


def test_rejections(emu_engine, student_weights):
    check_rejections(emu_engine, student_weights)


# ---- test 6: the last-call accessor (the entry points the emulator runs; the rest in the GPU file) ----------------------------------

def assert_chips_equal(got, want):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()


def check_after_landmarks(engine, frame, boxes, S=32):
    """pf_landmarks on a resident frame with one rejected box: face_chips == align_faces on what the call returned."""
    bad = np.array([[10.0, 10.0, 25.0, 60.0]], np.float32)
    b = np.concatenate([boxes[:1], bad, boxes[1:]], 0)
    engine.set_frame(frame)
    kps, _, valid = engine.landmarks(None, b)
    assert valid.tolist() == [True, False] + [True] * (len(boxes) - 1)
    n = len(b)
    got = engine.face_chips(n, S)
    assert not got[2][1]
    live = np.flatnonzero(valid)
    want = engine.align_faces(frame, kps[live][None], chip_size=S)
    assert_chips_equal((got[0][live], got[1][live], got[2][live]), (want[0][0], want[1][0], want[2][0]))
    assert (got[0][1] == 0).all()                 # the rejected row is left untouched
    return got


def check_after_landmarks_padded_rows(engine, frame, boxes, S=32):
    """pf_landmarks on host rows 5 bytes longer than 3 * W (no 4-byte aligned row starts): the chips are cut from those rows."""
    H, W = frame.shape[:2]
    stride = 3 * W + 5
    padded = np.full((H, stride), 0x5A, np.uint8)
    padded[:, :3 * W] = frame.reshape(H, 3 * W)
    n = len(boxes)
    b = np.ascontiguousarray(boxes[:, :4], np.float32)
    kps, scores, valid = np.zeros((n, 98, 2), np.float32), np.zeros((n, 98), np.float32), np.zeros((n,), np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    rc = engine.lib.pf_landmarks(engine.h, _native._ptr(padded), _native.PF_MEM_HOST, H, W, stride, b.ctypes.data_as(fp), n,
                                 kps.ctypes.data_as(fp), scores.ctypes.data_as(fp), valid.ctypes.data_as(ip))
    engine._check(rc, "pf_landmarks")
    assert valid.all()
    got = engine.face_chips(n, S)
    want = engine.align_faces(frame, kps[None], chip_size=S)
    assert_chips_equal(got, (want[0][0], want[1][0], want[2][0]))
    return got


def check_after_run_frames_resident(engine, frame, rows, top_k, min_face, S=32):
    """pf_run_frames on the resident frame (PF_MEM_RESIDENT): the chips come from that frame, not from a staging copy of an earlier call."""
    H, W = frame.shape[:2]
    engine.set_frame(frame)
    counts, boxes = np.zeros((1,), np.int32), np.zeros((1, top_k, 4), np.float32)
    kps, scores = np.zeros((1, top_k, 98, 2), np.float32), np.zeros((1, top_k, 98), np.float32)
    pr = np.ascontiguousarray(rows, np.float32)
    rc = engine.lib.pf_run_frames_planted(engine.h, _native._ptr(frame), _native.PF_MEM_RESIDENT, 1, H, W, _native._ptr(pr), pr.shape[0],
                                          0.5, 0.3, min_face, top_k, _native._ptr(counts), _native._ptr(boxes), _native._ptr(kps),
                                          _native._ptr(scores), _native.PF_MEM_HOST)
    engine._check(rc, "pf_run_frames_planted")
    got = engine.face_chips(top_k, S)
    want = engine.align_faces(frame, kps, counts=counts, chip_size=S)
    assert_chips_equal(got, (want[0][0], want[1][0], want[2][0]))
    return got


def check_after_run_frames(engine, frames, rows, top_k, min_face, S=32):
    counts, _, kps, _ = engine.run_frames(frames, 0.5, 0.3, min_face, top_k, planted_rows=rows)
    F = frames.shape[0]
    got = engine.face_chips(F * top_k, S)
    want = engine.align_faces(frames, kps, counts=counts, chip_size=S)
    assert_chips_equal(got, (want[0].reshape(got[0].shape), want[1].reshape(got[1].shape), want[2].reshape(-1)))
    assert not got[2].reshape(F, top_k)[np.arange(top_k)[None] >= counts[:, None]].any()
    return counts, got


def test_face_chips_after_landmarks_and_run_frames(emu_engine, student_weights):
    _load_small_student(emu_engine, student_weights, 8)
    frame, boxes = synth_frame(270, 480, 2, seed=11)
    check_after_landmarks(emu_engine, frame, boxes)
    F, K = 2, 4
    frames, rows = [], []
    for f in range(F):
        fr, bx = synth_frame(270, 480, 4 - f, seed=20 + f, face_w=300, face_h=400)
        bx[:, 2] += np.arange(len(bx)) * 6
        frames.append(fr)
        rows.append(plant_rows(bx, (270, 480), n_rows=1260, input_hw=(384, 640), per_box=6, seed=f))
    counts, _ = check_after_run_frames(emu_engine, np.stack(frames), np.stack(rows), K, 100.0)
    assert counts.tolist() == [4, 3]
    check_after_run_frames_resident(emu_engine, frames[1], rows[1], K, 100.0)       # the staging copy still starts with frames[0]
    check_after_landmarks_padded_rows(emu_engine, frame, boxes)


# ---- both kernel paths against the reference, explicitly ---------------------------------------------------------------------------

@pytest.fixture(scope="session")
def emu_tool_library():
    """The emulator build of the engine's TOOL flavour (-DPF_ABLATE=1): the only build that reads PEPPA_ALIGN_LDS, the LDS budget of
    align_warp_kernel, when a handle is created.  Same command as tests/simt_emu/build_emu.py, its own output file."""
    import os
    import subprocess
    from tests.simt_emu import build_emu as be
    if not be.available():
        pytest.skip("host clang not available for the SIMT emulator")
    os.makedirs(be.OUT_DIR, exist_ok=True)
    out = os.path.join(be.OUT_DIR, "libpeppa_emu_ablate.so")
    srcs = [os.path.join(be.CSRC, "engine.cpp"), os.path.join(be.CSRC, "mbx_launch.cpp"), os.path.join(be.HERE, "emu_runtime.cpp")]
    deps = [os.path.join(be.CSRC, f) for f in os.listdir(be.CSRC)] + [
        os.path.join(be.HERE, "emu_runtime.cpp"), os.path.join(be.HERE, "include", "pf_intrinsics.h"),
        os.path.join(be.HERE, "include", "hip", "hip_runtime.h"), os.path.join(be.ROOT, "include", "peppa_hip.h")]
    if not (os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps)):
        subprocess.run([be.CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-DPF_ABLATE=1",
                        "-I", os.path.join(be.HERE, "include"), "-I", be.CSRC] + srcs + ["-o", out], check=True)
    return out


@pytest.mark.parametrize("case", [c for c in ar.CASES if c[0] in ("scale04_roll30", "odd_width", "roll45_scale02")], ids=lambda c: c[0])
def test_direct_path_forced_equals_tiled_and_reference(emu_tool_library, monkeypatch, case):
    """The same case with the LDS budget as built (tiles that fit are staged) and forced to 0 (every tile reads the frame directly): both
    equal the reference, byte for byte.  Which path a tile takes is otherwise invisible, because the paths agree by construction."""
    from peppa_pig_face_landmark_amd._native import Engine
    frame, kps, S = ar.case_scene(case)
    outs = []
    for budget in (None, "0"):
        monkeypatch.delenv("PEPPA_ALIGN_LDS", raising=False)
        if budget is not None:
            monkeypatch.setenv("PEPPA_ALIGN_LDS", budget)
        eng = Engine(0, emu_tool_library)                 # the budget is read when the handle is created
        outs.append(eng.align_faces(frame, kps, chip_size=S))
        eng.close()
    assert outs[0][2].all()
    assert_chips_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][0][0, 0], ar.warp(frame, outs[0][1][0, 0], S))

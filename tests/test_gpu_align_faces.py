"""Aligned face chips on a real MI355X: the cases of tests/test_align_faces.py (fit, bit-exact warp on both kernel paths, dead slots,
layout, refusals) through the HIP library, the last-call accessor pf_face_chips after every pipeline entry point (pf_landmarks,
pf_run_frames, pf_track_frame, pf_track_streams, pf_batch_run_frames with front mode on and off) against pf_align_faces on what
those calls returned, the Python classes, and run-to-run bit identity."""
import numpy as np
import pytest
import torch

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
from tests import align_ref as ar
from tests import test_align_faces as T

pytestmark = pytest.mark.gpu

S = 32
SA = 112      # the accessor tests: the synthetic weights' landmarks are scattered, and at 112 their fits stay above the 1/64 scale limit
# The tracking tests plant small faces: the synthetic weights' landmarks scatter over several box widths and the track boxes are
# their hulls, so with the 200 x 260 faces of the other tests the tracked frame's landmarks spread over thousands of pixels and every
# fit falls below the 1/64 scale limit (dead rows only).  48 x 62 faces keep the tracked frame's fits valid.
SMALL = dict(face_w=48, face_h=62)
TRACK = dict(score_thres=0.5, nms_iou_thres=0.3, min_face=1600.0, track_iou_thres=0.5, smooth_box=0.3, diff_thres=5.0)


def _to_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.data_ptr(), t


@pytest.mark.parametrize("case", ar.CASES, ids=T.CASE_IDS)
def test_fit_and_warp(gpu_engine, case):
    T.check_fit_and_warp(gpu_engine, case)


def test_dead_slots(gpu_engine):
    T.check_dead_slots(gpu_engine)


def test_layout(gpu_engine):
    T.check_layout(gpu_engine, _to_device)


def test_rejections(gpu_engine, student_weights):
    T.check_rejections(gpu_engine, student_weights)


def test_device_outputs_and_unaligned_chip_pointer(gpu_engine):
    """out_mem = PF_MEM_DEVICE: the kernels write the caller's buffers (dead slots untouched); a chip pointer that is not 4-byte
    aligned takes the byte stores and gives the same bytes."""
    frame = ar.make_frame(120, 160, seed=3)
    kps = np.stack([ar.make_landmarks(60 + 30 * k, 60, 24, 15 * k, seed=70 + k) for k in range(3)])[None]
    counts = np.array([2], np.int32)
    want = gpu_engine.align_faces(frame, kps, counts=counts, chip_size=S)
    for off in (0, 1):
        d_chips = torch.full((3 * S * S * 3 + 4,), 0xAB, dtype=torch.uint8, device="cuda")
        d_mats = torch.zeros((3, 2, 3), dtype=torch.float64, device="cuda")
        d_valid = torch.full((3,), 7, dtype=torch.int32, device="cuda")
        T.raw_align(gpu_engine, frame.ctypes.data, _native.PF_MEM_HOST, 1, 120, 160, kps.ctypes.data, 0, _native.PF_MEM_HOST,
                    counts.ctypes.data, 3, S, d_chips.data_ptr() + off, d_mats.data_ptr(), d_valid.data_ptr(), _native.PF_MEM_DEVICE)
        gpu_engine.sync()
        got = d_chips.cpu().numpy()[off:off + 3 * S * S * 3].reshape(3, S, S, 3)
        assert d_valid.cpu().tolist() == [1, 1, 0]
        assert np.array_equal(got[:2], want[0][0, :2]) and (got[2] == 0xAB).all()
        assert np.array_equal(d_mats.cpu().numpy()[:2], want[1][0, :2]) and (d_mats.cpu().numpy()[2] == 0).all()


def test_repeatability(gpu_engine):
    """Two runs of a 64-face call are bit-identical."""
    F, K = 8, 8
    frames = np.stack([ar.make_frame(240, 320, seed=80 + f) for f in range(F)])
    kps = np.stack([np.stack([ar.make_landmarks(40 + 30 * k, 60 + 15 * f, 20 + 4 * k, 40 * k - 150 + 7 * f, seed=90 + 8 * f + k)
                              for k in range(K)]) for f in range(F)])
    a = gpu_engine.align_faces(frames, kps, chip_size=112)
    b = gpu_engine.align_faces(frames, kps, chip_size=112)
    assert a[2].all()
    T.assert_chips_equal(a, b)


# ---- the last-call accessor -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def blobs(student_weights, detector_weights):
    return (build_student_program(student_weights, 128, "f32")[0], build_detector_program(detector_weights, (384, 640), "f32s")[0])


def _scene(F, K, seed, face_w=200, face_h=260):
    frames, rows = [], []
    for f in range(F):
        frame, boxes = make_frame(1080, 1920, K, seed=seed + f, face_w=face_w, face_h=face_h)
        frames.append(frame)
        rows.append(plant_rows(boxes, (1080, 1920), 15120, (384, 640), 24, seed=seed + f))
    return np.stack(frames), np.stack(rows)


def test_face_chips_after_landmarks_and_run_frames(gpu_engine, blobs):
    gpu_engine.load_program(0, blobs[0], 8)
    gpu_engine.load_program(1, blobs[1], 2)
    frame, boxes = make_frame(1080, 1920, 3, seed=44)
    got = T.check_after_landmarks(gpu_engine, frame, boxes, SA)
    assert got[2].any()
    frames, rows = _scene(2, 4, seed=31)
    counts, got = T.check_after_run_frames(gpu_engine, frames, rows, 4, 1600.0, SA)
    assert counts.tolist() == [4, 4] and got[2].any()
    # device-resident frames: the caller's pointer is read again
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    gpu_engine.run_frames_device(d_frames.data_ptr(), 2, 1080, 1920, 0.5, 0.3, 1600.0, 4, d_planted=d_rows.data_ptr(), rows=rows.shape[1])
    T.assert_chips_equal(gpu_engine.face_chips(8, SA), got)
    assert T.check_after_run_frames_resident(gpu_engine, frames[1], rows[1], 4, 1600.0, SA)[2].any()
    assert T.check_after_landmarks_padded_rows(gpu_engine, frame, boxes, SA)[2].any()


def test_face_chips_after_track_frame(gpu_engine, blobs):
    """Two frames: the second is tracked, its landmarks are the smoothed float64 ones."""
    K = 4
    gpu_engine.load_program(0, blobs[0], K)
    gpu_engine.load_program(1, blobs[1], 1)
    frames, rows = _scene(1, K, seed=71, **SMALL)
    for rep in range(2):
        boxes, kps, _, ran = gpu_engine.track_frame(frames[0], TRACK["score_thres"], TRACK["nms_iou_thres"], TRACK["min_face"], K,
                                                    TRACK["track_iou_thres"], TRACK["smooth_box"], TRACK["diff_thres"], rows[0])
        assert ran == (rep == 0) and len(boxes) == K and kps.dtype == np.float64
        got = gpu_engine.face_chips(len(boxes), SA)
        want = gpu_engine.align_faces(frames[0], kps[None], chip_size=SA)
        T.assert_chips_equal(got, (want[0][0], want[1][0], want[2][0]))
        assert got[2].any(), rep        # the tracked frame's chips are compared too, not only dead rows


def test_face_chips_after_track_streams(gpu_engine, blobs):
    """Three streams, one of which sits out the second call: frame i of a call is read from the slot of stream_ids[i]."""
    K = 2
    gpu_engine.load_program(0, blobs[0], 3 * K)
    gpu_engine.load_program(1, blobs[1], 3)
    gpu_engine.track_streams_config(3, K)
    frames, rows = _scene(3, K, seed=120, **SMALL)
    for ids in ([2, 0, 1], [1, 2]):       # never the identity: frame i of a call lives in slot stream_ids[i], not in slot i
        fr, rw = frames[ids], rows[ids]
        res = gpu_engine.track_streams(ids, fr, planted_rows=rw, **TRACK)
        n = len(ids)
        kps = np.zeros((n, K, 98, 2), np.float64)
        counts = np.array([len(r[0]) for r in res], np.int32)
        for i, r in enumerate(res):
            kps[i, :counts[i]] = r[1]
        assert counts.tolist() == [K] * n
        got = gpu_engine.face_chips(n * K, SA)
        want = gpu_engine.align_faces(fr, kps, counts=counts, chip_size=SA)
        T.assert_chips_equal(got, (want[0].reshape(got[0].shape), want[1].reshape(got[1].shape), want[2].reshape(-1)))
        assert got[2].any(), ids


def test_face_chips_after_batch_run_frames(gpu_engine, blobs, hip_library):
    """pf_batch_run_frames with 2 lanes, front mode on (device-resident frames) and off: pf_batch_face_chips gathers the lanes' rows."""
    F, K = 3, 4
    frames, rows = _scene(F, K, seed=90)
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    for front in (1, 0):
        be = _native.BatchEngine(0, 2, hip_library)
        be.set_option(_native.PF_OPT_BATCH_FRONT, front)
        be.load_program(0, blobs[0], 2 * K)
        be.load_program(1, blobs[1], F if front else 2)
        with pytest.raises(_native.PeppaHipError, match="multiple of 16"):
            be.face_chips(0, 100)
        for device_path in (True, False):
            if device_path:
                d_counts = torch.zeros(F, dtype=torch.int32, device="cuda")
                d_kps = torch.zeros((F, K, 98, 2), dtype=torch.float32, device="cuda")
                be.run_frames_device(d_frames.data_ptr(), F, 1080, 1920, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(),
                                     rows=rows.shape[1], d_counts=d_counts.data_ptr(), d_kps=d_kps.data_ptr())
                d_chips = torch.zeros((F * K, SA, SA, 3), dtype=torch.uint8, device="cuda")
                d_mats = torch.zeros((F * K, 2, 3), dtype=torch.float64, device="cuda")
                d_valid = torch.zeros((F * K,), dtype=torch.int32, device="cuda")
                be.face_chips_device(F * K, SA, d_chips.data_ptr(), d_mats.data_ptr(), d_valid.data_ptr())
                be.sync()
                counts, kps = d_counts.cpu().numpy(), d_kps.cpu().numpy()
                got = (d_chips.cpu().numpy(), d_mats.cpu().numpy(), d_valid.cpu().numpy().astype(bool))
            else:
                counts, _, kps, _ = be.run_frames(frames, 0.5, 0.3, 1600.0, K, planted_rows=rows)
                got = be.face_chips(F * K, SA)
            assert counts.tolist() == [K] * F
            want = gpu_engine.align_faces(frames, kps, counts=counts, chip_size=SA)
            T.assert_chips_equal(got, (want[0].reshape(got[0].shape), want[1].reshape(got[1].shape), want[2].reshape(-1)))
            assert got[2].any()
        be.close()


# ---- the Python classes ---------------------------------------------------------------------------------------------------------

def _check_results(results, frame, off_results):
    """Every face: "chip" [32,32,3] == align_ref.warp(frame, its matrix), the matrix == align_ref.fit(its kps) within test 1's
    tolerances (a degenerate fit carries neither key); boxes, landmarks and scores equal those with the option off."""
    assert len(results) == len(off_results) and results
    n_chips = 0
    for r, r0 in zip(results, off_results):
        for key in ("box", "kps", "scores"):
            assert np.array_equal(r[key], r0[key]), key
        assert "chip" not in r0 and "chip_matrix" not in r0
        ref, ok = ar.fit(r["kps"], S)
        assert ("chip" in r) == ok and ("chip_matrix" in r) == ok
        if ok:
            n_chips += 1
            assert r["chip"].shape == (S, S, 3) and r["chip"].dtype == np.uint8 and r["chip_matrix"].shape == (2, 3)
            T.assert_fit_close(r["chip_matrix"], ref)
            assert np.array_equal(r["chip"], ar.warp(frame, r["chip_matrix"], S))
    return n_chips


@pytest.mark.parametrize("which", ["faceana_host_tracking", "faceana_device_tracking", "stream_tracker", "frame_batch_runner"])
def test_classes_carry_chips(hip_library, student_weights, detector_weights, which):
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.batch_runner import FrameBatchRunner
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker
    frames, rows = _scene(2, 4, seed=120)
    boxes = make_frame(1080, 1920, 4, seed=120)[1]
    W = {"detector": detector_weights, "keypoints": student_weights}
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["topk"] = 4
    cfg["Skps"]["Engine"]["device_tracking"] = which == "faceana_device_tracking"
    out = {}
    for size in (0, S):
        if which.startswith("faceana"):
            fa = FaceAna(cfg=cfg, weights=W, library=hip_library, face_chips=size)
            fa._planted_rows = lambda: rows[0]
            if which == "faceana_host_tracking":        # the planted boxes stand in for the synthetic detector's answer
                fa.face_detector = lambda image: np.concatenate([boxes, np.ones((len(boxes), 1), np.float32)], 1)
            out[size] = [fa.run(frames[0]), fa.run(frames[0])]       # a detector frame and a tracked one
            fa.engine.close()
        elif which == "stream_tracker":
            st = StreamTracker(cfg=cfg, weights=W, max_streams=2, library=hip_library, face_chips=size)
            st._planted_rows = lambda ids, fr: rows[:len(ids)]
            r = st.run({0: frames[0], 1: frames[1]})
            out[size] = [r[0], r[1]]
            st.close()
        else:
            fb = FrameBatchRunner(cfg=cfg, weights=W, lanes=2, frames_per_lane=1, library=hip_library, face_chips=size)
            fb._planted_rows = lambda fr: rows[:len(fr)]
            out[size] = fb.run(frames)
            fb.close()
    n_chips = 0
    for i in range(2):
        n_chips += _check_results(out[S][i], frames[0 if which.startswith("faceana") else i], out[0][i])
    assert n_chips >= 1      # (the synthetic landmarks are scattered: some fits fall below the 1/64 scale limit and carry no chip)

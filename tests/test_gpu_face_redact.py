"""Face redaction on a real MI355X: the cases of tests/test_face_redact.py (the restatement byte for byte under every mode and mask,
small frames, overlap and select, dead slots, device outputs through unaligned pointers, refusals) through the HIP library, the
last-call accessor pf_face_redact after every pipeline entry point (pf_landmarks, pf_run_frames with host, device and resident frames,
pf_track_frame, pf_track_streams, pf_batch_run_frames with front mode on and off) against pf_redact_faces on what those calls returned
and against the restatement, and the Python classes.  Frames are uniform random bytes throughout: the faces come from planted detector
rows, and what the landmark network makes of noise is as good a polygon as any."""
import numpy as np
import pytest
import torch

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
from tests import mask_ref as mr
from tests import redact_ref as rr
from tests import test_face_redact as T

pytestmark = pytest.mark.gpu

H, W = 1080, 1920
SMALL = dict(face_w=48, face_h=62)
TRACK = dict(score_thres=0.5, nms_iou_thres=0.3, min_face=1600.0, track_iou_thres=0.5, smooth_box=0.3, diff_thres=5.0)


def _dev_bytes(spec):
    t = torch.from_numpy(spec).cuda() if isinstance(spec, np.ndarray) else torch.full((spec[0],), spec[1], dtype=torch.uint8, device="cuda")
    return t.data_ptr(), lambda: t.cpu().numpy()


@pytest.mark.parametrize("case", mr.CASES, ids=mr.CASE_IDS)
def test_restatement(gpu_engine, case):
    T.check_restatement(gpu_engine, case)


def test_small_frames(gpu_engine):
    T.check_small_frames(gpu_engine)


def test_overlap_order_and_select(gpu_engine):
    T.check_overlap_select(gpu_engine)


def test_dead_slots(gpu_engine):
    T.check_dead_slots(gpu_engine)


def test_device_outputs_and_unaligned_pointers(gpu_engine):
    T.check_device_outputs(gpu_engine, _dev_bytes, gpu_engine.sync)


def test_repeatability(gpu_engine):
    T.check_repeatability(gpu_engine)


def test_rejections(gpu_engine, student_weights):
    T.check_rejections(gpu_engine, student_weights)


# ---- the last-call accessor -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def blobs(student_weights, detector_weights):
    return (build_student_program(student_weights, 128, "f32")[0], build_detector_program(detector_weights, (384, 640), "f32s")[0])


def _scene(F, K, seed, face_w=200, face_h=260):
    """F noise frames, the detector rows planted for K boxes each, and the boxes of the first frame."""
    rows, boxes0 = [], None
    for f in range(F):
        boxes = make_frame(H, W, K, seed=seed + f, face_w=face_w, face_h=face_h)[1]
        boxes0 = boxes if boxes0 is None else boxes0
        rows.append(plant_rows(boxes, (H, W), 15120, (384, 640), 24, seed=seed + f))
    return T.random_frame(H, W, seed=seed, F=F), np.stack(rows), boxes0


def test_face_redact_after_landmarks_and_run_frames(gpu_engine, blobs):
    gpu_engine.load_program(0, blobs[0], 8)
    gpu_engine.load_program(1, blobs[1], 2)
    frames, rows, boxes = _scene(2, 3, seed=44)
    T.check_after_landmarks(gpu_engine, frames[0], boxes)
    counts, kps, outs = T.check_after_run_frames(gpu_engine, frames, rows, 3, 1600.0)
    assert counts.tolist() == [3, 3]
    # device-resident frames: the redaction reads them again, so they stay alive; the output goes to device memory
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    gpu_engine.run_frames_device(d_frames.data_ptr(), 2, H, W, 0.5, 0.3, 1600.0, 3, d_planted=d_rows.data_ptr(), rows=rows.shape[1])
    for i, (mode, strength, label_mask, pad) in enumerate(T.ACCESSOR_MODES):
        d_out = torch.full((2, H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
        d_valid = torch.zeros((6,), dtype=torch.int32, device="cuda")
        gpu_engine.face_redact_device(6, d_out.data_ptr(), mode=mode, labels=label_mask, strength=strength, pad=pad, d_valid=d_valid.data_ptr())
        gpu_engine.sync()
        T.assert_frames_equal(d_out.cpu().numpy(), outs[i], mode)
        assert d_valid.cpu().numpy().all()
    # the resident frame of pf_set_frame (PF_MEM_RESIDENT)
    gpu_engine.set_frame(frames[1])
    c1, k1 = np.zeros((1,), np.int32), np.zeros((1, 3, 98, 2), np.float32)
    pr = np.ascontiguousarray(rows[1], np.float32)
    rc = gpu_engine.lib.pf_run_frames_planted(gpu_engine.h, _native._ptr(frames[1]), _native.PF_MEM_RESIDENT, 1, H, W, _native._ptr(pr), pr.shape[0], 0.5, 0.3,
                                              1600.0, 3, _native._ptr(c1), None, _native._ptr(k1), None, _native.PF_MEM_HOST)
    gpu_engine._check(rc, "pf_run_frames_planted")
    assert c1.tolist() == [3]
    T.check_accessor(gpu_engine, 3, frames[1:2], k1, c1)


def test_face_redact_after_track_frame(gpu_engine, blobs):
    """Two calls on one frame: the second is tracked, its landmarks are the smoothed float64 ones."""
    K = 4
    gpu_engine.load_program(0, blobs[0], K)
    gpu_engine.load_program(1, blobs[1], 1)
    frames, rows, _ = _scene(1, K, seed=71, **SMALL)
    for rep in range(2):
        boxes, kps, _, ran = gpu_engine.track_frame(frames[0], TRACK["score_thres"], TRACK["nms_iou_thres"], TRACK["min_face"], K,
                                                    TRACK["track_iou_thres"], TRACK["smooth_box"], TRACK["diff_thres"], rows[0])
        assert ran == (rep == 0) and len(boxes) >= 1 and kps.dtype == np.float64
        outs = T.check_accessor(gpu_engine, len(boxes), frames, kps[None], None)
        assert (outs[0] != frames).any(), rep


def test_face_redact_after_track_streams(gpu_engine, blobs):
    """Three streams, one of which sits out the second call; the ids are never the identity."""
    K = 2
    gpu_engine.load_program(0, blobs[0], 3 * K)
    gpu_engine.load_program(1, blobs[1], 3)
    gpu_engine.track_streams_config(3, K)
    frames, rows, _ = _scene(3, K, seed=120, **SMALL)
    for ids in ([2, 0, 1], [1, 2]):
        res = gpu_engine.track_streams(ids, frames[ids], planted_rows=rows[ids], **TRACK)
        n = len(ids)
        kps = np.zeros((n, K, 98, 2), np.float64)
        counts = np.array([len(r[0]) for r in res], np.int32)
        for i, r in enumerate(res):
            kps[i, :counts[i]] = r[1]
        assert counts.sum() >= 1
        outs = T.check_accessor(gpu_engine, n * K, frames[ids], kps, counts)
        assert outs[0].shape == (n, H, W, 3) and (outs[0] != frames[ids]).any(), ids


def test_face_redact_after_batch_run_frames(gpu_engine, blobs, hip_library):
    """pf_batch_run_frames with 2 lanes, front mode on (device-resident frames) and off: pf_batch_face_redact gathers the lanes' frames."""
    F, K = 3, 2
    frames, rows, _ = _scene(F, K, seed=90)
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    select = np.array([1, 0, 1, 1, 0, 1], np.int32)
    for front in (1, 0):
        be = _native.BatchEngine(0, 2, hip_library)
        be.set_option(_native.PF_OPT_BATCH_FRONT, front)
        be.load_program(0, blobs[0], 2 * K)
        be.load_program(1, blobs[1], F if front else 2)
        with pytest.raises(_native.PeppaHipError, match="pf_batch_face_redact.*cell size"):
            be.face_redact_device(0, 1, mode="mosaic", strength=5)
        with pytest.raises(_native.PeppaHipError, match="left face rows"):
            be.face_redact_device(1, 1)
        for device_path in (True, False):
            if device_path:
                d_counts = torch.zeros(F, dtype=torch.int32, device="cuda")
                d_kps = torch.zeros((F, K, 98, 2), dtype=torch.float32, device="cuda")
                be.run_frames_device(d_frames.data_ptr(), F, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(),
                                     rows=rows.shape[1], d_counts=d_counts.data_ptr(), d_kps=d_kps.data_ptr())
                d_out = torch.full((F, H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
                d_valid = torch.zeros((F * K,), dtype=torch.int32, device="cuda")
                be.face_redact_device(F * K, d_out.data_ptr(), select=select, mode="blur", labels=0x3FE, strength=8, pad=4, d_valid=d_valid.data_ptr())
                be.sync()
                counts, kps = d_counts.cpu().numpy(), d_kps.cpu().numpy()
                got, valid = d_out.cpu().numpy(), d_valid.cpu().numpy().astype(bool)
            else:
                counts, _, kps, _ = be.run_frames(frames, 0.5, 0.3, 1600.0, K, planted_rows=rows)
                got, valid = be.face_redact(F * K, select=select, mode="blur", labels=0x3FE, strength=8, pad=4)
            assert counts.tolist() == [K] * F
            want, want_valid = gpu_engine.redact_faces(frames, kps, counts=counts, select=select.reshape(F, K), mode="blur", labels=0x3FE,
                                                       strength=8, pad=4)
            T.assert_frames_equal(got, want, "front %d device %d" % (front, device_path))
            assert np.array_equal(valid, want_valid.reshape(-1))
            for f in range(F):
                ref = rr.frame_reference(frames[f], kps[f], counts[f], select.reshape(F, K)[f], rr.BLUR, 0x3FE, 8, 4)[0]
                T.assert_frames_equal(got[f], ref, "frame %d" % f)
                assert (got[f] != frames[f]).any()
        be.close()


# ---- the Python classes ---------------------------------------------------------------------------------------------------------

REDACT = {"mode": "mosaic", "labels": 0x3FE, "strength": 16, "pad": 6}


def _check_results(results, off_results, frame, redacted):
    """last_redacted == the restatement on the landmarks the dicts carry; boxes, landmarks and scores equal those with the option off."""
    assert len(results) == len(off_results)
    for r, r0 in zip(results, off_results):
        assert set(r) == set(r0)
        for key in ("box", "kps", "scores"):
            assert np.array_equal(r[key], r0[key]), key
    assert redacted.dtype == np.uint8 and redacted.shape == frame.shape
    if not results:
        assert np.array_equal(redacted, frame)
        return 0
    want = rr.frame_reference(frame, np.stack([r["kps"] for r in results]), None, None, rr.MOSAIC, REDACT["labels"], REDACT["strength"], REDACT["pad"])[0]
    T.assert_frames_equal(redacted, want, "last_redacted")
    return int((redacted != frame).any())


@pytest.mark.parametrize("which", ["faceana_host_tracking", "faceana_device_tracking", "stream_tracker", "frame_batch_runner"])
def test_classes_keep_redacted_frames(hip_library, student_weights, detector_weights, which):
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.batch_runner import FrameBatchRunner
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker
    frames, rows, boxes = _scene(2, 4, seed=120)
    weights = {"detector": detector_weights, "keypoints": student_weights}
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["topk"] = 4
    cfg["Skps"]["Engine"]["device_tracking"] = which == "faceana_device_tracking"
    out, kept, used = {}, {}, []
    for on in (None, REDACT):
        if which.startswith("faceana"):
            fa = FaceAna(cfg=cfg, weights=weights, library=hip_library, redact=on)
            fa._planted_rows = lambda: rows[0]
            if which == "faceana_host_tracking":        # the planted boxes stand in for the synthetic detector's answer
                fa.face_detector = lambda image: np.concatenate([boxes, np.ones((len(boxes), 1), np.float32)], 1)
            out[bool(on)], kept[bool(on)] = [], []
            for _ in range(2):                          # a detector frame and a tracked one
                out[bool(on)].append(fa.run(frames[0]))
                kept[bool(on)].append(fa.last_redacted)
            used = [frames[0], frames[0]]
            fa.engine.close()
        elif which == "stream_tracker":
            st = StreamTracker(cfg=cfg, weights=weights, max_streams=2, library=hip_library, redact=on)
            st._planted_rows = lambda ids, fr: rows[:len(ids)]
            r = st.run({0: frames[0], 1: frames[1]})
            out[bool(on)] = [r[0], r[1]]
            kept[bool(on)] = [st.last_redacted[s] for s in (0, 1)] if on else [st.last_redacted] * 2
            used = [frames[0], frames[1]]
            st.close()
        else:
            fb = FrameBatchRunner(cfg=cfg, weights=weights, lanes=2, frames_per_lane=1, library=hip_library, redact=on)
            fb._planted_rows = lambda fr: rows[:len(fr)]
            out[bool(on)] = fb.run(frames)
            kept[bool(on)] = [fb.last_redacted[f] for f in range(2)] if on else [fb.last_redacted] * 2
            used = [frames[0], frames[1]]
            fb.close()
    changed = 0
    for i in range(2):
        assert kept[False][i] is None
        changed += _check_results(out[True][i], out[False][i], used[i], kept[True][i])
    assert changed >= 1

"""Per-face region statistics on a real MI355X: the cases of tests/test_face_stats.py (the restatement value for value under two pairs
of thresholds, closed forms, small frames, overlap, dead slots, device outputs through offset pointers, refusals) through the HIP
library, the last-call accessor pf_face_stats after every pipeline entry point (pf_landmarks, pf_run_frames with host, device and
resident frames, pf_track_frame, pf_track_streams, pf_batch_run_frames with front mode on and off) against pf_measure_faces on what
those calls returned and against the restatement, one 2160 x 3840 frame that a 32-bit partial kept over a band would overflow, and the
Python classes.  Frames are uniform random bytes unless stated: the faces come from planted detector rows, and what the landmark
network makes of noise is as good a polygon as any."""
import numpy as np
import pytest
import torch

from peppa_pig_face_landmark_amd import _native
from tests import align_ref as ar
from tests import stats_ref as sr
from tests import test_face_stats as T
from tests.test_gpu_face_redact import H, W, SMALL, TRACK, _dev_bytes, _scene, blobs  # noqa: F401  (blobs: a fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", T.mr.CASES, ids=T.mr.CASE_IDS)
def test_restatement(gpu_engine, case):
    T.check_restatement(gpu_engine, case)


def test_closed_forms(gpu_engine):
    T.check_closed_forms(gpu_engine)


def test_small_frames(gpu_engine):
    T.check_small_frames(gpu_engine)


def test_overlap_and_ownership(gpu_engine):
    T.check_overlap(gpu_engine)


def test_dead_slots(gpu_engine):
    T.check_dead_slots(gpu_engine)


def test_device_outputs_and_offset_pointers(gpu_engine):
    T.check_device_outputs(gpu_engine, _dev_bytes, gpu_engine.sync)


def test_repeatability(gpu_engine):
    T.check_repeatability(gpu_engine)


def test_rejections(gpu_engine, student_weights):
    T.check_rejections(gpu_engine, student_weights)
    with pytest.raises(_native.PeppaHipError, match="pf_face_stats.*8-byte aligned"):
        gpu_engine.face_stats_device(1, 4)


# ---- the last-call accessor -----------------------------------------------------------------------------------------------------

def test_face_stats_after_landmarks_and_run_frames(gpu_engine, blobs):
    gpu_engine.load_program(0, blobs[0], 8)
    gpu_engine.load_program(1, blobs[1], 2)
    frames, rows, boxes = _scene(2, 3, seed=44)
    T.check_after_landmarks(gpu_engine, frames[0], boxes)
    counts, kps, got = T.check_after_run_frames(gpu_engine, frames, rows, 3, 1600.0)
    assert counts.tolist() == [3, 3]
    # device-resident frames: the reduction reads them again, so they stay alive; the output goes to device memory
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    gpu_engine.run_frames_device(d_frames.data_ptr(), 2, H, W, 0.5, 0.3, 1600.0, 3, d_planted=d_rows.data_ptr(), rows=rows.shape[1])
    d_out = torch.full((6 * 72 * 8,), 0xAB, dtype=torch.uint8, device="cuda")
    d_valid = torch.zeros((6,), dtype=torch.int32, device="cuda")
    gpu_engine.face_stats_device(6, d_out.data_ptr(), d_valid.data_ptr())
    gpu_engine.sync()
    T.assert_stats_equal(d_out.cpu().numpy().view(np.uint64).reshape(6, 8, 9), got, "device frames, device output")
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


def test_face_stats_after_track_frame(gpu_engine, blobs):
    """Two calls on one frame: the second is tracked, its landmarks are the smoothed float64 ones."""
    K = 4
    gpu_engine.load_program(0, blobs[0], K)
    gpu_engine.load_program(1, blobs[1], 1)
    frames, rows, _ = _scene(1, K, seed=71, **SMALL)
    for rep in range(2):
        boxes, kps, _, ran = gpu_engine.track_frame(frames[0], TRACK["score_thres"], TRACK["nms_iou_thres"], TRACK["min_face"], K,
                                                    TRACK["track_iou_thres"], TRACK["smooth_box"], TRACK["diff_thres"], rows[0])
        assert ran == (rep == 0) and len(boxes) >= 1 and kps.dtype == np.float64
        got = T.check_accessor(gpu_engine, len(boxes), frames, kps[None], None)
        assert int(got[:, :, 0].sum()) > 0, rep


def test_face_stats_after_track_streams(gpu_engine, blobs):
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
        got = T.check_accessor(gpu_engine, n * K, frames[ids], kps, counts)
        assert got.shape == (n * K, 8, 9) and int(got[:, :, 0].sum()) > 0, ids


def test_face_stats_after_batch_run_frames(gpu_engine, blobs, hip_library):
    """pf_batch_run_frames with 2 lanes, front mode on (device-resident frames) and off: pf_batch_face_stats gathers the lanes' rows."""
    F, K = 3, 2
    frames, rows, _ = _scene(F, K, seed=90)
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    for front in (1, 0):
        be = _native.BatchEngine(0, 2, hip_library)
        be.set_option(_native.PF_OPT_BATCH_FRONT, front)
        be.load_program(0, blobs[0], 2 * K)
        be.load_program(1, blobs[1], F if front else 2)
        with pytest.raises(_native.PeppaHipError, match="pf_batch_face_stats.*0 <= dark < bright <= 255"):
            be.face_stats_device(0, 8, dark=240, bright=16)
        with pytest.raises(_native.PeppaHipError, match="left face rows"):
            be.face_stats_device(1, 8)
        for device_path in (True, False):
            if device_path:
                d_counts = torch.zeros(F, dtype=torch.int32, device="cuda")
                d_kps = torch.zeros((F, K, 98, 2), dtype=torch.float32, device="cuda")
                be.run_frames_device(d_frames.data_ptr(), F, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(),
                                     rows=rows.shape[1], d_counts=d_counts.data_ptr(), d_kps=d_kps.data_ptr())
                d_out = torch.full((F * K * 72 * 8,), 0xAB, dtype=torch.uint8, device="cuda")
                d_valid = torch.zeros((F * K,), dtype=torch.int32, device="cuda")
                be.face_stats_device(F * K, d_out.data_ptr(), d_valid.data_ptr(), dark=64, bright=192)
                be.sync()
                counts, kps = d_counts.cpu().numpy(), d_kps.cpu().numpy()
                got, valid = d_out.cpu().numpy().view(np.uint64).reshape(F * K, 8, 9), d_valid.cpu().numpy().astype(bool)
            else:
                counts, _, kps, _ = be.run_frames(frames, 0.5, 0.3, 1600.0, K, planted_rows=rows)
                got, valid = be.face_stats(F * K, dark=64, bright=192)
            assert counts.tolist() == [K] * F
            want, want_valid = gpu_engine.measure_faces(frames, kps, counts=counts, dark=64, bright=192)
            T.assert_stats_equal(got, want.reshape(F * K, 8, 9), "front %d device %d" % (front, device_path))
            assert np.array_equal(valid, want_valid.reshape(-1)) and valid.all()
            for f in range(F):
                ref = sr.frame_reference(frames[f], kps[f], counts[f], 64, 192)[0]
                T.assert_stats_equal(got[f * K:(f + 1) * K], ref, "frame %d" % f)
                assert int(ref[:, :, 0].sum()) > 0
        be.close()


# ---- width discipline -----------------------------------------------------------------------------------------------------------

def test_one_face_over_a_whole_4k_frame(gpu_engine):
    """2160 x 3840, one face whose polygon covers the frame, on the 0 / 255 checkerboard: a workgroup's band is hundreds of pieces, the
    shape at which a per-thread 32-bit partial kept over a whole band overflows.  The per-label split is checked against the labels of
    the device's own pf_mask_faces (pinned to the restatement by tests/test_gpu_face_masks.py), so the numpy fill is not run here."""
    Hh, Ww = 2160, 3840
    kps = (ar.make_landmarks(80, 0, 600, 5, seed=6) * 24.0).astype(np.float32)[None]          # the `huge` case, scaled with the frame
    frame = sr.checkerboard(Hh, Ww)
    labels, owners, _, valid = gpu_engine.mask_faces(kps[None], Hh, Ww)
    assert valid.all() and (owners == 1).all()
    got, got_valid = gpu_engine.measure_faces(frame, kps[None], out=T.sentinel(1, 1, 8, 9))
    assert got_valid.all()
    s = got[0, 0]
    per_label = np.bincount(labels.reshape(-1), minlength=9)
    assert per_label[0] == 0 and (per_label[1:] > 0).sum() >= 2
    assert s[:, 0].astype(np.int64).tolist() == per_label[1:].tolist() and int(s[:, 0].sum()) == Hh * Ww
    assert sum(int(v) for v in s[:, 6]) == sr.checkerboard_lap2(Hh, Ww) == 2158 * 3838 * 1020 ** 2 + 2 * (2158 + 3838) * 765 ** 2 + 4 * 510 ** 2
    # a checkerboard pixel and its luma are 0 or 255: the other sums follow from the counts of the white pixels per label
    white = np.bincount(labels.reshape(-1), weights=(frame[:, :, 0] == 255).reshape(-1), minlength=9).astype(np.int64)[1:]
    for field, per_white in ((1, 255), (2, 255), (3, 255), (4, 255), (5, 255 * 255), (8, 1)):
        assert s[:, field].astype(np.int64).tolist() == (white * per_white).tolist(), field
    assert s[:, 7].astype(np.int64).tolist() == (per_label[1:] - white).tolist()


# ---- the Python classes ---------------------------------------------------------------------------------------------------------

def _check_results(engine, results, off_results, frame):
    """"stats" == measure_faces on the landmarks the dicts carry, "quality" == face_quality of it; boxes, landmarks and scores equal
    those with the option off."""
    from peppa_pig_face_landmark_amd.core.api.quality import face_quality
    assert len(results) == len(off_results)
    for r, r0 in zip(results, off_results):
        assert set(r) == set(r0) | {"stats", "quality"}
        for key in ("box", "kps", "scores"):
            assert np.array_equal(r[key], r0[key]), key
    if not results:
        return 0
    want, valid = engine.measure_faces(frame, np.stack([r["kps"] for r in results])[None])
    assert valid.all()
    measured = 0
    for i, r in enumerate(results):
        assert r["stats"].dtype == np.uint64
        T.assert_stats_equal(r["stats"], want[0, i], "result %d" % i)
        q = face_quality(want[0, i])
        assert set(r["quality"]) == set(q)
        for key in q:                                   # a face that owns no pixel (another face covers it) has NaN scores
            assert np.array_equal(r["quality"][key], q[key], equal_nan=True), key
        measured += int(q["pixels"] > 0)
    return measured


@pytest.mark.parametrize("which", ["faceana_host_tracking", "faceana_device_tracking", "stream_tracker", "frame_batch_runner"])
def test_classes_carry_stats(gpu_engine, hip_library, student_weights, detector_weights, which):
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.batch_runner import FrameBatchRunner
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker
    frames, rows, boxes = _scene(2, 4, seed=120)
    weights = {"detector": detector_weights, "keypoints": student_weights}
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["topk"] = 4
    cfg["Skps"]["Engine"]["device_tracking"] = which == "faceana_device_tracking"
    out, used, shots = {}, [], None
    for on in (None, True):
        ids = dict(track_ids=True, best_shots=True) if on and which != "frame_batch_runner" else {}
        if which.startswith("faceana"):
            fa = FaceAna(cfg=cfg, weights=weights, library=hip_library, face_stats=on, **ids)
            fa._planted_rows = lambda: rows[0]
            if which == "faceana_host_tracking":        # the planted boxes stand in for the synthetic detector's answer
                fa.face_detector = lambda image: np.concatenate([boxes, np.ones((len(boxes), 1), np.float32)], 1)
            out[bool(on)] = [fa.run(frames[0]) for _ in range(2)]          # a detector frame and a tracked one
            used = [frames[0], frames[0]]
            shots = fa.best_shots
            fa.engine.close()
        elif which == "stream_tracker":
            st = StreamTracker(cfg=cfg, weights=weights, max_streams=2, library=hip_library, face_stats=on, **ids)
            st._planted_rows = lambda sid, fr: rows[:len(sid)]
            r = st.run({0: frames[0], 1: frames[1]})
            out[bool(on)] = [r[0], r[1]]
            used = [frames[0], frames[1]]
            shots = st.best_shots
            st.close()
        else:
            fb = FrameBatchRunner(cfg=cfg, weights=weights, lanes=2, frames_per_lane=1, library=hip_library, face_stats=on)
            fb._planted_rows = lambda fr: rows[:len(fr)]
            out[bool(on)] = fb.run(frames)
            used = [frames[0], frames[1]]
            fb.close()
    faces = 0
    for i in range(2):
        off = [{k: v for k, v in r.items() if k not in ("id", "age")} for r in out[False][i]]
        on = [{k: v for k, v in r.items() if k not in ("id", "age")} for r in out[True][i]]
        faces += _check_results(gpu_engine, on, off, used[i])
    assert faces >= 1
    if which != "frame_batch_runner":
        assert shots is not None and len(shots.best) >= 1
        for (stream, ident), best in shots.best.items():
            assert best["id"] == ident and best["score"] > 0 and "stats" in best

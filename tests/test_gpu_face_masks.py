"""Face-region label maps on a real MI355X: the cases of tests/test_face_masks.py (the restatement byte for byte, overlap, dead slots,
chip space, device outputs through unaligned pointers, refusals) through the HIP library, the last-call accessor pf_face_masks after
every pipeline entry point (pf_landmarks, pf_run_frames with host, device and resident frames, pf_track_frame, pf_track_streams,
pf_batch_run_frames with front mode on and off) against pf_mask_faces on what those calls returned, and the Python classes."""
import numpy as np
import pytest
import torch

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
from tests import mask_ref as mr
from tests import test_face_masks as T

pytestmark = pytest.mark.gpu

S = 32
H, W = 1080, 1920
# the tracking tests plant small faces, as tests/test_gpu_align_faces.py does: the chip-space fits of the tracked frame stay valid
SMALL = dict(face_w=48, face_h=62)
TRACK = dict(score_thres=0.5, nms_iou_thres=0.3, min_face=1600.0, track_iou_thres=0.5, smooth_box=0.3, diff_thres=5.0)


def _dev_bytes(n, fill):
    t = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    return t.data_ptr(), lambda: t.cpu().numpy()


@pytest.mark.parametrize("case", mr.CASES, ids=mr.CASE_IDS)
def test_restatement(gpu_engine, case):
    T.check_restatement(gpu_engine, case)


def test_overlap_and_order(gpu_engine):
    T.check_overlap(gpu_engine)


def test_dead_slots(gpu_engine):
    T.check_dead_slots(gpu_engine)


@pytest.mark.parametrize("case", T.CHIP_CASES, ids=lambda c: c[0])
def test_chip_space(gpu_engine, case):
    T.check_chip_space(gpu_engine, case)


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
    frames, rows = [], []
    for f in range(F):
        frame, boxes = make_frame(H, W, K, seed=seed + f, face_w=face_w, face_h=face_h)
        frames.append(frame)
        rows.append(plant_rows(boxes, (H, W), 15120, (384, 640), 24, seed=seed + f))
    return np.stack(frames), np.stack(rows)


def test_face_masks_after_landmarks_and_run_frames(gpu_engine, blobs):
    gpu_engine.load_program(0, blobs[0], 8)
    gpu_engine.load_program(1, blobs[1], 2)
    frame, boxes = make_frame(H, W, 3, seed=44)
    assert T.check_after_landmarks(gpu_engine, frame, boxes, S)[0].any()
    frames, rows = _scene(2, 4, seed=31)
    counts, got = T.check_after_run_frames(gpu_engine, frames, rows, 4, 1600.0, S)
    assert counts.tolist() == [4, 4] and got[0].any()
    # device-resident frames; the maps never read them, so they may be gone by the time the maps are asked for
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    gpu_engine.run_frames_device(d_frames.data_ptr(), 2, H, W, 0.5, 0.3, 1600.0, 4, d_planted=d_rows.data_ptr(), rows=rows.shape[1])
    gpu_engine.sync()
    del d_frames
    T.assert_maps_equal(gpu_engine.face_masks(8), got)


def test_face_masks_after_track_frame(gpu_engine, blobs):
    """Two frames: the second is tracked, its landmarks are the smoothed float64 ones."""
    K = 4
    gpu_engine.load_program(0, blobs[0], K)
    gpu_engine.load_program(1, blobs[1], 1)
    frames, rows = _scene(1, K, seed=71, **SMALL)
    for rep in range(2):
        boxes, kps, _, ran = gpu_engine.track_frame(frames[0], TRACK["score_thres"], TRACK["nms_iou_thres"], TRACK["min_face"], K,
                                                    TRACK["track_iou_thres"], TRACK["smooth_box"], TRACK["diff_thres"], rows[0])
        assert ran == (rep == 0) and len(boxes) == K and kps.dtype == np.float64
        got = T.check_accessor(gpu_engine, K, kps[None], None, H, W, S)
        assert got[3].all() and got[0].any(), rep


def test_face_masks_after_track_streams(gpu_engine, blobs):
    """Three streams, one of which sits out the second call; the ids are never the identity."""
    K = 2
    gpu_engine.load_program(0, blobs[0], 3 * K)
    gpu_engine.load_program(1, blobs[1], 3)
    gpu_engine.track_streams_config(3, K)
    frames, rows = _scene(3, K, seed=120, **SMALL)
    for ids in ([2, 0, 1], [1, 2]):
        res = gpu_engine.track_streams(ids, frames[ids], planted_rows=rows[ids], **TRACK)
        n = len(ids)
        kps = np.zeros((n, K, 98, 2), np.float64)
        counts = np.array([len(r[0]) for r in res], np.int32)
        for i, r in enumerate(res):
            kps[i, :counts[i]] = r[1]
        assert counts.tolist() == [K] * n
        got = T.check_accessor(gpu_engine, n * K, kps, counts, H, W, S)
        assert got[0].shape == (n, H, W) and all(got[0][i].any() for i in range(n)), ids


def test_face_masks_after_batch_run_frames(gpu_engine, blobs, hip_library):
    """pf_batch_run_frames with 2 lanes, front mode on (device-resident frames) and off: pf_batch_face_masks gathers the lanes' maps."""
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
            be.face_masks(0, 100)
        with pytest.raises(_native.PeppaHipError, match="left face rows"):
            be.face_masks(1)
        for device_path in (True, False):
            if device_path:
                d_counts = torch.zeros(F, dtype=torch.int32, device="cuda")
                d_kps = torch.zeros((F, K, 98, 2), dtype=torch.float32, device="cuda")
                be.run_frames_device(d_frames.data_ptr(), F, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(),
                                     rows=rows.shape[1], d_counts=d_counts.data_ptr(), d_kps=d_kps.data_ptr())
                d_lab = torch.full((F, H, W), 0xAB, dtype=torch.uint8, device="cuda")
                d_own = torch.full((F, H, W), 0xAB, dtype=torch.uint8, device="cuda")
                d_box = torch.zeros((F * K, 4), dtype=torch.int32, device="cuda")
                d_valid = torch.zeros((F * K,), dtype=torch.int32, device="cuda")
                be.face_masks_device(F * K, 0, d_lab.data_ptr(), d_own.data_ptr(), d_box.data_ptr(), d_valid.data_ptr())
                d_map = torch.zeros((F * K, S, S), dtype=torch.uint8, device="cuda")
                d_valid_c = torch.zeros((F * K,), dtype=torch.int32, device="cuda")
                be.face_masks_device(F * K, S, d_map.data_ptr(), d_valid=d_valid_c.data_ptr())
                be.sync()
                counts, kps = d_counts.cpu().numpy(), d_kps.cpu().numpy()
                got = (d_lab.cpu().numpy(), d_own.cpu().numpy(), d_box.cpu().numpy(), d_valid.cpu().numpy().astype(bool))
                got_c = (d_map.cpu().numpy(), None, None, d_valid_c.cpu().numpy().astype(bool))
            else:
                counts, _, kps, _ = be.run_frames(frames, 0.5, 0.3, 1600.0, K, planted_rows=rows)
                got, got_c = be.face_masks(F * K), be.face_masks(F * K, S)
            assert counts.tolist() == [K] * F
            T.assert_maps_equal(got, gpu_engine.mask_faces(kps, H, W, counts=counts))
            T.assert_maps_equal(got_c, gpu_engine.mask_faces(kps, counts=counts, chip_size=S))
            assert all(got[0][f].any() for f in range(F))
        be.close()


# ---- the Python classes ---------------------------------------------------------------------------------------------------------

def _check_results(results, off_results, label_map, owner_map):
    """Every face: the keys are present iff the slot is valid and its box is not empty; "mask" == the restatement's labels cropped to
    the restatement's box with other faces' pixels zeroed; boxes, landmarks and scores equal those with the option off; the maps the
    object keeps are the restatement's."""
    assert len(results) == len(off_results) and results
    labels, owners, boxes, valid = mr.frame_maps(np.stack([r["kps"] for r in results]), None, H, W)
    assert np.array_equal(label_map, labels) and np.array_equal(owner_map, owners)
    n_masks = 0
    for i, (r, r0) in enumerate(zip(results, off_results)):
        for key in ("box", "kps", "scores"):
            assert np.array_equal(r[key], r0[key]), key
        assert "mask" not in r0 and "mask_box" not in r0
        x0, y0, x1, y1 = boxes[i]
        has = bool(valid[i]) and x1 > x0 and y1 > y0
        assert ("mask" in r) == has and ("mask_box" in r) == has
        if has:
            n_masks += 1
            assert r["mask_box"].dtype == np.int32 and r["mask_box"].tolist() == [x0, y0, x1, y1] and r["mask"].dtype == np.uint8
            assert np.array_equal(r["mask"], np.where(owners[y0:y1, x0:x1] == i + 1, labels[y0:y1, x0:x1], 0))
    return n_masks


@pytest.mark.parametrize("which", ["faceana_host_tracking", "faceana_device_tracking", "stream_tracker", "frame_batch_runner"])
def test_classes_carry_masks(hip_library, student_weights, detector_weights, which):
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.batch_runner import FrameBatchRunner
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker
    frames, rows = _scene(2, 4, seed=120)
    boxes = make_frame(H, W, 4, seed=120)[1]
    weights = {"detector": detector_weights, "keypoints": student_weights}
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["topk"] = 4
    cfg["Skps"]["Engine"]["device_tracking"] = which == "faceana_device_tracking"
    out, maps = {}, {}
    for on in (False, True):
        if which.startswith("faceana"):
            fa = FaceAna(cfg=cfg, weights=weights, library=hip_library, face_masks=on)
            fa._planted_rows = lambda: rows[0]
            if which == "faceana_host_tracking":        # the planted boxes stand in for the synthetic detector's answer
                fa.face_detector = lambda image: np.concatenate([boxes, np.ones((len(boxes), 1), np.float32)], 1)
            out[on], maps[on] = [], []
            for _ in range(2):                          # a detector frame and a tracked one
                out[on].append(fa.run(frames[0]))
                maps[on].append((fa.last_label_map, fa.last_owner_map))
            fa.engine.close()
        elif which == "stream_tracker":
            st = StreamTracker(cfg=cfg, weights=weights, max_streams=2, library=hip_library, face_masks=on)
            st._planted_rows = lambda ids, fr: rows[:len(ids)]
            r = st.run({0: frames[0], 1: frames[1]})
            out[on] = [r[0], r[1]]
            maps[on] = [(st.last_label_maps.get(s), st.last_owner_maps.get(s)) for s in (0, 1)]
            st.close()
        else:
            fb = FrameBatchRunner(cfg=cfg, weights=weights, lanes=2, frames_per_lane=1, library=hip_library, face_masks=on)
            fb._planted_rows = lambda fr: rows[:len(fr)]
            out[on] = fb.run(frames)
            maps[on] = [(fb.last_label_maps[f], fb.last_owner_maps[f]) for f in range(2)] if on else [(None, None)] * 2
            fb.close()
    n_masks = 0
    for i in range(2):
        assert maps[False][i] == (None, None)
        n_masks += _check_results(out[True][i], out[False][i], *maps[True][i])
    assert n_masks >= 1

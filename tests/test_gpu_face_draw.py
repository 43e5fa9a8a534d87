"""Face overlay on a real MI355X: the cases of tests/test_face_draw.py (the restatement byte for byte, hand-derived counts, small
frames, a strided frame, unaligned device pointers, priority, scores, dead slots, refusals, repeatability) through the HIP library, the
last-call accessor pf_face_draw after every pipeline entry point (pf_landmarks, pf_run_frames with host, device and resident frames,
pf_track_frame, pf_track_streams, pf_batch_run_frames with front mode on and off) against pf_draw_faces on what those calls returned
and against the restatement, redact -> draw through ``base``, the JPEG of the drawn device buffer, and the Python classes.  Frames are
uniform random bytes throughout: the faces come from planted detector rows."""
import numpy as np
import pytest
import torch

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
from tests import draw_ref as dr
from tests import mask_ref as mr
from tests import redact_ref as rr
from tests import test_face_draw as T

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


def test_hand_pins(gpu_engine):
    T.check_hand_pins(gpu_engine)


def test_small_frames(gpu_engine):
    T.check_small_frames(gpu_engine)


def test_device_outputs_and_unaligned_pointers(gpu_engine):
    T.check_device_outputs(gpu_engine, _dev_bytes, gpu_engine.sync)


def test_priority_and_overlap(gpu_engine):
    T.check_priority(gpu_engine)


def test_scores(gpu_engine):
    T.check_scores(gpu_engine)


def test_dead_slots(gpu_engine):
    T.check_dead_slots(gpu_engine)


def test_rejections(gpu_engine, student_weights):
    T.check_rejections(gpu_engine, student_weights)


def test_repeatability(gpu_engine):
    T.check_repeatability(gpu_engine)


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


def test_face_draw_after_landmarks_and_run_frames(gpu_engine, blobs):
    gpu_engine.load_program(0, blobs[0], 8)
    gpu_engine.load_program(1, blobs[1], 2)
    frames, rows, boxes = _scene(2, 3, seed=44)
    T.check_after_landmarks(gpu_engine, frames[0], boxes)
    T.check_row_stride(gpu_engine, _dev_bytes)
    counts, kps, scores, outs = T.check_after_run_frames(gpu_engine, frames, rows, 3, 1600.0)
    assert counts.tolist() == [3, 3]
    # device-resident frames: the overlay reads them again, so they stay alive; the output goes to device memory
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    gpu_engine.run_frames_device(d_frames.data_ptr(), 2, H, W, 0.5, 0.3, 1600.0, 3, d_planted=d_rows.data_ptr(), rows=rows.shape[1])
    for i, st in enumerate(T.ACCESSOR_STYLES):
        d_out = torch.full((2, H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
        d_valid = torch.zeros((6,), dtype=torch.int32, device="cuda")
        gpu_engine.face_draw_device(6, d_out.data_ptr(), scores=scores.reshape(-1, 98), d_valid=d_valid.data_ptr(), **st, **T.STYLE)
        gpu_engine.sync()
        T.assert_frames_equal(d_out.cpu().numpy(), outs[i], str(st))
        assert d_valid.cpu().numpy().all()
    # base given: pf_face_redact to the device, then pf_face_draw over it == the restatement applied to the redaction's restatement
    d_red = torch.full((2, H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    gpu_engine.face_redact_device(6, d_red.data_ptr(), mode="mosaic", labels=0x1FE, strength=16)
    st = T.ACCESSOR_STYLES[1]
    got, _ = gpu_engine.face_draw(6, scores=scores.reshape(-1, 98), base=d_red.data_ptr(), **st, **T.STYLE)
    red = np.stack([rr.frame_reference(frames[f], kps[f], counts[f], None, rr.MOSAIC, 0x1FE, 16)[0] for f in range(2)])
    T.assert_frames_equal(d_red.cpu().numpy(), red, "redaction")
    T.assert_frames_equal(got, T._scene_reference(red, kps, counts, scores, 7, 3, 2, 128), "redact -> draw")
    assert (got != outs[1]).any()
    with pytest.raises(_native.PeppaHipError, match="pf_face_draw: base must not alias out"):
        gpu_engine.face_draw_device(6, d_red.data_ptr(), d_base=d_red.data_ptr(), **st)
    # pf_encode_jpeg of the drawn device buffer == the encoding of its host copy
    d_out = torch.full((2, H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    gpu_engine.face_draw_device(6, d_out.data_ptr(), scores=scores.reshape(-1, 98), **st, **T.STYLE)
    files = gpu_engine.encode_jpeg((d_out.data_ptr(), 2, H, W), quality=90)
    assert files == gpu_engine.encode_jpeg(d_out.cpu().numpy(), quality=90) and all(f[:2] == b"\xff\xd8" for f in files)
    # the resident frame of pf_set_frame (PF_MEM_RESIDENT)
    gpu_engine.set_frame(frames[1])
    c1, k1, s1 = np.zeros((1,), np.int32), np.zeros((1, 3, 98, 2), np.float32), np.zeros((1, 3, 98), np.float32)
    pr = np.ascontiguousarray(rows[1], np.float32)
    rc = gpu_engine.lib.pf_run_frames_planted(gpu_engine.h, _native._ptr(frames[1]), _native.PF_MEM_RESIDENT, 1, H, W, _native._ptr(pr), pr.shape[0], 0.5, 0.3,
                                              1600.0, 3, _native._ptr(c1), None, _native._ptr(k1), _native._ptr(s1), _native.PF_MEM_HOST)
    gpu_engine._check(rc, "pf_run_frames_planted")
    assert c1.tolist() == [3]
    T.check_accessor(gpu_engine, 3, frames[1:2], k1, c1, s1)


def test_face_draw_after_track_frame(gpu_engine, blobs):
    """Two calls on one frame: the second is tracked, its landmarks are the smoothed float64 ones."""
    K = 4
    gpu_engine.load_program(0, blobs[0], K)
    gpu_engine.load_program(1, blobs[1], 1)
    frames, rows, _ = _scene(1, K, seed=71, **SMALL)
    for rep in range(2):
        boxes, kps, scores, ran = gpu_engine.track_frame(frames[0], TRACK["score_thres"], TRACK["nms_iou_thres"], TRACK["min_face"], K,
                                                         TRACK["track_iou_thres"], TRACK["smooth_box"], TRACK["diff_thres"], rows[0])
        assert ran == (rep == 0) and len(boxes) >= 1 and kps.dtype == np.float64
        outs = T.check_accessor(gpu_engine, len(boxes), frames, kps[None], None, np.asarray(scores, np.float32)[None])
        # tracked landmarks of noise may all lie outside the frame while their contours still cross it
        assert any((o != frames).any() for o in outs), (rep, float(kps.min()), float(kps.max()))


def test_face_draw_after_track_streams(gpu_engine, blobs):
    """Three streams, one of which sits out the second call; the ids are never the identity."""
    K = 2
    gpu_engine.load_program(0, blobs[0], 3 * K)
    gpu_engine.load_program(1, blobs[1], 3)
    gpu_engine.track_streams_config(3, K)
    frames, rows, _ = _scene(3, K, seed=120, **SMALL)
    for ids in ([2, 0, 1], [1, 2]):
        res = gpu_engine.track_streams(ids, frames[ids], planted_rows=rows[ids], **TRACK)
        n = len(ids)
        kps, scores = np.zeros((n, K, 98, 2), np.float64), np.zeros((n, K, 98), np.float32)
        counts = np.array([len(r[0]) for r in res], np.int32)
        for i, r in enumerate(res):
            kps[i, :counts[i]] = r[1]
            scores[i, :counts[i]] = r[2]
        assert counts.sum() >= 1
        outs = T.check_accessor(gpu_engine, n * K, frames[ids], kps, counts, scores)
        assert outs[0].shape == (n, H, W, 3) and any((o != frames[ids]).any() for o in outs), ids


def test_face_draw_after_batch_run_frames(gpu_engine, blobs, hip_library):
    """pf_batch_run_frames with 2 lanes, front mode on (device-resident frames) and off: pf_batch_face_draw gathers the lanes' frames."""
    F, K = 3, 2
    frames, rows, _ = _scene(F, K, seed=90)
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    st = dict(T.ACCESSOR_STYLES[1], **T.STYLE)
    for front in (1, 0):
        be = _native.BatchEngine(0, 2, hip_library)
        be.set_option(_native.PF_OPT_BATCH_FRONT, front)
        be.load_program(0, blobs[0], 2 * K)
        be.load_program(1, blobs[1], F if front else 2)
        with pytest.raises(_native.PeppaHipError, match="pf_batch_face_draw.*line_width"):
            be.face_draw_device(0, 1, line_width=0)
        with pytest.raises(_native.PeppaHipError, match="left face rows"):
            be.face_draw_device(1, 1)
        for device_path in (True, False):
            if device_path:
                d_counts = torch.zeros(F, dtype=torch.int32, device="cuda")
                d_kps = torch.zeros((F, K, 98, 2), dtype=torch.float32, device="cuda")
                d_scores = torch.zeros((F, K, 98), dtype=torch.float32, device="cuda")
                be.run_frames_device(d_frames.data_ptr(), F, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(),
                                     rows=rows.shape[1], d_counts=d_counts.data_ptr(), d_kps=d_kps.data_ptr(), d_scores=d_scores.data_ptr())
                be.sync()
                counts, kps, scores = d_counts.cpu().numpy(), d_kps.cpu().numpy(), d_scores.cpu().numpy()
                d_out = torch.full((F, H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
                d_valid = torch.zeros((F * K,), dtype=torch.int32, device="cuda")
                be.face_draw_device(F * K, d_out.data_ptr(), scores=scores.reshape(-1, 98), d_valid=d_valid.data_ptr(), **st)
                be.sync()
                got, valid = d_out.cpu().numpy(), d_valid.cpu().numpy().astype(bool)
            else:
                counts, _, kps, scores = be.run_frames(frames, 0.5, 0.3, 1600.0, K, planted_rows=rows)
                got, valid = be.face_draw(F * K, scores=scores.reshape(-1, 98), **st)
            assert counts.tolist() == [K] * F
            want, want_valid = gpu_engine.draw_faces(frames, kps, counts=counts, scores=scores, **st)
            T.assert_frames_equal(got, want, "front %d device %d" % (front, device_path))
            assert np.array_equal(valid, want_valid.reshape(-1))
            T.assert_frames_equal(got, T._scene_reference(frames, kps, counts, scores, 7, 3, 2, 128), "restatement")
            assert all((got[f] != frames[f]).any() for f in range(F))
        # base and out are offset per lane: a base of other frames, drawn over by both lanes
        other = T.random_frame(H, W, seed=91, F=F)
        d_other = torch.from_numpy(other).cuda()
        got, _ = be.face_draw(F * K, scores=scores.reshape(-1, 98), base=d_other.data_ptr(), **st)
        T.assert_frames_equal(got, T._scene_reference(other, kps, counts, scores, 7, 3, 2, 128), "base, front %d" % front)
        be.close()


# ---- the Python classes ---------------------------------------------------------------------------------------------------------

DRAW = {"what": ("points", "contours", "box"), "point_radius": 3, "line_width": 2, "alpha": 200}
REDACT = {"mode": "mosaic", "labels": 0x3FE, "strength": 16, "pad": 6}


def _jpeg_size(data):
    """(height, width) from the SOF0 segment of a baseline JPEG file"""
    i = 2
    while i + 9 < len(data):
        assert data[i] == 0xFF
        marker, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if marker == 0xC0:
            return int.from_bytes(data[i + 5:i + 7], "big"), int.from_bytes(data[i + 7:i + 9], "big")
        i += 2 + n
    raise AssertionError("no SOF0")


def _check_results(results, off_results, frame, drawn, file, redacted_base):
    """last_drawn == the restatement on the landmarks and scores the dicts carry (over the redaction's restatement where the base is
    the redaction); boxes, landmarks and scores equal those with the option off; the file is a JPEG of the frame's size."""
    assert len(results) == len(off_results)
    for r, r0 in zip(results, off_results):
        assert set(r) == set(r0)
        for key in ("box", "kps", "scores"):
            assert np.array_equal(r[key], r0[key]), key
    assert drawn.dtype == np.uint8 and drawn.shape == frame.shape
    assert file[:2] == b"\xff\xd8" and file[-2:] == b"\xff\xd9" and _jpeg_size(file) == frame.shape[:2]
    if not results:
        assert np.array_equal(drawn, frame)
        return 0
    kps, scores = np.stack([r["kps"] for r in results]), np.stack([r["scores"] for r in results])
    under = frame
    if redacted_base:
        under = rr.frame_reference(frame, kps, None, None, rr.MOSAIC, REDACT["labels"], REDACT["strength"], REDACT["pad"])[0]
    want = dr.frame_reference(under, kps, None, scores, 7, DRAW["point_radius"], DRAW["line_width"], DRAW["alpha"])[0]
    T.assert_frames_equal(drawn, want, "last_drawn")
    return int((drawn != frame).any())


@pytest.mark.parametrize("which", ["faceana_host_tracking", "faceana_device_tracking", "stream_tracker", "frame_batch_runner"])
def test_classes_keep_drawn_frames(hip_library, student_weights, detector_weights, which):
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.batch_runner import FrameBatchRunner
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker
    frames, rows, boxes = _scene(2, 4, seed=120)
    weights = {"detector": detector_weights, "keypoints": student_weights}
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["topk"] = 4
    cfg["Skps"]["Engine"]["device_tracking"] = which == "faceana_device_tracking"
    with pytest.raises(ValueError, match="redact"):
        FaceAna(cfg=cfg, weights=weights, library=hip_library, draw=dict(DRAW, base="redacted"))
    redacted_base = which in ("faceana_host_tracking", "stream_tracker")          # both bases in both kinds of call
    on_opts = dict(draw=dict(DRAW, base="redacted"), redact=REDACT, jpeg=90) if redacted_base else dict(draw=DRAW, jpeg=90)
    out, kept, files, logs, used = {}, {}, {}, {}, []
    for on in (False, True):
        opts = on_opts if on else {}
        if which.startswith("faceana"):
            fa = FaceAna(cfg=cfg, weights=weights, library=hip_library, **opts)
            fa._planted_rows = lambda: rows[0]
            if which == "faceana_host_tracking":        # the planted boxes stand in for the synthetic detector's answer
                fa.face_detector = lambda image: np.concatenate([boxes, np.ones((len(boxes), 1), np.float32)], 1)
            fa.engine.profile_enable(True)
            out[on], kept[on], files[on] = [], [], []
            for _ in range(2):                          # a detector frame and a tracked one
                out[on].append(fa.run(frames[0]))
                kept[on].append(fa.last_drawn)
                files[on].append(fa.last_drawn_jpeg)
            logs[on] = fa.engine.launch_log()
            used = [frames[0], frames[0]]
            fa.engine.close()
        elif which == "stream_tracker":
            st = StreamTracker(cfg=cfg, weights=weights, max_streams=2, library=hip_library, **opts)
            st._planted_rows = lambda ids, fr: rows[:len(ids)]
            st.engine.profile_enable(True)
            r = st.run({0: frames[0], 1: frames[1]})
            out[on] = [r[0], r[1]]
            kept[on] = [st.last_drawn[s] for s in (0, 1)] if on else [st.last_drawn] * 2
            files[on] = [st.last_drawn_jpeg[s] for s in (0, 1)] if on else [st.last_drawn_jpeg] * 2
            logs[on] = st.engine.launch_log()
            used = [frames[0], frames[1]]
            st.close()
        else:
            fb = FrameBatchRunner(cfg=cfg, weights=weights, lanes=2, frames_per_lane=1, library=hip_library, **opts)
            fb._planted_rows = lambda fr: rows[:len(fr)]
            fb.engine.lane(0).profile_enable(True)
            out[on] = fb.run(frames)
            kept[on] = [fb.last_drawn[f] for f in range(2)] if on else [fb.last_drawn] * 2
            files[on] = [fb.last_drawn_jpeg[f] for f in range(2)] if on else [fb.last_drawn_jpeg] * 2
            logs[on] = fb.engine.lane(0).launch_log()
            used = [frames[0], frames[1]]
            fb.close()
    assert not any("draw_" in k for k in logs[False]) and any("draw_kernel" in k for k in logs[True])
    changed = 0
    for i in range(2):
        assert kept[False][i] is None and files[False][i] is None
        changed += _check_results(out[True][i], out[False][i], used[i], kept[True][i], files[True][i], redacted_base)
    assert changed >= 1


def test_raw_false_drops_the_raw_copy(hip_library, student_weights, detector_weights):
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    frames, rows, _ = _scene(1, 2, seed=130)
    cfg = get_cfg()
    cfg["Skps"]["Engine"]["device_tracking"] = True
    fa = FaceAna(cfg=cfg, weights={"detector": detector_weights, "keypoints": student_weights}, library=hip_library, draw=DRAW,
                 jpeg={"quality": 85, "raw": False})
    fa._planted_rows = lambda: rows[0]
    assert len(fa.run(frames[0])) >= 1
    assert fa.last_drawn is None and _jpeg_size(fa.last_drawn_jpeg) == (H, W)
    fa.engine.close()

"""Face attributes (the landmark network's fc head, model.py:269,286-293) on a real MI355X: parity with the float64 restatement of
model.py:286-293 over the oracle's maps (tests/test_face_attrs.py), landmarks and scores unchanged by the head, run-to-run bit
identity, and the same rows through every entry point: pf_landmark_forward, pf_landmarks, pf_run_frames, pf_track_frame,
pf_track_streams and pf_batch_run_frames (2 and 3 lanes, front mode on and off), and the Python classes on top of them."""
import numpy as np
import pytest
import torch

from oracle import landmark_net as ln
from oracle import synth_weights as sw
from oracle import teacher_net as tn
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.graph.teacher import build_teacher_program
from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
from tests.test_face_attrs import FC_TAPS, _read, _shapes, fc_head_restatement, oracle_fc

pytestmark = pytest.mark.gpu


def oracle_fc_teacher(weights, crops):
    W = ln.to_torch(weights)
    x = torch.from_numpy(crops.astype(np.float32) / np.float32(255.0)).permute(0, 3, 1, 2).contiguous()
    taps = {}
    with torch.no_grad():
        tn.teacher_forward(W, x, taps)
    return fc_head_restatement(weights, [taps[n].float().permute(0, 2, 3, 1).numpy() for n in FC_TAPS])


CASES = [  # (name, builder, weights, size, dtype, batch, faces checked against the oracle, one_product, tolerance factor)
    ("student_f32s_256", "student", 256, "f32s", 384, 6, (), 2e-4),
    ("student_f32_128", "student", 128, "f32", 8, 8, (), 2e-4),
    ("teacher_f32s_256", "teacher", 256, "f32s", 32, 4, (), 2e-4),
    ("student_mix_256", "student", 256, "f32s", 64, 4, ("hero", "head"), 1e-3),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_face_attrs_parity_and_bit_identity(gpu_engine, student_weights, case):
    _, arch, size, dtype, B, n_ref, mix, tol = case
    w = student_weights if arch == "student" else sw.teacher_weights()
    build = build_student_program if arch == "student" else build_teacher_program
    crops = sw.smooth_blob_images(B, size, seed=600 + size)
    blob1, _ = build(w, size, dtype, one_product=mix, face_attrs=True)
    blob0, _ = build(w, size, dtype, one_product=mix)
    gpu_engine.load_program(0, blob1, B)
    loc1, score1, x1 = gpu_engine.landmark_forward(crops, attrs=True)
    loc1b, score1b, x1b = gpu_engine.landmark_forward(crops, attrs=True)
    assert np.array_equal(x1, x1b) and np.array_equal(loc1, loc1b) and np.array_equal(score1, score1b)
    gpu_engine.load_program(0, blob0, B)
    loc0, score0 = gpu_engine.landmark_forward(crops)
    assert np.array_equal(loc0, loc1) and np.array_equal(score0, score1)
    ref = (oracle_fc if arch == "student" else oracle_fc_teacher)(w, crops[:n_ref])
    err = np.abs(x1[:n_ref] - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))
    print("%s: raw fc output max rel err %.2e" % (case[0], err.max()))
    assert err.max() < tol, err
    # a face's record does not depend on the batch it ran in
    gpu_engine.load_program(0, blob1, B)
    _, _, xs = gpu_engine.landmark_forward(crops[:3], attrs=True)
    assert np.array_equal(xs, x1[:3])


def test_face_attrs_pools_match_engine_maps(gpu_engine, student_weights):
    """keep_all program: the head against the restatement over the engine's own decx4 / decx8 / aspp.out (pooling error alone)."""
    B = 4
    crops = sw.smooth_blob_images(B, 256, seed=17)
    blob, info = build_student_program(student_weights, 256, "f32s", keep_all=True, face_attrs=True)
    _shapes(blob, info)
    gpu_engine.load_program(0, blob, B)
    _, _, x = gpu_engine.landmark_forward(crops, attrs=True)
    own = fc_head_restatement(student_weights, [_read(gpu_engine, info, n, B) for n in FC_TAPS])
    assert np.abs(x - own).max() <= 1e-5 * max(1.0, float(np.abs(own).max()))


def test_entry_points_give_the_same_rows(gpu_engine, student_weights, detector_weights):
    """pf_run_frames ([F][top_k]) and pf_landmarks (box order) leave the rows that pf_landmark_forward + pf_face_attrs give on the crops
    pf_crop_faces makes from the same boxes, bit for bit; raw and cooked alike."""
    F, K = 2, 8
    blob, _ = build_student_program(student_weights, 256, "f32s", face_attrs=True)
    gpu_engine.load_program(0, blob, F * K)
    blob, _ = build_detector_program(detector_weights, (384, 640), "f32s")
    gpu_engine.load_program(1, blob, F)
    frames, rows_all = [], []
    for f in range(F):
        frame, boxes = make_frame(1080, 1920, K, seed=31 + f)
        frames.append(frame)
        rows_all.append(plant_rows(boxes, (1080, 1920), 15120, (384, 640), 24, seed=31 + f))
    counts, bout, _, _ = gpu_engine.run_frames(np.stack(frames), 0.5, 0.3, 1600.0, K, planted_rows=np.stack(rows_all))
    assert counts.tolist() == [K] * F
    raw_rf = gpu_engine.face_attrs(F * K, raw=True).reshape(F, K, 7)
    cooked_rf = gpu_engine.face_attrs(F * K).reshape(F, K, 7)
    for f in range(F):
        crops, _ = gpu_engine.crop_faces(frames[f], bout[f], 256)
        _, _, x = gpu_engine.landmark_forward(crops, attrs=True)
        cooked = gpu_engine.face_attrs(K)
        assert np.array_equal(x, raw_rf[f]) and np.array_equal(cooked, cooked_rf[f])
        _, _, valid = gpu_engine.landmarks(frames[f], bout[f])
        assert valid.all()
        assert np.array_equal(gpu_engine.face_attrs(K, raw=True), x)
    np.testing.assert_allclose(cooked_rf[..., :3], 90.0 * raw_rf[..., :3], rtol=1e-6)
    assert ((cooked_rf[..., 3:] >= 0) & (cooked_rf[..., 3:] <= 1)).all()      # sigmoid (saturates in f32 for the synthetic logits)


def test_face_analysis_api_keys(hip_library, student_weights, detector_weights):
    """FaceAna (device_tracking false) with the switch on: FaceLandmark returns the attribute rows of pf_landmarks, equal to
    pf_landmark_forward + pf_face_attrs on the crops of the same boxes, and every result dict gains float32 "pose" [3] and "attrs" [4];
    with the switch off the dicts keep exactly their three keys."""
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    frame, boxes = make_frame(1080, 1920, 3, seed=44)
    for on in (False, True):
        cfg = get_cfg()
        cfg["Skps"]["Engine"]["face_attributes"] = on
        fa = FaceAna(cfg=cfg, weights={"detector": detector_weights, "keypoints": student_weights}, library=hip_library)
        out = fa.face_landmark(frame, boxes)
        assert len(out) == (3 if on else 2)
        if on:
            crops, _ = fa.engine.crop_faces(frame, boxes, 256)
            _, _, x = fa.engine.landmark_forward(crops, attrs=True)
            assert np.array_equal(out[2], fa.engine.face_attrs(len(boxes)))
            np.testing.assert_allclose(out[2][:, :3], 90.0 * x[:, :3], rtol=1e-6)
        res = fa.to_dict(boxes, out[0], out[1], out[2] if on else None)
        res += fa.run(frame)
        for r in res:
            if on:
                assert set(r) == {"box", "kps", "scores", "pose", "attrs"}
                assert r["pose"].dtype == np.float32 and r["pose"].shape == (3,)
                assert r["attrs"].dtype == np.float32 and r["attrs"].shape == (4,)
                assert ((r["attrs"] >= 0) & (r["attrs"] <= 1)).all()
            else:
                assert set(r) == {"box", "kps", "scores"}


TRACK = dict(score_thres=0.5, nms_iou_thres=0.3, min_face=1600.0, track_iou_thres=0.5, smooth_box=0.3, diff_thres=5.0)


def _scene(F, K, seed):
    frames, rows = [], []
    for f in range(F):
        frame, boxes = make_frame(1080, 1920, K, seed=seed + f)
        frames.append(frame)
        rows.append(plant_rows(boxes, (1080, 1920), 15120, (384, 640), 24, seed=seed + f))
    return np.stack(frames), np.stack(rows)


def _engine_with_head(student_weights, detector_weights, faces, frames):
    from peppa_pig_face_landmark_amd import _native
    eng = _native.Engine(0)
    eng.load_program(0, build_student_program(student_weights, 256, "f32s", face_attrs=True)[0], faces)
    eng.load_program(1, build_detector_program(detector_weights, (384, 640), "f32s")[0], frames)
    return eng


def _reference_rows(eng, frames, rows, K):
    """pf_run_frames on the same frames and planted rows: per frame (count, scores [K][98], raw attrs [K][7])."""
    counts, _, _, scores = eng.run_frames(frames, 0.5, 0.3, 1600.0, K, planted_rows=rows)
    attrs = eng.face_attrs(frames.shape[0] * K, raw=True).reshape(frames.shape[0], K, 7)
    return counts, scores, attrs


def _match_by_scores(t_scores, t_attrs, r_count, r_scores, r_attrs):
    """Each tracked face is one of the frame's landmark rows: its scores are that row's bits, and so must its attributes be."""
    assert t_scores.shape[0] == t_attrs.shape[0] and t_scores.shape[0] > 0
    for i in range(t_scores.shape[0]):
        js = [j for j in range(int(r_count)) if np.array_equal(t_scores[i], r_scores[j])]
        assert len(js) == 1, ("tracked face %d matches %d landmark rows" % (i, len(js)))
        assert np.array_equal(t_attrs[i], r_attrs[js[0]]), i


def test_track_frame_and_track_streams_rows(student_weights, detector_weights):
    """pf_track_frame (rows [n_out]) and pf_track_streams (rows [n][top_k]) leave the attribute rows of their tracked faces,
    compacted like kps / scores: each equals, bit for bit, the row of pf_run_frames on the same frame whose scores it carries;
    over a detector frame and a tracked (repeated) frame."""
    K = 8
    frames, rows = _scene(2, K, seed=71)
    eng = _engine_with_head(student_weights, detector_weights, 2 * K, 2)
    r_count, r_scores, r_attrs = _reference_rows(eng, frames, rows, K)
    for rep in range(2):
        boxes, _, scores, ran = eng.track_frame(frames[0], TRACK["score_thres"], TRACK["nms_iou_thres"], TRACK["min_face"], K,
                                                TRACK["track_iou_thres"], TRACK["smooth_box"], TRACK["diff_thres"], rows[0])
        assert ran == (rep == 0)
        t_attrs = eng.face_attrs(len(boxes), raw=True)
        if rep == 0:
            _match_by_scores(scores, t_attrs, r_count[0], r_scores[0], r_attrs[0])
        else:
            assert t_attrs.shape[0] == len(boxes)
    eng.close()
    eng = _engine_with_head(student_weights, detector_weights, 2 * K, 2)
    eng.track_streams_config(2, K)
    for rep in range(2):
        res = eng.track_streams([1, 0], frames, planted_rows=rows, **TRACK)
        attrs = eng.face_attrs(2 * K, raw=True).reshape(2, K, 7)
        for i, (b, _, sc, ran) in enumerate(res):
            assert ran == (rep == 0)
            if rep == 0:
                _match_by_scores(sc, attrs[i, :len(b)], r_count[i], r_scores[i], r_attrs[i])
    eng.close()


@pytest.mark.parametrize("lanes", [2, 3])
def test_batch_run_frames_rows(student_weights, detector_weights, lanes):
    """pf_batch_run_frames, front mode on (device-resident frames) and off: pf_batch_face_attrs gathers [F][top_k] rows across the
    lanes equal, bit for bit, to one engine's pf_run_frames rows."""
    from peppa_pig_face_landmark_amd import _native
    F, K = 5, 8
    frames, rows = _scene(F, K, seed=90)
    one = _engine_with_head(student_weights, detector_weights, F * K, F)
    r_count, _, r_attrs = _reference_rows(one, frames, rows, K)
    one.close()
    per = (F + lanes - 1) // lanes
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    for front in (1, 0):
        be = _native.BatchEngine(0, lanes)
        be.set_option(_native.PF_OPT_BATCH_FRONT, front)
        be.load_program(0, build_student_program(student_weights, 256, "f32s", face_attrs=True)[0], per * K)
        be.load_program(1, build_detector_program(detector_weights, (384, 640), "f32s")[0], F if front else per)
        for device_path in (True, False):
            if device_path:
                d_counts = torch.zeros(F, dtype=torch.int32, device="cuda")
                be.run_frames_device(d_frames.data_ptr(), F, 1080, 1920, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(),
                                     rows=rows.shape[1], d_counts=d_counts.data_ptr())
                d_attrs = torch.zeros((F * K, 7), dtype=torch.float32, device="cuda")
                be.face_attrs_device(F * K, d_attrs.data_ptr(), raw=True)
                be.sync()
                counts, attrs = d_counts.cpu().numpy(), d_attrs.cpu().numpy().reshape(F, K, 7)
            else:
                counts = be.run_frames(frames, 0.5, 0.3, 1600.0, K, planted_rows=rows)[0]
                attrs = be.face_attrs(F * K, raw=True).reshape(F, K, 7)
            assert np.array_equal(counts, r_count)
            for f in range(F):
                n = int(r_count[f])
                assert np.array_equal(attrs[f, :n], r_attrs[f, :n]), (front, device_path, f)
        be.close()


def test_tracking_and_batch_classes_carry_attributes(hip_library, student_weights, detector_weights):
    """FaceAna with device_tracking true, StreamTracker and FrameBatchRunner: with the switch on every result dict has float32
    "pose" [3] and "attrs" [4] equal to the engine's rows; off, the dicts keep their keys."""
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.batch_runner import FrameBatchRunner
    from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    frames, rows = _scene(2, 4, seed=120)
    W = {"detector": detector_weights, "keypoints": student_weights}
    keys = {True: {"box", "kps", "scores", "pose", "attrs"}, False: {"box", "kps", "scores"}}
    for on in (False, True):
        cfg = get_cfg()
        cfg["Skps"]["Engine"]["device_tracking"] = True
        cfg["Skps"]["Detect"]["topk"] = 4
        fa = FaceAna(cfg=cfg, weights=W, library=hip_library, face_attributes=on)
        fa._planted_rows = lambda: rows[0]
        res = fa.run(frames[0])
        assert res and all(set(r) == keys[on] for r in res)
        if on:
            got = np.stack([np.concatenate([r["pose"], r["attrs"]]) for r in res])
            assert np.array_equal(got, fa.engine.face_attrs(len(res)))
            assert all(r["pose"].dtype == np.float32 and r["pose"].shape == (3,) and r["attrs"].shape == (4,) for r in res)
        st = StreamTracker(cfg=cfg, weights=W, max_streams=2, library=hip_library, face_attributes=on)
        st._planted_rows = lambda ids, fr: rows[:len(ids)]
        out = st.run({0: frames[0], 1: frames[1]})
        assert all(out[s] and all(set(r) == keys[on] for r in out[s]) for s in (0, 1))
        if on:
            a = st.engine.face_attrs(2 * 4).reshape(2, 4, 7)
            for i, s in enumerate((0, 1)):
                got = np.stack([np.concatenate([r["pose"], r["attrs"]]) for r in out[s]])
                assert np.array_equal(got, a[i, :len(out[s])])
        st.close()
        fb = FrameBatchRunner(cfg=cfg, weights=W, lanes=2, frames_per_lane=1, library=hip_library, face_attributes=on)
        counts, _, _, _ = fb.run_arrays(frames, planted_rows=rows)
        res_b = fb.run(frames)
        assert all(set(r) - {"det_box"} == keys[on] for fr in res_b for r in fr)

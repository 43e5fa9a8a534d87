"""The tracker at its decision edges (tests/tracking_video.py::video_edges): the gate at `diff == 5`, an area equal to
min_face, equal areas beyond top_k, two previous boxes / hulls above the IoU threshold, both branches of the One-Euro filter
inside one face, an empty track, a selected face the landmark stage rejects -- on 271 x 483 frames, whose byte count is no
multiple of 16, so pf_track_streams' gate takes its byte loop.  Expected values: the reference's own facer.py / lk.py from
source for the segments it runs (group A), the host facade plus hand-stated expectations for the one it raises on (group B);
both in tests/golden/tracking_video_edges.npz together with numpy-only evidence that every edge is hit.  Every test has an
emulator version (CPU tier) and a GPU twin; the device-pointer test runs on the GPU only."""
import numpy as np
import pytest

from oracle import prepost as pp
from oracle import ref_import as ri
from tests.test_track_streams import ARGS, TOP_K, _engine, _same, _schedule
from tests.test_tracking_parity import _make_facer_long, _PlantedDetector
from tests.tracking_video import GOLDEN_EDGES, HW_EDGES, S_LONG, long_video_weights, nms_boxes, scene, video_edges
from peppa_pig_face_landmark_amd.synth import plant_rows

N_FRAMES = 22
NBYTES = HW_EDGES[0] * HW_EDGES[1] * 3


def _iou(a, b):
    s = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])
    inter = max(0, min(a[2], b[2]) - max(a[0], b[0])) * max(0, min(a[3], b[3]) - max(a[1], b[1]))
    return float(inter / (s - inter))


def _hull(pts):
    return [np.min(pts[:, 0]), np.min(pts[:, 1]), np.max(pts[:, 0]), np.max(pts[:, 1])]


def _absdiff_sum(a, b):
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())


# ---- evidence that the edges are hit ---------------------------------------------------------------------------------------
def numpy_evidence(segs):
    """What can be said about the fixture without running anything but numpy: the exact difference sums, the areas NMS
    returns, the selection of the rejected-crop frame."""
    by = {s["name"]: s for s in segs}
    ev = {}
    fr = by["gate_equal"]["frames"]
    ev["gate_sums"] = np.asarray([_absdiff_sum(a, b) for a, b in zip(fr[:-1], fr[1:])], np.int64)
    b = nms_boxes(by["min_face_equal"]["rows"][0])
    ev["min_face_areas"] = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(np.float32)       # NMS order
    ev["min_face"] = np.float64(by["min_face_equal"]["min_face"])
    b = nms_boxes(by["equal_areas"]["rows"][0])
    ev["equal_areas_all"] = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(np.float32)
    e = by["empty"]
    ev["empty_rows_over_thres"] = np.asarray([int((r[:, 4] > ARGS["score_thres"]).sum()) for r in e["rows"]], np.int64)
    ev["empty_sums"] = np.asarray([_absdiff_sum(a, b) for a, b in zip(e["frames"][:-1], e["frames"][1:])], np.int64)
    r = by["rejected_crop"]
    sel = pp.sort_and_filter(nms_boxes(r["rows"][0])[:, :4], np.float32(r["min_face"]), TOP_K)
    ok = (sel[:, 2] - sel[:, 0] > 20) & (sel[:, 3] - sel[:, 1] > 20)            # FaceLandmark.min_face, face_landmark.py:76
    ev["reject_sel_wh"] = np.stack([sel[:, 2] - sel[:, 0], sel[:, 3] - sel[:, 1]], 1).astype(np.float32)
    ev["reject_n_sel"], ev["reject_n_valid"] = np.int64(len(sel)), np.int64(ok.sum())
    return ev


def reference_run_edges(student_weights, emu_library):
    """The reference's FaceAna (facer.py + lk.py from source, planted rows for the detector, the engine's f32 Student on the
    emulator for the landmark session -- see test_tracking_parity.reference_run_long) over the group-A segments.  Returns
    ({segment name: per-frame result lists}, {name: detector_ran}, evidence read off the reference's state with numpy: the
    competing IoUs of judge_boxs and GroupTrack, frozen / moving points of every smoothed face)."""
    from peppa_pig_face_landmark_amd._native import Engine
    from peppa_pig_face_landmark_amd.graph.student import build_student_program
    eng = Engine(0, emu_library)
    blob, _ = build_student_program(long_video_weights(student_weights), S_LONG, "f32")
    eng.load_program(0, blob, 1)
    state = {"rows": None, "det_calls": 0, "frame": 0}
    hull_iou, euro = [], []

    def det_model(x):
        state["det_calls"] += 1
        return [state["rows"][None]]

    def lmk_model(x):
        return eng.landmark_forward(np.ascontiguousarray(x, np.float32))

    ref = ri.reference_faceana(det_model, lmk_model, top_k=TOP_K, min_face=1600, kps_input=(S_LONG, S_LONG, 3))
    calculate = ref.trace.calculate

    def watched(img, now):                   # GroupTrack.calculate: note what it is about to decide, then let it
        prev = ref.trace.previous_landmarks_set
        if prev is not None and prev.shape[0] and len(now):
            scale = [img.shape[1], img.shape[0]]
            for i in range(now.shape[0]):
                ious = [_iou(_hull(now[i]), _hull(prev[j])) for j in range(prev.shape[0])]
                if len(ious) == 2:
                    hull_iou.append([state["frame"], i] + ious)
                hit = [j for j, v in enumerate(ious) if v > 0.5]
                if hit:
                    dx = np.sqrt(np.sum((now[i] / scale - prev[hit[0]] / scale) ** 2, axis=1))     # lk.py:125
                    euro.append([state["frame"], i, hit[0], int((dx < 0.002).sum()), int((dx >= 0.002).sum())])
        return calculate(img, now)

    ref.trace.calculate = watched
    out, ran, ev = {}, {}, {}
    try:
        for seg in video_edges():
            if seg["group"] != "A":
                state["frame"] += len(seg["frames"])
                continue
            ref.reset()
            ref.min_face = seg["min_face"]
            out[seg["name"]], ran[seg["name"]] = [], []
            for k, (fr, rw) in enumerate(zip(seg["frames"], seg["rows"])):
                state["rows"] = rw
                before = state["det_calls"]
                if seg["name"] == "iou_first" and k == 3:     # judge_boxs(track_box, detector boxes) is about to choose
                    now = nms_boxes(rw)
                    assert len(now) == 1
                    ev["iou_box"] = np.asarray([_iou(now[0], t) for t in ref.track_box], np.float64)
                out[seg["name"]].append([{kk: np.asarray(v) for kk, v in r.items()} for r in ref.run(fr.copy())])
                ran[seg["name"]].append(state["det_calls"] - before)
                state["frame"] += 1
    finally:
        eng.close()
    ev["hull_iou"] = np.asarray(hull_iou, np.float64).reshape(-1, 4)
    ev["euro"] = np.asarray(euro, np.int64).reshape(-1, 5)
    return out, ran, ev


def _facer(library, student_weights, detector_weights, device_tracking):
    return _make_facer_long(library, student_weights, detector_weights, device_tracking)


def facade_run_edges(library, student_weights, detector_weights, device_tracking, groups=("A", "B")):
    """FaceAna over the segments of the given groups: ({name: per-frame result lists}, {name: detector_ran})."""
    facer = _facer(library, student_weights, detector_weights, device_tracking)
    state = {"rows": None, "det_calls": 0}

    def rows_for():                              # host facade: the detector stage is asked for rows only when the gate opens
        state["det_calls"] += 1
        return state["rows"]

    track_frame = facer.engine.track_frame

    def watched(*a, **k):                        # device tracker: FaceAna.run() drops pf_track_frame's detector_ran
        r = track_frame(*a, **k)
        state["det_calls"] += int(r[3])
        return r

    facer.engine.track_frame = watched
    out, ran = {}, {}
    try:
        for seg in video_edges():
            if seg["group"] not in groups:
                continue
            facer.reset()
            facer.min_face = seg["min_face"]
            if facer.device_tracking:
                facer._planted_rows = lambda: state["rows"]
            else:
                facer.face_detector = _PlantedDetector(facer.engine, rows_for, seg["hw"])
            out[seg["name"]], ran[seg["name"]] = [], []
            for fr, rw in zip(seg["frames"], seg["rows"]):
                state["rows"] = rw
                before = state["det_calls"]
                res = facer.run(fr.copy())
                out[seg["name"]].append([{kk: np.asarray(v) for kk, v in d.items()} for d in res])
                ran[seg["name"]].append(state["det_calls"] - before)
    finally:
        facer.engine.close()
    return out, ran


def golden_edges():
    """({name: per-frame result lists}, {name: detector_ran}, the stored arrays) of the committed vector."""
    g = np.load(GOLDEN_EDGES)
    out, ran, i = {}, {}, 0
    for seg in video_edges():
        out[seg["name"]], ran[seg["name"]] = [], []
        for _ in seg["frames"]:
            out[seg["name"]].append([{"box": g["box"][i, j], "kps": g["kps"][i, j], "scores": g["scores"][i, j]}
                                     for j in range(int(g["counts"][i]))])
            ran[seg["name"]].append(int(g["detector_ran"][i]))
            i += 1
    assert i == N_FRAMES == len(g["counts"])
    return out, ran, g


# ---- comparisons -----------------------------------------------------------------------------------------------------------
def _close(ref, got, where, worst=None):
    """One frame against the golden one: the count and the row order exactly (a swapped or missing row is far outside the
    bounds), boxes and landmarks within 1e-3 of the crop width, scores within 1e-3 + 3e-4 max|score|
    (test_tracking_parity._compare_long)."""
    assert len(ref) == len(got), (where, len(ref), len(got))
    for a, b in zip(ref, got):
        bx = np.asarray(a["box"], np.float64)
        crop = 1.4 * (bx[2] - bx[0])                           # FaceLandmark.preprocess: the crop is 1.4 x the box width
        assert 40.0 < crop < 400.0, (where, crop)
        for key in ("box", "kps"):
            x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
            d = float(np.abs(x - y).max())
            if worst is not None:
                worst[key] = max(worst.get(key, 0.0), d / crop)
            assert d < 1e-3 * crop, (where, key, d, crop)
        sa, sb = np.asarray(a["scores"], np.float64), np.asarray(b["scores"], np.float64)
        d = float(np.abs(sa - sb).max())
        if worst is not None:
            worst["scores"] = max(worst.get("scores", 0.0), d / (1e-3 + 3e-4 * np.abs(sa).max()))
        assert d < 1e-3 + 3e-4 * np.abs(sa).max(), (where, "scores", d)


def _hand_stated(seg, results, ran, where):
    """What the segment's docstring promises, independent of any implementation: the counts, detector_ran, and which planted
    face every output row is (its track box is centred on that face, nearer to it than to any other)."""
    ex = seg["expect"]
    assert [len(r) for r in results] == ex["counts"], (where, [len(r) for r in results])
    assert [int(x) for x in ran] == ex["detector_ran"], (where, ran)
    for k, (res, faces, want) in enumerate(zip(results, seg["faces"], ex["row_face"])):
        centres = np.asarray([[cx, cy] for cx, cy, _, _ in faces], np.float64).reshape(-1, 2)
        for j, r in enumerate(res):
            bx = np.asarray(r["box"], np.float64)
            c = np.asarray([(bx[0] + bx[2]) / 2, (bx[1] + bx[3]) / 2])
            near = np.argsort(np.abs(centres - c).max(axis=1))
            if seg["name"] == "iou_first" and k < 3:
                continue          # the two faces are 19 px apart and their track boxes overlap: the count is what is stated
            assert int(near[0]) == want[j], (where, k, j, near.tolist(), want)


def test_edges_golden_hits_every_edge():
    """The fixture's own preconditions, from numpy and from what the generator read off the reference's state: all seven
    edges, none skipped."""
    segs = video_edges()
    assert sum(len(s["frames"]) for s in segs) == N_FRAMES and NBYTES % 16 == 7
    assert all(f.shape == HW_EDGES + (3,) and f.dtype == np.uint8 for s in segs for f in s["frames"])
    g = np.load(GOLDEN_EDGES)
    ev = numpy_evidence(segs)
    for k, v in ev.items():                                   # the stored evidence is what the fixture gives today
        assert np.array_equal(np.asarray(v), g["ev_" + k]), k
    # 1. the gate: mean difference exactly 5.0 (no detector), then one count above, then one below
    assert ev["gate_sums"].tolist() == [5 * NBYTES, 5 * NBYTES + 1, 5 * NBYTES - 1]
    assert 5 * NBYTES / HW_EDGES[0] / HW_EDGES[1] / 3.0 == 5.0
    # 2. min_face: the last NMS row has exactly that area, the one before it is one ulp larger
    a = ev["min_face_areas"]
    assert len(a) == 3 and np.float64(a[2]) == ev["min_face"] and a[1] == np.nextafter(a[2], np.float32(np.inf)) and a[0] > a[1]
    # 3. equal areas: rows 5 and 6 of seven are bit-equal, four rows are larger, one is smaller
    a = ev["equal_areas_all"]
    assert len(a) == 7 and a[5] == a[6] and int((a > a[5]).sum()) == 4 and int((a < a[5]).sum()) == 1 and a.min() > 1600
    # 4. two candidates above the IoU threshold, the better one second: track boxes (judge_boxs) and hulls (GroupTrack)
    ib = g["ev_iou_box"]
    assert ib.shape == (2,) and 0.5 < ib[0] < ib[1]
    hi = g["ev_hull_iou"]
    assert any(0.5 < r[2] < r[3] for r in hi), hi
    # 5. One-Euro: a smoothed face with frozen (dx < 0.002) and moving points at once
    eu = g["ev_euro"]
    assert any(r[3] > 0 and r[4] > 0 and r[3] + r[4] == 98 for r in eu), eu
    # 6. the rejected crop: five selected, the third of them 18 wide, four valid
    wh = ev["reject_sel_wh"]
    assert ev["reject_n_sel"] == 5 and ev["reject_n_valid"] == 4 and wh[2, 0] <= 20 < wh[2, 1] and (wh[[0, 1, 3, 4]] > 20).all()
    assert wh[2, 0] * wh[2, 1] > 1600
    # 7. the empty result: no row above the score threshold on three frames, the two repeats byte-identical, the frames around
    #    them different enough for the detector
    assert ev["empty_rows_over_thres"].tolist()[1:4] == [0, 0, 0] and ev["empty_rows_over_thres"][0] > 0 < ev["empty_rows_over_thres"][4]
    s = ev["empty_sums"]
    assert s[1] == s[2] == 0 and s[0] > 5 * NBYTES < s[3]
    # and what the golden says happened there
    gold, gran, _ = golden_edges()
    for seg in segs:
        _hand_stated(seg, gold[seg["name"]], gran[seg["name"]], seg["name"])


def test_edges_golden_is_what_the_reference_produces(student_weights, emu_library):
    gold, gran, g = golden_edges()
    if not ri.available():
        pytest.skip("reference checkout not present (GPU box): the vector was checked where it was generated")
    ref, ran, ev = reference_run_edges(student_weights, emu_library)
    for k, v in ev.items():
        assert np.array_equal(v, g["ev_" + k]), k
    for name, runs in ref.items():
        assert ran[name] == gran[name], name
        for r, q in zip(runs, gold[name]):
            assert len(r) == len(q), name
            for a, b in zip(r, q):
                for key in ("box", "kps", "scores"):
                    assert np.array_equal(np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)), (name, key)


# ---- 1. the facade against the golden --------------------------------------------------------------------------------------
def _facade_vs_golden(library, student_weights, detector_weights, device_tracking):
    gold, gran, _ = golden_edges()
    got, ran = facade_run_edges(library, student_weights, detector_weights, device_tracking)
    worst = {}
    for seg in video_edges():
        name = seg["name"]
        w = worst.setdefault(seg["group"], {})
        assert ran[name] == gran[name], (name, ran[name])
        for k, (r, q) in enumerate(zip(gold[name], got[name])):
            _close(r, q, (name, k), w)
        _hand_stated(seg, got[name], ran[name], name)
    print("worst deviation as a fraction of the bound", {grp: {k: round(v / (1e-3 if k != "scores" else 1.0), 4) for k, v in w.items()}
                                                         for grp, w in worst.items()})


@pytest.mark.parametrize("device_tracking", [False, True])
def test_edges_facade_matches_golden_emulator(emu_library, student_weights, detector_weights, device_tracking):
    _facade_vs_golden(emu_library, student_weights, detector_weights, device_tracking)


@pytest.mark.gpu
@pytest.mark.parametrize("device_tracking", [False, True])
def test_edges_facade_matches_golden_gpu(hip_library, student_weights, detector_weights, device_tracking):
    _facade_vs_golden(hip_library, student_weights, detector_weights, device_tracking)


# ---- 2. pf_track_streams: three staggered streams against the golden and against pf_track_frame --------------------------
def _args(seg):
    return dict(ARGS, min_face=seg["min_face"])


_STREAM_RUNS = {}


def _staggered(library, student_weights, detector_weights):
    """Three streams play the video: stream 0 from the first call, stream 1 one call later, stream 2 sits out the second call
    of every segment (in gate_equal: the call in which stream 0 meets `diff == 5`, so stream 2 meets it a call later, against
    ITS last frame).  A single-stream engine replays the video once -- every stream sees the same frames in the same order.
    Returns ({stream: {name: [result tuples]}}, {name: [result tuples]} of pf_track_frame); one run per library."""
    if library in _STREAM_RUNS:
        return _STREAM_RUNS[library]
    kw = long_video_weights(student_weights)
    plans = {0: (0, ()), 1: (1, ()), 2: (0, (1,))}
    multi = _engine(library, detector_weights, kw, len(plans))
    single = _engine(library, detector_weights, kw, 0)
    got = {s: {} for s in plans}
    alone = {}
    try:
        for seg in video_edges():
            frames, rows, name = seg["frames"], seg["rows"], seg["name"]
            multi.track_streams_reset(-1)
            when = {s: _schedule(len(frames), off, skip) for s, (off, skip) in plans.items()}
            for s in plans:
                got[s][name] = []
            for c in range(max(max(v) for v in when.values()) + 1):
                call = {s: when[s].index(c) for s in plans if c in when[s]}
                ids = sorted(call)
                out = multi.track_streams(ids, np.stack([frames[call[s]] for s in ids]),
                                          planted_rows=np.stack([rows[call[s]] for s in ids]), **_args(seg))
                for s, r in zip(ids, out):
                    got[s][name].append(r)
            single.track_reset()
            a = _args(seg)
            alone[name] = [single.track_frame(fr, a["score_thres"], a["nms_iou_thres"], a["min_face"], TOP_K, a["track_iou_thres"],
                                              a["smooth_box"], a["diff_thres"], rw) for fr, rw in zip(frames, rows)]
    finally:
        multi.close()
        single.close()
    _STREAM_RUNS[library] = (got, alone)
    return got, alone


def _streams_vs_golden(library, student_weights, detector_weights):
    gold, gran, _ = golden_edges()
    got, _ = _staggered(library, student_weights, detector_weights)
    for seg in video_edges():
        name = seg["name"]
        for s, runs in got.items():
            assert [int(r[3]) for r in runs[name]] == gran[name], (s, name)        # a gate against another stream's frame fails here
            res = [[{"box": b, "kps": k, "scores": sc} for b, k, sc in zip(*r[:3])] for r in runs[name]]
            for k, (r, q) in enumerate(zip(gold[name], res)):
                _close(r, q, (s, name, k))
            _hand_stated(seg, res, [r[3] for r in runs[name]], (s, name))


def _streams_vs_single(library, student_weights, detector_weights):
    got, alone = _staggered(library, student_weights, detector_weights)
    for s, runs in got.items():
        for name, seq in runs.items():
            assert len(seq) == len(alone[name])
            for k, (a, b) in enumerate(zip(seq, alone[name])):
                _same(a, b, (s, name, k))


def test_edges_streams_match_golden_emulator(emu_library, student_weights, detector_weights):
    _streams_vs_golden(emu_library, student_weights, detector_weights)


def test_edges_streams_equal_single_stream_emulator(emu_library, student_weights, detector_weights):
    _streams_vs_single(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_edges_streams_match_golden_gpu(hip_library, student_weights, detector_weights):
    _streams_vs_golden(hip_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_edges_streams_equal_single_stream_gpu(hip_library, student_weights, detector_weights):
    _streams_vs_single(hip_library, student_weights, detector_weights)


# ---- 3. GPU only: the stream frames by device pointer, 16-byte aligned and one byte off -----------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hw", [HW_EDGES, (272, 480)])
def test_edges_stream_frames_by_device_pointer_gpu(hip_library, student_weights, detector_weights, hw):
    """Host frames, a 16-byte-aligned device pointer and that pointer + 1 (vec == 0 through the pointer condition alone at
    272 x 480, whose bytes are a multiple of 16) give the same bits, call by call, with both gate outcomes."""
    import torch
    h, w = hw
    faces = [[(120, 100, 52, 68), (330, 150, 64, 84)], [(126, 100, 52, 68), (336, 150, 64, 84)]]
    fr = [scene(h, w, f, 81 + i) for i, f in enumerate(faces)]
    rows = [plant_rows(b, hw, 15120, (384, 640), 6, seed=470 + i) for i, (_, b) in enumerate(fr)]
    frames = [f for f, _ in fr]
    calls = [(0, 1), (0, 0), (1, 0), (1, 1)]                 # the frame each of the two streams sends: repeats close the gate
    kw = long_video_weights(student_weights)
    engines = [_engine(hip_library, detector_weights, kw, 2) for _ in range(3)]
    try:
        seen = []
        for c, pick in enumerate(calls):
            host = np.stack([frames[j] for j in pick])
            pr = np.stack([rows[j] for j in pick])
            a = engines[0].track_streams([0, 1], host, planted_rows=pr, **ARGS)
            outs = []
            for off, eng in ((0, engines[1]), (1, engines[2])):
                buf = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
                base = (-buf.data_ptr()) % 16 + off              # offset of the first frame byte inside the buffer
                buf[base:base + host.size].copy_(torch.from_numpy(host.reshape(-1)))
                torch.cuda.synchronize()
                assert (buf.data_ptr() + base) % 16 == off
                outs.append(eng.track_streams([0, 1], buf.data_ptr() + base, planted_rows=pr, shape=host.shape[:3], **ARGS))
            for s in range(2):
                _same(a[s], outs[0][s], ("aligned device pointer", c, s))
                _same(a[s], outs[1][s], ("device pointer + 1", c, s))
                assert len(a[s][0]) == 2
            seen += [r[3] for r in a]
        assert seen == [True, True, False, True, True, False, False, True]
    finally:
        for e in engines:
            e.close()


# ---- 4. the gate kernel alone: 2-frame calls at the smallest sizes ----------------------------------------------------------
def _second_frames(first, rng):
    """Three frames whose absolute difference to `first` sums to exactly 5 N, 5 N + 1 and 5 N - 1 (N bytes): every byte moves
    by 5 towards the middle of the range, then one byte by one more / one less."""
    step = np.where(first < 128, 5, -5).astype(np.int16)
    out = []
    for extra in (0, 1, -1):
        s = step.copy().reshape(-1)
        k = int(rng.integers(s.size))
        s[k] += extra * np.sign(s[k])
        out.append((first.astype(np.int16) + s.reshape(first.shape)).astype(np.uint8))
    return out


def _gate_at_equality(library, student_weights, detector_weights, hw):
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    first = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    second = _second_frames(first, rng)
    n = h * w * 3
    assert [_absdiff_sum(first, s) for s in second] == [5 * n, 5 * n + 1, 5 * n - 1]
    rows = plant_rows(np.zeros((0, 4), np.float32), hw, 15120, (384, 640), 6, seed=480)      # no row above the score threshold
    assert (rows[:, 4] < ARGS["score_thres"]).all()
    args = dict(ARGS, min_face=0.0)
    multi = _engine(library, detector_weights, long_video_weights(student_weights), 3)
    single = _engine(library, detector_weights, long_video_weights(student_weights), 0)
    try:
        pr = np.stack([rows] * 3)
        a = multi.track_streams([0, 1, 2], np.stack([first] * 3), planted_rows=pr, **args)
        assert [r[3] for r in a] == [True] * 3 and all(len(r[0]) == 0 for r in a)
        b = multi.track_streams([0, 1, 2], np.stack(second), planted_rows=pr, **args)
        assert [int(r[3]) for r in b] == [0, 1, 0] and all(len(r[0]) == 0 for r in b)
        for k, s in enumerate(second):                        # absdiff_sum_kernel decides the same
            single.track_reset()
            for fr, want in ((first, True), (s, k == 1)):
                r = single.track_frame(fr, args["score_thres"], args["nms_iou_thres"], args["min_face"], TOP_K, args["track_iou_thres"],
                                       args["smooth_box"], args["diff_thres"], rows)
                assert r[3] == want and len(r[0]) == 0, (k, want)
    finally:
        multi.close()
        single.close()


GATE_SIZES = [(1, 1), (5, 7), HW_EDGES, (272, 480)]


@pytest.mark.parametrize("hw", GATE_SIZES)
def test_gate_at_equality_emulator(emu_library, student_weights, detector_weights, hw):
    _gate_at_equality(emu_library, student_weights, detector_weights, hw)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", GATE_SIZES)
def test_gate_at_equality_gpu(hip_library, student_weights, detector_weights, hw):
    _gate_at_equality(hip_library, student_weights, detector_weights, hw)

"""N video streams on one handle (pf_track_streams / StreamTracker): per stream the answers of pf_track_frame on a handle of
its own.  Golden (the reference's own facer.py / lk.py on video_long) with staggered streams, bit-identity with single-stream
replays, state isolation and argument checks, the range guard.  Every test has an emulator (CPU tier) and a GPU twin; the
1080p scale test runs on the GPU only."""
import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from tests.test_range_guard import _scaled
from tests.test_tracking_parity import golden_run_long
from tests.tracking_video import S_LONG, long_video_weights, video, video_long

# Skps.yml: Detect score_thrs / iou_thrs / min_face, Trace iou_thres / smooth_box; diff_thres 5 (facer.py:40)
ARGS = dict(score_thres=0.5, nms_iou_thres=0.3, min_face=1600.0, track_iou_thres=0.5, smooth_box=0.3, diff_thres=5.0)
TOP_K = 5


def _engine(library, detector_weights, kps_weights, streams, top_k=TOP_K, size=S_LONG, lm_dtype="f32", det_dtype="f32"):
    """Engine with the 384 x 640 detector (its rows are replaced by planted ones) and the Student; streams == 0: a
    single-stream (pf_track_frame) engine."""
    eng = _native.Engine(0, library)
    n = max(streams, 1)
    eng.load_program(_native.PF_NET_DETECTOR, build_detector_program(detector_weights, (384, 640), det_dtype)[0], n)
    eng.load_program(_native.PF_NET_LANDMARK, build_student_program(kps_weights, size, lm_dtype)[0], n * top_k)
    if streams:
        eng.track_streams_config(streams, top_k)
    return eng


def _single(eng, frame, rows, top_k=TOP_K):
    return eng.track_frame(frame, ARGS["score_thres"], ARGS["nms_iou_thres"], ARGS["min_face"], top_k,
                           ARGS["track_iou_thres"], ARGS["smooth_box"], ARGS["diff_thres"], rows)


def _multi(eng, ids, frames, rows):
    return eng.track_streams(ids, np.stack(frames), planted_rows=np.stack(rows), **ARGS)


def _same(a, b, what=""):
    """bit-identical (boxes, kps, scores, detector_ran)"""
    assert a[3] == b[3], ("detector_ran", what)
    assert a[0].shape == b[0].shape, ("count", what, a[0].shape, b[0].shape)
    for k, name in enumerate(("box", "kps", "scores")):
        assert np.array_equal(a[k], b[k]), (name, what)


# ---- 1. golden, staggered --------------------------------------------------------------------------------------------------
def _schedule(length, offset, skip):
    """call index of each frame of a stream that starts at `offset` and sits out the calls in `skip`"""
    calls, c = [], offset
    while len(calls) < length:
        if c not in skip:
            calls.append(c)
        c += 1
    return calls


def _golden_staggered(library, student_weights, detector_weights):
    from Skps import StreamTracker
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    gold, gran = golden_run_long()
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["input_shape"] = [384, 640, 3]
    cfg["Skps"]["Keypoints"]["input_shape"] = [S_LONG, S_LONG, 3]
    cfg["Skps"]["Engine"]["dtype"] = "f32"
    tr = StreamTracker(cfg=cfg, weights={"detector": detector_weights, "keypoints": long_video_weights(student_weights)},
                       max_streams=3, library=library)
    # stream 0 from the first call, stream 2 one call later, stream 1 two calls later; stream 2 sits out two calls
    plans = {0: (0, ()), 1: (2, ()), 2: (1, (4, 5))}
    got = {s: [] for s in plans}
    try:
        for si, (frames, rows, hw) in enumerate(video_long()):
            if si:
                for s in plans:
                    tr.reset(s)                              # the stream restarts (here: a new frame size)
            when = {s: _schedule(len(frames), off, skip) for s, (off, skip) in plans.items()}
            last = max(max(c) for c in when.values())
            for c in range(last + 1):
                call = {s: when[s].index(c) for s in plans if c in when[s]}
                if not call:
                    continue
                tr._planted_rows = lambda ids, _b, call=call: np.stack([rows[call[s]] for s in ids])
                out = tr.run({s: frames[j].copy() for s, j in call.items()})
                for s in call:
                    got[s].append((out[s], tr.last_detector_ran[s]))
    finally:
        tr.close()
    for s, seq in got.items():
        assert [len(r) for r, _ in seq] == [len(g) for g in gold], s
        assert [int(ran) for _, ran in seq] == gran, s     # a gate against another stream's frame fails here
        for i, ((res, _), ref) in enumerate(zip(seq, gold)):
            for a, b in zip(ref, res):
                bx = np.asarray(a["box"], np.float64)
                crop = 1.4 * (bx[2] - bx[0])
                for key in ("box", "kps"):                   # the bounds of test_tracking_parity._compare_long
                    x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
                    assert np.abs(x - y).max() < 1e-3 * crop, (s, i, key)
                sa, sb = np.asarray(a["scores"], np.float64), np.asarray(b["scores"], np.float64)
                assert np.abs(sa - sb).max() < 1e-3 + 3e-4 * np.abs(sa).max(), (s, i)


def test_staggered_streams_match_golden_emulator(emu_library, student_weights, detector_weights):
    _golden_staggered(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_staggered_streams_match_golden_gpu(hip_library, student_weights, detector_weights):
    _golden_staggered(hip_library, student_weights, detector_weights)


# ---- 2. the same as N single-stream engines, bit for bit --------------------------------------------------------------------
def _orders(n):
    fwd = list(range(n))
    return [fwd, fwd[::-1], fwd[3:] + fwd[:3]]           # forward, reversed, shifted


def _replay_equal(library, student_weights, detector_weights, length):
    frames, rows, _ = video_long()[0]
    frames, rows = frames[:length], rows[:length]
    kw = long_video_weights(student_weights)
    orders = _orders(length)
    multi = _engine(library, detector_weights, kw, len(orders))
    single = _engine(library, detector_weights, kw, 0)
    try:
        got = [[] for _ in orders]
        for c in range(length):
            out = _multi(multi, list(range(len(orders))), [frames[o[c]] for o in orders], [rows[o[c]] for o in orders])
            for s in range(len(orders)):
                got[s].append(out[s])
        for s, order in enumerate(orders):
            single.track_reset()
            for c, j in enumerate(order):
                _same(got[s][c], _single(single, frames[j], rows[j]), (s, c))
        assert any(not r[3] for g in got for r in g) and any(r[3] for g in got for r in g)   # both gate outcomes seen
    finally:
        multi.close()
        single.close()


def test_streams_equal_single_stream_replay_emulator(emu_library, student_weights, detector_weights):
    _replay_equal(emu_library, student_weights, detector_weights, 7)


@pytest.mark.gpu
def test_streams_equal_single_stream_replay_gpu(hip_library, student_weights, detector_weights):
    _replay_equal(hip_library, student_weights, detector_weights, 10)


# ---- 3. state isolation and argument checks ---------------------------------------------------------------------------------
def _isolation(library, student_weights, detector_weights):
    (f, r, _), (f2, r2, _) = video_long()
    kw = long_video_weights(student_weights)
    eng = _engine(library, detector_weights, kw, 3)
    ref = _engine(library, detector_weights, kw, 3)          # the undisturbed run
    try:
        with pytest.raises(_native.PeppaHipError, match="track_streams_config"):
            fresh = _native.Engine(0, library)
            try:
                fresh.track_streams([0], f[0][None], **ARGS)
            finally:
                fresh.close()
        for e in (eng, ref):
            _multi(e, [0, 1], [f[0], f[3]], [r[0], r[3]])
        # rejected calls change nothing
        for ids, fr, msg in (([1, 1], [f[1], f[1]], "twice"), ([0, 3], [f[1], f[1]], "outside"),
                             ([-1], [f[1]], "outside"), ([0, 1, 2, 0], [f[1]] * 4, "max_streams")):
            with pytest.raises(_native.PeppaHipError, match=msg):
                _multi(eng, ids, fr, [r[1]] * len(ids))
        # stream 0 is reset, stream 1 sits this call out, stream 2 starts
        eng.track_streams_reset(0)
        a = _multi(eng, [0, 2], [f[3], f[0]], [r[3], r[0]])
        b = _multi(ref, [2], [f[0]], [r[0]])
        assert a[0][3]                                        # reset: no previous frame, the detector runs
        _same(a[1], b[0], "stream 2")
        # stream 1 gates against ITS last frame (f[3]), not the f[0] streams 0 / 2 saw since
        a = _multi(eng, [1], [f[3]], [r[3]])
        b = _multi(ref, [1], [f[3]], [r[3]])
        assert not a[0][3]
        _same(a[0], b[0], "stream 1 after sitting out")
        # a frame of another size counts as "no previous frame"
        a = _multi(eng, [1, 2], [f2[0], f2[0]], [r2[0], r2[0]])
        assert a[0][3] and a[1][3]
    finally:
        eng.close()
        ref.close()


def test_stream_state_isolation_and_arguments_emulator(emu_library, student_weights, detector_weights):
    _isolation(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_stream_state_isolation_and_arguments_gpu(hip_library, student_weights, detector_weights):
    _isolation(hip_library, student_weights, detector_weights)


# ---- 4. range guard ---------------------------------------------------------------------------------------------------------
def _range_guard(library, student_weights, detector_weights):
    from Skps import StreamTracker
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    frames, rows = video()
    w = _scaled(student_weights, 3.0e5)
    # engine level: the failing call names the landmark slot, resets its streams and keeps the others
    eng = _engine(library, detector_weights, w, 3, size=64)
    try:
        assert len(_multi(eng, [2], [frames[0]], [rows[0]])[0][0]) >= 2
        eng.load_program(_native.PF_NET_LANDMARK, build_student_program(w, 64, "f32s")[0], 3 * TOP_K)
        with pytest.raises(_native.PeppaHipError, match=r"program %d" % _native.PF_NET_LANDMARK):
            _multi(eng, [0, 1], [frames[0], frames[1]], [rows[0], rows[1]])
        eng.load_program(_native.PF_NET_LANDMARK, build_student_program(w, 64, "f32")[0], 3 * TOP_K)
        out = _multi(eng, [0, 1, 2], [frames[1]] * 3, [rows[1]] * 3)
        assert out[0][3] and out[1][3]                        # reset: no previous frame
        assert not out[2][3]                                  # kept its track and its frame (frames[1] == frames[0])
    finally:
        eng.close()

    # StreamTracker: reload the landmark network as f32, keep the detector f32s, answer like an f32 tracker
    def run(dtype):
        cfg = get_cfg()
        cfg["Skps"]["Detect"]["input_shape"] = [384, 640, 3]
        cfg["Skps"]["Keypoints"]["input_shape"] = [64, 64, 3]
        cfg["Skps"]["Engine"]["dtype"] = dtype
        tr = StreamTracker(cfg=cfg, weights={"detector": detector_weights, "keypoints": w}, max_streams=2, library=library)
        state = {"i": 0}
        tr._planted_rows = lambda ids, _b: np.stack([rows[state["i"]]] * len(ids))
        out = []
        try:
            for i in range(3):
                state["i"] = i
                out.append(tr.run({0: frames[i].copy(), 1: frames[i].copy()}))
            return out, tr.landmark.dtype, tr.detector.dtype
        finally:
            tr.close()

    want, _, _ = run("f32")
    got, lm_dtype, det_dtype = run("f32s")
    assert lm_dtype == "f32" and det_dtype == "f32s"
    for a, b in zip(want, got):
        for s in (0, 1):
            assert len(a[s]) == len(b[s]) >= 2
            for x, y in zip(a[s], b[s]):
                assert np.isfinite(y["box"]).all() and np.isfinite(y["kps"]).all()
                for key in ("box", "kps", "scores"):
                    assert np.array_equal(x[key], y[key]), key


def test_range_guard_resets_the_streams_of_the_call_emulator(emu_library, student_weights, detector_weights):
    _range_guard(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_range_guard_resets_the_streams_of_the_call_gpu(hip_library, student_weights, detector_weights):
    _range_guard(hip_library, student_weights, detector_weights)


# ---- 5. scale (GPU only): 32 streams x 4 calls of 1080p frames with 8 faces ------------------------------------------------
@pytest.mark.gpu
def test_32_streams_1080p_equal_single_stream_replay_gpu(hip_library, student_weights, detector_weights):
    import torch
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
    S, calls, K = 32, 4, 8
    base = [make_frame(1080, 1920, 8, seed=100 + k) for k in range(4)]
    rows = [plant_rows(b, (1080, 1920), 15120, (384, 640), 6, seed=200 + k) for k, (_, b) in enumerate(base)]
    shifted = [np.roll(f, 9 * (k + 1), axis=1) for k, (f, _) in enumerate(base)]
    srows = [plant_rows(b + np.float32([9 * (k + 1), 0, 9 * (k + 1), 0]), (1080, 1920), 15120, (384, 640), 6, seed=300 + k)
             for k, (_, b) in enumerate(base)]

    def pick(s, c):      # streams with s % 3 == 0 repeat their frame every other call (the gate closes)
        k = s % 4
        moved = (c % 2 == 1) and (s % 3 != 0)
        return (shifted[k], srows[k]) if moved else (base[k][0], rows[k])

    kw = long_video_weights(student_weights)
    multi = _engine(hip_library, detector_weights, kw, S, top_k=K)
    dev = _engine(hip_library, detector_weights, kw, S, top_k=K)
    single = _engine(hip_library, detector_weights, kw, 0, top_k=K)
    try:
        got = []
        for c in range(calls):
            fr = [pick(s, c) for s in range(S)]
            host = np.stack([x for x, _ in fr])
            pr = np.stack([y for _, y in fr])
            a = multi.track_streams(list(range(S)), host, planted_rows=pr, **ARGS)
            t = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            b = dev.track_streams(list(range(S)), t.data_ptr(), planted_rows=pr, shape=tuple(t.shape[:3]), **ARGS)
            for s in range(S):
                _same(a[s], b[s], ("device frames", c, s))
            got.append(a)
        assert any(not r[3] for g in got for r in g) and all(len(r[0]) == 8 for g in got for r in g)
        for s in range(S):
            single.track_reset()
            for c in range(calls):
                fr, pr = pick(s, c)
                _same(got[c][s], _single(single, fr, pr, K), (s, c))
    finally:
        multi.close()
        dev.close()
        single.close()

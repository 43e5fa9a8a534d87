"""Persistent face ids of the tracker (pf_track_ids_config / pf_track_ids, FaceAna / StreamTracker ``track_ids`` and
``spare_ids``) over tests/track_ident_video.py: the hand-stated ids and ages of every segment, the numpy restatement
tests/track_ident_ref.py replayed on the host facade's arrays, both tracking modes, three staggered streams, bit-identity of
the tracking results with ids on and off, the launch log, the refusals and redaction by identity.  Every device test has an
emulator version (CPU tier) and a GPU twin; the device-output test runs on the GPU only."""
import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from tests import draw_ref as dr
from tests import mask_ref as mr
from tests import redact_ref as rr
from tests import track_ident_ref as ref
from tests.test_track_streams import ARGS, TOP_K, _engine, _schedule
from tests.test_tracking_parity import _PlantedDetector
from tests.track_ident_video import NMS_IOU, TRACK_IOU, episodes, numpy_evidence, video_ident
from tests.tracking_video import S_LONG, long_video_weights, video, video_long


# ---- the fixture's own preconditions ----------------------------------------------------------------------------------------
def test_ident_fixture_hits_every_edge():
    ev = numpy_evidence()
    # duplicate_claim: both detections over the track threshold, under the NMS threshold against each other, the greater one row 1
    w = ev["duplicate_claim_iou"]
    assert w.dtype == np.float32 and TRACK_IOU < w[0] < w[1] and ev["duplicate_claim_mutual"] < NMS_IOU
    assert ev["duplicate_claim_areas"][0] < ev["duplicate_claim_areas"][1]
    # duplicate_equal: bit-equal float32 areas (inside the track box the judge's IoU is a function of the area alone)
    a = ev["duplicate_equal_areas"]
    assert a.dtype == np.float32 and a[0] == a[1] and a[0].tobytes() == a[1].tobytes()
    assert (ev["duplicate_equal_iou"] > TRACK_IOU).all() and ev["duplicate_equal_mutual"] < NMS_IOU
    # lost_and_found: absent from exactly three frames; the restatement replayed on the planted boxes has every entry at gone 3 in
    # front of the last frame and every returning box over the threshold against a lost one, so the segment's keep_lost values sit
    # on both sides of the boundary (3 keeps, 2 and 0 drop), and its replay gives the ids and ages the segment states
    assert ev["absent_frames"] == 3 and ev["gone_on_return"] == [3, 3, 3] and min(ev["return_iou"]) > TRACK_IOU
    laf = [s for s in video_ident() if s["name"] == "lost_and_found"][0]
    assert sorted(laf["expect"]) == [0, 2, 3]
    for kl, ex in laf["expect"].items():
        kept = kl > 0 and not ev["gone_on_return"][0] > kl
        assert ex["ids"][-1] == ([1, 2, 3] if kept else [4, 5, 6]) == ev["return_ids"][kl], kl
        assert ex["ages"][-1] == ev["return_ages"][kl], kl
    assert ev["lost_rows_over_thres"][0] > 0 < ev["lost_rows_over_thres"][4]
    # reorder: seven distinct areas over min_face in NMS order G F E D C B A: A sixth, G seventh, newcomer E larger than newcomer F
    ar = ev["reorder_areas"]
    assert len(ar) == 7 and len(set(ar.tolist())) == 7 and ar.min() > 1600
    assert int((ar > ar[6]).sum()) == 5 and int((ar > ar[0]).sum()) == 6 and ar[2] > ar[1] > ar[6]


def test_lost_list_eviction_host_rule_against_restatement():
    """The 64-entry limit of the lost list (rule step 6, last clause), which no video with top_k 5 reaches: the package's host
    rule (core/smoother/ident.py) and the restatement on synthetic detector frames of 20 faces, numpy only.  Face r of frame f is
    the 50 x 50 box at (100 r, 100 f), so boxes of different frames never meet; keep_lost 255, so nothing expires.  Hand-stated:
    frames 0-3 hand out ids 1-80, frame 4 ids 81-100 and leaves 80 entries (gone 4, 3, 2, 1 in twenties) of which the 16 EARLIEST
    of the gone-4 group go: ids 17-80 stay, in order.  Frame 5 has face (0, 16) back (id 17, lost and kept: age 2), face (0, 3)
    back (id 4 was evicted: a fresh id, 101) and face (4, 5) carried on (id 86, age 2); 63 + 19 entries remain, and the 18 longest
    gone go: 18-20 (gone 5) and the earliest 15 of the gone-4 group, 21-35."""
    from peppa_pig_face_landmark_amd.core.smoother.ident import MAX_LOST, IdentityTracker
    assert MAX_LOST == ref.LOST_CAP == 64
    box = lambda f, r: np.asarray([100.0 * r, 100.0 * f, 100.0 * r + 50, 100.0 * f + 50])          # noqa: E731
    frames = [([box(f, r) for r in range(20)], [-1] * 20) for f in range(5)]
    frames.append(([box(0, 16), box(0, 3), box(4, 5)], [-1, -1, 5]))
    want_ids = [list(range(20 * f + 1, 20 * f + 21)) for f in range(5)] + [[17, 101, 86]]
    want_ages = [[1] * 20] * 5 + [[2, 1, 2]]
    want_lost = {4: (list(range(17, 81)), [4] * 4 + [3] * 20 + [2] * 20 + [1] * 20),
                 5: (list(range(36, 81)) + [i for i in range(81, 101) if i != 86], [4] * 5 + [3] * 20 + [2] * 20 + [1] * 19)}
    host, state, prev = IdentityTracker(255, 0.5), ref.new_state(), None
    for k, (boxes, sources) in enumerate(frames):
        b = np.stack(boxes)
        ids, ages = host.update(sources, [1.0 if j >= 0 else 0.0 for j in sources], b, prev)
        rid, rage = ref.step(state, prev, b, list(range(len(b))), np.ones(len(b), bool), b, 255, 0.5)
        assert ids.tolist() == rid.tolist() == want_ids[k] and ages.tolist() == rage.tolist() == want_ages[k], k
        assert [e[0] for e in host.lost] == [e["id"] for e in state["lost"]] and len(host.lost) <= 64, k
        assert [e[3] for e in host.lost] == [e["gone"] for e in state["lost"]], k
        assert [e[1] for e in host.lost] == [e["age"] for e in state["lost"]], k
        assert all(np.array_equal(e[2], r["box"]) for e, r in zip(host.lost, state["lost"])), k
        if k in want_lost:
            assert ([e[0] for e in host.lost], [e[3] for e in host.lost]) == want_lost[k], k
        prev = b


# ---- playing the episodes ---------------------------------------------------------------------------------------------------
def _track(eng, seg, fr, rw):
    return eng.track_frame(fr, ARGS["score_thres"], ARGS["nms_iou_thres"], seg["min_face"], TOP_K, ARGS["track_iou_thres"],
                           ARGS["smooth_box"], ARGS["diff_thres"], rw)


class _Bases:
    """The ids a tracker used before an episode: 0 after a change of keep_lost (ids restart), else the greatest id seen."""

    def __init__(self):
        self.keep_lost, self.top = None, 0

    def begin(self, keep_lost):
        changed = keep_lost != self.keep_lost
        if changed:
            self.keep_lost, self.top = keep_lost, 0
        return changed, self.top

    def saw(self, ids):
        self.top = max([self.top] + [int(i) for i in ids])


_RUNS = {}


def _play_engine(library, student_weights, detector_weights):
    """pf_track_frame + pf_track_ids over the episodes: [(segment, keep_lost, base, [(boxes, ids, ages)])]; one run per library."""
    key = ("engine", library)
    if key in _RUNS:
        return _RUNS[key]
    eng = _engine(library, detector_weights, long_video_weights(student_weights), 0)
    bases, out = _Bases(), []
    try:
        for seg, kl in episodes():
            changed, base = bases.begin(kl)
            if changed:
                eng.track_ids_config(True, kl)
            eng.track_reset()
            res = []
            for fr, rw in zip(seg["frames"], seg["rows"]):
                r = _track(eng, seg, fr, rw)
                ids, ages = eng.track_ids(len(r[0]))
                bases.saw(ids)
                res.append((r[0], ids, ages))
            out.append((seg, kl, base, res))
    finally:
        eng.close()
    _RUNS[key] = out
    return out


def _facer(library, student_weights, detector_weights, device_tracking, **opts):
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    cfg = get_cfg()
    cfg["Skps"]["Engine"]["device_tracking"] = device_tracking
    cfg["Skps"]["Detect"]["input_shape"] = [384, 640, 3] if device_tracking else [96, 160, 3]
    cfg["Skps"]["Keypoints"]["input_shape"] = [S_LONG, S_LONG, 3]
    cfg["Skps"]["Engine"]["dtype"] = "f32"
    return FaceAna(cfg=cfg, weights={"detector": detector_weights, "keypoints": long_video_weights(student_weights)}, library=library,
                   **opts)


def _plant(facer, state, hw, seen=None):
    """Planted rows for either tracking mode; ``seen``: dict that receives the NMS boxes of a host-mode detector call."""
    if facer.device_tracking:
        facer._planted_rows = lambda: state["rows"]
        return
    det = _PlantedDetector(facer.engine, lambda: state["rows"], hw)

    def watched(image):
        b = det(image)
        if seen is not None:
            seen["nms"] = b
        return b
    facer.face_detector = watched


def _play_facade(library, student_weights, detector_weights, device_tracking):
    """FaceAna over the episodes, like _play_engine; in host mode every frame also records the arrays the stages saw:
    (previous track boxes, NMS boxes or None, selected rows, valid flags, new track boxes)."""
    key = ("facade", library, device_tracking)
    if key in _RUNS:
        return _RUNS[key]
    facer = _facer(library, student_weights, detector_weights, device_tracking, track_ids=True)
    bases, out, state = _Bases(), [], {"rows": None}
    try:
        for seg, kl in episodes():
            changed, base = bases.begin(kl)
            if changed:
                facer.configure_track_ids(kl)
            facer.reset()
            facer.min_face = seg["min_face"]
            seen = {}
            _plant(facer, state, seg["hw"], seen)
            res = []
            for fr, rw in zip(seg["frames"], seg["rows"]):
                state["rows"] = rw
                seen.pop("nms", None)
                prev = None if facer.track_box is None else np.array(facer.track_box)
                dicts = facer.run(fr.copy())
                assert all(isinstance(d["id"], int) and isinstance(d["age"], int) for d in dicts)
                ids, ages = np.asarray([d["id"] for d in dicts], np.int32), np.asarray([d["age"] for d in dicts], np.int32)
                bases.saw(ids)
                arrays = None
                if not device_tracking:
                    sel = list(facer._sel_rows)
                    valid = np.asarray(facer.face_landmark.last_valid, bool) if sel else np.zeros((0,), bool)
                    arrays = (prev, seen.get("nms"), sel, valid, np.asarray(facer.track_box, np.float64).reshape(-1, 4))
                res.append((np.asarray([d["box"] for d in dicts], np.float64).reshape(-1, 4), ids, ages, arrays))
            out.append((seg, kl, base, res))
    finally:
        facer.engine.close()
    _RUNS[key] = out
    return out


def _by_face(boxes, faces, ids, ages):
    """{planted face: (id, age)} of a frame's rows: a row is the face its track box is centred nearest to."""
    centres = np.asarray([[cx, cy] for cx, cy, _, _ in faces], np.float64).reshape(-1, 2)
    out = {}
    for bx, i, a in zip(boxes, ids, ages):
        c = np.asarray([(bx[0] + bx[2]) / 2, (bx[1] + bx[3]) / 2])
        out[int(np.argmin(np.abs(centres - c).max(axis=1)))] = (int(i), int(a))
    return out


def _hand_stated(run, where):
    """Ids and ages of every frame of every episode as the fixture states them, and every row on the planted face it states."""
    for seg, kl, base, res in run:
        ex = seg["expect"][kl]
        for k, (r, faces, want) in enumerate(zip(res, seg["faces"], ex["row_face"])):
            boxes, ids, ages = r[0], r[1], r[2]
            at = (where, seg["name"], kl, k)
            if k in ex.get("any_order", ()):
                stated = {f: (base + i, a) for f, i, a in zip(want, ex["ids"][k], ex["ages"][k])}
                assert len(ids) == len(want) and _by_face(boxes, faces, ids, ages) == stated, (at, ids, ages, stated)
                continue
            assert [int(i) for i in ids] == [base + i for i in ex["ids"][k]], (at, ids, base, ex["ids"][k])
            assert [int(a) for a in ages] == ex["ages"][k], (at, ages, ex["ages"][k])
            if seg["name"] in ("duplicate_claim", "duplicate_equal", "iou_first"):
                continue          # overlapping track boxes by construction: the ids above are what is stated
            centres = np.asarray([[cx, cy] for cx, cy, _, _ in faces], np.float64).reshape(-1, 2)
            for j, bx in enumerate(boxes):
                c = np.asarray([(bx[0] + bx[2]) / 2, (bx[1] + bx[3]) / 2])
                assert int(np.argmin(np.abs(centres - c).max(axis=1))) == want[j], (at, j)


def _single(library, student_weights, detector_weights):
    run = _play_engine(library, student_weights, detector_weights)
    _hand_stated(run, "pf_track_frame")
    # the restatement replayed on the arrays the host facade's stages saw gives the same ids, frame by frame
    host = _play_facade(library, student_weights, detector_weights, False)
    state, kl_now = ref.new_state(), None
    for (seg, kl, base, res), (_, _, _, dev) in zip(host, run):
        if kl != kl_now:
            state, kl_now = ref.new_state(), kl
        ref.forget(state)
        for k, ((_, ids, ages, arrays), d) in enumerate(zip(res, dev)):
            prev, nms, sel, valid, new = arrays
            want = ref.step(state, prev, nms, sel, valid, new, kl, ARGS["track_iou_thres"])
            assert want[0].tolist() == ids.tolist() == d[1].tolist(), (seg["name"], kl, k, want[0], ids, d[1])
            assert want[1].tolist() == ages.tolist() == d[2].tolist(), (seg["name"], kl, k)
            if seg["name"] in ("duplicate_claim", "duplicate_equal") and k == 1:
                # the evidence numpy alone cannot give: the track box takes both detections in, so the weights are area / track area
                assert len(prev) == 1 and len(nms) == 2
                t = prev[0]
                assert all(t[0] <= b[0] and t[1] <= b[1] and b[2] <= t[2] and b[3] <= t[3] for b in nms), (t, nms)
                w = [ref._iou(np.asarray(b), np.asarray(t)) for b in nms]
                assert min(w) > TRACK_IOU and ((w[0] == w[1]) if seg["name"] == "duplicate_equal" else (w[1] > w[0])), w


def test_ids_match_hand_stated_and_restatement_emulator(emu_library, student_weights, detector_weights):
    _single(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_ids_match_hand_stated_and_restatement_gpu(hip_library, student_weights, detector_weights):
    _single(hip_library, student_weights, detector_weights)


# ---- 2. FaceAna: the same ids with device_tracking on and off ----------------------------------------------------------------
def _facade_modes(library, student_weights, detector_weights):
    host = _play_facade(library, student_weights, detector_weights, False)
    dev = _play_facade(library, student_weights, detector_weights, True)
    _hand_stated(host, "host tracking")
    _hand_stated(dev, "device tracking")
    for (seg, kl, _, a), (_, _, _, b) in zip(host, dev):
        for k, (x, y) in enumerate(zip(a, b)):
            assert x[1].tolist() == y[1].tolist() and x[2].tolist() == y[2].tolist(), (seg["name"], kl, k)


def test_faceana_ids_equal_in_both_tracking_modes_emulator(emu_library, student_weights, detector_weights):
    _facade_modes(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_faceana_ids_equal_in_both_tracking_modes_gpu(hip_library, student_weights, detector_weights):
    _facade_modes(hip_library, student_weights, detector_weights)


# ---- 3. three staggered streams ----------------------------------------------------------------------------------------------
def _streams(library, student_weights, detector_weights):
    """Streams 0 and 1 start a call apart, stream 2 sits out the second call of every episode; each plays every episode of
    episodes().  So the call index of a stream's frame differs from its slot (stream 1 is frame 0 of the calls stream 0 has left,
    stream 2 frame 1 or 2), under top_k filtering (reorder), compaction (rejected_crop) and the expiry of the lost list
    (lost_and_found with keep_lost 0, 3 and 2).  Per stream the ids are those of the single-stream replay counted from that
    stream's own base: a counter that leaked between streams would shift them."""
    single = {(seg["name"], kl): (base, res) for seg, kl, base, res in _play_engine(library, student_weights, detector_weights)}
    eps = episodes()
    plans = {0: (0, ()), 1: (1, ()), 2: (0, (1,))}
    multi = _engine(library, detector_weights, long_video_weights(student_weights), len(plans))
    bases = {s: _Bases() for s in plans}
    try:
        for seg, kl in eps:
            begin = {s: bases[s].begin(kl) for s in plans}
            if begin[0][0]:
                multi.track_ids_config(True, kl)
            multi.track_streams_reset(-1)
            frames, rows = seg["frames"], seg["rows"]
            when = {s: _schedule(len(frames), off, skip) for s, (off, skip) in plans.items()}
            got = {s: [] for s in plans}
            for c in range(max(max(v) for v in when.values()) + 1):
                call = {s: when[s].index(c) for s in plans if c in when[s]}
                order = sorted(call)
                out = multi.track_streams(order, np.stack([frames[call[s]] for s in order]),
                                          planted_rows=np.stack([rows[call[s]] for s in order]), **dict(ARGS, min_face=seg["min_face"]))
                ids, ages = (x.reshape(len(order), TOP_K) for x in multi.track_ids(len(order) * TOP_K))
                for i, s in enumerate(order):
                    n = len(out[i][0])
                    assert not ids[i, n:].any() and not ages[i, n:].any()          # rows beyond a frame's count are 0
                    got[s].append((ids[i, :n], ages[i, :n]))
                    bases[s].saw(ids[i, :n])
            sbase, sres = single[(seg["name"], kl)]
            for s in plans:
                for k, ((ids, ages), want) in enumerate(zip(got[s], sres)):
                    assert (ids - begin[s][1]).tolist() == (want[1] - sbase).tolist(), (s, seg["name"], k, ids, want[1])
                    assert ages.tolist() == want[2].tolist(), (s, seg["name"], k)
    finally:
        multi.close()


def _stream_tracker_keys(library, student_weights, detector_weights):
    from Skps import StreamTracker
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    seg = video_ident()[0]
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["input_shape"] = [384, 640, 3]
    cfg["Skps"]["Keypoints"]["input_shape"] = [S_LONG, S_LONG, 3]
    cfg["Skps"]["Engine"]["dtype"] = "f32"
    w = {"detector": detector_weights, "keypoints": long_video_weights(student_weights)}
    with pytest.raises(ValueError, match="track_ids"):
        StreamTracker(cfg=cfg, weights=w, max_streams=2, library=library, spare_ids={0: {1}})
    tr = StreamTracker(cfg=cfg, weights=w, max_streams=2, library=library, track_ids={"keep_lost": 1})
    try:
        for k in (0, 1):
            tr._planted_rows = lambda ids, _b, k=k: np.stack([seg["rows"][k]] * len(ids))
            out = tr.run({1: seg["frames"][k].copy(), 0: seg["frames"][k].copy()})
            for s in (0, 1):
                assert [d["id"] for d in out[s]] == [1, 2, 3] and [d["age"] for d in out[s]] == [k + 1] * 3
    finally:
        tr.close()


def test_streams_ids_equal_single_stream_replay_emulator(emu_library, student_weights, detector_weights):
    _streams(emu_library, student_weights, detector_weights)
    _stream_tracker_keys(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_streams_ids_equal_single_stream_replay_gpu(hip_library, student_weights, detector_weights):
    _streams(hip_library, student_weights, detector_weights)
    _stream_tracker_keys(hip_library, student_weights, detector_weights)


# ---- 4. results bit-identical with ids on and off; the launch log --------------------------------------------------------------
def _on_off(library, student_weights, detector_weights):
    frames, rows, _ = video_long()[0]
    kw = long_video_weights(student_weights)
    off, on = _engine(library, detector_weights, kw, 0), _engine(library, detector_weights, kw, 0)
    try:
        on.track_ids_config(True, 2)
        seg = dict(min_face=ARGS["min_face"])
        logs = {}
        for k, (fr, rw) in enumerate(zip(frames, rows)):
            if k == 3:                       # a detector frame with a track: every kernel of the tracker runs
                off.profile_enable(True)
                on.profile_enable(True)
            a, b = _track(off, seg, fr, rw), _track(on, seg, fr, rw)
            if k == 3:
                logs["never"], logs["on"] = off.launch_log(), on.launch_log()
                off.profile_enable(False)
                on.profile_enable(False)
            assert a[3] == b[3] and len(a[0]) == len(b[0]), k
            for x, y, name in zip(a[:3], b[:3], ("box", "kps", "scores")):
                assert x.tobytes() == y.tobytes(), (k, name)
            ids, ages = on.track_ids(len(b[0]))
            assert (ids > 0).all() and (ages > 0).all() and len(set(ids.tolist())) == len(ids)
        # the second segment of video_long() (360 x 640) after a reset, as test_track_streams plays it
        frames2, rows2, _ = video_long()[1]
        off.track_reset()
        on.track_reset()
        for k, (fr, rw) in enumerate(zip(frames2, rows2)):
            a, b = _track(off, seg, fr, rw), _track(on, seg, fr, rw)
            assert a[3] == b[3] and len(a[0]) == len(b[0]), ("segment 2", k)
            for x, y, name in zip(a[:3], b[:3], ("box", "kps", "scores")):
                assert x.tobytes() == y.tobytes(), ("segment 2", k, name)
            ids, ages = on.track_ids(len(b[0]))
            assert (ids > 0).all() and (ages > 0).all() and len(set(ids.tolist())) == len(ids)
        # ids switched off again: the log of the same call is the log of an engine that never had them
        on.track_ids_config(False, 0)
        on.track_reset()
        off.track_reset()
        for k, (fr, rw) in enumerate(zip(frames[:4], rows[:4])):
            if k == 3:
                off.profile_enable(True)
                on.profile_enable(True)
            a, b = _track(off, seg, fr, rw), _track(on, seg, fr, rw)
            for x, y in zip(a[:3], b[:3]):
                assert x.tobytes() == y.tobytes(), k
        logs["off_again"], logs["never_again"] = on.launch_log(), off.launch_log()
        assert logs["never"] == logs["never_again"] == logs["off_again"]
        assert not any("track_ident" in t for t in logs["never"]) and any("track_judge_kernel" in t for t in logs["never"])
        assert sum("track_ident_kernel" in t for t in logs["on"]) == 1
        assert [t for t in logs["on"] if "track_ident" not in t] == logs["never"]
    finally:
        off.close()
        on.close()


def test_results_bit_identical_with_ids_on_and_off_emulator(emu_library, student_weights, detector_weights):
    _on_off(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_results_bit_identical_with_ids_on_and_off_gpu(hip_library, student_weights, detector_weights):
    _on_off(hip_library, student_weights, detector_weights)


# ---- 5. refusals, resets, the range guard ---------------------------------------------------------------------------------------
def _refusals(library, student_weights, detector_weights):
    seg = video_ident()[0]
    fr, rw = seg["frames"], seg["rows"]
    kw = long_video_weights(student_weights)
    eng = _engine(library, detector_weights, kw, 2)
    try:
        with pytest.raises(_native.PeppaHipError, match="keep_lost"):
            eng.track_ids_config(True, 256)
        with pytest.raises(_native.PeppaHipError, match="keep_lost"):
            eng.track_ids_config(True, -1)
        with pytest.raises(_native.PeppaHipError, match="ids are off"):
            eng.track_ids(0)
        eng.track_ids_config(True, 0)
        with pytest.raises(_native.PeppaHipError, match="left no face rows"):          # before any tracking call
            eng.track_ids(0)
        eng.run_frames(fr[0][None], ARGS["score_thres"], ARGS["nms_iou_thres"], ARGS["min_face"], TOP_K, planted_rows=rw[0][None])
        with pytest.raises(_native.PeppaHipError, match="not a tracking call"):
            eng.track_ids(1)
        r = _track(eng, seg, fr[0], rw[0])
        assert eng.track_ids(3)[0].tolist() == [1, 2, 3] and len(r[0]) == 3
        with pytest.raises(_native.PeppaHipError, match="4 rows asked, the last call left 3"):
            eng.track_ids(4)
        eng.track_ids_config(False, 0)
        with pytest.raises(_native.PeppaHipError, match="ids are off"):
            eng.track_ids(3)
        # reset(): the next faces get ids above every id used before; a new pool starts at 1 again
        eng.track_ids_config(True, 0)
        for want in ([1, 2, 3], [4, 5, 6]):
            eng.track_reset()
            _track(eng, seg, fr[0], rw[0])
            assert eng.track_ids(3)[0].tolist() == want
        for want in ([1, 2, 3], [4, 5, 6], [1, 2, 3]):
            if want[0] == 4:
                eng.track_streams_reset(1)
            out = eng.track_streams([1], fr[0][None], planted_rows=rw[0][None], **ARGS)
            assert len(out[0][0]) == 3
            ids, ages = eng.track_ids(TOP_K)
            assert ids.tolist() == want + [0, 0] and ages.tolist() == [1, 1, 1, 0, 0]
            with pytest.raises(_native.PeppaHipError, match="rows asked"):
                eng.track_ids(TOP_K + 1)
            if want[0] == 4:
                eng.track_streams_config(2, TOP_K)
        # ids are kept for at most 64 faces per frame: with ids on a larger top_k is refused before anything changes -- the pool,
        # stream 1 and the single stream go on where they were
        with pytest.raises(_native.PeppaHipError, match="pf_track_streams_config: persistent ids are kept for at most 64 faces"):
            eng.track_streams_config(2, 65)
        out = eng.track_streams([1], fr[0][None], planted_rows=rw[0][None], **ARGS)
        ids, ages = eng.track_ids(TOP_K)
        assert not out[0][3] and ids.tolist() == [1, 2, 3, 0, 0] and ages.tolist() == [2, 2, 2, 0, 0]
        with pytest.raises(_native.PeppaHipError, match="pf_track_frame: persistent ids are kept for at most 64 faces"):
            eng.track_frame(fr[0], ARGS["score_thres"], ARGS["nms_iou_thres"], seg["min_face"], 65, ARGS["track_iou_thres"],
                            ARGS["smooth_box"], ARGS["diff_thres"], rw[0])
        _track(eng, seg, fr[0], rw[0])
        ids, ages = eng.track_ids(3)
        assert ids.tolist() == [4, 5, 6] and ages.tolist() == [2, 2, 2]
        # and the other way round: a pool of 65 faces first, then ids cannot be switched on
        eng.track_ids_config(False, 0)
        eng.track_streams_config(1, 65)
        with pytest.raises(_native.PeppaHipError, match="pf_track_ids_config: persistent ids are kept for at most 64 faces"):
            eng.track_ids_config(True, 0)
        with pytest.raises(_native.PeppaHipError, match="ids are off"):
            eng.track_ids(0)
    finally:
        eng.close()


def _range_guard_ids(library, student_weights, detector_weights):
    """The recipe of test_track_streams._range_guard: an f32s landmark program whose activations leave the f16 range fails the
    call; its streams restart with fresh ids (never a reused one), the stream that sat out keeps its ids."""
    from peppa_pig_face_landmark_amd.graph.student import build_student_program
    from tests.test_range_guard import _scaled
    frames, rows = video()
    w = _scaled(student_weights, 3.0e5)
    eng = _engine(library, detector_weights, w, 3, size=64)
    args = dict(ARGS)
    try:
        eng.track_ids_config(True, 0)
        out = eng.track_streams([0, 1, 2], np.stack([frames[0]] * 3), planted_rows=np.stack([rows[0]] * 3), **args)
        n = len(out[0][0])
        assert n >= 2
        first = eng.track_ids(3 * TOP_K)[0].reshape(3, TOP_K)
        assert first[:, :n].tolist() == [list(range(1, n + 1))] * 3
        eng.load_program(_native.PF_NET_LANDMARK, build_student_program(w, 64, "f32s")[0], 3 * TOP_K)
        with pytest.raises(_native.PeppaHipError, match=r"program %d" % _native.PF_NET_LANDMARK):
            eng.track_streams([0, 1], np.stack([frames[0], frames[1]]), planted_rows=np.stack([rows[0], rows[1]]), **args)
        with pytest.raises(_native.PeppaHipError, match="pf_track_ids"):
            eng.track_ids(1)
        eng.load_program(_native.PF_NET_LANDMARK, build_student_program(w, 64, "f32")[0], 3 * TOP_K)
        out = eng.track_streams([0, 1, 2], np.stack([frames[1]] * 3), planted_rows=np.stack([rows[1]] * 3), **args)
        assert out[0][3] and out[1][3] and not out[2][3]
        ids, ages = (x.reshape(3, TOP_K) for x in eng.track_ids(3 * TOP_K))
        m = len(out[0][0])
        for s in (0, 1):                     # the failed call may have handed ids out before it failed: fresh means above the old ones
            assert (ids[s, :m] > n).all() and len(set(ids[s, :m].tolist())) == m and ages[s, :m].tolist() == [1] * m
        assert ids[2, :n].tolist() == list(range(1, n + 1)) and ages[2, :n].tolist() == [2] * n
    finally:
        eng.close()


def test_track_ids_refusals_and_lifetime_emulator(emu_library, student_weights, detector_weights):
    _refusals(emu_library, student_weights, detector_weights)
    _range_guard_ids(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_track_ids_refusals_and_lifetime_gpu(hip_library, student_weights, detector_weights):
    _refusals(hip_library, student_weights, detector_weights)
    _range_guard_ids(hip_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_track_ids_device_output_equals_host_gpu(hip_library, student_weights, detector_weights):
    import torch
    seg = [s for s in video_ident() if s["name"] == "reorder"][0]
    eng = _engine(hip_library, detector_weights, long_video_weights(student_weights), 2)
    try:
        eng.track_ids_config(True, 1)
        for fr, rw in zip(seg["frames"], seg["rows"]):
            r = _track(eng, seg, fr, rw)
            n = len(r[0])
            ids, ages = eng.track_ids(n)
            d = torch.full((2, TOP_K), -1, dtype=torch.int32, device="cuda")
            eng.track_ids_device(n, d[0].data_ptr(), d[1].data_ptr())
            eng.sync()
            got = d.cpu().numpy()
            assert got[0, :n].tolist() == ids.tolist() and got[1, :n].tolist() == ages.tolist() and (got[:, n:] == -1).all()
            eng.track_ids_device(n, 0, d[1].data_ptr())          # either pointer may be NULL
        out = eng.track_streams([1, 0], np.stack([seg["frames"][1]] * 2), planted_rows=np.stack([seg["rows"][1]] * 2), **ARGS)
        ids, ages = eng.track_ids(2 * TOP_K)
        d = torch.zeros((2, 2 * TOP_K), dtype=torch.int32, device="cuda")
        eng.track_ids_device(2 * TOP_K, d[0].data_ptr(), d[1].data_ptr())
        eng.sync()
        assert d.cpu().numpy().tolist() == [ids.tolist(), ages.tolist()] and len(out) == 2
    finally:
        eng.close()


# ---- 6. redaction by identity ---------------------------------------------------------------------------------------------------
def _spare(library, student_weights, detector_weights, device_tracking):
    from Skps import FaceAna  # noqa: F401
    with pytest.raises(ValueError, match="track_ids"):
        _facer(library, student_weights, detector_weights, device_tracking, redact={"mode": "fill"}, spare_ids={2})
    seg = [s for s in video_ident() if s["name"] == "reorder"][0]
    ex = seg["expect"][0]
    colour = (0, 255, 0)
    facer = _facer(library, student_weights, detector_weights, device_tracking, track_ids=True, spare_ids={2},
                   redact={"mode": "fill", "colour": colour}, jpeg=90, draw={"base": "redacted"})
    state = {"rows": None}
    try:
        facer.min_face = seg["min_face"]
        _plant(facer, state, seg["hw"])
        for k, (fr, rw) in enumerate(zip(seg["frames"], seg["rows"])):
            if k == 3:
                facer.spare_ids = {2, 7}         # changed between calls: A, who comes back as 7, is spared in its first frame
            state["rows"] = rw
            dicts = facer.run(fr.copy())
            ids = [d["id"] for d in dicts]
            stated = {f: (i, a) for f, i, a in zip(ex["row_face"][k], ex["ids"][k], ex["ages"][k])}
            assert _by_face([d["box"] for d in dicts], seg["faces"][k], ids, [d["age"] for d in dicts]) == stated, (k, ids)
            kps = np.stack([d["kps"] for d in dicts])
            select = [0 if i in facer.spare_ids else 1 for i in ids]
            H, W = fr.shape[:2]
            maps = mr.frame_maps(kps, None, H, W)
            want = rr.frame_reference(fr, kps, None, select, rr.FILL, rr.FACE_ALL, 0, 0, colour[0] | colour[1] << 8 | colour[2] << 16, maps=maps)[0]
            got = facer.last_redacted
            assert got.tobytes() == want.tobytes(), k
            # the files and the overlay follow: the engine's encoding of that frame, the overlay's restatement drawn over it
            assert facer.last_redacted_jpeg == facer.engine.encode_jpeg(want, quality=90, subsampling=420)[0], k
            scores = np.stack([d["scores"] for d in dicts])
            assert facer.last_drawn.tobytes() == dr.frame_reference(want, kps, None, scores)[0].tobytes(), k
            labels, owners = maps[0], maps[1]
            for j, i in enumerate(ids):          # the spared faces byte for byte, every labelled pixel of the others changed
                own = (owners == j + 1) & (labels > 0)
                assert own.sum() > 0, (k, j)
                if i in facer.spare_ids:
                    assert (got[own] == fr[own]).all(), (k, j)
                else:
                    assert (got[own] != fr[own]).any(axis=1).all(), (k, j)
            assert (k != 1) or select[0] == 1    # the face that first appears in frame 1 (row 0, id 4) is redacted at once
    finally:
        facer.engine.close()


def _spare_streams(library, student_weights, detector_weights):
    """StreamTracker: ``spare_ids`` per stream, with the files and the overlay that follow the redaction.  Two streams see the same
    two frames of the reorder segment but spare different ids, and the call lists stream 1 first, so a select built for the wrong
    stream or put together in another order than the call's shows in ``last_redacted``; ``last_redacted_jpeg`` is the engine's
    encoding of that frame and ``last_drawn`` the overlay's restatement over it."""
    from Skps import StreamTracker
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    seg =[s for s in video_ident() if s["name"] == "reorder"][0]
    ex = seg["expect"][0]
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["input_shape"] = [384, 640, 3]
    cfg["Skps"]["Keypoints"]["input_shape"] = [S_LONG, S_LONG, 3]
    cfg["Skps"]["Engine"]["dtype"] = "f32"
    colour = (0, 255, 0)
    spare = {0: {2}, 1: {1, 4}}
    tr = StreamTracker(cfg=cfg, weights={"detector": detector_weights, "keypoints": long_video_weights(student_weights)}, max_streams=2,
                       library=library, track_ids=True, spare_ids=spare, redact={"mode": "fill", "colour": colour}, jpeg=90,
                       draw={"base": "redacted"})
    try:
        tr.min_face = seg["min_face"]
        for k in (0, 1):
            fr = seg["frames"][k]
            tr._planted_rows = lambda ids, _b, k=k: np.stack([seg["rows"][k]] * len(ids))
            if k == 1:
                tr.spare_ids[0] = {2, 3}          # changed between calls
            out = tr.run({1: fr.copy(), 0: fr.copy()})
            selects = {}
            for s in (0, 1):
                ids = [d["id"] for d in out[s]]
                assert ids == ex["ids"][k] and [d["age"] for d in out[s]] == ex["ages"][k], (k, s, ids)
                kps, scores = np.stack([d["kps"] for d in out[s]]), np.stack([d["scores"] for d in out[s]])
                selects[s] = [0 if i in tr.spare_ids[s] else 1 for i in ids]
                want = rr.frame_reference(fr, kps, None, selects[s], rr.FILL, rr.FACE_ALL, 0, 0, colour[0] | colour[1] << 8 | colour[2] << 16)[0]
                assert tr.last_redacted[s].tobytes() == want.tobytes(), (k, s)
                assert tr.last_redacted_jpeg[s] == tr.engine.encode_jpeg(want, quality=90, subsampling=420)[0], (k, s)
                assert tr.last_drawn[s].tobytes() == dr.frame_reference(want, kps, None, scores)[0].tobytes(), (k, s)
            assert selects[0] != selects[1] and 0 in selects[0] and 0 in selects[1] and 1 in selects[0], k
    finally:
        tr.close()


def test_spare_ids_per_stream_with_files_and_overlay_emulator(emu_library, student_weights, detector_weights):
    _spare_streams(emu_library, student_weights, detector_weights)


@pytest.mark.gpu
def test_spare_ids_per_stream_with_files_and_overlay_gpu(hip_library, student_weights, detector_weights):
    _spare_streams(hip_library, student_weights, detector_weights)


@pytest.mark.parametrize("device_tracking", [False, True])
def test_spare_ids_redacts_everybody_else_emulator(emu_library, student_weights, detector_weights, device_tracking):
    _spare(emu_library, student_weights, detector_weights, device_tracking)


@pytest.mark.gpu
@pytest.mark.parametrize("device_tracking", [False, True])
def test_spare_ids_redacts_everybody_else_gpu(hip_library, student_weights, detector_weights, device_tracking):
    _spare(hip_library, student_weights, detector_weights, device_tracking)

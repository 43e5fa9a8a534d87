"""core/api/quality.py: the quality scores computed from the engine's exact per-face sums, the best-shot bookkeeping and the options of
the classes.  Pure Python: no engine is created."""
import numpy as np
import pytest

from peppa_pig_face_landmark_amd.core.api import quality as Q


def _stats(rows):
    """rows: {label: 9 values} -> uint64 [8,9]."""
    s = np.zeros((8, 9), np.uint64)
    for label, v in rows.items():
        s[label - 1] = v
    return s


def test_face_quality_on_hand_made_stats():
    # n = 100, sum Y = 12 800, sum Y^2 = 1 648 400: mean 128, variance 16 484 - 16 384 = 100
    q = Q.face_quality(_stats({1: [100, 1000, 2000, 3000, 12800, 1648400, 50000, 10, 20]}))
    assert q["pixels"] == 100 and q["brightness"] == 128.0 and q["contrast"] == 10.0
    assert q["sharpness"] == 500.0 and q["dark"] == 0.1 and q["bright"] == 0.2
    assert q["skin_bgr"].tolist() == [10.0, 20.0, 30.0]
    # N sums over the labels; skin_bgr over labels 1 and 6 only
    s = _stats({1: [60, 600, 1200, 1800, 6000, 700000, 6000, 6, 0], 6: [20, 600, 400, 200, 3000, 500000, 2000, 0, 4],
                4: [20, 9999, 9999, 9999, 1000, 100000, 2000, 4, 0]})
    q = Q.face_quality(s)
    assert q["pixels"] == 100 and q["brightness"] == 100.0 and q["sharpness"] == 100.0
    assert q["contrast"] == np.sqrt(1300000 / 100 - 100.0 ** 2)
    assert q["dark"] == 0.1 and q["bright"] == 0.04
    assert q["skin_bgr"].tolist() == [1200 / 80, 1600 / 80, 2000 / 80]
    # a negative variance from rounding is clamped; batches keep their leading shape
    q = Q.face_quality(np.stack([_stats({1: [3, 0, 0, 0, 30, 300, 0, 0, 0]}), _stats({})])[None])
    assert q["pixels"].shape == (1, 2) and q["skin_bgr"].shape == (1, 2, 3)
    assert q["contrast"][0, 0] == 0.0 and q["pixels"][0, 1] == 0
    for key in ("brightness", "contrast", "sharpness", "dark", "bright"):
        assert np.isnan(q[key][0, 1]), key
    assert np.isnan(q["skin_bgr"][0, 1]).all()
    # sums above 2^32 survive
    q = Q.face_quality(_stats({6: [13392, 0, 0, 0, 0, 0, 13749354000, 0, 0]}))
    assert q["sharpness"] == 13749354000 / 13392
    with pytest.raises(ValueError):
        Q.face_quality(np.zeros((8, 8), np.uint64))


def _result(ident, sharp, pixels=1000, dark=0.0, bright=0.0, **extra):
    return dict({"id": ident, "quality": {"pixels": float(pixels), "sharpness": float(sharp), "dark": dark, "bright": bright,
                                          "brightness": 100.0, "contrast": 10.0}}, **extra)


def test_best_shots_keeps_the_best_per_stream_and_id():
    bs = Q.BestShots()
    assert bs.update([_result(1, 10.0, chip="a"), _result(2, 50.0, chip="b")]) == [(0, 1), (0, 2)]
    assert bs.update([_result(1, 5.0, chip="c"), _result(2, 60.0, chip="d")]) == [(0, 2)]
    assert bs.best[(0, 1)]["chip"] == "a" and bs.best[(0, 1)]["call"] == 0 and bs.best[(0, 1)]["score"] == 10.0
    assert bs.best[(0, 2)]["chip"] == "d" and bs.best[(0, 2)]["call"] == 1
    # the default score: sharpness * (1 - dark - bright), 0 below min_pixels
    assert bs.score(_result(0, 100.0, dark=0.25, bright=0.25)["quality"]) == 50.0
    assert bs.score(_result(0, 100.0, pixels=399)["quality"]) == 0.0
    assert bs.score({"pixels": 0.0, "sharpness": float("nan"), "dark": float("nan"), "bright": float("nan")}) == 0.0
    assert bs.update([_result(3, 1e9, pixels=399)]) == [] and (0, 3) not in bs.best          # too small: ignored
    assert bs.update([_result(1, 11.0, dark=0.5)]) == []                                      # 5.5 < 10
    # streams keep their own ids
    assert bs.update([_result(1, 1.0)], stream=7) == [(7, 1)]
    assert set(bs.best) == {(0, 1), (0, 2), (7, 1)} and bs.calls == 5
    bs.forget(stream=0)
    assert set(bs.best) == {(7, 1)}
    bs.forget()
    assert bs.best == {}
    with pytest.raises(ValueError, match="needs 'id'"):
        bs.update([{"quality": {}}])


def test_best_shots_custom_key_and_min_pixels():
    bs = Q.BestShots(key=lambda q: -abs(q["brightness"] - 128.0))      # any callable; scores need not be positive
    a, b = _result(1, 0.0), _result(1, 0.0)
    a["quality"]["brightness"], b["quality"]["brightness"] = 100.0, 120.0
    assert bs.update([a]) == [(0, 1)] and bs.update([b]) == [(0, 1)] and bs.update([a]) == []
    assert bs.best[(0, 1)]["score"] == -8.0 and bs.best[(0, 1)]["call"] == 1
    assert Q.BestShots(min_pixels=10).update([_result(1, 2.0, pixels=10)]) == [(0, 1)]


def test_options():
    assert Q.stats_options(None, {}) is None and Q.stats_options(False, {"face_stats": True}) is None
    assert Q.stats_options(None, {"face_stats": True}) == {"dark": 16, "bright": 240}
    assert Q.stats_options({"dark": 64}, {}) == {"dark": 64, "bright": 240}
    with pytest.raises(ValueError, match="unknown keys"):
        Q.stats_options({"darkness": 1}, {})
    assert Q.best_shots_options(None, None, None) is None
    assert Q.best_shots_options({"min_pixels": 5}, {"keep_lost": 0}, {"dark": 16, "bright": 240}).min_pixels == 5
    with pytest.raises(ValueError, match="unknown keys"):
        Q.best_shots_options({"best": 1}, {"keep_lost": 0}, {"dark": 16, "bright": 240})


def test_attach_stats():
    stats = np.stack([_stats({1: [100, 1000, 2000, 3000, 12800, 1648400, 50000, 10, 20]}), np.full((8, 9), 0xAB, np.uint64)])
    dicts = Q.attach_stats([{}, {}], stats, np.array([True, False]))
    assert dicts[0]["stats"].dtype == np.uint64 and np.array_equal(dicts[0]["stats"], stats[0]) and dicts[0]["quality"]["brightness"] == 128.0
    assert (dicts[1]["stats"] == 0).all() and dicts[1]["quality"]["pixels"] == 0.0 and np.isnan(dicts[1]["quality"]["sharpness"])
    assert dicts[0]["quality"]["skin_bgr"].shape == (3,)


@pytest.mark.parametrize("kw", [dict(best_shots=True), dict(best_shots=True, track_ids=True), dict(best_shots=True, face_stats=True)])
def test_classes_refuse_best_shots_without_ids_and_stats(student_weights, detector_weights, kw):
    """The options are judged before an engine is created."""
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker
    weights = {"detector": detector_weights, "keypoints": student_weights}
    with pytest.raises(ValueError, match="best_shots needs track_ids and face_stats"):
        FaceAna(weights=weights, library="/nonexistent/libpeppa_hip.so", **kw)
    with pytest.raises(ValueError, match="best_shots needs track_ids and face_stats"):
        StreamTracker(weights=weights, library="/nonexistent/libpeppa_hip.so", **kw)

"""Quality scores from the per-face region statistics the engine measures on the device (``Engine.measure_faces`` / ``face_stats``,
include/peppa_hip.h pf_measure_faces), and the bookkeeping that keeps the best shot of every tracked id.  Host code only: the sums
are exact integers, everything here is float64 arithmetic on 72 numbers per face."""
from typing import Callable, Optional

import numpy as np

LABELS, FIELDS = 8, 9
SKIN_LABELS = (1, 6)            # face skin and nose


def stats_options(value, eng_cfg):
    """The ``face_stats`` option of the classes: ``None`` -> ``Engine.face_stats`` of the configuration if present, else off
    (``None`` is returned); ``True`` is the defaults; a dict gives any of "dark" (16) and "bright" (240)."""
    if value is None:
        value = eng_cfg.get("face_stats", None)
    if not value:
        return None
    opts = {"dark": 16, "bright": 240}
    if isinstance(value, dict):
        unknown = set(value) - set(opts)
        if unknown:
            raise ValueError("face_stats: unknown keys %s" % sorted(unknown))
        opts.update(value)
    return opts


def best_shots_options(value, track_ids, face_stats):
    """The ``best_shots`` option of FaceAna / StreamTracker: a false value is off (``None``), ``True`` or a dict with any of "key" and
    "min_pixels" gives a ``BestShots``; it needs ``track_ids`` and ``face_stats`` on."""
    if not value:
        return None
    if not track_ids or not face_stats:
        raise ValueError("best_shots needs track_ids and face_stats on")
    if isinstance(value, dict):
        unknown = set(value) - {"key", "min_pixels"}
        if unknown:
            raise ValueError("best_shots: unknown keys %s" % sorted(unknown))
        return BestShots(**value)
    return BestShots()


def face_quality(stats) -> dict:
    """stats uint64 [...,8,9] (row L - 1 = label L; n, sum c0, sum c1, sum c2, sum Y, sum Y^2, sum Lap^2, dark, bright) -> a dict of
    float64 arrays of shape [...] (``skin_bgr``: [...,3]).  With N the pixels of all eight labels: ``pixels`` N, ``brightness`` the
    mean luma, ``contrast`` its standard deviation, ``sharpness`` the mean squared Laplacian (per FRAME pixel, so it falls as a face
    grows), ``dark`` / ``bright`` the fractions of dark and bright pixels, ``skin_bgr`` the channel means over labels 1 and 6.  A
    face without pixels gives ``pixels`` 0 and NaN elsewhere."""
    s = np.asarray(stats)
    if s.shape[-2:] != (LABELS, FIELDS):
        raise ValueError("stats must be [...,8,9]")
    s = s.astype(np.float64)                            # every sum of a frame is far below 2^53: exact
    tot = s.sum(-2)
    N = tot[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        brightness = tot[..., 4] / N
        skin = s[..., [L - 1 for L in SKIN_LABELS], :].sum(-2)
        return {
            "pixels": N,
            "brightness": brightness,
            "contrast": np.sqrt(np.maximum(tot[..., 5] / N - brightness * brightness, 0.0)),
            "sharpness": tot[..., 6] / N,
            "dark": tot[..., 7] / N,
            "bright": tot[..., 8] / N,
            "skin_bgr": skin[..., 1:4] / skin[..., 0:1],
        }


def attach_stats(dicts, stats, valid=None):
    """Result dict i gets ``"stats"`` (uint64 [8,9], row i of ``stats``) and ``"quality"`` (``face_quality`` of it, scalars); a row
    whose ``valid`` flag is false carries zeros."""
    for i, d in enumerate(dicts):
        st = np.array(stats[i], np.uint64)
        if valid is not None and not valid[i]:
            st[:] = 0
        q = face_quality(st)
        d["stats"] = st
        d["quality"] = {k: (v.copy() if v.ndim else float(v)) for k, v in q.items()}
    return dicts


class BestShots:
    """The best result of every (stream, id) seen so far.  ``update(results, stream)`` takes the result dicts of one call (each with
    ``"id"`` and ``"quality"``) and returns the keys whose best improved; ``best[(stream, id)]`` is the result dict that scored
    highest -- with its ``"chip"`` / ``"chip_jpeg"`` when the chips are on -- plus ``"score"`` and ``"call"``, the index of the
    update that brought it.

    The default score is 0 below ``min_pixels`` labelled pixels, else ``sharpness * (1 - dark - bright)``: sharp and neither
    crushed nor blown out.  It is a CONVENTION NOBODY HAS CALIBRATED -- the trained weights are absent and no recognition network
    is at hand to say which chip it would rather see; ``key`` takes any callable on the quality dict instead."""

    def __init__(self, key: Optional[Callable[[dict], float]] = None, min_pixels: int = 400):
        self.key = key
        self.min_pixels = int(min_pixels)
        self.best = {}
        self.calls = 0

    def score(self, quality: dict) -> float:
        if self.key is not None:
            return float(self.key(quality))
        if not quality["pixels"] >= self.min_pixels:     # NaN and too few pixels alike
            return 0.0
        return float(quality["sharpness"] * (1.0 - quality["dark"] - quality["bright"]))

    def update(self, results, stream=0):
        improved = []
        for r in results:
            if "id" not in r or "quality" not in r:
                raise ValueError("BestShots.update: a result needs 'id' (track_ids) and 'quality' (face_stats)")
            s = self.score(r["quality"])
            k = (stream, int(r["id"]))
            if self.key is None and not s > 0.0:         # the default's zero: too small (or all dark and bright) to be a shot at all
                continue
            if k not in self.best or s > self.best[k]["score"]:
                self.best[k] = dict(r, score=s, call=self.calls)
                improved.append(k)
        self.calls += 1
        return improved

    def forget(self, stream=None):
        """Drops every record (``None``) or those of one stream."""
        if stream is None:
            self.best.clear()
        else:
            for k in [k for k in self.best if k[0] == stream]:
                del self.best[k]

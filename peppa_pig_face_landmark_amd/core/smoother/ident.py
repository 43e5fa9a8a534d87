"""Persistent face ids of a tracked stream on the host: the identity rule of include/peppa_hip.h ("Persistent face ids",
steps 1-6) in numpy, for ``FaceAna`` without ``device_tracking``.  With ``device_tracking`` the same rule runs on the GPU
(track_ident_kernel, csrc/k_track.h) and the two give the same ids on the same video."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_LOST = 64


def box_iou_f64(a, b) -> float:
    """IoU of judge_boxs on float64 scalars, one rounding per operation (pf_box_iou_f64_strict)."""
    a = [float(v) for v in a[:4]]
    b = [float(v) for v in b[:4]]
    s1 = (a[2] - a[0]) * (a[3] - a[1])
    s2 = (b[2] - b[0]) * (b[3] - b[1])
    inter = max(0.0, min(a[2], b[2]) - max(a[0], b[0])) * max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    den = (s1 + s2) - inter
    if den == 0.0 or den != den or inter != inter:
        return float("nan")
    return inter / den


class IdentityTracker:
    """State of one stream: ids / ages of the rows of the track boxes, the counter, the lost list."""

    def __init__(self, keep_lost: int = 0, iou_thres: float = 0.5):
        if not 0 <= int(keep_lost) <= 255:
            raise ValueError("keep_lost must be in [0, 255]")
        self.keep_lost = int(keep_lost)
        self.iou_thres = float(np.float32(iou_thres))      # the C ABI takes the threshold as a float
        self.next_id = 0                                   # ids handed out so far
        self.ids: List[int] = []
        self.ages: List[int] = []
        self.lost: List[list] = []                         # [id, age, box, gone], insertion order

    def reset(self):
        """FaceAna.reset(): ids, ages and the lost list go, the counter stays (an id is never reused)."""
        self.ids, self.ages, self.lost = [], [], []

    def update(self, sources: Sequence[int], weights: Sequence[float], new_boxes, prev_boxes) -> Tuple[np.ndarray, np.ndarray]:
        """One frame.  ``sources[o]`` / ``weights[o]``: previous row (or -1) and claim weight of output row o (step 1, before the
        id-0 clause); ``new_boxes`` [n_out,4]: the track boxes after this frame; ``prev_boxes``: those before it (or None)."""
        n_prev = len(self.ids)
        src = [int(j) if 0 <= int(j) < n_prev and self.ids[int(j)] != 0 else -1 for j in sources]
        keeper = [-1] * n_prev
        for o, j in enumerate(src):                        # step 3
            if j >= 0 and (keeper[j] < 0 or float(weights[o]) > float(weights[keeper[j]])):
                keeper[j] = o
        lost = self.lost if self.keep_lost > 0 else []
        claimed = [False] * len(lost)
        ids, ages = [], []
        for o, j in enumerate(src):                        # steps 4, 5
            if j >= 0 and keeper[j] == o:
                ids.append(self.ids[j])
                ages.append(self.ages[j] + 1)
                continue
            best, bw = -1, self.iou_thres
            for e, ent in enumerate(lost):
                if claimed[e]:
                    continue
                v = box_iou_f64(new_boxes[o], ent[2])
                if v > bw:
                    best, bw = e, v
            if best >= 0:
                ids.append(lost[best][0])
                ages.append(lost[best][1] + 1)
                claimed[best] = True
            else:
                self.next_id += 1
                ids.append(self.next_id)
                ages.append(1)
        new_lost = []                                      # step 6
        for e, ent in enumerate(lost):
            if not claimed[e] and ent[3] + 1 <= self.keep_lost:
                new_lost.append([ent[0], ent[1], ent[2], ent[3] + 1])
        if self.keep_lost > 0:
            for j in range(n_prev):
                if self.ids[j] != 0 and keeper[j] < 0:
                    new_lost.append([self.ids[j], self.ages[j], np.array(prev_boxes[j][:4], np.float64), 1])
        while len(new_lost) > MAX_LOST:
            gone = [ent[3] for ent in new_lost]
            del new_lost[gone.index(max(gone))]
        self.ids, self.ages, self.lost = ids, ages, new_lost
        return np.asarray(ids, np.int32), np.asarray(ages, np.int32)


def ids_options(value, eng_cfg) -> Optional[dict]:
    """The ``track_ids`` option of the classes: ``None`` -> ``Engine.track_ids`` of Skps.yml; a false value is off (``None`` is
    returned); ``True`` is ``{"keep_lost": 0}``; a dict gives ``"keep_lost"``."""
    if value is None:
        value = eng_cfg.get("track_ids", None)
    if not value:
        return None
    opts = {"keep_lost": 0}
    if isinstance(value, dict):
        unknown = set(value) - set(opts)
        if unknown:
            raise ValueError("track_ids: unknown keys %s" % sorted(unknown))
        opts.update(value)
    opts["keep_lost"] = int(opts["keep_lost"])
    if not 0 <= opts["keep_lost"] <= 255:
        raise ValueError("track_ids: keep_lost must be in [0, 255]")
    return opts


def spare_select(ids, spare) -> np.ndarray:
    """``select`` of pf_face_redact / pf_redact_faces from the rows' ids: 0 (not redacted) where the id is spared, 1 elsewhere."""
    spare = set(int(v) for v in (spare or ()))
    return np.asarray([0 if int(i) in spare else 1 for i in np.asarray(ids).reshape(-1)], np.int32)

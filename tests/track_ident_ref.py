"""numpy restatement of the identity rule (include/peppa_hip.h, "Persistent face ids", steps 1-6), written from the text of the
rule and independent of the package's host implementation (core/smoother/ident.py).  It takes the per-frame arrays the stages
see: the previous track boxes, the NMS boxes of a detector frame (None on a gated frame), the input row of every selected row,
the valid flags of the landmark stage and the new track boxes."""
import numpy as np

LOST_CAP = 64


def new_state():
    return {"id": np.zeros(0, np.int64), "age": np.zeros(0, np.int64), "next": 1,
            "lost": []}          # each entry: dict(id, age, box float64 [4], gone), insertion order


def forget(state):
    """What a reset does: ids, ages and the lost list go, the counter stays."""
    state["id"], state["age"], state["lost"] = np.zeros(0, np.int64), np.zeros(0, np.int64), []


def _iou(a, b):
    """Intersection over union, in float32 when both boxes are float32 and in float64 otherwise, one rounding per operation."""
    t = np.float32 if (a.dtype == np.float32 and b.dtype == np.float32) else np.float64
    a, b = a[:4].astype(t), b[:4].astype(t)
    zero = t(0)
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    iw = np.maximum(zero, np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]))
    ih = np.maximum(zero, np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]))
    inter = iw * ih
    with np.errstate(all="ignore"):
        return np.float64(inter / ((area_a + area_b) - inter))


def step(state, prev_track, nms, sel_rows, valid, new_track, keep_lost, thres=0.5):
    """One frame; returns (ids, ages) of the output rows.  prev_track: [P,4] or None (no track); nms: [N,>=4] of a detector frame
    or None; sel_rows[q]: row of nms (detector frame) or of prev_track (gated frame) that selected row q is."""
    thres = float(np.float32(thres))
    prev_id, prev_age = state["id"], state["age"]
    P = 0 if prev_track is None else min(len(prev_track), len(prev_id))
    # 1. source and weight of every selected row
    source, weight = [], []
    for q, r in enumerate(sel_rows):
        j, w = None, 0.0
        if nms is not None:
            if prev_track is not None:
                for cand in range(len(prev_track)):
                    v = _iou(np.asarray(nms[r]), np.asarray(prev_track[cand]))
                    if v > thres:
                        j, w = cand, float(v)
                        break
        else:
            j = int(r)
        if j is not None and (j >= P or prev_id[j] == 0):
            j = None
        source.append(j)
        weight.append(w)
    # 2. output rows
    out = [q for q in range(len(sel_rows)) if valid[q]]
    source, weight = [source[q] for q in out], [weight[q] for q in out]
    assert len(out) == len(new_track)
    # 3. conflicts
    for j in set(x for x in source if x is not None):
        rows = [o for o in range(len(out)) if source[o] == j]
        winner = max(rows, key=lambda o: (weight[o], -o))
        for o in rows:
            if o != winner:
                source[o] = None
    ids, ages = np.zeros(len(out), np.int64), np.zeros(len(out), np.int64)
    taken = set()
    for o in range(len(out)):
        if source[o] is not None:                                  # 4.
            ids[o], ages[o] = prev_id[source[o]], prev_age[source[o]] + 1
            continue
        pick = None                                                # 5.
        if keep_lost > 0:
            scores = [(_iou(np.asarray(new_track[o], np.float64), ent["box"]), e) for e, ent in enumerate(state["lost"]) if e not in taken]
            scores = [(v, e) for v, e in scores if v > thres]
            if scores:
                top = max(v for v, _ in scores)
                pick = min(e for v, e in scores if v == top)
        if pick is None:
            ids[o], ages[o] = state["next"], 1
            state["next"] += 1
        else:
            taken.add(pick)
            ids[o], ages[o] = state["lost"][pick]["id"], state["lost"][pick]["age"] + 1
    # 6. the lost list
    lost = [dict(ent, gone=ent["gone"] + 1) for e, ent in enumerate(state["lost"]) if e not in taken]
    lost = [ent for ent in lost if ent["gone"] <= keep_lost]
    kept = set(x for x in source if x is not None)
    for j in range(P):
        if prev_id[j] != 0 and j not in kept:
            lost.append(dict(id=int(prev_id[j]), age=int(prev_age[j]), box=np.asarray(prev_track[j][:4], np.float64).copy(), gone=1))
    while len(lost) > LOST_CAP:
        worst = max(ent["gone"] for ent in lost)
        lost.pop([ent["gone"] for ent in lost].index(worst))
    state["lost"] = lost if keep_lost > 0 else []
    state["id"], state["age"] = ids, ages
    return ids.copy(), ages.copy()

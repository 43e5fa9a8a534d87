"""The video of the persistent-id tests (tests/test_track_ident.py): named segments in the manner of
tracking_video.video_edges(), each hand-stating, per frame, which planted face every output row is and the id and age it must
carry.  The expectations follow from which planted face a row is -- ground truth by construction -- and from the identity rule
of include/peppa_hip.h, never from code under test.  Conventions of video_long() / video_edges(): scene() frames, plant_rows()
rows for the 384 x 640 detector, S_LONG crops with long_video_weights, top_k = 5, face widths that are no multiple of 5.  NMS
returns the planted boxes in REVERSE planting order, and with at most top_k boxes over min_face that is the row order.

A segment is a dict: name, hw, frames, rows, faces (planted (cx, cy, w, h) per frame), min_face and expect -- keep_lost ->
dict(row_face, ids, ages[, any_order: frames whose rows are stated per face, in no particular order]), ids counted from 1 as on a tracker that has handed out none before (a test adds the ids the tracker
used earlier).  episodes() is the order the tests play them in.

carry            three faces, a gated repeat, a 5-pixel shift on a detector frame: ids {1, 2, 3} stay on the same faces.
reorder          three faces; a fourth, larger one, planted last, takes row 0 (id 4) and the others move down with their ids;
                 seven faces with top_k = 5: the five largest survive in area order, the kept ones keep their ids, A (the
                 smallest of the tracked ones, smaller than both newcomers E and F) is dropped and loses its id, E and F get 5
                 and 6 (E is the larger, so the earlier row); then B, E and G leave and A is back: the survivors C, F, D keep their ids in
                 changed rows, A is a new face (7) -- with keep_lost = 0 nothing is remembered.  The areas sort_and_filter
                 compares on that frame are those of the SMOOTHED boxes, which depend on the networks, so the expectation of
                 that frame is stated per planted face (expect["any_order"]), not per row.
rejected_crop    video_edges' layout: five selected, the 18 x 130 one rejected by the crop stage, four rows; two gated repeats,
                 then the same layout on a detector frame: selected rows 3 and 4 are output rows 2 and 3 and keep ids 3 and 4.
duplicate_claim  one face whose track box takes the whole 101-wide planted box in; then two detections inside it, its left 64
                 and its right 62 columns: both are over 0.5 against the track box and 0.25 against each other, so NMS keeps
                 both and both claim track row 0.  The 64 columns are output row 1 and win (greatest weight); row 0 is new.
duplicate_equal  the same with the left 62 and the right 62 columns, whose float32 areas are bit-equal: for a box inside the
                 track box the judge's IoU is area / (area + track area - area), so the weights are bit-equal and row 0 wins.
iou_first        video_edges' layout: the single detection of the last frame is over 0.5 against both track rows and takes the
                 id of the first.
lost_and_found   video_edges' `empty` layout: three faces, three frames without a face (one detector frame, two gated), the
                 faces back 6 pixels away.  keep_lost 0: new ids 4, 5, 6.  keep_lost 3: `gone` is 3 when they return, 3 > 3 is
                 false, ids 1, 2, 3 with age 2.  keep_lost 2: the entries were dropped when `gone` reached 3: ids 4, 5, 6."""
import numpy as np

from tests import track_ident_ref as ref
from tests.tracking_video import HW_EDGES, nms_boxes, scene
from peppa_pig_face_landmark_amd.synth import plant_rows

HW_SMALL = (270, 480)
TRACK_IOU = 0.5
NMS_IOU = 0.3


def _rows(faces, hw, seed):
    b = np.asarray([[cx - fw / 2, cy - fh / 2, cx + fw / 2, cy + fh / 2] for cx, cy, fw, fh in faces], np.float32).reshape(-1, 4)
    return plant_rows(b, hw, 15120, (384, 640), 6, seed=seed)


def _segment(name, hw, layouts, seeds, seed0, expect, min_face=1600.0):
    return dict(name=name, hw=hw, faces=layouts, min_face=float(min_face), expect=expect,
                frames=[scene(hw[0], hw[1], lay, s)[0] for lay, s in zip(layouts, seeds)],
                rows=[_rows(lay, hw, seed0 + i) for i, lay in enumerate(layouts)])


def _expect(row_face, ids, ages):
    return dict(row_face=row_face, ids=ids, ages=ages)


# the 101-wide face of the duplicate_* segments and the columns of it the second frame plants
# (cx = 241 is one of the positions at which NMS returns the two 62-column boxes with bit-equal float32 areas, 8059.997)
DUP_FACE = (241, 135, 101, 130)
DUP_LEFT64, DUP_RIGHT62, DUP_LEFT62 = (222.5, 135, 64, 130), (260.5, 135, 62, 130), (221.5, 135, 62, 130)


def video_ident():
    segs = []
    sh = lambda fs, dx: [(cx + dx, cy, fw, fh) for cx, cy, fw, fh in fs]           # noqa: E731
    A, B, C = (70, 80, 64, 84), (200, 180, 81, 104), (380, 90, 72, 94)
    # carry
    segs.append(_segment("carry", HW_SMALL, [[A, B, C], [A, B, C], sh([A, B, C], 5)], [21, 21, 22], 600,
                         {0: _expect([[2, 1, 0]] * 3, [[1, 2, 3]] * 3, [[1, 1, 1], [2, 2, 2], [3, 3, 3]])}))
    # reorder: planted areas D 10556 > E 8798 > B 8424 > F 7900 > C 6768 > A 5376 > G 3366
    D, E, F, G = (330, 200, 91, 116), (60, 210, 83, 106), (200, 58, 79, 100), (440, 210, 51, 66)
    segs.append(_segment("reorder", HW_SMALL, [[A, B, C], [A, B, C, D], [A, B, C, D, E, F, G], [D, A, F, C]], [23, 24, 25, 26], 610,
                         {0: dict(_expect([[2, 1, 0], [3, 2, 1, 0], [3, 1, 2, 4, 5], [3, 2, 1, 0]],
                                          [[1, 2, 3], [4, 1, 2, 3], [4, 2, 1, 5, 6], [1, 6, 7, 4]],
                                          [[1, 1, 1], [1, 2, 2, 2], [2, 3, 3, 1, 1], [4, 2, 1, 3]]), any_order=[2])}))
    # rejected_crop
    six = [(70, 75, 91, 116), (200, 70, 74, 96), (300, 80, 18, 130), (390, 60, 42, 52), (120, 210, 38, 49), (280, 215, 34, 50)]
    segs.append(_segment("rejected_crop", HW_EDGES, [six] * 4, [78, 78, 78, 79], 620,
                         {0: _expect([[0, 1, 3, 4]] * 4, [[1, 2, 3, 4]] * 4, [[k] * 4 for k in (1, 2, 3, 4)])}))
    # duplicate_claim / duplicate_equal
    segs.append(_segment("duplicate_claim", HW_EDGES, [[DUP_FACE], [DUP_LEFT64, DUP_RIGHT62]], [90, 91], 630,
                         {0: _expect([[0], [1, 0]], [[1], [2, 1]], [[1], [1, 2]])}))
    segs.append(_segment("duplicate_equal", HW_EDGES, [[DUP_FACE], [DUP_LEFT62, DUP_RIGHT62]], [90, 92], 640,
                         {0: _expect([[0], [1, 0]], [[1], [1, 2]], [[1], [2, 1]])}))
    # iou_first
    pair = [(240, 120, 52, 32), (240, 139, 52, 32)]
    between = [(237.5, 134, 81, 82)]
    segs.append(_segment("iou_first", HW_EDGES, [pair, pair, pair, between], [61, 61, 61, 74], 430,
                         {0: _expect([[1, 0]] * 3 + [[0]], [[1, 2]] * 3 + [[1]], [[1, 1], [2, 2], [3, 3], [4]])}, min_face=1200))
    # lost_and_found
    three = [(90, 90, 52, 68), (240, 170, 64, 84), (400, 100, 58, 76)]
    moved = [(96, 96, 52, 68), (246, 164, 64, 84), (394, 106, 58, 76)]
    fresh = _expect([[2, 1, 0], [], [], [], [2, 1, 0]], [[1, 2, 3], [], [], [], [4, 5, 6]], [[1, 1, 1], [], [], [], [1, 1, 1]])
    found = _expect([[2, 1, 0], [], [], [], [2, 1, 0]], [[1, 2, 3], [], [], [], [1, 2, 3]], [[1, 1, 1], [], [], [], [2, 2, 2]])
    segs.append(_segment("lost_and_found", HW_EDGES, [three, [], [], [], moved], [75, 76, 76, 76, 77], 450, {0: fresh, 3: found, 2: fresh}))
    return segs


def episodes(segs=None):
    """[(segment, keep_lost)] in playing order: a tracker is reset between episodes and reconfigured (ids restart at 1) where
    keep_lost changes."""
    segs = segs if segs is not None else video_ident()
    out = [(s, 0) for s in segs]
    laf = [s for s in segs if s["name"] == "lost_and_found"][0]
    return out + [(laf, 3), (laf, 2)]


# ---- numpy-only evidence that the edges are hit ---------------------------------------------------------------------------
def _iou32(a, b):
    """IoU as the judge computes it for two float32 boxes (csrc/k_track.h pf_box_iou_f32): every operation rounded to float32."""
    a, b = np.asarray(a[:4], np.float32), np.asarray(b[:4], np.float32)
    s1 = (a[2] - a[0]) * (a[3] - a[1])
    s2 = (b[2] - b[0]) * (b[3] - b[1])
    inter = np.maximum(np.float32(0), np.minimum(a[2], b[2]) - np.maximum(a[0], b[0])) * \
        np.maximum(np.float32(0), np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]))
    assert inter.dtype == np.float32 and s1.dtype == np.float32
    return inter / ((s1 + s2) - inter)


def numpy_evidence(segs=None):
    """What numpy alone says about the fixture.  The track box of the duplicate_* segments is not known without the networks; the
    planted box stands in for it here (the tests check on the tracker's own arrays that the track box takes it in, which makes the
    judge's IoU of a detection inside it area / track area, monotonic and tie-preserving in the detection's area)."""
    by = {s["name"]: s for s in (segs if segs is not None else video_ident())}
    ev = {}
    for name in ("duplicate_claim", "duplicate_equal"):
        s = by[name]
        face = nms_boxes(s["rows"][0], s["hw"])
        now = nms_boxes(s["rows"][1], s["hw"])
        assert len(face) == 1 and len(now) == 2
        ev[name + "_iou"] = np.asarray([_iou32(b, face[0]) for b in now], np.float32)          # NMS order = output rows
        ev[name + "_mutual"] = np.float32(_iou32(now[0], now[1]))
        ev[name + "_areas"] = np.asarray([(b[2] - b[0]) * (b[3] - b[1]) for b in now[:, :4].astype(np.float32)], np.float32)
    s = by["lost_and_found"]
    over = [int((r[:, 4] > 0.5).sum()) for r in s["rows"]]
    ev["absent_frames"] = np.int64(sum(1 for n in over[1:-1] if n == 0))
    ev["lost_rows_over_thres"] = np.asarray(over, np.int64)
    # `gone` at the boundary: the restatement of the rule replayed on the planted boxes, which stand in for the track boxes (the
    # frames without a row over the threshold have no selected rows, whether the detector ran or the gate repeated the empty
    # track).  With keep_lost 255 nothing expires, so the lost list in front of the last frame shows how long the faces were gone.
    def replay(keep_lost):
        st, out = ref.new_state(), None
        prev = None
        for k, r in enumerate(s["rows"]):
            b = nms_boxes(r, s["hw"])[:, :4].astype(np.float64) if over[k] else np.zeros((0, 4))
            if k == len(s["rows"]) - 1:
                gone = [e["gone"] for e in st["lost"]]
                back = [max([ref._iou(x, e["box"]) for e in st["lost"]] or [0.0]) for x in b]
            out = ref.step(st, prev, b, list(range(len(b))), np.ones(len(b), bool), b, keep_lost, TRACK_IOU)
            prev = b
        return gone, back, out
    ev["gone_on_return"], ev["return_iou"], _ = replay(255)
    ev["return_ids"] = {kl: replay(kl)[2][0].tolist() for kl in s["expect"]}
    ev["return_ages"] = {kl: replay(kl)[2][1].tolist() for kl in s["expect"]}
    b = nms_boxes(by["reorder"]["rows"][2], by["reorder"]["hw"])
    ev["reorder_areas"] = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(np.float32)           # NMS order: G F E D C B A
    return ev

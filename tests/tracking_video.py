"""The short synthetic video of the frame-to-frame tests (tests/test_tracking_parity.py) and of the golden vector the
reference's own facer.py / lk.py produced for it (tests/golden/make_tracking_golden.py)."""
import os

import numpy as np

from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking_video.npz")
S = 64          # landmark crop size of these tests


def video():
    """5 frames: f0, f0 again (static: detector skipped, float64 track boxes feed the landmark stage), a shifted scene
    (detector runs, IoU-matched boxes are EMA-smoothed), the same again, and a frame with one face fewer."""
    f0, b0 = make_frame(270, 480, 3, seed=11, face_w=330, face_h=430)
    f1 = np.roll(f0, 6, axis=1)
    b1 = b0 + np.float32([6, 0, 6, 0])
    f2, b2 = make_frame(270, 480, 2, seed=12, face_w=330, face_h=430)
    frames = [f0, f0, f1, f1, f2]
    boxes = [b0, b0, b1, b1, b2]
    rows = [plant_rows(b, (270, 480), 15120, (384, 640), 6, seed=3 + i) for i, b in enumerate(boxes)]
    return frames, rows


# ---- the long video (round 3) -------------------------------------------------------------------------------------------------
GOLDEN_LONG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking_video_long.npz")
S_LONG = 128    # landmark crop size of the long video


def scene(h, w, faces, seed):
    """BGR uint8 frame with one ellipse-face per (cx, cy, width, height) entry; returns (frame, boxes_xyxy float32)."""
    rng = np.random.default_rng(seed)
    frame = np.clip(np.rint(114 + rng.normal(0, 6, (h, w, 3))), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    boxes = []
    for cx, cy, fw, fh in faces:
        frame[((xx - cx) / (fw / 2)) ** 2 + ((yy - cy) / (fh / 2)) ** 2 <= 1.0] = (140, 170, 210)
        for dx, dy, r in ((-0.2, -0.15, 0.09), (0.2, -0.15, 0.09), (0.0, 0.25, 0.14)):
            frame[(xx - (cx + dx * fw)) ** 2 + (yy - (cy + dy * fh)) ** 2 <= (r * fw) ** 2] = (40, 40, 60)
        boxes.append([cx - fw / 2, cy - fh / 2, cx + fw / 2, cy + fh / 2])
    return frame, np.asarray(boxes, np.float32)


def long_video_weights(student_weights):
    """The BN-calibrated synthetic Student with its 2 x 98 offset channels damped: random-init offsets are tens of heat-map
    cells, which throws landmarks (and the hull boxes the tracker makes from them) thousands of pixels out of the crop; at
    1/50 they stay within a cell, landmarks stay inside the crop, and parity can be judged in absolute pixels."""
    w = dict(student_weights)
    hw, hb = np.array(w["hm.weight"], np.float32), np.array(w["hm.bias"], np.float32)
    hw[98:] *= np.float32(0.02)
    hb[98:] *= np.float32(0.02)
    w["hm.weight"], w["hm.bias"] = hw, hb
    return w


def video_long():
    """13 frames in two segments (reset() between them -- the frame size changes).  What the frames exercise, in order:
    three faces; two repeats of the same frame (the difference gate closes: detector skipped, float64 track boxes feed the
    landmark stage, One-Euro history grows); a 5-pixel shift (gate opens, IoU-matched boxes are EMA-smoothed); a fourth face
    enters; seven faces of distinct sizes (more than top_k = 5: the five largest survive); the same frame again; three of
    them leave; down to two faces; the two shift; then 360 x 640 frames after reset(): three faces, a repeat, a shift.
    Returns [(frames, planted rows, (h, w))] per segment.

    Face widths avoid multiples of 5: FaceLandmark.preprocess computes ``face_width = 1.4 * w`` (face_landmark.py:83), which
    for a float32 ``w`` is a float64 product under the reference's pinned numpy 1.23 (1.4 * 90 = 125.99999999999999, // 2 =
    62) and a float32 one under numpy >= 2 (126.0, // 2 = 63): the engine follows the pinned version, the reference executed
    in this container follows numpy 2, and the two differ exactly where 1.4 w is an integer."""
    h, w = 270, 480
    A, B, C = (70, 80, 64, 84), (200, 180, 81, 104), (380, 90, 72, 94)
    D = (330, 200, 58, 76)
    seven = [(60, 70, 51, 66), (180, 70, 58, 76), (300, 70, 66, 86), (420, 70, 74, 96),
             (60, 200, 82, 106), (190, 200, 62, 80), (320, 200, 91, 116)]
    sh = lambda fs, dx: [(cx + dx, cy, fw, fh) for cx, cy, fw, fh in fs]           # noqa: E731
    layouts = [[A, B, C], [A, B, C], [A, B, C], sh([A, B, C], 5), sh([A, B, C], 5) + [D], seven, seven,
               [seven[3], seven[4], seven[6], seven[2]], [seven[4], seven[6]], sh([seven[4], seven[6]], 7)]
    seeds = [21, 21, 21, 22, 23, 24, 24, 25, 26, 27]
    seg1 = [scene(h, w, lay, seed) for lay, seed in zip(layouts, seeds)]
    h2, w2 = 360, 640
    E, F, G = (120, 120, 96, 124), (330, 220, 111, 142), (520, 130, 88, 114)
    lay2 = [[E, F, G], [E, F, G], sh([E, F, G], 6)]
    seg2 = [scene(h2, w2, lay, seed) for lay, seed in zip(lay2, [31, 31, 32])]
    out = []
    for seg, hw in ((seg1, (h, w)), (seg2, (h2, w2))):
        frames = [f for f, _ in seg]
        rows = [plant_rows(b, hw, 15120, (384, 640), 6, seed=40 + i) for i, (_, b) in enumerate(seg)]
        out.append((frames, rows, hw))
    return out


# ---- the edge video: every decision of the tracker at its boundary, on a frame whose byte count is no multiple of 16 ----------
GOLDEN_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking_video_edges.npz")
HW_EDGES = (271, 483)       # 271 * 483 * 3 = 392679 = 16 * 24542 + 7: the stream gate takes its byte loop for the tail


def _planted(faces_per_frame, seed0, hw=HW_EDGES):
    rows = []
    for i, faces in enumerate(faces_per_frame):
        b = np.asarray([[cx - fw / 2, cy - fh / 2, cx + fw / 2, cy + fh / 2] for cx, cy, fw, fh in faces], np.float32).reshape(-1, 4)
        rows.append(plant_rows(b, hw, 15120, (384, 640), 6, seed=seed0 + i))
    return rows


def nms_boxes(rows, hw=HW_EDGES):
    """What the reference's detector stage returns for planted rows (numpy restatement: xywh2xyxy, py_nms, scale_coords)."""
    from oracle import prepost as pp
    s, _, _, top, _, left, _ = pp.letterbox_geometry(hw[0], hw[1], (384, 640))
    return pp.detector_postprocess(rows, [s, left, top], 0.3, 0.5)


def video_edges():
    """22 frames of 271 x 483 in seven segments with reset() between them, each named after the decision it puts on its
    boundary.  Conventions of video_long(): scene() frames, plant_rows() rows for the 384 x 640 detector, S_LONG crops with
    long_video_weights, top_k = 5, face widths that are no multiple of 5 (see video_long: 1.4 * w).  A segment is a dict:
    name, group ("A": the reference itself runs it; "B": the reference raises, the engine's documented behaviour decides),
    frames, rows, faces (the planted (cx, cy, w, h) per frame), hw, min_face, and expect -- hand-stated counts, detector_ran
    and, per frame, which planted face each output row is.  NMS returns the planted boxes in REVERSE planting order (the
    k-th planted box scores 0.99 + 0.0005 k), which is what "earlier / later row" refers to below.

    gate_equal       f, f + 5 on every byte (mean difference exactly 5.0: `diff > 5` is false, the detector is skipped),
                     that + 5 with one byte + 6 (sum 5 N + 1: it runs), that - 5 with one byte - 4 (5 N - 1: skipped).
    min_face_equal   min_face is the float32 area NMS returns for the first planted face (46 x 58 at x = 62: 2667.99976,
                     one ulp under 2668); the same face at x = 160 comes back as 2668.0.  Strict `>` drops the first only.
    equal_areas      seven faces; the 5th and 6th by area (58 x 76 at x = 60 and x = 180) come back with bit-equal float32
                     areas (4408.0).  top_k = 5 keeps one: the later row (x = 60), as the reversed ascending argsort does.
    iou_first        two flat faces 19 px apart (box IoU 0.26, under the NMS threshold) whose landmark hulls and track
                     boxes overlap heavily; two gated repeats give GroupTrack two previous hulls above 0.5 for one face, then a
                     detector frame plants one face on the SECOND track box: its IoU with both exceeds 0.5, the first wins.
    one_euro         a 26 x 36 face (min_face 300) and a gated repeat: one of its 98 points moves less than 0.002 of the
                     frame (al = 0.01), the others more.  With the random-weight Student every crop change moves almost
                     every point, so frozen points are rare; this layout has one.
    empty            three faces, a changed frame with no row above the score threshold (detector runs, zero faces, the
                     track stays -- empty), the same frame twice (gate closed, zero faces), a changed frame with three faces.
    rejected_crop    (B) six faces, five selected by area; the third of them is 18 x 130 (area 2340 > min_face, width <= 20),
                     which the landmark stage rejects: four rows come back, the two after it one row up, and stay so on two
                     gated repeats.  The reference dereferences None there (face_landmark.py:76-77, :44)."""
    h, w = HW_EDGES
    segs = []

    def seg(name, group, faces, seeds, seed0, min_face, expect, frames=None):
        fr = frames if frames is not None else [scene(h, w, f, s)[0] for f, s in zip(faces, seeds)]
        segs.append(dict(name=name, group=group, frames=fr, rows=_planted(faces, seed0), faces=faces, hw=(h, w),
                         min_face=float(min_face), expect=expect))

    # gate_equal
    two = [(120, 100, 52, 68), (330, 150, 64, 84)]
    f0 = np.minimum(scene(h, w, two, 71)[0], 240)
    f1 = f0 + 5
    f2 = f1 + 5
    f2[0, 0, 0] += 1
    f3 = f2 - 5
    f3[h - 1, w - 1, 2] += 1                                   # the last byte of the frame: the tail of the byte loop
    seg("gate_equal", "A", [two] * 4, None, 400, 1600, dict(counts=[2, 2, 2, 2], detector_ran=[1, 0, 1, 0], row_face=[[1, 0]] * 4),
        frames=[f0, f1, f2, f3])
    # min_face_equal
    mf = [(62, 100, 46, 58), (160, 100, 46, 58), (330, 150, 64, 84)]
    min_face = nms_boxes(_planted([mf], 410)[0])[2]      # the first planted face is the last NMS row
    min_face = np.float32(min_face[2] - min_face[0]) * np.float32(min_face[3] - min_face[1])
    seg("min_face_equal", "A", [mf] * 2, [72, 72], 410, min_face, dict(counts=[2, 2], detector_ran=[1, 0], row_face=[[2, 1]] * 2))
    # equal_areas
    seven = [(60, 70, 58, 76), (180, 70, 58, 76), (300, 70, 66, 86), (420, 70, 74, 96),
             (60, 200, 82, 106), (190, 200, 51, 66), (320, 200, 91, 116)]
    seg("equal_areas", "A", [seven] * 2, [73, 73], 420, 1600, dict(counts=[5, 5], detector_ran=[1, 0], row_face=[[6, 4, 3, 2, 0]] * 2))
    # iou_first
    pair = [(240, 120, 52, 32), (240, 139, 52, 32)]
    between = [(237.5, 134, 81, 82)]
    seg("iou_first", "A", [pair, pair, pair, between], [61, 61, 61, 74], 430, 1200,
        dict(counts=[2, 2, 2, 1], detector_ran=[1, 0, 0, 1], row_face=[[1, 0]] * 3 + [[0]]))
    # one_euro
    tiny = [(222, 130, 26, 36)]
    seg("one_euro", "A", [tiny] * 2, [62, 62], 440, 300, dict(counts=[1, 1], detector_ran=[1, 0], row_face=[[0]] * 2))
    # empty
    three = [(90, 90, 52, 68), (240, 170, 64, 84), (400, 100, 58, 76)]
    moved = [(96, 96, 52, 68), (246, 164, 64, 84), (394, 106, 58, 76)]
    seg("empty", "A", [three, [], [], [], moved], [75, 76, 76, 76, 77], 450, 1600,
        dict(counts=[3, 0, 0, 0, 3], detector_ran=[1, 1, 0, 0, 1], row_face=[[2, 1, 0], [], [], [], [2, 1, 0]]))
    # rejected_crop
    six = [(70, 75, 91, 116), (200, 70, 74, 96), (300, 80, 18, 130), (390, 60, 42, 52), (120, 210, 38, 49), (280, 215, 34, 50)]
    seg("rejected_crop", "B", [six] * 3, [78, 78, 78], 460, 1600,
        dict(counts=[4, 4, 4], detector_ran=[1, 0, 0], row_face=[[0, 1, 3, 4]] * 3, n_sel=5, n_valid=4))
    return segs

"""Face overlay: the integer restatement of the rule the engine's pf_draw_faces specifies, written from that
specification and not from the kernels.  A helper of tests/test_face_draw.py and tests/test_gpu_face_draw.py, not a test.

``frame_cover(kps, count, scores, H, W, what, r, w, thres)`` -> (colour index per pixel, -1 = uncovered; valid [K]);
``frame_reference(frame, kps, ...)`` -> (the drawn frame, valid, number of covered pixels).  Python integers and int64 only: the
largest term, 64 w^2 len2, stays below 2^58."""
import numpy as np

from tests import mask_ref as mr

POINTS, CONTOURS, BOX = 1, 2, 4
HI, LO, CONTOUR, BOXC = 0, 1, 2, 3
DEFAULT_COLOURS = ((255, 255, 255), (0, 0, 255), (0, 255, 0), (255, 255, 0))          # hi, lo, contour, box; channel 0 first


def _window(lo, hi, size):
    """Pixels p of [0, size) with lo <= 16 p <= hi -> (first, one past the last): only an economy, the tests inside decide."""
    return max(-(-lo // 16), 0), min(hi // 16 + 1, size)


def _disc(cover, cx, cy, R, H, W):
    """|P - C|^2 <= R^2 over the frame -> bool [H,W] (evaluated inside the disc's bounding window)."""
    x0, x1 = _window(cx - R, cx + R, W)
    y0, y1 = _window(cy - R, cy + R, H)
    if x0 >= x1 or y0 >= y1:
        return
    qx = 16 * np.arange(x0, x1, dtype=np.int64)[None, :] - cx
    qy = 16 * np.arange(y0, y1, dtype=np.int64)[:, None] - cy
    cover[y0:y1, x0:x1] |= qx * qx + qy * qy <= R * R


def _edge(cover, ax, ay, bx, by, w, H, W):
    R = 8 * w
    _disc(cover, ax, ay, R, H, W)
    _disc(cover, bx, by, R, H, W)
    dx, dy = bx - ax, by - ay
    len2 = dx * dx + dy * dy
    if len2 == 0:
        return
    x0, x1 = _window(min(ax, bx) - R, max(ax, bx) + R, W)
    y0, y1 = _window(min(ay, by) - R, max(ay, by) + R, H)
    if x0 >= x1 or y0 >= y1:
        return
    qx = 16 * np.arange(x0, x1, dtype=np.int64)[None, :] - ax
    qy = 16 * np.arange(y0, y1, dtype=np.int64)[:, None] - ay
    dot = qx * dx + qy * dy
    cross = qx * dy - qy * dx                                 # |cross| < 2^43: the square would not fit, so compare in Python integers
    lim = 64 * w * w * len2
    root = int(np.sqrt(float(lim)))
    while root * root > lim:
        root -= 1
    while (root + 1) * (root + 1) <= lim:
        root += 1                                             # root^2 <= lim < (root + 1)^2, hence cross^2 <= lim iff |cross| <= root
    cover[y0:y1, x0:x1] |= (dot >= 0) & (dot <= len2) & (np.abs(cross) <= root)


def slot_cover(kps, scores, H, W, what, r, w, thres):
    """One valid slot -> colour index int8 [H,W], -1 where nothing of it covers the pixel: the box first, the contours over it, the
    points over those in rising index, so that the last writer is the winner the specification names."""
    k = np.asarray(kps).astype(np.float64)
    q = mr.q4(np.where(np.isfinite(k), k, 0.0))           # only a pupil can be not finite here, and then it is not drawn
    X, Y = [int(v) for v in q[:, 0]], [int(v) for v in q[:, 1]]
    idx = np.full((H, W), -1, np.int8)
    if what & BOX:
        x0, y0, x1, y1 = (int(v) for v in mr.box_of(q[:, 0], q[:, 1], H, W))
        if x1 > x0 and y1 > y0:
            ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
            outer = (xs >= x0 - w) & (xs < x1 + w) & (ys >= y0 - w) & (ys < y1 + w)
            inner = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
            idx[outer & ~inner] = BOXC
    if what & CONTOURS:
        cover = np.zeros((H, W), bool)
        for label in sorted(mr.REGIONS):
            poly = mr.REGIONS[label]
            for j in range(len(poly)):
                a, b = poly[j], poly[(j + 1) % len(poly)]
                _edge(cover, X[a], Y[a], X[b], Y[b], w, H, W)
        idx[cover] = CONTOUR
    if what & POINTS:
        thres32 = np.float32(thres)
        for i in range(98):
            if i >= 96 and not np.isfinite(k[i]).all():
                continue
            cover = np.zeros((H, W), bool)
            _disc(cover, X[i], Y[i], 16 * r, H, W)
            hi = scores is None or bool(np.float32(scores[i]) > thres32)          # NaN and equality: lo
            idx[cover] = HI if hi else LO
    return idx


def frame_cover(kps, count, scores, H, W, what, r, w, thres=0.8):
    """kps [K,98,2] of one frame, count live slots (None: all), scores [K,98] or None -> (colour index int8 [H,W], valid bool [K]):
    the lowest valid slot that covers a pixel decides it."""
    K = len(kps)
    idx = np.full((H, W), -1, np.int8)
    valid = np.zeros((K,), bool)
    for k in range(K):
        if (count is not None and k >= count) or not mr.finite96(kps[k]):
            continue
        valid[k] = True
        s = slot_cover(kps[k], None if scores is None else np.asarray(scores)[k], H, W, what, r, w, thres)
        take = (s >= 0) & (idx < 0)
        idx[take] = s[take]
    return idx, valid


def blend(frame, idx, alpha, colours=DEFAULT_COLOURS):
    """One colour, once: (in (256 - a) + c a + 128) >> 8 per channel where idx >= 0, the input elsewhere."""
    table = np.array([[int(v) & 255 for v in c] for c in colours], np.int64)
    c = table[np.maximum(idx, 0)]
    mixed = (frame.astype(np.int64) * (256 - alpha) + c * alpha + 128) >> 8
    return np.where((idx >= 0)[:, :, None], mixed, frame).astype(np.uint8)


def frame_reference(frame, kps, count=None, scores=None, what=POINTS, r=2, w=1, alpha=256, thres=0.8, colours=DEFAULT_COLOURS):
    """-> (drawn frame, valid [K], number of covered pixels)."""
    H, W = frame.shape[:2]
    idx, valid = frame_cover(kps, count, scores, H, W, what, r, w, thres)
    return blend(frame, idx, alpha, colours), valid, int((idx >= 0).sum())

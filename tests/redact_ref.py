"""Face redaction: the integer restatement of the arithmetic the engine's pf_redact_faces specifies, written from
that specification and not from the kernel.  A helper of tests/test_face_redact.py and tests/test_gpu_face_redact.py, not a test.

``selected(maps, select, label_mask, pad)`` -> which pixels of a frame are selected, from the (labels, owners, boxes, valid) of
tests/mask_ref.py; ``apply(frame, sel, mode, strength, colour)`` -> the redacted frame; ``frame_reference(...)`` -> both for one
frame's landmarks."""
import numpy as np

from tests import mask_ref as mr

FILL, MOSAIC, BLUR = 0, 1, 2
BACKGROUND, FACE_ALL, BOX = 0x001, 0x1FE, 0x200


def selected(maps, select, label_mask, pad=0):
    """maps = (labels [H,W], owners [H,W], boxes [K,4], valid [K]); select [K] or None -> bool [H,W]."""
    labels, owners, boxes, valid = maps
    H, W = labels.shape
    K = len(valid)
    chosen = np.ones((K,), bool) if select is None else np.asarray(select).reshape(K) != 0
    bit = ((int(label_mask) >> labels.astype(np.int64)) & 1).astype(bool)
    owner_chosen = np.concatenate([[True], chosen])[owners]          # background pixels (owner 0) need no slot
    sel = bit & ((labels == 0) | owner_chosen)
    if int(label_mask) & BOX:
        ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
        for k in range(K):
            x0, y0, x1, y1 = (int(v) for v in boxes[k])
            if valid[k] and chosen[k] and x1 > x0 and y1 > y0:
                sel |= (xs >= x0 - pad) & (xs < x1 + pad) & (ys >= y0 - pad) & (ys < y1 + pad)
    return sel


def _mosaic(frame, c):
    H, W = frame.shape[:2]
    out = np.empty_like(frame)
    for y0 in range(0, H, c):
        for x0 in range(0, W, c):
            cell = frame[y0:y0 + c, x0:x0 + c].astype(np.int64)
            n = cell.shape[0] * cell.shape[1]
            out[y0:y0 + c, x0:x0 + c] = (cell.sum((0, 1)) + (n >> 1)) // n
    return out


def _blur(frame, r):
    H, W = frame.shape[:2]
    acc = np.zeros((H + 1, W + 1, 3), np.int64)
    acc[1:, 1:] = frame.astype(np.int64).cumsum(0).cumsum(1)
    ylo, yhi = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r, H - 1) + 1
    xlo, xhi = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r, W - 1) + 1
    s = acc[yhi][:, xhi] - acc[ylo][:, xhi] - acc[yhi][:, xlo] + acc[ylo][:, xlo]
    n = ((yhi - ylo)[:, None] * (xhi - xlo)[None, :])[:, :, None]
    return ((s + (n >> 1)) // n).astype(np.uint8)


def apply(frame, sel, mode, strength=0, colour=0):
    """frame uint8 [H,W,3], sel bool [H,W] -> the redacted frame; every sum reads `frame`."""
    if mode == FILL:
        full = np.empty_like(frame)
        full[:] = [(int(colour) >> (8 * c)) & 255 for c in range(3)]
    elif mode == MOSAIC:
        full = _mosaic(frame, int(strength))
    else:
        full = _blur(frame, int(strength))
    return np.where(sel[:, :, None], full, frame)


def frame_reference(frame, kps, count, select, mode, label_mask, strength=0, pad=0, colour=0, maps=None):
    """One frame: kps [K,98,2], count live slots (None: all) -> (out, valid [K], number of selected pixels).  ``maps``: the frame's
    mask_ref.frame_maps where the caller already has them."""
    H, W = frame.shape[:2]
    if maps is None:
        maps = mr.frame_maps(kps, count, H, W)
    sel = selected(maps, select, label_mask, pad)
    return apply(frame, sel, mode, strength, colour), maps[3], int(sel.sum())

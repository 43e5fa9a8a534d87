"""Per-face region statistics: the integer restatement of the arithmetic the engine's pf_measure_faces specifies,
written from that specification and not from the kernel.  A helper of tests/test_face_stats.py and tests/test_gpu_face_stats.py, not
a test.

``luma(frame)`` -> Y int64 [H,W]; ``laplacian(Y)`` -> the 4-neighbour Laplacian with edge replication; ``frame_stats(frame, maps, dark,
bright)`` -> uint64 [K,8,9] from the (labels, owners, boxes, valid) of tests/mask_ref.py, rows of invalid slots zero;
``frame_reference(...)`` -> the same with the maps computed here; ``checkerboard_lap2(H, W)`` -> the closed form of sum Lap^2 over a
0 / 255 checkerboard."""
import numpy as np

from tests import mask_ref as mr

LABELS, FIELDS = 8, 9


def luma(frame):
    f = np.asarray(frame).astype(np.int64)
    return (29 * f[..., 0] + 150 * f[..., 1] + 77 * f[..., 2] + 128) >> 8


def laplacian(Y):
    p = np.pad(Y, 1, mode="edge")
    return 4 * Y - p[1:-1, :-2] - p[1:-1, 2:] - p[:-2, 1:-1] - p[2:, 1:-1]


def pixel_fields(frame, dark, bright):
    """The nine per-pixel addends int64 [9,H,W]."""
    f = np.asarray(frame).astype(np.int64)
    Y = luma(frame)
    lap = laplacian(Y)
    return np.stack([np.ones_like(Y), f[..., 0], f[..., 1], f[..., 2], Y, Y * Y, lap * lap, (Y <= dark).astype(np.int64),
                     (Y >= bright).astype(np.int64)])


def frame_stats(frame, maps, dark=16, bright=240):
    """frame uint8 [H,W,3], maps = (labels, owners, boxes, valid) of one frame -> uint64 [K,8,9]: one weighted bincount per field over
    the key (owner - 1) * 8 + (label - 1) of the labelled pixels."""
    labels, owners, _, valid = maps
    K = len(valid)
    on = labels != 0
    key = (owners[on].astype(np.int64) - 1) * LABELS + (labels[on].astype(np.int64) - 1)
    fields = pixel_fields(frame, dark, bright)
    out = np.zeros((K * LABELS, FIELDS), np.uint64)
    for i in range(FIELDS):
        w = fields[i][on]
        # exact: every weight is an integer below 2^21 and a frame has fewer than 2^31 pixels, so float64 sums stay below 2^53
        out[:, i] = np.bincount(key, weights=w.astype(np.float64), minlength=K * LABELS).astype(np.uint64)
    return out.reshape(K, LABELS, FIELDS)


def frame_reference(frame, kps, count, dark=16, bright=240, maps=None):
    """One frame: kps [K,98,2], count live slots (None: all) -> (stats uint64 [K,8,9], valid [K])."""
    H, W = np.asarray(frame).shape[:2]
    if maps is None:
        maps = mr.frame_maps(kps, count, H, W)
    return frame_stats(frame, maps, dark, bright), maps[3]


def checkerboard(H, W):
    """The 0 / 255 grey checkerboard ((x + y) & 1) * 255 as a BGR frame."""
    g = (((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, 2)


def checkerboard_lap2(H, W):
    """Sum of Lap^2 over every pixel of checkerboard(H, W), H, W >= 2: an interior pixel differs from its four neighbours (|Lap| =
    1020), an edge pixel from three (the replica equals it: 765), a corner from two (510)."""
    return (H - 2) * (W - 2) * 1020 ** 2 + 2 * ((H - 2) + (W - 2)) * 765 ** 2 + 4 * 510 ** 2

"""Face-region label maps: the integer restatement of the arithmetic the engine's pf_mask_faces specifies, written
from that specification and not from the kernels.  A helper of tests/test_face_masks.py and tests/test_gpu_face_masks.py, not a test.

``q4(kps)`` -> the Q4 vertices; ``fill(X, Y, H, W)`` -> one face's label map, even-odd with half-open edges and exact integer
ceilings; ``frame_maps(kps, counts, H, W)`` -> (labels, owners, boxes, valid) of one frame with the overlap rule;
``chip_map(kps, M, S)`` -> a face's map in the coordinates of its chip.  ``CASES`` is the table both test files share."""
import numpy as np

from tests import align_ref as ar

# label -> the closed polygon's WFLW indices, in order
REGIONS = {
    1: list(range(0, 33)) + [46, 45, 44, 43, 42] + [37, 36, 35, 34, 33],
    2: list(range(33, 42)),
    3: list(range(42, 51)),
    4: list(range(60, 68)),
    5: list(range(68, 76)),
    6: [51, 55, 56, 57, 58, 59],
    7: list(range(76, 88)),
    8: list(range(88, 96)),
}
assert sum(len(v) for v in REGIONS.values()) == 103


def q4(xy):
    """float coordinates of any float type -> Q4 integers: float64, clamped to [-65536, 65536], floor(16 v + 0.5)."""
    v = np.clip(np.asarray(xy).astype(np.float64), -65536.0, 65536.0)
    return np.floor(v * 16.0 + 0.5).astype(np.int64)


def finite96(kps):
    return bool(np.isfinite(np.asarray(kps, np.float64)[:96]).all())


def inside(X, Y, idx, H, W):
    """Even-odd fill of the closed polygon idx over Q4 vertices X, Y -> bool [H,W].  Python integers: exact."""
    hit = np.zeros((H, W), bool)
    px = np.arange(W)
    n = len(idx)
    for j in range(n):
        xa, ya, xb, yb = int(X[idx[j]]), int(Y[idx[j]]), int(X[idx[(j + 1) % n]]), int(Y[idx[(j + 1) % n]])
        if ya == yb:
            continue
        if ya > yb:
            xa, ya, xb, yb = xb, yb, xa, ya
        # rows with ya <= 16 py < yb
        for py in range(max(-(-ya // 16), 0), min(-(-yb // 16), H)):
            num, den = xa * (yb - ya) + (xb - xa) * (16 * py - ya), 16 * (yb - ya)
            T = -(-num // den)
            hit[py] ^= px < T
    return hit


def fill(X, Y, H, W):
    """One face -> labels uint8 [H,W]: the highest-numbered region containing the pixel."""
    lab = np.zeros((H, W), np.uint8)
    for label in sorted(REGIONS):
        lab[inside(X, Y, REGIONS[label], H, W)] = label
    return lab


def box_of(X, Y, H, W):
    c = lambda v: -(-int(v) // 16)
    return np.array([min(max(c(X[:96].min()), 0), W), min(max(c(Y[:96].min()), 0), H),
                     min(max(c(X[:96].max()), 0), W), min(max(c(Y[:96].max()), 0), H)], np.int32)


def frame_maps(kps, count, H, W, boxes_init=None):
    """kps [K,98,2] of one frame, count live slots (None: all) -> labels [H,W], owners [H,W], boxes [K,4], valid [K]; box rows of
    invalid slots keep boxes_init (zero when None)."""
    K = len(kps)
    labels, owners = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    boxes = np.zeros((K, 4), np.int32) if boxes_init is None else np.array(boxes_init, np.int32).reshape(K, 4)
    valid = np.zeros((K,), bool)
    for k in range(K):
        if (count is not None and k >= count) or not finite96(kps[k]):
            continue
        valid[k] = True
        q = q4(np.asarray(kps[k])[:96])             # the pupils 96 / 97 are not used
        X, Y = q[:, 0], q[:, 1]
        boxes[k] = box_of(X, Y, H, W)
        lab = fill(X, Y, H, W)
        take = (lab != 0) & (labels == 0)             # the lowest valid slot that labels the pixel owns it
        labels[take] = lab[take]
        owners[take] = k + 1
    return labels, owners, boxes, valid


def chip_map(kps, M, S):
    """A face's map in chip coordinates: every vertex through M = [[a, -b, tx], [b, a, ty]], each float64 operation rounded on its
    own, then the Q4 conversion."""
    k = np.asarray(kps).astype(np.float64)[:96]
    a, b, tx, ty = np.float64(M[0][0]), np.float64(M[1][0]), np.float64(M[0][2]), np.float64(M[1][2])
    x, y = k[:, 0], k[:, 1]
    cx = (a * x - b * y) + tx
    cy = (b * x + a * y) + ty
    return fill(q4(cx), q4(cy), S, S)


# ---- the shared case table -----------------------------------------------------------------------------------------------------

TILE_W, TILE_H = 128, 16        # mask_fill_kernel's tile (csrc/k_mask.h): the tile_corner case sits on a corner four tiles share


def rect_landmarks(o):
    """All 98 points at (20 + o, 10 + o), except that the 43 face-polygon vertices walk the perimeter of the rectangle
    (20, 10)-(100, 90) shifted by o: 11 + 11 + 11 + 10 points along the four sides."""
    k = np.full((98, 2), (20.0 + o, 10.0 + o), np.float64)
    walk = ([(20 + 8 * i, 10) for i in range(10)] + [(100, 10 + 8 * i) for i in range(10)] +
            [(100 - 8 * i, 90) for i in range(10)] + [(20, 90 - 80.0 * i / 13) for i in range(13)])
    assert len(walk) == 43
    for j, v in enumerate(REGIONS[1]):
        k[v] = (walk[j][0] + o, walk[j][1] + o)
    return k.astype(np.float32)


def _scatter(lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, (98, 2)).astype(np.float32)


# name -> (H, W, [landmarks [98,2] per slot])
def _cases():
    f = ar.make_landmarks
    return [
        ("upright_io40_odd", 121, 161, [f(80, 60, 40, 20, seed=1)]),             # no row is 4-byte aligned, no multiple of the tile
        ("roll-75_io25", 120, 160, [f(80, 60, 25, -75, seed=2)]),
        ("small_io10", 120, 160, [f(80, 60, 10, 0, seed=3)]),
        ("half_outside", 120, 160, [f(8, 10, 40, 10, seed=4)]),
        ("outside", 120, 160, [f(-400, 60, 40, 0, seed=5)]),                     # valid, draws nothing
        ("huge", 120, 160, [f(80, 0, 600, 5, seed=6)]),                          # every tile is interior to some polygon
        ("tile_corner", 120, 320, [f(TILE_W, 4 * TILE_H, 40, -15, seed=7)]),
        ("rect_integer", 120, 160, [rect_landmarks(0.0)]),
        ("rect_half", 120, 160, [rect_landmarks(0.5)]),
        ("rect_7_5_sixteenths", 120, 160, [rect_landmarks(0.46875)]),
        ("scattered", 120, 160, [_scatter(-100, 260, seed=15)]),               # seed chosen so that each label keeps > 100 pixels
        ("far_scattered", 120, 160, [_scatter(-3000, 3000, seed=9)]),
    ]


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
_REF = {}


def case_reference(case):
    """-> (labels, owners, boxes, valid) of the case's one frame, computed once and shared; callers must not change it."""
    name, H, W, faces = case
    if name not in _REF:
        _REF[name] = frame_maps(np.stack(faces), None, H, W)
    return _REF[name]

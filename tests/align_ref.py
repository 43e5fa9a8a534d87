"""Aligned face chips: the float64 / integer restatement of the arithmetic the engine's pf_align_faces specifies,
written from that specification and not from the kernels.  A helper of tests/test_align_faces.py and tests/test_gpu_align_faces.py,
not a test.

``fit(kps) -> (M, valid)``: the five points of a face's 98 WFLW landmarks onto the ArcFace template, least-squares similarity
without reflection in closed form.  ``warp(frame, M, S) -> chip``: Q10 bilinear sampling at the inverse map, in integers.  Every
float64 operation is one numpy / Python operation, i.e. individually rounded, in the order the specification writes them.
``CASES`` and the scene builders are the table both test files share."""
import math

import numpy as np

Q112 = ((38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041))


def five_points(kps):
    """kps [98][2] of any float type -> five (x, y) pairs of Python floats (float64)."""
    k = np.asarray(kps).astype(np.float64)
    pts = []
    for lo in (60, 68):
        sx, sy = 0.0, 0.0
        for i in range(lo, lo + 8):             # summed in index order
            sx, sy = sx + float(k[i, 0]), sy + float(k[i, 1])
        pts.append((sx / 8.0, sy / 8.0))
    for i in (54, 76, 82):
        pts.append((float(k[i, 0]), float(k[i, 1])))
    return pts


def fit(kps, S=112):
    """-> (M float64 [2,3] frame -> chip, valid).  M is None when the fit is invalid."""
    with np.errstate(all="ignore"):
        p = [(np.float64(x), np.float64(y)) for x, y in five_points(kps)]
        k = np.float64(S) / np.float64(112.0)
        q = [(np.float64(x) * k, np.float64(y) * k) for x, y in Q112]
        z = np.float64(0.0)
        mpx = mpy = mqx = mqy = z
        for i in range(5):
            mpx, mpy, mqx, mqy = mpx + p[i][0], mpy + p[i][1], mqx + q[i][0], mqy + q[i][1]
        mpx, mpy, mqx, mqy = mpx / 5.0, mpy / 5.0, mqx / 5.0, mqy / 5.0
        den = na = nb = z
        for i in range(5):
            dpx, dpy, dqx, dqy = p[i][0] - mpx, p[i][1] - mpy, q[i][0] - mqx, q[i][1] - mqy
            den = den + (dpx * dpx + dpy * dpy)
            na = na + (dpx * dqx + dpy * dqy)
            nb = nb + (dpx * dqy - dpy * dqx)
        if not den > 0:
            return None, False
        a, b = na / den, nb / den
        tx = mqx - (a * mpx - b * mpy)
        ty = mqy - (b * mpx + a * mpy)
        det = a * a + b * b
        if not all(math.isfinite(v) for v in (a, b, tx, ty)):
            return None, False
        if not (2.0 ** -12 <= det <= 2.0 ** 12):
            return None, False
        return np.array([[a, -b, tx], [b, a, ty]], np.float64), True


def warp(frame, M, S):
    """frame uint8 [H,W,3], M float64 [2,3] (frame -> chip) -> chip uint8 [S,S,3]."""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    M = np.asarray(M, np.float64)
    a, b, tx, ty = M[0, 0], M[1, 0], M[0, 2], M[1, 2]
    det = a * a + b * b
    ia, ib = a / det, b / det
    itx = -(ia * tx + ib * ty)
    ity = -(ia * ty - ib * tx)
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    u = (ia * x + ib * y) + itx
    v = (ia * y - ib * x) + ity
    u = np.clip(u, -2.0, float(W + 1))
    v = np.clip(v, -2.0, float(H + 1))
    U = np.floor(u * 1024.0 + 0.5).astype(np.int64)
    V = np.floor(v * 1024.0 + 0.5).astype(np.int64)
    x0, fx, y0, fy = U >> 10, U & 1023, V >> 10, V & 1023
    padded = np.zeros((H + 6, W + 6, 3), np.int64)          # constant border 0; coordinates lie in [-2, W + 2] x [-2, H + 2]
    padded[3:3 + H, 3:3 + W] = frame

    def tap(yy, xx):
        return padded[yy + 3, xx + 3]
    fx, fy = fx[..., None], fy[..., None]
    acc = (tap(y0, x0) * (1024 - fx) * (1024 - fy) + tap(y0, x0 + 1) * fx * (1024 - fy) + tap(y0 + 1, x0) * (1024 - fx) * fy +
           tap(y0 + 1, x0 + 1) * fx * fy + (1 << 19)) >> 20
    return acc.astype(np.uint8)


# ---- scenes shared by the CPU (emulator) and the GPU file ------------------------------------------------------------------------

def layout98():
    """A fixed 98-point face layout in a unit box (x, y in about [-1, 1]): outline, brows, nose, eye contours, mouth, pupils.  Only its
    fixedness matters; points 60..67 / 68..75 ring the eyes, 54 is the nose tip, 76 / 82 the mouth corners."""
    pts = np.zeros((98, 2), np.float64)
    for i in range(33):                                   # jaw line
        t = math.pi * i / 32.0
        pts[i] = (-math.cos(t), 0.1 + 0.9 * math.sin(t))
    for i in range(9):                                    # brows
        pts[33 + i] = (-0.75 + 0.06 * i, -0.55 - 0.02 * (i % 3))
        pts[42 + i] = (0.27 + 0.06 * i, -0.55 - 0.02 * (i % 3))
    for i in range(9):                                    # nose, 54 = tip
        pts[51 + i] = (0.04 * (i - 3), -0.3 + 0.12 * i) if i < 4 else (0.08 * (i - 6), 0.12)
    pts[54] = (0.0, 0.1)
    for i in range(8):                                    # eye contours
        t = 2 * math.pi * i / 8.0
        pts[60 + i] = (-0.42 + 0.16 * math.cos(t), -0.3 + 0.07 * math.sin(t))
        pts[68 + i] = (0.42 + 0.16 * math.cos(t), -0.3 + 0.07 * math.sin(t))
    for i in range(20):                                   # mouth: 76 and 82 are the corners
        t = 2 * math.pi * i / 12.0
        pts[76 + i] = (-0.33 * math.cos(t), 0.52 + 0.12 * math.sin(t)) if i < 12 else (-0.2 * math.cos(2 * math.pi * (i - 12) / 8.0), 0.52 + 0.05 * math.sin(2 * math.pi * (i - 12) / 8.0))
    pts[96], pts[97] = (-0.42, -0.3), (0.42, -0.3)
    return pts


def make_frame(H, W, seed):
    """Seeded uint8 noise on a smooth gradient: every bilinear weight matters."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = np.stack([80 + 100.0 * xx / W, 60 + 120.0 * yy / H, 100 + 50.0 * (xx + yy) / (H + W)], axis=2)
    return np.clip(base + rng.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)


def make_landmarks(cx, cy, interocular, roll_deg, seed, jitter=1.5, dtype=np.float32):
    """The layout through a similarity (eye-centre distance `interocular` pixels, rolled, centred at cx, cy) + seeded jitter."""
    rng = np.random.default_rng(seed)
    s = interocular / 0.84
    c, sn = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
    L = layout98()
    out = np.stack([cx + s * (c * L[:, 0] - sn * L[:, 1]), cy + s * (sn * L[:, 0] + c * L[:, 1])], axis=1)
    out += rng.uniform(-jitter, jitter, out.shape)
    return out.astype(dtype)


def landmarks_with_p0_on_integers(cx, cy, interocular, seed):
    """A face whose p0 (mean of points 60..67) lands exactly on the integer pixel (cx, cy): float32-exact integers whose sum is 8 cx."""
    k = make_landmarks(cx + 0.42 / 0.84 * interocular, cy + 0.3 / 0.84 * interocular, interocular, 0.0, seed)
    k[60:68] = np.round(k[60:68])
    k[60] += (np.float32(8 * cx) - k[60:68, 0].sum(dtype=np.float64), np.float32(8 * cy) - k[60:68, 1].sum(dtype=np.float64))
    assert k[60:68].sum(axis=0, dtype=np.float64).tolist() == [8.0 * cx, 8.0 * cy]
    return k


# (name, frame H, W, chip size, [(cx, cy, interocular, roll)]).  For S = 32 the template's eye distance is 35.24 * 32 / 112 = 10.07
# pixels, so the scale is 10.07 / interocular: 10 -> about 1, 25 -> 0.4, 50 -> 0.2, 600 -> 0.017 (det 2.8e-4, above 2^-12).
CASES = [
    ("scale1_roll0", 120, 160, 32, [(80.0, 60.0, 10.0, 0.0)]),
    ("scale04_roll30", 240, 320, 32, [(150.0, 120.0, 25.0, 30.0)]),
    ("scale04_roll-75", 240, 320, 32, [(150.0, 120.0, 25.0, -75.0)]),
    ("half_outside", 240, 320, 32, [(8.0, 10.0, 25.0, 10.0)]),            # border zeros on two sides
    ("p0_on_integers", 240, 320, 32, "p0"),
    ("odd_width", 120, 161, 32, [(80.0, 60.0, 25.0, 20.0)]),              # rows of 483 bytes: no row starts 4-byte aligned, byte staging
    ("chip112", 240, 320, 112, [(160.0, 120.0, 60.0, -20.0)]),
    ("huge_face", 720, 1280, 32, [(640.0, 400.0, 600.0, 5.0)]),           # every tile's footprint exceeds the LDS budget
    # a 16 x 16 tile covers about 115 x 115 source pixels (40 KB): only the tiles the frame's corner clips fit the budget
    ("roll45_scale02", 240, 320, 32, [(40.0, 40.0, 50.0, 45.0)]),
]


def case_scene(case):
    """-> (frame uint8 [H,W,3], kps float32 [1,n,98,2], S)."""
    name, H, W, S, faces = case
    frame = make_frame(H, W, seed=len(name) * 7 + H)
    if faces == "p0":
        kps = landmarks_with_p0_on_integers(140.0, 110.0, 25.0, seed=5)[None]
    else:
        kps = np.stack([make_landmarks(cx, cy, io, roll, seed=11 + i) for i, (cx, cy, io, roll) in enumerate(faces)])
    return frame, kps[None].astype(np.float32), S

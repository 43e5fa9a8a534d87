"""Case builders and regime formulas for tests/test_prepost_edges.py: the pre/post-processing kernels of csrc/k_prepost.h
(letterbox_kernel, nms_compact_kernel, nms_kernel, crop_params_kernel, crop_resize_kernel, crop_resize_direct_kernel,
absdiff_sum_kernel) at the sizes where they change path.

Every case comes with the regime it claims, computed here from the inputs and oracle/prepost.py alone -- never from what a kernel
returned -- so that a later change of a kernel constant cannot quietly move a case to another path.  The constants and the few
formulas the kernels decide by are restated below next to the names they have in the sources."""
import numpy as np

from oracle import prepost as pp

# ---- nms_kernel ------------------------------------------------------------------------------------------------------------------
NMS_LDS_KEYS = 2048     # PF_NMS_LDS_KEYS: keys and flags in LDS while next_pow2(C) <= this
NMS_LDS_BOXES = 1024    # rows of s_box: the candidates' boxes in LDS too while C <= this
MAX_KEEP = 1024         # kMaxKeep (pipeline.inl) == capacity of s_keep: rows kept per frame
WAVE = 64

NMS_R = 3000
NMS_CS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2600)
NMS_INFO = [np.float32(1.0 / 3.0), 0, 12]       # letterbox scale / left / top of a 1080p frame
SCORE_THRES, IOU_THRES = 0.5, 0.3
ROW_ID = 15             # column that carries the row's own index (exact in float32), so kept rows name their source


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def nms_cap(max_rows):
    """Slots per frame of the key / flag buffers (ensure_pipeline): a power of two >= the most rows the engine has seen."""
    return next_pow2(max(max_rows, 2))


def nms_candidates(rows, score_thres=SCORE_THRES):
    """C of nms_kernel: rows whose score passes the strict '>' of nms_compact_kernel (NaN does not)."""
    return int(np.count_nonzero(rows[:, 4] > np.float32(score_thres)))


def nms_regime(C):
    """Where nms_kernel keeps its working set for C candidates: 'lds' (keys and boxes in LDS), 'lds_keys' (keys in LDS, boxes
    re-read from global memory) or 'global' (keys and flags in global memory)."""
    if next_pow2(C) > NMS_LDS_KEYS:
        return "global"
    return "lds" if C <= NMS_LDS_BOXES else "lds_keys"


def ranked_rows(rows, score_thres=SCORE_THRES):
    """Candidate row indices in the engine's visiting order: score descending, equal scores by ascending row."""
    cand = np.nonzero(rows[:, 4] > np.float32(score_thres))[0]
    return cand[np.argsort(-rows[cand, 4], kind="stable")]


def nms_background(R, rng, score):
    """R rows with centres uniform in the 640 x 384 letterbox, sides uniform in [4, 40] and one score everywhere."""
    rows = np.zeros((R, 16), np.float32)
    rows[:, 0] = rng.uniform(0, 640, R)
    rows[:, 1] = rng.uniform(0, 384, R)
    rows[:, 2:4] = rng.uniform(4, 40, (R, 2))
    rows[:, 4] = score
    rows[:, 5:ROW_ID] = rng.uniform(0, 1, (R, ROW_ID - 5))
    rows[:, ROW_ID] = np.arange(R)
    return rows


def nms_case(C, tied, R=NMS_R, seed=0):
    """R rows scored exactly at the threshold except C chosen ones, which get distinct scores in (0.5, 1) -- or, `tied`, those
    scores rounded up to sixteenths, so that eight values are shared by all candidates.  For C > 5 the 4th-ranked candidate has
    a zero-area box, and the 6th-ranked one is a copy of that box: their IoU is 0 / 0 = NaN, which must suppress."""
    rng = np.random.default_rng(1000 * seed + 2 * C + int(tied))
    rows = nms_background(R, rng, SCORE_THRES)
    chosen = rng.choice(R, size=C, replace=False)
    scores = rng.permutation(np.linspace(0.5, 1.0, C + 2)[1:-1]).astype(np.float32)
    if tied:
        scores = (np.ceil(scores * np.float32(16)) / np.float32(16)).astype(np.float32)
    rows[chosen, 4] = scores
    if C > 5:
        order = ranked_rows(rows)
        rows[order[3], 2:4] = 0.0
        rows[order[5], :4] = rows[order[3], :4]
    return rows


def nms_full_case(R=4096, seed=1):
    """Every row above the threshold with distinct scores: C == cap, so the sort has no zero padding."""
    rng = np.random.default_rng(seed)
    rows = nms_background(R, rng, SCORE_THRES)
    rows[:, 4] = rng.permutation(np.linspace(0.5, 1.0, R + 2)[1:-1]).astype(np.float32)
    return rows


def nms_nonfinite_case(C=300, seed=2):
    """C ordinary candidates plus one row scored NaN (fails '>' and must be dropped) and one scored +inf (must rank first).
    Returns (rows, nan_row, inf_row)."""
    rng = np.random.default_rng(seed)
    rows = nms_background(NMS_R, rng, SCORE_THRES)
    chosen = rng.choice(NMS_R, size=C + 2, replace=False)
    rows[chosen[:C], 4] = rng.permutation(np.linspace(0.5, 1.0, C + 2)[1:-1]).astype(np.float32)
    rows[chosen[C], 4] = np.nan
    rows[chosen[C + 1], 4] = np.inf
    return rows, int(chosen[C]), int(chosen[C + 1])


def nms_reference(rows, info, tied):
    """All rows the reference keeps (no cap), xyxy un-letterboxed in columns 0:4."""
    return pp.detector_postprocess(rows, info, IOU_THRES, SCORE_THRES, ties_by_row=tied)


# ---- selection (step 5 of nms_kernel == FaceAna.sort_and_filter) over a ragged batch ---------------------------------------------
SEL_HW = (192, 320)     # letterbox scale to 384 x 640 is exactly 2 with no padding: halving keeps equal areas equal
SEL_TOP_K, SEL_MIN_FACE, SEL_F = 5, 400.0, 4


def _plant(rows, slots, boxes_cxcywh, scores):
    for r, b, s in zip(slots, boxes_cxcywh, scores):
        rows[r, :4] = b
        rows[r, 4] = s


def selection_case(seed=3):
    """Four frames of NMS_R rows (letterboxed coordinates) that take different paths of one nms_kernel launch:
      0  nine disjoint boxes whose areas tie in threes, more than top_k, some scores equal
      1  nothing above the threshold
      2  2500 candidates (global-memory regime), seven of them large, two pairs of equal area
      3  three candidates, one of them under min_face
    Background rows sit exactly at the score threshold; their boxes (sides < 40, so < 20 in the frame) are below min_face."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (SEL_F,) + SEL_HW + (3,), dtype=np.uint8)
    rows = np.stack([nms_background(NMS_R, rng, SCORE_THRES) for _ in range(SEL_F)])
    # frame 0: centres on a 3 x 3 grid 192 x 128 apart, sides powers of two <= 128: disjoint, every coordinate exact
    sizes = [(64, 32), (128, 64), (64, 64), (32, 64), (64, 128), (128, 32), (64, 32), (128, 64), (32, 128)]
    boxes = [(128 + 192 * (k % 3), 64 + 128 * (k // 3), w, h) for k, (w, h) in enumerate(sizes)]
    _plant(rows[0], rng.choice(NMS_R, 9, replace=False), boxes, [0.9, 0.9, 0.8, 0.8, 0.8, 0.7, 0.95, 0.6, 0.6])
    # frame 2
    chosen = rng.choice(NMS_R, 2500, replace=False)
    rows[2, chosen, 4] = rng.permutation(np.linspace(0.5, 0.9, 2502)[1:-1]).astype(np.float32)
    big = [(96, 96), (128, 72), (80, 80), (100, 64), (120, 120), (64, 64), (112, 112)]
    boxes = [(80 + 160 * (k % 4), 80 + 200 * (k // 4), w, h) for k, (w, h) in enumerate(big)]
    _plant(rows[2], chosen[:7], boxes, [0.99, 0.98, 0.97, 0.96, 0.95, 0.94, 0.93])
    # frame 3
    _plant(rows[3], rng.choice(NMS_R, 3, replace=False), [(100, 100, 64, 64), (300, 200, 30, 26), (500, 300, 96, 48)], [0.7, 0.9, 0.8])
    return frames, rows


def selection_reference(rows_f, info, min_face=SEL_MIN_FACE, top_k=SEL_TOP_K):
    """(selected boxes, areas of every box over min_face in keep order).  NMS with ties by row, the kMaxKeep cap, the area
    filter, then the reference's `area.argsort()[-top_k:][::-1]` written with a stable sort: numpy's default sort is an insertion
    sort -- stable -- for the handful of boxes that reach it, and it is the order nms_kernel documents (equal areas: later index
    first)."""
    kept = nms_reference(rows_f, info, True)[:MAX_KEEP]
    b = kept[:, :4]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    sel = area > np.float32(min_face)
    b, area = b[sel], area[sel]
    if b.shape[0] > top_k:
        b = b[np.argsort(area, kind="stable")[-top_k:][::-1]]
    return b, area


# ---- crop_resize_kernel / crop_resize_direct_kernel ------------------------------------------------------------------------------
CROP_TY = 8                 # PF_CROP_TY: output rows per workgroup
CROP_SRC_BYTES = 16384      # PF_CROP_SRC_BYTES: LDS budget for a tile's source rows
CROP_FRAMES = ((201, 333), (240, 410), (203, 331), (200, 332))     # row stride mod 4 = 3, 2, 1, 0
CROP_S_TILED = (32, 64, 128, 256)
CROP_S_DIRECT = (48, 112)


def crop_kernel(S):
    """run_crop_stage's choice."""
    return "crop_resize_kernel" if S <= 256 and 256 % S == 0 and (S * 3) % 4 == 0 else "crop_resize_direct_kernel"


def crop_shift(ci):
    """`shift` of crop_resize_kernel: where the crop's first byte sits inside its 32-bit word, (xs - add) * 3 mod 4."""
    return ((max(ci.x0, 0) - ci.add) * 3) % 4     # xs = x0 clamped into the padded frame; a valid crop starts left of its right edge


def crop_tiles_fit(ci, S):
    """Per tile of CROP_TY output rows: do its source rows fit the LDS budget (True) or does the workgroup take the per-pixel
    path (False)?  nrows from the vertical taps the oracle derives, lds_stride as the kernel rounds it."""
    lds_stride = (ci.w_crop * 3 + 6) & ~3
    exact2 = ci.w_crop == 2 * S and ci.h_crop == 2 * S
    r0, r1, _, _ = pp.linear_coeffs_vertical(ci.h_crop, S)
    fits = []
    for oy0 in range(0, S, CROP_TY):
        last = min(oy0 + CROP_TY, S) - 1
        if exact2:
            nrows = 2 * (last + 1) - 2 * oy0
        else:
            nrows = int(max(r0[last], r1[last]) - min(r0[oy0], r1[oy0])) + 1
        fits.append(nrows * lds_stride <= CROP_SRC_BYTES)
    return fits


def crop_boxes(H, W, S):
    """{name: xyxy rows} for one frame size and output size."""
    w2 = 2 * S / 1.4 + 0.8                  # floor(1.4 * w2 / 2) == S: a crop of exactly 2S x 2S
    return {
        "step": [[100.0 + k, 60.0, 140.0 + k, 104.0] for k in range(8)],        # left edge one pixel further each
        "edges": [[-15.0, 60.0, 35.0, 110.0], [W - 35.0, 60.0, W + 15.0, 110.0], [100.0, -15.0, 150.0, 35.0], [100.0, H - 35.0, 150.0, H + 15.0]],
        "small": [[150.0, 90.0, 171.5, 111.5]],                                 # 21.5 pixels, barely over min_face 20: up-sampled
        "outside": [[W + 200.0, H + 200.0, W + 260.0, H + 260.0]],
        "whole": [[2.0, 2.0, W - 2.0, H - 2.0]],
        "twice": [[10.0, 5.0, 10.0 + w2, 5.0 + w2]],
    }


# ---- letterbox_kernel as pf_resize / pf_letterbox --------------------------------------------------------------------------------
RESIZE_CASES = (((101, 333), (37, 53)), ((64, 96), (128, 192)), ((37, 53), (37, 53)), ((200, 300), (100, 150)), ((1, 1), (5, 7)),
                ((5, 7), (1, 1)), ((203, 331), (64, 64)))
LETTERBOX_CASES = (((101, 333), (64, 96)), ((203, 331), (96, 160)))


def resize_path(hw, out_hw):
    """letterbox_kernel's branch: the 2 x 2 box average of an exact halving, or the fixed-point taps."""
    return "box" if hw[0] == 2 * out_hw[0] and hw[1] == 2 * out_hw[1] else "taps"


# ---- absdiff_sum_kernel ----------------------------------------------------------------------------------------------------------
ABSDIFF_SHAPES = ((1, 1), (1, 5), (1, 6), (3, 7), (37, 53), (64, 64))
ABSDIFF_VEC = 16            # bytes per uint4 load; the rest is the scalar tail of thread 0


def absdiff_class(hw):
    n = hw[0] * hw[1] * 3
    return "short" if n < ABSDIFF_VEC else ("tail" if n % ABSDIFF_VEC else "whole")

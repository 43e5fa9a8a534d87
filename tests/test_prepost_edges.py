"""The pre/post-processing kernels of csrc/k_prepost.h at their branch edges, bit-exact against oracle/prepost.py: every case once
on the CPU SIMT emulator and once, with the same inputs, on the GPU.  These are integer, byte and correctly-rounded float32
operations, so every comparison is np.array_equal.  The emulator sees the arithmetic; only the GPU run can falsify the wave ballot
and atomics of nms_compact_kernel, the barriers around nms_kernel's keys and flags in LDS or global memory, and the 32-bit staging
loads of crop_resize_kernel.  tests/prepost_cases.py builds the inputs and states, from inputs and oracle alone, which path each one
takes; the assertions on that come before the engine runs."""
import functools

import numpy as np
import pytest

from oracle import prepost as pp
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from tests import prepost_cases as pc
from tests.test_emu_pipeline import _f64_boxes


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _ids(cases):
    """Test ids that spell the sizes: ((201, 333), 64) -> '201x333-64', ((101, 333), (37, 53)) -> '101x333-37x53', (3, 7) -> '3x7'."""
    def size(v):
        return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
    return ["-".join(size(v) for v in (c if isinstance(c[0], tuple) else (c,))) for c in cases]


def _random_image(hw, seed):
    return np.random.default_rng(seed).integers(0, 256, tuple(hw) + (3,), dtype=np.uint8)


# ---- 1. NMS regimes --------------------------------------------------------------------------------------------------------------
# the regime each candidate count is here for: both sides of a wave, of s_box (1024) and of PF_NMS_LDS_KEYS (2048)
NMS_REGIME = {0: "lds", 1: "lds", 2: "lds", 63: "lds", 64: "lds", 65: "lds", 255: "lds", 256: "lds", 257: "lds", 1023: "lds",
              1024: "lds", 1025: "lds_keys", 2047: "lds_keys", 2048: "lds_keys", 2049: "global", 2600: "global"}
NMS_SWEEP = [(C, tied) for C in pc.NMS_CS for tied in (False, True)]       # under 0.1 s a case on the emulator: nothing is thinned there


@functools.lru_cache(maxsize=None)
def _nms(C, tied):
    rows = pc.nms_case(C, tied)
    return _frozen(rows, pc.nms_reference(rows, pc.NMS_INFO, tied))


def _assert_keeps(eng, rows, ref):
    """The engine returns the reference's keep list up to the documented kMaxKeep rows."""
    got = eng.nms_rows(rows, pc.NMS_INFO[0], pc.NMS_INFO[1], pc.NMS_INFO[2], pc.SCORE_THRES, pc.IOU_THRES)
    assert got.shape[0] == min(len(ref), pc.MAX_KEEP)
    assert np.array_equal(got, ref[:pc.MAX_KEEP])


def check_nms(eng, C, tied):
    rows, ref = _nms(C, tied)
    assert rows.shape[0] == pc.NMS_R and pc.nms_cap(pc.NMS_R) == 4096
    assert pc.nms_candidates(rows) == C and pc.nms_regime(C) == NMS_REGIME[C]
    assert np.count_nonzero(rows[:, 4] == np.float32(pc.SCORE_THRES)) == pc.NMS_R - C      # the rest sits exactly on the strict '>'
    cand_scores = rows[rows[:, 4] > pc.SCORE_THRES, 4]
    if tied:
        assert len(np.unique(cand_scores)) <= 8         # sixteenths in (0.5, 1]: beyond 8 candidates the row half of the key decides
    else:
        assert len(np.unique(cand_scores)) == C
    if C > 5:
        order = pc.ranked_rows(rows)
        kept_ids = ref[:pc.MAX_KEEP, pc.ROW_ID].astype(np.int64)
        assert not rows[order[3], 2:4].any() and np.array_equal(rows[order[5], :4], rows[order[3], :4])
        assert order[3] in kept_ids and order[5] not in kept_ids        # zero area against zero area: IoU NaN suppresses
    if C >= 2047:
        assert len(ref) > pc.MAX_KEEP                   # the s_keep cap is what ends the list
    _assert_keeps(eng, rows, ref)


@pytest.mark.parametrize("C,tied", NMS_SWEEP)
def test_nms_regimes_emu(emu_engine, C, tied):
    check_nms(emu_engine, C, tied)


@pytest.mark.gpu
@pytest.mark.parametrize("C,tied", NMS_SWEEP)
def test_nms_regimes_gpu(gpu_engine, C, tied):
    check_nms(gpu_engine, C, tied)


@functools.lru_cache(maxsize=None)
def _nms_full():
    rows = pc.nms_full_case()
    return _frozen(rows, pc.nms_reference(rows, pc.NMS_INFO, False))


def check_nms_full(eng):
    rows, ref = _nms_full()
    C = pc.nms_candidates(rows)
    assert C == rows.shape[0] == pc.nms_cap(rows.shape[0]) == pc.next_pow2(C)       # n2 == cap: nothing to pad
    assert pc.nms_regime(C) == "global" and len(ref) > pc.MAX_KEEP
    _assert_keeps(eng, rows, ref)


def test_nms_every_row_a_candidate_emu(emu_engine):
    check_nms_full(emu_engine)


@pytest.mark.gpu
def test_nms_every_row_a_candidate_gpu(gpu_engine):
    check_nms_full(gpu_engine)


def check_nms_nonfinite(eng):
    rows, nan_row, inf_row = pc.nms_nonfinite_case()
    ref = pc.nms_reference(rows, pc.NMS_INFO, False)
    assert np.isnan(rows[nan_row, 4]) and np.isposinf(rows[inf_row, 4])
    assert pc.nms_candidates(rows) == 301 and pc.nms_regime(301) == "lds"
    assert ref[0, pc.ROW_ID] == inf_row and nan_row not in ref[:, pc.ROW_ID]        # the oracle: +inf first, NaN never
    _assert_keeps(eng, rows, ref)


def test_nms_nan_and_inf_scores_emu(emu_engine):
    check_nms_nonfinite(emu_engine)


@pytest.mark.gpu
def test_nms_nan_and_inf_scores_gpu(gpu_engine):
    check_nms_nonfinite(gpu_engine)


# ---- 2. ragged multi-frame selection ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _selection():
    frames, rows = pc.selection_case()
    _, info = pp.detector_preprocess_u8(frames[0], (384, 640))
    assert info == [2.0, 0, 0]                          # halving is exact: planted equal areas stay equal in the frame
    info = [np.float32(info[0]), info[1], info[2]]
    refs = [pc.selection_reference(rows[f], info) for f in range(pc.SEL_F)]
    return _frozen(frames, rows) + (refs,)


def check_selection(eng, student_weights):
    frames, rows, refs = _selection()
    C = [pc.nms_candidates(rows[f]) for f in range(pc.SEL_F)]
    assert C == [9, 0, 2500, 3] and [pc.nms_regime(c) for c in C] == ["lds", "lds", "global", "lds"]
    assert pc.nms_cap(rows.shape[1]) == 4096            # one cap for all four frames
    passing = [len(area) for _, area in refs]
    assert passing == [9, 0, 7, 2]                      # frames 0 and 2 take the top-k branch, frame 3 loses one box to min_face
    assert np.unique(refs[0][1], return_counts=True)[1].tolist() == [3, 3, 3]       # areas tie in threes
    assert sorted(np.unique(refs[2][1], return_counts=True)[1].tolist()) == [1, 1, 1, 2, 2]
    for f in (0, 2):                                    # the k-th largest area is shared with a box that is left out
        area = np.sort(refs[f][1])
        assert area[-pc.SEL_TOP_K] == area[-pc.SEL_TOP_K - 1]
    blob, _ = build_student_program(student_weights, 64, "f32")
    eng.load_program(0, blob, pc.SEL_F * pc.SEL_TOP_K)
    counts, boxes, _, _ = eng.run_frames(frames, pc.SCORE_THRES, pc.IOU_THRES, pc.SEL_MIN_FACE, pc.SEL_TOP_K, planted_rows=rows)
    assert counts.tolist() == [min(n, pc.SEL_TOP_K) for n in passing]
    for f in range(pc.SEL_F):
        assert np.array_equal(boxes[f, :counts[f]], refs[f][0]), f


def test_ragged_selection_emu(emu_engine, student_weights):
    check_selection(emu_engine, student_weights)


@pytest.mark.gpu
def test_ragged_selection_gpu(gpu_engine, student_weights):
    check_selection(gpu_engine, student_weights)


# ---- 3. crop alignment and routes ------------------------------------------------------------------------------------------------
CROP_STRIDE_MOD4 = {(201, 333): 3, (240, 410): 2, (203, 331): 1, (200, 332): 0}
CROP_CASES = [(hw, S) for hw in pc.CROP_FRAMES for S in pc.CROP_S_TILED + pc.CROP_S_DIRECT]


def _logged(eng, call):
    eng.profile_enable(True)
    out = call()
    log = eng.launch_log()
    eng.profile_enable(False)
    return out, log


def _assert_crops(frame, boxes, S, crops, params):
    H, W = frame.shape[:2]
    for i, b in enumerate(boxes):
        ci = pp.landmark_crop_box(b, H, W)
        assert bool(params[i, 0]) == ci.valid, i
        if not ci.valid:
            assert not crops[i].any(), i
            continue
        assert params[i, [1, 2, 3, 6, 7]].tolist() == [ci.add, ci.x0, ci.y0, ci.w_crop, ci.h_crop], i
        assert np.array_equal(crops[i], pp.landmark_crop(frame, ci, (S, S))), i


def check_crops(eng, hw, S):
    H, W = hw
    frame = _random_image(hw, seed=H + W)
    named = pc.crop_boxes(H, W, S)
    boxes = np.asarray([b for group in named.values() for b in group], np.float32)
    ci = {name: [pp.landmark_crop_box(np.asarray(b, np.float32), H, W) for b in group] for name, group in named.items()}
    tiled = S in pc.CROP_S_TILED
    assert (W * 3) % 4 == CROP_STRIDE_MOD4[hw]          # rows_aligned only on the control frame
    assert pc.crop_kernel(S) == ("crop_resize_kernel" if tiled else "crop_resize_direct_kernel")
    assert all(c.valid for c in ci["step"] + ci["edges"] + ci["small"] + ci["whole"] + ci["twice"]) and not ci["outside"][0].valid
    assert ci["small"][0].w_crop < S and ci["small"][0].h_crop < S                  # up-sampling
    assert ci["twice"][0].w_crop == ci["twice"][0].h_crop == 2 * S                 # the 2 x 2 box average
    if tiled:
        assert all(all(pc.crop_tiles_fit(c, S)) for c in ci["step"])               # staged through LDS ...
        assert {pc.crop_shift(c) for c in ci["step"]} == {0, 1, 2, 3}               # ... at every byte alignment
        if S >= 64:
            assert not any(pc.crop_tiles_fit(ci["whole"][0], S))                    # over the LDS budget: per-pixel path
        fits = pc.crop_tiles_fit(ci["twice"][0], S)
        assert all(fits) if S <= 128 else not any(fits)                            # box average inside LDS / per pixel
    (crops, params), log = _logged(eng, lambda: eng.crop_faces(frame, boxes, S))
    assert [k for k in log if k.startswith("crop_resize")] == [pc.crop_kernel(S)]
    _assert_crops(frame, boxes, S, crops, params)


@pytest.mark.parametrize("hw,S", CROP_CASES, ids=_ids(CROP_CASES))
def test_crop_routes_emu(emu_engine, hw, S):
    check_crops(emu_engine, hw, S)


@pytest.mark.gpu
@pytest.mark.parametrize("hw,S", CROP_CASES, ids=_ids(CROP_CASES))
def test_crop_routes_gpu(gpu_engine, hw, S):
    check_crops(gpu_engine, hw, S)


def check_crops_f64(eng):
    """pf_crop_faces_f64 (float64 rows of tracked frames) on the frame whose row stride is 3 mod 4."""
    hw, S = (201, 333), 64
    frame = _random_image(hw, seed=64)
    boxes = _f64_boxes()
    assert boxes.dtype == np.float64 and (hw[1] * 3) % 4 == 3 and pc.crop_kernel(S) == "crop_resize_kernel"
    cis = [pp.landmark_crop_box(b, hw[0], hw[1]) for b in boxes]
    assert {pc.crop_shift(c) for c in cis if c.valid and all(pc.crop_tiles_fit(c, S))} == {0, 1, 2, 3}
    assert any(not c.valid for c in cis)
    (crops, params), log = _logged(eng, lambda: eng.crop_faces(frame, boxes, S))
    assert [k for k in log if k.startswith("crop_resize")] == ["crop_resize_kernel"]
    _assert_crops(frame, boxes, S, crops, params)


def test_crop_float64_rows_unaligned_emu(emu_engine):
    check_crops_f64(emu_engine)


@pytest.mark.gpu
def test_crop_float64_rows_unaligned_gpu(gpu_engine):
    check_crops_f64(gpu_engine)


# ---- 4. pf_resize and pf_letterbox -----------------------------------------------------------------------------------------------
def check_resize(eng, hw, out_hw):
    assert pc.resize_path(hw, out_hw) == ("box" if (hw, out_hw) == ((200, 300), (100, 150)) else "taps")
    img = _random_image(hw, seed=hw[0] * 7 + out_hw[1])
    assert np.array_equal(eng.resize(img, out_hw), pp.resize_linear_u8(img, out_hw[1], out_hw[0]))


@pytest.mark.parametrize("hw,out_hw", pc.RESIZE_CASES, ids=_ids(pc.RESIZE_CASES))
def test_resize_emu(emu_engine, hw, out_hw):
    check_resize(emu_engine, hw, out_hw)


@pytest.mark.gpu
@pytest.mark.parametrize("hw,out_hw", pc.RESIZE_CASES, ids=_ids(pc.RESIZE_CASES))
def test_resize_gpu(gpu_engine, hw, out_hw):
    check_resize(gpu_engine, hw, out_hw)


def check_letterbox(eng, hw, out_hw):
    img = _random_image(hw, seed=hw[1])
    got, info = eng.letterbox(img, out_hw)
    ref, rinfo = pp.detector_preprocess_u8(img, out_hw)
    assert np.array_equal(got, ref)
    assert (info[0], info[1], info[2]) == (np.float32(rinfo[0]), rinfo[1], rinfo[2])


@pytest.mark.parametrize("hw,out_hw", pc.LETTERBOX_CASES, ids=_ids(pc.LETTERBOX_CASES))
def test_letterbox_odd_frames_emu(emu_engine, hw, out_hw):
    check_letterbox(emu_engine, hw, out_hw)


@pytest.mark.gpu
@pytest.mark.parametrize("hw,out_hw", pc.LETTERBOX_CASES, ids=_ids(pc.LETTERBOX_CASES))
def test_letterbox_odd_frames_gpu(gpu_engine, hw, out_hw):
    check_letterbox(gpu_engine, hw, out_hw)


# ---- 5. frame-difference sum -----------------------------------------------------------------------------------------------------
ABSDIFF_CLASS = {(1, 1): "short", (1, 5): "short", (1, 6): "tail", (3, 7): "tail", (37, 53): "tail", (64, 64): "whole"}


def check_absdiff(eng, hw):
    assert pc.absdiff_class(hw) == ABSDIFF_CLASS[hw]
    a, b = _random_image(hw, seed=1), _random_image(hw, seed=2)
    assert eng.set_frame(a) is None
    ref = np.abs(a.astype(np.int64) - b.astype(np.int64)).sum() / hw[0] / hw[1] / 3
    assert eng.set_frame(b) == ref
    assert eng.set_frame(np.zeros((hw[0] + 1, hw[1], 3), np.uint8)) is None         # a shape change has nothing to compare with


@pytest.mark.parametrize("hw", pc.ABSDIFF_SHAPES, ids=_ids(pc.ABSDIFF_SHAPES))
def test_absdiff_tails_emu(emu_engine, hw):
    check_absdiff(emu_engine, hw)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", pc.ABSDIFF_SHAPES, ids=_ids(pc.ABSDIFF_SHAPES))
def test_absdiff_tails_gpu(gpu_engine, hw):
    check_absdiff(gpu_engine, hw)


@pytest.mark.gpu
def test_absdiff_sum_above_32_bits_gpu(gpu_engine):
    """An all-0 then an all-255 frame at 2160 x 3840: the sum needs the 64-bit accumulator and atomic."""
    H, W = 2160, 3840
    total = H * W * 3 * 255
    assert total == 6345216000 and total > 2 ** 32
    assert gpu_engine.set_frame(np.zeros((H, W, 3), np.uint8)) is None
    assert gpu_engine.set_frame(np.full((H, W, 3), 255, np.uint8)) == total / H / W / 3

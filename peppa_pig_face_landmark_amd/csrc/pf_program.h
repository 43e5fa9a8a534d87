// Packed network program: the binary interface between the Python graph builder
// (peppa_pig_face_landmark_amd/graph/ir.py) and the HIP executor.  Every op's record has a named layout here (struct Pf<Name>Op) and the
// same list of names in ir.py's OP_LAYOUT; tests/test_program_layout.py reads this header as text and fails when the two disagree.
//
// A program is a straight-line list of fused layer ops over NHWC activation tensors that live in
// one device arena.  Everything is little-endian int32 (floats are bit-cast), so the Python side
// needs nothing but struct.pack.
//
//   blob := Header | BufRec[n_bufs] | TensorRec[n_tensors] | OpRec[n_ops] | pad to 256 | const bytes
//
// Buffers scale linearly with the batch: buffer i lives at arena + offset_units*256*max_batch and
// item b of it at + b * item_bytes.  Tensors are (buffer, channel offset, pixel stride) views, which
// is how torch.cat (DecoderBlock, ASPP, detector PAN) costs nothing: producers write channel slices.
#pragma once
#include <stdint.h>
#include <string.h>

#include <type_traits>

#define PF_PROGRAM_MAGIC 0x47504650  // "PFPG"
#define PF_PROGRAM_VERSION 11

enum PfElem : int32_t { PF_ELEM_ACT = 0, PF_ELEM_F32 = 1, PF_ELEM_I32 = 2, PF_ELEM_U8 = 3 };

struct PfHeader {
    int32_t magic, version, dtype, n_bufs, n_tensors, n_ops, const_bytes, arena_units_per_item;
    int32_t in_h, in_w, out_buf0, out_buf1, out_buf2, reserved0, reserved1, reserved2;
};
struct PfBufRec {
    int32_t etype, elems_per_item, offset_units, reserved;
};
struct PfTensorRec {
    int32_t buf, coff, ld, H, W, C, reserved0, reserved1;
};
#define PF_OP_FIELDS 39
struct PfOpRec {
    int32_t code;
    int32_t f[PF_OP_FIELDS];
    // the record as its op's layout (one of the Pf*Op structs below): the only way the executor reads `f`
    template <class R>
    R as() const {
        R r;
        memcpy(&r, f, sizeof(R));
        return r;
    }
};

enum PfOpCode : int32_t {
    PF_OP_STEM = 1,
    PF_OP_CONV = 2,
    PF_OP_DW = 3,
    PF_OP_UPCAT = 4,
    PF_OP_GAP = 5,
    PF_OP_FC = 6,
    PF_OP_SCSE = 7,
    PF_OP_HMDEC = 8,
    PF_OP_MAXPOOL = 9,
    PF_OP_COPY = 10,
    PF_OP_DETDEC = 11,
    PF_OP_SEPUP = 12,
    PF_OP_ADDUP = 13,
    PF_OP_MBCONV = 14,
    PF_OP_EXPDW = 15,
    PF_OP_CHAIN = 16,
    PF_OP_BLOCK = 17,
    PF_OP_DETUNIT = 18,
    PF_OP_DETC3 = 19,
    PF_OP_DETSTEM = 20,
    // (21 is unassigned)
    PF_OP_HRB = 22,
    PF_OP_FUSEUP = 23,
    PF_OP_MBX = 24,
    PF_OP_FC2 = 25,
    PF_OP_FRONT2 = 26,
    PF_OP_FACEATTR = 27,
};

// ---------------------------------------------------------------------------------------------
// Record layouts: struct Pf<Name>Op overlays PfOpRec::f of an op with code PF_OP_<NAME>, member by member in wire order; words
// behind the last member are zero.  Members are int32_t or float (bit-cast on the wire) and nothing else, so that every member is
// one word of `f`; a repeated tail is an array of a nested struct of the same kind.  Suffixes: _t = tensor index, _buf = buffer
// index, no suffix on a weight / bias name = byte offset into the program's constants; -1 = none wherever a comment says so.
// graph/ir.py OP_LAYOUT lists the same names in the same order for the packer; tests/test_program_layout.py reads this file as
// text and compares, so keep declarations in the plain shape they have: `int32_t a, b;` / `float x;` / `PfNested name[N];`.
#define PF_OP_LAYOUT(R, WORDS)                                                                                                    \
    static_assert(std::is_trivially_copyable<R>::value && std::is_standard_layout<R>::value && alignof(R) == 4, #R " must be plain words"); \
    static_assert(sizeof(R) == 4 * (WORDS) && (WORDS) <= PF_OP_FIELDS, #R ": every member is one 4-byte word and the record fits PfOpRec::f")

// 3x3 stride-2 pad-1 conv on the 3-channel program input (or on a tensor).  wt_u8 has 1/255 folded in (u8 input), wt_f32 serves a float
// input; mfma_w_* / s_* = the same weights pre-split for the staged-image matrix-core kernel of f32s programs (k_front.h; -1 = none).
struct PfStemOp {
    int32_t in_t, out_t, wt_u8, bias, act, wt_f32, mfma_w_u8, mfma_w_f32;      // in_t -1 = program input
    float s_u8, s_f32;
};
PF_OP_LAYOUT(PfStemOp, 10);

// Dense conv as implicit GEMM.  use_split: 0 direct kernel, 1 split precision, 2 split weights on ONE f16 product where a kernel has it.
// gap_parts_plus1: buffer + 1 of per-tile channel sums of the output, [face][(OHW / 128) * 4][Npad] (0 = none; the hero / halo 3x3
// kernels with 128 outputs only).  cfg = tile configuration (PF_CONV_NCFG below), -1 = chosen at launch.
struct PfConvOp {
    int32_t in_t, out_t, wt, bias, res_t, gate_buf, fbias_buf, KH, KW, stride, pad, dil, Cpad, Npad, N, act, outCs;      // res_t, gate_buf, fbias_buf: -1 = none
    int32_t amax_val_buf, amax_idx_buf, amaxN, store_out, cfg;      // amax_*_buf -1 = no arg-max epilogue
    float acc_scale;
    int32_t use_split, gap_parts_plus1;
};
PF_OP_LAYOUT(PfConvOp, 25);

// depthwise K x K conv
struct PfDwOp {
    int32_t in_t, out_t, wt, bias, K, stride, pad, dil, act;
};
PF_OP_LAYOUT(PfDwOp, 9);

// out = cat(bilinear_x2(lo), skip)
struct PfUpcatOp {
    int32_t lo_t, skip_t, out_t;
};
PF_OP_LAYOUT(PfUpcatOp, 3);

// per-face channel means
struct PfGapOp {
    int32_t in_t, out_buf;
};
PF_OP_LAYOUT(PfGapOp, 2);

// y = act2(scale2 * act(W x + b) + shift2) on pooled f32 vectors (scale2, shift2: -1 = none)
struct PfFcOp {
    int32_t x_buf, y_buf, wt, bias, K, N, act, scale2, shift2, act2;
};
PF_OP_LAYOUT(PfFcOp, 10);

// concurrent spatial / channel squeeze-excite.  gap_parts_plus1: buffer + 1 of per-32-pixel-tile channel sums of the output,
// [face][HW / 32][C] (0 = none; k_layers.h scse_tile_sum_kernel)
struct PfScseOp {
    int32_t in_t, out_t, cse_buf, sse_w;
    float sse_b;
    int32_t gap_parts_plus1;
};
PF_OP_LAYOUT(PfScseOp, 6);

// heat-map decode: arg-max slots + offset head -> landmark coordinates and scores
struct PfHmdecOp {
    int32_t val_buf, idx_buf, feat_t, off_wt, off_bias, P, nslots, loc_buf, score_buf;
};
PF_OP_LAYOUT(PfHmdecOp, 9);

// 2x2 stride 2, ceil mode
struct PfMaxpoolOp {
    int32_t in_t, out_t;
};
PF_OP_LAYOUT(PfMaxpoolOp, 2);

// channel-strided copy, optional nearest x`up` upsample
struct PfCopyOp {
    int32_t in_t, out_t, out_cs, up;
};
PF_OP_LAYOUT(PfCopyOp, 4);

// decode of one Detect level into rows [row0, row0 + 3 H W) of rows_buf; anchors = 6 floats
struct PfDetdecOp {
    int32_t in_t, rows_buf, row0;
    float stride;
    int32_t anchors, nrows_total;
};
PF_OP_LAYOUT(PfDetdecOp, 6);

// fused bilinear-x2-upsample + concat + depthwise 3x3 + pointwise conv (split kernels).  dw_e = the lo channels' depthwise filters with
// the upsample folded in (16 position classes), dw_b = zeros (the depthwise bias is folded into pw_bias), dw_skip = the skip channels'
// filters, dw_lo = the lo channels' plain filters [9][C1], dw_v = [4 row classes][9][C1] with the vertical interpolation folded in,
// skipx_buf = scratch of the pipelined kernel, gap_parts_plus1 = buffer + 1 of per-tile channel sums of the output (0 = none)
struct PfSepupOp {
    int32_t lo_t, skip_t, out_t, dw_e, dw_b, pw_wt, pw_bias, Cpad, Npad, N, act;
    float acc_scale;
    int32_t dw_skip, skipx_buf, dw_lo, dw_v, gap_parts_plus1;
};
PF_OP_LAYOUT(PfSepupOp, 17);

// out = act(a + nearest_up(b, 2^shift))
struct PfAddupOp {
    int32_t a_t, b_t, out_t, shift, act;
};
PF_OP_LAYOUT(PfAddupOp, 5);

// Inverted-residual block (expand 1x1 -> depthwise 3x3 -> project 1x1 [+ res]) in one launch (k_mbconv.h).  variant: 0 split (KS = Cin / 32),
// 1 exact f32 (KS = Cin padded to 16), 2 no expand conv, 3 ShuffleNetV2 unit, which reads `shuffle` (separate activations,
// channel-strided store, pass-through copy; pass_src_t -1 = none)
struct PfMbconvShuffle {
    int32_t act_dw, act_out, out_cs, pass_src_t, pass_dst_t;
};
struct PfMbconvOp {
    int32_t in_t, out_t, res_t, w_exp, b_exp, w_dw, b_dw, w_pwl, b_pwl, K, stride, pad, dil, act, MidPad, KS, CoutPad, Cout, Mid16;      // res_t -1 = none
    float scale_exp, scale_pwl;
    int32_t variant;
    PfMbconvShuffle shuffle[1];
};
PF_OP_LAYOUT(PfMbconvOp, 27);

// pointwise expand + depthwise K x K in one launch, the expanded tensor stays in LDS; gap_buf = per-face channel means of the output
// (-1 = none); stride 0 = 1
struct PfExpdwOp {
    int32_t in_t, out_t, gap_buf, w_exp, b_exp, w_dw, b_dw, K, pad, dil, act, Cpad, Npad, N;
    float acc_scale;
    int32_t stride;
};
PF_OP_LAYOUT(PfExpdwOp, 16);

// one 3x3 conv of a BasicBlock (PF_OP_CHAIN, PF_OP_BLOCK)
struct PfBlockConv {
    int32_t wt, bias;
    float acc_scale;
};
// chain of BasicBlocks (two 3x3 convs + identity residual each; n_convs of `convs` used), one face's map resident in LDS (k_chain.h);
// split programs only
struct PfChainOp {
    int32_t in_t, out_t, n_convs, C;
    PfBlockConv convs[11];
};
PF_OP_LAYOUT(PfChainOp, 37);

// one BasicBlock, TR rows per workgroup, flat-K weights (k_chain.h basic_block_kernel); split programs only
struct PfBlockOp {
    int32_t in_t, out_t, C;
    PfBlockConv convs[2];
};
PF_OP_LAYOUT(PfBlockOp, 9);

// a whole ShuffleV2Block of the detector per launch (k_det.h det_unit_kernel); in_t = the block's input (stride 1: both halves), out_t =
// its 2C-channel output (channel shuffle folded into the store); wd1, bd1, w3, b3, s3 = branch 1 of a stride-2 block (-1 = none);
// split programs only
struct PfDetunitOp {
    int32_t in_t, out_t, w1, b1, wd, bd, w2, b2, wd1, bd1, w3, b3;
    float s1, s2, s3;
    int32_t C, K1, stride, Cin;
};
PF_OP_LAYOUT(PfDetunitOp, 19);

// a C3 block of the detector's PAN head per launch (k_det.h det_c3_kernel) on the concatenation [srcA (nearest x2 upsampled if upA) | srcB];
// tail 1 = + a 1x1 conv (silu) into out2, tail 2 = + the Detect conv (raw output into out2 if given) and its decode into rows_buf;
// srcB_t, out_t, out2_t, rows_buf, anchors: -1 = none; split programs only
struct PfDetc3Op {
    int32_t srcA_t, srcB_t, out_t, out2_t, rows_buf, wA, bA, wB, bB, wC, bC, wD, bD, wE, bE, anchors;
    float sA, sB, sC, sD, sE, det_stride;
    int32_t CIN, tail, upA, row0, nrows_total;
};
PF_OP_LAYOUT(PfDetc3Op, 27);

// the detector's StemBlock (stem_1 3x3 s2, stem_2a 1x1, stem_2b 3x3 s2, max-pool, stem_3 1x1) in one launch on the program input
// (k_det.h det_stem_kernel)
struct PfDetstemOp {
    int32_t out_t, w1_u8, w1_f32, b1, w2a, b2a, w2b, b2b, w3, b3;
    float s1_u8, s1_f32, s2a, s2b, s3;
};
PF_OP_LAYOUT(PfDetstemOp, 15);

// an HRNet Bottleneck (1x1 -> 3x3 -> 1x1 + shortcut, mid 64, out 256; wd / bd = the first block's shortcut conv, -1 = identity) in one
// launch (k_hrb.h hr_bottleneck_kernel); split programs only
struct PfHrbOp {
    int32_t in_t, out_t, w1, b1, w2, b2, w3, b3, wd, bd;
    float s1, s2, s3, sd;
    int32_t CIN;
};
PF_OP_LAYOUT(PfHrbOp, 15);

// an HRNet fuse sum towards a higher-resolution branch, out = act(y + sum_s nearest_up(conv1x1_s(src_s), 2^shift_s)) over the first nsrc
// of `src` (src_t -1 = unused), weights f32 [srcC][C padded to 4] (k_layers.h fuse_up_kernel); f32 tensors only
struct PfFuseupSrc {
    int32_t src_t, wt, bias, shift;
};
struct PfFuseupOp {
    int32_t y_t, out_t, act, nsrc;
    PfFuseupSrc src[3];
    int32_t C;
};
PF_OP_LAYOUT(PfFuseupOp, 17);

// a whole inverted-residual block at 16 x 16 with the face's input stationary in registers and the expanded tile in LDS (k_mbx.h
// mbx_kernel); mode 0 = block without squeeze-excite, 1 = expand + depthwise -> per-face channel means into gap_buf (the SE squeeze),
// 2 = expand + depthwise recomputed, x gate_buf, projected (+ res), 3 = mode 1 + the activated depthwise map stored in out_t (for the
// layer-wise gated projection); out_t, res_t, gap_buf, gate_buf, w2, b2: -1 = none; waves = 8 | 16; split programs only
struct PfMbxOp {
    int32_t in_t, out_t, res_t, gap_buf, gate_buf, w1, ctile, w2, b2, K, pad, dil, act, KS, T, Cout, Cexp;
    float scale1, scale2;
    int32_t mode, waves;
};
PF_OP_LAYOUT(PfMbxOp, 21);

// two dependent FCs on pooled vectors in one launch; x = xscale * sum of nparts partial vectors (nparts 0 = 1; k_layers.h fc2_kernel:
// SE gate, cSE gate, ASPP pooled branch); K, R <= 960, R % 4 == 0, N % 4 == 0; b1, scale2, shift2, b2: -1 = none
struct PfFc2Op {
    int32_t x_buf, y_buf, w1, b1, K, R, act1, scale2, shift2, act1b, w2, b2, N, act2, nparts;
    float xscale;
};
PF_OP_LAYOUT(PfFc2Op, 16);

// conv_stem + blocks.0.0 of the Student encoder (3x3 s2 3 -> 16 + act, depthwise 3x3 + relu -> 1x1 16 -> 16 + x) in one launch on the
// program input (k_front2.h); split programs only
struct PfFront2Op {
    int32_t out_t, w_u8, w_f32, b_stem;
    float s_u8, s_f32;
    int32_t act_stem, w_dw, b_dw, w_pw, b_pw;
};
PF_OP_LAYOUT(PfFront2Op, 11);

// the landmark network's fc head (model.py:269,286-293) on partial-sum slabs / pooled means of three sources (decx4, decx8, encx16):
// pooled = scale * (sum of nparts vectors of ld floats, first C used); one record per face (k_layers.h face_attrs_kernel, record layout
// PF_FACE_ATTR_* below); programs built with face_attrs=True only
struct PfFaceattrSrc {
    int32_t src_buf, nparts, C, ld;
    float scale;
};
struct PfFaceattrOp {
    int32_t out_buf, wt, bias;
    PfFaceattrSrc src[3];
};
PF_OP_LAYOUT(PfFaceattrOp, 18);

// Face-attribute record (out_buf2 of a program built with face_attrs=True): 16 f32 per face.
//   [0, 7)   raw x of Net.forward's first output (model.py:293): x[0:3] head pose / 90, x[3:7] face-state logits
//   [7]      0
//   [8, 11)  head pose in degrees, 90 * x[0:3], in cv2.decomposeProjectionMatrix's order (about x, y, z; headpose.py:48-78)
//   [11, 15) sigmoid(x[3:7]): eye of points 60-67 closed, eye of points 68-75 closed, mouth closed, mouth wide open
//   [15]     0
#define PF_FACE_ATTR_REC 16
#define PF_FACE_ATTR_RAW 0
#define PF_FACE_ATTR_COOKED 8

// tile configurations of conv_gemm_kernel (index = cfg field)
#define PF_CONV_NCFG 9

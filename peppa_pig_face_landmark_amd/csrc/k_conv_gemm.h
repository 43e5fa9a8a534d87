// Implicit-GEMM convolution on the CDNA4 matrix cores (1x1 and kxk dense convs, NHWC).
//
// Replaces what onnxruntime's CPU conv kernels compute for the reference
// (Skps/core/api/onnx_model_base.py:23-24) for every dense conv of the landmark regressor
// (TRAIN/face_landmark/lib/core/base_trainer/model.py: 1x1 expand/project convs of the encoder,
// ASPP :70-83, DecoderBlock conv1/conv2 :146-172, hm head :271) and of the detector.
//
// GEMM view:  D[n][m] = sum_k  W[n][k] * X[m][k]
//   m = output pixel (b, oy, ox) flattened,  n = output channel,  k = (tap, input channel)
//   MFMA "A" operand = weight rows, "B" operand = pixels, so each lane ends up owning 4 consecutive
//   output channels of one pixel (contiguous in NHWC -> one 8/16-byte store per accumulator).
//
// Tiling: block = 256 threads = 4 waves arranged WARPS_M x WARPS_N over a BM(pixels) x BN(channels)
// tile; K advances 64 bytes per step (32 f16 / 16 f32 per row) through two LDS stages
// (register-staged global->LDS copy overlapping the MFMAs of the previous stage).  The 16-byte
// chunk index inside a 64-byte LDS row is rotated by 2*(row>>2) so that the four 16-lane groups
// of a ds_read_b128 fragment read hit 16 distinct bank slots.
//
// Fused epilogue: + bias[n] (BN folded) (+ per-face bias) (+ residual) -> activation -> store,
// optional SE gate on the input channels (applied while staging), optional per-(face,channel)
// running arg-max for the heat-map head (COTRAIN.postp, model.py:520-522).
#pragma once
#include "pf_common.h"
#include <type_traits>
#include <utility>

struct ConvGemmArgs {
    const void* in;
    const void* wt;       // [Npad][KH*KW][Cpad], element type T, zero padded
    const float* bias;    // [Npad]
    void* out;
    const void* res;      // residual (same pixel indexing as out) or nullptr
    const float* gate;    // [B][inC] multiplicative gate on input channels, or nullptr
    const float* fbias;   // [B][Npad] per-face bias, or nullptr
    float* amax_val;      // [B][amaxN][nslots] partial maxima, or nullptr
    int* amax_idx;
    int B, inH, inW, inC, inLd;
    int outH, outW, N, Npad, outLd, outCs;  // channel n is stored at element n*outCs of the pixel row
    int outCpad;          // channels [N, outCpad) of the output view are written as zeros (vector padding)
    int resLd;
    int KH, KW, stride, pad, dil, Cpad;
    int act;
    int amaxN;
    int head_segs;        // pw_head_kernel (k_pwhead.h): work items per face
    int store_out;
    float acc_scale;      // split-precision kernels: 1 / (power-of-two weight scale); 1 otherwise
    // fused "upsample x2 (bilinear) + concat + depthwise 3x3 + BN" producer of the pixel operand
    // (DecoderBlock.forward model.py:184-189 + SeparableConv2d.conv_dw :21-27), STAGE == 1 kernels only
    const float* up_lo;   // [B][loH][loW][loLd]  channels [0, C1)   -> upsampled
    const float* up_skip; // [B][2loH][2loW][skipLd] channels [C1, C1+C2)
    const float* dw_w;    // [16 position classes][9][C1]: upsample (x) depthwise collapsed onto the low-res grid
    const float* dw_w2;   // [9][C2] plain depthwise weights of the skip channels (BN folded)
    const float* dw_b;    // [C1+C2]
    int loH, loW, C1, loLd, skipLd;
    // fused "pointwise expand -> depthwise kxk" (EPI != 0 kernels): dw_w2 = [K*K][N] depthwise weights, dw_b = [N]
    // bias, both BN folded; the depthwise output goes to `out`, its per-face channel means (SE squeeze) to gap_out
    float* gap_out;       // [B][N] or nullptr
    unsigned* range_slot; // f32s range guard: max |v| (raw bits) over everything this launch splits into f16 hi / lo, or nullptr
    int dbg;              // PEPPA_DBG bit mask of the ablation build, 0 in production: pf_ablate.h has the table (PF_ABL_* bits)
    // per-tile channel sums of the stored output (GAPP epilogue instances only, conv_gemm_epilogue): [B][nslots][Npad] f32,
    // nslots = (OHW / BM) * WARPS_M -- slot = (tile of the face, M-wave); the face-attribute head's pools (k_layers.h face_attrs_kernel)
    float* gap_parts;
};

template <typename T> struct ConvMma;
template <> struct ConvMma<pf_half> {
    static constexpr int KSUB = 1;   // one v_mfma_f32_16x16x32_f16 consumes the whole 64-byte K step
    __device__ static __forceinline__ pf_f32x4 step(pf_half8 w, pf_half8 x, pf_f32x4 c, int) {
        return pf_mfma_16x16x32_f16(w, x, c);
    }
};
template <> struct ConvMma<float> {
    static constexpr int KSUB = 4;   // four v_mfma_f32_16x16x4_f32 per 64-byte K step
    __device__ static __forceinline__ pf_f32x4 step(pf_f32x4 w, pf_f32x4 x, pf_f32x4 c, int ks) {
        return pf_mfma_16x16x4_f32(w[ks], x[ks], c);
    }
};

__device__ __forceinline__ int pf_lds_chunk_off(int row, int chunk) {
    return row * 64 + (((chunk + 2 * (row >> 2)) & 3) << 4);
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the fully unrolled K loops of k_conv_split.h and k_hero.h
template <int N, typename F, int... I> __device__ __forceinline__ void pf_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F> __device__ __forceinline__ void pf_static_for(F&& f) { pf_static_for_impl<N>(f, std::make_integer_sequence<int, N>{}); }

// ---- fused epilogue shared by the direct and the split-precision kernels ----------------------
// acc[j][i][r] = D[channel n0 + wn*WN + 16j + 4*(lane>>4) + r][pixel m0 + wm*WM + 16i + (lane&15)]
//
// GAPP (compile-time, off in every default instance): the epilogue also leaves the channel sums of exactly the values it stores
// (after bias, residual and activation) in a.gap_parts[face][slot][Npad], slot = (tile of the face) * WARPS_M + wm.  A lane adds its
// MT pixels per channel, the 16 lanes of a row (the 16 pixels of a sub-tile) meet by four DPP exchanges, lane 0 of the row stores
// its four channels as one vector.  Every slot is written by exactly one wave with a plain store and the consumer adds the slots in
// a fixed order: no atomics, the same bits at any batch size or tile-to-workgroup mapping.  Host guarantees: OHW % BM == 0, so a
// tile never straddles a face, and Npad % 4 == 0.
template <typename T, int BM, int BN, int WARPS_M, int WARPS_N, bool GAPP = false>
__device__ __forceinline__ void conv_gemm_epilogue(const ConvGemmArgs& a, pf_f32x4 (&acc)[BN / WARPS_N / 16][BM / WARPS_M / 16],
                                                   int m0, int n0, int wm, int wn, int lane, int M, int OHW, float acc_scale) {
    constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
    constexpr int MT = WM / 16, NT = WN / 16;
    T* __restrict__ out = static_cast<T*>(a.out);
    const T* __restrict__ res = static_cast<const T*>(a.res);
    const int pcol = lane & 15;        // pixel within the 16-wide sub-tile
    const int crow = (lane >> 4) * 4;  // first of the 4 channels this lane owns
    const bool want_amax = a.amax_val != nullptr;

    // every bias of this lane in one round trip (Npad is a multiple of 16: a lane's four channels are inside or outside together)
    pf_f32x4 bvv[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * WN + j * 16 + crow;
        bvv[j] = pf_f32x4{0.f, 0.f, 0.f, 0.f};
        if (n + 3 < a.Npad) bvv[j] = *reinterpret_cast<const pf_f32x4*>(a.bias + n);
    }
    const bool res_vec = res != nullptr && sizeof(T) == 4 && (a.resLd & 3) == 0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * WN + j * 16 + crow;
        float bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = bvv[j][r];
        // the residual vectors of this channel tile's MT pixel sub-tiles: one round trip per channel tile, not one per sub-tile
        pf_f32x4 rvv[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int m = m0 + wm * WM + i * 16 + pcol;
            rvv[i] = pf_f32x4{0.f, 0.f, 0.f, 0.f};
            if (res_vec && m < M && n + 3 < a.N) rvv[i] = *reinterpret_cast<const pf_f32x4*>(reinterpret_cast<const float*>(res) + (size_t)m * a.resLd + n);
        }
        float best_v[4];
        int best_i[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { best_v[r] = -3.0e38f; best_i[r] = 0x7fffffff; }
        float gsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int m = m0 + wm * WM + i * 16 + pcol;
            const bool mok = m < M;
            const int b = mok ? m / OHW : 0;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[j][i][r] * acc_scale + bv[r];
            if (a.fbias && mok) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < a.Npad) v[r] += a.fbias[(size_t)b * a.Npad + n + r];
            }
            if (res && mok) {
                if (res_vec && n + 3 < a.N) {      // one 16-byte load (views start on vector boundaries), requested above
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += rvv[i][r];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n + r < a.N) v[r] += (float)res[(size_t)m * a.resLd + n + r];
                }
            }
            pf_act_n<4>(v, a.act);
            if constexpr (GAPP) {
                if (mok) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) gsum[r] += v[r];
                }
            }
            if (want_amax && mok) {
                const int local = m - b * OHW;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (v[r] > best_v[r]) { best_v[r] = v[r]; best_i[r] = local; }
            }
            if (a.store_out && mok && !(pf_dbg(a) & PF_ABL_NO_STORE)) {
                T* o = out + (size_t)m * a.outLd;
                if (a.outCs == 1 && n + 3 < a.N) {
                    if constexpr (sizeof(T) == 2) {
                        pf_half4 pk;
#pragma unroll
                        for (int r = 0; r < 4; ++r) pk[r] = (pf_half)v[r];
                        *reinterpret_cast<pf_half4*>(o + n) = pk;
                    } else {
                        pf_f32x4 pk;
#pragma unroll
                        for (int r = 0; r < 4; ++r) pk[r] = v[r];
                        *reinterpret_cast<pf_f32x4*>(o + n) = pk;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (n + r < a.N) o[(size_t)(n + r) * a.outCs] = (T)v[r];
                        else if (n + r < a.outCpad) o[(size_t)(n + r) * a.outCs] = (T)0.f;
                    }
                }
            }
        }
        if constexpr (GAPP) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                gsum[r] += pf_row_xchg_f32<0>(gsum[r]);
                gsum[r] += pf_row_xchg_f32<1>(gsum[r]);
                gsum[r] += pf_row_xchg_f32<2>(gsum[r]);
                gsum[r] += pf_row_xchg_f32<3>(gsum[r]);
            }
            if (pcol == 0 && m0 < M && n + 3 < a.Npad) {
                const int b = m0 / OHW;
                const int nslots = (OHW / BM) * WARPS_M;
                const int slot = ((m0 - b * OHW) / BM) * WARPS_M + wm;
                *reinterpret_cast<pf_f32x4*>(a.gap_parts + ((size_t)b * nslots + slot) * a.Npad + n) = pf_f32x4{gsum[0], gsum[1], gsum[2], gsum[3]};
            }
        }
        if (want_amax) {
            // all BM pixels of this block belong to one face (host guarantees OHW % BM == 0)
#pragma unroll
            for (int mask = 1; mask < 16; mask <<= 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float ov = pf_shfl_xor_f32(best_v[r], mask);
                    const int oi = pf_shfl_xor_i32(best_i[r], mask);
                    if (ov > best_v[r] || (ov == best_v[r] && oi < best_i[r])) { best_v[r] = ov; best_i[r] = oi; }
                }
            }
            if (pcol == 0 && m0 < M) {
                const int b = m0 / OHW;
                const int blocks_per_face = OHW / BM;
                const int nslots = blocks_per_face * WARPS_M;
                const int slot = ((m0 - b * OHW) / BM) * WARPS_M + wm;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n + r < a.amaxN) {
                        const size_t o = ((size_t)b * a.amaxN + n + r) * nslots + slot;
                        a.amax_val[o] = best_v[r];
                        a.amax_idx[o] = best_i[r];
                    }
                }
            }
        }
    }
}

// ---- arg-max-only epilogue of the heat-map score head (COTRAIN.postp, model.py:520-522) ----------------------------------
// The generic epilogue above serves every conv of both networks through run-time switches (residual, per-face bias, five
// activations, strided stores, optional arg-max); on the score head -- bias only, nothing stored, 128-pixel tiles that
// never straddle a face -- those switches and the ds_bpermute shuffles of its arg-max were most of the kernel (SQ
// counters: VALU 56 % busy, MFMA 15 %).  This one does exactly the head's work: bias, running (max, first index) per
// lane, then a 16-lane reduction by DPP row exchanges.  Host guarantees: OHW % BM == 0 (so every pixel of the tile exists and
// belongs to one face), no residual / per-face bias / gate / activation, store_out == 0.
template <int BM, int BN, int WARPS_M, int WARPS_N>
__device__ __forceinline__ void conv_gemm_argmax_epilogue(const ConvGemmArgs& a, pf_f32x4 (&acc)[BN / WARPS_N / 16][BM / WARPS_M / 16],
                                                          int m0, int n0, int wm, int wn, int lane, int OHW, float acc_scale) {
    constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
    constexpr int MT = WM / 16, NT = WN / 16;
    const int pcol = lane & 15;
    const int crow = (lane >> 4) * 4;
    const int b = m0 / OHW;
    const int local0 = m0 - b * OHW + wm * WM + pcol;
    const int nslots = (OHW / BM) * WARPS_M;
    const int slot = ((m0 - b * OHW) / BM) * WARPS_M + wm;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * WN + j * 16 + crow;
        float best_v[4];
        int best_i[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float bv = (n + r < a.Npad) ? a.bias[n + r] : 0.f;
            best_v[r] = fmaf(acc[j][0][r], acc_scale, bv);
            best_i[r] = local0;
#pragma unroll
            for (int i = 1; i < MT; ++i) {           // ascending pixel index: strict > keeps the first maximum
                const float v = fmaf(acc[j][i][r], acc_scale, bv);
                if (v > best_v[r]) { best_v[r] = v; best_i[r] = local0 + i * 16; }
            }
        }
#define PF_AMAX_STEP(STEP)                                                                                   \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                              \
        const float ov = pf_row_xchg_f32<STEP>(best_v[r]);                                                    \
        const int oi = pf_row_xchg_i32<STEP>(best_i[r]);                                                      \
        if (ov > best_v[r] || (ov == best_v[r] && oi < best_i[r])) { best_v[r] = ov; best_i[r] = oi; }        \
    }
        PF_AMAX_STEP(0) PF_AMAX_STEP(1) PF_AMAX_STEP(2) PF_AMAX_STEP(3)
#undef PF_AMAX_STEP
        if (pcol == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < a.amaxN) {
                    const size_t o = ((size_t)b * a.amaxN + n + r) * nslots + slot;
                    a.amax_val[o] = best_v[r];
                    a.amax_idx[o] = best_i[r];
                }
        }
    }
}

// KS = 1: pointwise conv (1x1, stride 1, no padding) -- tap arithmetic compiled out;
// KS = 3: general kxk conv (any kernel size / stride / dilation / padding).
template <typename T, int BM, int BN, int WARPS_M, int WARPS_N, int KS>
__global__ __launch_bounds__(256) void conv_gemm_kernel(ConvGemmArgs a) {
    typedef typename PfVec<T>::type vec_t;
    constexpr int VE = PfVec<T>::N;       // elements per 16-byte chunk
    constexpr int KE = 4 * VE;            // elements per 64-byte K step
    constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
    constexpr int MT = WM / 16, NT = WN / 16;
    constexpr int XROWS = BM / 64;                     // pixel rows staged per thread
    constexpr int WROWS = (BN + 63) / 64;              // weight rows staged per thread
    constexpr int STAGE_BYTES = (BM + BN) * 64;
    static_assert(WARPS_M * WARPS_N == 4, "4 waves per block");
    static_assert(BM % 64 == 0 && WM % 16 == 0 && WN % 16 == 0, "tile shape");

    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE_BYTES];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int wm = wave % WARPS_M, wn = wave / WARPS_M;
    // XCD-aware tile order for kxk convs: workgroup b runs on XCD b % 8 (private 4 MiB L2 each), so
    // give every XCD a contiguous run of pixel tiles -- vertically adjacent tiles, which share their
    // halo rows, then meet in the same L2.  Pure speed choice; any mapping is correct.
    int mtile = blockIdx.x;
    if (KS != 1 && (gridDim.x & 7) == 0) mtile = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int m0 = mtile * BM;
    const int n0 = blockIdx.y * BN;
    const int OHW = a.outH * a.outW;
    const int M = a.B * OHW;
    const T* __restrict__ in = static_cast<const T*>(a.in);
    const T* __restrict__ wt = static_cast<const T*>(a.wt);

    // ---- per-thread staging geometry -------------------------------------------------
    const int chunk = t & 3;
    const int srow = t >> 2;  // 0..63
    int xb[XROWS], xiy0[XROWS], xix0[XROWS];
    bool xvalid[XROWS];
#pragma unroll
    for (int r = 0; r < XROWS; ++r) {
        const int m = m0 + srow + 64 * r;
        xvalid[r] = m < M;
        const int mm = xvalid[r] ? m : 0;
        const int b = mm / OHW;
        const int rem = mm - b * OHW;
        const int oy = rem / a.outW;
        const int ox = rem - oy * a.outW;
        xb[r] = b;
        xiy0[r] = KS == 1 ? oy : oy * a.stride - a.pad;
        xix0[r] = KS == 1 ? ox : ox * a.stride - a.pad;
    }
    const int taps = KS == 1 ? 1 : a.KH * a.KW;
    const int cchunks = a.Cpad / KE;
    const int nk = taps * cchunks;
    const size_t wrow_stride = (size_t)taps * a.Cpad;

    vec_t xreg[XROWS], wreg[WROWS];

    auto load_tile = [&](int tap, int cc) {
        const int ky = KS == 1 ? 0 : tap / a.KW;
        const int kx = KS == 1 ? 0 : tap - ky * a.KW;
        const int kelem = cc * KE + chunk * VE;
        const bool kok = kelem < a.inC;
#pragma unroll
        for (int r = 0; r < XROWS; ++r) {
            const int iy = KS == 1 ? xiy0[r] : xiy0[r] + ky * a.dil;
            const int ix = KS == 1 ? xix0[r] : xix0[r] + kx * a.dil;
            const bool ok = xvalid[r] && kok && (KS == 1 || ((unsigned)iy < (unsigned)a.inH && (unsigned)ix < (unsigned)a.inW));
            vec_t v = pf_zero_vec<T>();
            if (ok) {
                const size_t off = ((size_t)(xb[r] * a.inH + iy) * a.inW + ix) * a.inLd + kelem;
                v = pf_ldv<T>(in + off);
                if (a.gate) {
                    const float* g = a.gate + (size_t)xb[r] * a.inC + kelem;
#pragma unroll
                    for (int e = 0; e < VE; ++e) v[e] = (T)((float)v[e] * g[e]);
                }
            }
            xreg[r] = v;
        }
#pragma unroll
        for (int r = 0; r < WROWS; ++r) {
            const int row = srow + 64 * r;
            const int n = n0 + row;
            vec_t v = pf_zero_vec<T>();
            if (row < BN && n < a.Npad) v = pf_ldv<T>(wt + (size_t)n * wrow_stride + (size_t)tap * a.Cpad + kelem);
            wreg[r] = v;
        }
    };
    auto store_tile = [&](int stage) {
        unsigned char* xs = smem + stage * STAGE_BYTES;
        unsigned char* ws = xs + BM * 64;
#pragma unroll
        for (int r = 0; r < XROWS; ++r)
            *reinterpret_cast<vec_t*>(xs + pf_lds_chunk_off(srow + 64 * r, chunk)) = xreg[r];
#pragma unroll
        for (int r = 0; r < WROWS; ++r) {
            const int row = srow + 64 * r;
            if (row < BN) *reinterpret_cast<vec_t*>(ws + pf_lds_chunk_off(row, chunk)) = wreg[r];
        }
    };

    pf_f32x4 acc[NT][MT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[j][i] = pf_f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- main loop ---------------------------------------------------------------------
    int tap = 0, cc = 0;
    load_tile(tap, cc);
    store_tile(0);
    __syncthreads();
    const int frow = lane & 15, fchunk = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) {
            // channel-chunk outer, tap inner: the KH*KW shifted reads of one 64-byte channel chunk are
            // issued back to back, so the halo re-reads hit L1/L2 instead of going back to the fabric
            if (++tap == taps) { tap = 0; ++cc; }
            load_tile(tap, cc);
        }
        const unsigned char* xs = smem + cur * STAGE_BYTES;
        const unsigned char* ws = xs + BM * 64;
        vec_t xf[MT], wf[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
            xf[i] = *reinterpret_cast<const vec_t*>(xs + pf_lds_chunk_off(wm * WM + i * 16 + frow, fchunk));
#pragma unroll
        for (int j = 0; j < NT; ++j)
            wf[j] = *reinterpret_cast<const vec_t*>(ws + pf_lds_chunk_off(wn * WN + j * 16 + frow, fchunk));
        // issue order: all (j,i) accumulators for one k sub-step before the next sub-step, so that
        // consecutive MFMAs never depend on each other (v_mfma_f32_16x16x4_f32: 32-cycle issue, 40-cycle
        // dependent latency)
#pragma unroll
        for (int ks = 0; ks < ConvMma<T>::KSUB; ++ks)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[j][i] = ConvMma<T>::step(wf[j], xf[i], acc[j][i], ks);
        if (more) store_tile(cur ^ 1);
        __syncthreads();
    }

    conv_gemm_epilogue<T, BM, BN, WARPS_M, WARPS_N>(a, acc, m0, n0, wm, wn, lane, M, OHW, 1.0f);
}

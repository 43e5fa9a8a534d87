#pragma once
#include "k_conv_gemm.h"

// ---- fused depthwise epilogue (MobileNetV3 inverted residual, expand -> depthwise, model.py:252-264) -------
// The workgroup's BM pixels are BM / (H*W) WHOLE images (host guarantees H*W divides BM, W <= 16), so the
// expanded tile act(acc) can stay in LDS and the k x k depthwise conv (+bias, act) reads it from there:
// the expanded tensor -- the largest one of the block -- never exists in HBM.  Thread = (channel, image row):
// per filter row it loads the W-pixel input row once and slides the filter along it in registers.  Also
// emits the per-face channel means of the depthwise output (the SE squeeze), complete because a workgroup
// owns whole images.
// WS = compile-time image width (16: the shape of every such layer of the Student at 256 x 256; 0 = read it from the
// arguments): with the width known the per-pixel "x < W" selects, the row / image index divisions and the padding tests
// fold away -- the epilogue is VALU-bound (57 % VALU busy, 12 % MFMA by SQ counters), so instruction count is its time.
template <int BM, int BN, int WARPS_M, int WARPS_N, int K, int DIL, int WS>
__device__ __forceinline__ void expdw_epilogue(const ConvGemmArgs& a, pf_f32x4 (&acc)[BN / WARPS_N / 16][BM / WARPS_M / 16],
                                               unsigned char* smem, int m0, int n0, int wm, int wn, int t, int M) {
    constexpr int NTHR = WARPS_M * WARPS_N * 64;
    constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
    constexpr int MT = WM / 16, NT = WN / 16;
    constexpr int ES = BN + 4;                 // E row stride (floats)
    constexpr int NG = NTHR / BN;              // row groups
    constexpr int MAXF = 4;                    // images per workgroup
    constexpr int PAD = DIL * (K - 1) / 2;
    constexpr int MAXW = 16;
    static_assert(NTHR % BN == 0, "thread = (channel, row group)");
    float* es = reinterpret_cast<float*>(smem);          // [BM][ES]
    float* sums = es + BM * ES;                           // [NG][MAXF][BN]
    const int lane = t & 63;
    const int pcol = lane & 15, crow = (lane >> 4) * 4;
    const int c = t % BN, g = t / BN;
    const int n = n0 + c;
    const bool cok = n < a.N;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int nl = wn * WN + j * 16 + crow;
        float bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = (n0 + nl + r < a.Npad) ? a.bias[n0 + nl + r] : 0.f;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            pf_f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaf(acc[j][i][r], a.acc_scale, bv[r]);
            pf_act_rh<4>(v, a.act);
            *reinterpret_cast<pf_f32x4*>(es + (wm * WM + i * 16 + pcol) * ES + nl) = v;
        }
    }
    if constexpr (WS == 16 && BM == 256 && BN == 64 && NTHR == 512) {
        // One 16 x 16 image per workgroup: thread = (channel PAIR, image row).  Two adjacent channels of a pixel are one aligned
        // 8-byte LDS word, so every tap is a v_pk_fma_f32 on a ds_read_b64 operand -- half the VALU and LDS instructions of the
        // one-channel-per-thread form below (the launch is VALU-bound: 57 % VALU busy against 12 % matrix pipe).  The filter taps
        // sit in LDS (6.4 KB at 5 x 5) instead of 2 x 25 registers.  Same fma order per output as the generic path.
        constexpr int KK = K * K;
        float* wks = sums + 16 * BN;                     // [K * K][BN]
        static_assert((BM * ES + 16 * BN + KK * BN) * 4 <= 80 * 1024, "E tile + row sums + taps: two workgroups per CU");
        {
            float wv[(KK * BN + NTHR - 1) / NTHR];
#pragma unroll
            for (int i = 0; i < (KK * BN + NTHR - 1) / NTHR; ++i) {
                const int id = t + i * NTHR;
                const int k = id / BN, cc = id - k * BN;
                wv[i] = (id < KK * BN && n0 + cc < a.N) ? a.dw_w2[(size_t)k * a.N + n0 + cc] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < (KK * BN + NTHR - 1) / NTHR; ++i)
                if (t + i * NTHR < KK * BN) wks[t + i * NTHR] = wv[i];
        }
        const int c2 = (t & 31) * 2, row = t >> 5;
        const int n2 = n0 + c2;
        pf_f32x2 bd2;
        bd2[0] = n2 < a.N ? a.dw_b[n2] : 0.f;
        bd2[1] = n2 + 1 < a.N ? a.dw_b[n2 + 1] : 0.f;
        __syncthreads();
        pf_f32x2 o[16];
#pragma unroll
        for (int x = 0; x < 16; ++x) o[x] = bd2;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int yy = row + ky * DIL - PAD;
            if ((unsigned)yy >= 16u || (pf_dbg(a) & PF_ABL_EXPDW_NO_DW_TAPS)) continue;
            const float* erow = es + (yy * 16) * ES + c2;
            pf_f32x2 in[16];
#pragma unroll
            for (int x = 0; x < 16; ++x) in[x] = *reinterpret_cast<const pf_f32x2*>(erow + x * ES);
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const pf_f32x2 w = *reinterpret_cast<const pf_f32x2*>(wks + (ky * K + kx) * BN + c2);
#pragma unroll
                for (int x = 0; x < 16; ++x) {
                    const int xx = x + kx * DIL - PAD;       // compile-time register index
                    if (xx >= 0 && xx < 16) o[x] = __builtin_elementwise_fma(w, in[xx], o[x]);
                }
            }
            asm volatile("" ::: "memory");       // one filter row's LDS reads in flight at a time (register footprint)
        }
        float of[32];
#pragma unroll
        for (int x = 0; x < 16; ++x) { of[2 * x] = o[x][0]; of[2 * x + 1] = o[x][1]; }
        pf_act_rh<32>(of, a.act);
        const int m = m0 + row * 16;
        pf_f32x2 rs = pf_f32x2{0.f, 0.f};
        float* out = static_cast<float*>(a.out);
        if (m < M && !(pf_dbg(a) & PF_ABL_NO_STORE)) {
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                float* po = out + (size_t)(m + x) * a.outLd + n2;
                if (n2 + 1 < a.N) *reinterpret_cast<pf_f32x2*>(po) = pf_f32x2{of[2 * x], of[2 * x + 1]};
                else if (n2 < a.N) po[0] = of[2 * x];
                rs[0] += of[2 * x];
                rs[1] += of[2 * x + 1];
            }
        }
        if (a.gap_out) {
            *reinterpret_cast<pf_f32x2*>(sums + row * BN + c2) = rs;
            __syncthreads();
            if (t < BN && n0 + t < a.N) {
                float tot = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) tot += sums[r * BN + t];
                const int b = m0 / 256;
                if (b < a.B) a.gap_out[(size_t)b * a.N + n0 + t] = tot / 256.f;
            }
        }
        return;
    }
    float wk[K * K];                           // requested before the barrier (accumulators are dead by now)
#pragma unroll
    for (int k = 0; k < K * K; ++k) wk[k] = cok ? a.dw_w2[(size_t)k * a.N + n] : 0.f;
    const float bd = cok ? a.dw_b[n] : 0.f;
    __syncthreads();
    const int W = WS ? WS : a.outW, H = WS ? WS : a.outH, OHW = H * W;
    const int rows = BM / W;
    float fsum[MAXF];
#pragma unroll
    for (int f = 0; f < MAXF; ++f) fsum[f] = 0.f;
    float* out = static_cast<float*>(a.out);
    for (int r = g; r < rows; r += NG) {
        const int f = r / H, y = r - f * H;
        float o[MAXW];
#pragma unroll
        for (int x = 0; x < MAXW; ++x) o[x] = bd;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int yy = y + ky * DIL - PAD;
            if ((unsigned)yy >= (unsigned)H) continue;
            const float* erow = es + ((f * H + yy) * W) * ES + c;
            float in[MAXW];
#pragma unroll
            for (int x = 0; x < MAXW; ++x) in[x] = x < W ? erow[x * ES] : 0.f;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const float w = wk[ky * K + kx];
#pragma unroll
                for (int x = 0; x < MAXW; ++x) {
                    const int xx = x + kx * DIL - PAD;       // compile-time register index
                    if (xx >= 0 && xx < MAXW) o[x] = fmaf(w, in[xx], o[x]);   // in[xx] is 0 beyond the image width
                }
            }
            asm volatile("" ::: "memory");       // one filter row's LDS reads in flight at a time (register footprint)
        }
        pf_act_rh<MAXW>(o, a.act);
        const int m = m0 + r * W;                             // first pixel of the row
        if (cok && m < M) {
            float rs = 0.f;
#pragma unroll
            for (int x = 0; x < MAXW; ++x)
                if (x < W) {
                    out[(size_t)(m + x) * a.outLd + n] = o[x];
                    rs += o[x];
                }
#pragma unroll
            for (int ff = 0; ff < MAXF; ++ff)
                if (ff == f) fsum[ff] += rs;
        }
    }
    if (a.gap_out) {
#pragma unroll
        for (int f = 0; f < MAXF; ++f) sums[(g * MAXF + f) * BN + c] = fsum[f];
        __syncthreads();
        const int faces = BM / OHW;
        if (t < faces * BN) {
            const int f = t / BN, cc = t - f * BN;
            float tot = 0.f;
#pragma unroll
            for (int gg = 0; gg < NG; ++gg) tot += sums[(gg * MAXF + f) * BN + cc];
            const int b = m0 / OHW + f;
            if (b < a.B && n0 + cc < a.N) a.gap_out[(size_t)b * a.N + n0 + cc] = tot / (float)OHW;
        }
    }
}

// ---- expand 1x1 -> depthwise k x k (+ SE squeeze) on 32 x 32 maps: one workgroup = one image x 16 expanded channels ----
// The 16 x 16 variant above (expdw_epilogue, called from conv_gemm_split_kernel<.., EPI_K != 0> in k_conv_split.h) owns whole images inside a 256-pixel GEMM tile; a 32 x 32 image is 1024
// pixels, too many rows for the GEMM's LDS staging.  With <= 64 input channels (stage 2 of the Student: 40 -> 120) the
// expand GEMM is tiny, so it skips LDS altogether: every wave loads the pixel fragments of its 128 pixels straight from
// global memory (the image's 160 KB of input is re-read by the 8 channel tiles out of L2), splits them and runs
// 3 MFMAs per 16 x 16 tile; the activated 32 x 32 x 16 tile (67 KB, rows padded so four rows land in different banks)
// lives in LDS and the depthwise conv reads it there, thread = (channel, image row), as in the 16 x 16 kernel.
// ACT >= 0: the activation at compile time (as in k_mbconv.h: the run-time switch put two scalar branches behind every 16-pixel tile of
// the expand loop and the tiles could not overlap).
template <int K, int DIL, int ACT = -1>
__global__ __launch_bounds__(512, 4) void expdw_image_kernel(ConvGemmArgs a) {
    unsigned amax = 0;                                 // range guard (pf_common.h)
    const unsigned amax_seen = pf_amax_seen(a.range_slot);
    constexpr int HW = 32, CB = 16;
    constexpr int RS = HW * CB + 16;            // floats per image row in LDS
    constexpr int PAD = DIL * (K - 1) / 2;
    constexpr int MAXKS = 2;                    // input channels <= 64
    __shared__ __attribute__((aligned(16))) float es[HW * RS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x, n0 = blockIdx.y * CB;
    const bool track = blockIdx.y == 0;
    const int frow = lane & 15, kg = lane >> 4;
    const int ksteps = a.Cpad / 32;
    const float* __restrict__ in = static_cast<const float*>(a.in) + (size_t)b * HW * HW * a.inLd;
    const unsigned char* __restrict__ wt = static_cast<const unsigned char*>(a.wt);
    // weight fragments of this channel tile (rows n0 + frow), all K steps
    pf_half8 whf[MAXKS], wlf[MAXKS];
    {
        const int row = min(n0 + frow, a.Npad - 1);
#pragma unroll
        for (int ks = 0; ks < MAXKS; ++ks) {
            whf[ks] = pf_half8{0, 0, 0, 0, 0, 0, 0, 0};
            wlf[ks] = whf[ks];
            if (ks < ksteps) {
                const unsigned char* p = wt + ((size_t)row * ksteps + ks) * 128 + kg * 16;
                whf[ks] = *reinterpret_cast<const pf_half8*>(p);
                wlf[ks] = *reinterpret_cast<const pf_half8*>(p + 64);
            }
        }
    }
    const int cch = 4 * kg;                     // accumulator layout: channels cch..cch+3 of pixel frow
    pf_f32x4 bv;
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = (n0 + cch + r < a.Npad) ? a.bias[n0 + cch + r] : 0.f;
    // ---- expand: 8 waves x 8 tiles of 16 pixels ----------------------------------------------------------------
#pragma unroll 2
    for (int mt = 0; mt < 8; ++mt) {
        const int p = wave * 128 + mt * 16 + frow;
        const float* px = in + (size_t)p * a.inLd;
        pf_f32x4 acc = pf_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < MAXKS; ++ks) {
            if (ks < ksteps) {
                const int c = ks * 32 + kg * 8;
                pf_f32x4 v0 = pf_f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
                if (c < a.inC) {                // inC % 8 == 0
                    v0 = *reinterpret_cast<const pf_f32x4*>(px + c);
                    v1 = *reinterpret_cast<const pf_f32x4*>(px + c + 4);
                }
                pf_half8 xh, xl;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = e < 4 ? v0[e & 3] : v1[e & 3];
                    const pf_half hv = (pf_half)v;
                    xh[e] = hv;
                    xl[e] = pf_split_lo(v, hv);
                }
                if (track) {                    // (wave-uniform) the eight channel tiles of an image split the SAME input: one of them reports its range
#pragma unroll
                    for (int e = 0; e < 8; ++e) amax = pf_amax(amax, e < 4 ? v0[e & 3] : v1[e & 3]);
                }
                acc = pf_mfma_16x16x32_f16(wlf[ks], xh, acc);
                acc = pf_mfma_16x16x32_f16(whf[ks], xl, acc);
                acc = pf_mfma_16x16x32_f16(whf[ks], xh, acc);
            }
        }
        pf_f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaf(acc[r], a.acc_scale, bv[r]);
        if constexpr (ACT >= 0) {
#pragma unroll
            for (int q_ = 0; q_ < 4; ++q_) v[q_] = pf_act_c<ACT>(v[q_]);
        } else pf_act_rh<4>(v, a.act);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n0 + cch + r >= a.N) v[r] = 0.f;
        *reinterpret_cast<pf_f32x4*>(es + (p >> 5) * RS + (p & 31) * CB + cch) = v;
    }
    // depthwise filters of this thread's channel (requested before the barrier)
    const int c = t & 15, y = t >> 4;
    const int n = n0 + c;
    const bool cok = n < a.N;
    float wk[K * K];
#pragma unroll
    for (int k = 0; k < K * K; ++k) wk[k] = cok ? a.dw_w2[(size_t)k * a.N + n] : 0.f;
    const float bd = cok ? a.dw_b[n] : 0.f;
    __syncthreads();
    // ---- depthwise: thread = (channel c, image row y) -------------------------------------------------------------
    float o[HW];
#pragma unroll
    for (int x = 0; x < HW; ++x) o[x] = bd;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const int yy = y + ky * DIL - PAD;
        if ((unsigned)yy >= (unsigned)HW) continue;
        const float* erow = es + yy * RS + c;
        float iv[HW];
#pragma unroll
        for (int x = 0; x < HW; ++x) iv[x] = erow[x * CB];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const float w = wk[ky * K + kx];
#pragma unroll
            for (int x = 0; x < HW; ++x) {
                const int xx = x + kx * DIL - PAD;           // compile-time register index
                if (xx >= 0 && xx < HW) o[x] = fmaf(w, iv[xx], o[x]);
            }
        }
    }
    if constexpr (ACT >= 0) {
#pragma unroll
        for (int q_ = 0; q_ < HW; ++q_) o[q_] = pf_act_c<ACT>(o[q_]);
    } else pf_act_rh<HW>(o, a.act);
    float rs = 0.f;
    if (cok) {
        float* out = static_cast<float*>(a.out) + ((size_t)b * HW * HW + (size_t)y * HW) * a.outLd + n;
#pragma unroll
        for (int x = 0; x < HW; ++x) {
            out[(size_t)x * a.outLd] = o[x];
            rs += o[x];
        }
    }
    if (track) pf_amax_commit(a.range_slot, amax, amax_seen);
    if (a.gap_out) {
        __syncthreads();                        // E is dead: its LDS becomes the row-sum scratch
        es[y * CB + c] = rs;
        __syncthreads();
        if (t < CB && n0 + t < a.N) {
            float tot = 0.f;
#pragma unroll
            for (int r = 0; r < HW; ++r) tot += es[r * CB + t];
            a.gap_out[(size_t)b * a.N + n0 + t] = tot / (float)(HW * HW);
        }
    }
}

// ---- same for the stride-2 block that enters stage 2 (64 x 64 x 24 -> expand 72 -> depthwise 5x5 / 2 -> 32 x 32) -------------
// One workgroup = one image x 16 expanded channels, looping over the four 16 x 16 output quadrants: per quadrant the
// expand conv is evaluated on the 35 x 35 input pixels the quadrant's windows cover (1.2x recompute, input from L2,
// pixels outside the image forced to 0 = the depthwise conv's zero padding), parked in LDS (78 KB) and consumed by the
// strided depthwise conv, thread = (channel, output row, half row).  The SE squeeze is complete per workgroup because it
// visits all four quadrants.  Input channels <= 32 (one K step).
template <int K, int ACT = -1>
__global__ __launch_bounds__(512, 4) void expdw_image_s2_kernel(ConvGemmArgs a) {
    unsigned amax = 0;                                 // range guard (pf_common.h)
    const unsigned amax_seen = pf_amax_seen(a.range_slot);
    constexpr int IN = 64, OUT = 32, Q = 16, CB = 16;    // input / output size, quadrant size, channels per workgroup
    constexpr int PAD = (K - 1) / 2;
    constexpr int R = (Q - 1) * 2 + K;                   // 35: input rows / columns a quadrant needs
    constexpr int RS = R * CB + 8;                       // floats per region row: 2 * RS = 48 (mod 64) -> 4 output rows, 4 bank groups
    constexpr int NPX = R * R, MTILES = (NPX + 15) / 16;
    constexpr int OX = Q / 2, SPAN = (OX - 1) * 2 + K;   // outputs per thread along x, input span they need
    __shared__ __attribute__((aligned(16))) float es[R * RS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x, n0 = blockIdx.y * CB;
    const bool track = blockIdx.y == 0;
    const int frow = lane & 15, kg = lane >> 4;
    const float* __restrict__ in = static_cast<const float*>(a.in) + (size_t)b * IN * IN * a.inLd;
    const unsigned char* __restrict__ wt = static_cast<const unsigned char*>(a.wt);
    const int wrow = min(n0 + frow, a.Npad - 1);
    const pf_half8 whf = *reinterpret_cast<const pf_half8*>(wt + (size_t)wrow * 128 + kg * 16);
    const pf_half8 wlf = *reinterpret_cast<const pf_half8*>(wt + (size_t)wrow * 128 + 64 + kg * 16);
    const int cch = 4 * kg;
    pf_f32x4 bv;
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = (n0 + cch + r < a.Npad) ? a.bias[n0 + cch + r] : 0.f;
    const int c = t & 15, y = (t >> 4) & 15, xh = t >> 8;
    const int n = n0 + c;
    const bool cok = n < a.N;
    float wk[K * K];
#pragma unroll
    for (int k = 0; k < K * K; ++k) wk[k] = cok ? a.dw_w2[(size_t)k * a.N + n] : 0.f;
    const float bd = cok ? a.dw_b[n] : 0.f;
    float rs = 0.f;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        const int oy0 = (q >> 1) * Q, ox0 = (q & 1) * Q;
        const int iy0 = oy0 * 2 - PAD, ix0 = ox0 * 2 - PAD;
        // ---- expand on the quadrant's input region ---------------------------------------------------------------
        for (int mt = wave; mt < MTILES; mt += 8) {
            const int p = mt * 16 + frow;
            const int ry = p / R, rx = p - ry * R;
            const int iy = iy0 + ry, ix = ix0 + rx;
            const bool ok = p < NPX && (unsigned)iy < (unsigned)IN && (unsigned)ix < (unsigned)IN;
            pf_f32x4 v0 = pf_f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (ok && kg * 8 < a.inC) {
                const float* px = in + ((size_t)iy * IN + ix) * a.inLd + kg * 8;
                v0 = *reinterpret_cast<const pf_f32x4*>(px);
                v1 = *reinterpret_cast<const pf_f32x4*>(px + 4);
            }
            pf_half8 xhf, xlf;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = e < 4 ? v0[e & 3] : v1[e & 3];
                const pf_half hv = (pf_half)v;
                xhf[e] = hv;
                xlf[e] = pf_split_lo(v, hv);
            }
            if (track) {                        // (wave-uniform) one channel tile per image reports the range of the shared input
#pragma unroll
                for (int e = 0; e < 8; ++e) amax = pf_amax(amax, e < 4 ? v0[e & 3] : v1[e & 3]);
            }
            pf_f32x4 acc = pf_f32x4{0.f, 0.f, 0.f, 0.f};
            acc = pf_mfma_16x16x32_f16(wlf, xhf, acc);
            acc = pf_mfma_16x16x32_f16(whf, xlf, acc);
            acc = pf_mfma_16x16x32_f16(whf, xhf, acc);
            pf_f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaf(acc[r], a.acc_scale, bv[r]);
            if constexpr (ACT >= 0) {
#pragma unroll
                for (int q_ = 0; q_ < 4; ++q_) v[q_] = pf_act_c<ACT>(v[q_]);
            } else pf_act_rh<4>(v, a.act);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (!ok || n0 + cch + r >= a.N) v[r] = 0.f;        // zero padding of the EXPANDED map / padding channels
            if (p < NPX) *reinterpret_cast<pf_f32x4*>(es + ry * RS + rx * CB + cch) = v;
        }
        __syncthreads();
        // ---- depthwise K x K / 2: thread = (channel, output row y, half row xh) ----------------------------------------
        float o[OX];
#pragma unroll
        for (int x = 0; x < OX; ++x) o[x] = bd;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const float* erow = es + (2 * y + ky) * RS + (2 * xh * OX) * CB + c;
            float iv[SPAN];
#pragma unroll
            for (int i = 0; i < SPAN; ++i) iv[i] = erow[i * CB];
#pragma unroll
            for (int kx = 0; kx < K; ++kx)
#pragma unroll
                for (int x = 0; x < OX; ++x) o[x] = fmaf(wk[ky * K + kx], iv[2 * x + kx], o[x]);
        }
        if constexpr (ACT >= 0) {
#pragma unroll
            for (int q_ = 0; q_ < OX; ++q_) o[q_] = pf_act_c<ACT>(o[q_]);
        } else pf_act_rh<OX>(o, a.act);
        if (cok) {
            float* out = static_cast<float*>(a.out) + ((size_t)b * OUT * OUT + (size_t)(oy0 + y) * OUT + ox0 + xh * OX) * a.outLd + n;
#pragma unroll
            for (int x = 0; x < OX; ++x) {
                out[(size_t)x * a.outLd] = o[x];
                rs += o[x];
            }
        }
        __syncthreads();                        // the next quadrant overwrites the region
    }
    if (track) pf_amax_commit(a.range_slot, amax, amax_seen);
    if (a.gap_out) {
        es[(t >> 4) * CB + c] = rs;             // 32 partial sums per channel
        __syncthreads();
        if (t < CB && n0 + t < a.N) {
            float tot = 0.f;
#pragma unroll
            for (int r = 0; r < 32; ++r) tot += es[r * CB + t];
            a.gap_out[(size_t)b * a.N + n0 + t] = tot / (float)(OUT * OUT);
        }
    }
}

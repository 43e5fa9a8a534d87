// Split-precision variant of the implicit-GEMM convolution (k_conv_gemm.h): f32 tensors in HBM, f16 matrix cores, f32-grade results.
//
// Every f32 operand is written as hi + lo with hi = f16(v), lo = f16(v - hi) (22 significand bits) and
// the product is accumulated as  wh*xh + wh*xl + wl*xh  on v_mfma_f32_16x16x32_f16 (f32 accumulate; the
// dropped wl*xl term is 2^-22 relative).  Three f16 MFMAs replace eight v_mfma_f32_16x16x4_f32 per 32 k,
// i.e. ~5x the matrix throughput of the exact-f32 path at the same accuracy (measured against float64:
// both 3.9e-7 of the output range on the hero layer's shape).  Weights are split at pack time and scaled
// by a per-layer power of two so that their lo parts stay clear of f16 subnormals (undone by acc_scale);
// activations are split while they are staged into LDS.
//
// K step = 32 elements: per row 64 B of hi + 64 B of lo in LDS (same chunk rotation as k_conv_gemm.h).
// Weight rows in HBM: [taps][Cpad/32][hi: 32 x f16 | lo: 32 x f16].
// STAGE = 0: the pixel operand is read from a.in.  STAGE = 1 (pointwise only): it is produced on the
// fly -- bilinear x2 upsample of up_lo / pass-through of up_skip, depthwise 3x3 (+bias) -- so the
// concatenated and the depthwise tensors never exist in HBM.
// EPI_K != 0 (pointwise only): the epilogue is the fused depthwise EPI_K x EPI_K conv (dilation EPI_DIL) of k_expdw.h.
// NK > 0 (plain pointwise convs only; host: Cpad == 32 NK): the K loop is unrolled completely and runs TWO steps ahead -- see the
// PW2 path in the body.
#pragma once
#include "k_conv_gemm.h"
#include "k_expdw.h"

// STAGE == 1 pixel producer (launch_sepup's fall-back instances): this thread's units of the K step that starts at channel kelem,
// bilinear x2 upsample of up_lo / pass-through of up_skip, then depthwise 3x3 (+bias)
template <int XUNITS>
__device__ __forceinline__ void conv_split_produce_updw(const ConvGemmArgs& a, int kelem, const int (&xb)[XUNITS], const int (&xiy0)[XUNITS],
                                                        const int (&xix0)[XUNITS], const bool (&xvalid)[XUNITS], pf_f32x4 (&xr)[XUNITS][2]) {
#pragma unroll
    for (int u = 0; u < XUNITS; ++u) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = 0.f;
        const int y = xiy0[u], x = xix0[u];           // output pixel (KS == 1: no stride / padding)
        const int H = 2 * a.loH, W = 2 * a.loW;
        if (xvalid[u] && kelem < a.inC) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = a.dw_b[kelem + e];
            if (kelem < a.C1) {
                // The bilinear taps of the whole 3x3 depthwise window live in the 3x3 low-res patch around
                // (y>>1, x>>1) (coordinates clamped), so upsample + depthwise collapse into ONE 3x3 filter
                // on the low-res map whose weights depend only on the position class of (y, x):
                // first / last / even / odd row  x  first / last / even / odd column  (16 classes,
                // precomputed at pack time: E = A_cls^T . Wdw . B_cls, zero padding included).
                const int my = y >> 1, mx = x >> 1;
                const int ycls = y == 0 ? 0 : (y == H - 1 ? 1 : 2 + (y & 1));
                const int xcls = x == 0 ? 0 : (x == W - 1 ? 1 : 2 + (x & 1));
                const float* we = a.dw_w + (size_t)((ycls * 4 + xcls) * 9) * a.C1 + kelem;
                const float* lo = a.up_lo + (size_t)xb[u] * a.loH * a.loW * a.loLd + kelem;
#pragma unroll 1
                for (int j = 0; j < 3; ++j) {   // one patch row at a time keeps the live loads (and VGPRs) bounded
                    const int ry = min(max(my - 1 + j, 0), a.loH - 1);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const int rx = min(max(mx - 1 + i, 0), a.loW - 1);
                        const float* pp = lo + ((size_t)ry * a.loW + rx) * a.loLd;
                        const float* ww = we + (size_t)(j * 3 + i) * a.C1;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const pf_f32x4 v4 = *reinterpret_cast<const pf_f32x4*>(pp + 4 * h);
                            const pf_f32x4 w4 = *reinterpret_cast<const pf_f32x4*>(ww + 4 * h);
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[4 * h + e] = fmaf(w4[e], v4[e], o[4 * h + e]);
                        }
                    }
                }
            } else {
                const int C2 = a.inC - a.C1;
                const float* wd = a.dw_w2 + (kelem - a.C1);
                const float* sk = a.up_skip + (size_t)xb[u] * H * W * a.skipLd + (kelem - a.C1);
#pragma unroll 1
                for (int k1 = 0; k1 < 3; ++k1) {
                    const int yy = y - 1 + k1;
                    if ((unsigned)yy >= (unsigned)H) continue;
#pragma unroll
                    for (int k2 = 0; k2 < 3; ++k2) {
                        const int xx = x - 1 + k2;
                        if ((unsigned)xx >= (unsigned)W) continue;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const pf_f32x4 v4 = *reinterpret_cast<const pf_f32x4*>(sk + ((size_t)yy * W + xx) * a.skipLd + 4 * h);
                            const pf_f32x4 w4 = *reinterpret_cast<const pf_f32x4*>(wd + (size_t)(k1 * 3 + k2) * C2 + 4 * h);
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[4 * h + e] = fmaf(w4[e], v4[e], o[4 * h + e]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) xr[u][e >> 2][e & 3] = o[e];
    }
}

template <int BM, int BN, int WARPS_M, int WARPS_N, int KS, int STAGE = 0, int EPI_K = 0, int EPI_DIL = 1, int EPI_W = 0, int NK = 0>
__global__ __launch_bounds__(WARPS_M * WARPS_N * 64, BN >= 256 ? WARPS_M * WARPS_N / 4 : WARPS_M * WARPS_N / 2) void conv_gemm_split_kernel(ConvGemmArgs a) {
    // second launch bound = waves per SIMD for two resident workgroups per CU (<= 128 VGPRs at 8 waves);
    // 256-channel tiles hold 64 accumulators + 64 weight-fragment registers and run one workgroup per CU;
    // the fused-depthwise variants keep an 80 KB tile in LDS (one workgroup per CU) and may use 256
    constexpr int NTHR = WARPS_M * WARPS_N * 64;       // 256 or 512 threads (8 waves hide the staging latency)
    constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
    constexpr int MT = WM / 16, NT = WN / 16;
    constexpr int XUNITS = (BM * 4 + NTHR - 1) / NTHR; // (row, 8-float unit) pairs staged per thread
    constexpr int XROWSTEP = NTHR / 4;                 // rows covered by one pass of the block
    constexpr int WCHUNKS = (BN * 8 + NTHR - 1) / NTHR;  // 16-byte weight chunks staged per thread
    constexpr int PLANE_X = BM * 64, PLANE_W = BN * 64;
    constexpr int W_BYTES = WCHUNKS * NTHR * 16;         // weight planes (hi | lo), rounded up to whole LDS-DMA passes
    constexpr int STAGE_BYTES = 2 * PLANE_X + W_BYTES;
    static_assert((NTHR == 256 || NTHR == 512) && WM % 16 == 0 && WN % 16 == 0 && WM > 0 && WN > 0, "tile shape");
    static_assert((BM * 4) % NTHR == 0, "pixel tile must split evenly over the block");

    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE_BYTES];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int wm = wave % WARPS_M, wn = wave / WARPS_M;
    int mtile = blockIdx.x;
    if (KS != 1 && (gridDim.x & 7) == 0) mtile = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int m0 = mtile * BM;
    const int n0 = blockIdx.y * BN;
    const int OHW = a.outH * a.outW;
    const int M = a.B * OHW;
    const float* __restrict__ in = static_cast<const float*>(a.in);
    const unsigned char* __restrict__ wt = static_cast<const unsigned char*>(a.wt);

    // pixel staging: unit u of this thread = row (t>>2) + XROWSTEP*u, floats [8*(t&3), 8*(t&3)+8) of the K step
    const int xc = t & 3;
    const int xrow0 = t >> 2;
    int xb[XUNITS], xiy0[XUNITS], xix0[XUNITS];
    bool xvalid[XUNITS];
#pragma unroll
    for (int u = 0; u < XUNITS; ++u) {
        const int m = m0 + xrow0 + XROWSTEP * u;
        xvalid[u] = m < M;
        const int mm = xvalid[u] ? m : 0;
        const int b = mm / OHW;
        const int rem = mm - b * OHW;
        const int oy = rem / a.outW;
        const int ox = rem - oy * a.outW;
        xb[u] = b;
        // plain pointwise (stride 1, no padding): the input pixel IS output pixel m
        xiy0[u] = (KS == 1 && STAGE == 0) ? mm : (KS == 1 ? oy : oy * a.stride - a.pad);
        xix0[u] = (KS == 1 && STAGE == 0) ? 0 : (KS == 1 ? ox : ox * a.stride - a.pad);
    }
    const int taps = KS == 1 ? 1 : a.KH * a.KW;
    const int cblocks = a.Cpad / 32;
    const int nk = taps * cblocks;
    const size_t wrow_bytes = (size_t)taps * cblocks * 128;

    constexpr bool PW2 = KS == 1 && STAGE == 0;                       // plain pointwise conv: leaner operand staging (below)
    constexpr bool GATED = PW2 && EPI_K == 0;                         // ... which may carry an SE gate on its input channels
    static_assert(NK == 0 || (KS == 1 && STAGE == 0), "unrolled K loop: plain pointwise convs");
    pf_f32x4 xreg[NK > 1 ? 2 : 1][XUNITS][2];
    // The gate vector of the tile's face sits in LDS when the tile lies inside one face (every gated layer of the Student at
    // 256 x 256); otherwise each unit fetches its gate values when it is split (correct, no look-ahead: small crops only).
    // Multiplying right behind the pixel load put an s_waitcnt vmcnt(0) behind each of a K step's loads.
    // It gets its own 4 KB where two workgroups still fit a CU with it, else the tail of weight stage 0 that no row uses (W_BYTES
    // is rounded up to whole 512-slot DMA passes; load_w skips the slots beyond row BN - 1).
    constexpr int W_USED = BN * 128;
    constexpr bool GATE_SEP = 2 * STAGE_BYTES + 4096 <= 80 * 1024;
    constexpr int GATE_CAP = !GATED ? 0 : (GATE_SEP ? 1024 : (W_BYTES - W_USED) / 4);
    __shared__ __attribute__((aligned(16))) float sgate_sep[GATED && GATE_SEP ? 1024 : 4];
    float* sgate = GATE_SEP ? sgate_sep : reinterpret_cast<float*>(smem + 2 * PLANE_X + W_USED);
    const bool gate_lds = GATED && a.gate != nullptr && (OHW % BM) == 0 && a.Cpad <= GATE_CAP;
    unsigned amax = 0;                                 // range guard (pf_common.h)
    const unsigned amax_seen = pf_amax_seen(a.range_slot);

    // Weights are pre-split bytes: they go global -> LDS directly (no VGPRs, no ds_write pass, which costs 13
    // LDS-path cycles per 16 bytes against 4 for a read).  LDS slot s (16 B, lane-linear as the DMA requires) is
    // (plane, row, position) with the row's four chunks rotated; the rotation is applied to the SOURCE address.
    // Rows past Npad re-read the last row (their outputs are never stored); slots past the planes land in padding.
    auto load_w = [&](int tap, int cb, int stage) {
        unsigned char* wdst = smem + stage * STAGE_BYTES + 2 * PLANE_X;
#pragma unroll
        for (int c = 0; c < WCHUNKS; ++c) {
            const int sl = t + NTHR * c;
            const int plane = sl >= BN * 4 ? 1 : 0;
            const int r = (sl - plane * BN * 4) >> 2;
            const int row = r < BN ? r : BN - 1;
            const int chunk = ((sl & 3) - 2 * (row >> 2)) & 3;
            const int n = min(n0 + row, a.Npad - 1);
            const unsigned char* src = wt + (size_t)n * wrow_bytes + ((size_t)tap * cblocks + cb) * 128 + plane * 64 + chunk * 16;
            if constexpr (PW2) { if (sl < BN * 8) pf_glds16(src, wdst + sl * 16); } else pf_glds16(src, wdst + sl * 16);   // (the tail may hold the gate)
        }
    };
    auto load_tile = [&](int tap, int cb, int stage) {
        const int ky = KS == 1 ? 0 : tap / a.KW;
        const int kx = KS == 1 ? 0 : tap - ky * a.KW;
        const int kelem = cb * 32 + xc * 8;
        if constexpr (STAGE == 1) {
            conv_split_produce_updw<XUNITS>(a, kelem, xb, xiy0, xix0, xvalid, xreg[0]);
        } else {
#pragma unroll
        for (int u = 0; u < XUNITS; ++u) {
            const int iy = KS == 1 ? xiy0[u] : xiy0[u] + ky * a.dil;
            const int ix = KS == 1 ? xix0[u] : xix0[u] + kx * a.dil;
            const bool pok = xvalid[u] && (KS == 1 || ((unsigned)iy < (unsigned)a.inH && (unsigned)ix < (unsigned)a.inW));
            const size_t off = KS == 1 ? (size_t)iy * a.inLd + kelem : ((size_t)(xb[u] * a.inH + iy) * a.inW + ix) * a.inLd + kelem;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                pf_f32x4 v = pf_f32x4{0.f, 0.f, 0.f, 0.f};
                if (pok && kelem + 4 * h < a.inC) {
                    v = *reinterpret_cast<const pf_f32x4*>(in + off + 4 * h);
                    if (a.gate) {
                        const float* g = a.gate + (size_t)xb[u] * a.inC + kelem + 4 * h;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] *= g[e];
                    }
                }
                xreg[0][u][h] = v;
            }
        }
        }
        load_w(tap, cb, stage);
    };
    // plain pointwise path: this thread's pixel units of K step cb, requested and nothing else (out-of-range units read element 0
    // and are zeroed when they are split; the SE gate is applied there too: multiplying on the spot put an s_waitcnt vmcnt(0)
    // behind each of a K step's loads)
    auto load_x = [&](int cb, pf_f32x4 (&xr)[XUNITS][2]) {
        const int kelem = cb * 32 + xc * 8;
#pragma unroll
        for (int u = 0; u < XUNITS; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bool ok = xvalid[u] && kelem + 4 * h < a.inC;
                xr[u][h] = *reinterpret_cast<const pf_f32x4*>(in + (ok ? (size_t)xiy0[u] * a.inLd + kelem + 4 * h : (size_t)0));
            }
    };
    auto store_tile = [&](int stage, int cb, const pf_f32x4 (&xr)[XUNITS][2]) {
        unsigned char* xh = smem + stage * STAGE_BYTES;
        unsigned char* xl = xh + PLANE_X;
#pragma unroll
        for (int u = 0; u < XUNITS; ++u) {
            pf_f32x4 xv[2] = {xr[u][0], xr[u][1]};
            if constexpr (GATED) {
                // the gate is applied INSIDE each branch: a value loaded in the fall-back branch and used behind the join would make
                // the compiler wait for vmcnt(0) on every path, i.e. for the look-ahead loads too
                const int kelem = cb * 32 + xc * 8;
                if (gate_lds) {
                    xv[0] *= *reinterpret_cast<const pf_f32x4*>(sgate + kelem);
                    xv[1] *= *reinterpret_cast<const pf_f32x4*>(sgate + kelem + 4);
                } else if (a.gate) {
                    const float* g = a.gate + (size_t)xb[u] * a.inC + kelem;
                    if (xvalid[u] && kelem < a.inC) xv[0] *= *reinterpret_cast<const pf_f32x4*>(g);
                    if (xvalid[u] && kelem + 4 < a.inC) xv[1] *= *reinterpret_cast<const pf_f32x4*>(g + 4);
                }
            }
            pf_half8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = xv[e >> 2][e & 3];
                if constexpr (PW2) { if (!(xvalid[u] && cb * 32 + xc * 8 + (e & 4) < a.inC)) v = 0.f; }
                const pf_half hv = (pf_half)v;
                hi[e] = hv;
                lo[e] = pf_split_lo(v, hv);
                amax = pf_amax(amax, v);
            }
            const int off = pf_lds_chunk_off(xrow0 + XROWSTEP * u, xc);
            *reinterpret_cast<pf_half8*>(xh + off) = hi;
            *reinterpret_cast<pf_half8*>(xl + off) = lo;
        }
    };

    pf_f32x4 acc[NT][MT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[j][i] = pf_f32x4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fchunk = lane >> 4;
    auto mma_stage = [&](int cur) {
        const unsigned char* xh = smem + cur * STAGE_BYTES;
        const unsigned char* xl = xh + PLANE_X;
        const unsigned char* wh = xl + PLANE_X;
        const unsigned char* wl = wh + PLANE_W;
        if constexpr (MT == 2 && NT >= 4) {
            // wide-N tiles: the two pixel fragments stay live and the weight fragments come one 16-channel tile at a time -- 24
            // fragment registers instead of 8 NT + 8 (same products in the same order per accumulator)
            if (!(pf_dbg(a) & PF_ABL_NO_MFMA)) {
                pf_half8 xhf[MT], xlf[MT];
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const int off = pf_lds_chunk_off(wm * WM + i * 16 + frow, fchunk);
                    xhf[i] = *reinterpret_cast<const pf_half8*>(xh + off);
                    xlf[i] = *reinterpret_cast<const pf_half8*>(xl + off);
                }
                // weight fragments of tile j + 1 are requested in front of tile j's MFMAs and no further ahead (the compiler fence):
                // left alone, the scheduler of the unrolled instances hoists every tile's reads and spills
                pf_half8 wq[2][2];
                {
                    const int off = pf_lds_chunk_off(wn * WN + frow, fchunk);
                    wq[0][0] = *reinterpret_cast<const pf_half8*>(wh + off);
                    wq[0][1] = *reinterpret_cast<const pf_half8*>(wl + off);
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    if (j + 1 < NT) {
                        const int off = pf_lds_chunk_off(wn * WN + (j + 1) * 16 + frow, fchunk);
                        wq[(j + 1) & 1][0] = *reinterpret_cast<const pf_half8*>(wh + off);
                        wq[(j + 1) & 1][1] = *reinterpret_cast<const pf_half8*>(wl + off);
                    }
                    const pf_half8 whj = wq[j & 1][0], wlj = wq[j & 1][1];
#pragma unroll
                    for (int i = 0; i < MT; ++i) acc[j][i] = pf_mfma_16x16x32_f16(wlj, xhf[i], acc[j][i]);
#pragma unroll
                    for (int i = 0; i < MT; ++i) acc[j][i] = pf_mfma_16x16x32_f16(whj, xlf[i], acc[j][i]);
#pragma unroll
                    for (int i = 0; i < MT; ++i) acc[j][i] = pf_mfma_16x16x32_f16(whj, xhf[i], acc[j][i]);
                    asm volatile("" ::: "memory");
                }
            }
        } else {
        pf_half8 whf[NT], wlf[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int off = pf_lds_chunk_off(wn * WN + j * 16 + frow, fchunk);
            whf[j] = *reinterpret_cast<const pf_half8*>(wh + off);
            wlf[j] = *reinterpret_cast<const pf_half8*>(wl + off);
        }
        if (!(pf_dbg(a) & PF_ABL_NO_MFMA))
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int off = pf_lds_chunk_off(wm * WM + i * 16 + frow, fchunk);
            const pf_half8 xhf = *reinterpret_cast<const pf_half8*>(xh + off);
            const pf_half8 xlf = *reinterpret_cast<const pf_half8*>(xl + off);
            // small terms first, the dominant hi*hi term last
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j][i] = pf_mfma_16x16x32_f16(wlf[j], xhf, acc[j][i]);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j][i] = pf_mfma_16x16x32_f16(whf[j], xlf, acc[j][i]);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j][i] = pf_mfma_16x16x32_f16(whf[j], xhf, acc[j][i]);
        }
        }
    };
    if constexpr (PW2) {
        // Plain pointwise convs.  Same schedule as the general loop below (operands of step kt + 1 requested before step kt's MFMAs);
        // the pixel loads are unconditional (masked when split) and the SE gate comes from LDS, so nothing waits between a step's
        // requests.  Two steps of look-ahead were tried this round (second register set): asm-issued loads are unsafe -- the
        // register allocator copies / reuses destination registers of loads it cannot see -- and compiler-visible ones get an
        // s_waitcnt vmcnt(0) at the loop head because the in-flight set is loop-carried.
        load_w(0, 0, 0);
        load_x(0, xreg[0]);
        if constexpr (GATED) {
            if (gate_lds) {                                         // behind the first operand requests: its round trip overlaps theirs
                const float* g = a.gate + (size_t)(m0 / OHW) * a.inC;
                for (int i = t; i < a.Cpad; i += NTHR) sgate[i] = i < a.inC ? g[i] : 0.f;
                __syncthreads();
            }
        }
        if constexpr (NK > 0) {
            // One base pointer per pixel unit / weight slot for ALL steps, the step in the instruction's immediate offset: computed per
            // step, the unrolled loop's 30 x 5 addresses are hoisted to its head and spill.  Rows / channels outside the tensor read
            // inside it or at most 124 bytes behind it (the arena carries that slack) and are zeroed when they are split.
            const float* xbase[XUNITS];
#pragma unroll
            for (int u = 0; u < XUNITS; ++u) xbase[u] = in + (xvalid[u] ? (size_t)xiy0[u] * a.inLd : (size_t)0) + xc * 8;
            const unsigned char* wsrc[WCHUNKS];
#pragma unroll
            for (int c = 0; c < WCHUNKS; ++c) {
                const int sl = t + NTHR * c;
                const int plane = sl >= BN * 4 ? 1 : 0;
                const int r = (sl - plane * BN * 4) >> 2;
                const int row = r < BN ? r : BN - 1;
                const int chunk = ((sl & 3) - 2 * (row >> 2)) & 3;
                wsrc[c] = wt + (size_t)min(n0 + row, a.Npad - 1) * wrow_bytes + plane * 64 + chunk * 16;
            }
            auto load_x_at = [&](auto cb_tag, pf_f32x4 (&xr)[XUNITS][2]) {
                constexpr int cb = decltype(cb_tag)::value;
#pragma unroll
                for (int u = 0; u < XUNITS; ++u) {
                    xr[u][0] = *reinterpret_cast<const pf_f32x4*>(xbase[u] + cb * 32);
                    xr[u][1] = *reinterpret_cast<const pf_f32x4*>(xbase[u] + cb * 32 + 4);
                }
            };
            auto load_w_at = [&](auto cb_tag, int stage) {
                constexpr int cb = decltype(cb_tag)::value;
                unsigned char* wdst = smem + stage * STAGE_BYTES + 2 * PLANE_X;
#pragma unroll
                for (int c = 0; c < WCHUNKS; ++c)
                    if (t + NTHR * c < BN * 8) pf_glds16_raw_off<cb * 128>(wsrc[c], wdst + (t + NTHR * c) * 16);
            };
            // Unrolled: the pixel operands of steps kt + 1 AND kt + 2 are in flight (two register sets, no loop-carried value, so the
            // compiler's own vmcnt counting is exact) while step kt's MFMAs run; the weights of step kt + 1 by asm-issued LDS-DMA,
            // requested BEFORE the newest pixels: vmcnt retires in order, so "all but the 2 XUNITS youngest" at the barrier = the
            // weights of the next step have landed, the newest pixels have not.  With one step of look-ahead and __syncthreads()
            // (which drains vmcnt) a K step of conv1x1 960 -> 160 was 8.3 k cycles against 1.9 k of MFMA issue.
            if constexpr (NK > 1) load_x_at(std::integral_constant<int, 1>{}, xreg[1]);
            store_tile(0, 0, xreg[0]);
            if constexpr (NK > 1) pf_wait_vm_barrier<2 * XUNITS>(); else pf_wait_vm_barrier<0>();
            pf_sched_fence();
            pf_static_for<NK>([&](auto kt_tag) {
                constexpr int kt = decltype(kt_tag)::value;
                constexpr int cur = kt & 1;
                if constexpr (kt + 1 < NK) { if (!(pf_dbg(a) & PF_ABL_OPERANDS_FIRST_K)) load_w_at(std::integral_constant<int, kt + 1>{}, cur ^ 1); }
                if constexpr (kt + 2 < NK) { if (!(pf_dbg(a) & PF_ABL_OPERANDS_FIRST_K)) load_x_at(std::integral_constant<int, kt + 2>{}, xreg[cur]); }
                mma_stage(cur);
                if constexpr (kt + 1 < NK) { if (!(pf_dbg(a) & PF_ABL_NO_SPLIT_STORE)) store_tile(cur ^ 1, kt + 1, xreg[cur ^ 1]); }
                pf_pin(amax);       // the range guard's running maximum is due NOW: left alone, the compiler keeps every step's eight
                                    // values (in scratch) and folds them at the end of the unrolled loop
                if constexpr (kt + 2 < NK) pf_wait_vm_barrier<2 * XUNITS>(); else pf_wait_vm_barrier<0>();
                pf_sched_fence();
            });
        } else {
        store_tile(0, 0, xreg[0]);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            const bool more = kt + 1 < nk;
            if (more && !(pf_dbg(a) & PF_ABL_OPERANDS_FIRST_K)) { load_x(kt + 1, xreg[0]); load_w(0, kt + 1, cur ^ 1); }
            mma_stage(cur);
            if (more && !(pf_dbg(a) & PF_ABL_NO_SPLIT_STORE)) store_tile(cur ^ 1, kt + 1, xreg[0]);
            __syncthreads();
        }
        }
    } else {
    int tap = 0, cb = 0;
    load_tile(tap, cb, 0);
    store_tile(0, 0, xreg[0]);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) {
            if (++tap == taps) { tap = 0; ++cb; }
            if (!(pf_dbg(a) & PF_ABL_OPERANDS_FIRST_K)) load_tile(tap, cb, cur ^ 1);
        }
        mma_stage(cur);
        if (more && !(pf_dbg(a) & PF_ABL_NO_SPLIT_STORE)) store_tile(cur ^ 1, cb, xreg[0]);
        __syncthreads();
    }
    }
    pf_amax_commit(a.range_slot, amax, amax_seen);
    if constexpr (EPI_K < 0) {
        conv_gemm_argmax_epilogue<BM, BN, WARPS_M, WARPS_N>(a, acc, m0, n0, wm, wn, lane, OHW, a.acc_scale);
    } else if constexpr (EPI_K != 0) {
        static_assert(KS == 1 && STAGE == 0, "fused depthwise epilogue: pointwise expand only");
        static_assert(2 * STAGE_BYTES >= (BM * (BN + 4) + (NTHR / BN) * 4 * BN) * 4, "E tile must fit the staging LDS");
        expdw_epilogue<BM, BN, WARPS_M, WARPS_N, EPI_K, EPI_DIL, EPI_W>(a, acc, smem, m0, n0, wm, wn, t, M);   // loop ended on a barrier
    } else {
        conv_gemm_epilogue<float, BM, BN, WARPS_M, WARPS_N>(a, acc, m0, n0, wm, wn, lane, M, OHW, a.acc_scale);
    }
}

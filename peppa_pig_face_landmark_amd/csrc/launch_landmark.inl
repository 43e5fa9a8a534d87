// Launchers of the landmark networks' encoder / decoder ops: dense conv (k_conv_gemm.h, k_conv_split.h, k_halo.h, k_hero.h, k_pwhead.h), the fused decoder front end
// (k_sepup.h, k_sepup_patch.h), the inverted-residual blocks (k_mbconv.h, k_mbx.h, k_expdw.h) and the Student's fused front (k_front2.h).
// Included by engine.cpp only.
// Dense conv: launch_conv (below its parts) builds the arguments, picks the tile configuration and tries the kernel families in a fixed
// order; a family function returns -1 when the conv is not its own.  Tile configurations: index -> (BM pixels, BN channels)
static const int kConvBM[PF_CONV_NCFG] = {128, 128, 256, 256, 128, 128, 128, 256, 128};
static const int kConvBN[PF_CONV_NCFG] = {128, 64, 32, 16, 80, 96, 112, 48, 160};

static ConvGemmArgs conv_args(const pf_handle* h, const Program& p, const PfConvOp& o, int B, unsigned* range_slot) {
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    ConvGemmArgs a{};
    a.in = p.tensor_ptr(o.in_t); a.out = p.tensor_ptr(o.out_t);
    a.wt = p.cptr(o.wt); a.bias = (const float*)p.cptr(o.bias);
    a.res = p.opt_tensor(o.res_t); a.resLd = p.opt_ld(o.res_t);
    a.gate = (const float*)p.opt_buf(o.gate_buf); a.fbias = (const float*)p.opt_buf(o.fbias_buf);
    a.amax_val = (float*)p.opt_buf(o.amax_val_buf); a.amax_idx = (int*)p.opt_buf(o.amax_idx_buf);
    a.B = B; a.inH = ti.H; a.inW = ti.W; a.inC = ti.C; a.inLd = ti.ld;
    a.outH = to.H; a.outW = to.W; a.N = o.N; a.Npad = o.Npad; a.outLd = to.ld; a.outCs = o.outCs;
    a.outCpad = o.outCs == 1 ? to.C : o.N;
    a.KH = o.KH; a.KW = o.KW; a.stride = o.stride; a.pad = o.pad; a.dil = o.dil; a.Cpad = o.Cpad;
    a.act = o.act; a.amaxN = o.amaxN; a.store_out = o.store_out; a.acc_scale = o.acc_scale;
    a.dbg = h->dbg; a.range_slot = range_slot;
    a.gap_parts = (float*)p.opt_buf(o.gap_parts_plus1 - 1);
    return a;
}

static inline bool conv_is_pointwise(const ConvGemmArgs& a) { return a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0; }

// The packer's configuration, or: the channel tile is chosen so that q tiles of NT*16 channels cover Npad with the least
// padding (NT <= 8), ties -> fewer tiles.
static int pick_conv_cfg(const PfConvOp& o, const ConvGemmArgs& a, bool split) {
    static const int cfg_of_nt[9] = {-1, 3, 2, 7, 1, 4, 5, 6, 0};
    if (o.cfg >= 0) return o.cfg;
    const int t16 = a.Npad / 16;
    int best_nt = 0, best_cost = 1 << 30;
    for (int q = (t16 + 7) / 8; q <= (t16 + 7) / 8 + 3; ++q) {
        const int nt = (t16 + q - 1) / q;
        if (nt < 1 || nt > 8) continue;
        if (q * nt < best_cost) { best_cost = q * nt; best_nt = nt; }
    }
    // 160 output channels (stage-5 projections, K = 672 / 960): one 128 x 160 tile reads the wide input once
    // instead of twice (two 80-channel tiles); split-precision pointwise only
    if (split && o.use_split != 0 && a.Npad == 160 && conv_is_pointwise(a) && !a.amax_val) return 8;
    return cfg_of_nt[best_nt];
}

// 3x3 / stride 1 / pad 1 with 128 outputs on 16-, 32- or 64-pixel-wide maps: input patch resident in LDS
// (the Student's hero conv; HRNet's 18 / 36 / 72-channel 3x3 stacks of the Teacher take the narrow variants)
template <bool SPLIT>
static int launch_conv3x3_resident(pf_handle* h, const PfConvOp& o, const ConvGemmArgs& a, int M) {
    if constexpr (SPLIT) {
        if (o.use_split != 0 && a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.dil == 1 && !a.gate && !a.amax_val &&
            (a.outW == 16 || a.outW == 32 || a.outW == 64) && ((a.outH * a.outW) % 128) == 0 && a.inH == a.outH && a.inW == a.outW &&
            (a.Npad == 128 || (a.Npad == 64 && a.outW == 64) || a.Npad == 32 || a.Npad == 48 || a.Npad == 80)) {
            dim3 grid(pf_div_up(M, 128), 1);
            const bool big = ((a.outH * a.outW) % 256) == 0 && !(host_dbg(h) & PF_SEL_HALO_TILES_128);     // narrow variants: 256-pixel tiles
            if (big && a.Npad <= 64) grid = dim3(pf_div_up(M, 256), 1);
            // k_hero.h loads all 128 channels of every pixel as 16-byte vectors, unmasked: a 3x3 conv whose inC < Cpad == 128 would feed
            // neighbouring bytes to the MFMAs and the range guard -- such a layer takes the masked halo kernel below
            const bool hero = a.Npad == 128 && a.Cpad == 128 && a.inC == 128 && (a.inLd & 3) == 0 && a.outW == 64;
            if (a.gap_parts) {          // + per-tile channel sums of the output (the face-attribute head's decx4 pool; ir.py conv(gap_parts=True))
                if (hero && o.use_split == 2) PF_LAUNCH((conv3x3_hero_kernel<4, true, true, true>), grid, dim3(512), h->stream, a);
                else if (hero) PF_LAUNCH((conv3x3_hero_kernel<4, true, false, true>), grid, dim3(512), h->stream, a);
                else if (a.Npad == 128) PF_LAUNCH((conv3x3_halo_split_kernel<128, 4, 2, 128, true>), grid, dim3(512), h->stream, a);
                else PF_FAIL(h, "conv: per-tile channel sums need 128 output channels (Npad %d)", a.Npad);
                return 0;
            }
            if (hero && (host_dbg(h) & PF_SEL_HERO_AB)) PF_LAUNCH((conv3x3_hero_kernel<4, false>), grid, dim3(512), h->stream, a);   // A/B aid (ablation build)
            else if (hero && o.use_split == 2) PF_LAUNCH((conv3x3_hero_kernel<4, true, true>), grid, dim3(512), h->stream, a);   // ONE f16 product (opt-in per conv)
            else if (hero && !(host_dbg(h) & PF_SEL_HERO_TO_HALO)) PF_LAUNCH((conv3x3_hero_kernel<4>), grid, dim3(512), h->stream, a);   // k_hero.h
            else if (a.Npad == 128) PF_LAUNCH((conv3x3_halo_split_kernel<128, 4, 2>), grid, dim3(512), h->stream, a);
            else if (a.Npad == 64 && big) PF_LAUNCH((conv3x3_halo_split_kernel<64, 4, 2, 256>), grid, dim3(512), h->stream, a);   // HRNet layer1's 64 -> 64
            else if (a.Npad == 64) PF_LAUNCH((conv3x3_halo_split_kernel<64, 4, 2>), grid, dim3(512), h->stream, a);
            else if (a.Npad == 80) PF_LAUNCH((conv3x3_halo_split_kernel<80, 8, 1>), grid, dim3(512), h->stream, a);
            else if (a.Npad == 48 && big) PF_LAUNCH((conv3x3_halo_split_kernel<48, 8, 1, 256>), grid, dim3(512), h->stream, a);
            else if (a.Npad == 48) PF_LAUNCH((conv3x3_halo_split_kernel<48, 8, 1>), grid, dim3(512), h->stream, a);
            else if (big) PF_LAUNCH((conv3x3_halo_split_kernel<32, 8, 1, 256>), grid, dim3(512), h->stream, a);
            else PF_LAUNCH((conv3x3_halo_split_kernel<32, 8, 1>), grid, dim3(512), h->stream, a);
            return 0;
        }
    }
    return -1;
}

// Work items of pw_head_kernel per face: a run of tiles of one face; a face is split only while there are fewer faces than CUs
static int pick_head_segs(const pf_handle* h, int B, int tpf) {
#ifdef PF_SIMT_EMULATION
    const int fill = 8;                 // CPU test build: a few faces must still exercise items of SEVERAL tiles and several items per face
#else
    const int fill = h->num_cus;
#endif
    int segs = 1;
    while (segs < tpf && (tpf % (2 * segs)) == 0 && B * segs < fill) segs *= 2;
    if (B * segs > fill) {              // more items than CUs: pick the split whose LAST round of the persistent grid is full
        double best = 1e30;
        for (int sg = 1; sg <= 8 && sg <= tpf && (tpf % sg) == 0; sg *= 2) {
            const double face_times = last_round_cost(B, sg, fill);
            if (face_times < best - 1e-9) { best = face_times; segs = sg; }
        }
    }
    return segs;
}

// heat-map score head: bias-only arg-max epilogue (nothing stored, tiles never straddle a face)
template <bool SPLIT>
static int launch_conv_score_head(pf_handle* h, const PfConvOp& o, ConvGemmArgs& a, int cfg, int M, dim3 grid) {
    if constexpr (SPLIT) {
        if (o.use_split != 0 && conv_is_pointwise(a) && cfg == 0 && a.amax_val && !a.store_out && !a.res && !a.fbias && !a.gate && a.act == PF_ACT_NONE &&
            (M % 128) == 0) {
            // 128 input channels (the Student's and the Teacher's head): the weight-stationary stream of k_pwhead.h
            if (a.Cpad == 128 && a.inC == 128 && a.Npad <= 112 && ((a.outH * a.outW) % 128) == 0 && !(host_dbg(h) & PF_SEL_NO_PW_HEAD)) {
                a.head_segs = pick_head_segs(h, a.B, (a.outH * a.outW) / 128);
                if (o.use_split == 2) PF_LAUNCH((pw_head_kernel<4, true>), dim3(persistent_grid(a.B * a.head_segs, 1)), dim3(512), h->stream, a);   // ONE f16 product (opt-in per conv)
                else PF_LAUNCH((pw_head_kernel<4>), dim3(persistent_grid(a.B * a.head_segs, 1)), dim3(512), h->stream, a);
            } else if (a.Cpad == 128) PF_LAUNCH((conv_gemm_split_kernel<128, 128, 4, 2, 1, 0, -1, 1, 0, 4>), grid, dim3(512), h->stream, a);   // K loop unrolled, two steps ahead
            else PF_LAUNCH((conv_gemm_split_kernel<128, 128, 4, 2, 1, 0, -1>), grid, dim3(512), h->stream, a);
            return 0;
        }
    }
    return -1;
}

// everything else: the unrolled-K pointwise instances, configuration 8, the generic (configuration x precision x 1x1 / 3x3) table
template <typename T, bool SPLIT>
static int launch_conv_table(pf_handle* h, const PfConvOp& o, const ConvGemmArgs& a, int cfg, dim3 grid) {
    const bool pointwise = conv_is_pointwise(a);
    const bool use_split = o.use_split != 0;   // per-conv choice made by the packer (weights are laid out accordingly)
    // plain pointwise convs whose K depth has an unrolled instance (two K steps of look-ahead, k_conv_split.h): the Student's
    // stage-3 to stage-5 projections at 256 x 256 and a few neighbours; every other depth takes the rolled loop of the same kernel
    if constexpr (SPLIT) {
        if (use_split && pointwise && !a.amax_val) {
            const int nk = a.Cpad / 32;
#define PF_PW_NK(CFG, BM_, BN_, WM_, WN_, NK_)                                                                        \
            if (cfg == CFG && nk == NK_) {                                                                            \
                PF_LAUNCH((conv_gemm_split_kernel<BM_, BN_, WM_, WN_, 1, 0, 0, 1, 0, NK_>), grid, dim3(512), h->stream, a); \
                return 0;                                                                                             \
            }
            // measured (profiles/r04_run25 vs run23): 960 -> 160 0.204 -> 0.175 ms per 256 faces, 480 -> 112 -10 %; the shallow ones
            // (K <= 224, and the expand + depthwise launches) did not move and keep the rolled loop
            PF_PW_NK(8, 128, 160, 4, 2, 30) PF_PW_NK(8, 128, 160, 4, 2, 21)
            PF_PW_NK(6, 128, 112, 8, 1, 21) PF_PW_NK(6, 128, 112, 8, 1, 15)
#undef PF_PW_NK
        }
    }
    if (cfg == 8) {
        if constexpr (SPLIT) {
            PF_LAUNCH((conv_gemm_split_kernel<128, 160, 4, 2, 1>), grid, dim3(512), h->stream, a);
            return 0;
        } else {
            PF_FAIL(h, "conv tile configuration 8 is split-precision only");
        }
    }
#define PF_CONV_CASE(idx, BM_, BN_, WM_, WN_)                                                              \
    case idx:                                                                                           \
        if (SPLIT && use_split) {   /* 8 waves per workgroup: twice the M-waves of the direct kernel */ \
            if (pointwise) PF_LAUNCH((conv_gemm_split_kernel<BM_, BN_, 2 * WM_, WN_, 1>), grid, dim3(512), h->stream, a); \
            else PF_LAUNCH((conv_gemm_split_kernel<BM_, BN_, 2 * WM_, WN_, 3>), grid, dim3(512), h->stream, a);          \
        } else {                                                                                        \
            if (pointwise) PF_LAUNCH((conv_gemm_kernel<T, BM_, BN_, WM_, WN_, 1>), grid, dim3(256), h->stream, a); \
            else PF_LAUNCH((conv_gemm_kernel<T, BM_, BN_, WM_, WN_, 3>), grid, dim3(256), h->stream, a);          \
        }                                                                                               \
        break;
    switch (cfg) {
        PF_CONV_CASE(0, 128, 128, 2, 2)
        PF_CONV_CASE(1, 128, 64, 2, 2)
        PF_CONV_CASE(2, 256, 32, 4, 1)
        PF_CONV_CASE(3, 256, 16, 4, 1)
        PF_CONV_CASE(4, 128, 80, 4, 1)
        PF_CONV_CASE(5, 128, 96, 4, 1)
        PF_CONV_CASE(6, 128, 112, 4, 1)
        default:
            PF_CONV_CASE(7, 256, 48, 4, 1)
    }
#undef PF_CONV_CASE
    return 0;
}

template <typename T, bool SPLIT>
static int launch_conv(pf_handle* h, const Program& p, const PfConvOp& o, int B, unsigned* range_slot) {
    ConvGemmArgs a = conv_args(h, p, o, B, range_slot);
    const int cfg = pick_conv_cfg(o, a, SPLIT);
    const int M = B * a.outH * a.outW;
    if (a.amax_val && ((a.outH * a.outW) % kConvBM[cfg]) != 0) PF_FAIL(h, "argmax conv: H*W=%d not a multiple of BM=%d", a.outH * a.outW, kConvBM[cfg]);
    const dim3 grid(pf_div_up(M, kConvBM[cfg]), pf_div_up(a.Npad, kConvBN[cfg]));
    ProfScope ps(h, "conv%dx%d%s_c%d_n%d_%dx%d", a.KH, a.KW, a.amax_val ? "_argmax" : "", a.inC, a.N, a.outH, a.outW);
    if (const int rc = launch_conv3x3_resident<SPLIT>(h, o, a, M); rc >= 0) return rc;
    if (a.gap_parts) PF_FAIL(h, "conv: per-tile channel sums are produced by the split-precision 3x3 kernels with 128 outputs only");
    if (const int rc = launch_conv_score_head<SPLIT>(h, o, a, cfg, M, grid); rc >= 0) return rc;
    return launch_conv_table<T, SPLIT>(h, o, a, cfg, grid);
}

static int launch_sepup(pf_handle* h, const Program& p, const PfSepupOp& o, int B, unsigned* range_slot) {
    const PfTensorRec& tl = p.tens[o.lo_t];
    const PfTensorRec& tk = p.tens[o.skip_t];
    const PfTensorRec& to = p.tens[o.out_t];
    ConvGemmArgs a{};
    a.up_lo = (const float*)p.tensor_ptr(o.lo_t); a.up_skip = (const float*)p.tensor_ptr(o.skip_t);
    a.out = p.tensor_ptr(o.out_t);
    a.dw_w = (const float*)p.cptr(o.dw_e); a.dw_b = (const float*)p.cptr(o.dw_b); a.dw_w2 = (const float*)p.cptr(o.dw_skip);
    a.wt = p.cptr(o.pw_wt); a.bias = (const float*)p.cptr(o.pw_bias);
    a.Cpad = o.Cpad; a.Npad = o.Npad; a.N = o.N; a.act = o.act; a.acc_scale = o.acc_scale;
    a.loH = tl.H; a.loW = tl.W; a.C1 = tl.C; a.loLd = tl.ld; a.skipLd = tk.ld;
    a.B = B; a.inH = to.H; a.inW = to.W; a.inC = tl.C + tk.C; a.inLd = 0;
    a.outH = to.H; a.outW = to.W; a.outLd = to.ld; a.outCs = 1; a.outCpad = to.C;
    a.KH = a.KW = 1; a.stride = 1; a.pad = 0; a.dil = 1; a.store_out = 1;
    a.dbg = h->dbg;
    a.range_slot = range_slot;
    if (to.H != 2 * tl.H || to.W != 2 * tl.W || tk.H != to.H || tk.W != to.W || (tl.C % 32) != 0 || to.H < 6 || to.W < 6)
        PF_FAIL(h, "sepup: inconsistent tensor shapes");
    dim3 grid(pf_div_up(B * to.H * to.W, 128), pf_div_up(a.Npad, 128));
    ProfScope ps(h, "sepup_c%d_n%d_%dx%d", a.inC, a.N, to.H, to.W);
    const bool patch_ok = (to.W == 16 || to.W == 32 || to.W == 64) && ((to.H * to.W) % 128) == 0 && (tl.C % 32) == 0 && a.Cpad <= 640;
    // producer / consumer pipelined kernel (k_sepup.h): persistent workgroups, one per CU
    const bool pipe_ok = patch_ok && (to.H * to.W) / 128 >= 2 && (tk.C % 8) == 0 && tk.C <= 64 && a.N == a.Npad && (a.Npad == 128 || a.Npad == 256) &&
                         o.skipx_buf > 0 && o.dw_lo > 0 && o.dw_v > 0 && !(host_dbg(h) & PF_SEL_SEPUP_TO_PATCH);
    if (pipe_ok) {
        SepupArgs s{};
        s.lo = a.up_lo; s.skip = a.up_skip; s.out = (float*)a.out; s.dw_lo = (const float*)p.cptr(o.dw_lo); s.dw_w2 = a.dw_w2;
        s.dw_v = (const float*)p.cptr(o.dw_v);
        s.gap_part = (float*)p.opt_buf(o.gap_parts_plus1 - 1);
        if (s.gap_part && !(a.Npad == 256)) PF_FAIL(h, "sepup: per-tile channel sums need the 256-output instance");
        // one K step per tile leaves nothing between a fast wave's next tile sums and a slow wave's read of the previous ones (k_sepup.h gsum)
        if (s.gap_part && a.Cpad < 64) PF_FAIL(h, "sepup: per-tile channel sums need at least two K steps (Cpad %d < 64)", a.Cpad);
        s.wt = (const unsigned char*)a.wt; s.bias = a.bias; s.skipx = (unsigned char*)p.buf_ptr(o.skipx_buf);
        s.B = B; s.H = to.H; s.C1 = tl.C; s.C2 = tk.C; s.loLd = tl.ld; s.skipLd = tk.ld; s.outLd = to.ld;
        s.N = a.N; s.Cpad = a.Cpad; s.act = a.act; s.acc_scale = a.acc_scale; s.dbg = h->dbg; s.range_slot = a.range_slot;
        if (host_dbg(h) & PF_ACC_CYCLES) {      // per-role cycle accounting of the pipelined kernel (printed at pf_destroy)
            if (ensure_cycle_counters(h)) return 1;
            s.prof = h->d_dbg + PF_CYC_SEPUP.at(a.Npad == 128 ? 0 : 1);
        }
        const int tpf = to.H * to.W / 128, nskip = a.Cpad / 32 - tl.C / 32;
        const int per_xcd = ((B + 7) / 8) * tpf;                  // tiles of the busiest XCD
        const int wgs = 8 * std::min(h->num_cus / 8, per_xcd);
        const dim3 sg(B * tpf);
// (VCOL: at W = 16 a tile is eight image rows and their eight filter sets do not fit the request stage)
#define PF_SEPUP_CASE(WW)                                                                                          \
    if (to.W == WW) {                                                                                              \
        if (nskip > 0 && tk.C <= 32) PF_LAUNCH((sepup_skip_kernel<WW, 32>), sg, dim3(512), h->stream, s);          \
        else if (nskip > 0) PF_LAUNCH((sepup_skip_kernel<WW, 64>), sg, dim3(512), h->stream, s);                   \
        if (a.Npad == 128) PF_LAUNCH((sepup_pipe_kernel<128, WW, 3, false, true, (WW >= 32)>), dim3(wgs), dim3(1024), h->stream, s);                   \
        else PF_LAUNCH((sepup_pipe_kernel<256, WW, 2, true, false, (WW >= 32)>), dim3(wgs), dim3(1024), h->stream, s);                   \
    }
        PF_SEPUP_CASE(64) PF_SEPUP_CASE(32) PF_SEPUP_CASE(16)
#undef PF_SEPUP_CASE
    } else if (o.gap_parts_plus1 > 0) {
        PF_FAIL(h, "sepup: the program asks for per-tile channel sums, which only the pipelined kernel produces");
    } else if (patch_ok && a.Npad == 256) {
        grid.y = 1;
        PF_LAUNCH((sepup_patch_kernel<256, 4, 2>), grid, dim3(512), h->stream, a);
    } else if (patch_ok && a.Npad <= 128) {
        PF_LAUNCH((sepup_patch_kernel<128, 4, 2>), grid, dim3(512), h->stream, a);
    } else if (a.Npad == 256) {   // both 128-channel halves from one pass of the (expensive) fused producer
        grid.y = 1;
        PF_LAUNCH((conv_gemm_split_kernel<128, 256, 4, 2, 1, 1>), grid, dim3(512), h->stream, a);
    } else {
        PF_LAUNCH((conv_gemm_split_kernel<128, 128, 4, 2, 1, 1>), grid, dim3(512), h->stream, a);
    }
    return 0;
}

static int launch_mbconv(pf_handle* h, const Program& p, const PfMbconvOp& o, bool split, int B, unsigned* range_slot) {
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    MbconvArgs a{};
    a.in = (const float*)p.tensor_ptr(o.in_t); a.out = (float*)p.tensor_ptr(o.out_t);
    a.res = (const float*)p.opt_tensor(o.res_t);
    a.resLd = p.opt_ld(o.res_t);
    a.w_exp = (const pf_half*)p.cptr(o.w_exp); a.b_exp = (const float*)p.cptr(o.b_exp);
    a.w_dw = (const float*)p.cptr(o.w_dw); a.b_dw = (const float*)p.cptr(o.b_dw);
    a.w_pwl = (const pf_half*)p.cptr(o.w_pwl); a.b_pwl = (const float*)p.cptr(o.b_pwl);
    const int K = o.K, S = o.stride, dil = o.dil, KS = o.KS;
    a.pad = o.pad; a.act = o.act; a.MidPad = o.MidPad; a.CoutPad = o.CoutPad; a.Cout = o.Cout; a.Mid16 = o.Mid16;
    a.scale_exp = o.scale_exp; a.scale_pwl = o.scale_pwl;
    a.B = B; a.inH = ti.H; a.inW = ti.W; a.Cin = ti.C; a.inLd = ti.ld;
    a.outH = to.H; a.outW = to.W; a.outLd = to.ld;
    a.act_dw = a.act; a.act_out = PF_ACT_NONE; a.outCs = 1;
    a.range_slot = range_slot;
    if (o.variant == 3) {   // ShuffleNetV2 unit: separate activations, channel-strided store, pass-through copy
        a.act_dw = o.shuffle[0].act_dw; a.act_out = o.shuffle[0].act_out; a.outCs = o.shuffle[0].out_cs;
        if (o.shuffle[0].pass_src_t >= 0) {
            a.pass_src = (const float*)p.tensor_ptr(o.shuffle[0].pass_src_t); a.pass_dst = (float*)p.tensor_ptr(o.shuffle[0].pass_dst_t);
            a.passLd = p.tens[o.shuffle[0].pass_src_t].ld; a.passC = p.tens[o.shuffle[0].pass_src_t].C;
            if (a.passC % 16) PF_FAIL(h, "shuffle unit: pass-through channels must be a multiple of 16");
        }
    }
    if ((o.variant == 0 && ((a.MidPad % 32) || a.Cin > 32 * KS)) || (a.Cin % 8) || K != 3 || dil != 1) PF_FAIL(h, "mbconv: unsupported block shape");
    if (o.variant != 3 && a.act != PF_ACT_RELU && a.act != PF_ACT_HSWISH) PF_FAIL(h, "mbconv: activation must be relu or hard-swish");
    ProfScope ps(h, "%s_k%ds%d_c%d_m%d_n%d_%dx%d", o.variant == 3 ? "shuffle" : "mbconv", K, S, a.Cin, a.Mid16, a.Cout, to.H, to.W);
    // (stride, Cin/32, Cout/16) -> patch shape and mid-channel split; low-resolution blocks use MSPLIT = 4
#define PF_MBCONV_CASE(SS, KSS, PHH, PWW, NTT, MS)                                                                \
    if (S == SS && KS == KSS && a.CoutPad <= 16 * NTT) {                                                           \
        const int patches = pf_div_up(to.H, PHH) * pf_div_up(to.W, PWW);                                           \
        PF_LAUNCH((mbconv_wave_kernel<SS, KSS, PHH, PWW, NTT, MS>),                                                \
                  dim3(MS > 1 ? patches : pf_div_up(patches, 4), B), dim3(256), h->stream, a);                     \
    } else
    if (o.variant == 2) {   // depthwise-separable block (no expand conv): dw 3x3 + act -> pointwise [+ x]
        a.w_pwl32 = (const float*)p.cptr(o.w_pwl);
        if (S != 1 || a.Cin != 16 || a.Mid16 != 16 || a.MidPad != 16 || a.CoutPad > 32) PF_FAIL(h, "dsconv: unsupported block shape");
        // (exact f32 in f32s programs too: with no expand conv the block is bandwidth-bound, the split flavour measured 0.17 vs 0.16 ms)
        if (a.act == PF_ACT_RELU) PF_LAUNCH((mbconv_wave_f32_kernel<1, 16, 4, 8, true, false, PF_ACT_RELU>), dim3(pf_div_up(pf_div_up(to.H, 4) * pf_div_up(to.W, 8), 4), B), dim3(256), h->stream, a);
        else PF_LAUNCH((mbconv_wave_f32_kernel<1, 16, 4, 8, true>), dim3(pf_div_up(pf_div_up(to.H, 4) * pf_div_up(to.W, 8), 4), B), dim3(256), h->stream, a);
    } else if (o.variant == 1) {   // exact-f32 variant (high-resolution blocks), weights packed as f32
        a.w_exp32 = (const float*)p.cptr(o.w_exp); a.w_pwl32 = (const float*)p.cptr(o.w_pwl);
        const int CP = o.KS;
        if (a.MidPad != a.Mid16 || a.CoutPad > 32) PF_FAIL(h, "mbconv(f32): unsupported block shape");
        if (S == 2 && CP == 16) {
            const dim3 g(pf_div_up(pf_div_up(to.H, 4) * pf_div_up(to.W, 4), 4), B);
            if (split && a.act == PF_ACT_RELU) PF_LAUNCH((mbconv_wave_f32_kernel<2, 16, 4, 4, false, true, PF_ACT_RELU>), g, dim3(256), h->stream, a);
            else if (split) PF_LAUNCH((mbconv_wave_f32_kernel<2, 16, 4, 4, false, true>), g, dim3(256), h->stream, a);
            else PF_LAUNCH((mbconv_wave_f32_kernel<2, 16, 4, 4>), g, dim3(256), h->stream, a);
        } else if (S == 1 && CP == 32) {
            const dim3 g(pf_div_up(pf_div_up(to.H, 4) * pf_div_up(to.W, 8), 4), B);
            if (split && a.act == PF_ACT_RELU) PF_LAUNCH((mbconv_wave_f32_kernel<1, 32, 4, 8, false, true, PF_ACT_RELU>), g, dim3(256), h->stream, a);
            else if (split) PF_LAUNCH((mbconv_wave_f32_kernel<1, 32, 4, 8, false, true>), g, dim3(256), h->stream, a);
            else PF_LAUNCH((mbconv_wave_f32_kernel<1, 32, 4, 8>), g, dim3(256), h->stream, a);
        }
        else PF_FAIL(h, "mbconv(f32): no kernel for stride %d, %d input channels", S, a.Cin);
    } else
    if (o.variant == 3) {
        PF_MBCONV_CASE(1, 1, 4, 8, 2, 1)
        PF_MBCONV_CASE(1, 2, 4, 8, 4, 4)
        PF_MBCONV_CASE(1, 4, 4, 4, 8, 4)
        PF_FAIL(h, "shuffle unit: no kernel for %d channels", a.Cin);
    } else
    PF_MBCONV_CASE(2, 2, 4, 4, 5, 4)
    PF_MBCONV_CASE(1, 3, 4, 8, 5, 4)
    PF_FAIL(h, "mbconv: no kernel for stride %d, %d input channels, %d output channels", S, a.Cin, a.Cout);
#undef PF_MBCONV_CASE
    return 0;
}

static int launch_expdw(pf_handle* h, const Program& p, const PfExpdwOp& o, int B, unsigned* range_slot) {
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    ConvGemmArgs a{};
    a.in = p.tensor_ptr(o.in_t); a.out = p.tensor_ptr(o.out_t);
    a.gap_out = (float*)p.opt_buf(o.gap_buf);
    a.wt = p.cptr(o.w_exp); a.bias = (const float*)p.cptr(o.b_exp);
    a.dw_w2 = (const float*)p.cptr(o.w_dw); a.dw_b = (const float*)p.cptr(o.b_dw);
    const int K = o.K, pad = o.pad, dil = o.dil;
    a.act = o.act; a.Cpad = o.Cpad; a.Npad = o.Npad; a.N = o.N; a.acc_scale = o.acc_scale;
    a.B = B; a.inH = ti.H; a.inW = ti.W; a.inC = ti.C; a.inLd = ti.ld;
    a.outH = to.H; a.outW = to.W; a.outLd = to.ld; a.outCs = 1; a.outCpad = to.C;
    a.KH = a.KW = 1; a.stride = 1; a.pad = 0; a.dil = 1; a.store_out = 1;
    a.dbg = h->dbg;
    a.range_slot = range_slot;
    const int ohw = to.H * to.W;
    const int dstride = o.stride > 0 ? o.stride : 1;
    if (dstride == 2) {   // 64 x 64 -> 32 x 32, depthwise stride 2: whole image per workgroup, quadrant by quadrant
        if (ti.H != 64 || ti.W != 64 || to.H != 32 || to.W != 32 || a.Cpad != 32 || (a.inC % 8) || K != 5 || dil != 1 || pad != 2 ||
            to.C != a.N || (a.act != PF_ACT_RELU && a.act != PF_ACT_HSWISH))
            PF_FAIL(h, "expdw(stride 2): unsupported shape");
        ProfScope ps2(h, "expdw%dx%ds2_c%d_n%d_%dx%d", K, K, a.inC, a.N, to.H, to.W);
        if (a.act == PF_ACT_RELU) PF_LAUNCH((expdw_image_s2_kernel<5, PF_ACT_RELU>), dim3(B, pf_div_up(a.N, 16)), dim3(512), h->stream, a);
        else PF_LAUNCH((expdw_image_s2_kernel<5>), dim3(B, pf_div_up(a.N, 16)), dim3(512), h->stream, a);
        return 0;
    }
    if (to.H == 32 && to.W == 32 && ti.H == 32 && ti.W == 32) {   // whole 32 x 32 image per workgroup, GEMM straight from global
        if (a.Cpad > 64 || (a.inC % 8) || pad != dil * (K - 1) / 2 || to.C != a.N || (a.act != PF_ACT_RELU && a.act != PF_ACT_HSWISH))
            PF_FAIL(h, "expdw(32x32): unsupported shape");
        ProfScope ps2(h, "expdw%dx%dd%d_c%d_n%d_%dx%d", K, K, dil, a.inC, a.N, to.H, to.W);
        dim3 g2(B, pf_div_up(a.N, 16));
        if (K == 5 && dil == 1 && a.act == PF_ACT_RELU) PF_LAUNCH((expdw_image_kernel<5, 1, PF_ACT_RELU>), g2, dim3(512), h->stream, a);
        else if (K == 5 && dil == 1) PF_LAUNCH((expdw_image_kernel<5, 1>), g2, dim3(512), h->stream, a);
        else if (K == 3 && dil == 1) PF_LAUNCH((expdw_image_kernel<3, 1>), g2, dim3(512), h->stream, a);
        else PF_FAIL(h, "expdw(32x32): no kernel for k%d dil %d", K, dil);
        return 0;
    }
    if (ti.H != to.H || ti.W != to.W || to.W > 16 || (256 % ohw) != 0 || 256 / ohw > 4 || pad != dil * (K - 1) / 2 || to.C != a.N)
        PF_FAIL(h, "expdw: unsupported shape (%dx%d, k%d pad %d dil %d)", to.H, to.W, K, pad, dil);
    if (a.act != PF_ACT_RELU && a.act != PF_ACT_HSWISH) PF_FAIL(h, "expdw: activation must be relu or hard-swish");
    dim3 grid(pf_div_up(B * ohw, 256), pf_div_up(a.N, 64));
    ProfScope ps(h, "expdw%dx%dd%d_c%d_n%d_%dx%d", K, K, dil, a.inC, a.N, to.H, to.W);
    const bool w16 = to.W == 16 && to.H == 16;      // image shape known at compile time: leaner depthwise epilogue
    if (K == 3 && dil == 1 && w16) PF_LAUNCH((conv_gemm_split_kernel<256, 64, 8, 1, 1, 0, 3, 1, 16>), grid, dim3(512), h->stream, a);
    else if (K == 5 && dil == 1 && w16) PF_LAUNCH((conv_gemm_split_kernel<256, 64, 8, 1, 1, 0, 5, 1, 16>), grid, dim3(512), h->stream, a);
    else if (K == 5 && dil == 2 && w16) PF_LAUNCH((conv_gemm_split_kernel<256, 64, 8, 1, 1, 0, 5, 2, 16>), grid, dim3(512), h->stream, a);
    else if (K == 3 && dil == 1) PF_LAUNCH((conv_gemm_split_kernel<256, 64, 8, 1, 1, 0, 3, 1>), grid, dim3(512), h->stream, a);
    else if (K == 5 && dil == 1) PF_LAUNCH((conv_gemm_split_kernel<256, 64, 8, 1, 1, 0, 5, 1>), grid, dim3(512), h->stream, a);
    else if (K == 5 && dil == 2) PF_LAUNCH((conv_gemm_split_kernel<256, 64, 8, 1, 1, 0, 5, 2>), grid, dim3(512), h->stream, a);
    else PF_FAIL(h, "expdw: no kernel for k%d dil %d", K, dil);
    return 0;
}

static int launch_mbx(pf_handle* h, const Program& p, const PfMbxOp& o, int B, unsigned* range_slot) {
    const PfTensorRec& ti = p.tens[o.in_t];
    MbxArgs a{};
    a.in = (const float*)p.tensor_ptr(o.in_t);
    a.out = (float*)p.opt_tensor(o.out_t);
    a.res = (const float*)p.opt_tensor(o.res_t);
    a.gap_out = (float*)p.opt_buf(o.gap_buf);
    a.gate = (const float*)p.opt_buf(o.gate_buf);
    a.w1 = (const unsigned char*)p.cptr(o.w1); a.ctile = (const float*)p.cptr(o.ctile);
    a.w2 = (const unsigned char*)p.cptr(o.w2); a.b2 = (const float*)p.cptr(o.b2);
    const int K = o.K, pad = o.pad, dil = o.dil, KS = o.KS, Cout = o.Cout, mode = o.mode, nw = o.waves;
    a.act = o.act; a.T = o.T; a.CEXP = o.Cexp;
    a.scale1 = o.scale1; a.scale2 = o.scale2;
    a.B = B; a.inC = ti.C; a.inLd = ti.ld;
    a.outLd = p.opt_ld(o.out_t); a.resLd = p.opt_ld(o.res_t);
    a.range_slot = range_slot;
    a.dbg = h->dbg;
    const bool proj = mode == 0 || mode == 2, sq = mode == 1 || mode == 3;
    if (host_dbg(h) & PF_ACC_CYCLES) {      // per-wave cycle accounting (ablation build; printed at pf_destroy)
        if (ensure_cycle_counters(h)) return 1;
        const int shape = KS == 3 ? 0 : (KS == 4 ? (K == 3 ? 1 : 2) : 3);
        a.prof = h->d_dbg + PF_CYC_MBX.at(shape * 4 + mode);
    }
    if (ti.H != 16 || ti.W != 16 || (ti.C & 3) || ti.C > 32 * KS || (ti.ld & 3) || pad != dil * (K - 1) / 2 || mode < 0 || mode > 3 ||
        (a.act != PF_ACT_RELU && a.act != PF_ACT_HSWISH) || a.T < 1 || a.CEXP > 32 * a.T || (nw != 8 && nw != 16) ||
        (proj && (!a.out || !a.w2 || !a.b2 || (a.outLd & 3) || p.tens[o.out_t].C != Cout || (a.res && (a.resLd & 3)))) ||
        (sq && !a.gap_out) || (mode == 2 && (!a.gate || (a.CEXP & 31))) ||      // mode 2 DMAs whole 32-float gate tiles of the face
         (mode == 3 && (!a.out || (a.outLd & 1) || p.tens[o.out_t].C < a.CEXP)))
        PF_FAIL(h, "mbx: unsupported shape (%dx%dx%d, k%d pad %d dil %d, mode %d, %d waves)", ti.H, ti.W, ti.C, K, pad, dil, mode, nw);
    ProfScope ps(h, "mbx%s%dx%dd%d_c%d_m%d_n%d_16x16", mode == 0 ? "" : (mode == 1 ? "A" : (mode == 2 ? "B" : "S")), K, K, dil, ti.C, a.CEXP, proj ? Cout : 0);
    // One workgroup per CU, work units strided over the grid.  A unit is a face -- or, in the squeeze modes (whose channel
    // tiles are independent), one of `nsplit` tile ranges of a face, chosen so that the last round of the persistent grid is
    // full (last_round_cost).
    a.nsplit = 1;
    if (sq) {
        const int cus = std::max(1, persistent_grid(1 << 20, 1));
        double best = 1e30;
        for (int ns = 1; ns <= 4 && ns <= a.T; ++ns) {
            const double face_times = last_round_cost(B, ns, cus);
            if (face_times < best - 1e-9) { best = face_times; a.nsplit = ns; }
        }
    }
    const dim3 grid(persistent_grid(B * a.nsplit, 1));
    const int lrc = pf_mbx_launch(a, nw, KS, Cout, K, dil, mode, (int)grid.x, h->stream);      // mbx_launch.cpp (own translation unit)
    if (lrc > 0) PF_FAIL(h, "launch of mbx_kernel failed: %s", hipGetErrorString((hipError_t)lrc));
    if (lrc != 0) PF_FAIL(h, "mbx: no kernel for %d waves, KS %d Cout %d k%d dil %d mode %d", nw, KS, Cout, K, dil, mode);
    return 0;
}

static int launch_front2(pf_handle* h, const Program& p, const PfFront2Op& o, const void* d_input, int input_kind, int B, unsigned* range_slot) {
    const PfTensorRec& to = p.tens[o.out_t];
    Front2Args a{};
    a.in = d_input; a.out = (float*)p.tensor_ptr(o.out_t); a.outLd = to.ld;
    a.w_u8 = (const pf_half*)p.cptr(o.w_u8); a.w_f32 = (const pf_half*)p.cptr(o.w_f32); a.b_stem = (const float*)p.cptr(o.b_stem);
    a.s_u8 = o.s_u8; a.s_f32 = o.s_f32;
    a.act_stem = o.act_stem;
    a.w_dw = (const float*)p.cptr(o.w_dw); a.b_dw = (const float*)p.cptr(o.b_dw); a.w_pw = (const float*)p.cptr(o.w_pw); a.b_pw = (const float*)p.cptr(o.b_pw);
    a.B = B; a.H = p.hdr.in_h; a.W = p.hdr.in_w; a.OH = to.H; a.OW = to.W; a.tilesX = pf_div_up(to.W, 32);
    a.range_slot = range_slot;
    if (to.C != 16 || (to.ld & 3) || to.H != (a.H + 1) / 2 || to.W != (a.W + 1) / 2 || (a.W & 3) || ((size_t)d_input & 3))
        PF_FAIL(h, "front2: unsupported shapes (%dx%d input, %dx%dx%d output)", a.H, a.W, to.H, to.W, to.C);
    ProfScope ps(h, "stem_block0");
    const dim3 grid(a.tilesX * pf_div_up(to.H, 8), B);
    if (input_kind == PF_INPUT_F32_NCHW) PF_LAUNCH((lm_front2_kernel<true>), grid, dim3(256), h->stream, a);
    else PF_LAUNCH((lm_front2_kernel<false>), grid, dim3(256), h->stream, a);
    return 0;
}

// Launchers of the small layers (k_layers.h, k_front.h stem): one function per op code, each builds its kernel's argument struct from
// the op's named record (pf_program.h) and launches.  Included by engine.cpp only, after its Program / PF_FAIL / PF_LAUNCH / ProfScope.
template <typename T>
static int launch_stem(pf_handle* h, const Program& p, const PfStemOp& o, const void* d_input, int input_kind, bool split, int B, unsigned* range_slot) {
    const PfTensorRec& to = p.tens[o.out_t];
    StemArgs a{};
    a.in = o.in_t < 0 ? d_input : (const void*)p.tensor_ptr(o.in_t);
    a.in_f32_nchw = (o.in_t < 0 && input_kind == PF_INPUT_F32_NCHW) ? 1 : 0;
    a.wt = (const float*)p.cptr(a.in_f32_nchw ? o.wt_f32 : o.wt_u8);
    a.bias = (const float*)p.cptr(o.bias);
    a.out = p.tensor_ptr(o.out_t);
    a.B = B; a.inH = p.hdr.in_h; a.inW = p.hdr.in_w;
    a.outH = to.H; a.outW = to.W; a.outLd = to.ld; a.act = o.act; a.CO = to.C;
    if (to.C % 16) PF_FAIL(h, "stem conv needs a multiple of 16 output channels, got %d", to.C);
    if (a.act != PF_ACT_NONE && a.act != PF_ACT_RELU && a.act != PF_ACT_HSWISH && a.act != PF_ACT_SILU) PF_FAIL(h, "stem conv: unsupported activation %d", a.act);
    ProfScope ps(h, "stem_conv");
    if (split) {
        // f32s programs whose packer provided MFMA weights: the staged-image matrix-core kernel (k_front.h)
        if (o.in_t < 0 && o.mfma_w_u8 >= 0 && (to.C == 16 || to.C == 64) && (p.hdr.in_w & 3) == 0 && ((size_t)d_input & 3) == 0 && to.H == p.hdr.in_h / 2) {
            StemMfmaArgs s{};
            s.in = d_input; s.out = (float*)p.tensor_ptr(o.out_t); s.outLd = to.ld;
            s.w_u8 = (const pf_half*)p.cptr(o.mfma_w_u8); s.w_f32 = (const pf_half*)p.cptr(o.mfma_w_f32); s.bias = (const float*)p.cptr(o.bias);
            s.s_u8 = o.s_u8; s.s_f32 = o.s_f32;
            s.B = B; s.H = p.hdr.in_h; s.W = p.hdr.in_w; s.OH = to.H; s.OW = to.W; s.act = a.act;
            s.TH = 8; s.TW = 32; s.tilesX = pf_div_up(to.W, s.TW);
            s.range_slot = range_slot;
            // the float-input staging loop divides i < IRH * IRW * 3 by IRW * 3 with pf_div_small (IRH = 2 TH + 1, IRW = 2 TW + 1)
            if (!pf_div_small_domain_ok((2 * s.TH + 1) * (2 * s.TW + 1) * 3, (2 * s.TW + 1) * 3)) PF_FAIL(h, "stem: tile %dx%d outside pf_div_small's exact range", s.TH, s.TW);
            const dim3 sg(s.tilesX * pf_div_up(to.H, s.TH), B);
            // tile 8 x 32 output pixels: image region 17 rows x 65 pixels (200 halves per LDS row)
            if (to.C == 16) {
                if (a.in_f32_nchw) PF_LAUNCH((stem_mfma_kernel<1, 256, 17, 200, true>), sg, dim3(256), h->stream, s);
                else PF_LAUNCH((stem_mfma_kernel<1, 256, 17, 200, false>), sg, dim3(256), h->stream, s);
            } else {
                if (a.in_f32_nchw) PF_LAUNCH((stem_mfma_kernel<4, 256, 17, 200, true>), sg, dim3(256), h->stream, s);
                else PF_LAUNCH((stem_mfma_kernel<4, 256, 17, 200, false>), sg, dim3(256), h->stream, s);
            }
            return 0;
        }
    }
    PF_LAUNCH((stem_conv_kernel<T>), dim3(pf_div_up(B * to.H * to.W, 256), to.C / 16), dim3(256), h->stream, a);
    return 0;
}

template <typename T>
static int launch_dw(pf_handle* h, const Program& p, const PfDwOp& o, int B) {
    constexpr int VE = PfVec<T>::N;
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    DwArgs a{};
    a.in = p.tensor_ptr(o.in_t); a.wt = p.cptr(o.wt); a.bias = (const float*)p.cptr(o.bias);
    a.out = p.tensor_ptr(o.out_t);
    a.B = B; a.inH = ti.H; a.inW = ti.W; a.C = ti.C; a.inLd = ti.ld;
    a.outH = to.H; a.outW = to.W; a.outLd = to.ld;
    a.K = o.K; a.stride = o.stride; a.pad = o.pad; a.dil = o.dil; a.act = o.act;
    ProfScope ps(h, "dw%dx%ds%dd%d_c%d_%dx%d", a.K, a.K, a.stride, a.dil, a.C, a.outH, a.outW);
    auto tgrid = [&](int tx) {
        const long long n = (long long)B * to.H * ((to.W + tx - 1) / tx) * (ti.C / VE);
        return dim3((unsigned)((n + 255) / 256));
    };
    if (a.K == 3 && a.stride == 1 && a.dil == 1) PF_LAUNCH((dw_conv_tiled_kernel<T, 3, 1, 1, 4>), tgrid(4), dim3(256), h->stream, a);
    else if (a.K == 3 && a.stride == 2 && a.dil == 1) PF_LAUNCH((dw_conv_tiled_kernel<T, 3, 2, 1, 4>), tgrid(4), dim3(256), h->stream, a);
    else if (a.K == 5 && a.stride == 1 && a.dil == 1) PF_LAUNCH((dw_conv_tiled_kernel<T, 5, 1, 1, 4>), tgrid(4), dim3(256), h->stream, a);
    else if (a.K == 5 && a.stride == 2 && a.dil == 1) PF_LAUNCH((dw_conv_tiled_kernel<T, 5, 2, 1, 4>), tgrid(4), dim3(256), h->stream, a);
    else if (a.K == 5 && a.stride == 1 && a.dil == 2) PF_LAUNCH((dw_conv_tiled_kernel<T, 5, 1, 2, 8>), tgrid(8), dim3(256), h->stream, a);
    else {
        const long long total = (long long)B * to.H * to.W * (ti.C / VE);
        PF_LAUNCH((dw_conv_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), h->stream, a);
    }
    return 0;
}

template <typename T>
static int launch_upcat(pf_handle* h, const Program& p, const PfUpcatOp& o, int B) {
    constexpr int VE = PfVec<T>::N;
    const PfTensorRec& tl = p.tens[o.lo_t];
    const PfTensorRec& tk = p.tens[o.skip_t];
    const PfTensorRec& to = p.tens[o.out_t];
    UpcatArgs a{};
    a.lo = p.tensor_ptr(o.lo_t); a.skip = p.tensor_ptr(o.skip_t); a.out = p.tensor_ptr(o.out_t);
    a.B = B; a.loH = tl.H; a.loW = tl.W; a.C1 = tl.C; a.loLd = tl.ld;
    a.C2 = tk.C; a.skipLd = tk.ld; a.outLd = to.ld;
    const long long total = (long long)B * to.H * to.W * ((tl.C + tk.C) / VE);
    ProfScope ps(h, "upsample_concat");
    PF_LAUNCH((upsample_concat_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), h->stream, a);
    return 0;
}

template <typename T>
static int launch_gap(pf_handle* h, const Program& p, const PfGapOp& o, int B) {
    constexpr int VE = PfVec<T>::N;
    const PfTensorRec& ti = p.tens[o.in_t];
    GapArgs a{};
    a.in = p.tensor_ptr(o.in_t); a.out = (float*)p.buf_ptr(o.out_buf);
    a.B = B; a.HW = ti.H * ti.W; a.C = ti.C; a.ld = ti.ld;
    ProfScope ps(h, "gap");
    PF_LAUNCH((gap_kernel<T>), dim3(pf_div_up(ti.C / VE, 8), B), dim3(256), h->stream, a);
    return 0;
}

static int launch_fc(pf_handle* h, const Program& p, const PfFcOp& o, int B) {
    FcArgs a{};
    a.x = (const float*)p.buf_ptr(o.x_buf); a.y = (float*)p.buf_ptr(o.y_buf);
    a.wt = (const float*)p.cptr(o.wt); a.bias = (const float*)p.cptr(o.bias);
    a.B = B; a.K = o.K; a.N = o.N; a.act = o.act;
    a.scale2 = (const float*)p.cptr(o.scale2); a.shift2 = (const float*)p.cptr(o.shift2); a.act2 = o.act2;
    ProfScope ps(h, "fc");
    if (a.K <= PF_FC_MAXK) PF_LAUNCH(fc_kernel<true>, dim3(pf_div_up(a.N, PF_FC_BN), pf_div_up(B, PF_FC_BB)), dim3(256), h->stream, a);
    else PF_LAUNCH(fc_kernel<false>, dim3(pf_div_up(a.N, PF_FC_BN), pf_div_up(B, PF_FC_BB)), dim3(256), h->stream, a);
    return 0;
}

static int launch_fc2(pf_handle* h, const Program& p, const PfFc2Op& o, int B) {
    Fc2Args a{};
    a.x = (const float*)p.buf_ptr(o.x_buf); a.y = (float*)p.buf_ptr(o.y_buf);
    a.w1 = (const float*)p.cptr(o.w1); a.b1 = (const float*)p.cptr(o.b1);
    a.K = o.K; a.R = o.R; a.act1 = o.act1;
    a.scale2 = (const float*)p.cptr(o.scale2); a.shift2 = (const float*)p.cptr(o.shift2); a.act1b = o.act1b;
    a.w2 = (const float*)p.cptr(o.w2); a.b2 = (const float*)p.cptr(o.b2); a.N = o.N; a.act2 = o.act2;
    a.B = B;
    a.nparts = o.nparts > 0 ? o.nparts : 1; a.xscale = o.xscale;
    if (a.nparts == 1) a.xscale = 1.f;
    if (a.K < 1 || a.K > 960 || a.R < 4 || a.R > 960 || (a.R & 3) || a.N < 4 || a.N > 960 || (a.N & 3) || !a.w1 || !a.w2 || (a.scale2 && !a.shift2))
        PF_FAIL(h, "fc2: unsupported shape %d -> %d -> %d", a.K, a.R, a.N);
    ProfScope ps(h, "fc");
    PF_LAUNCH(fc2_kernel, dim3(pf_div_up(B, PF_FC2_FB)), dim3(1024), h->stream, a);
    return 0;
}

template <typename T>
static int launch_scse(pf_handle* h, const Program& p, const PfScseOp& o, int B) {
    constexpr int VE = PfVec<T>::N;
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    ScseArgs a{};
    a.in = p.tensor_ptr(o.in_t); a.out = p.tensor_ptr(o.out_t);
    a.cse = (const float*)p.buf_ptr(o.cse_buf); a.sse_w = (const float*)p.cptr(o.sse_w);
    a.sse_b = o.sse_b;
    a.B = B; a.HW = ti.H * ti.W; a.C = ti.C; a.ld = ti.ld; a.outLd = to.ld;
    const int lpp = ti.C / VE;
    if (lpp < 1 || lpp > 64 || (lpp & (lpp - 1))) PF_FAIL(h, "scse: C/VE=%d must be a power of two <= 64", lpp);
    const long long total = (long long)B * a.HW;
    if (o.gap_parts_plus1 > 0) {        // + per-tile channel sums (the face-attribute head's decx8 pool; ir.py scse(gap_parts=True))
        if (lpp != 64 || (a.HW % PF_SCSE_TILE) != 0) PF_FAIL(h, "scse: tile sums need C/VE == 64 and HW %% %d == 0", PF_SCSE_TILE);
        ProfScope ps(h, "scse_sum");
        PF_LAUNCH((scse_tile_sum_kernel<T>), dim3((unsigned)(B * (a.HW / PF_SCSE_TILE))), dim3(256), h->stream, a,
                  (float*)p.buf_ptr(o.gap_parts_plus1 - 1));
        return 0;
    }
    ProfScope ps(h, "scse");
    PF_LAUNCH((scse_kernel<T>), dim3((unsigned)((total + 256 / lpp - 1) / (256 / lpp))), dim3(256), h->stream, a);
    return 0;
}

static int launch_faceattr(pf_handle* h, const Program& p, const PfFaceattrOp& o, int B) {
    FaceAttrsArgs a{};
    a.out = (float*)p.buf_ptr(o.out_buf); a.wt = (const float*)p.cptr(o.wt); a.bias = (const float*)p.cptr(o.bias);
    a.B = B;
    int k = 0;
    for (int s = 0; s < 3; ++s) {
        const PfFaceattrSrc& g = o.src[s];
        a.src[s].p = (const float*)p.buf_ptr(g.src_buf);
        a.src[s].nparts = g.nparts; a.src[s].C = g.C; a.src[s].ld = g.ld;
        a.src[s].scale = g.scale;
        if (g.nparts < 1 || g.C < 1 || g.ld < g.C || (long long)g.nparts * g.ld > p.bufs[g.src_buf].elems_per_item)
            PF_FAIL(h, "face_attrs: bad pooled source %d", s);
        k += g.C;
    }
    if (k != PF_FACE_ATTR_K || p.bufs[o.out_buf].elems_per_item < PF_FACE_ATTR_REC)
        PF_FAIL(h, "face_attrs: pooled vector of %d channels (the fc head takes %d)", k, PF_FACE_ATTR_K);
    ProfScope ps(h, "face_attrs");
    PF_LAUNCH(face_attrs_kernel, dim3(B), dim3(256), h->stream, a);
    return 0;
}

template <typename T>
static int launch_hmdec(pf_handle* h, const Program& p, const PfHmdecOp& o, int B) {
    const PfTensorRec& tf = p.tens[o.feat_t];
    HmDecodeArgs a{};
    a.amax_val = (const float*)p.buf_ptr(o.val_buf); a.amax_idx = (const int*)p.buf_ptr(o.idx_buf);
    a.feat = p.tensor_ptr(o.feat_t); a.off_wt = (const float*)p.cptr(o.off_wt); a.off_bias = (const float*)p.cptr(o.off_bias);
    a.P = o.P; a.nslots = o.nslots;
    a.loc = (float*)p.buf_ptr(o.loc_buf); a.score = (float*)p.buf_ptr(o.score_buf);
    a.crop = h->pipe.d_crop_for_decode; a.kps = h->pipe.d_kps_for_decode;
    a.B = B; a.H = tf.H; a.W = tf.W; a.C = tf.C; a.featLd = tf.ld;
    ProfScope ps(h, "hm_decode");
    PF_LAUNCH((hm_decode_kernel<T>), dim3(pf_div_up(B * a.P, 4)), dim3(256), h->stream, a);
    return 0;
}

template <typename T>
static int launch_addup(pf_handle* h, const Program& p, const PfAddupOp& o, int B) {
    constexpr int VE = PfVec<T>::N;
    const PfTensorRec& ta = p.tens[o.a_t];
    const PfTensorRec& tb = p.tens[o.b_t];
    const PfTensorRec& to = p.tens[o.out_t];
    AddUpArgs a{};
    a.a = p.tensor_ptr(o.a_t); a.b = p.tensor_ptr(o.b_t); a.out = p.tensor_ptr(o.out_t);
    a.B = B; a.H = ta.H; a.W = ta.W; a.C = ta.C; a.aLd = ta.ld; a.bLd = tb.ld; a.outLd = to.ld;
    a.shift = o.shift; a.act = o.act;
    if ((tb.H << a.shift) != ta.H || (tb.W << a.shift) != ta.W || tb.C != ta.C || to.C != ta.C)
        PF_FAIL(h, "addup: inconsistent shapes");
    const long long total = (long long)B * ta.H * ta.W * (ta.C / VE);
    ProfScope ps(h, "add_upsample");
    PF_LAUNCH((add_upsample_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), h->stream, a);
    return 0;
}

template <typename T>
static int launch_maxpool(pf_handle* h, const Program& p, const PfMaxpoolOp& o, int B) {
    constexpr int VE = PfVec<T>::N;
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    PoolArgs a{};
    a.in = p.tensor_ptr(o.in_t); a.out = p.tensor_ptr(o.out_t);
    a.B = B; a.inH = ti.H; a.inW = ti.W; a.C = ti.C; a.inLd = ti.ld;
    a.outH = to.H; a.outW = to.W; a.outLd = to.ld;
    const long long total = (long long)B * to.H * to.W * (ti.C / VE);
    ProfScope ps(h, "maxpool");
    PF_LAUNCH((maxpool2_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), h->stream, a);
    return 0;
}

template <typename T>
static int launch_copy(pf_handle* h, const Program& p, const PfCopyOp& o, int B) {
    constexpr int VE = PfVec<T>::N;
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    CopyArgs a{};
    a.in = p.tensor_ptr(o.in_t); a.out = p.tensor_ptr(o.out_t);
    a.B = B; a.inH = ti.H; a.inW = ti.W; a.C = ti.C; a.inLd = ti.ld; a.outLd = to.ld;
    a.outCs = o.out_cs; a.up = o.up;
    const long long total = (long long)B * ti.H * a.up * ti.W * a.up * (ti.C / VE);
    ProfScope ps(h, "copy_channels");
    PF_LAUNCH((copy_channels_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), h->stream, a);
    return 0;
}

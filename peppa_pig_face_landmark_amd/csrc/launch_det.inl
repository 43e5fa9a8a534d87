// Launchers of the detector's ops (k_det.h).  Included by engine.cpp only.

// LDS rows (MAXR) of the det_unit_kernel / det_c3_kernel instance an op runs on, 0 if there is none; the PF_DETUNIT_CASE / PF_DETC3_CASE
// tables below are asserted against these
constexpr int det_unit_maxr(int C, int S) {
    return S == 1 ? (C == 32 ? 256 : C == 64 ? 128 : C == 128 ? 144 : 0) : S == 2 ? (C == 32 ? 480 : C == 64 ? 256 : C == 128 ? 128 : 0) : 0;
}
constexpr int det_c3_maxr(int CIN, int tail) { return CIN == 192 && tail == 1 ? 128 : CIN == 128 && tail == 2 ? 176 : 0; }

// PF_OPT_DET_TILE: the forced tile replaces the picker's choice (cut to the map like the ablation build's PEPPA_DET_TILE); one whose
// region does not fit is an error, here and -- for the whole program, before its first launch -- in det_forced_tile_fits
static int det_forced_tile(pf_handle* h, const char* what, int S, int max_rows, int outH, int outW, int* TH, int* TW) {
    if (!h->det_tile) return 0;
    const int th = h->det_tile >> 16, tw = h->det_tile & 0xffff;
    const long long rows = ((long long)(th - 1) * S + 3) * ((long long)(tw - 1) * S + 3);      // th < 2^15, tw < 2^16: not an int product
    if (th < 1 || tw < 1 || rows > max_rows)
        PF_FAIL(h, "PF_OPT_DET_TILE: tile %dx%d needs a region of %lld rows, %s holds %d", th, tw, rows, what, max_rows);
    *TH = std::min(th, outH); *TW = std::min(tw, outW);
    return 0;
}

static int det_forced_tile_fits(pf_handle* h, const Program& p) {
    int th = 0, tw = 0;
    char what[64];
    for (const PfOpRec& op : p.ops) {
        if (op.code == PF_OP_DETUNIT) {
            const PfDetunitOp& o = op.as<PfDetunitOp>();
            snprintf(what, sizeof(what), "det_unit_kernel<%d, %d, %d>", o.C, o.K1, o.stride);
            if (det_unit_maxr(o.C, o.stride) && det_forced_tile(h, what, o.stride, det_unit_maxr(o.C, o.stride), 1 << 16, 1 << 16, &th, &tw)) return 1;
        } else if (op.code == PF_OP_DETC3) {
            const PfDetc3Op& o = op.as<PfDetc3Op>();
            snprintf(what, sizeof(what), "det_c3_kernel<%d, %d>", o.CIN, o.tail);
            if (det_c3_maxr(o.CIN, o.tail) && det_forced_tile(h, what, 1, det_c3_maxr(o.CIN, o.tail), 1 << 16, 1 << 16, &th, &tw)) return 1;
        }
    }
    return 0;
}

static int launch_detunit(pf_handle* h, const Program& p, const PfDetunitOp& o, int B, unsigned* range_slot) {
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    DetUnitArgs a{};
    a.in = (const float*)p.tensor_ptr(o.in_t); a.out = (float*)p.tensor_ptr(o.out_t);
    a.w1 = (const pf_half*)p.cptr(o.w1); a.b1 = (const float*)p.cptr(o.b1);
    a.wd = (const float*)p.cptr(o.wd); a.bd = (const float*)p.cptr(o.bd);
    a.w2 = (const pf_half*)p.cptr(o.w2); a.b2 = (const float*)p.cptr(o.b2);
    a.wd1 = (const float*)p.cptr(o.wd1); a.bd1 = (const float*)p.cptr(o.bd1);
    a.w3 = (const pf_half*)p.cptr(o.w3); a.b3 = (const float*)p.cptr(o.b3);
    a.s1 = o.s1; a.s2 = o.s2; a.s3 = o.s3;
    const int C = o.C, K1 = o.K1, S = o.stride;
    a.Cin = o.Cin;
    a.B = B; a.inH = ti.H; a.inW = ti.W; a.inLd = ti.ld; a.outH = to.H; a.outW = to.W; a.outLd = to.ld;
    a.range_slot = range_slot;
    if (host_dbg(h) & PF_ACC_DET_CYCLES) {      // per-phase cycle accounting of det_unit_kernel (ablation build; printed at pf_destroy)
        if (ensure_cycle_counters(h)) return 1;
        a.prof = h->d_dbg + PF_CYC_DETUNIT.at((C == 32 ? 0 : (C == 64 ? 1 : 2)) + 3 * (S - 1));
    }
    if (to.C != 2 * C || ti.C != a.Cin || (S != 1 && S != 2) || to.H != (ti.H - 1) / S + 1 || to.W != (ti.W - 1) / S + 1 ||
        (S == 1 && a.Cin != 2 * C) || (S == 2 && !a.w3))
        PF_FAIL(h, "detunit: inconsistent shapes");
    ProfScope ps(h, "unit_s%d_c%d_%dx%d", S, C, to.H, to.W);
#define PF_DETUNIT_CASE(CC, KK, SS, MAXR, NTHR, PERCU)                                                             \
    if (C == CC && K1 == KK && S == SS) {                                                                          \
        static_assert(det_unit_maxr(CC, SS) == MAXR, "det_unit_maxr");                                             \
        det_pick_tile(h->num_cus, to.H, to.W, SS, MAXR, B, PERCU, &a.TH, &a.TW);                                               \
        if (det_forced_tile(h, "det_unit_kernel<" #CC ", " #KK ", " #SS ">", SS, MAXR, to.H, to.W, &a.TH, &a.TW)) return 1; \
        a.tilesX = pf_div_up(to.W, a.TW); a.tpf = a.tilesX * pf_div_up(to.H, a.TH);                                 \
        PF_LAUNCH((det_unit_kernel<CC, KK, SS, MAXR, NTHR, PERCU * NTHR / 256>), dim3(a.tpf * B), dim3(NTHR), h->stream, a); \
        PF_LAUNCH_NOTE(" tile=%dx%d tpf=%d grid=%d", a.TH, a.TW, a.tpf, a.tpf * B);                                \
    } else
    PF_DETUNIT_CASE(32, 32, 1, 256, 512, 2)
    PF_DETUNIT_CASE(64, 64, 1, 128, 512, 2)
    PF_DETUNIT_CASE(128, 128, 1, 144, 512, 1)
    PF_DETUNIT_CASE(32, 32, 2, 480, 512, 1)
    PF_DETUNIT_CASE(64, 64, 2, 256, 512, 1)
    PF_DETUNIT_CASE(128, 128, 2, 128, 512, 1)
    PF_FAIL(h, "detunit: no kernel for %d branch channels, K %d, stride %d", C, K1, S);
#undef PF_DETUNIT_CASE
    return 0;
}

static int launch_detc3(pf_handle* h, const Program& p, const PfDetc3Op& o, int B, unsigned* range_slot) {
    const PfTensorRec& ta = p.tens[o.srcA_t];
    DetC3Args a{};
    a.srcA = (const float*)p.tensor_ptr(o.srcA_t); a.ldA = ta.ld; a.CA = ta.C;
    a.srcB = (const float*)p.opt_tensor(o.srcB_t); a.ldB = p.opt_ld(o.srcB_t);
    a.out = (float*)p.opt_tensor(o.out_t); a.outLd = p.opt_ld(o.out_t);
    a.out2 = (float*)p.opt_tensor(o.out2_t); a.out2Ld = p.opt_ld(o.out2_t);
    a.rows = (float*)p.opt_buf(o.rows_buf);
    a.wA = (const pf_half*)p.cptr(o.wA); a.bA = (const float*)p.cptr(o.bA);
    a.wB = (const pf_half*)p.cptr(o.wB); a.bB = (const float*)p.cptr(o.bB);
    a.wC = (const pf_half*)p.cptr(o.wC); a.bC = (const float*)p.cptr(o.bC);
    a.wD = (const pf_half*)p.cptr(o.wD); a.bD = (const float*)p.cptr(o.bD);
    a.wE = (const pf_half*)p.cptr(o.wE); a.bE = (const float*)p.cptr(o.bE);
    a.anchors = (const float*)p.cptr(o.anchors);
    a.sA = o.sA; a.sB = o.sB; a.sC = o.sC; a.sD = o.sD;
    a.sE = o.sE; a.det_stride = o.det_stride;
    const int CIN = o.CIN, tail = o.tail;
    a.upA = o.upA; a.row0 = o.row0; a.nrows_total = o.nrows_total;
    a.B = B; a.H = ta.H << a.upA; a.W = ta.W << a.upA;
    a.range_slot = range_slot;
    const int cb = o.srcB_t >= 0 ? p.tens[o.srcB_t].C : 0;
    if (ta.C + cb != CIN || (ta.C % 8) || (o.srcB_t >= 0 && (p.tens[o.srcB_t].H != a.H || p.tens[o.srcB_t].W != a.W)) ||
        (tail == 1 && !a.out2) || (tail == 2 && (!a.rows || !a.anchors)))
        PF_FAIL(h, "detc3: inconsistent shapes");
    ProfScope ps(h, "c3_c%d_t%d_%dx%d", CIN, tail, a.H, a.W);
#define PF_DETC3_CASE(CC, TT, MAXR, NTHR)                                                                          \
    if (CIN == CC && tail == TT) {                                                                                 \
        static_assert(det_c3_maxr(CC, TT) == MAXR, "det_c3_maxr");                                                 \
        det_pick_tile(h->num_cus, a.H, a.W, 1, MAXR, B, 1, &a.TH, &a.TW);                                                      \
        if (det_forced_tile(h, "det_c3_kernel<" #CC ", " #TT ">", 1, MAXR, a.H, a.W, &a.TH, &a.TW)) return 1;     \
        a.tilesX = pf_div_up(a.W, a.TW); a.tpf = a.tilesX * pf_div_up(a.H, a.TH);                                   \
        PF_LAUNCH((det_c3_kernel<CC, TT, MAXR, NTHR>), dim3(a.tpf * B), dim3(NTHR), h->stream, a); \
        PF_LAUNCH_NOTE(" tile=%dx%d tpf=%d grid=%d", a.TH, a.TW, a.tpf, a.tpf * B);                                \
    } else
    PF_DETC3_CASE(192, 1, 128, 512)
    PF_DETC3_CASE(128, 2, 176, 512)
    PF_FAIL(h, "detc3: no kernel for %d input channels, tail %d", CIN, tail);
#undef PF_DETC3_CASE
    return 0;
}

static int launch_detstem(pf_handle* h, const Program& p, const PfDetstemOp& o, const void* d_input, int input_kind, int B, unsigned* range_slot) {
    const PfTensorRec& to = p.tens[o.out_t];
    DetStemArgs a{};
    a.in = d_input; a.in_f32_nchw = input_kind == PF_INPUT_F32_NCHW ? 1 : 0;
    a.out = (float*)p.tensor_ptr(o.out_t); a.outLd = to.ld;
    a.w1_u8 = (const pf_half*)p.cptr(o.w1_u8); a.w1_f32 = (const pf_half*)p.cptr(o.w1_f32); a.b1 = (const float*)p.cptr(o.b1);
    a.w2a = (const pf_half*)p.cptr(o.w2a); a.b2a = (const float*)p.cptr(o.b2a);
    a.w2b = (const pf_half*)p.cptr(o.w2b); a.b2b = (const float*)p.cptr(o.b2b);
    a.w3 = (const pf_half*)p.cptr(o.w3); a.b3 = (const float*)p.cptr(o.b3);
    a.s1_u8 = o.s1_u8; a.s1_f32 = o.s1_f32; a.s2a = o.s2a; a.s2b = o.s2b; a.s3 = o.s3;
    a.B = B; a.H = p.hdr.in_h; a.W = p.hdr.in_w; a.SH = (a.H + 1) / 2; a.SW = (a.W + 1) / 2; a.OH = to.H; a.OW = to.W;
    if (to.C != 16 || a.OH != (a.SH + 1) / 2 || a.OW != (a.SW + 1) / 2) PF_FAIL(h, "detstem: inconsistent shapes");
    a.TH = 4; a.TW = 16; a.tilesX = pf_div_up(a.OW, a.TW);
    a.range_slot = range_slot;
    // the float-input staging loop divides i < IRH * IRW * 3 by IRW * 3 with pf_div_small (IRH = 4 TH + 3, IRW = 4 TW + 3)
    if (!pf_div_small_domain_ok((4 * a.TH + 3) * (4 * a.TW + 3) * 3, (4 * a.TW + 3) * 3)) PF_FAIL(h, "detstem: tile %dx%d outside pf_div_small's exact range", a.TH, a.TW);
    ProfScope ps(h, "stem_block");
    if ((a.W & 3) || ((size_t)d_input & 3)) PF_FAIL(h, "detstem: the image width must be a multiple of 4 and the input 4-byte aligned");
    // tile 4 x 16: stem_1 region 9 x 33 = 297 (304 rows), image region 19 rows x 67 pixels (208 halves per LDS row)
    const dim3 sg(persistent_grid(a.tilesX * pf_div_up(a.OH, a.TH) * B, 3));     // persistent: three workgroups per CU walk the tiles
    if (a.in_f32_nchw) PF_LAUNCH((det_stem_kernel<64, 304, 19, 208, true, 256>), sg, dim3(256), h->stream, a);
    else PF_LAUNCH((det_stem_kernel<64, 304, 19, 208, false, 256>), sg, dim3(256), h->stream, a);
    return 0;
}

template <typename T>
static int launch_detdec(pf_handle* h, const Program& p, const PfDetdecOp& o, int B) {
    const PfTensorRec& ti = p.tens[o.in_t];
    DetDecArgs a{};
    a.in = p.tensor_ptr(o.in_t); a.rows = (float*)p.buf_ptr(o.rows_buf);
    a.row0 = o.row0; a.stride = o.stride; a.anchors = (const float*)p.cptr(o.anchors);
    a.nrows_total = o.nrows_total;
    a.B = B; a.ny = ti.H; a.nx = ti.W; a.ld = ti.ld;
    const long long total = (long long)B * 3 * ti.H * ti.W;
    ProfScope ps(h, "detect_decode");
    PF_LAUNCH((detect_decode_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), h->stream, a);
    return 0;
}

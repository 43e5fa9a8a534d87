// Launchers of the Teacher's HRNet ops (k_chain.h, k_hrb.h, k_layers.h fuse_up_kernel).  Included by engine.cpp only.
static int launch_chain(pf_handle* h, const Program& p, const PfChainOp& o, int B, unsigned* range_slot) {
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    ChainArgs a{};
    a.in = (const float*)p.tensor_ptr(o.in_t); a.out = (float*)p.tensor_ptr(o.out_t);
    a.B = B; a.inLd = ti.ld; a.outLd = to.ld;
    a.n_convs = o.n_convs;
    const int C = o.C;
    static_assert(PF_CHAIN_MAX_CONVS <= sizeof(o.convs) / sizeof(o.convs[0]), "the record holds every conv the kernel takes");
    if (a.n_convs < 2 || a.n_convs > PF_CHAIN_MAX_CONVS || (a.n_convs & 1)) PF_FAIL(h, "chain: %d convs", a.n_convs);
    if (ti.C != C || to.C != C || ti.H != to.H || ti.W != to.W || ti.H != ti.W) PF_FAIL(h, "chain: tensor shapes");
    for (int c = 0; c < a.n_convs; ++c) {
        a.wt[c] = p.cptr(o.convs[c].wt); a.bias[c] = (const float*)p.cptr(o.convs[c].bias);
        a.acc_scale[c] = o.convs[c].acc_scale;
    }
    a.range_slot = range_slot;
    a.dbg = h->dbg;
    ProfScope ps(h, "chain%d_c%d_%dx%d", a.n_convs, C, ti.H, ti.W);
    // 16 / 12 waves per workgroup and a 3 / 4-stage weight ring: measured against 8 waves and against two stages
    // (profiles/r02_run14_teacher_*): 1.30 vs 1.38 / 1.39 ms and 0.68 vs 0.75 / 0.83 ms per 64 faces
    if (C == 72 && ti.H == 16) PF_LAUNCH((basic_chain_kernel<72, 16, 8, 2, 3, 3>), dim3(B), dim3(1024), h->stream, a);
    else if (C == 144 && ti.H == 8) PF_LAUNCH((basic_chain_kernel<144, 8, 4, 3, 3, 4>), dim3(B), dim3(768), h->stream, a);
    else PF_FAIL(h, "chain: no kernel for %d channels at %dx%d", C, ti.H, ti.W);
    return 0;
}

static int launch_block(pf_handle* h, const Program& p, const PfBlockOp& o, int B, unsigned* range_slot) {
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    BlockArgs a{};
    a.in = (const float*)p.tensor_ptr(o.in_t); a.out = (float*)p.tensor_ptr(o.out_t);
    a.B = B; a.H = ti.H; a.inLd = ti.ld; a.outLd = to.ld; a.Cs = ti.C;
    const int C = o.C;
    if (to.C != ti.C || ti.H != to.H || ti.W != to.W || ti.H != ti.W || ti.C < C || ti.C >= C + 4) PF_FAIL(h, "block: tensor shapes");
    for (int c = 0; c < 2; ++c) {
        a.wt[c] = p.cptr(o.convs[c].wt); a.bias[c] = (const float*)p.cptr(o.convs[c].bias);
        a.acc_scale[c] = o.convs[c].acc_scale;
    }
    a.range_slot = range_slot;
    a.dbg = h->dbg;
    ProfScope ps(h, "block_c%d_%dx%d", C, ti.H, ti.W);
    if (C == 18 && ti.W == 64) PF_LAUNCH((basic_block_kernel<18, 64, 4, 7, 1>), dim3(B * (ti.H / 4)), dim3(512), h->stream, a);
    else if (C == 36 && ti.W == 32) PF_LAUNCH((basic_block_kernel<36, 32, 8, 1, 2>), dim3(B * (ti.H / 8)), dim3(512), h->stream, a);
    else if (C == 18 && ti.W == 16) PF_LAUNCH((basic_block_kernel<18, 16, 8, 7, 1>), dim3(B * (ti.H / 8)), dim3(512), h->stream, a);
    else PF_FAIL(h, "block: no kernel for %d channels at %dx%d", C, ti.H, ti.W);
    return 0;
}

static int launch_hrb(pf_handle* h, const Program& p, const PfHrbOp& o, int B, unsigned* range_slot) {
    const PfTensorRec& ti = p.tens[o.in_t];
    const PfTensorRec& to = p.tens[o.out_t];
    HrbArgs a{};
    a.x = (const float*)p.tensor_ptr(o.in_t); a.out = (float*)p.tensor_ptr(o.out_t);
    a.w1 = (const pf_half*)p.cptr(o.w1); a.b1 = (const float*)p.cptr(o.b1);
    a.w2 = (const pf_half*)p.cptr(o.w2); a.b2 = (const float*)p.cptr(o.b2);
    a.w3 = (const pf_half*)p.cptr(o.w3); a.b3 = (const float*)p.cptr(o.b3);
    a.wd = (const pf_half*)p.cptr(o.wd); a.bd = (const float*)p.cptr(o.bd);
    a.s1 = o.s1; a.s2 = o.s2; a.s3 = o.s3; a.sd = o.sd;
    const int CIN = o.CIN;
    a.B = B; a.H = ti.H; a.W = ti.W; a.xLd = ti.ld; a.outLd = to.ld;
    if (ti.C != CIN || to.C != 256 || to.H != ti.H || to.W != ti.W || (CIN == 64) != (a.wd != nullptr))
        PF_FAIL(h, "hrb: inconsistent shapes");
    {   // tile: <= 128 pixels (MAXP), region <= 256 pixels (one load item per thread and chunk); least halo'd pixels in total
        long best = -1;
        for (int tw = 128; tw >= 8; tw /= 2) {
            const int th = 128 / tw;
            const int twc = std::min(tw, (int)ti.W), thc = std::min(th, (int)ti.H);
            const int region = (thc + 2) * (twc + 2);
            if (region > 256 || thc < 1) continue;
            const long cost = (long)pf_div_up(ti.H, thc) * pf_div_up(ti.W, twc) * (region + 64);
            if (best < 0 || cost < best) { best = cost; a.TR = thc; a.TW = twc; }
        }
        if (best < 0) PF_FAIL(h, "hrb: no tile shape for a %d x %d map", ti.H, ti.W);
    }
    a.tiles_x = pf_div_up(ti.W, a.TW);
    a.tpf = a.tiles_x * pf_div_up(ti.H, a.TR);
    a.range_slot = range_slot;
    if (host_dbg(h) & PF_ACC_DET_CYCLES) {      // per-phase cycle accounting (ablation build; printed at pf_destroy)
        if (ensure_cycle_counters(h)) return 1;
        a.prof = h->d_dbg + PF_CYC_HRB.at(CIN == 64 ? 0 : 1);
    }
    ProfScope ps(h, "bottleneck_c%d_%dx%d", CIN, ti.H, ti.W);
    if (CIN == 64) PF_LAUNCH((hr_bottleneck_kernel<64, true, 272, 128, 1>), dim3(a.tpf * B), dim3(1024), h->stream, a);
    else if (CIN == 256) PF_LAUNCH((hr_bottleneck_kernel<256, false, 272, 128, 1>), dim3(a.tpf * B), dim3(1024), h->stream, a);
    else PF_FAIL(h, "hrb: no kernel for %d input channels", CIN);
    return 0;
}

static int launch_fuseup(pf_handle* h, const Program& p, const PfFuseupOp& o, int B) {
    const PfTensorRec& ty = p.tens[o.y_t];
    const PfTensorRec& to = p.tens[o.out_t];
    FuseUpArgs a{};
    a.y = (const float*)p.tensor_ptr(o.y_t); a.out = (float*)p.tensor_ptr(o.out_t);
    a.B = B; a.H = ty.H; a.W = ty.W; a.Cs = ty.C; a.C = o.C; a.yLd = ty.ld; a.outLd = to.ld; a.act = o.act; a.nsrc = o.nsrc;
    if (a.nsrc < 1 || a.nsrc > 3 || to.H != ty.H || to.W != ty.W || to.C != ty.C || (ty.C & 3) || a.C > a.Cs) PF_FAIL(h, "fuseup: inconsistent shapes");
    int need = 0;
    for (int s = 0; s < a.nsrc; ++s) {
        const PfFuseupSrc& g = o.src[s];
        const PfTensorRec& ts = p.tens[g.src_t];
        a.src[s] = (const float*)p.tensor_ptr(g.src_t); a.wt[s] = (const float*)p.cptr(g.wt); a.bias[s] = (const float*)p.cptr(g.bias);
        a.shift[s] = g.shift; a.srcLd[s] = ts.ld; a.srcC[s] = ts.C;
        if (a.shift[s] < 1 || a.shift[s] > 3 || (ts.H << a.shift[s]) != ty.H || (ts.W << a.shift[s]) != ty.W || (ts.C & 3))
            PF_FAIL(h, "fuseup: source %d does not match the output", s);
        const int r = std::max(1, 16 >> a.shift[s]);
        need += ts.C * a.Cs + r * r * (ts.C + a.Cs);
    }
    ProfScope ps(h, "fuse_up");
    const int ntiles = B * pf_div_up(ty.H, 16) * pf_div_up(ty.W, 16);
    // (512-thread workgroups with y requested at the head of a tile and an 80 KB middle tier: 1.59 ms for the Teacher's 18
    // launches against 1.18 ms in this form, profiles/r04_run29 / r04_run30)
    if (need <= 12288) PF_LAUNCH((fuse_up_kernel<12288>), dim3(persistent_grid(ntiles, 3)), dim3(256), h->stream, a);        // 48 KB: three per CU
    else if (need <= 20480) PF_LAUNCH((fuse_up_kernel<20480>), dim3(persistent_grid(ntiles, 2)), dim3(256), h->stream, a);   // 80 KB: two
    else if (need <= 24576) PF_LAUNCH((fuse_up_kernel<24576>), dim3(persistent_grid(ntiles, 1)), dim3(256), h->stream, a);
    else PF_FAIL(h, "fuseup: %d floats of LDS needed", need);
    return 0;
}

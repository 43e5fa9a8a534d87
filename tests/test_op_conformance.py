"""Op-level conformance: one ProgramBuilder op at a time against torch on the CPU in float64, applied to the tensor the engine
itself produced upstream ("x": stem -> 1x1 conv to C channels), never against another engine launch.  This module: conv (every branch
of csrc/launch_landmark.inl launch_conv), dw (launch_layers.inl launch_dw), maxpool, copy, upcat, add_up;
tests/test_op_conformance_fused.py holds the pooled-vector ops, sepconv_up, the fused blocks and the arg-max ties.

Tolerance, per case, from the reference's own error: e32 = max|ref32 - ref64| / max|ref64| with ref32 the same torch op in float32 on
the same x.  Bound = max(4 e32, 8 * 2^-24) in f32s programs (split operands carry 22 significand bits against float32's 24) and
max(2 e32, 8 * 2^-24) in f32 programs and for the non-MFMA ops (summation order only).  Every case prints one "OPCONF" line with e32,
the bound and the engine's error (profiles/op_conformance_mi355x.txt is those lines from the MI355X).  The dispatch cases also assert
which kernel instance ran (Engine.launch_log).  The detector's det_* fusions are held to the same rule, at every tile production
picks, in tests/test_op_conformance_det.py.  Not covered here: f16 programs, mbx and front2 (they keep tests/test_fused_blocks.py
and test_emu_landmark.py)."""
import numpy as np
import pytest

from peppa_pig_face_landmark_amd.graph import ir

EPS_FLOOR = 8.0 * 2.0 ** -24
BIG = 261          # more faces than one round of 256 compute units


def torch_act(t, act):
    import torch
    import torch.nn.functional as F
    if act == "none":
        return t
    if act == "relu":
        return torch.relu(t)
    if act == "hswish":
        return t * F.relu6(t + 3.0) / 6.0
    if act == "silu":
        return t * torch.sigmoid(t)
    if act == "sigmoid":
        return torch.sigmoid(t)
    if act == "hsigmoid":
        return F.relu6(t + 3.0) / 6.0
    raise KeyError(act)


def base_program(dtype, h, w, c, rng, in_hw=None, x_act="none"):
    """stem -> 1x1 conv to c channels, named "x", on an h x w map (program input 2h x 2w unless ``in_hw`` gives it: odd inputs)."""
    ih, iw = in_hw if in_hw is not None else (2 * h, 2 * w)
    assert ((ih + 1) // 2, (iw + 1) // 2) == (h, w)
    pb = ir.ProgramBuilder(dtype, ih, iw, keep_all=True)
    f0 = pb.stem(rng.normal(0, 0.6, (16, 3, 3, 3)), rng.normal(0, 0.1, 16), "relu")
    x = pb.conv(f0, rng.normal(0, 0.35, (c, 16, 1, 1)), rng.normal(0, 0.2, c), x_act, out_name="x")
    return pb, x


def run_program(eng, pb, batch, rng, outs=None, crops=None):
    """Load, run on random u8 crops with the launch log on; returns (loc, score, launched kernel names)."""
    if outs is None:
        outs = [pb.buffer(196, ir.ELEM_F32, "loc"), pb.buffer(98, ir.ELEM_F32, "score")]
    blob = pb.finish(outs)
    eng.load_program(0, blob, batch)
    if crops is None:
        crops = rng.integers(0, 256, (batch, pb.in_h, pb.in_w, 3), dtype=np.uint8)
    eng.profile_enable(True)
    try:
        loc, score = eng.landmark_forward(crops)
        log = eng.launch_log()
    finally:
        eng.profile_enable(False)
    return loc, score, log


def read(eng, pb, t, batch, real=True):
    """Tensor `t` (id or name) as float64 [B,H,W,C]; with ``real`` the vector-padding channels are asserted zero and cut."""
    tid = pb.tensor_names[t] if isinstance(t, str) else t
    tt = pb.tensors[tid]
    a = eng.read_tensor(0, tid, batch, (tt.H, tt.W, tt.C))
    if real and tt.real_c < tt.C:
        assert not a[..., tt.real_c:].any(), "padding channels must be written as zeros"
        a = a[..., :tt.real_c]
    return a


def read_buffer(eng, pb, buf, batch):
    """A pooled f32 vector buffer [B, elems], through a 1 x 1 view over it (scalar reads: no vector-alignment requirement)."""
    n = pb.bufs[buf].elems
    return eng.read_tensor(0, buf_view(pb, buf), batch, (1, 1, n)).reshape(batch, n)


def buf_view(pb, buf):
    n = pb.bufs[buf].elems
    return pb.strided_view(buf, 1, 1, n, 0, n)


def nchw(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).double().numpy()


def assert_inputs_alive(x):
    """The comparison is not vacuous: finite, some negative inputs, every face non-zero."""
    assert np.isfinite(x).all() and (x < 0).any()
    assert (np.abs(x).reshape(x.shape[0], -1).max(1) > 0.05).all()


def check_close(tag, got, ref_fn, factor, ref_floor=0.1, eps_floor=EPS_FLOOR):
    """ref_fn(torch dtype) -> numpy float64 array shaped like `got`.  Prints the OPCONF line, then asserts the bound.
    ``eps_floor``: the bound's floor where a chain of stages has one of its own (tests/test_op_conformance_det.py)."""
    import torch
    ref64, ref32 = ref_fn(torch.float64), ref_fn(torch.float32)
    scale = np.abs(ref64).max()
    assert np.isfinite(ref64).all() and scale > ref_floor, (tag, scale)
    assert got.shape == ref64.shape, (tag, got.shape, ref64.shape)
    e32 = np.abs(ref32 - ref64).max() / scale
    bound = max(factor * e32, eps_floor)
    err = np.abs(got - ref64).max() / scale
    print("OPCONF %-58s e32 %.3e bound %.3e err %.3e ratio %.3f" % (tag, e32, bound, err, err / bound))
    assert np.isfinite(got).all() and err <= bound, (tag, err, bound)
    return err / bound


def assert_launched(log, want, tag=""):
    """`want`: a substring of the kernel instance the case was written for (str), or several."""
    for w in ([want] if isinstance(want, str) else want or []):
        assert any(w in k for k in log), "%s: kernel %r was not launched; launched: %s" % (tag, w, log)


def mfma_factor(dtype):
    return 4.0 if dtype == "f32s" else 2.0


# ---- conv ----------------------------------------------------------------------------------------------------------------------
CFG_TILES = {0: (128, 128, 2, 2), 1: (128, 64, 2, 2), 2: (256, 32, 4, 1), 3: (256, 16, 4, 1), 4: (128, 80, 4, 1), 5: (128, 96, 4, 1),
             6: (128, 112, 4, 1), 7: (256, 48, 4, 1)}


def generic_kernel(cfg, split, pointwise):
    """The name launch_conv's PF_CONV_CASE spells for tile configuration `cfg`."""
    bm, bn, wm, wn = CFG_TILES[cfg]
    ks = 1 if pointwise else 3
    if split:
        return "conv_gemm_split_kernel<%d, %d, 2 * %d, %d, %d>" % (bm, bn, wm, wn, ks)
    return "conv_gemm_kernel<T, %d, %d, %d, %d, %d>" % (bm, bn, wm, wn, ks)


def C(c, h, w, n, k=1, stride=1, pad=0, dil=1, act="none", res=False, cfg=-1, kern=None, in_hw=None, tag=""):
    return dict(c=c, h=h, w=w, n=n, k=k, stride=stride, pad=pad, dil=dil, act=act, res=res, cfg=cfg, kern=kern, in_hw=in_hw, tag=tag)


def conv_case(eng, dtype, case, batch, seed, where):
    import torch
    import torch.nn.functional as F
    c, h, w, n, k = case["c"], case["h"], case["w"], case["n"], case["k"]
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, h, w, c, rng, in_hw=case["in_hw"])
    wt = rng.normal(0, np.sqrt(2.0 / (k * k * c)), (n, c, k, k))
    b = rng.normal(0, 0.3, n)
    pb.conv(x, wt, b, case["act"], stride=case["stride"], pad=case["pad"], dil=case["dil"], res=x if case["res"] else -1, cfg=case["cfg"],
            out_name="y")
    _, _, log = run_program(eng, pb, batch, rng)
    xv = read(eng, pb, "x", batch)
    got = read(eng, pb, "y", batch)
    assert_inputs_alive(xv)
    kern = case["kern"]
    split = dtype == "f32s" and pb.conv_uses_split(c, k * k)
    if kern is None:          # generic tile configuration: the automatic choice by Npad, or the forced one
        npad = ir._round_up(n, 16)
        cfg = case["cfg"] if case["cfg"] >= 0 else {1: 3, 2: 2, 3: 7, 4: 1, 5: 4, 6: 5, 7: 6, 8: 0, 9: 7}[npad // 16]
        kern = generic_kernel(cfg, split, (k, case["stride"], case["pad"]) == (1, 1, 0))
    elif isinstance(kern, dict):
        kern = kern[dtype]
    tag = "conv %s %s c%d n%d k%d s%d p%d d%d %dx%d b%d %s%s" % (where, dtype, c, n, k, case["stride"], case["pad"], case["dil"], h, w, batch,
                                                                  case["act"], " +res" if case["res"] else "")
    assert_launched(log, kern, tag)

    def ref(dt):
        xt = nchw(xv, dt)
        y = F.conv2d(xt, torch.from_numpy(wt).to(dt), torch.from_numpy(b).to(dt), stride=case["stride"], padding=case["pad"], dilation=case["dil"])
        if case["res"]:
            y = y + xt
        return nhwc(torch_act(y, case["act"]))
    check_close(tag, got, ref, mfma_factor(dtype))


HALO = "conv3x3_halo_split_kernel<%s>"
# kernels by program dtype where the two differ: the LDS-resident 3x3 family and the unrolled pointwise loops are split-precision only
def _s(split_kernel, cfg, pointwise=False):
    return {"f32s": split_kernel, "f32": generic_kernel(cfg, False, pointwise)}


CONV_CASES = [
    # every tile configuration by Npad (cfg 3, 2, 7, 1, 4, 5, 6, 0), pointwise: split (64+ inputs) and, below, the direct kernel (Cin < 64)
    C(64, 8, 8, 16), C(64, 8, 8, 32, act="relu"), C(72, 8, 8, 48, act="hswish"), C(64, 8, 8, 64, act="silu"), C(96, 8, 8, 80, act="sigmoid"),
    C(64, 8, 8, 96, act="hsigmoid"), C(64, 8, 8, 112), C(80, 8, 8, 128, act="relu"),
    C(24, 8, 8, 16), C(40, 8, 8, 48, act="relu"), C(16, 8, 8, 96), C(32, 8, 8, 128, act="hswish"),
    # Npad 144: three 48-channel tiles;  160 outputs: the one-tile configuration 8 in split programs, two 80-channel tiles otherwise
    C(64, 8, 8, 144), C(128, 8, 8, 160, kern=_s("conv_gemm_split_kernel<128, 160, 4, 2, 1>", 4, True)),
    # each configuration forced through cfg= on a 32-output conv (several channel tiles or a mostly empty one)
    *[C(64, 9, 7, 32, cfg=g, act="relu") for g in range(8)],
    # the unrolled pointwise instances (NK = Cpad / 32 of 15 / 21 at 112 outputs, 21 / 30 at 160) and rolled neighbours
    C(480, 4, 8, 112, kern=_s("conv_gemm_split_kernel<128, 112, 8, 1, 1, 0, 0, 1, 0, 15>", 6, True)),
    C(672, 4, 8, 112, kern=_s("conv_gemm_split_kernel<128, 112, 8, 1, 1, 0, 0, 1, 0, 21>", 6, True)),
    C(672, 4, 8, 160, kern=_s("conv_gemm_split_kernel<128, 160, 4, 2, 1, 0, 0, 1, 0, 21>", 4, True)),
    C(960, 4, 8, 160, kern=_s("conv_gemm_split_kernel<128, 160, 4, 2, 1, 0, 0, 1, 0, 30>", 4, True)),
    C(512, 4, 8, 112), C(640, 4, 8, 160, kern=_s("conv_gemm_split_kernel<128, 160, 4, 2, 1>", 4, True)),
    # 3x3 s1 p1 with the input patch in LDS: Npad 32 / 48 / 64 / 80 / 128, H*W a multiple of 256 and of 128 only, widths 16 / 32 / 64
    C(18, 16, 16, 18, k=3, pad=1, act="relu", res=True, kern=_s(HALO % "32, 8, 1, 256", 2)),
    C(20, 8, 16, 32, k=3, pad=1, kern=_s(HALO % "32, 8, 1", 2)),
    C(36, 8, 32, 36, k=3, pad=1, act="relu", kern=_s(HALO % "48, 8, 1, 256", 7)),
    C(40, 12, 32, 48, k=3, pad=1, kern=_s(HALO % "48, 8, 1", 7)),
    C(64, 4, 64, 64, k=3, pad=1, act="relu", kern=_s(HALO % "64, 4, 2, 256", 1)),
    C(48, 6, 64, 56, k=3, pad=1, kern=_s(HALO % "64, 4, 2", 1)),
    C(72, 16, 16, 72, k=3, pad=1, act="relu", res=True, kern=_s(HALO % "80, 8, 1", 4)),
    C(72, 8, 16, 80, k=3, pad=1, kern=_s(HALO % "80, 8, 1", 4)),
    C(96, 12, 32, 128, k=3, pad=1, act="relu", kern=_s(HALO % "128, 4, 2", 0)),
    C(64, 16, 32, 64, k=3, pad=1, act="relu"),        # 64 outputs on a 32-wide map: outside the family, generic k x k
    # the hero kernel's guard must turn these away: 120 real input channels under Cpad 128, and 128 -> 128 on a 32-wide map
    C(120, 4, 64, 128, k=3, pad=1, act="relu", kern=_s(HALO % "128, 4, 2", 0)),
    C(128, 8, 32, 128, k=3, pad=1, act="relu", res=True, kern=_s(HALO % "128, 4, 2", 0)),
    # generic k x k: stride 2 on odd maps, 5x5, dilation 2, 1x1 with stride 2, rectangular maps with B*H*W not a multiple of 128,
    # N not a multiple of 16 (zero padding channels are asserted by read())
    C(24, 9, 7, 18, k=3, stride=2, pad=1, act="relu", in_hw=(17, 13)), C(64, 15, 11, 40, k=3, stride=2, pad=1),
    C(16, 9, 7, 24, k=5, pad=2, act="hswish"), C(32, 10, 6, 30, k=3, pad=2, dil=2, act="relu"), C(64, 7, 9, 64, k=3, pad=0),
    C(64, 9, 7, 50, stride=2, kern=_s("conv_gemm_split_kernel<128, 64, 2 * 2, 2, 3>", 1)), C(100, 5, 13, 100, act="relu", res=True),
]
# the hero shape itself, 128 -> 128 at 64 x 64 (csrc/k_hero.h)
HERO = C(128, 64, 64, 128, k=3, pad=1, act="relu", res=True, kern=_s("conv3x3_hero_kernel<4>", 0))


def _ids(cases):
    return ["%d-c%dn%dk%d-%dx%d%s" % (i, c["c"], c["n"], c["k"], c["h"], c["w"], ("-cfg%d" % c["cfg"]) if c["cfg"] >= 0 else "") for i, c in enumerate(cases)]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("case", CONV_CASES, ids=_ids(CONV_CASES))
def test_conv_emu(emu_engine, case, dtype):
    conv_case(emu_engine, dtype, case, 3, 1000 + CONV_CASES.index(case), "emu")


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
def test_conv_hero_emu(emu_engine, dtype):
    conv_case(emu_engine, dtype, HERO, 1, 1900, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("case", CONV_CASES, ids=_ids(CONV_CASES))
def test_conv_gpu(gpu_engine, case, dtype):
    i = CONV_CASES.index(case)
    conv_case(gpu_engine, dtype, case, 5, 2000 + i, "gpu")
    if case["h"] * case["w"] <= 512 and case["c"] <= 128:          # and more work than one round of the chip
        conv_case(gpu_engine, dtype, case, BIG, 2500 + i, "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,batch", [("f32s", 3), ("f32s", 66), ("f32", 2)])
def test_conv_hero_gpu(gpu_engine, dtype, batch):
    conv_case(gpu_engine, dtype, HERO, batch, 2900 + batch, "gpu")


def test_conv_cfg8_is_refused_in_f32_programs(emu_engine):
    """Tile configuration 8 (128 x 160) exists for split-precision pointwise convs only: an f32 program that forces it must fail
    with the engine's message, not run some other kernel."""
    from peppa_pig_face_landmark_amd._native import PeppaHipError
    rng = np.random.default_rng(7)
    pb, x = base_program("f32", 8, 8, 64, rng)
    pb.conv(x, rng.normal(0, 0.1, (160, 64, 1, 1)), np.zeros(160), "none", cfg=8)
    with pytest.raises(PeppaHipError, match="split-precision only"):
        run_program(emu_engine, pb, 1, rng)


def strided_conv_case(eng, dtype, batch, seed, where):
    """Two convs whose outputs interleave channel by channel (out_cs = 2) in one buffer through strided views: a channel shuffle."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    c, h, w, n = 64, 6, 10, 24
    pb, x = base_program(dtype, h, w, c, rng)
    buf = pb.buffer(h * w * 2 * n, ir.ELEM_ACT, "shuffled")
    ws = [rng.normal(0, np.sqrt(2.0 / c), (n, c, 1, 1)) for _ in range(2)]
    bs = [rng.normal(0, 0.3, n) for _ in range(2)]
    for j in range(2):
        pb.conv(x, ws[j], bs[j], "relu", out=pb.strided_view(buf, h, w, n, j, 2 * n), out_cs=2)
    whole = pb.view(buf, h, w, 2 * n, 0, 2 * n, name="y")
    run_program(eng, pb, batch, rng)
    xv, got = read(eng, pb, "x", batch), read(eng, pb, whole, batch)
    assert_inputs_alive(xv)

    def ref(dt):
        ys = [torch.relu(F.conv2d(nchw(xv, dt), torch.from_numpy(ws[j]).to(dt), torch.from_numpy(bs[j]).to(dt))) for j in range(2)]
        return nhwc(torch.stack(ys, 2).reshape(batch, 2 * n, h, w))
    check_close("conv %s %s out_cs=2 c%d n2x%d %dx%d b%d" % (where, dtype, c, n, h, w, batch), got, ref, mfma_factor(dtype))


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
def test_conv_strided_store_emu(emu_engine, dtype):
    strided_conv_case(emu_engine, dtype, 3, 3000, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("batch", [5, BIG])
def test_conv_strided_store_gpu(gpu_engine, dtype, batch):
    strided_conv_case(gpu_engine, dtype, batch, 3100 + batch, "gpu")


def gated_conv_case(eng, dtype, c, h, w, n, batch, seed, where, use_gate, use_fbias, res):
    """conv(gate_buf=, fbias_buf=): the SE gate on the input channels and the per-face bias both come from a gap -> fc chain in the
    same program; the reference computes the same gate / bias in float64 from x.  Also covers gap and fc at these shapes."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, h, w, c, rng)
    npad = ir._round_up(n, 16)
    pooled = pb.gap(x)
    wg, bg = rng.normal(0, 1.0 / np.sqrt(c) * 3, (c, c)), rng.normal(0, 0.3, c)
    wf, bf = rng.normal(0, 1.0 / np.sqrt(c) * 3, (npad, c)), rng.normal(0, 0.3, npad)
    gate = pb.fc(pooled, wg, bg, "hsigmoid") if use_gate else -1
    fb = pb.fc(pooled, wf, bf, "none") if use_fbias else -1
    wt, b = rng.normal(0, np.sqrt(2.0 / c), (n, c, 1, 1)), rng.normal(0, 0.3, n)
    pb.conv(x, wt, b, "none", gate_buf=gate, fbias_buf=fb, res=x if res else -1, out_name="y")
    run_program(eng, pb, batch, rng)
    xv, got = read(eng, pb, "x", batch), read(eng, pb, "y", batch)
    assert_inputs_alive(xv)

    def ref(dt):
        xt = nchw(xv, dt)
        p = xt.mean((2, 3))
        t = lambda a: torch.from_numpy(a).to(dt)
        xin = xt * torch_act(p @ t(wg).T + t(bg), "hsigmoid")[:, :, None, None] if use_gate else xt
        y = F.conv2d(xin, t(wt), t(b))
        if use_fbias:
            y = y + (p @ t(wf).T + t(bf))[:, :n, None, None]
        return nhwc(y + xt if res else y)
    check_close("conv %s %s c%d n%d %dx%d b%d%s%s%s" % (where, dtype, c, n, h, w, batch, " gate" if use_gate else "", " fbias" if use_fbias else "",
                                                        " +res" if res else ""), got, ref, mfma_factor(dtype))


GATED = [(96, 8, 8, 112, True, False, False), (64, 16, 8, 64, True, False, True), (128, 9, 7, 48, False, True, False),
         (72, 16, 16, 72, True, True, True), (24, 5, 9, 40, True, True, False)]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("c,h,w,n,g,f,res", GATED)
def test_conv_gate_and_face_bias_emu(emu_engine, dtype, c, h, w, n, g, f, res):
    gated_conv_case(emu_engine, dtype, c, h, w, n, 3, 3200 + c, "emu", g, f, res)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("c,h,w,n,g,f,res", GATED)
def test_conv_gate_and_face_bias_gpu(gpu_engine, dtype, c, h, w, n, g, f, res):
    for batch in (5, BIG):
        gated_conv_case(gpu_engine, dtype, c, h, w, n, batch, 3300 + c + batch, "gpu", g, f, res)


# ---- depthwise -----------------------------------------------------------------------------------------------------------------
def D(c, h, w, k, stride=1, pad=None, dil=1, act="relu", kern="dw_conv_kernel<T>"):
    return dict(c=c, h=h, w=w, k=k, stride=stride, pad=dil * (k - 1) // 2 if pad is None else pad, dil=dil, act=act, kern=kern)


TILED = "dw_conv_tiled_kernel<T, %s>"
DW_CASES = [
    D(16, 16, 16, 3, kern=TILED % "3, 1, 1, 4"), D(4, 9, 7, 3, act="none", kern=TILED % "3, 1, 1, 4"), D(960, 4, 5, 3, act="hswish", kern=TILED % "3, 1, 1, 4"),
    D(24, 9, 7, 3, stride=2, kern=TILED % "3, 2, 1, 4"), D(40, 10, 14, 3, stride=2, act="hswish", kern=TILED % "3, 2, 1, 4"),
    D(72, 8, 10, 5, kern=TILED % "5, 1, 1, 4"), D(20, 5, 3, 5, act="silu", kern=TILED % "5, 1, 1, 4"),
    D(48, 11, 9, 5, stride=2, kern=TILED % "5, 2, 1, 4"), D(96, 16, 12, 5, stride=2, act="hswish", kern=TILED % "5, 2, 1, 4"),
    D(32, 16, 16, 5, dil=2, kern=TILED % "5, 1, 2, 8"), D(112, 9, 13, 5, dil=2, act="hswish", kern=TILED % "5, 1, 2, 8"),
    D(8, 3, 21, 5, dil=2, act="none", kern=TILED % "5, 1, 2, 8"),
    # the fallback: 7 x 7, 3 x 3 with dilation 2;  pad 0 on the tiled kernels
    D(12, 9, 11, 7), D(36, 10, 6, 3, dil=2, act="sigmoid"), D(28, 8, 9, 7, stride=2, act="hsigmoid"),
    D(16, 9, 10, 3, pad=0, kern=TILED % "3, 1, 1, 4"), D(24, 11, 8, 5, pad=0, stride=2, act="none", kern=TILED % "5, 2, 1, 4"),
]


def dw_case(eng, dtype, case, batch, seed, where):
    import torch
    import torch.nn.functional as F
    c, h, w, k = case["c"], case["h"], case["w"], case["k"]
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, h, w, c, rng)
    wt, b = rng.normal(0, 1.5 / k, (c, 1, k, k)), rng.normal(0, 0.3, c)
    pb.dw(x, wt, b, case["act"], stride=case["stride"], pad=case["pad"], dil=case["dil"], out_name="y")
    _, _, log = run_program(eng, pb, batch, rng)
    xv, got = read(eng, pb, "x", batch), read(eng, pb, "y", batch)
    assert_inputs_alive(xv)
    tag = "dw %s %s c%d k%d s%d p%d d%d %dx%d b%d %s" % (where, dtype, c, k, case["stride"], case["pad"], case["dil"], h, w, batch, case["act"])
    assert_launched(log, case["kern"], tag)

    def ref(dt):
        y = F.conv2d(nchw(xv, dt), torch.from_numpy(wt).to(dt), torch.from_numpy(b).to(dt), stride=case["stride"], padding=case["pad"],
                     dilation=case["dil"], groups=c)
        return nhwc(torch_act(y, case["act"]))
    check_close(tag, got, ref, 2.0)


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("case", DW_CASES, ids=lambda d: "c%dk%ds%dd%dp%d-%dx%d" % (d["c"], d["k"], d["stride"], d["dil"], d["pad"], d["h"], d["w"]))
def test_dw_emu(emu_engine, case, dtype):
    dw_case(emu_engine, dtype, case, 2, 4000 + DW_CASES.index(case), "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("case", DW_CASES, ids=lambda d: "c%dk%ds%dd%dp%d-%dx%d" % (d["c"], d["k"], d["stride"], d["dil"], d["pad"], d["h"], d["w"]))
def test_dw_gpu(gpu_engine, case, dtype):
    i = DW_CASES.index(case)
    dw_case(gpu_engine, dtype, case, 5, 4100 + i, "gpu")
    if case["c"] <= 128:
        dw_case(gpu_engine, dtype, case, BIG, 4200 + i, "gpu")


# ---- max-pool, copy, upcat, add_up ---------------------------------------------------------------------------------------------
def pool_copy_case(eng, dtype, c, h, w, batch, seed, where):
    """maxpool (2 x 2 stride 2, ceil mode) and copy (out_cs 1 / 2, up 1 / 2) move values: bit-equal to the float64 reference."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, h, w, c, rng)
    cs = pb.tensors[x].C
    pb.maxpool(x, out_name="pool")
    plain = pb.tensor(2 * h, 2 * w, cs, name="up2")
    pb.copy(x, plain, out_cs=1, up=2)
    ibuf = pb.buffer(h * w * 2 * cs, ir.ELEM_ACT, "interleaved")
    pb.copy(x, pb.strided_view(ibuf, h, w, cs, 0, 2 * cs), out_cs=2, up=1)
    pb.copy(x, pb.strided_view(ibuf, h, w, cs, 1, 2 * cs), out_cs=2, up=1)
    iv = pb.view(ibuf, h, w, 2 * cs, 0, 2 * cs, name="shuf")
    ubuf = pb.buffer(4 * h * w * 2 * cs, ir.ELEM_ACT, "interleaved.up")
    pb.copy(x, pb.strided_view(ubuf, 2 * h, 2 * w, cs, 0, 2 * cs), out_cs=2, up=2)
    pb.copy(x, pb.strided_view(ubuf, 2 * h, 2 * w, cs, 1, 2 * cs), out_cs=2, up=2)
    uv = pb.view(ubuf, 2 * h, 2 * w, 2 * cs, 0, 2 * cs, name="shuf.up")
    _, _, log = run_program(eng, pb, batch, rng)
    assert_launched(log, ["maxpool2_kernel<T>", "copy_channels_kernel<T>"])
    xa = read(eng, pb, "x", batch, real=False)
    assert_inputs_alive(xa)
    xt = nchw(xa, torch.float64)
    pool = nhwc(F.max_pool2d(xt, 2, 2, ceil_mode=True)).astype(np.float32)
    assert pool.shape[1:3] == ((h + 1) // 2, (w + 1) // 2)
    assert np.array_equal(read(eng, pb, "pool", batch, real=False), pool)
    up = nhwc(F.interpolate(xt, scale_factor=2, mode="nearest")).astype(np.float32)
    assert np.array_equal(read(eng, pb, "up2", batch, real=False), up)
    assert np.array_equal(read(eng, pb, iv, batch), np.repeat(xa, 2, axis=3))
    assert np.array_equal(read(eng, pb, uv, batch), np.repeat(up, 2, axis=3))
    print("OPCONF %-58s bit-equal" % ("maxpool+copy %s %s c%d %dx%d b%d" % (where, dtype, c, h, w, batch)))


POOL = [(16, 9, 7), (24, 1, 13), (18, 8, 8), (64, 5, 1), (132, 3, 3)]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("c,h,w", POOL)
def test_maxpool_copy_emu(emu_engine, dtype, c, h, w):
    pool_copy_case(emu_engine, dtype, c, h, w, 3, 5000 + c, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("c,h,w", POOL)
def test_maxpool_copy_gpu(gpu_engine, dtype, c, h, w):
    for batch in (5, BIG):
        pool_copy_case(gpu_engine, dtype, c, h, w, batch, 5100 + c + batch, "gpu")


def upcat_addup_case(eng, dtype, c, c2, h, w, batch, seed, where):
    """upcat: cat(bilinear x2 of lo, skip) with lo = maxpool(x) ... ; add_up: act(a + nearest-upsampled b) for shift 1 - 3.  The low
    resolution operands are max-pools of x (h, w multiples of 8), read back and used as the reference's inputs."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, h, w, c, rng)
    lows = [x]
    for s in range(3):
        lows.append(pb.maxpool(lows[-1], out_name="low%d" % (s + 1)))
    skip = pb.conv(x, rng.normal(0, 0.2, (c2, c, 1, 1)), rng.normal(0, 0.3, c2), "none", out_name="skip")
    pb.upcat(lows[1], skip, out_name="upcat")
    acts = ["relu", "none", "hswish"]
    for s in (1, 2, 3):
        pb.add_up(x, lows[s], s, acts[s - 1], out_name="addup%d" % s)
    _, _, log = run_program(eng, pb, batch, rng)
    assert_launched(log, ["upsample_concat_kernel<T>", "add_upsample_kernel<T>"])
    xa = read(eng, pb, "x", batch, real=False)
    assert_inputs_alive(xa)
    lo = [xa] + [read(eng, pb, "low%d" % s, batch, real=False) for s in (1, 2, 3)]
    sk = read(eng, pb, "skip", batch, real=False)
    tag = "%s %s c%d+%d %dx%d b%d" % (where, dtype, c, c2, h, w, batch)

    def ref_upcat(dt):
        u = F.interpolate(nchw(lo[1], dt), scale_factor=2, mode="bilinear", align_corners=False)
        return nhwc(torch.cat([u, nchw(sk, dt)], 1))
    check_close("upcat " + tag, read(eng, pb, "upcat", batch, real=False), ref_upcat, 2.0)
    for s in (1, 2, 3):
        def ref_add(dt, s=s):
            u = F.interpolate(nchw(lo[s], dt), scale_factor=2 ** s, mode="nearest")
            return nhwc(torch_act(nchw(xa, dt) + u, acts[s - 1]))
        check_close("add_up shift %d %s " % (s, acts[s - 1]) + tag, read(eng, pb, "addup%d" % s, batch, real=False), ref_add, 2.0)


UPCAT = [(16, 8, 8, 8), (36, 20, 16, 24), (128, 64, 8, 16)]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("c,c2,h,w", UPCAT)
def test_upcat_addup_emu(emu_engine, dtype, c, c2, h, w):
    upcat_addup_case(emu_engine, dtype, c, c2, h, w, 2, 6000 + c, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("c,c2,h,w", UPCAT)
def test_upcat_addup_gpu(gpu_engine, dtype, c, c2, h, w):
    for batch in (5, BIG):
        upcat_addup_case(gpu_engine, dtype, c, c2, h, w, batch, 6100 + c + batch, "gpu")


# ---- launch log ----------------------------------------------------------------------------------------------------------------
def test_launch_log_exists_only_while_profiling(emu_engine):
    rng = np.random.default_rng(11)
    pb, x = base_program("f32s", 8, 8, 64, rng)
    pb.maxpool(x)
    blob = pb.finish([pb.buffer(196, ir.ELEM_F32, "loc"), pb.buffer(98, ir.ELEM_F32, "score")])
    emu_engine.load_program(0, blob, 1)
    crops = rng.integers(0, 256, (1, 16, 16, 3), dtype=np.uint8)
    emu_engine.landmark_forward(crops)
    assert emu_engine.launch_log() == []                 # profiling off: nothing is recorded
    emu_engine.profile_enable(True)
    emu_engine.landmark_forward(crops)
    log = emu_engine.launch_log()
    assert [k for k in log if "maxpool" in k] == ["(maxpool2_kernel<T>)"] and any("stem" in k for k in log), log
    emu_engine.landmark_forward(crops)
    assert emu_engine.launch_log() == log + log          # in launch order, accumulated until profiling is switched
    emu_engine.profile_enable(False)
    assert emu_engine.launch_log() == []

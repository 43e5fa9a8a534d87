"""Op-level conformance, second half (see tests/test_op_conformance.py for the method and the tolerance rule): the pooled-vector ops
(gap, fc, fc_pair, scse), sepconv_up on each of launch_sepup's routes, the fused blocks (mbconv, dsconv, expdw) against
expand -> depthwise -> project in float64, and the arg-max epilogue + hmdec on EXACT ties (the first index wins at
every reduction level)."""
import numpy as np
import pytest

from peppa_pig_face_landmark_amd.graph import ir
from tests.test_op_conformance import (BIG, assert_inputs_alive, assert_launched, base_program, buf_view, check_close, nchw, nhwc, read,
                                       run_program, torch_act)


def _t(a, dt):
    import torch
    return torch.from_numpy(np.asarray(a, np.float64)).to(dt)


def read_vec(eng, view, n, batch):
    return eng.read_tensor(0, view, batch, (1, 1, n)).reshape(batch, n).astype(np.float64)


# ---- gap, fc, fc_pair ----------------------------------------------------------------------------------------------------------
def fc_case(eng, dtype, k, n, batch, act, affine, seed, where):
    """gap -> fc (one launch): K above and below PF_FC_MAXK = 1024 (whole-K staging or K tiles), N off the 64-column tile, batches off
    the 8 faces of a workgroup."""
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, 3, 2, k, rng)
    pooled = pb.gap(x)
    w, b = rng.normal(0, 2.0 / np.sqrt(k), (n, k)), rng.normal(0, 0.3, n)
    s2, t2 = (rng.uniform(0.5, 1.5, n), rng.normal(0, 0.3, n)) if affine else (None, None)
    y = pb.fc(pooled, w, b, act, scale2=s2, shift2=t2, act2="relu" if affine else "none")
    vp, vy = buf_view(pb, pooled), buf_view(pb, y)
    _, _, log = run_program(eng, pb, batch, rng)
    assert_launched(log, ["gap_kernel<T>", "fc_kernel<true>" if k <= 1024 else "fc_kernel<false>"])
    xv = read(eng, pb, "x", batch, real=False)
    assert_inputs_alive(xv)
    tag = "%s %s k%d n%d b%d %s%s" % (where, dtype, k, n, batch, act, " affine" if affine else "")
    check_close("gap " + tag, read_vec(eng, vp, pb.bufs[pooled].elems, batch), lambda dt: nchw(xv, dt).mean((2, 3)).double().numpy(), 2.0, 0.02)

    def ref(dt):
        v = torch_act(nchw(xv, dt).mean((2, 3))[:, :k] @ _t(w, dt).T + _t(b, dt), act)
        return (torch_act(v * _t(s2, dt) + _t(t2, dt), "relu") if affine else v).double().numpy()
    check_close("fc " + tag, read_vec(eng, vy, n, batch), ref, 2.0)


FC = [(64, 24, "relu", False), (960, 240, "hswish", True), (1024, 70, "none", False), (1100, 130, "sigmoid", True), (20, 7, "hsigmoid", False)]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("k,n,act,affine", FC)
def test_gap_fc_emu(emu_engine, dtype, k, n, act, affine):
    fc_case(emu_engine, dtype, k, n, 11, act, affine, 7000 + k, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("k,n,act,affine", FC)
def test_gap_fc_gpu(gpu_engine, dtype, k, n, act, affine):
    for batch in (7, BIG):
        fc_case(gpu_engine, dtype, k, n, batch, act, affine, 7100 + k + batch, "gpu")


def fc_pair_case(eng, dtype, k, r, n, batch, affine, fuse, seed, where):
    """y = act2(W2 h + b2), h = act1b(scale2 * act1(W1 x + b1) + shift2): the fused PF_OP_FC2 (f32s programs) and the two-launch form."""
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, 2, 3, k, rng)
    pb.fuse_fc_pairs = fuse
    pooled = pb.gap(x)
    w1, b1 = rng.normal(0, 2.0 / np.sqrt(k), (r, k)), rng.normal(0, 0.3, r)
    w2, b2 = rng.normal(0, 2.0 / np.sqrt(r), (n, r)), rng.normal(0, 0.3, n)
    s2, t2 = (rng.uniform(0.5, 1.5, r), rng.normal(0, 0.3, r)) if affine else (None, None)
    fused = pb.fc_pair_fuses(k, r, n)
    assert fused == (fuse and dtype == "f32s" and r % 4 == 0 and n % 4 == 0 and k * r + r * n <= 131072)      # (larger pairs: two launches are faster)
    y = pb.fc_pair(pooled, w1, b1, "relu", w2, b2, "hsigmoid", scale2=s2, shift2=t2, act1b="hswish" if affine else "none")
    vy = buf_view(pb, y)
    _, _, log = run_program(eng, pb, batch, rng)
    assert_launched(log, "fc2_kernel" if fused else "fc_kernel<true>")
    assert fused or sum("fc_kernel" in q for q in log) == 2
    xv = read(eng, pb, "x", batch, real=False)
    assert_inputs_alive(xv)

    def ref(dt):
        h = torch_act(nchw(xv, dt).mean((2, 3))[:, :k] @ _t(w1, dt).T + _t(b1, dt), "relu")
        if affine:
            h = torch_act(h * _t(s2, dt) + _t(t2, dt), "hswish")
        return torch_act(h @ _t(w2, dt).T + _t(b2, dt), "hsigmoid").double().numpy()
    check_close("fc_pair %s %s %d-%d-%d b%d%s %s" % (where, dtype, k, r, n, batch, " affine" if affine else "", "fused" if fused else "2 launches"),
                read_vec(eng, vy, n, batch), ref, 2.0)


FCP = [(72, 24, 72, False, True), (480, 120, 480, True, True), (960, 240, 960, False, True), (96, 24, 96, True, False), (40, 10, 40, False, True),
       (256, 64, 132, True, True)]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("k,r,n,affine,fuse", FCP)
def test_fc_pair_emu(emu_engine, dtype, k, r, n, affine, fuse):
    fc_pair_case(emu_engine, dtype, k, r, n, 6, affine, fuse, 7200 + k, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("k,r,n,affine,fuse", FCP)
def test_fc_pair_gpu(gpu_engine, dtype, k, r, n, affine, fuse):
    for batch in (5, BIG):
        fc_pair_case(gpu_engine, dtype, k, r, n, batch, affine, fuse, 7300 + k + batch, "gpu")


# ---- scse ----------------------------------------------------------------------------------------------------------------------
def scse_case(eng, dtype, c, h, w, batch, parts, seed, where):
    """out = x * cse + x * sigmoid(<x, sse_w> + sse_b), cse = sigmoid(fc(gap(x))).  With gap_parts the per-32-pixel-tile channel sums must
    add up to the sums of the output that was read back, and an fc_pair(nparts=...) on them must equal one on the output's mean."""
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, h, w, c, rng)
    pooled = pb.gap(x)
    wg, bg = rng.normal(0, 2.0 / np.sqrt(c), (c, c)), rng.normal(0, 0.3, c)
    cse = pb.fc(pooled, wg, bg, "sigmoid")
    sw, sb = rng.normal(0, 2.0 / np.sqrt(c), c), 0.1
    vparts = vg = None
    if parts:
        assert pb.scse_can_sum(x)
        y, pbuf = pb.scse(x, cse, sw, sb, out_name="y", gap_parts=True)
        vparts = buf_view(pb, pbuf)
        if dtype == "f32s":         # partial sums as the input of the fused FC pair (the Student's decx8 pool)
            w1, b1, w2, b2 = rng.normal(0, 0.3, (24, c)), rng.normal(0, 0.1, 24), rng.normal(0, 0.3, (40, 24)), rng.normal(0, 0.1, 40)
            g = pb.fc_pair(pbuf, w1, b1, "relu", w2, b2, "none", nparts=h * w // ir.SCSE_TILE, xscale=1.0 / (h * w))
            vg = buf_view(pb, g)
    else:
        pb.scse(x, cse, sw, sb, out_name="y")
    _, _, log = run_program(eng, pb, batch, rng)
    assert_launched(log, "scse_tile_sum_kernel<T>" if parts else "scse_kernel<T>")
    xv, got = read(eng, pb, "x", batch, real=False), read(eng, pb, "y", batch, real=False)
    assert_inputs_alive(xv)
    tag = "%s %s c%d %dx%d b%d%s" % (where, dtype, c, h, w, batch, " +parts" if parts else "")

    def ref(dt):
        import torch
        xt = nchw(xv, dt)
        gate = torch.sigmoid(xt.mean((2, 3)) @ _t(wg, dt).T + _t(bg, dt))[:, :, None, None]
        sse = torch.sigmoid((xt * _t(sw, dt)[None, :, None, None]).sum(1, keepdim=True) + sb)
        return nhwc(xt * gate + xt * sse)
    check_close("scse " + tag, got, ref, 2.0)
    if parts:
        nt = h * w // ir.SCSE_TILE
        pv = read_vec(eng, vparts, nt * c, batch).reshape(batch, nt, c)
        tiles = got.astype(np.float64).reshape(batch, nt, ir.SCSE_TILE, c)
        check_close("scse tile sums " + tag, pv, lambda dt: np.asarray(_t(tiles, dt).sum(2).double()), 2.0)
        if vg is not None:
            def ref_g(dt):
                m = _t(got, dt).mean((1, 2))
                return (torch_act(m @ _t(w1, dt).T + _t(b1, dt), "relu") @ _t(w2, dt).T + _t(b2, dt)).double().numpy()
            check_close("fc_pair nparts=%d " % nt + tag, read_vec(eng, vg, 40, batch), ref_g, 2.0)


SCSE = [(4, 3, 5, False), (8, 4, 4, False), (16, 5, 3, False), (32, 8, 8, False), (64, 7, 9, False), (128, 4, 4, False), (256, 5, 7, False),
        (256, 8, 8, True), (256, 4, 24, True)]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("c,h,w,parts", SCSE)
def test_scse_emu(emu_engine, dtype, c, h, w, parts):
    scse_case(emu_engine, dtype, c, h, w, 3, parts, 7400 + c + h, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("c,h,w,parts", SCSE)
def test_scse_gpu(gpu_engine, dtype, c, h, w, parts):
    for batch in (5, BIG):
        scse_case(gpu_engine, dtype, c, h, w, batch, parts, 7500 + c + h + batch, "gpu")


# ---- sepconv_up ----------------------------------------------------------------------------------------------------------------
def sepup_case(eng, c1, c2, h, w, n, batch, kern, parts, seed, where):
    """cat(bilinear x2 of lo, skip) -> depthwise 3x3 (+bias) -> 1x1 (+bias) -> act; lo = maxpool of the 2h x 2w... map x, skip a 1x1 conv
    of it.  (h, w) is the OUTPUT map."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    pb, x = base_program("f32s", h, w, c1, rng)
    lo = pb.maxpool(x, out_name="lo")
    skip = pb.conv(x, rng.normal(0, 0.25, (c2, c1, 1, 1)), rng.normal(0, 0.3, c2), "none", out_name="skip")
    c = c1 + c2
    wd, bd = rng.normal(0, 0.5, (c, 1, 3, 3)), rng.normal(0, 0.2, c)
    wp, bp = rng.normal(0, np.sqrt(2.0 / c), (n, c, 1, 1)), rng.normal(0, 0.3, n)
    vparts = None
    if parts:
        assert pb.sepconv_up_can_sum(lo, skip, n)
        y, pbuf = pb.sepconv_up(lo, skip, wd, bd, wp, bp, "relu", out_name="y", gap_parts=True)
        vparts = buf_view(pb, pbuf)
    else:
        pb.sepconv_up(lo, skip, wd, bd, wp, bp, "relu", out_name="y")
    _, _, log = run_program(eng, pb, batch, rng)
    tag = "sepconv_up %s f32s c%d+%d n%d %dx%d b%d%s" % (where, c1, c2, n, h, w, batch, " +parts" if parts else "")
    assert_launched(log, kern, tag)
    lov, skv = read(eng, pb, "lo", batch, real=False), read(eng, pb, "skip", batch, real=False)
    got = read(eng, pb, "y", batch, real=False)
    assert not got[..., n:].any(), "padding channels must be written as zeros"
    got = got[..., :n]
    assert_inputs_alive(lov)
    assert_inputs_alive(skv)

    def ref(dt):
        u = F.interpolate(nchw(lov, dt), scale_factor=2, mode="bilinear", align_corners=False)
        t = F.conv2d(torch.cat([u, nchw(skv, dt)], 1), _t(wd, dt), _t(bd, dt), padding=1, groups=c)
        return nhwc(torch.relu(F.conv2d(t, _t(wp, dt), _t(bp, dt))))
    check_close(tag, got, ref, 4.0)
    if parts:
        nt = h * w // 128
        pv = read_vec(eng, vparts, nt * n, batch).reshape(batch, nt, n)
        tiles = got.astype(np.float64).reshape(batch, nt, 128, n)
        check_close("sepconv_up tile sums " + tag[11:], pv, lambda dt: np.asarray(_t(tiles, dt).sum(2).double()), 2.0)


PIPE128, PIPE256 = "sepup_pipe_kernel<128, %d,", "sepup_pipe_kernel<256, %d,"
SEPUP = [
    # (lo channels, skip channels, H, W, outputs, kernels): pipelined, 128 and 256 outputs, widths 16 / 32 / 64, skip <= 32 and in (32, 64]
    (64, 24, 16, 16, 128, [PIPE128 % 16, "sepup_skip_kernel<16, 32>"], False),
    (96, 40, 8, 32, 128, [PIPE128 % 32, "sepup_skip_kernel<32, 64>"], False),
    (32, 32, 6, 64, 128, [PIPE128 % 64, "sepup_skip_kernel<64, 32>"], False),
    (64, 64, 16, 16, 256, [PIPE256 % 16, "sepup_skip_kernel<16, 64>"], False),
    (160, 16, 8, 32, 256, [PIPE256 % 32, "sepup_skip_kernel<32, 32>"], True),
    (64, 48, 6, 64, 256, [PIPE256 % 64, "sepup_skip_kernel<64, 64>"], True),
    # patch kernels: more than 64 skip channels, N != Npad, one 128-pixel tile per face
    (64, 72, 16, 16, 128, "sepup_patch_kernel<128", False), (64, 32, 8, 32, 120, "sepup_patch_kernel<128", False),
    (96, 80, 8, 32, 256, "sepup_patch_kernel<256", False), (64, 16, 16, 16, 250, "sepup_patch_kernel<256", False),
    (64, 32, 8, 16, 128, "sepup_patch_kernel<128", False), (32, 32, 8, 16, 256, "sepup_patch_kernel<256", False),
    # generic fused-producer instances: a map that is not 16 / 32 / 64 wide, the minimum 6 x 6 map
    (64, 20, 12, 20, 100, "conv_gemm_split_kernel<128, 128, 4, 2, 1, 1>", False), (32, 36, 10, 24, 256, "conv_gemm_split_kernel<128, 256, 4, 2, 1, 1>", False),
    (64, 8, 6, 6, 128, "conv_gemm_split_kernel<128, 128, 4, 2, 1, 1>", False), (32, 40, 6, 6, 256, "conv_gemm_split_kernel<128, 256, 4, 2, 1, 1>", False),
]


@pytest.mark.parametrize("c1,c2,h,w,n,kern,parts", SEPUP)
def test_sepconv_up_emu(emu_engine, c1, c2, h, w, n, kern, parts):
    sepup_case(emu_engine, c1, c2, h, w, n, 2, kern, parts, 8000 + c1 + c2 + n, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("c1,c2,h,w,n,kern,parts", SEPUP)
def test_sepconv_up_gpu(gpu_engine, c1, c2, h, w, n, kern, parts):
    for batch in (5, 9, BIG):
        sepup_case(gpu_engine, c1, c2, h, w, n, batch, kern, parts, 8100 + c1 + c2 + n + batch, "gpu")


def test_sepconv_up_sums_need_two_k_steps(emu_engine):
    """with ONE K step (Cpad == 32) a fast wave of sepup_pipe_kernel could overwrite the tile sums in LDS before a slow wave
    has read the previous tile's.  No such program is ever built; both the packer's predicate and the launcher must say so."""
    from peppa_pig_face_landmark_amd._native import PeppaHipError
    rng = np.random.default_rng(5)
    pb, x = base_program("f32s", 16, 16, 64, rng)
    lo = pb.maxpool(x)
    skip = pb.conv(x, rng.normal(0, 0.25, (32, 64, 1, 1)), rng.normal(0, 0.3, 32), "none")
    assert pb.sepconv_up_can_sum(lo, skip, 256)
    assert not pb.sepconv_up_can_sum(pb.tensor(8, 8, 0, buf=pb.tensors[lo].buf, coff=0, ld=64), skip, 256)       # Cpad = 32: no low-res channels
    pb.sepconv_up(lo, skip, rng.normal(0, 0.5, (96, 1, 3, 3)), np.zeros(96), rng.normal(0, 0.1, (256, 96, 1, 1)), np.zeros(256), "relu", gap_parts=True)
    code, f, r, wr = pb.ops[-1]
    assert code == ir.OP_SEPUP
    f = list(f)
    f[ir.OP_LAYOUT[ir.OP_SEPUP].index("Cpad")] = 32          # the launcher sees a one-step request
    pb.ops[-1] = (code, f, r, wr)
    with pytest.raises(PeppaHipError, match="two K steps"):
        run_program(emu_engine, pb, 1, rng)


# ---- mbconv, dsconv, expdw -----------------------------------------------------------------------------------------------------
def _dw_weights(rng, c, k):
    return rng.normal(0, 1.5 / k, (c, 1, k, k)), rng.normal(0, 0.2, c)


def mbconv_case(eng, dtype, cin, mid, cout, stride, h, w, act, batch, kern, seed, where):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, h, w, cin, rng)
    assert pb.mbconv_supported(cin, 3, stride, 1, cout)
    we, be = rng.normal(0, np.sqrt(2.0 / cin), (mid, cin, 1, 1)), rng.normal(0, 0.2, mid)
    wd, bd = _dw_weights(rng, mid, 3)
    wp, bp = rng.normal(0, np.sqrt(1.0 / mid), (cout, mid, 1, 1)), rng.normal(0, 0.2, cout)
    res = stride == 1 and cin == cout
    pb.mbconv(x, we, be, wd, bd, wp, bp, act, stride=stride, pad=1, res=x if res else -1, out_name="y")
    _, _, log = run_program(eng, pb, batch, rng)
    tag = "mbconv %s %s %d-%d-%d s%d %dx%d b%d %s%s" % (where, dtype, cin, mid, cout, stride, h, w, batch, act, " +res" if res else "")
    assert_launched(log, kern[dtype] if isinstance(kern, dict) else kern, tag)
    xv, got = read(eng, pb, "x", batch), read(eng, pb, "y", batch)
    assert_inputs_alive(xv)

    def ref(dt):
        xt = nchw(xv, dt)
        t = torch_act(F.conv2d(xt, _t(we, dt), _t(be, dt)), act)
        t = torch_act(F.conv2d(t, _t(wd, dt), _t(bd, dt), stride=stride, padding=1, groups=mid), act)
        y = F.conv2d(t, _t(wp, dt), _t(bp, dt))
        return nhwc(y + xt if res else y)
    check_close(tag, got, ref, 4.0 if dtype == "f32s" else 2.0)


F32K = "mbconv_wave_f32_kernel<%s"
MBCONV = [
    # every entry of ProgramBuilder.MBCONV_KERNELS, at its edges: (Cin, Mid, Cout, stride, H, W, act, kernel)
    (16, 64, 24, 2, 9, 11, "relu", {"f32s": F32K % "2, 16, 4, 4, false, true, PF_ACT_RELU", "f32": F32K % "2, 16, 4, 4>"}),
    (8, 48, 32, 2, 16, 16, "hswish", {"f32s": F32K % "2, 16, 4, 4, false, true>", "f32": F32K % "2, 16, 4, 4>"}),
    (24, 72, 24, 1, 9, 11, "relu", {"f32s": F32K % "1, 32, 4, 8, false, true, PF_ACT_RELU", "f32": F32K % "1, 32, 4, 8>"}),
    (32, 96, 20, 1, 8, 16, "hswish", {"f32s": F32K % "1, 32, 4, 8, false, true>", "f32": F32K % "1, 32, 4, 8>"}),
    (40, 120, 80, 2, 9, 11, "hswish", "mbconv_wave_kernel<2, 2, 4, 4, 5, 4>"), (64, 200, 40, 2, 16, 16, "relu", "mbconv_wave_kernel<2, 2, 4, 4, 5, 4>"),
    (80, 184, 80, 1, 9, 11, "hswish", "mbconv_wave_kernel<1, 3, 4, 8, 5, 4>"), (96, 240, 72, 1, 8, 16, "relu", "mbconv_wave_kernel<1, 3, 4, 8, 5, 4>"),
]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("cin,mid,cout,stride,h,w,act,kern", MBCONV)
def test_mbconv_emu(emu_engine, dtype, cin, mid, cout, stride, h, w, act, kern):
    mbconv_case(emu_engine, dtype, cin, mid, cout, stride, h, w, act, 2, kern, 9000 + cin, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("cin,mid,cout,stride,h,w,act,kern", MBCONV)
def test_mbconv_gpu(gpu_engine, dtype, cin, mid, cout, stride, h, w, act, kern):
    for batch in (5, BIG):
        mbconv_case(gpu_engine, dtype, cin, mid, cout, stride, h, w, act, batch, kern, 9100 + cin + batch, "gpu")


def dsconv_case(eng, dtype, cout, h, w, act, res, batch, seed, where):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    pb, x = base_program(dtype, h, w, 16, rng)
    assert pb.dsconv_supported(16, 3, 1, 1, cout)
    wd, bd = _dw_weights(rng, 16, 3)
    wp, bp = rng.normal(0, 0.3, (cout, 16, 1, 1)), rng.normal(0, 0.2, cout)
    pb.dsconv(x, wd, bd, wp, bp, act, res=x if res else -1, out_name="y")
    _, _, log = run_program(eng, pb, batch, rng)
    assert_launched(log, "mbconv_wave_f32_kernel<1, 16, 4, 8, true" + (", false, PF_ACT_RELU>" if act == "relu" else ">"))
    xv, got = read(eng, pb, "x", batch), read(eng, pb, "y", batch)
    assert_inputs_alive(xv)

    def ref(dt):
        xt = nchw(xv, dt)
        y = F.conv2d(torch_act(F.conv2d(xt, _t(wd, dt), _t(bd, dt), padding=1, groups=16), act), _t(wp, dt), _t(bp, dt))
        return nhwc(y + xt if res else y)
    check_close("dsconv %s %s 16-%d %dx%d b%d %s%s" % (where, dtype, cout, h, w, batch, act, " +res" if res else ""), got, ref, 2.0)


DSCONV = [(16, 9, 11, "relu", True), (32, 8, 16, "hswish", False), (4, 5, 3, "relu", False), (28, 16, 16, "hswish", False)]


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("cout,h,w,act,res", DSCONV)
def test_dsconv_emu(emu_engine, dtype, cout, h, w, act, res):
    dsconv_case(emu_engine, dtype, cout, h, w, act, res, 2, 9200 + cout, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32s", "f32"])
@pytest.mark.parametrize("cout,h,w,act,res", DSCONV)
def test_dsconv_gpu(gpu_engine, dtype, cout, h, w, act, res):
    for batch in (5, BIG):
        dsconv_case(gpu_engine, dtype, cout, h, w, act, res, batch, 9300 + cout + batch, "gpu")


def expdw_case(eng, cin, mid, h, w, k, dil, stride, act, batch, kern, seed, where):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    pb, x = base_program("f32s", h, w, cin, rng)
    pad = dil * (k - 1) // 2
    assert pb.expdw_supported(h, w, k, stride, pad, dil, cin)
    we, be = rng.normal(0, np.sqrt(2.0 / cin), (mid, cin, 1, 1)), rng.normal(0, 0.2, mid)
    wd, bd = _dw_weights(rng, mid, k)
    y, gap = pb.expdw(x, we, be, wd, bd, act, pad=pad, dil=dil, stride=stride, want_gap=True, out_name="y")
    vg = buf_view(pb, gap)
    _, _, log = run_program(eng, pb, batch, rng)
    tag = "expdw %s f32s %d-%d k%d d%d s%d %dx%d b%d %s" % (where, cin, mid, k, dil, stride, h, w, batch, act)
    assert_launched(log, kern, tag)
    xv, got = read(eng, pb, "x", batch), read(eng, pb, "y", batch)
    assert_inputs_alive(xv)

    def ref(dt):
        t = torch_act(F.conv2d(nchw(xv, dt), _t(we, dt), _t(be, dt)), act)
        return nhwc(torch_act(F.conv2d(t, _t(wd, dt), _t(bd, dt), stride=stride, padding=pad, dilation=dil, groups=mid), act))
    check_close(tag, got, ref, 4.0)
    check_close("expdw means " + tag[6:], read_vec(eng, vg, mid, batch), lambda dt: np.asarray(_t(got, dt).mean((1, 2)).double()), 2.0, 0.02)


GEMM_DW = "conv_gemm_split_kernel<256, 64, 8, 1, 1, 0, %s>"
EXPDW = [
    # every shape family expdw_supported accepts: (Cin, Mid, H, W, k, dil, stride, act, kernel)
    (16, 64, 64, 64, 5, 1, 2, "relu", "expdw_image_s2_kernel<5, PF_ACT_RELU>"), (32, 72, 64, 64, 5, 1, 2, "hswish", "expdw_image_s2_kernel<5>"),
    (24, 72, 32, 32, 3, 1, 1, "relu", "expdw_image_kernel<3, 1>"), (40, 120, 32, 32, 5, 1, 1, "relu", "expdw_image_kernel<5, 1, PF_ACT_RELU>"),
    (64, 100, 32, 32, 5, 1, 1, "hswish", "expdw_image_kernel<5, 1>"),
    (80, 200, 16, 16, 3, 1, 1, "hswish", GEMM_DW % "3, 1, 16"), (112, 480, 16, 16, 5, 1, 1, "hswish", GEMM_DW % "5, 1, 16"),
    (160, 320, 16, 16, 5, 2, 1, "relu", GEMM_DW % "5, 2, 16"),
    (40, 96, 8, 8, 3, 1, 1, "relu", GEMM_DW % "3, 1"), (72, 132, 8, 16, 5, 1, 1, "hswish", GEMM_DW % "5, 1"), (96, 64, 16, 8, 5, 2, 1, "relu", GEMM_DW % "5, 2"),
    (36, 68, 16, 4, 3, 1, 1, "relu", GEMM_DW % "3, 1"),
]


@pytest.mark.parametrize("cin,mid,h,w,k,dil,stride,act,kern", EXPDW)
def test_expdw_emu(emu_engine, cin, mid, h, w, k, dil, stride, act, kern):
    expdw_case(emu_engine, cin, mid, h, w, k, dil, stride, act, 2, kern, 9400 + cin, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("cin,mid,h,w,k,dil,stride,act,kern", EXPDW)
def test_expdw_gpu(gpu_engine, cin, mid, h, w, k, dil, stride, act, kern):
    for batch in (5, BIG) if h * w <= 256 else (5, 33):
        expdw_case(gpu_engine, cin, mid, h, w, k, dil, stride, act, batch, kern, 9500 + cin + batch, "gpu")


def _refused(eng, pb, rng, match):
    from peppa_pig_face_landmark_amd._native import PeppaHipError
    with pytest.raises(PeppaHipError, match=match):
        run_program(eng, pb, 1, rng)


def test_fused_blocks_outside_their_predicates_are_refused(emu_engine):
    """A shape just outside each *_supported predicate: the predicate says no, and a program packed anyway fails with the engine's
    message instead of running some kernel."""
    rng = np.random.default_rng(3)
    # mbconv: 104 input channels at stride 1 (four K steps; the stride-1 kernel has three)
    pb, x = base_program("f32s", 8, 8, 104, rng)
    assert not pb.mbconv_supported(104, 3, 1, 1, 40) and not pb.mbconv_supported(96, 3, 1, 1, 96) and not pb.mbconv_supported(96, 5, 1, 1, 40)
    pb.mbconv_supported = lambda *a, **k: True
    pb.mbconv(x, rng.normal(0, 0.1, (128, 104, 1, 1)), np.zeros(128), *_dw_weights(rng, 128, 3), rng.normal(0, 0.1, (40, 128, 1, 1)), np.zeros(40), "relu",
              stride=1, pad=1)
    _refused(emu_engine, pb, rng, "mbconv: no kernel for stride 1, 104 input channels")
    # dsconv: 36 outputs (the kernel holds 32)
    pb, x = base_program("f32s", 8, 8, 16, rng)
    assert not pb.dsconv_supported(16, 3, 1, 1, 36) and not pb.dsconv_supported(24, 3, 1, 1, 32) and not pb.dsconv_supported(16, 3, 2, 1, 32)
    pb.dsconv_supported = lambda *a, **k: True
    pb.dsconv(x, *_dw_weights(rng, 16, 3), rng.normal(0, 0.3, (36, 16, 1, 1)), np.zeros(36), "relu")
    _refused(emu_engine, pb, rng, "dsconv: unsupported block shape")
    # expdw: a 12 x 12 map (144 pixels do not divide the 256-pixel tile), and f32 programs
    pb, x = base_program("f32s", 12, 12, 64, rng)
    assert not pb.expdw_supported(12, 12, 3, 1, 1, 1, 64) and not pb.expdw_supported(16, 16, 3, 2, 1, 1, 64) and not pb.expdw_supported(32, 32, 5, 1, 4, 2, 64)
    pb.expdw_supported = lambda *a, **k: True
    pb.expdw(x, rng.normal(0, 0.1, (64, 64, 1, 1)), np.zeros(64), *_dw_weights(rng, 64, 3), "relu", pad=1)
    _refused(emu_engine, pb, rng, "expdw: unsupported shape")
    pb, x = base_program("f32", 16, 16, 64, rng)
    assert not pb.expdw_supported(16, 16, 3, 1, 1, 1, 64)
    pb.expdw_supported = lambda *a, **k: True
    pb.expdw(x, rng.normal(0, 0.1, (64, 64, 1, 1)), np.zeros(64), *_dw_weights(rng, 64, 3), "relu", pad=1)
    _refused(emu_engine, pb, rng, "needs a split-precision")


# ---- arg-max epilogue + hmdec on exact ties ------------------------------------------------------------------------------------
P = 98
PW_HEAD = "pw_head_kernel<4>"
AMAX_NK4 = "conv_gemm_split_kernel<128, 128, 4, 2, 1, 0, -1, 1, 0, 4>"
AMAX_ROLLED = "conv_gemm_split_kernel<128, 128, 4, 2, 1, 0, -1>"
AMAX_F32 = "conv_gemm_kernel<T, 128, 128, 2, 2, 1>"


def head_program(dtype, h, w, c, rng, hw_, hb_):
    """x (c channels, h x w) -> conv(amax=..., store_out=False, cfg=0) -> hmdec with zero offset weights, 98 points."""
    pb, x = base_program(dtype, h, w, c, rng)
    bm, _, warps_m = ir.CONV_CFGS[0]
    if pb.conv_uses_split(c):
        warps_m *= 2
    assert (h * w) % bm == 0
    nslots = (h * w // bm) * warps_m
    val, idx = pb.buffer(P * nslots, ir.ELEM_F32, "amax_val"), pb.buffer(P * nslots, ir.ELEM_I32, "amax_idx")
    dummy = pb.tensor(h, w, ir._round_up(P, pb.ve), buf=pb.buffer(pb.ve, ir.ELEM_ACT, "hm.unused"), coff=0, ld=ir._round_up(P, pb.ve))
    pb.conv(x, hw_, hb_, "none", out=dummy, amax=(val, idx, P), store_out=False, cfg=0)
    loc, score = pb.hmdec(val, idx, x, np.zeros((2 * P, pb.tensors[x].C)), np.zeros(2 * P), P, nslots)
    return pb, [loc, score]


def all_tie_case(eng, dtype, h, w, c, batch, kern, seed):
    """Head weights all zero, distinct biases: EVERY pixel ties, every landmark must decode to pixel 0 and score == its bias."""
    rng = np.random.default_rng(seed)
    hb_ = rng.permutation(P) * 0.25 - 7.0
    pb, outs = head_program(dtype, h, w, c, rng, np.zeros((P, c, 1, 1)), hb_)
    loc, score, log = run_program(eng, pb, batch, rng, outs=outs)
    assert_launched(log, [kern, "hm_decode_kernel<T>"], "all-tie %s %dx%d c%d b%d" % (dtype, h, w, c, batch))
    assert np.array_equal(score, np.broadcast_to(hb_.astype(np.float32), (batch, P)))
    assert np.array_equal(loc, np.zeros((batch, 2 * P), np.float32)), np.argwhere(loc != 0)[:8]


def class_tie_case(eng, dtype, h, w, c, batch, kern, seed, where):
    """One constant image per face: all interior pixels of x carry bit-identical features (the stem's zero padding sets the first row and
    column apart), so every heat map attains its maximum on a whole class of pixels.  Expected index = first pixel of the maximal
    class of the float64 heat map of x, for the landmarks whose class-to-class margin in float64 exceeds 1e-3 (at most 10 % dropped)."""
    rng = np.random.default_rng(seed)
    hw_, hb_ = rng.normal(0, 1.0 / np.sqrt(c), (P, c, 1, 1)), rng.normal(0, 0.5, P)
    pb, outs = head_program(dtype, h, w, c, rng, hw_, hb_)
    crops = np.broadcast_to(rng.integers(30, 256, (batch, 1, 1, 3), dtype=np.uint8), (batch, 2 * h, 2 * w, 3)).copy()
    loc, score, log = run_program(eng, pb, batch, rng, outs=outs, crops=crops)
    tag = "arg-max ties %s %s c%d %dx%d b%d" % (where, dtype, c, h, w, batch)
    assert_launched(log, [kern, "hm_decode_kernel<T>"], tag)
    xv = read(eng, pb, "x", batch).reshape(batch, h * w, c)
    assert_inputs_alive(xv)
    want, ok, ref_score = np.zeros((batch, P), np.int64), np.zeros((batch, P), bool), np.zeros((batch, P))
    for b in range(batch):
        feats, first, inv = np.unique(xv[b], axis=0, return_index=True, return_inverse=True)
        assert len(feats) <= 9 and np.bincount(inv.reshape(-1)).max() >= (h - 2) * (w - 2)      # a handful of classes, one of them the interior
        heat = feats.astype(np.float64) @ hw_.reshape(P, c).T + hb_            # [classes][P]
        order = np.sort(heat, axis=0)
        top = heat.argmax(0)
        want[b], ref_score[b] = first[top], order[-1]
        ok[b] = order[-1] - order[-2] > 1e-3
    assert ok.mean() >= 0.9, "the float64 reference itself leaves %.1f %% of the landmarks decided" % (100 * ok.mean())
    got = np.rint(loc.reshape(batch, P, 2)[..., 1] * h).astype(np.int64) * w + np.rint(loc.reshape(batch, P, 2)[..., 0] * w).astype(np.int64)
    bad = np.argwhere((got != want) & ok)
    assert not len(bad), "%s: %d landmarks decode to another pixel than the first of the maximal class, e.g. (face, point) %s got %s want %s" % (
        tag, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    err = np.abs(score - ref_score)[ok].max() / np.abs(ref_score).max()
    print("OPCONF %-58s indices exact on %d/%d, score err %.3e" % (tag, ok.sum(), ok.size, err))
    assert err < 1e-5


# (dtype, H, W, channels of x, kernel): pw_head_kernel, the two generic fallbacks (Cpad != 128; Cpad == 128 with 120 real channels), f32
HEADS = [("f32s", 16, 8, 128, PW_HEAD), ("f32s", 32, 32, 128, PW_HEAD), ("f32s", 64, 64, 128, PW_HEAD),
         ("f32s", 16, 16, 96, AMAX_ROLLED), ("f32s", 16, 16, 120, AMAX_NK4), ("f32", 16, 16, 128, AMAX_F32), ("f32", 32, 8, 40, AMAX_F32)]


@pytest.mark.parametrize("dtype,h,w,c,kern", HEADS)
def test_argmax_all_pixels_tie_emu(emu_engine, dtype, h, w, c, kern):
    # 32 x 32 (8 tiles per face) with the emulator's fill of 8 work items: batches 1 / 2 / 4 / 8 give head_segs 8 / 4 / 2 / 1, 11 the cost model
    for batch in ((1, 2, 4, 8, 11) if (h, w) == (32, 32) else (1, 3)):
        all_tie_case(emu_engine, dtype, h, w, c, batch, kern, 9600 + h + c + batch)


@pytest.mark.parametrize("dtype,h,w,c,kern", HEADS)
def test_argmax_class_ties_emu(emu_engine, dtype, h, w, c, kern):
    for batch in ((2, 4, 11) if (h, w) == (32, 32) else (3,)):
        class_tie_case(emu_engine, dtype, h, w, c, batch, kern, 9700 + h + c + batch, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,h,w,c,kern", HEADS)
def test_argmax_all_pixels_tie_gpu(gpu_engine, dtype, h, w, c, kern):
    # below / at / above one and two rounds of the 256 compute units
    batches = (3, 255, 256, 257, 511, 512, 513) if h * w <= 256 else ((5, 31, 32, 33, 255, 257) if h * w == 1024 else (1, 7, 9, 63, 65))
    for batch in batches:
        all_tie_case(gpu_engine, dtype, h, w, c, batch, kern, 9800 + h + c + batch)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,h,w,c,kern", HEADS)
def test_argmax_class_ties_gpu(gpu_engine, dtype, h, w, c, kern):
    batches = (3, 255, 257, 513) if h * w <= 256 else ((5, 33, 257) if h * w == 1024 else (1, 9, 65))
    for batch in batches:
        class_tie_case(gpu_engine, dtype, h, w, c, batch, kern, 9900 + h + c + batch, "gpu")

"""Op-level conformance of the detector's workgroup-level fusions (csrc/k_det.h): det_unit_kernel (six instances), det_c3_kernel (two)
and det_stem_kernel (two), each alone in its own f32s program with random BN-folded weights, against plain torch (F.conv2d, SiLU,
shuffle, nearest upsample, cat) in float64 and float32 -- the method of tests/test_op_conformance.py: the op's input is the tensor the
engine itself produced upstream (stem -> 1x1 conv), read back; nothing is compared with another engine launch.

Tiles.  These kernels take their output tile TH x TW at run time; production (384 x 640, B = 1 .. 32, 256 compute units) runs 9 to 30
different tiles per instance (tests/det_tiles.py restates the picker; test_every_production_tile_has_a_forced_case asserts the table
here holds them all).  Every such tile is forced (PF_OPT_DET_TILE) on a map of H = 2 TH + r, W = 2 TW + q with 1 <= r < TH,
1 <= q < TW (three rows / columns where TH / TW is 1): border, interior and ragged tiles both ways, B = 2 with different frames, at
most 33 x 33 pixels.  Sources nearest-upsampled by the kernel (det_c3's upA) have even maps by construction: there r and q are even
(2, or full tiles where TH / TW <= 2 -- an even map never leaves such a tile ragged in production either).  The automatic cases run
with the option at 0 and assert the logged tile equals det_tiles.pick().

Views.  Inputs and outputs are channel slices of wider buffers (ld > C, coff = 16, like the PAN head's concat slices); output buffers
are filled beforehand by a zero-weight conv whose bias is 1000 + channel, and the channels next to the slice must still hold exactly
that afterwards.  The rows buffer of the detect tail is filled the same way (-7 - k) and rows outside [row0, row0 + 3 H W) must keep it.

Tolerance, per case: bound = max(4 e32, (8 + 4 n_silu) 2^-24) with e32 the float32 reference's own error over the whole fused chain
(split operands: the rule of test_op_conformance.py) and n_silu the SiLU / sigmoid stages in the chain -- on the GPU det_silu is
v_exp_f32 + v_rcp_f32 (1 ulp each) + two roundings, at most 4 ulp per stage that float32 torch does not have; the emulator's libm
SiLU needs no more.  Every half / output / column group is scaled by its own maximum.  profiles/op_conformance_det_mi355x.txt is the
OPCONF lines of the MI355X.

Tiers.  The GPU tier runs every case.  The emulator tier runs, per instance, the smallest tile, the tile with the largest region, one
with TH TW a multiple of 16 and one without, one with an odd count of 16-row GEMM tiles, the automatic cases and every det_stem case
(EMU_TILES); PF_EMU_POISON stays active in that build, so no case can lean on zeroed LDS.  The other forced tiles would join it only
while this module's CPU time stays below that of tests/test_op_conformance.py's emulator cases; measured when this module was
added, that module takes 24 s (94 s of CPU time), this one 23 s (121 s) as it is and 42 s (230 s) with every forced tile -- all 163 pass
there -- so they stay on the GPU tier (EMU_ALL_FORCED)."""
import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd.graph import ir
from peppa_pig_face_landmark_amd.graph.detector import ANCHORS, STRIDES
from tests import det_tiles
from tests.test_op_conformance import assert_inputs_alive, assert_launched, buf_view, check_close, nchw, nhwc

ULP = 2.0 ** -24
PRODUCTION = det_tiles.production_tiles()
# the forced-tile case table: every (instance, TH, TW) production picks; test_every_production_tile_has_a_forced_case recomputes it
FORCED = [(inst, th, tw) for inst in sorted(PRODUCTION) for th, tw in PRODUCTION[inst]]
UNIT_FORCED = [c for c in FORCED if c[0][0] == "unit"]
C3_FORCED = [c for c in FORCED if c[0][0] == "c3"]


def floor_for(n_silu):
    return (8 + 4 * n_silu) * ULP


def tile_rows(inst, th, tw):
    return det_tiles.region_rows(th, tw, det_tiles.INSTANCES[inst][0])


def emu_tiles(inst):
    """The emulator tier's tiles of an instance (see the module docstring), chosen by rule from the production tiles."""
    tiles = PRODUCTION[inst]
    by_region = sorted(tiles, key=lambda t: (tile_rows(inst, *t), t))
    pick = [by_region[0], by_region[-1]]
    pick.append(next(t for t in by_region if (t[0] * t[1]) % 16 == 0))
    pick.append(next(t for t in by_region[1:] if (t[0] * t[1]) % 16 != 0))
    pick.append(next(t for t in by_region[1:] if ((tile_rows(inst, *t) + 15) // 16) % 2 == 1))
    return sorted(set(pick))


EMU_TILES = {inst: emu_tiles(inst) for inst in PRODUCTION}
EMU_ALL_FORCED = False      # True: the emulator tier also runs the remaining forced tiles (see "Tiers" for why it does not)


def map_for(th, tw, even=False):
    """H = 2 TH + r, W = 2 TW + q (module docstring); r, q vary with the tile, at most 33 x 33."""
    def side(t, other):
        if t == 1:
            return 4 if even else 3
        if even:
            assert t < 16, "an even map over a 16-wide tile would pass 33 pixels"
            return 2 * t + 2
        return 2 * t + (1 + other % 2 if 3 <= t < 16 else 1)
    return side(th, tw), side(tw, th)


def case_id(c):
    inst, th, tw = c
    return "%s-%dx%d" % ("_".join(str(v) for v in inst), th, tw)


def silu(t):
    import torch
    return t * torch.sigmoid(t)


def run_det_program(eng, pb, batch, crops, tile, slot=0):
    """Load, force `tile` ((TH, TW), or None: the engine picks), run with the launch log on; returns the log."""
    if not hasattr(pb, "det_blob"):
        pb.det_blob = pb.finish([pb.buffer(196, ir.ELEM_F32, "loc"), pb.buffer(98, ir.ELEM_F32, "score")])
    eng.load_program(slot, pb.det_blob, batch)
    eng.set_option(_native.PF_OPT_DET_TILE, _native.det_tile_option(*tile) if tile else 0)
    eng.profile_enable(True)
    try:
        eng.landmark_forward(crops[:batch])
        return eng.launch_log()
    finally:
        eng.profile_enable(False)


def rd(eng, pb, name, batch, slot=0):
    tt = pb.tensors[pb.tensor_names[name]]
    return eng.read_tensor(slot, pb.tensor_names[name], batch, (tt.H, tt.W, tt.C))


def device_cus(where):
    if where == "emu":
        return 256          # tests/simt_emu: the emulated device reports 256 compute units
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_tile(log, inst, want, out_hw, batch, tag):
    """The instance ran, once, with tile `want`, and the note's tiles-per-frame and grid follow from it."""
    assert_launched(log, det_tiles.kernel_name(inst), tag)
    runs = det_tiles.logged_tiles(log, inst)
    assert len(runs) == 1, (tag, log)
    _, th, tw, tpf, grid = runs[0]
    assert (th, tw) == tuple(want), "%s: ran tile %dx%d, expected %dx%d" % (tag, th, tw, want[0], want[1])
    assert tpf == -(-out_hw[0] // th) * -(-out_hw[1] // tw) and grid == tpf * batch, (tag, runs[0])


def prefill(pb, src, ld, base, name, stride=1):
    """A `ld`-channel tensor at src's resolution (/ stride) holding exactly base + channel: zero weights, bias only."""
    bias = base + np.arange(ld, dtype=np.float64) if base >= 0 else base - np.arange(ld, dtype=np.float64)
    t = pb.conv(src, np.zeros((ld, 16, 1, 1)), bias, "none", stride=stride, out_name=name)
    return t, bias.astype(np.float32)


def assert_neighbours(tag, wide, bias, lo, hi):
    """Channels outside [lo, hi) of a prefilled buffer are untouched, bit for bit."""
    keep = np.r_[0:lo, hi:wide.shape[-1]]
    assert np.array_equal(wide[..., keep], np.broadcast_to(bias[keep], wide[..., keep].shape)), tag + ": channels next to the slice were written"


# ---- det_unit ------------------------------------------------------------------------------------------------------------------
def unit_weights(rng, c, cin, s):
    cin2 = c if s == 1 else cin
    w = dict(w1=rng.normal(0, np.sqrt(2.0 / cin2), (c, cin2, 1, 1)), b1=rng.normal(0, 0.3, c), wd=rng.normal(0, 0.5, (c, 1, 3, 3)), bd=rng.normal(0, 0.3, c),
             w2=rng.normal(0, np.sqrt(2.0 / c), (c, c, 1, 1)), b2=rng.normal(0, 0.3, c))
    if s == 2:
        w.update(wd1=rng.normal(0, 0.5, (cin, 1, 3, 3)), bd1=rng.normal(0, 0.3, cin), w3=rng.normal(0, np.sqrt(2.0 / cin), (c, cin, 1, 1)), b3=rng.normal(0, 0.3, c))
    return w


def unit_ref(xv, w, c, s, dt):
    """(even channels, odd channels) of the ShuffleV2Block's output, NHWC float64 numpy."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(a).to(dt)
    x = nchw(xv, dt)
    if s == 1:
        even, x2 = x[:, :c], x[:, c:]
    else:
        even = silu(F.conv2d(F.conv2d(x, t(w["wd1"]), t(w["bd1"]), stride=2, padding=1, groups=x.shape[1]), t(w["w3"]), t(w["b3"])))
        x2 = x
    y = silu(F.conv2d(x2, t(w["w1"]), t(w["b1"])))
    y = F.conv2d(y, t(w["wd"]), t(w["bd"]), stride=s, padding=1, groups=c)
    odd = silu(F.conv2d(y, t(w["w2"]), t(w["b2"])))
    return nhwc(even), nhwc(odd)


def unit_case(eng, inst, tile, where, seed, in_odd=(0, 0), out_hw=None, batch=2, also_b1=False):
    """`tile` None: automatic.  in_odd (S = 2): the input is (2 OH - odd_h) x (2 OW - odd_w)."""
    import torch
    _, c, cin, s = inst
    oh, ow = out_hw if out_hw else map_for(*tile)
    ih, iw = (oh, ow) if s == 1 else (2 * oh - in_odd[0], 2 * ow - in_odd[1])
    rng = np.random.default_rng(seed)
    pb = ir.ProgramBuilder("f32s", 2 * ih, 2 * iw, keep_all=True)
    f0 = pb.stem(rng.normal(0, 0.6, (16, 3, 3, 3)), rng.normal(0, 0.1, 16), "relu")
    ld_in, ld_out, coff = cin + 32, 2 * c + 32, 16
    xw = pb.conv(f0, rng.normal(0, 0.35, (ld_in, 16, 1, 1)), rng.normal(0, 0.2, ld_in), "none", out_name="xwide")
    x = pb.view(pb.tensors[xw].buf, ih, iw, cin, coff, ld_in, name="x")
    yw, fill = prefill(pb, f0, ld_out, 1000.0, "ywide", stride=s)
    y = pb.view(pb.tensors[yw].buf, oh, ow, 2 * c, coff, ld_out, name="y")
    w = unit_weights(rng, c, cin, s)
    pb.det_unit(x, y, s, w["w1"], w["b1"], w["wd"], w["bd"], w["w2"], w["b2"], *([w["wd1"], w["bd1"], w["w3"], w["b3"]] if s == 2 else []))
    crops = rng.integers(0, 256, (batch, pb.in_h, pb.in_w, 3), dtype=np.uint8)
    log = run_det_program(eng, pb, batch, crops, tile)
    tag = "det_unit %s c%d cin%d s%d %dx%d<-%dx%d b%d tile %s" % (where, c, cin, s, oh, ow, ih, iw, batch, "%dx%d" % tile if tile else "auto")
    want = tile if tile else det_tiles.pick(inst, device_cus(where), oh, ow, batch)
    assert_tile(log, inst, want, (oh, ow), batch, tag)
    xv, got, wide = rd(eng, pb, "x", batch), rd(eng, pb, "y", batch), rd(eng, pb, "ywide", batch)
    assert_inputs_alive(xv)
    assert np.array_equal(rd(eng, pb, "xwide", batch)[..., coff:coff + cin], xv)
    assert_neighbours(tag, wide, fill, coff, coff + 2 * c)
    assert np.array_equal(wide[..., coff:coff + 2 * c], got)
    refs = {dt: unit_ref(xv, w, c, s, dt) for dt in (torch.float64, torch.float32)}
    if s == 1:
        assert np.array_equal(got[..., 0::2], xv[..., :c]), tag + ": the pass-through half must be x[..., :C] bit for bit"
    else:
        check_close(tag + " even", got[..., 0::2], lambda dt: refs[dt][0], 4.0, eps_floor=floor_for(1))
    check_close(tag + " odd", got[..., 1::2], lambda dt: refs[dt][1], 4.0, eps_floor=floor_for(2))
    if also_b1:      # frame 0 alone, same forced tile: the same bits
        run_det_program(eng, pb, 1, crops, want)
        assert np.array_equal(rd(eng, pb, "y", 1)[0], got[0]), tag + ": frame 0 at B = 1 differs from frame 0 at B = 2"


def unit_forced(eng, case, where):
    inst, th, tw = case
    i = FORCED.index(case)
    b1 = (th, tw) in (EMU_TILES[inst][0], max(PRODUCTION[inst], key=lambda t: (tile_rows(inst, *t), t)))
    if inst[3] == 1:
        unit_case(eng, inst, (th, tw), where, 7000 + i, also_b1=b1)
    else:       # the input once with odd height and even width, once the other way round
        unit_case(eng, inst, (th, tw), where, 7000 + i, in_odd=(1, 0), also_b1=b1)
        unit_case(eng, inst, (th, tw), where, 7500 + i, in_odd=(0, 1))


# automatic mode: (out H, out W, B) per instance -- two small maps, a production-sized map and a batch that fills the chip more than once
UNIT_AUTO = [(inst, hw, b) for inst in sorted(det_tiles.UNIT) for hw, b in (((9, 11), 2), ((6, 7), 5), (det_tiles.PRODUCTION_MAPS[("unit",) + inst][0], 1), ((12, 20), 9))]
UNIT_AUTO_EMU = [a for a in UNIT_AUTO if a[1][0] * a[1][1] * a[2] <= 240]


def unit_auto(eng, case, where):
    inst, hw, b = case
    unit_case(eng, ("unit",) + inst, None, where, 7900 + UNIT_AUTO.index(case), in_odd=(1, 0), out_hw=hw, batch=b)


_auto_id = lambda a: "%s-%dx%d-b%d" % ("_".join(str(v) for v in a[0]), a[1][0], a[1][1], a[2])


@pytest.mark.parametrize("case", [c for c in UNIT_FORCED if EMU_ALL_FORCED or c[1:] in EMU_TILES[c[0]]], ids=case_id)
def test_det_unit_forced_tile_emu(emu_engine, case):
    unit_forced(emu_engine, case, "emu")


@pytest.mark.parametrize("case", UNIT_AUTO_EMU, ids=_auto_id)
def test_det_unit_auto_tile_emu(emu_engine, case):
    unit_auto(emu_engine, case, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", UNIT_FORCED, ids=case_id)
def test_det_unit_forced_tile_gpu(gpu_engine, case):
    unit_forced(gpu_engine, case, "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", UNIT_AUTO, ids=_auto_id)
def test_det_unit_auto_tile_gpu(gpu_engine, case):
    unit_auto(gpu_engine, case, "gpu")


# ---- det_c3 --------------------------------------------------------------------------------------------------------------------
# (CA, CB, upA) of every det_c3 build_detector_program emits: model.10 (192, conv tail), model.14 and model.17 / model.20 (128, detect)
C3_SOURCES = {(192, 1): [(64, 128, True)], (128, 2): [(128, 0, False), (64, 64, True)]}


def c3_weights(rng, cin, tail):
    cv = lambda n, k, ks=1: rng.normal(0, np.sqrt(2.0 / (k * ks * ks)), (n, k, ks, ks))
    w = dict(cv1=cv(32, cin), b_cv1=rng.normal(0, 0.3, 32), cv2=cv(32, cin), b_cv2=rng.normal(0, 0.3, 32), m1=cv(32, 32), b_m1=rng.normal(0, 0.3, 32),
             m2=cv(32, 32, 3), b_m2=rng.normal(0, 0.3, 32), cv3=cv(64, 64), b_cv3=rng.normal(0, 0.3, 64))
    if tail == 1:
        w.update(wt=cv(64, 64), bt=rng.normal(0, 0.3, 64))
    else:
        w.update(wt=rng.normal(0, np.sqrt(1.0 / 64), (48, 64, 1, 1)), bt=rng.normal(0, 0.5, 48))
    return w


def c3_ref(av, bv, up, w, tail, dt, anchors=None, stride=0.0):
    """C3 output, tail output (conv: silu; detect: raw 48 channels), decoded rows [B, 3 H W, 16] (detect only); NHWC float64 numpy."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(dt)
    a = nchw(av, dt)
    if up:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    x = torch.cat([a, nchw(bv, dt)], 1) if bv is not None else a
    y1 = silu(F.conv2d(x, t(w["cv1"]), t(w["b_cv1"])))
    y1 = silu(F.conv2d(silu(F.conv2d(y1, t(w["m1"]), t(w["b_m1"]))), t(w["m2"]), t(w["b_m2"]), padding=1))
    y2 = silu(F.conv2d(x, t(w["cv2"]), t(w["b_cv2"])))
    out = silu(F.conv2d(torch.cat([y1, y2], 1), t(w["cv3"]), t(w["b_cv3"])))
    raw = F.conv2d(out, t(w["wt"]), t(w["bt"]))
    if tail == 1:
        return nhwc(out), nhwc(silu(raw)), None
    B, _, H, W = raw.shape
    v = raw.reshape(B, 3, 16, H, W)
    gx = torch.arange(W, dtype=dt).reshape(1, 1, 1, W) * stride
    gy = torch.arange(H, dtype=dt).reshape(1, 1, H, 1) * stride
    an = t(anchors).reshape(3, 2)
    aw, ah = an[:, 0].reshape(1, 3, 1, 1), an[:, 1].reshape(1, 3, 1, 1)
    sg = torch.sigmoid(v)
    cols = [(sg[:, :, 0] * 2 - 0.5) * stride + gx, (sg[:, :, 1] * 2 - 0.5) * stride + gy, (sg[:, :, 2] * 2) ** 2 * aw, (sg[:, :, 3] * 2) ** 2 * ah, sg[:, :, 4]]
    for k in range(5, 15):
        cols.append(v[:, :, k] * aw + gx if k % 2 == 1 else v[:, :, k] * ah + gy)
    cols.append(sg[:, :, 15])
    rows = torch.stack(cols, -1).reshape(B, 3 * H * W, 16)            # row = (anchor * H + y) * W + x
    return nhwc(out), nhwc(raw), rows.double().numpy()


ROW_GROUPS = [("box", slice(0, 4)), ("conf", slice(4, 5)), ("landmarks", slice(5, 15)), ("class", slice(15, 16))]


def c3_case(eng, inst, tile, where, seed, src, with_out=True, with_out2=True, level=0, out_hw=None, batch=2, also_b1=False):
    import torch
    _, cin, tail = inst
    ca, cb, up = src
    h, w_ = out_hw if out_hw else map_for(*tile, even=up)
    rng = np.random.default_rng(seed)
    pb = ir.ProgramBuilder("f32s", 2 * h, 2 * w_, keep_all=True)
    f0 = pb.stem(rng.normal(0, 0.6, (16, 3, 3, 3)), rng.normal(0, 0.1, 16), "relu")
    coff = 16
    fa = pb.maxpool(f0) if up else f0
    aw_ = pb.conv(fa, rng.normal(0, 0.35, (ca + 32, 16, 1, 1)), rng.normal(0, 0.2, ca + 32), "none", out_name="awide")
    ta = pb.tensors[aw_]
    src_a = pb.view(ta.buf, ta.H, ta.W, ca, coff, ca + 32, name="a")
    src_b = -1
    if cb:
        bw = pb.conv(f0, rng.normal(0, 0.35, (cb + 32, 16, 1, 1)), rng.normal(0, 0.2, cb + 32), "none", out_name="bwide")
        src_b = pb.view(pb.tensors[bw].buf, h, w_, cb, coff, cb + 32, name="b")
    out = out2 = -1
    if with_out:
        ow_, ofill = prefill(pb, f0, 96, 1000.0, "outwide")
        out = pb.view(pb.tensors[ow_].buf, h, w_, 64, coff, 96, name="out")
    c2 = 64 if tail == 1 else 48
    if with_out2:
        o2w, o2fill = prefill(pb, f0, c2 + 32, 2000.0, "out2wide")
        out2 = pb.view(pb.tensors[o2w].buf, h, w_, c2, coff, c2 + 32, name="out2")
    wt = c3_weights(rng, cin, tail)
    kw = dict(out=out, out2=out2, w_tail=wt["wt"], b_tail=wt["bt"])
    if tail == 2:        # rows [row0, row0 + 3 H W) of a buffer of 4 H W rows, all prefilled
        nrows, row0 = 4 * h * w_, (h * w_) // 2
        rows_buf = pb.buffer(nrows * 16, ir.ELEM_F32, "rows", pinned=True)
        rfill = -7.0 - np.arange(64, dtype=np.float64)
        pb.conv(f0, np.zeros((64, 16, 1, 1)), rfill, "none", out=pb.view(rows_buf, h, w_, 64, 0, 64))
        rows_view = buf_view(pb, rows_buf)          # made before finish(): read_buffer() would add it to a finished program
        read_rows = lambda b: eng.read_tensor(0, rows_view, b, (1, 1, nrows * 16)).reshape(b, nrows, 16)
        kw.update(tail="detect", rows_buf=rows_buf, row0=row0, det_stride=float(STRIDES[level]), anchors=ANCHORS[level], nrows_total=nrows)
    else:
        kw.update(tail="conv")
    pb.det_c3(src_a, src_b, up, wt["cv1"], wt["b_cv1"], wt["cv2"], wt["b_cv2"], wt["m1"], wt["b_m1"], wt["m2"], wt["b_m2"], wt["cv3"], wt["b_cv3"], **kw)
    crops = rng.integers(0, 256, (batch, pb.in_h, pb.in_w, 3), dtype=np.uint8)
    log = run_det_program(eng, pb, batch, crops, tile)
    tag = "det_c3 %s cin%d t%d src %d%s+%d %dx%d b%d%s%s%s tile %s" % (where, cin, tail, ca, "up" if up else "", cb, h, w_, batch, " out" if with_out else "",
                                                                      " out2" if with_out2 else "", " lvl%d" % level if tail == 2 else "", "%dx%d" % tile if tile else "auto")
    want = tile if tile else det_tiles.pick(inst, device_cus(where), h, w_, batch)
    assert_tile(log, inst, want, (h, w_), batch, tag)
    av = rd(eng, pb, "a", batch)
    bv = rd(eng, pb, "b", batch) if cb else None
    assert_inputs_alive(av)
    if cb:
        assert_inputs_alive(bv)
    refs = {dt: c3_ref(av, bv, up, wt, tail, dt, ANCHORS[level], float(STRIDES[level])) for dt in (torch.float64, torch.float32)}
    outs = {}
    if with_out:
        outs["out"] = rd(eng, pb, "out", batch)
        assert_neighbours(tag + " out", rd(eng, pb, "outwide", batch), ofill, coff, coff + 64)
        check_close(tag + " c3", outs["out"], lambda dt: refs[dt][0], 4.0, eps_floor=floor_for(4))
    if with_out2:
        outs["out2"] = rd(eng, pb, "out2", batch)
        assert_neighbours(tag + " out2", rd(eng, pb, "out2wide", batch), o2fill, coff, coff + c2)
        check_close(tag + (" tail" if tail == 1 else " raw"), outs["out2"], lambda dt: refs[dt][1], 4.0, eps_floor=floor_for(5 if tail == 1 else 4))
    if tail == 2:
        allrows = read_rows(batch)
        outs["rows"] = allrows
        filled = np.tile(rfill.astype(np.float32), nrows * 16 // 64).reshape(nrows, 16)
        outside = np.r_[0:row0, row0 + 3 * h * w_:nrows]
        assert np.array_equal(allrows[:, outside], np.broadcast_to(filled[outside], (batch, len(outside), 16))), tag + ": rows outside the level's range were written"
        got = allrows[:, row0:row0 + 3 * h * w_]
        for name, cols in ROW_GROUPS:
            check_close(tag + " rows " + name, got[..., cols], lambda dt, cols=cols: refs[dt][2][..., cols], 4.0, eps_floor=floor_for(5))
    if also_b1:
        run_det_program(eng, pb, 1, crops, want)
        for name, g in outs.items():
            g1 = read_rows(1) if name == "rows" else rd(eng, pb, name, 1)
            assert np.array_equal(g1[0], g[0]), tag + ": %s of frame 0 at B = 1 differs from frame 0 at B = 2" % name


def c3_forced_source(case):
    """The source combinations go round with the tile's index; a tile too large for an even map within 33 pixels takes the next one."""
    inst, th, tw = case
    srcs = C3_SOURCES[inst[1:]]
    i = C3_FORCED.index(case)
    return next(s for s in srcs[i % len(srcs):] + srcs if not s[2] or max(th, tw) < 16)


def c3_forced(eng, case, where):
    inst, th, tw = case
    i = C3_FORCED.index(case)
    b1 = (th, tw) in (EMU_TILES[inst][0], max(PRODUCTION[inst], key=lambda t: (tile_rows(inst, *t), t)))
    # the variants go round with the tile's index: source combination, optional outputs, anchor / stride set
    c3_case(eng, inst, (th, tw), where, 8000 + i, c3_forced_source(case), with_out=i % 2 == 0, with_out2=inst[2] == 1 or i % 4 < 2, level=i % 3, also_b1=b1)


# every variant on one mid-sized tile, whatever the rotation above gives it
C3_VARIANTS = [(("c3", 192, 1), (3, 4), (64, 128, True), o, True, 0) for o in (True, False)] + \
              [(("c3", 128, 2), (3, 4), s, o, o2, lvl) for s in C3_SOURCES[(128, 2)] for o, o2, lvl in ((True, True, 0), (False, True, 1), (True, False, 2), (False, False, 0))]
_var_id = lambda v: "%s-%dup%d+%d-out%d-out2%d-lvl%d" % ("_".join(str(x) for x in v[0]), v[2][0], v[2][2], v[2][1], v[3], v[4], v[5])
C3_AUTO = [(inst, C3_SOURCES[inst][-1], hw, b) for inst in sorted(det_tiles.C3) for hw, b in (((10, 12), 2), ((6, 8), 5), ((12, 20), 1), ((12, 20), 9))]
C3_AUTO_EMU = [a for a in C3_AUTO if a[2][0] * a[2][1] * a[3] <= 240]
_c3_auto_id = lambda a: "%d_%d-%dx%d-b%d" % (a[0][0], a[0][1], a[2][0], a[2][1], a[3])


def c3_variant(eng, v, where):
    inst, tile, src, o, o2, lvl = v
    c3_case(eng, inst, tile, where, 8500 + C3_VARIANTS.index(v), src, with_out=o, with_out2=o2, level=lvl)


def c3_auto(eng, a, where):
    inst, src, hw, b = a
    c3_case(eng, ("c3",) + inst, None, where, 8900 + C3_AUTO.index(a), src, out_hw=hw, batch=b)


@pytest.mark.parametrize("case", [c for c in C3_FORCED if EMU_ALL_FORCED or c[1:] in EMU_TILES[c[0]]], ids=case_id)
def test_det_c3_forced_tile_emu(emu_engine, case):
    c3_forced(emu_engine, case, "emu")


@pytest.mark.parametrize("v", C3_VARIANTS, ids=_var_id)
def test_det_c3_variants_emu(emu_engine, v):
    c3_variant(emu_engine, v, "emu")


@pytest.mark.parametrize("a", C3_AUTO_EMU, ids=_c3_auto_id)
def test_det_c3_auto_tile_emu(emu_engine, a):
    c3_auto(emu_engine, a, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", C3_FORCED, ids=case_id)
def test_det_c3_forced_tile_gpu(gpu_engine, case):
    c3_forced(gpu_engine, case, "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("v", C3_VARIANTS, ids=_var_id)
def test_det_c3_variants_gpu(gpu_engine, v):
    c3_variant(gpu_engine, v, "gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("a", C3_AUTO, ids=_c3_auto_id)
def test_det_c3_auto_tile_gpu(gpu_engine, a):
    c3_auto(gpu_engine, a, "gpu")


# ---- det_stem ------------------------------------------------------------------------------------------------------------------
def stem_case(eng, in_hw, f32_input, where, seed, batch=2):
    """StemBlock on the program input (fixed 4 x 16 tile, persistent grid): 20 x 24 -> 5 x 6 is one ragged tile, 36 x 80 -> 9 x 20 is
    3 x 2 tiles, ragged both ways.  Runs in the detector slot: detector_forward feeds both input kinds."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    ih, iw = in_hw
    pb = ir.ProgramBuilder("f32s", ih, iw, keep_all=True)
    cv = lambda n, k, ks=1: rng.normal(0, np.sqrt(2.0 / (k * ks * ks)), (n, k, ks, ks))
    w = dict(w1=cv(16, 3, 3), b1=rng.normal(0, 0.3, 16), w2a=cv(8, 16), b2a=rng.normal(0, 0.3, 8), w2b=cv(16, 8, 3), b2b=rng.normal(0, 0.3, 16),
             w3=cv(16, 32), b3=rng.normal(0, 0.3, 16))
    pb.det_stem(w["w1"], w["b1"], w["w2a"], w["b2a"], w["w2b"], w["b2b"], w["w3"], w["b3"], out_name="y")
    blob = pb.finish([pb.buffer(16, ir.ELEM_F32, "rows")])
    eng.load_program(1, blob, batch)
    if f32_input:
        img = rng.random((batch, 3, ih, iw)).astype(np.float32)
        x01 = img.astype(np.float64)
    else:
        img = rng.integers(0, 256, (batch, ih, iw, 3), dtype=np.uint8)
        x01 = None
    eng.profile_enable(True)
    try:
        eng.detector_forward(img, 1)
        log = eng.launch_log()
    finally:
        eng.profile_enable(False)
    tag = "det_stem %s %s %dx%d b%d" % (where, "f32 nchw" if f32_input else "u8 nhwc", ih, iw, batch)
    assert_launched(log, "det_stem_kernel<64, 304, 19, 208, %s, 256>" % ("true" if f32_input else "false"), tag)
    got = rd(eng, pb, "y", batch, slot=1)
    assert got.shape[1:] == (ih // 4, iw // 4, 16)

    def ref(dt):
        t = lambda a: torch.from_numpy(a).to(dt)
        x = torch.from_numpy(x01).to(dt) if f32_input else torch.from_numpy(img.astype(np.float64)).to(dt).permute(0, 3, 1, 2) / 255.0
        s1 = silu(F.conv2d(x, t(w["w1"]), t(w["b1"]), stride=2, padding=1))
        s2 = silu(F.conv2d(silu(F.conv2d(s1, t(w["w2a"]), t(w["b2a"]))), t(w["w2b"]), t(w["b2b"]), stride=2, padding=1))
        return nhwc(silu(F.conv2d(torch.cat([s2, F.max_pool2d(s1, 2, 2, ceil_mode=True)], 1), t(w["w3"]), t(w["b3"]))))
    check_close(tag, got, ref, 4.0, eps_floor=floor_for(4))


STEM_CASES = [((20, 24), False), ((20, 24), True), ((36, 80), False), ((36, 80), True)]
_stem_id = lambda c: "%dx%d-%s" % (c[0][0], c[0][1], "f32" if c[1] else "u8")


@pytest.mark.parametrize("case", STEM_CASES, ids=_stem_id)
def test_det_stem_emu(emu_engine, case):
    stem_case(emu_engine, case[0], case[1], "emu", 9000 + STEM_CASES.index(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", STEM_CASES, ids=_stem_id)
def test_det_stem_gpu(gpu_engine, case):
    stem_case(gpu_engine, case[0], case[1], "gpu", 9100 + STEM_CASES.index(case))


# ---- the option itself, and the coverage of the table ---------------------------------------------------------------------------
def test_every_production_tile_has_a_forced_case():
    """256 compute units, the 384 x 640 layer maps, B = 1 .. 32: every tile det_pick_tile chooses is in FORCED, its region fits its
    kernel and its test map stays within 33 x 33; the emulator tier holds the tiles the module docstring promises."""
    picked = {(inst, th, tw) for inst, maps in det_tiles.PRODUCTION_MAPS.items() for h, w in maps for b in det_tiles.PRODUCTION_BATCHES
              for th, tw in [det_tiles.pick(inst, det_tiles.PRODUCTION_CUS, h, w, b)]}
    uncovered = sorted(picked - set(FORCED))
    print("production tiles: %d, uncovered: %d" % (len(picked), len(uncovered)))
    assert not uncovered, uncovered
    assert set(det_tiles.PRODUCTION_MAPS) == set(det_tiles.INSTANCES)
    for inst, th, tw in FORCED:
        assert tile_rows(inst, th, tw) <= det_tiles.INSTANCES[inst][1]
        for even in ([False] if inst[0] == "unit" else [c3_forced_source((inst, th, tw))[2]]):
            h, w = map_for(th, tw, even)
            assert h <= 33 and w <= 33 and h > 2 * th - (th == 1) and w > 2 * tw - (tw == 1), (inst, th, tw, h, w)
    # the example the issue gives for det_unit<32, 32, 1> at 48 x 80
    assert PRODUCTION[("unit", 32, 64, 1)] == sorted([(2, 5), (3, 5), (5, 5), (6, 5), (8, 5), (6, 8), (6, 9), (6, 10), (7, 10), (8, 10), (10, 9), (12, 8), (12, 9),
                                                      (12, 10), (8, 16), (16, 9), (16, 10), (12, 16)])
    for inst, tiles in EMU_TILES.items():
        rows = [tile_rows(inst, *t) for t in tiles]
        assert min(rows) == min(tile_rows(inst, *t) for t in PRODUCTION[inst]) and max(rows) == max(tile_rows(inst, *t) for t in PRODUCTION[inst])
        assert any(t[0] * t[1] % 16 == 0 for t in tiles) and any(t[0] * t[1] % 16 for t in tiles) and any(((r + 15) // 16) % 2 for r in rows)


def test_det_tile_that_does_not_fit_is_refused_before_any_launch(emu_engine):
    """A forced tile whose region exceeds the kernel's LDS rows fails the forward call with a message and launches nothing (not even
    the ops in front of the det op); the option back at 0 runs again.  Host-side path only: no kernel ever sees such a tile."""
    rng = np.random.default_rng(5)
    inst = ("unit", 64, 128, 1)          # 128 LDS rows: 6 x 10 (96 rows) fits, 9 x 13 (165 rows) does not
    pb = ir.ProgramBuilder("f32s", 16, 16, keep_all=True)
    f0 = pb.stem(rng.normal(0, 0.6, (16, 3, 3, 3)), rng.normal(0, 0.1, 16), "relu")
    x = pb.conv(f0, rng.normal(0, 0.35, (128, 16, 1, 1)), rng.normal(0, 0.2, 128), "none", out_name="x")
    w = unit_weights(rng, 64, 128, 1)
    pb.det_unit(x, pb.tensor(8, 8, 128, name="y"), 1, w["w1"], w["b1"], w["wd"], w["bd"], w["w2"], w["b2"])
    crops = rng.integers(0, 256, (1, 16, 16, 3), dtype=np.uint8)
    log = run_det_program(emu_engine, pb, 1, crops, None)
    assert det_tiles.logged_tiles(log, inst)
    emu_engine.set_option(_native.PF_OPT_DET_TILE, _native.det_tile_option(9, 13))
    emu_engine.profile_enable(True)
    with pytest.raises(_native.PeppaHipError, match=r"PF_OPT_DET_TILE: tile 9x13 needs a region of 165 rows, det_unit_kernel<64, 64, 1> holds 128"):
        emu_engine.landmark_forward(crops)
    assert emu_engine.launch_log() == []
    emu_engine.profile_enable(False)
    with pytest.raises(_native.PeppaHipError, match="PF_OPT_DET_TILE"):
        emu_engine.set_option(_native.PF_OPT_DET_TILE, 5)          # th = 0
    emu_engine.set_option(_native.PF_OPT_DET_TILE, 0)
    emu_engine.landmark_forward(crops)

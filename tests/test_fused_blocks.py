"""Fused encoder blocks (csrc/k_mbconv.h, expdw epilogue of csrc/k_expdw.h) against the layer-by-layer
program of the same weights and against the oracle.

The fused program replaces, per inverted-residual block (timm InvertedResidual, Student encoder
model.py:252-264), "pointwise expand -> depthwise -> [SE] -> pointwise project" by
  * one MBCONV launch (blocks without SE, 3x3 depthwise), or
  * one EXPDW launch (expand + depthwise + SE squeeze) followed by the gated projection,
so every block output ("encoder.blocks.i.j.out") must agree with the unfused program to f32 rounding.
Batch sizes that do not fill the last workgroup (3 faces, 4 whole images per workgroup at 8x8) exercise
the ragged-tile guards."""
import numpy as np
import pytest

from oracle import synth_weights as sw
from peppa_pig_face_landmark_amd.graph import ir
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from tests import helpers


def _op_codes(blob: bytes):
    import struct
    hdr = struct.unpack_from("<16i", blob, 0)
    n_bufs, n_tensors, n_ops = hdr[3], hdr[4], hdr[5]
    off = 64 + n_bufs * 16 + n_tensors * 32
    return [struct.unpack_from("<i", blob, off + 160 * i)[0] for i in range(n_ops)]


def _compare_programs(eng, weights, size, batch):
    crops = sw.smooth_blob_images(batch, size, seed=4200 + size + batch)
    outs = {}
    for fuse in (False, True):
        blob, info = build_student_program(weights, size, "f32s", keep_all=True, fuse_mbconv=fuse)
        codes = _op_codes(blob)
        assert (ir.OP_MBCONV in codes) == fuse and (ir.OP_EXPDW in codes) == fuse and (ir.OP_MBX in codes) == (fuse and size == 256)
        eng.load_program(0, blob, batch)
        loc, score = eng.landmark_forward(crops)
        outs[fuse] = (loc, score)
    return crops, outs


def _check(eng, weights, size, batch):
    crops, outs = _compare_programs(eng, weights, size, batch)
    loc0, score0 = outs[False]
    loc1, score1 = outs[True]
    oloc, oscore, taps = helpers.oracle_student(weights, crops)
    # every block output of the fused program against the oracle's taps (the unfused program passes the same check
    # in test_emu_landmark / test_gpu_landmark)
    blob, info = build_student_program(weights, size, "f32s", keep_all=True, fuse_mbconv=True)
    eng.load_program(0, blob, batch)
    eng.landmark_forward(crops)
    checked = 0
    for name in info["tensors"]:
        if name not in taps or not name.startswith("encoder.blocks."):
            continue
        ref = helpers.tap_nhwc(taps, name)
        got = helpers.read_engine_tensor(eng, 0, info, name, batch, ref.shape[1:], 4)
        rel = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12)
        assert rel < 2e-4, (name, rel)
        checked += 1
    assert checked >= 15
    safe = helpers.heat_margins(taps) > 1e-3
    d = np.abs(loc1 - loc0).reshape(batch, 98, 2).max(2)
    assert d[safe].max() < 1e-4          # fused vs unfused program
    d = np.abs(loc1 - oloc).reshape(batch, 98, 2).max(2)
    assert d[safe].max() < 2e-4          # fused program vs oracle (north-star tolerance is 1e-3)
    assert np.abs(score1 - score0)[safe].max() < 2e-3


@pytest.mark.parametrize("size,batch", [(64, 3), (128, 2), (256, 1)])
def test_fused_blocks_match_unfused_emu(emu_engine, student_weights, size, batch):
    _check(emu_engine, student_weights, size, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("size,batch", [(128, 3), (256, 5)])
def test_fused_blocks_match_unfused_gpu(gpu_engine, student_weights, size, batch):
    _check(gpu_engine, student_weights, size, batch)


def _mbx_vs_layerwise(eng, weights, batch, keep_all, on_gpu=False, n_mbx=8, **mbx_kw):
    """Stages 3-5 at 16 x 16 through the input-stationary block kernel (csrc/k_mbx.h, PF_OP_MBX: non-SE blocks in one launch, SE
    blocks as squeeze pass + FCs + either a recompute-gate-project pass or the layer-wise projection on the map the squeeze pass
    stored) against the same program with those blocks as expand + depthwise launch -> gated projection (fuse_mbx=False): the
    non-SE blocks bit for bit (same products in the same order), the SE blocks to the rounding noise of the f32s path (their channel
    means are summed in another order and the SE gates amplify it; each block is held to the ORACLE at 2e-4 by _check above)."""
    crops = sw.smooth_blob_images(batch, 256, seed=5100 + batch)
    res = {}
    for mbx in (False, True):
        blob, info = build_student_program(weights, 256, "f32s", keep_all=keep_all, fuse_mbx=mbx, **(mbx_kw if mbx else {}))
        codes = _op_codes(blob)
        assert (ir.OP_MBX in codes) == mbx and codes.count(ir.OP_MBX) == (n_mbx if mbx else 0), codes.count(ir.OP_MBX)
        eng.load_program(0, blob, batch)
        loc, score = eng.landmark_forward(crops)
        blocks = {}
        if keep_all:
            for name in info["tensors"]:
                if name.startswith("encoder.blocks.") and name.endswith(".out") and name.split(".")[2] in "345":
                    c = {"3": 80, "4": 112, "5": 160}[name.split(".")[2]]
                    blocks[name] = helpers.read_engine_tensor(eng, 0, info, name, batch, (16, 16, c), 4)
        res[mbx] = (loc, score, blocks)
    for name, ref in res[False][2].items():
        got = res[True][2][name]
        if name.split(".")[2] == "3":
            assert np.array_equal(got, ref), (name, float(np.abs(got - ref).max()))
        else:
            rel = np.abs(got - ref).max() / np.abs(ref).max()
            assert rel < 2e-4, (name, rel)
    if keep_all:
        assert len(res[True][2]) == 9
    oloc, oscore, taps = helpers.oracle_student(weights, crops[:min(batch, 8)])
    n = oloc.shape[0]
    safe = helpers.heat_margins(taps) > 1e-3
    d = np.abs(res[True][0][:n] - oloc).reshape(n, 98, 2).max(2)
    assert d[safe].max() < 2e-4
    d = np.abs(res[True][0] - res[False][0]).reshape(batch, 98, 2).max(2)
    assert np.quantile(d, 0.99) < 1e-4                   # (a near-tie arg-max may flip on a last-bit difference: not the kernels' business here)
    assert np.isfinite(res[True][1]).all()


_MBX_VARIANTS = [({}, 8),                                        # default: non-SE blocks in one launch, SE blocks squeeze-and-store + layer-wise projection
                 ({"mbx_se": "recompute"}, 13),                  # every SE block: squeeze pass + 8- / 16-wave recompute-gate-project pass
                 ({"mbx_waves": 8}, 8)]                          # the non-SE blocks on 8 waves


@pytest.mark.parametrize("kw,n_mbx", [_MBX_VARIANTS[0], ({"mbx_se": "recompute", "mbx_waves": 8}, 13)])      # (the 16-wave recompute pass: GPU tier)
def test_mbx_blocks_match_layerwise_emu(emu_engine, student_weights, kw, n_mbx):
    # 7 faces on the emulator's 5 workgroups: the unit loop runs, and the squeeze passes split every face into 2 tile ranges
    # (engine.cpp PF_OP_MBX nsplit: 14 half faces = three rounds of five); 6 faces: 4 ranges per face (24 units, five rounds)
    _mbx_vs_layerwise(emu_engine, student_weights, 7 if not kw else 6, True, n_mbx=n_mbx, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kw,n_mbx", _MBX_VARIANTS)
@pytest.mark.parametrize("batch,keep_all", [(5, True), (300, False)])
def test_mbx_blocks_match_layerwise_gpu(gpu_engine, student_weights, batch, keep_all, kw, n_mbx):
    _mbx_vs_layerwise(gpu_engine, student_weights, batch, keep_all, on_gpu=True, n_mbx=n_mbx, **kw)   # 300 faces on 256 CUs: some workgroups walk two faces

"""Face attributes from the landmark network's fc head (Net.fc, model.py:269,286-293), opt-in per program (face_attrs=True).

CPU tier: program structure, the SIMT-emulator parity of the fused pools (hero / halo conv partial sums for decx4, the tile-sum SCSE
kernel for decx8) and of the gap fall-back, the ABI's refusals and the weights opt-in.  The GPU twins live in
tests/test_gpu_face_attrs.py."""
import struct

import numpy as np
import pytest

from oracle import synth_weights as sw
from tests import helpers
from peppa_pig_face_landmark_amd.graph import ir
from peppa_pig_face_landmark_amd.graph.student import build_student_program

FC_TAPS = ("decoder.upsampler2.conv2", "decoder.upsampler1.scse", "decoder.aspp.out")


def fc_head_restatement(weights, maps):
    """model.py:286-293 in float64: fmx4 / fmx8 / fmx16 = adaptive average pools of decx4, decx8 and the ASPP output (Decoder.forward's
    third map), concatenated in that order, then fc = nn.Linear(640, 7).  ``maps``: three NHWC arrays [B][H][W][C]."""
    fm = np.concatenate([np.asarray(m, np.float64).mean(axis=(1, 2)) for m in maps], axis=1)
    return fm @ weights["fc.weight"].astype(np.float64).T + weights["fc.bias"].astype(np.float64)


def oracle_fc(weights, crops):
    _, _, taps = helpers.oracle_student(weights, crops)
    return fc_head_restatement(weights, [helpers.tap_nhwc(taps, n) for n in FC_TAPS])


def _read(engine, info, name, batch):
    tid = info["tensors"][name]
    h, w, c = info["shapes"][name]
    return engine.read_tensor(0, tid, batch, (h, w, c))


def _ops(blob):
    hdr = struct.unpack("<16i", blob[:64])
    n_bufs, n_tensors, n_ops = hdr[3], hdr[4], hdr[5]
    off = 64 + 16 * n_bufs
    tens = [struct.unpack("<8i", blob[off + 32 * i: off + 32 * i + 32]) for i in range(n_tensors)]
    off += 32 * n_tensors
    ops = [struct.unpack("<40i", blob[off + 160 * i: off + 160 * i + 160]) for i in range(n_ops)]
    return hdr, tens, ops


def _shapes(blob, info):
    _, tens, _ = _ops(blob)
    info["shapes"] = {n: (tens[t][3], tens[t][4], tens[t][5]) for n, t in info["tensors"].items()}
    return info


def _raw_bound(ref):
    return 2e-4 * max(1.0, float(np.abs(ref).max()))


# ---- 1. program structure ------------------------------------------------------------------------------------------------------

def test_program_structure_fused_pools(student_weights):
    """f32s@256: one new op, at most one GAP more than without the head and it reads aspp.out; decx4 / decx8 are pooled from slabs."""
    blob0, info0 = build_student_program(student_weights, 256, "f32s")
    blob1, info1 = build_student_program(student_weights, 256, "f32s", face_attrs=True)
    h0, _, ops0 = _ops(blob0)
    h1, _, ops1 = _ops(blob1)
    assert h0[12] == -1 and h1[12] >= 0
    assert [o[0] for o in ops1].count(ir.OP_FACEATTR) == 1 and ir.OP_FACEATTR not in [o[0] for o in ops0]
    gaps0 = [o for o in ops0 if o[0] == ir.OP_GAP]
    gaps1 = [o for o in ops1 if o[0] == ir.OP_GAP]
    assert len(gaps1) - len(gaps0) <= 1
    t = info1["tensors"]
    new_gap_inputs = {o[1] for o in gaps1} - {o[1] for o in gaps0}
    assert new_gap_inputs <= {t["decoder.aspp.out"]}
    for name in ("decoder.upsampler2.conv2", "decoder.upsampler1.scse", "decoder.upsampler1.pw"):
        assert all(o[1] != t[name] for o in gaps1), name
    # the hero conv and the SCSE carry their slab fields; the record buffer is the third output
    conv2 = [o for o in ops1 if o[0] == ir.OP_CONV and o[2] == t["decoder.upsampler2.conv2"]]
    scse = [o for o in ops1 if o[0] == ir.OP_SCSE and o[2] == t["decoder.upsampler1.scse"]]
    assert len(conv2) == 1 and conv2[0][1 + 24] > 0
    assert len(scse) == 1 and scse[0][1 + 5] > 0
    fa = [o for o in ops1 if o[0] == ir.OP_FACEATTR][0]
    assert fa[1] == h1[12]


def test_f32_program_pools(student_weights):
    """Exact-f32 programs: decx8 from the SCSE tile sums (256 channels = 64 lanes of 4), decx4 and aspp.out by gap ops."""
    blob, info = build_student_program(student_weights, 128, "f32", face_attrs=True)
    _, _, ops = _ops(blob)
    t = info["tensors"]
    gap_inputs = {o[1] for o in ops if o[0] == ir.OP_GAP}
    assert {t["decoder.upsampler2.conv2"], t["decoder.aspp.out"]} <= gap_inputs and t["decoder.upsampler1.scse"] not in gap_inputs
    scse = [o for o in ops if o[0] == ir.OP_SCSE and o[2] == t["decoder.upsampler1.scse"]]
    assert scse[0][1 + 5] > 0


def test_program_without_head_is_unchanged(student_weights):
    """face_attrs=False is the default: no third output, no new op, and the teacher gets the same switch."""
    from peppa_pig_face_landmark_amd.graph.teacher import build_teacher_program
    for blob, _ in (build_student_program(student_weights, 128, "f32", face_attrs=False),
                    build_student_program(student_weights, 256, "f32s")):
        h, _, ops = _ops(blob)
        assert h[12] == -1 and all(o[0] != ir.OP_FACEATTR for o in ops)
    blob, _ = build_teacher_program(sw.teacher_weights(), 256, "f32s", face_attrs=True)
    h, _, ops = _ops(blob)
    assert h[12] >= 0 and sum(o[0] == ir.OP_FACEATTR for o in ops) == 1


def test_onnx_style_weights_without_fc_are_refused(student_weights):
    w = {k: v for k, v in student_weights.items() if not k.startswith("fc.")}
    build_student_program(w, 128, "f32")            # the landmark program alone does not need the head
    with pytest.raises(ValueError, match=r"fc\.weight.*\.pth"):
        build_student_program(w, 128, "f32", face_attrs=True)
    bad = dict(student_weights)
    bad["fc.weight"] = np.zeros((7, 600), np.float32)
    with pytest.raises(ValueError, match="shape"):
        build_student_program(bad, 128, "f32", face_attrs=True)


# ---- 2. emulator parity --------------------------------------------------------------------------------------------------------

def _run(engine, weights, size, dtype, batch, crops, **kw):
    blob, info = build_student_program(weights, size, dtype, **kw)
    engine.load_program(0, blob, batch)
    out = engine.landmark_forward(crops, attrs=kw.get("face_attrs", False))
    return out, _shapes(blob, info)


def test_emu_fused_path_f32s_256(emu_engine, student_weights):
    """Hero conv slabs (decx4 at 64 x 64) + SCSE tile sums (decx8) + gap(aspp.out), one 256 x 256 face."""
    crops = sw.smooth_blob_images(1, 256, seed=5)
    (loc1, score1, x), info = _run(emu_engine, student_weights, 256, "f32s", 1, crops, face_attrs=True)
    ref = oracle_fc(student_weights, crops)
    assert np.abs(x - ref).max() < _raw_bound(ref), (x, ref)
    cooked = emu_engine.face_attrs(1, raw=False)
    np.testing.assert_allclose(cooked[:, :3], 90.0 * x[:, :3], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(cooked[:, 3:], 1.0 / (1.0 + np.exp(-x[:, 3:].astype(np.float64))), rtol=1e-5, atol=1e-6)
    (loc0, score0), _ = _run(emu_engine, student_weights, 256, "f32s", 1, crops)
    assert np.array_equal(loc0, loc1) and np.array_equal(score0, score1)


@pytest.mark.parametrize("dtype", ["f32s", "f32"])
def test_emu_halo_path_and_gap_fallback_128(emu_engine, student_weights, dtype):
    """f32s@128: decx4 from the 32-wide halo kernel's slabs; f32@128: decx4 and aspp.out by gap ops (nparts = 1), decx8 from the SCSE
    tile sums (f32's 256 channels are 64 lanes of 4).  Two faces; against the oracle
    and against the same restatement over the engine's own maps of a keep_all program (separates pooling from layer error)."""
    B = 2
    crops = sw.smooth_blob_images(B, 128, seed=77)
    (loc1, score1, x), _ = _run(emu_engine, student_weights, 128, dtype, B, crops, face_attrs=True)
    ref = oracle_fc(student_weights, crops)
    assert np.abs(x - ref).max() < _raw_bound(ref), (x, ref)
    (loc0, score0), _ = _run(emu_engine, student_weights, 128, dtype, B, crops)
    assert np.array_equal(loc0, loc1) and np.array_equal(score0, score1)
    (_, _, xk), info = _run(emu_engine, student_weights, 128, dtype, B, crops, face_attrs=True, keep_all=True)
    own = fc_head_restatement(student_weights, [_read(emu_engine, info, n, B) for n in FC_TAPS])
    assert np.abs(xk - own).max() <= 1e-5 * max(1.0, float(np.abs(own).max())), (xk, own)


def test_emu_f16_program_with_head(emu_engine, student_weights):
    """f16 programs take the gap fall-back for all three pools."""
    crops = sw.smooth_blob_images(1, 64, seed=3)
    (_, _, x), _ = _run(emu_engine, student_weights, 64, "f16", 1, crops, face_attrs=True)
    ref = oracle_fc(student_weights, crops)
    assert np.abs(x - ref).max() < 5e-2 * max(1.0, float(np.abs(ref).max()))


# ---- 3. ABI refusals, weights opt-in -------------------------------------------------------------------------------------------

def test_face_attrs_needs_the_head_and_a_call(emu_engine, student_weights):
    from peppa_pig_face_landmark_amd._native import PeppaHipError
    crops = sw.smooth_blob_images(1, 64, seed=9)
    blob, _ = build_student_program(student_weights, 64, "f32")
    emu_engine.load_program(0, blob, 1)
    emu_engine.landmark_forward(crops)
    with pytest.raises(PeppaHipError, match="no face-attribute head"):
        emu_engine.face_attrs(1)
    blob, _ = build_student_program(student_weights, 64, "f32", face_attrs=True)
    emu_engine.load_program(0, blob, 1)
    with pytest.raises(PeppaHipError, match="left no face-attribute rows"):
        emu_engine.face_attrs(1)
    emu_engine.landmark_forward(crops)
    with pytest.raises(PeppaHipError, match="2 rows asked"):
        emu_engine.face_attrs(2)
    assert emu_engine.face_attrs(1).shape == (1, 7)


def _cotrain_sd(student_weights, teacher=None, **over):
    sd = {"student." + k: v for k, v in student_weights.items()}
    if teacher is not None:
        sd.update({"teacher." + k: v for k, v in teacher.items()})
    sd.update(over)
    return sd


def test_weights_keep_fc_opt_in(student_weights, tmp_path):
    from peppa_pig_face_landmark_amd import weights as W
    tw = sw.teacher_weights()
    sd = _cotrain_sd(student_weights, tw)
    s0, t0 = W.split_cotrain_state_dict(sd)
    assert "fc.weight" not in s0 and "fc.weight" not in t0            # the default drops the head, as before
    s1, t1 = W.split_cotrain_state_dict(sd, keep_fc=True)
    for got, src in ((s1, student_weights), (t1, tw)):
        assert got["fc.weight"].shape == (7, 640) and got["fc.bias"].shape == (7,)
        assert np.array_equal(got["fc.weight"], src["fc.weight"])
    bad = _cotrain_sd(student_weights, tw, **{"student.fc.weight": np.zeros((7, 64), np.float32)})
    W.split_cotrain_state_dict(bad)                                   # ignored without the opt-in
    with pytest.raises(ValueError, match="student.fc.weight has shape"):
        W.split_cotrain_state_dict(bad, keep_fc=True)
    gone = {k: v for k, v in sd.items() if k != "teacher.fc.bias"}
    with pytest.raises(ValueError, match="teacher"):
        W.split_cotrain_state_dict(gone, keep_fc=True)
    # .npz files and the ONNX refusal of load_weights
    p = tmp_path / "kps_student.npz"
    np.savez(p, **s0)
    with pytest.raises(ValueError, match="fc head"):
        W.load_weights(str(p), "student", keep_fc=True)
    np.savez(p, **s1)
    assert W.load_weights(str(p), "student", keep_fc=True)["fc.bias"].shape == (7,)
    with pytest.raises(ValueError, match="ONNX"):
        W.load_weights(str(tmp_path / "kps_student.onnx"), "student", keep_fc=True)


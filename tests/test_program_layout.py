"""The packed-program contract between ``graph/ir.py`` (packer) and ``csrc/pf_program.h`` (executor).

1. ``ir.OP_LAYOUT`` and the ``Pf<Name>Op`` structs of the header name the same fields, in the same order, with the same type
   (int32 / float), for the same op codes; ``OP_FIELDS`` and ``VERSION`` agree too.  The header is read as text: its declarations
   keep a regular shape (``int32_t a, b;`` / ``float x;`` / ``PfNested name[N];``), so a few regular expressions are enough.
2. The blobs of a fixed set of programs are byte for byte what they were when the named layout was introduced (SHA-256 below).
   A change that alters the wire format on purpose bumps ``PF_PROGRAM_VERSION`` and these constants together.
"""
import hashlib
import os
import re

import pytest

from oracle import synth_weights as sw
from peppa_pig_face_landmark_amd.graph import ir
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.graph.teacher import build_teacher_program

HEADER = os.path.join(os.path.dirname(ir.__file__), "..", "csrc", "pf_program.h")


def _parse_header():
    text = re.sub(r"//[^\n]*", "", open(HEADER).read())
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(PF_\w+)\s+(\d+)\s*$", text, re.M)}
    codes = {name: int(v) for name, v in re.findall(r"\bPF_OP_(\w+)\s*=\s*(\d+)\s*,", text)}
    words = {name: int(n) for name, n in re.findall(r"^PF_OP_LAYOUT\((\w+),\s*(\d+)\);", text, re.M)}
    structs = {}
    for name, body in re.findall(r"\bstruct\s+(Pf\w+)\s*\{(.*?)\n\};", text, re.S):
        members = []
        for stmt in body.split(";"):
            stmt = " ".join(stmt.split())
            m = re.fullmatch(r"(int32_t|float) (\w+(?: ?, ?\w+)*)", stmt)
            if m:
                members += [(n.strip(), "float" if m.group(1) == "float" else "int") for n in m.group(2).split(",")]
                continue
            m = re.fullmatch(r"(Pf\w+) (\w+)\[(\d+)\]", stmt)
            if m:
                members.append((m.group(2), int(m.group(3)), m.group(1)))
            elif stmt:
                members = None          # not a plain record (PfOpRec with its accessor)
                break
        if members is not None:
            structs[name] = members
    return defines, codes, words, structs


def _expected(layout):
    """ir.OP_LAYOUT entry -> [(name, "int" | "float") | (name, count, [sub-members])]"""
    out = []
    for spec in layout:
        if isinstance(spec, tuple):
            out.append((spec[0], spec[1], _expected(spec[2])))
            continue
        name = spec.rstrip("?")
        out.append((name[:-2], "float") if name.endswith(":f") else (name, "int"))
    return out


def _resolved(structs, members):
    return [(m[0], m[1], structs[m[2]]) if len(m) == 3 else m for m in members]


def _n_words(members):
    return sum(m[1] * _n_words(m[2]) if len(m) == 3 else 1 for m in members)


def test_constants_and_op_codes():
    defines, codes, _, _ = _parse_header()
    assert defines["PF_OP_FIELDS"] == ir.OP_FIELDS == 39
    assert defines["PF_PROGRAM_VERSION"] == ir.VERSION == 11
    py_codes = {k[3:]: v for k, v in vars(ir).items() if k.startswith("OP_") and isinstance(v, int) and k != "OP_FIELDS"}
    assert py_codes == codes
    assert len(set(codes.values())) == len(codes) == 26
    assert set(ir.OP_LAYOUT) == set(codes.values())


def test_every_op_layout_matches_the_header():
    _, codes, words, structs = _parse_header()
    for name, code in sorted(codes.items(), key=lambda kv: kv[1]):
        st = "Pf%sOp" % name.capitalize()
        assert st in structs, "no struct %s for PF_OP_%s" % (st, name)
        got, want = _resolved(structs, structs[st]), _expected(ir.OP_LAYOUT[code])
        assert got == want, "PF_OP_%s: header %s\n  != ir.OP_LAYOUT %s" % (name, got, want)
        assert words.get(st) == _n_words(want) <= ir.OP_FIELDS, "PF_OP_LAYOUT(%s, ...) does not count its words" % st


def test_only_trailing_fields_are_optional():
    for code, layout in ir.OP_LAYOUT.items():
        flags = [isinstance(s, str) and s.endswith("?") for s in layout]
        first = flags.index(True) if True in flags else len(flags)
        assert all(flags[first:]), "op %d: an optional field in front of a mandatory one" % code


def test_packer_refuses_unknown_and_missing_fields():
    pb = ir.ProgramBuilder("f32", 64, 64)
    with pytest.raises(AssertionError, match="unknown fields"):
        pb._op(ir.OP_GAP, [], [], in_t=0, out_buf=0, out_t=0)
    with pytest.raises(AssertionError, match="out_buf is missing"):
        pb._op(ir.OP_GAP, [], [], in_t=0)
    with pytest.raises(AssertionError, match="unknown fields"):
        pb._op(ir.OP_BLOCK, [], [], in_t=0, out_t=0, C=18, convs=[dict(wt=0, bias=0, acc_scale=1.0, shift=0)])
    pb._op(ir.OP_SCSE, [], [], in_t=1, out_t=2, cse_buf=3, sse_w=4, sse_b=0.5)          # gap_parts_plus1 may be left out
    assert pb.ops[-1][1][:6] == [1, 2, 3, 4, 0x3F000000, 0] and len(pb.ops[-1][1]) == ir.OP_FIELDS


# SHA-256 of the blobs built from oracle.synth_weights
BLOB_SHA256 = {
    "student_128_f16": "5b12a4ffdb50f5fff810bb36341a53fdc92d0a57e5430ec60fe3aafc5eac5782",
    "student_128_f32": "37a61d388bd8e58c6060c713bdd8e22bebc20f2349fcbc8895a5077273b3f997",
    "student_128_f32s": "19d27352586ecf3839b6ab4cd97bd67b0ec86967dd8578720baad424912b3607",
    "student_256_f16": "865e773f7bed2a76b1905fcd740d9aae1d7de36edcebb00874ee8afe34ad785f",
    "student_256_f32": "2f865132bf607af1ada422860c35b6ac03835fff1962d1def819858b6b1d18b7",
    "student_256_f32s": "e4be4f52eee70f91ac1ae78e849f93c211be8dd9af6f82d9b370edfc55401133",
    "student_256_f32s_face_attrs": "d8f02aacf95c8278674582aeb9a0360f1a43c35c646b882a6f10047881604b73",
    "student_256_f32s_no_mbx": "582b693abaaa4b5a66c91f744074656349c2d78b64b855883ad9e3378adf4fec",
    "student_256_f32s_no_mbconv": "9ef95de623f15863b34de42a3ec40575444dffa0bd1ead4c3e5c5a97afdb3e2a",
    "student_256_f32s_one_product_hero": "738ac643ad159bfd1a06c4e9b4d49500d85ff05a46d256c472992953b9d53525",
    "teacher_256_f32s": "d566091ec1a866eedc7220cf8ddbc180a1a9cd105267ee5948e2cd4829782a09",
    "teacher_256_f16": "5162ec0beef7f5b41348815fd53e2eb6191313aff3099ea76fb572b93ad59c73",
    "teacher_256_f32s_face_attrs": "3111360d3dfa3226b34c2cf9ea755f5bb26f500b8a7b049167a5efca91b1ccd6",
    "detector_384x640_f16": "4638162bab78fd07864a346c4dcca53f5504ccecf333d3d561a5ab89acf2e341",
    "detector_384x640_f32": "ba7ddb888288668ea221dc76c8470c360a167bb7f318dfe0a2e91c097a86033c",
    "detector_384x640_f32s": "239a0abd0732339307e171549a571bdbd08426527a73e048b0aa0f13343be089",
    "detector_384x640_f32s_no_wg_units": "3c0e1f67d2cc3f60570484c1b23c1df39bdcdff17f03cee0d5d2949174568bc5",
}


def _build(case, student_weights, detector_weights):
    net, size, dtype, *opt = case.split("_", 3)
    opt = opt[0] if opt else ""
    if net == "detector":
        return build_detector_program(detector_weights, (384, 640), dtype, wg_units=opt != "no_wg_units")
    if net == "teacher":
        return build_teacher_program(sw.teacher_weights(), int(size), dtype, face_attrs=opt == "face_attrs")
    kw = {"": {}, "face_attrs": {"face_attrs": True}, "no_mbx": {"fuse_mbx": False}, "no_mbconv": {"fuse_mbconv": False},
          "one_product_hero": {"one_product": ("hero",)}}[opt]
    return build_student_program(student_weights, int(size), dtype, **kw)


@pytest.mark.parametrize("case", sorted(BLOB_SHA256))
def test_blob_bytes_are_unchanged(case, student_weights, detector_weights):
    built = _build(case, student_weights, detector_weights)
    blob = built[0] if isinstance(built, tuple) else built
    assert hashlib.sha256(blob).hexdigest() == BLOB_SHA256[case]

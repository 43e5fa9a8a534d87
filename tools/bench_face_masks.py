"""Cost of the face-region label maps (pf_mask_faces / pf_face_masks, csrc/k_mask.h), in one process on one device.

  * mask_edges and mask_fill (pf_profile_fetch) for 96 frames of 1080p with 8 planted faces each in frame space, and for 768
    chip-space maps at S = 112; beside each the time of hipMemsetAsync over the same `labels` bytes -- the floor for a kernel that
    must write every byte -- and the ratio;
  * the same fill with the tile culling and the parity folding disabled (every slot of the image evaluated in every tile).  That is
    a knob of the TOOL build only (libpeppa_hip_ablate.so reads PEPPA_MASK_NOCULL when a handle is created; the production library
    has no such switch), so this half runs two handles of that library and checks that both give the same bytes;
  * pf_run_frames on 1080p synthetic frames with 8 planted faces each (Student f32s@256, detector running, top_k 8): masks off
    against pf_face_masks into device outputs (labels, owners, boxes, valid) after every call; the landmarks must be bit-identical.

Both sides of each comparison run interleaved, --repeats times; every repetition is reported.  Writes
profiles/face_masks_bench.json and prints the same JSON line.

    python tools/bench_face_masks.py [--frames 48] [--mask-frames 96] [--iters 10] [--repeats 2] [--ablate-library PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S = 112


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=48, help="1080p frames per pf_run_frames call (8 faces each)")
    ap.add_argument("--mask-frames", type=int, default=96, help="frames of the kernel measurement (8 faces each)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--ablate-library", default=None, help="tool build of the engine (default: build it, flavour 'ablate')")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_masks_bench.json"))
    return ap.parse_args()


def face_landmarks(layout, box, roll_deg, rng):
    """The fixed 98-point layout of tests/align_ref.py on a planted box: interocular distance 0.42 box widths, rolled about the
    box centre, one pixel of jitter."""
    cx, cy, s = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2, 0.42 * (box[2] - box[0]) / 0.84
    c, sn = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
    out = np.stack([cx + s * (c * layout[:, 0] - sn * layout[:, 1]), cy + s * (sn * layout[:, 0] + c * layout[:, 1])], axis=1)
    return (out + rng.uniform(-1.0, 1.0, out.shape)).astype(np.float32)


def main():
    args = parse_args()
    import torch
    from oracle import synth_weights as sw
    from peppa_pig_face_landmark_amd import _native, build
    from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
    from peppa_pig_face_landmark_amd.graph.student import build_student_program
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
    from tests.align_ref import layout98

    dev = torch.device("cuda:0")
    K, H, W, R = 8, 1080, 1920, 15120
    Fp, Fm = args.frames, args.mask_frames
    rng = np.random.default_rng(1)
    layout = layout98()
    fr, rows, kps = [], [], []
    for f in range(max(Fp, Fm)):
        frame, boxes = make_frame(H, W, K, seed=100 + f)
        if f < Fp:
            fr.append(frame)
            rows.append(plant_rows(boxes, (H, W), R, (384, 640), 24, seed=100 + f))
        kps.append(np.stack([face_landmarks(layout, b, rng.uniform(-30, 30), rng) for b in boxes]))
    d_frames = torch.from_numpy(np.stack(fr)).to(dev)
    d_rows = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)
    d_kps = torch.from_numpy(np.stack(kps)[:Fm]).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "chip_size": S, "faces_per_frame": K, "frame": [H, W]}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]

    def memset_ms(t):
        """hipMemsetAsync over the tensor's bytes on the null stream, between two events: ms per call."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            assert hip.hipMemsetAsync(t.data_ptr(), 0, t.numel(), None) == 0
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    def mask(e, space, d_labels, d_valid):
        rc = e.lib.pf_mask_faces(e.h, Fm, H, W, C.c_void_p(d_kps.data_ptr()), 0, _native.PF_MEM_DEVICE, None, K, S if space == "chip" else 0,
                                 C.c_void_p(d_labels.data_ptr()), None, None, C.c_void_p(d_valid.data_ptr()), _native.PF_MEM_DEVICE)
        e._check(rc, "pf_mask_faces")

    def kernel_ms(e, space, d_labels, d_valid):
        e.profile_enable(True)
        for _ in range(args.iters):
            mask(e, space, d_labels, d_valid)
        e.sync()
        prof = e.profile_fetch()
        e.profile_enable(False)
        return {k: round(prof[k][0] / prof[k][1], 4) for k in ("mask_edges", "mask_fill")}

    shapes = {"frame": (Fm, H, W), "chip": (Fm * K, S, S)}
    d_valid = torch.zeros((Fm * K,), dtype=torch.int32, device=dev)

    # ---- 1. the kernels against hipMemsetAsync over the same bytes, interleaved ---------------------------------------------------
    eng = _native.Engine(0)
    for space, shape in shapes.items():
        d_labels = torch.full(shape, 0xAB, dtype=torch.uint8, device=dev)
        sec = {"maps": shape[0], "label_bytes": int(d_labels.numel()), "ms_mask_edges": [], "ms_mask_fill": [], "ms_memset": []}
        for _ in range(args.warmup):
            mask(eng, space, d_labels, d_valid)
            eng.sync()
            memset_ms(d_labels)
        for _ in range(args.repeats):
            ms = kernel_ms(eng, space, d_labels, d_valid)
            sec["ms_mask_edges"].append(ms["mask_edges"])
            sec["ms_mask_fill"].append(ms["mask_fill"])
            sec["ms_memset"].append(round(memset_ms(d_labels), 4))
        mask(eng, space, d_labels, d_valid)
        eng.sync()
        assert int(d_valid.sum().item()) == Fm * K
        sec["labelled_fraction"] = round(float((d_labels != 0).float().mean().item()), 4)
        sec["fill_over_memset"] = round(min(sec["ms_mask_fill"]) / min(sec["ms_memset"]), 2)
        sec["label_GBps_fill"] = round(sec["label_bytes"] / (min(sec["ms_mask_fill"]) * 1e-3) / 1e9, 1)
        result[space + "_space"] = sec
    eng.close()

    # ---- 2. culled (as built) against every slot in every tile, two handles of the tool build ------------------------------------
    lib = args.ablate_library or build.build_hip(flavour="ablate")
    engines = {}
    for name, knob in (("culled", None), ("unculled", "1")):
        os.environ.pop("PEPPA_MASK_NOCULL", None)
        if knob is not None:
            os.environ["PEPPA_MASK_NOCULL"] = knob
        engines[name] = _native.Engine(0, lib)            # the knob is read when the handle is created
    os.environ.pop("PEPPA_MASK_NOCULL", None)
    result["culling"] = {}
    for space, shape in shapes.items():
        d_labels = {k: torch.full(shape, 0xAB, dtype=torch.uint8, device=dev) for k in engines}
        sec = {"ms_fill_culled": [], "ms_fill_unculled": []}
        for name, e in engines.items():
            for _ in range(args.warmup):
                mask(e, space, d_labels[name], d_valid)
            e.sync()
        for _ in range(args.repeats):
            for name, e in engines.items():
                sec["ms_fill_" + name].append(kernel_ms(e, space, d_labels[name], d_valid)["mask_fill"])
        assert torch.equal(d_labels["culled"], d_labels["unculled"]), "both forms must give the same bytes"
        sec["unculled_over_culled"] = round(min(sec["ms_fill_unculled"]) / min(sec["ms_fill_culled"]), 3)
        result["culling"][space + "_space"] = sec
    for e in engines.values():
        e.close()

    # ---- 3. pipeline: masks off / on (device outputs after every call), interleaved ----------------------------------------------
    eng = _native.Engine(0)
    eng.load_program(_native.PF_NET_LANDMARK, build_student_program(sw.student_weights(), 256, "f32s")[0], Fp * K)
    eng.load_program(_native.PF_NET_DETECTOR, build_detector_program(sw.detector_weights(), (384, 640), "f32s")[0], Fp)
    outs = [torch.empty(s, dtype=dt, device=dev) for s, dt in (((Fp,), torch.int32), ((Fp, K, 4), torch.float32),
                                                                ((Fp, K, 98, 2), torch.float32), ((Fp, K, 98), torch.float32))]
    m_lab = torch.zeros((Fp, H, W), dtype=torch.uint8, device=dev)
    m_own = torch.zeros((Fp, H, W), dtype=torch.uint8, device=dev)
    m_box = torch.zeros((Fp * K, 4), dtype=torch.int32, device=dev)
    m_valid = torch.zeros((Fp * K,), dtype=torch.int32, device=dev)

    def pipe(on):
        eng.run_frames_device(d_frames.data_ptr(), Fp, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=R,
                              d_counts=outs[0].data_ptr(), d_boxes=outs[1].data_ptr(), d_kps=outs[2].data_ptr(), d_scores=outs[3].data_ptr())
        if on:
            eng.face_masks_device(Fp * K, 0, m_lab.data_ptr(), m_own.data_ptr(), m_box.data_ptr(), m_valid.data_ptr())
        eng.sync()

    kps_seen = {}
    for _ in range(args.warmup):
        for on in (False, True):
            pipe(on)
            kps_seen[on] = outs[2].clone()
    assert torch.equal(kps_seen[False].view(torch.int32), kps_seen[True].view(torch.int32)), "landmarks must be bit-identical"
    sec = {"frames_per_call": Fp, "valid_masks_per_call": int(m_valid.sum().item()), "landmarks_bit_identical": True,
           "labelled_fraction": round(float((m_lab != 0).float().mean().item()), 4), "faces_per_s_off": [], "faces_per_s_on": []}
    for _ in range(args.repeats):
        for on in (False, True):
            t0 = time.perf_counter()
            for _ in range(args.iters):
                pipe(on)
            s = (time.perf_counter() - t0) / args.iters
            sec["faces_per_s_on" if on else "faces_per_s_off"].append(round(Fp * K / s, 1))
    sec["on_over_off"] = round(max(sec["faces_per_s_on"]) / max(sec["faces_per_s_off"]), 4)
    result["pipeline"] = sec
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

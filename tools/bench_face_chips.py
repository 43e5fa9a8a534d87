"""Cost of the aligned face chips (pf_face_chips / pf_align_faces, csrc/k_align.h), in one process on one device.

  * pf_run_frames on 1080p synthetic frames with 8 planted faces each (Student f32s@256, detector running, top_k 8): chips off
    against chips on at S = 112 with the chip rows copied out to the host (pf_face_chips, host outputs);
  * align_warp (pf_profile_fetch) per 768 faces at S = 112, once as built and once with the LDS budget forced to 0 so that every tile
    takes the direct path.  The budget is a knob of the TOOL build only (libpeppa_hip_ablate.so reads PEPPA_ALIGN_LDS when a handle
    is created; the production library has no such switch), so this half runs two handles of that library.

Both sides of each comparison run interleaved, --repeats times; every repetition is reported.  Writes
profiles/face_chips_bench.json and prints the same JSON line.

    python tools/bench_face_chips.py [--frames 48] [--iters 10] [--repeats 2] [--ablate-library PATH]
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
    ap.add_argument("--warp-faces", type=int, default=768)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--ablate-library", default=None, help="tool build of the engine (default: build it, flavour 'ablate')")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_chips_bench.json"))
    return ap.parse_args()


def face_landmarks(box, roll_deg, rng):
    """98 points for a planted box: the 19 the fit reads (eye rings 60..75, nose tip 54, mouth corners 76 / 82) laid out on the face
    with an interocular distance of 0.42 box widths (scale to a 112 chip about 0.42), rolled about the box centre; the rest at the centre."""
    cx, cy, w = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2, box[2] - box[0]
    c, s = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
    L = np.zeros((98, 2))
    for i in range(8):
        t = 2 * math.pi * i / 8
        L[60 + i] = (-0.21 + 0.08 * math.cos(t), -0.15 + 0.035 * math.sin(t))
        L[68 + i] = (0.21 + 0.08 * math.cos(t), -0.15 + 0.035 * math.sin(t))
    L[54], L[76], L[82] = (0.0, 0.05), (-0.16, 0.26), (0.16, 0.26)
    L *= w
    out = np.stack([cx + c * L[:, 0] - s * L[:, 1], cy + s * L[:, 0] + c * L[:, 1]], axis=1)
    return (out + rng.uniform(-1.0, 1.0, out.shape)).astype(np.float32)


def main():
    args = parse_args()
    import torch
    from oracle import synth_weights as sw
    from peppa_pig_face_landmark_amd import _native, build
    from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
    from peppa_pig_face_landmark_amd.graph.student import build_student_program
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows

    dev = torch.device("cuda:0")
    K, H, W, R = 8, 1080, 1920, 15120
    F = max(args.frames, (args.warp_faces + K - 1) // K)
    rng = np.random.default_rng(1)
    fr, rows, kps = [], [], []
    for f in range(F):
        frame, boxes = make_frame(H, W, K, seed=100 + f)
        fr.append(frame)
        rows.append(plant_rows(boxes, (H, W), R, (384, 640), 24, seed=100 + f))
        kps.append(np.stack([face_landmarks(b, rng.uniform(-30, 30), rng) for b in boxes]))
    d_frames = torch.from_numpy(np.stack(fr)).to(dev)
    d_rows = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)
    d_kps = torch.from_numpy(np.stack(kps)).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "chip_size": S, "faces_per_frame": K, "frame": [H, W]}

    # ---- 1. pipeline: chips off / on, interleaved ------------------------------------------------------------------------------
    Fp = args.frames
    eng = _native.Engine(0)
    eng.load_program(_native.PF_NET_LANDMARK, build_student_program(sw.student_weights(), 256, "f32s")[0], Fp * K)
    eng.load_program(_native.PF_NET_DETECTOR, build_detector_program(sw.detector_weights(), (384, 640), "f32s")[0], Fp)
    outs = [torch.empty(s, dtype=dt, device=dev) for s, dt in (((Fp,), torch.int32), ((Fp, K, 4), torch.float32),
                                                                ((Fp, K, 98, 2), torch.float32), ((Fp, K, 98), torch.float32))]
    chips, mats = np.zeros((Fp * K, S, S, 3), np.uint8), np.zeros((Fp * K, 2, 3), np.float64)

    def pipe(on):
        eng.run_frames_device(d_frames.data_ptr(), Fp, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=R,
                              d_counts=outs[0].data_ptr(), d_boxes=outs[1].data_ptr(), d_kps=outs[2].data_ptr(), d_scores=outs[3].data_ptr())
        if on:
            return eng.face_chips(Fp * K, S, out=(chips, mats))[2]
        eng.sync()
        return None

    for _ in range(args.warmup):
        pipe(False)
        valid = pipe(True)
    result["pipeline"] = {"frames_per_call": Fp, "valid_chips_per_call": int(valid.sum()), "faces_per_s_off": [], "faces_per_s_on": []}
    for _ in range(args.repeats):
        for on in (False, True):
            t0 = time.perf_counter()
            for _ in range(args.iters):
                pipe(on)
            s = (time.perf_counter() - t0) / args.iters
            result["pipeline"]["faces_per_s_on" if on else "faces_per_s_off"].append(round(Fp * K / s, 1))
    result["pipeline"]["on_over_off"] = round(max(result["pipeline"]["faces_per_s_on"]) / max(result["pipeline"]["faces_per_s_off"]), 4)
    eng.close()

    # ---- 2. align_warp: tiled (as built) against direct (LDS budget 0), two handles of the tool build --------------------------
    lib = args.ablate_library or build.build_hip(flavour="ablate")
    n = args.warp_faces
    Fw = n // K
    engines = {}
    for name, budget in (("tiled", None), ("direct", "0")):
        os.environ.pop("PEPPA_ALIGN_LDS", None)
        if budget is not None:
            os.environ["PEPPA_ALIGN_LDS"] = budget
        engines[name] = _native.Engine(0, lib)            # the knob is read when the handle is created
    os.environ.pop("PEPPA_ALIGN_LDS", None)
    d_chips = {k: torch.zeros((Fw * K, S, S, 3), dtype=torch.uint8, device=dev) for k in engines}
    d_valid = torch.zeros((Fw * K,), dtype=torch.int32, device=dev)

    def warp(name):
        e = engines[name]
        rc = e.lib.pf_align_faces(e.h, C.c_void_p(d_frames.data_ptr()), _native.PF_MEM_DEVICE, Fw, H, W, C.c_void_p(d_kps.data_ptr()), 0,
                                  _native.PF_MEM_DEVICE, None, K, S, C.c_void_p(d_chips[name].data_ptr()), None,
                                  C.c_void_p(d_valid.data_ptr()), _native.PF_MEM_DEVICE)
        e._check(rc, "pf_align_faces")

    result["align_warp"] = {"faces": Fw * K, "ms_tiled": [], "ms_direct": [], "ms_fit": []}
    for name in engines:
        for _ in range(args.warmup):
            warp(name)
        engines[name].sync()
    for _ in range(args.repeats):
        for name in ("tiled", "direct"):
            e = engines[name]
            e.profile_enable(True)
            for _ in range(args.iters):
                warp(name)
            e.sync()
            prof = e.profile_fetch()
            e.profile_enable(False)
            result["align_warp"]["ms_" + name].append(round(prof["align_warp"][0] / prof["align_warp"][1], 4))
            if name == "tiled":
                result["align_warp"]["ms_fit"].append(round(prof["align_fit"][0] / prof["align_fit"][1], 4))
    assert int(d_valid.sum().item()) == Fw * K
    assert torch.equal(d_chips["tiled"], d_chips["direct"]), "the two paths must give the same bytes"
    aw = result["align_warp"]
    aw["direct_over_tiled"] = round(min(aw["ms_direct"]) / min(aw["ms_tiled"]), 3)
    moved = Fw * K * S * S * 3                       # chip bytes written
    aw["chip_GBps_tiled"] = round(moved / (min(aw["ms_tiled"]) * 1e-3) / 1e9, 1)
    for e in engines.values():
        e.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

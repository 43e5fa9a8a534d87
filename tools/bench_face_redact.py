"""Cost of the face redaction (pf_redact_faces / pf_face_redact, csrc/k_redact.h), in one process on one device.

  * redact_kernel (pf_profile_fetch) for 96 frames of 1080p with 8 planted faces each, per mode -- fill, mosaic 16, blur 8, blur 32 --
    beside hipMemcpyAsync device-to-device over the same frame bytes, the floor of an out-of-place pass that reads and writes every
    byte once, and beside mask_edges + mask_fill, which the redaction always pays first;
  * the same with every tile staged through LDS instead of copying the tiles that hold no selected pixel.  That is a knob of the TOOL
    build only (libpeppa_hip_ablate.so reads PEPPA_REDACT_STAGE_ALL when a handle is created; the production library has no such
    switch), so this half runs two handles of that library and checks that both give the same bytes;
  * pf_run_frames on 1080p synthetic frames with 8 planted faces each (Student f32s@256, detector running, top_k 8): without
    redaction against pf_face_redact (mosaic 16) into a device buffer after every call; the landmarks must be bit-identical.

Both sides of each comparison run interleaved, --repeats times; every repetition is reported.  Writes
profiles/face_redact_bench.json and prints the same JSON line.

    python tools/bench_face_redact.py [--frames 48] [--redact-frames 96] [--iters 10] [--repeats 2] [--ablate-library PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = [("fill", 0, 0), ("mosaic16", 1, 16), ("blur8", 2, 8), ("blur32", 2, 32)]      # name, mode, strength


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=48, help="1080p frames per pf_run_frames call (8 faces each)")
    ap.add_argument("--redact-frames", type=int, default=96, help="frames of the kernel measurement (8 faces each)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--ablate-library", default=None, help="tool build of the engine (default: build it, flavour 'ablate')")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_redact_bench.json"))
    return ap.parse_args()


def main():
    args = parse_args()
    import torch
    from oracle import synth_weights as sw
    from peppa_pig_face_landmark_amd import _native, build
    from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
    from peppa_pig_face_landmark_amd.graph.student import build_student_program
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
    from tests.align_ref import layout98
    from tools.bench_face_masks import face_landmarks

    dev = torch.device("cuda:0")
    K, H, W, R = 8, 1080, 1920, 15120
    Fp, Fm = args.frames, args.redact_frames
    rng = np.random.default_rng(1)
    layout = layout98()
    fr, rows, kps = [], [], []
    for f in range(max(Fp, Fm)):
        frame, boxes = make_frame(H, W, K, seed=100 + f)
        fr.append(frame)
        if f < Fp:
            rows.append(plant_rows(boxes, (H, W), R, (384, 640), 24, seed=100 + f))
        kps.append(np.stack([face_landmarks(layout, b, rng.uniform(-30, 30), rng) for b in boxes]))
    d_frames = torch.from_numpy(np.stack(fr)).to(dev)
    d_rows = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)
    d_kps = torch.from_numpy(np.stack(kps)[:Fm]).to(dev)
    del fr
    frame_bytes = Fm * H * W * 3
    result = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "faces_per_frame": K, "frame": [H, W],
              "frames": Fm, "frame_bytes": frame_bytes, "label_mask": "0x1FE"}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    d_out = torch.full((Fm, H, W, 3), 0xAB, dtype=torch.uint8, device=dev)

    def memcpy_ms():
        """hipMemcpyAsync device-to-device over the frame bytes on the null stream, between two events: ms per call."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            assert hip.hipMemcpyAsync(d_out.data_ptr(), d_frames.data_ptr(), frame_bytes, 3, None) == 0
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    def redact(e, mode, strength, out):
        rc = e.lib.pf_redact_faces(e.h, C.c_void_p(d_frames.data_ptr()), _native.PF_MEM_DEVICE, Fm, H, W, C.c_void_p(d_kps.data_ptr()), 0,
                                   _native.PF_MEM_DEVICE, None, None, K, mode, 0x1FE, strength, 0, C.c_uint(0), C.c_void_p(out.data_ptr()),
                                   None, _native.PF_MEM_DEVICE)
        e._check(rc, "pf_redact_faces")

    def kernel_ms(e, mode, strength, out):
        e.profile_enable(True)
        for _ in range(args.iters):
            redact(e, mode, strength, out)
        e.sync()
        prof = e.profile_fetch()
        e.profile_enable(False)
        return {k: round(prof[k][0] / prof[k][1], 4) for k in ("mask_edges", "mask_fill", "redact")}

    # ---- 1. the kernel against hipMemcpyAsync over the same bytes and against the label maps, interleaved -------------------------
    eng = _native.Engine(0)
    result["modes"] = {}
    for name, mode, strength in MODES:
        sec = {"ms_redact": [], "ms_mask_edges": [], "ms_mask_fill": [], "ms_memcpy_d2d": []}
        for _ in range(args.warmup):
            redact(eng, mode, strength, d_out)
            eng.sync()
            memcpy_ms()
        for _ in range(args.repeats):
            ms = kernel_ms(eng, mode, strength, d_out)
            sec["ms_redact"].append(ms["redact"])
            sec["ms_mask_edges"].append(ms["mask_edges"])
            sec["ms_mask_fill"].append(ms["mask_fill"])
            sec["ms_memcpy_d2d"].append(round(memcpy_ms(), 4))
        redact(eng, mode, strength, d_out)
        eng.sync()
        sec["changed_pixel_fraction"] = round(float((d_out != d_frames[:Fm]).any(dim=3).float().mean().item()), 4)
        best = min(sec["ms_redact"])
        sec["redact_over_memcpy"] = round(best / min(sec["ms_memcpy_d2d"]), 3)
        sec["redact_over_masks"] = round(best / (min(sec["ms_mask_edges"]) + min(sec["ms_mask_fill"])), 2)
        sec["mask_fill_share_of_call"] = round(min(sec["ms_mask_fill"]) / (best + min(sec["ms_mask_edges"]) + min(sec["ms_mask_fill"])), 4)
        sec["GBps_read_plus_written"] = round(2 * frame_bytes / (best * 1e-3) / 1e9, 1)
        result["modes"][name] = sec
    eng.close()

    # ---- 2. tiles without a selected pixel copied (as built) against every tile staged through LDS, two handles of the tool build -
    lib = args.ablate_library or build.build_hip(flavour="ablate")
    engines = {}
    for name, knob in (("copy_tiles", None), ("stage_all", "1")):
        os.environ.pop("PEPPA_REDACT_STAGE_ALL", None)
        if knob is not None:
            os.environ["PEPPA_REDACT_STAGE_ALL"] = knob
        engines[name] = _native.Engine(0, lib)            # the knob is read when the handle is created
    os.environ.pop("PEPPA_REDACT_STAGE_ALL", None)
    outs2 = {"copy_tiles": d_out, "stage_all": torch.full((Fm, H, W, 3), 0xAB, dtype=torch.uint8, device=dev)}
    result["variants"] = {}
    for name, mode, strength in MODES:
        sec = {"ms_redact_copy_tiles": [], "ms_redact_stage_all": []}
        for vn, e in engines.items():
            for _ in range(args.warmup):
                redact(e, mode, strength, outs2[vn])
            e.sync()
        for _ in range(args.repeats):
            for vn, e in engines.items():
                sec["ms_redact_" + vn].append(kernel_ms(e, mode, strength, outs2[vn])["redact"])
        assert torch.equal(outs2["copy_tiles"], outs2["stage_all"]), "both forms must give the same bytes"
        sec["stage_all_over_copy_tiles"] = round(min(sec["ms_redact_stage_all"]) / min(sec["ms_redact_copy_tiles"]), 3)
        result["variants"][name] = sec
    for e in engines.values():
        e.close()
    del outs2, d_out

    # ---- 3. pipeline: redaction off / on (device output after every call), interleaved ---------------------------------------------
    eng = _native.Engine(0)
    eng.load_program(_native.PF_NET_LANDMARK, build_student_program(sw.student_weights(), 256, "f32s")[0], Fp * K)
    eng.load_program(_native.PF_NET_DETECTOR, build_detector_program(sw.detector_weights(), (384, 640), "f32s")[0], Fp)
    outs = [torch.empty(s, dtype=dt, device=dev) for s, dt in (((Fp,), torch.int32), ((Fp, K, 4), torch.float32),
                                                                ((Fp, K, 98, 2), torch.float32), ((Fp, K, 98), torch.float32))]
    r_out = torch.zeros((Fp, H, W, 3), dtype=torch.uint8, device=dev)
    r_valid = torch.zeros((Fp * K,), dtype=torch.int32, device=dev)

    def pipe(on):
        eng.run_frames_device(d_frames.data_ptr(), Fp, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=R,
                              d_counts=outs[0].data_ptr(), d_boxes=outs[1].data_ptr(), d_kps=outs[2].data_ptr(), d_scores=outs[3].data_ptr())
        if on:
            eng.face_redact_device(Fp * K, r_out.data_ptr(), mode="mosaic", strength=16, d_valid=r_valid.data_ptr())
        eng.sync()

    kps_seen = {}
    for _ in range(args.warmup):
        for on in (False, True):
            pipe(on)
            kps_seen[on] = outs[2].clone()
    assert torch.equal(kps_seen[False].view(torch.int32), kps_seen[True].view(torch.int32)), "landmarks must be bit-identical"
    sec = {"frames_per_call": Fp, "mode": "mosaic16", "valid_faces_per_call": int(r_valid.sum().item()), "landmarks_bit_identical": True,
           "changed_pixel_fraction": round(float((r_out != d_frames[:Fp]).any(dim=3).float().mean().item()), 4),
           "faces_per_s_off": [], "faces_per_s_on": []}
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

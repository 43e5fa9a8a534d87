"""Cost of the face overlay (pf_draw_faces / pf_face_draw, csrc/k_draw.h), in one process on one device.

  * draw_prims_kernel and draw_kernel (pf_profile_fetch) for 96 frames of 1080p with 8 planted faces each, points only and points +
    contours + box, beside hipMemcpyAsync device-to-device over the same frame bytes -- the floor of an out-of-place pass that reads
    and writes every byte once -- and beside redact_kernel in fill mode, the nearest existing kernel (k_redact.h is byte for byte the
    parent commit's), run in the same process;
  * the same with tile culling disabled: every tile stages its pixels and lists every primitive of its image.  That is a knob of the
    TOOL build only (libpeppa_hip_ablate.so reads PEPPA_DRAW_NOCULL when a handle is created; the production library has no such
    switch), so this half runs two handles of that library and checks that both give the same bytes;
  * pf_run_frames on 1080p synthetic frames with 8 planted faces each (Student f32s@256, detector running, top_k 8), timed three
    ways: alone; with pf_face_draw + pf_encode_jpeg to device memory and only the files copied out; with the raw drawn frames copied
    out.  The landmarks must be bit-identical.

Both sides of each comparison run interleaved, --repeats times; every repetition is reported.  Writes
profiles/face_draw_bench.json and prints the same JSON line.

    python tools/bench_face_draw.py [--frames 48] [--draw-frames 96] [--iters 10] [--repeats 2] [--ablate-library PATH]
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

WHATS = [("points", 1), ("points_contours_box", 7)]


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=48, help="1080p frames per pf_run_frames call (8 faces each)")
    ap.add_argument("--draw-frames", type=int, default=96, help="frames of the kernel measurement (8 faces each)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--nocull-iters", type=int, default=2, help="iterations of the form without culling, which is slow")
    ap.add_argument("--ablate-library", default=None, help="tool build of the engine (default: build it, flavour 'ablate')")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_draw_bench.json"))
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
    Fp, Fm = args.frames, args.draw_frames
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
    d_sc = torch.from_numpy(rng.uniform(0.6, 1.0, (Fm, K, 98)).astype(np.float32)).to(dev)
    del fr
    frame_bytes = Fm * H * W * 3
    result = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "faces_per_frame": K, "frame": [H, W],
              "frames": Fm, "frame_bytes": frame_bytes, "point_radius": 2, "line_width": 1, "alpha": 256}
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

    def draw(e, what, out):
        st = _native._draw_style(what=what)
        rc = e.lib.pf_draw_faces(e.h, C.c_void_p(d_frames.data_ptr()), _native.PF_MEM_DEVICE, Fm, H, W, C.c_void_p(d_kps.data_ptr()), 0,
                                 _native.PF_MEM_DEVICE, None, C.c_void_p(d_sc.data_ptr()), K, C.byref(st), C.c_void_p(out.data_ptr()), None,
                                 _native.PF_MEM_DEVICE)
        e._check(rc, "pf_draw_faces")

    def redact_fill(e, out):
        rc = e.lib.pf_redact_faces(e.h, C.c_void_p(d_frames.data_ptr()), _native.PF_MEM_DEVICE, Fm, H, W, C.c_void_p(d_kps.data_ptr()), 0,
                                   _native.PF_MEM_DEVICE, None, None, K, 0, 0x1FE, 0, 0, C.c_uint(0), C.c_void_p(out.data_ptr()), None,
                                   _native.PF_MEM_DEVICE)
        e._check(rc, "pf_redact_faces")

    def kernel_ms(e, fn, keys, iters):
        e.profile_enable(True)
        for _ in range(iters):
            fn()
        e.sync()
        prof = e.profile_fetch()
        e.profile_enable(False)
        return {k: round(prof[k][0] / prof[k][1], 4) for k in keys}

    # ---- 1. the kernels against hipMemcpyAsync over the same bytes and against redact_kernel (fill), interleaved ---------------------
    eng = _native.Engine(0)
    result["whats"] = {}
    for name, what in WHATS:
        sec = {"ms_draw": [], "ms_draw_prims": [], "ms_memcpy_d2d": [], "ms_redact_fill": []}
        for _ in range(args.warmup):
            draw(eng, what, d_out)
            redact_fill(eng, d_out)
            eng.sync()
            memcpy_ms()
        for _ in range(args.repeats):
            ms = kernel_ms(eng, lambda: draw(eng, what, d_out), ("draw_prims", "draw"), args.iters)
            sec["ms_draw"].append(ms["draw"])
            sec["ms_draw_prims"].append(ms["draw_prims"])
            sec["ms_memcpy_d2d"].append(round(memcpy_ms(), 4))
            sec["ms_redact_fill"].append(kernel_ms(eng, lambda: redact_fill(eng, d_out), ("redact",), args.iters)["redact"])
        draw(eng, what, d_out)
        eng.sync()
        sec["changed_pixel_fraction"] = round(float((d_out != d_frames[:Fm]).any(dim=3).float().mean().item()), 5)
        best = min(sec["ms_draw"])
        sec["draw_over_memcpy"] = round(best / min(sec["ms_memcpy_d2d"]), 3)
        sec["draw_over_redact_fill"] = round(best / min(sec["ms_redact_fill"]), 3)
        sec["prims_share_of_call"] = round(min(sec["ms_draw_prims"]) / (best + min(sec["ms_draw_prims"])), 4)
        sec["GBps_read_plus_written"] = round(2 * frame_bytes / (best * 1e-3) / 1e9, 1)
        result["whats"][name] = sec
    eng.close()

    # ---- 2. tile culling as built against no culling, two handles of the tool build --------------------------------------------------
    lib = args.ablate_library or build.build_hip(flavour="ablate")
    engines = {}
    for name, knob in (("culled", None), ("no_cull", "1")):
        os.environ.pop("PEPPA_DRAW_NOCULL", None)
        if knob is not None:
            os.environ["PEPPA_DRAW_NOCULL"] = knob
        engines[name] = _native.Engine(0, lib)            # the knob is read when the handle is created
    os.environ.pop("PEPPA_DRAW_NOCULL", None)
    outs2 = {"culled": d_out, "no_cull": torch.full((Fm, H, W, 3), 0xAB, dtype=torch.uint8, device=dev)}
    iters2 = {"culled": args.iters, "no_cull": args.nocull_iters}
    result["variants"] = {}
    for name, what in WHATS:
        sec = {"ms_draw_culled": [], "ms_draw_no_cull": []}
        for vn, e in engines.items():
            draw(e, what, outs2[vn])
            e.sync()
        for _ in range(args.repeats):
            for vn, e in engines.items():
                sec["ms_draw_" + vn].append(kernel_ms(e, lambda: draw(e, what, outs2[vn]), ("draw",), iters2[vn])["draw"])
        assert torch.equal(outs2["culled"], outs2["no_cull"]), "both forms must give the same bytes"
        sec["no_cull_over_culled"] = round(min(sec["ms_draw_no_cull"]) / min(sec["ms_draw_culled"]), 2)
        result["variants"][name] = sec
    for e in engines.values():
        e.close()
    del outs2, d_out

    # ---- 3. pipeline: alone / + draw + JPEG on the device, files out / + raw drawn frames out, interleaved --------------------------
    eng = _native.Engine(0)
    eng.load_program(_native.PF_NET_LANDMARK, build_student_program(sw.student_weights(), 256, "f32s")[0], Fp * K)
    eng.load_program(_native.PF_NET_DETECTOR, build_detector_program(sw.detector_weights(), (384, 640), "f32s")[0], Fp)
    outs = [torch.empty(s, dtype=dt, device=dev) for s, dt in (((Fp,), torch.int32), ((Fp, K, 4), torch.float32),
                                                                ((Fp, K, 98, 2), torch.float32), ((Fp, K, 98), torch.float32))]
    r_out = torch.zeros((Fp, H, W, 3), dtype=torch.uint8, device=dev)
    r_valid = torch.zeros((Fp * K,), dtype=torch.int32, device=dev)
    style = dict(what=7)
    file_bytes = [0]

    def pipe(mode):
        """as tools/bench_jpeg_encode.py times the redaction: the files through Engine.encode_jpeg (only they are copied out), the raw
        frames through the host-output accessor"""
        eng.run_frames_device(d_frames.data_ptr(), Fp, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=R,
                              d_counts=outs[0].data_ptr(), d_boxes=outs[1].data_ptr(), d_kps=outs[2].data_ptr(), d_scores=outs[3].data_ptr())
        eng.sync()
        if mode == "alone":
            return
        sc = outs[3].cpu().numpy().reshape(-1, 98)     # the accessor takes the scores from host memory: a caller has just received them
        if mode == "files":
            eng.face_draw_device(Fp * K, r_out.data_ptr(), scores=sc, d_valid=r_valid.data_ptr(), **style)
            files = eng.encode_jpeg((r_out.data_ptr(), Fp, H, W), quality=85, subsampling=420, capacity=3 * H * W // 2)
            file_bytes[0] = sum(len(f) for f in files)
        else:
            eng.face_draw(Fp * K, scores=sc, **style)
        eng.sync()

    kps_seen = {}
    modes = ("alone", "files", "raw")
    for _ in range(args.warmup):
        for m in modes:
            pipe(m)
            kps_seen[m] = outs[2].clone()
    for m in modes[1:]:
        assert torch.equal(kps_seen["alone"].view(torch.int32), kps_seen[m].view(torch.int32)), "landmarks must be bit-identical"
    sec = {"frames_per_call": Fp, "what": "points_contours_box", "valid_faces_per_call": int(r_valid.sum().item()), "landmarks_bit_identical": True,
           "changed_pixel_fraction": round(float((r_out != d_frames[:Fp]).any(dim=3).float().mean().item()), 5),
           "file_bytes_per_call": file_bytes[0], "raw_bytes_per_call": Fp * H * W * 3}
    for m in modes:
        sec["faces_per_s_" + m] = []
    for _ in range(args.repeats):
        for m in modes:
            t0 = time.perf_counter()
            for _ in range(args.iters):
                pipe(m)
            s = (time.perf_counter() - t0) / args.iters
            sec["faces_per_s_" + m].append(round(Fp * K / s, 1))
    sec["files_over_alone"] = round(max(sec["faces_per_s_files"]) / max(sec["faces_per_s_alone"]), 4)
    sec["raw_over_alone"] = round(max(sec["faces_per_s_raw"]) / max(sec["faces_per_s_alone"]), 4)
    result["pipeline"] = sec
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

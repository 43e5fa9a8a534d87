"""Cost of the per-face region statistics (pf_measure_faces / pf_face_stats, csrc/k_stats.h), in one process on one device.

  * face_stats (pf_profile_fetch: face_stats_zero_kernel + face_stats_kernel) for two scenes of 768 faces -- 96 frames of 1080p with
    8 planted faces of 200 x 260 each, and 96 frames of 540 x 960 with 8 faces of 100 x 130 -- beside mask_edges + mask_fill, which
    the statistics always pay first, and beside hipMemcpyAsync device-to-device over 5 bytes per box pixel (3 of the frame, a label,
    an owner), the bytes the kernel must read: the floor;
  * the same beside the other form of the kernel.  Two were written: the direct one (a thread per box pixel, global reads, LDS
    atomics per (label, field)) and the staged one (128 x 16 pieces through LDS, register partials, shuffle reduction).  The faster
    ships as face_stats_kernel; the other is a knob of the TOOL build only (libpeppa_hip_ablate.so reads PEPPA_STATS_STAGED when a
    handle is created; the production library has no such switch), so this half runs two handles of that library and checks that
    both give the same values;
  * the host alternative: the device-to-host copy of the frames, labels and owners, then the numpy restatement's arithmetic
    (tests/stats_ref.py: one weighted bincount per field) on at most 16 host threads, one frame per task;
  * pf_run_frames on 1080p synthetic frames with 8 planted faces each (Student f32s@256, detector running, top_k 8): alone against
    pf_face_stats to HOST memory after every call; the landmarks must be bit-identical.  With --parent-library (the parent commit's
    build of libpeppa_hip.so) the "alone" side also runs on that library, interleaved with the others.

Both sides of each comparison run interleaved, --repeats times; every repetition is reported.  Writes profiles/face_stats_bench.json
and prints the same JSON line.

    python tools/bench_face_stats.py [--frames 48] [--stats-frames 96] [--iters 10] [--repeats 2] [--ablate-library PATH]
                                     [--parent-library PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCENES = [("1080p_200x260", 1080, 1920, 200, 260), ("540p_100x130", 540, 960, 100, 130)]      # name, H, W, face_w, face_h


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=48, help="1080p frames per pf_run_frames call (8 faces each)")
    ap.add_argument("--stats-frames", type=int, default=96, help="frames of the kernel measurement (8 faces each)")
    ap.add_argument("--host-frames", type=int, default=16, help="frames of the host alternative")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--ablate-library", default=None, help="tool build of the engine (default: build it, flavour 'ablate')")
    ap.add_argument("--parent-library", default=None, help="the parent commit's libpeppa_hip.so for the pipeline's 'alone' side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_stats_bench.json"))
    return ap.parse_args()


def main():
    args = parse_args()
    import torch
    from oracle import synth_weights as sw
    from peppa_pig_face_landmark_amd import _native, build
    from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
    from peppa_pig_face_landmark_amd.graph.student import build_student_program
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
    from tests import stats_ref as sr
    from tests.align_ref import layout98
    from tools.bench_face_masks import face_landmarks

    dev = torch.device("cuda:0")
    K, R = 8, 15120
    Fp, Fm, Fh = args.frames, args.stats_frames, min(args.host_frames, args.stats_frames)
    layout = layout98()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    result = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "faces_per_frame": K, "frames": Fm,
              "thresholds": [16, 240], "scenes": {}, "variants": {}}

    def measure(e, d_frames, d_kps, H, W, out):
        rc = e.lib.pf_measure_faces(e.h, C.c_void_p(d_frames.data_ptr()), _native.PF_MEM_DEVICE, Fm, H, W, C.c_void_p(d_kps.data_ptr()), 0,
                                    _native.PF_MEM_DEVICE, None, K, 16, 240, C.c_void_p(out.data_ptr()), None, _native.PF_MEM_DEVICE)
        e._check(rc, "pf_measure_faces")

    def kernel_ms(e, call):
        e.profile_enable(True)
        for _ in range(args.iters):
            call()
        e.sync()
        prof = e.profile_fetch()
        e.profile_enable(False)
        return {k: round(prof[k][0] / prof[k][1], 4) for k in ("mask_edges", "mask_fill", "face_stats")}

    def memcpy_ms(dst, src, nbytes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None) == 0
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    lib_ablate = args.ablate_library or build.build_hip(flavour="ablate")
    pipe_scene = None
    for name, H, W, fw, fh in SCENES:
        rng = np.random.default_rng(1)
        fr, rows, kps = [], [], []
        for f in range(max(Fp, Fm) if H == 1080 else Fm):
            frame, boxes = make_frame(H, W, K, seed=100 + f, face_w=fw, face_h=fh)
            fr.append(frame)
            if H == 1080 and f < Fp:
                rows.append(plant_rows(boxes, (H, W), R, (384, 640), 24, seed=100 + f))
            kps.append(np.stack([face_landmarks(layout, b, rng.uniform(-30, 30), rng) for b in boxes]))
        h_frames, h_kps = np.stack(fr), np.stack(kps)[:Fm]
        del fr
        d_frames = torch.from_numpy(h_frames).to(dev)
        d_kps = torch.from_numpy(h_kps).to(dev)
        d_stats = torch.full((Fm, K, 8, 9), -1, dtype=torch.int64, device=dev)

        # ---- 1. the kernel against the label maps it pays first and against hipMemcpyAsync over the bytes it must read ------------
        eng = _native.Engine(0)
        boxes_px = eng.mask_faces(h_kps, H, W)[2].astype(np.int64)
        box_pixels = int(((boxes_px[..., 2] - boxes_px[..., 0]) * (boxes_px[..., 3] - boxes_px[..., 1])).sum())
        floor_bytes = 5 * box_pixels
        src = torch.empty((floor_bytes,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        call = lambda: measure(eng, d_frames, d_kps, H, W, d_stats)
        sec = {"frame": [H, W], "face": [fw, fh], "box_pixels": box_pixels, "floor_bytes": floor_bytes, "ms_face_stats": [],
               "ms_mask_edges": [], "ms_mask_fill": [], "ms_memcpy_d2d_floor": []}
        for _ in range(args.warmup):
            call()
            eng.sync()
            memcpy_ms(dst, src, floor_bytes)
        for _ in range(args.repeats):
            ms = kernel_ms(eng, call)
            sec["ms_face_stats"].append(ms["face_stats"])
            sec["ms_mask_edges"].append(ms["mask_edges"])
            sec["ms_mask_fill"].append(ms["mask_fill"])
            sec["ms_memcpy_d2d_floor"].append(round(memcpy_ms(dst, src, floor_bytes), 4))
        eng.sync()
        got = d_stats.cpu().numpy().view(np.uint64)
        sec["labelled_pixels"] = int(got[..., 0].sum())
        best = min(sec["ms_face_stats"])
        sec["stats_over_memcpy_floor"] = round(best / min(sec["ms_memcpy_d2d_floor"]), 2)
        sec["stats_over_masks"] = round(best / (min(sec["ms_mask_edges"]) + min(sec["ms_mask_fill"])), 3)
        sec["stats_share_of_call"] = round(best / (best + min(sec["ms_mask_edges"]) + min(sec["ms_mask_fill"])), 4)
        sec["GBps_over_floor_bytes"] = round(floor_bytes / (best * 1e-3) / 1e9, 1)
        del src, dst

        # ---- 2. the host alternative: copy frames, labels and owners out, numpy arithmetic on at most 16 threads -------------------
        d_lab = torch.empty((Fm, H, W), dtype=torch.uint8, device=dev)
        d_own = torch.empty_like(d_lab)
        rc = eng.lib.pf_mask_faces(eng.h, Fm, H, W, C.c_void_p(d_kps.data_ptr()), 0, _native.PF_MEM_DEVICE, None, K, 0, C.c_void_p(d_lab.data_ptr()),
                                   C.c_void_p(d_own.data_ptr()), None, None, _native.PF_MEM_DEVICE)
        eng._check(rc, "pf_mask_faces")
        eng.sync()
        sec["host_frames"] = Fh
        sec["ms_host_copy_per_frame"], sec["ms_host_numpy_per_frame"] = [], []
        valid = np.ones((K,), bool)
        pool = ThreadPoolExecutor(max_workers=min(16, Fh))
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hf, hl, ho = d_frames[:Fh].cpu().numpy(), d_lab[:Fh].cpu().numpy(), d_own[:Fh].cpu().numpy()
            t1 = time.perf_counter()
            host = list(pool.map(lambda f: sr.frame_stats(hf[f], (hl[f], ho[f], None, valid)), range(Fh)))
            t2 = time.perf_counter()
            sec["ms_host_copy_per_frame"].append(round((t1 - t0) * 1e3 / Fh, 3))
            sec["ms_host_numpy_per_frame"].append(round((t2 - t1) * 1e3 / Fh, 3))
        pool.shutdown()
        assert np.array_equal(np.stack(host), got[:Fh]), "the host alternative must give the device's values"
        sec["host_over_device_call"] = round((min(sec["ms_host_copy_per_frame"]) + min(sec["ms_host_numpy_per_frame"])) * Fm /
                                             (best + min(sec["ms_mask_edges"]) + min(sec["ms_mask_fill"])), 1)
        eng.close()
        del d_lab, d_own
        result["scenes"][name] = sec

        # ---- 3. as built against the staged form, two handles of the tool build -------- --------------------------------------------
        engines = {}
        for vn, knob in (("shipped", None), ("staged", "1")):
            os.environ.pop("PEPPA_STATS_STAGED", None)
            if knob is not None:
                os.environ["PEPPA_STATS_STAGED"] = knob
            engines[vn] = _native.Engine(0, lib_ablate)       # the knob is read when the handle is created
        os.environ.pop("PEPPA_STATS_STAGED", None)
        outs = {"shipped": d_stats, "staged": torch.full_like(d_stats, -1)}
        var = {"ms_face_stats_shipped": [], "ms_face_stats_staged": []}
        for vn, e in engines.items():
            for _ in range(args.warmup):
                measure(e, d_frames, d_kps, H, W, outs[vn])
            e.sync()
        for _ in range(args.repeats):
            for vn, e in engines.items():
                var["ms_face_stats_" + vn].append(kernel_ms(e, lambda: measure(e, d_frames, d_kps, H, W, outs[vn]))["face_stats"])
        assert torch.equal(outs["shipped"], outs["staged"]), "both forms must give the same values"
        assert np.array_equal(outs["shipped"].cpu().numpy().view(np.uint64), got), "the tool build must give the production library's values"
        var["identical_values"] = True
        var["staged_over_shipped"] = round(min(var["ms_face_stats_staged"]) / min(var["ms_face_stats_shipped"]), 3)
        result["variants"][name] = var
        for e in engines.values():
            e.close()
        if H == 1080:
            pipe_scene = (d_frames, torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev), H, W)
        del outs, d_stats

    # ---- 4. pipeline: alone / with pf_face_stats to host after every call (/ alone on the parent's build), interleaved --------------
    d_frames, d_rows, H, W = pipe_scene
    blobs = (build_student_program(sw.student_weights(), 256, "f32s")[0], build_detector_program(sw.detector_weights(), (384, 640), "f32s")[0])
    sides = {"alone": None, "with_stats": None}
    if args.parent_library:
        sides["alone_parent"] = args.parent_library
    engines, outs = {}, {}
    for side, lib in sides.items():
        e = _native.Engine(0, lib)
        e.load_program(_native.PF_NET_LANDMARK, blobs[0], Fp * K)
        e.load_program(_native.PF_NET_DETECTOR, blobs[1], Fp)
        engines[side] = e
        outs[side] = [torch.empty(s, dtype=dt, device=dev) for s, dt in (((Fp,), torch.int32), ((Fp, K, 4), torch.float32),
                                                                         ((Fp, K, 98, 2), torch.float32), ((Fp, K, 98), torch.float32))]
    seen = {}

    def pipe(side):
        e, o = engines[side], outs[side]
        e.run_frames_device(d_frames.data_ptr(), Fp, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=R,
                            d_counts=o[0].data_ptr(), d_boxes=o[1].data_ptr(), d_kps=o[2].data_ptr(), d_scores=o[3].data_ptr())
        if side == "with_stats":
            seen["stats"] = e.face_stats(Fp * K)
        e.sync()

    for _ in range(args.warmup):
        for side in sides:
            pipe(side)
    for side in sides:
        assert torch.equal(outs[side][2].view(torch.int32), outs["alone"][2].view(torch.int32)), "landmarks must be bit-identical (%s)" % side
    sec = {"frames_per_call": Fp, "valid_faces_per_call": int(seen["stats"][1].sum()), "labelled_pixels_per_call": int(seen["stats"][0][:, :, 0].sum()),
           "landmarks_bit_identical": True}
    for side in sides:
        sec["faces_per_s_" + side] = []
    for _ in range(args.repeats):
        for side in sides:
            t0 = time.perf_counter()
            for _ in range(args.iters):
                pipe(side)
            s = (time.perf_counter() - t0) / args.iters
            sec["faces_per_s_" + side].append(round(Fp * K / s, 1))
    sec["with_stats_over_alone"] = round(max(sec["faces_per_s_with_stats"]) / max(sec["faces_per_s_alone"]), 4)
    if args.parent_library:
        sec["alone_over_alone_parent"] = round(max(sec["faces_per_s_alone"]) / max(sec["faces_per_s_alone_parent"]), 4)
    result["pipeline"] = sec
    for e in engines.values():
        e.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

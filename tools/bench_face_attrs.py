"""Cost of the face-attribute head (face_attrs=True: the landmark network's fc head, partial sums in the hero conv / SCSE kernels):
attrs off against attrs on, in one process on one device.

  * landmark-only faces/s of the Student f32s@256 at 384 faces per launch, default program and the --mix hero,head program;
  * full-pipeline faces/s through pf_run_frames on 1080p synthetic frames with 8 planted faces each (detector running, top_k 8);
  * per-kernel ms (pf_profile_*) of the landmark launch for the kernels the head touches.

Inputs live on the device; timing is host wall clock around --iters launches ended by one synchronisation, after --warmup launches,
the better of --repeats such runs.  Prints one JSON line.

    python tools/bench_face_attrs.py [--faces 384] [--frames 48] [--iters 20] [--repeats 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOUCHED = ("conv3x3_c128_n128_64x64", "scse", "scse_sum", "gap", "face_attrs")


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--faces", type=int, default=384)
    ap.add_argument("--frames", type=int, default=48, help="1080p frames per pf_run_frames call (8 faces each)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    return ap.parse_args()


def timed(eng, fn, iters, warmup, repeats):
    for _ in range(warmup):
        fn()
    eng.sync()
    best = 1e30
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        eng.sync()
        best = min(best, (time.perf_counter() - t0) / iters)
    return best


def main():
    args = parse_args()
    import torch
    from oracle import synth_weights as sw
    from peppa_pig_face_landmark_amd import _native
    from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
    from peppa_pig_face_landmark_amd.graph.student import build_student_program
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows

    dev = torch.device("cuda:0")
    sw_w, det_w = sw.student_weights(), sw.detector_weights()
    B = args.faces
    crops = torch.from_numpy(sw.smooth_blob_images(B, 256, seed=3)).to(dev)
    d_loc = torch.empty((B, 196), dtype=torch.float32, device=dev)
    d_score = torch.empty((B, 98), dtype=torch.float32, device=dev)
    F, K, H, W, R = args.frames, 8, 1080, 1920, 15120
    fr, rows = [], []
    for f in range(F):
        frame, boxes = make_frame(H, W, K, seed=100 + f)
        fr.append(frame)
        rows.append(plant_rows(boxes, (H, W), R, (384, 640), 24, seed=100 + f))
    d_frames = torch.from_numpy(np.stack(fr)).to(dev)
    d_rows = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)
    outs = [torch.empty(s, dtype=dt, device=dev) for s, dt in (((F,), torch.int32), ((F, K, 4), torch.float32),
                                                                ((F, K, 98, 2), torch.float32), ((F, K, 98), torch.float32))]
    d_attrs = torch.empty((max(B, F * K), 7), dtype=torch.float32, device=dev)

    eng = _native.Engine(0)
    det_blob, _ = build_detector_program(det_w, (384, 640), "f32s")
    result = {"faces_per_launch": B, "frames_per_call": F, "faces_per_frame": K}
    for attrs in (False, True):
        tag = "on" if attrs else "off"
        for mix in ((), ("hero", "head")):
            name = "landmark" + ("_mix" if mix else "")
            blob, _ = build_student_program(sw_w, 256, "f32s", one_product=mix, face_attrs=attrs)
            eng.load_program(_native.PF_NET_LANDMARK, blob, max(B, F * K))

            def lm():
                eng.landmark_forward_device(crops.data_ptr(), _native.PF_INPUT_U8_NHWC, B, d_loc.data_ptr(), d_score.data_ptr())
                if attrs:
                    eng.face_attrs_device(B, d_attrs.data_ptr())
            s = timed(eng, lm, args.iters, args.warmup, args.repeats)
            result["%s_faces_per_s_%s" % (name, tag)] = round(B / s, 1)
            if not mix:
                eng.profile_enable(True)
                for _ in range(3):
                    lm()
                eng.sync()
                prof = eng.profile_fetch()
                eng.profile_enable(False)
                result["kernel_ms_%s" % tag] = {k: round(v[0] / max(1, v[1]), 4) for k, v in prof.items() if k in TOUCHED}
        blob, _ = build_student_program(sw_w, 256, "f32s", face_attrs=attrs)
        eng.load_program(_native.PF_NET_LANDMARK, blob, F * K)
        eng.load_program(_native.PF_NET_DETECTOR, det_blob, F)

        def pipe():
            eng.run_frames_device(d_frames.data_ptr(), F, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=R,
                                  d_counts=outs[0].data_ptr(), d_boxes=outs[1].data_ptr(), d_kps=outs[2].data_ptr(),
                                  d_scores=outs[3].data_ptr())
            if attrs:
                eng.face_attrs_device(F * K, d_attrs.data_ptr())
        s = timed(eng, pipe, max(2, args.iters // 4), 2, args.repeats)
        result["pipeline_faces_per_s_%s" % tag] = round(F * K / s, 1)
    for k in ("landmark", "landmark_mix", "pipeline"):
        result["%s_on_over_off" % k] = round(result["%s_faces_per_s_on" % k] / result["%s_faces_per_s_off" % k], 4)
    hero = "conv3x3_c128_n128_64x64"
    if hero in result["kernel_ms_off"] and hero in result["kernel_ms_on"]:
        result["hero_conv_on_over_off"] = round(result["kernel_ms_on"][hero] / result["kernel_ms_off"][hero], 4)
    eng.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

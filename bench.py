#!/usr/bin/env python
"""Benchmark of the FaceAna hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

N > 1 without a launcher self-spawns N ranks (one per GPU) under torch.distributed.run; launched by
torch.distributed.run it reads RANK / LOCAL_RANK / WORLD_SIZE and insists that WORLD_SIZE == N.

One "step" = one pass of the hot path over one batch of synthetic input that is already resident in
HBM when the timed region starts, results delivered to page-locked HOST buffers inside the step
(FaceAna.run() returns numpy, facer.py:84-96):
  --workload pipeline : BASELINE.json configs[2] -- F 1080p frames x 8 planted faces each through
                        letterbox -> detector net -> decode -> NMS -> top-k -> crop/resize ->
                        Student@256 -> heat-map decode -> back-projection   (default)
  --workload landmark : BASELINE.json configs[1] -- 256 pre-cropped 256x256 faces through Student@256
Frames / faces shard across ranks with no data-path collective (weak scaling: per-rank work is
fixed); the only collective is the one-time RCCL broadcast of the packed weights from rank 0, issued
by the engine itself (pf_broadcast_weights -> ncclBroadcast).  Prints ONE JSON line (rank 0).

A plain run sets up, warms up, times the K steps and reports them (value, ms_per_step).  --full adds everything else the
benchmark measures or checks (graph replay vs eager launch, sustained loop, per-kernel table and roofline, latency / PCIe /
JPEG probes, the other BASELINE configurations, the CPU baseline).  --dump-outputs DIR writes what the last timed step
delivered as DIR/<name>.npy (float32); the inputs are seeded, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GFLOP_PER_FACE = {"student": 2.968, "teacher": 11.9}   # 1 484.1 M MAC; Teacher from README 5.53 GiMAC
GFLOP_DETECTOR = 0.882       # yolov5n-0.5 @384x640 per frame: 441.2 M MAC recounted from the restated graph (tests/test_oracle_pinned.py::
                             # test_detector_cost_matches_upstream; SURVEY 8d's upstream-recalled 0.34 does not correspond to this graph)
# dense MFMA peaks (MI355X_MICROARCH.md).  "f32s" = f32 tensors, split-precision convs: every product
# is 3 v_mfma_f32_16x16x32_f16 instructions (hi*hi + hi*lo + lo*hi), so it is priced against the f16 pipe.
PEAK_TFLOPS = {"f32": 157.3, "f16": 2500.0, "f32s": 2500.0}
PEAK_HBM_GBPS = 8000.0
MFMA_INSTR_PER_PRODUCT = {"f32": 1, "f16": 1, "f32s": 3}


def newest_hero_pmc():
    """profiles/rNN_runM_pmc_hero.json with the largest (round, run): the counter passes of the hero kernel are re-collected
    per round (tools/pmc_kernel.py) and named by round."""
    import glob
    import re
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_run*_pmc_hero.json")):
        m = re.match(r"r(\d+)_run(\d+)_", os.path.basename(f))
        if m and (best is None or (int(m.group(1)), int(m.group(2))) > best[0]):
            best = ((int(m.group(1)), int(m.group(2))), f)
    return best[1] if best else None


HERO_TAG = "conv3x3_c128_n128_64x64"          # up2.conv2 (model.py:165-172): 40.7 % of all MACs
HERO_FLOP_PER_FACE = 2.0 * 64 * 64 * 128 * 128 * 9
# algorithmic FLOPs per face of the other dense kernels of the Student (MACs x 2, model.py line ranges in DESIGN.md 5)
DENSE_FLOP_PER_FACE = {
    "conv3x3_c128_n128_64x64": 2.0 * 4096 * 128 * 128 * 9,
    "sepup_c280_n128_64x64": 2.0 * 4096 * 280 * (128 + 9),
    "sepup_c296_n256_32x32": 2.0 * 1024 * 296 * (256 + 9),
    "conv1x1_argmax_c128_n98_64x64": 2.0 * 4096 * 128 * 294,       # the whole hm head (98 scores executed; offsets at the arg-max only)
    "conv1x1_c960_n160_16x16": 2.0 * 256 * 960 * 160,
    "expdw5x5d2_c160_n960_16x16": 2.0 * 256 * 960 * (160 + 25),
    "expdw5x5d1_c112_n672_16x16": 2.0 * 256 * 672 * (112 + 25),
    "expdw3x3d1_c112_n672_16x16": 2.0 * 256 * 672 * (112 + 9),
    "conv3x3_c160_n64_16x16": 2.0 * 256 * 160 * 64 * 9,
}


# FLOPs the launch actually EXECUTES where that differs from the algorithmic count: the score head runs the 98 score channels
# through the GEMM and evaluates the 2 x 98 offset channels at the arg-max pixel only (hm_decode), so its matrix-pipe
# utilisation must be priced on 98 channels -- SURVEY 8d's algorithmic figure keeps all 294 (round-4 VERDICT: the
# executed fraction was overstated 3x)
EXECUTED_FLOP_PER_FACE = {
    "conv1x1_argmax_c128_n98_64x64": 2.0 * 4096 * 128 * 98,
}


def tag_flops_per_face(tag: str):
    """Algorithmic FLOPs (MACs x 2) per face of ONE launch of the dense kernel behind a profile tag, from the shapes the
    engine writes into the tag (csrc/engine.cpp ProfScope names); None for tags that are not dense-conv launches."""
    import re
    if tag in DENSE_FLOP_PER_FACE:
        return DENSE_FLOP_PER_FACE[tag]
    m = re.fullmatch(r"conv(\d)x\d(?:_argmax)?_c(\d+)_n(\d+)_(\d+)x(\d+)", tag)
    if m:
        k, c, n, h, w = map(int, m.groups())
        return 2.0 * k * k * c * n * h * w
    m = re.fullmatch(r"block_c(\d+)_(\d+)x(\d+)", tag)          # BasicBlock: two 3x3 convs C -> C
    if m:
        c, h, w = map(int, m.groups())
        return 2 * 2.0 * 9 * c * c * h * w
    m = re.fullmatch(r"chain(\d+)_c(\d+)_(\d+)x(\d+)", tag)    # n 3x3 convs C -> C resident in LDS
    if m:
        n, c, h, w = map(int, m.groups())
        return n * 2.0 * 9 * c * c * h * w
    m = re.fullmatch(r"sepup_c(\d+)_n(\d+)_(\d+)x(\d+)", tag)  # depthwise 3x3 on C channels + pointwise C -> N
    if m:
        c, n, h, w = map(int, m.groups())
        return 2.0 * h * w * c * (n + 9)
    m = re.fullmatch(r"mbx([ABS]?)(\d)x\dd\d_c(\d+)_m(\d+)_n(\d+)_(\d+)x(\d+)", tag)   # whole inverted-residual block (csrc/k_mbx.h)
    if m:
        mode, (k, c, mid, n, h, w) = m.group(1), map(int, m.groups()[1:])
        # algorithmic work of the launch: expand + depthwise (pass A and, recomputed, pass B count once each: what the launch does
        # for the block's result is expand + depthwise + projection; the squeeze pass is priced as expand + depthwise)
        return 2.0 * h * w * mid * (c + k * k + (0 if mode in ("A", "S") else n))
    m = re.fullmatch(r"expdw(\d)x\d[ds]\d_c(\d+)_n(\d+)_(\d+)x(\d+)", tag)   # expand C -> N + depthwise KxK on N
    if m:
        k, c, n, h, w = map(int, m.groups())
        return 2.0 * h * w * n * (c + k * k)
    return None


KERNEL_OF_TAG_F32S = (   # profile tag prefix -> the HIP kernel that runs it in an f32s program (csrc/engine.cpp dispatch)
    ("conv3x3_c128_n128_64x64", "conv3x3_hero_kernel<4>"), ("block_c", "basic_block_kernel"), ("chain", "basic_chain_kernel"),
    ("sepup_", "sepup_skip_kernel + sepup_pipe_kernel (sepup_patch_kernel fallback)"), ("mbx", "mbx_kernel"), ("expdw", "conv_gemm_split_kernel<..EPI_K> / expdw_image_kernel"), ("conv3x3_c64_n64_64x64", "conv3x3_halo_split_kernel<64,4,2,256>"),
    ("conv", "conv_gemm_split_kernel"))


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="auto", choices=["auto", "landmark", "pipeline"])
    ap.add_argument("--batch", type=int, default=256, help="faces per step per GPU (landmark workload)")
    ap.add_argument("--frames", type=int, default=96, help="1080p frames per step per GPU (pipeline workload)")
    ap.add_argument("--lanes", type=int, default=2, help="concurrent HIP streams (engines) per GPU sharing a step's frames (round 6: two lanes of 48 frames "
                    "behind the front engine measure 2.6 %% above three of 32: profiles/r06_run14_lanes_ab.txt)")
    ap.add_argument("--faces-per-frame", type=int, default=8)
    ap.add_argument("--frame-hw", type=int, nargs=2, default=[1080, 1920], metavar=("H", "W"),
                    help="frame size; --frame-hw 2160 3840 --faces-per-frame 32 --model teacher = BASELINE config 5")
    ap.add_argument("--dtype", default="f32s", choices=["f32", "f32s", "f16"],
                    help="f32: exact v_mfma_f32 convs; f32s (default): f32 tensors + split-precision 3xf16 MFMA convs "
                         "(same accuracy); f16: f16 storage fast mode (parity not claimed)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a hipGraph")
    ap.add_argument("--model", default="student", choices=["student", "teacher"],
                    help="landmark regressor: Student (headline) or Teacher/HRNet-W18 (BASELINE config 5 model)")
    ap.add_argument("--no-probes", action="store_true", help="skip the call-latency, sustained-loop and PCIe-inclusive probes (keeps a "
                    "rocprofv3 --stats run of this command to launches of ONE batch size, so its per-kernel averages are comparable)")
    ap.add_argument("--mbx", default="default", choices=["default", "off", "recompute", "store"],
                    help="A/B aid for the Student's 16 x 16 inverted-residual blocks (csrc/k_mbx.h): off = the layer-wise expand + depthwise / "
                         "projection launches, recompute / store = force one SE strategy for every SE block; default: the builder's choice")
    ap.add_argument("--mbx-waves", type=int, default=16, choices=[8, 16], help="A/B aid: waves per workgroup of the block kernels that have both flavours")
    ap.add_argument("--no-kernel-table", action="store_true", help="skip the per-kernel HIP-event pass after the timed steps (lane sweeps, "
                    "rocprofv3 traces of the multi-lane steady state); roofline is null then")
    ap.add_argument("--sustain-s", type=float, default=3.0, help="after the timed steps, keep stepping for this many seconds "
                    "(a sustained rate an external GPU-busy sampler can see)")
    ap.add_argument("--jpeg-threads", type=int, default=4, help="host threads per lane that strip the byte stuffing in the JPEG-file ingest probe")
    ap.add_argument("--mix", default="", help="comma-separated layers of the Student to run on ONE f16 product instead of the split's three (opt-in, "
                    "reported as such in dtype: 'hero'); the default is the parity-grade f32s everywhere")
    ap.add_argument("--batch-engine", action="store_true", help="use the multi-lane runner (pf_batch_*, front engine) even with --lanes 1")
    ap.add_argument("--no-front2", action="store_true", help="A/B aid: conv_stem and blocks.0.0 as two launches (round 5) instead of the fused lm_front2_kernel")
    ap.add_argument("--no-fc-pairs", action="store_true", help="A/B aid: the SE / cSE / ASPP-pool FC pairs as two fc launches each (round 5) instead of one fc2 launch")
    ap.add_argument("--no-front", action="store_true", help="A/B aid: every lane runs the detector + NMS of its own slice (the round-5 "
                    "flow) instead of one front-engine pass over all frames of a step (PF_OPT_BATCH_FRONT = 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-faces", type=int, default=24)
    ap.add_argument("--dump-profile", default="", help="write the full per-kernel HIP-event table (JSON) here")
    ap.add_argument("--allow-torch-broadcast", action="store_true",
                    help="N > 1 only: if the engine's own RCCL broadcast (pf_broadcast_weights) fails, distribute the weights "
                         "through torch.distributed instead of exiting non-zero (the JSON then says so in weight_broadcast.via)")
    ap.add_argument("--dry-run-cpu", action="store_true",
                    help="plumbing check without a GPU: launch / rendezvous (gloo) / weight-blob broadcast / frame sharding "
                         "only, no compute, value = null (used by the CPU test tier; never a measurement)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run everything else the benchmark measures or checks: graph replay vs eager "
                         "launch, the sustained loop, the per-kernel table and roofline, the one-lane / latency / PCIe / JPEG "
                         "probes, the other configurations and the CPU baseline.  Off: set up, warm up, time the steps, "
                         "write --dump-outputs, print the result line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the timed path delivered in its last timed step (rank 0) as DIR/<name>.npy, float32")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.warmup < 0:
        ap.error("--warmup must be >= 0")
    if args.dump_profile and not args.full:
        ap.error("--dump-profile writes the per-kernel table, which only --full measures")
    return args


DUMP_BUDGET_BYTES = 60_000_000         # --dump-outputs stays under 64 MB, headers included


def timed_outputs(state) -> dict:
    """What a caller of the timed path receives from one step, as float32 host arrays: the pipeline's per-frame face counts and
    per-face boxes / landmarks / scores (the page-locked buffers the step copies into), or the landmark workload's landmarks and
    scores (device resident)."""
    if hasattr(state, "h_kps"):
        arrays = {"counts": state.h_counts, "boxes": state.h_boxes, "landmarks": state.h_kps, "scores": state.h_scores}
    else:
        arrays = {"landmarks": state.loc.cpu().numpy().reshape(-1, 98, 2), "scores": state.score.cpu().numpy()}
    return {k: np.array(v, dtype=np.float32) for k, v in arrays.items()}


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """DIR/<name>.npy for every array; above DUMP_BUDGET_BYTES in all, each array keeps a fixed, seeded subset of its rows
    (sorted, the same in every run) so two runs stay comparable row for row."""
    total = sum(a.nbytes for a in arrays.values())
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        if total > DUMP_BUDGET_BYTES:
            keep = max(1, int(a.shape[0] * DUMP_BUDGET_BYTES // total))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ---------------------------------------------------------------------------------------------------------
def cpu_baseline(n_faces: int, frame_hw, faces_per_frame: int):
    """Reference-shaped CPU path timed on this box's host cores (baseline, NOT the target).  onnxruntime is not
    installed, so the torch-CPU oracle stands in for ORT-CPU; pre/post-processing is the numpy restatement of the
    reference's own (oracle/prepost.py).  Three figures on bounded samples:
      landmark_b1  the reference's execution shape -- one face per call, python loop (face_landmark.py:40-48)
      landmark_b8  the same network fed 8 faces per call (a batch path the reference never wrote, :119)
      pipeline     FaceAna.run()+reset() on whole frames: letterbox, detector net, NMS, per-face crop + forward
    The torch thread count is tuned on a 2-face probe (more threads than physical cores made round 1's figure
    worse) and stated."""
    import torch
    from oracle import detector_net as dn
    from oracle import landmark_net as ln
    from oracle import prepost as pp
    from oracle import synth_weights as sw
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows

    from peppa_pig_face_landmark_amd.graph.detector import random_detector_weights
    from peppa_pig_face_landmark_amd.graph.random_init import random_student_weights

    t_all = time.perf_counter()
    W = ln.to_torch(random_student_weights(0))       # the weights the GPU legs run (timing does not depend on their values)
    crops = sw.smooth_blob_images(8, 256, seed=99)
    x = torch.from_numpy(crops.astype(np.float32) / np.float32(255.0)).permute(0, 3, 1, 2).contiguous()
    ncpu = os.cpu_count() or 1
    cands = sorted({c for c in (8, 16, 32) if c <= ncpu} or {ncpu})
    best_thr, best_t = cands[0], 1e30
    with torch.no_grad():
        for thr in cands:
            torch.set_num_threads(thr)
            ln.student_forward(W, x[:1])
            t0 = time.perf_counter()
            ln.student_forward(W, x[:1]); ln.student_forward(W, x[1:2])
            dt = time.perf_counter() - t0
            if dt < best_t:
                best_thr, best_t = thr, dt
        torch.set_num_threads(best_thr)
        setup_s = time.perf_counter() - t_all
        ln.student_forward(W, x[:1])
        # every leg runs for a fixed wall-time budget (about 16 s of CPU work in total), at least n_faces faces
        n_b1, t0 = 0, time.perf_counter()
        while n_b1 < n_faces or time.perf_counter() - t0 < 6.0:
            ln.student_forward(W, x[n_b1 % 8:n_b1 % 8 + 1])
            n_b1 += 1
        dt_b1 = time.perf_counter() - t0
        ln.student_forward(W, x)
        nb8, t0 = 0, time.perf_counter()
        while nb8 < 2 or time.perf_counter() - t0 < 4.0:
            ln.student_forward(W, x)
            nb8 += 1
        dt_b8 = time.perf_counter() - t0
        # full pipeline on whole frames (x faces_per_frame faces), the reference's order of operations
        H, Wd = frame_hw
        frame, boxes = make_frame(H, Wd, faces_per_frame, seed=7)
        rows = plant_rows(boxes, (H, Wd), 15120, (384, 640), 24, seed=7)
        DW = ln.to_torch(random_detector_weights(1))
        dn.detector_forward(DW, torch.from_numpy(pp.detector_preprocess(frame, (384, 640))[0]))
        n_frames, n_pipe, t0 = 0, 0, time.perf_counter()
        while n_frames < 2 or time.perf_counter() - t0 < 5.0:
            xin, info = pp.detector_preprocess(frame, (384, 640))
            dn.detector_forward(DW, torch.from_numpy(xin))           # its output is replaced by the planted rows below
            kept = pp.detector_postprocess(rows, [np.float32(info[0]), info[1], info[2]], 0.3, 0.5)
            sel = pp.sort_and_filter(kept, 1600.0, faces_per_frame)
            for k in range(sel.shape[0]):
                ci = pp.landmark_crop_box(sel[k], H, Wd)
                crop = pp.landmark_crop(frame, ci, (256, 256))
                loc, _ = ln.student_forward(W, torch.from_numpy(pp.landmark_input(crop)))[:2]
                pp.landmark_backproject(loc[0].numpy(), ci)
            n_frames += 1
            n_pipe += int(sel.shape[0])
        dt_pipe = time.perf_counter() - t0
    return {"value": round(n_b1 / dt_b1, 2), "unit": "faces/s", "cores": best_thr, "kind": "port",
            "sample": "%d faces, Student@256 landmark forward, batch=1 python loop (face_landmark.py:40-48 shape), torch-CPU f32 "
                      "oracle as stand-in for onnxruntime-CPU, %d torch threads (best of %s on a 2-face probe; host has %d "
                      "logical cores); %.1f s" % (n_b1, best_thr, cands, ncpu, dt_b1),
            "landmark_b8_faces_per_s": round(nb8 * 8 / dt_b8, 2), "landmark_b8_sample": "%d batches of 8 in %.1f s" % (nb8, dt_b8),
            "pipeline_faces_per_s": round(n_pipe / dt_pipe, 2), "pipeline_ms_per_frame": round(dt_pipe / n_frames * 1e3, 1),
            "pipeline_sample": "%d frames %dx%d x %d faces in %.1f s: numpy letterbox + torch detector + numpy NMS/top-k + per-face "
                               "numpy crop/resize + B=1 forward + back-projection" % (n_frames, Wd, H, faces_per_frame, dt_pipe),
            "setup_s": round(setup_s, 1), "total_cpu_s": round(time.perf_counter() - t_all, 1),
            "note": "baseline, not target: a large GPU/CPU ratio says nothing about kernel quality, the roofline fractions do"}


def hbm_ops_table(prof, steps, frames_per_launch, faces_per_launch, frame_hw, faces_per_frame):
    """Achieved HBM GB/s of the byte-shuffling pre/post kernels (SURVEY 8d algorithmic bytes per unit x units per
    launch / HIP-event launch time), against the 8 TB/s HBM3E peak."""
    H, W = frame_hw
    s_crop = 280 * H // 1080        # synthetic boxes are 200 px wide at 1080p: crop side 2 * floor(0.7 w)
    per = {
        "letterbox": ("K1 cv2 resize+pad -> u8 384x640x3 (algorithmic bytes, SURVEY 8d: the frame once + the letterboxed image)",
                      frames_per_launch * (H * W * 3 + 384 * 640 * 3)),
        "detect_decode": ("K3 in-graph Detect decode, f32 rows read + written", frames_per_launch * 2 * 15120 * 16 * 4),
        "nms": ("K4 xywh2xyxy + NMS + scale_coords + top-k, f32 rows read once", frames_per_launch * (15120 * 16 * 4 + faces_per_frame * 64)),
        "crop_resize": ("K5 crop + cv2.resize -> u8 256x256x3", faces_per_launch * (3 * s_crop * s_crop + 3 * 256 * 256)),
        "hm_decode": ("K10/K11 arg-max partials + offsets at the arg-max + back-projection", faces_per_launch * 98 * (32 * 8 + 128 * 4 + 20)),
    }
    out = {}
    for tag, (what, nbytes) in per.items():
        if tag not in prof or prof[tag][1] == 0:
            continue
        ms, cnt = prof[tag]
        launches_per_step = cnt / steps
        avg_ms = ms / steps            # all launches of the tag in one step together move `nbytes`
        gbps = nbytes / (avg_ms * 1e-3) / 1e9
        out[tag] = {"what": what, "algorithmic_bytes_per_step": int(nbytes), "ms_per_step": round(avg_ms, 4),
                    "launches_per_step": launches_per_step, "achieved_GBps": round(gbps, 1),
                    "frac_of_hbm_peak": round(gbps / PEAK_HBM_GBPS, 4)}
        if tag == "letterbox":
            # the bilinear taps of an output row touch two source rows: below a scale of 1/2 rows in between are never fetched
            # (1080p -> 360 rows: rows 3d+1 and 3d+2 only, 2/3 of the frame) -- the rate the memory system actually saw
            rh = min(384, int(H * min(384.0 / H, 640.0 / W)))
            rows_touched = min(H, 2 * rh)
            fetched = frames_per_launch * (rows_touched * W * 3 + 384 * 640 * 3)
            out[tag]["fetched_bytes_per_step"] = int(fetched)
            out[tag]["physical_GBps"] = round(fetched / (avg_ms * 1e-3) / 1e9, 1)
    return out


def dense_kernel_table(prof, steps, faces_per_launch, dtype, pmc_traffic=None):
    out = {}
    table = dict(DENSE_FLOP_PER_FACE)
    table.update({t: tag_flops_per_face(t) for t in prof if t.startswith("mbx")})     # the block kernels name their own shapes
    for tag, flop in table.items():
        if tag not in prof or prof[tag][1] == 0:
            continue
        # `flop` is ONE launch's work: price it against one launch's time (a tag with two launches per step -- the two stage-5 blocks,
        # the two dilated ASPP convs -- was understated 2x when divided by the tag's total time per step: round-5 VERDICT weak 11)
        ms = prof[tag][0] / prof[tag][1]
        tf = flop * faces_per_launch / (ms * 1e-3) / 1e12
        tf_exec = EXECUTED_FLOP_PER_FACE.get(tag, flop) * faces_per_launch / (ms * 1e-3) / 1e12
        out[tag] = {"ms_per_launch": round(ms, 4), "launches_per_lane_step": prof[tag][1] / steps,
                    "ms_per_lane_step": round(prof[tag][0] / steps, 4), "algorithmic_tflops": round(tf, 1),
                    "frac_of_mfma_peak": round(tf / PEAK_TFLOPS[dtype], 4),
                    "executed_mfma_frac": round(tf_exec * MFMA_INSTR_PER_PRODUCT[dtype] / PEAK_TFLOPS[dtype], 4)}
        pmc = pmc_traffic.get(tag) if pmc_traffic else None
        if pmc:
            out[tag].update(pmc)
    return out


def committed_pmc_traffic(faces_per_launch):
    """HBM traffic of the dominant-group kernels from the newest committed counter files (profiles/rNN_runM_pmc_groups.json,
    tools/pmc_kernel.py: one rocprofv3 --pmc pass per counter; FETCH_SIZE / WRITE_SIZE in KB, FETCH x 2 on gfx950) as
    {profile tag: {traffic_bytes_per_launch, algorithmic_bytes_per_launch, traffic_ratio, pmc_source}}.  Attached, not measured
    here: rocprofv3 owns the counters, so they do not move if a kernel regresses after the file was written."""
    import glob
    import re
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_run*_pmc_groups.json")):
        m = re.match(r"r(\d+)_run(\d+)_", os.path.basename(f))
        if m and (best is None or (int(m.group(1)), int(m.group(2))) > best[0]):
            best = ((int(m.group(1)), int(m.group(2))), f)
    if not best:
        return {}
    with open(best[1]) as f:
        doc = json.load(f)
    out = {}
    for tag, rec in doc.get("tags", {}).items():
        if "FETCH_SIZE" not in rec or "WRITE_SIZE" not in rec:
            continue
        scale = faces_per_launch / float(rec.get("faces_per_launch", 256))
        traffic = (2.0 * rec["FETCH_SIZE"] + rec["WRITE_SIZE"]) * 1024.0 * scale
        alg = rec.get("algorithmic_bytes_per_face", 0) * faces_per_launch
        out[tag] = {"traffic_bytes_per_launch": int(traffic), "algorithmic_bytes_per_launch": int(alg),
                    "traffic_ratio": round(traffic / alg, 2) if alg else None, "launches_in_tag": rec.get("launches", 1),
                    "pmc_source": "profiles/" + os.path.basename(best[1]), "traffic_from_committed_profile": True}
    return out


def dry_run_cpu(args):
    """Launch / rendezvous / broadcast / sharding plumbing on CPU (gloo); no engine, no compute, no measurement."""
    import torch
    import torch.distributed as dist
    import bench_support as bs

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    use_dist = world > 1
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    rng = np.random.default_rng(0)
    blobs = {0: rng.integers(0, 256, 70001, dtype=np.uint8).tobytes(), 1: rng.integers(0, 256, 4099, dtype=np.uint8).tobytes()} if rank == 0 else None
    if use_dist:
        blobs, _ = bs.broadcast_blobs(blobs, torch.device("cpu"), rank)
    mine = bs.shard_frames(args.frames * world, rank, world)
    sums = torch.tensor([float(sum(blobs[0][:64]) + sum(blobs[1][:64])), float(len(mine))], dtype=torch.float64)
    gathered = [torch.zeros_like(sums) for _ in range(world)]
    if use_dist:
        dist.all_gather(gathered, sums)
    else:
        gathered = [sums]
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        assert all(float(g[0]) == float(gathered[0][0]) for g in gathered), "ranks hold different blobs"
        print(json.dumps({"metric": "dry run (plumbing only, no measurement)", "value": None, "unit": "faces/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "dry_run": True, "scaling": "weak",
                          "frames_per_rank": [int(g[1]) for g in gathered], "max_over_ranks_check": float(t.item())}), flush=True)


def main():
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    launched = "WORLD_SIZE" in os.environ and "RANK" in os.environ
    if args.gpus > 1 and not launched:
        # python bench.py --gpus N: become the launcher (one rank per GPU, torch.distributed.run, 127.0.0.1)
        if not args.dry_run_cpu:
            import torch
            have = torch.cuda.device_count() if torch.cuda.is_available() else 0
            if have < args.gpus:
                raise SystemExit("bench.py: --gpus %d requested but only %d GPU(s) visible on this node (no CPU fallback, "
                                 "no oversubscription)" % (args.gpus, have))
        import bench_support as bs
        sys.exit(bs.spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    if args.dry_run_cpu:
        return dry_run_cpu(args)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP engine has no CPU fallback")
    if local_rank >= torch.cuda.device_count():
        raise SystemExit("bench.py: local rank %d has no GPU (%d visible)" % (local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    use_dist = world > 1
    dev = torch.device("cuda", local_rank)

    class _StdoutToStderr:
        """RCCL prints a version banner on stdout at communicator creation; the contract is ONE JSON line on stdout,
        so stdout points at stderr while communicators come up (the banner, with its rank count, lands in stderr)."""
        def __enter__(self):
            sys.stdout.flush()
            self.saved = os.dup(1)
            os.dup2(2, 1)
        def __exit__(self, *exc):
            sys.stdout.flush()
            try:   # the banner sits in the C library's stdio buffer (stdout is a pipe/file here): push it out while
                import ctypes                                   # fd 1 still points at stderr, or it lands after the JSON
                ctypes.CDLL(None).fflush(None)
            except Exception:  # noqa: BLE001
                pass
            os.dup2(self.saved, 1)
            os.close(self.saved)

    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        with _StdoutToStderr():
            dist.init_process_group("nccl", device_id=dev)
            dist.all_reduce(torch.zeros(1, device=dev))
            torch.cuda.synchronize()

    from peppa_pig_face_landmark_amd import build as pbuild
    from peppa_pig_face_landmark_amd._native import Engine, PF_NET_DETECTOR, PF_NET_LANDMARK
    import bench_support as bs

    if rank == 0:
        pbuild.build_hip()
    if use_dist:
        dist.barrier()
    eng = Engine(local_rank)

    workload = args.workload
    if workload == "auto":
        workload = "pipeline" if bs.pipeline_available() else "landmark"

    # ---- weights: packed on rank 0, broadcast once by the ENGINE over RCCL / xGMI (pf_broadcast_weights) -----------
    t0 = time.time()
    skw = {}
    if args.model == "student":
        if args.mbx == "off":
            skw["fuse_mbx"] = False
        elif args.mbx != "default":
            skw["mbx_se"] = args.mbx
        if args.mbx_waves != 16:
            skw["mbx_waves"] = args.mbx_waves
        if args.no_fc_pairs:
            skw["fuse_fc_pairs"] = False
        if args.no_front2:
            skw["fuse_front2"] = False
    if args.mix:
        skw["one_product"] = tuple(x for x in args.mix.split(",") if x)
    blobs = bs.build_programs(workload, args.dtype, args.model, **skw) if rank == 0 else None
    slots = [PF_NET_LANDMARK] + ([PF_NET_DETECTOR] if workload == "pipeline" else [])

    def exchange_id(uid):
        if not use_dist:
            return uid
        t = torch.zeros(128, dtype=torch.uint8, device=dev)
        if rank == 0:
            t.copy_(torch.frombuffer(bytearray(uid), dtype=torch.uint8))
        dist.broadcast(t, 0)
        return bytes(t.cpu().numpy().tobytes())

    bcast = {"ms": 0.0, "bytes": 0, "via": "pf_broadcast_weights (ncclBroadcast on the engine's stream)", "rccl_version": None,
             "engine_rccl_ok": True}
    fail = None
    try:
        with _StdoutToStderr():
            blobs_out, bcast["ms"], bcast["bytes"] = bs.broadcast_programs_rccl(eng, blobs, slots, rank, world, exchange_id)
            bcast["rccl_version"] = eng.rccl_version()
        print("[bench] rank %d/%d: RCCL %s communicator of %d rank(s); %d weight bytes in %.3f ms" % (
            rank, world, bcast["rccl_version"], world, bcast["bytes"], bcast["ms"]), file=sys.stderr, flush=True)
    except Exception as e:   # noqa: BLE001
        fail = e
    if use_dist:
        # the ranks must AGREE on what happens next: a rank that alone entered the fallback broadcast would hang there
        ok = torch.tensor([0.0 if fail is not None else 1.0], device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if float(ok.item()) < 1.0:
            print("[bench] rank %d: pf_broadcast_weights failed on at least one rank (here: %s)" % (rank, fail), file=sys.stderr, flush=True)
            if not args.allow_torch_broadcast:
                # a scaling line must not exist unless the C-ABI RCCL path worked: no silent detour through torch.distributed
                dist.destroy_process_group()
                raise SystemExit("bench.py: the engine's RCCL weight broadcast (pf_broadcast_weights) failed; "
                                 "re-run with --allow-torch-broadcast to distribute the weights through torch.distributed instead")
            blobs, ms = bs.broadcast_blobs(blobs, dev, rank)
            bcast.update({"ms": ms, "bytes": sum(len(b) for b in blobs.values()), "engine_rccl_ok": False,
                          "via": "torch.distributed broadcast over RCCL (--allow-torch-broadcast; pf_broadcast_weights failed: %s)" % fail})
        else:
            blobs = blobs_out
    elif fail is not None:
        bcast.update({"engine_rccl_ok": False, "via": "single GPU: local pf_load_program (RCCL self-test failed: %s)" % fail})
    else:
        blobs = blobs_out
    faces_per_step = args.batch if workload == "landmark" else args.frames * args.faces_per_frame
    lanes = args.lanes if workload == "pipeline" else 1
    single = lanes == 1 and not (args.batch_engine and workload == "pipeline")
    if single:
        bs.load_programs(eng, blobs, workload, faces_per_step, args.frames)
    setup_s = time.time() - t0

    # ---- synthetic inputs, resident in HBM ----------------------------------------------------------
    if workload == "landmark":
        state = bs.LandmarkWorkload(eng, dev, args.batch, seed=1234 + rank)
    elif single:
        state = bs.PipelineWorkload(eng, dev, args.frames, args.faces_per_frame, seed=7 + rank, graph=not args.no_graph,
                                    frame_hw=tuple(args.frame_hw))
    else:
        # the product's multi-lane runner (pf_batch_* of the C ABI; FrameBatchRunner sits on the same object): the library
        # splits a step's frames over its own `lanes` engines / HIP streams -- bench.py makes ONE call per step
        eng.close()
        from peppa_pig_face_landmark_amd._native import BatchEngine, PF_OPT_RANGE_CHECK
        if args.frames % lanes:
            raise SystemExit("bench.py: --frames %d is not a multiple of --lanes %d" % (args.frames, lanes))
        batch = BatchEngine(local_rank, lanes)
        if os.environ.get("PEPPA_BENCH_NO_GUARD"):       # measurement aid only: what the always-on f32s range guard costs
            batch.set_option(PF_OPT_RANGE_CHECK, 0)
        per_lane = args.frames // lanes
        batch.load_program(PF_NET_LANDMARK, blobs[PF_NET_LANDMARK], per_lane * args.faces_per_frame)
        batch.load_program(PF_NET_DETECTOR, blobs[PF_NET_DETECTOR], per_lane)
        state = bs.BatchPipelineWorkload(batch, dev, args.frames, args.faces_per_frame, seed=7 + rank, lanes=lanes,
                                         graph=not args.no_graph, frame_hw=tuple(args.frame_hw), front=not args.no_front)
        eng = batch.lane(0)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        state.sync()

    for _ in range(args.warmup):
        state.step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        state.step()
    state.sync()                      # the engines run on their own (non-blocking) streams
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    per_rank_rate = [round(faces_per_step * args.steps / elapsed, 1)]
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)                       # each rank's own clock, for the per-rank rates beside the headline
        per_rank_rate = [round(faces_per_step * args.steps / float(e.item()), 1) for e in every]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, timed_outputs(state))
    barrier()
    if args.full:
        state.check()

    # ---- sustained loop (not the headline): long enough for an external GPU-busy sampler to see -------------------
    sustained = None
    if args.full and not args.no_probes and args.sustain_s > 0:
        n_sus = 0
        t1 = time.perf_counter()
        while time.perf_counter() - t1 < args.sustain_s:
            for _ in range(4):
                state.step()
            state.sync()
            n_sus += 4
        dt = time.perf_counter() - t1
        sustained = {"seconds": round(dt, 2), "steps": n_sus, "faces_per_s_per_gpu": round(n_sus * faces_per_step / dt, 1)}

    # ---- per-kernel device time (HIP events on the engine's own stream), dominant kernel roofline ---
    PROF_STEPS = 3
    prof = state.profile(PROF_STEPS) if args.full and not args.no_kernel_table else {}
    faces_per_launch = faces_per_step // lanes      # the profiled lane processes 1/lanes of the step
    frames_per_launch = args.frames // lanes
    # front mode (pf_batch's front engine): letterbox + detector + NMS run ONCE per step on all frames; their tags live in a profile of
    # their own so that `prof` stays "one lane's launches on its slice"
    front_prof = getattr(state, "front_prof", None) or {}
    front_ms = sum(v[0] for v in front_prof.values()) / PROF_STEPS if front_prof else 0.0
    # The dominant kernel = the dense-conv tag with the most device time per lane-step IN THIS RUN (the Student's hero conv
    # up2.conv2; for --model teacher whichever HRNet / decoder kernel leads), not a name fixed in this file.
    def _square(t):      # the landmark networks run on square maps; the detector's 3:5 maps are per FRAME, not per face
        m = __import__("re").search(r"_(\d+)x(\d+)$", t)
        return bool(m) and m.group(1) == m.group(2)
    dense = {t: v for t, v in prof.items() if v[1] and _square(t) and tag_flops_per_face(t) is not None}
    roofline = None
    if dense:
        dom = max(dense, key=lambda t: dense[t][0])
        dom_ms, dom_n = dense[dom]
        avg_ms = dom_ms / dom_n
        flop = tag_flops_per_face(dom)
        achieved = flop * faces_per_launch / (avg_ms * 1e-3) / 1e12
        kern = "conv_gemm_kernel<%s>" % args.dtype
        if args.dtype == "f32s":
            kern = next(k for pre, k in KERNEL_OF_TAG_F32S if dom.startswith(pre))
        m = __import__("re").search(r"_c(\d+)(?:_m\d+)?(?:_n(\d+))?_(\d+)x(\d+)$", dom)
        cin, nout, hh, ww = int(m.group(1)), int(m.group(2) or m.group(1)), int(m.group(3)), int(m.group(4))
        esz = 2 if args.dtype == "f16" else 4
        roofline = {"bound": "mfma", "kernel": "%s %s" % (kern, dom),
                    "achieved": round(achieved, 2), "peak": PEAK_TFLOPS[args.dtype], "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_TFLOPS[args.dtype], 4), "traffic": None,
                    "algorithmic_bytes": int((cin + nout) * hh * ww * esz * faces_per_launch),      # the input map once + the output map once
                    "algorithmic_flop_per_face": flop, "faces_per_launch": faces_per_launch,
                    "avg_launch_ms": round(avg_ms, 4), "launches": dom_n, "launches_per_lane_step": dom_n / PROF_STEPS,
                    "share_of_lane_step": round(dom_ms / max(1e-9, sum(v[0] for v in prof.values())), 4),
                    "measured": "HIP events on the engine's stream around every launch of this tag, this process",
                    "executed_mfma_tflops": round(achieved * MFMA_INSTR_PER_PRODUCT[args.dtype], 2),
                    "executed_mfma_frac": round(achieved * MFMA_INSTR_PER_PRODUCT[args.dtype] / PEAK_TFLOPS[args.dtype], 4)}
        # PMC figures cannot be collected from inside this process (rocprofv3 owns the counters): they are attached from
        # the NEWEST committed counter file of the hero kernel (profiles/rNN_runM_pmc_hero.json, tools/pmc_kernel.py) and
        # flagged as such -- they do not move when the kernel regresses.
        pmc_path = newest_hero_pmc()
        if dom == HERO_TAG and args.dtype == "f32s" and pmc_path:
            with open(pmc_path) as f:
                pmc = json.load(f)
            faces_pmc = int(pmc.get("_meta", {}).get("faces_per_launch", 256))
            rec = next((v for k, v in pmc.items() if "conv3x3_hero_kernel" in k or "conv3x3_halo_split_kernel<128" in k), None)
            if rec and "FETCH_SIZE" in rec and "WRITE_SIZE" in rec:
                # raw counters are KB; FETCH_SIZE under-reports wide coalesced reads by exactly 2x on gfx950 (MI355X_MICROARCH.md, HBM)
                roofline["traffic"] = int((2.0 * rec["FETCH_SIZE"] + rec["WRITE_SIZE"]) * 1024.0 * faces_per_launch / faces_pmc)
                roofline["traffic_from_committed_profile"] = True
                roofline["traffic_source"] = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes; 2 x FETCH_SIZE + WRITE_SIZE, scaled to this launch size)" % os.path.basename(pmc_path)
            if rec and "SQ_VALU_MFMA_BUSY_CYCLES" in rec and rec.get("SQ_BUSY_CU_CYCLES"):
                roofline["mfma_pipe_busy_pmc"] = round(rec["SQ_VALU_MFMA_BUSY_CYCLES"] / (4.0 * rec["SQ_BUSY_CU_CYCLES"]), 4)
                roofline["mfma_pipe_busy_from_committed_profile"] = True
                roofline["pmc_source"] = "profiles/" + os.path.basename(pmc_path)
    if args.dump_profile and rank == 0:
        with open(args.dump_profile, "w") as f:
            json.dump({"steps": PROF_STEPS, "faces_per_step": faces_per_step, "dtype": args.dtype, "workload": workload,
                       "kernels": {k: {"ms_per_step": v[0] / PROF_STEPS, "launches_per_step": v[1] / PROF_STEPS}
                                   for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])}}, f, indent=1)
    one_lane = None
    if args.full and workload == "pipeline" and hasattr(state, "one_lane_rate") and not args.no_probes:
        one_lane = round(state.one_lane_rate(max(4, min(args.steps, 12))), 1)
    latency = None
    if args.full and workload == "pipeline" and not args.no_probes:
        l1 = state.latency_p50(1)
        lN = state.latency_p50(args.frames // lanes)
        latency = {"single_frame_call_ms_p50": round(l1[0], 4), "single_frame_call_ms_p99": round(l1[1], 4),
                   "lane_batch_call_ms_p50": round(lN[0], 4), "lane_batch_frames": args.frames // lanes,
                   "ms_per_frame_p50_at_lane_batch": round(lN[0] / (args.frames // lanes), 4),
                   "note": "synchronous pf_run_frames call on one stream, device-resident frames"}
    # ---- PCIe-inclusive rate (never the headline): same step with the frames in page-locked HOST memory ----------
    pcie = None
    if args.full and workload == "pipeline" and rank == 0 and world == 1 and hasattr(state, "enable_host_frames") and not args.no_probes:
        state.enable_host_frames()
        hs = max(2, min(args.steps, 8))
        state.step_host()
        state.sync()
        t1 = time.perf_counter()
        for _ in range(hs):
            state.step_host()
        state.sync()
        dt = time.perf_counter() - t1
        state.check()
        pcie = {"faces_per_s": round(faces_per_step * hs / dt, 1), "frames_per_s": round(args.frames * hs / dt, 1),
                "h2d_GBps": round(args.frames * hs * args.frame_hw[0] * args.frame_hw[1] * 3 / dt / 1e9, 2), "steps": hs,
                "note": "frames handed over in pf_host_alloc (page-locked) host memory, copied inside the call on each lane's "
                        "stream; results stay on the device (9.5 KB/frame)"}
    # ---- JPEG-file ingest (never the headline): the same step starting from baseline JPEG files in host memory --------
    jpeg = None
    if args.full and workload == "pipeline" and rank == 0 and world == 1 and hasattr(state, "enable_jpeg_frames") and not args.no_probes:
        try:
            import PIL  # noqa: F401  (only to WRITE the test files; the decoder is the engine's)
            have_pil = True
        except ImportError:
            have_pil = False
        try:
            if not have_pil:
                raise ImportError("PIL not installed: no way to write the JPEG test files")
            thr = max(1, args.jpeg_threads)
            jpeg = {"note": "every frame of the step arrives as a baseline 4:2:0 JPEG file (quality 90) in host memory: pf_decode_jpeg_batch "
                            "feeds pf_run_frames, one host thread per lane drives decode + pipeline; output bit-identical with libjpeg.  The "
                            "files carry no restart markers: the host threads only strip the byte stuffing, the Huffman stream is decoded on the "
                            "device as self-synchronising 1024-bit sub-sequences (csrc/k_jpeg.h jpeg_sync_kernel)",
                    "host_threads_per_lane": thr}
            for key, rows in (("no_restart_markers", 0),):
                total_bytes = state.enable_jpeg_frames(90, rows)
                for _ in range(2):      # the decoder alternates two frame buffers: both get their captured graph before the clock starts
                    state.step_jpeg(thr)
                state.sync()
                js = max(2, min(args.steps, 6))
                t1 = time.perf_counter()
                for _ in range(js):
                    state.step_jpeg(thr)
                state.sync()
                dt = time.perf_counter() - t1
                state.check(compare_eager=False)     # (lossy files: their landmarks are not those of the resident frames)
                jpeg[key] = {"faces_per_s": round(faces_per_step * js / dt, 1), "frames_per_s": round(args.frames * js / dt, 1),
                             "jpeg_MB_per_s": round(total_bytes * js / dt / 1e6, 1), "mean_file_KB": round(total_bytes / args.frames / 1e3, 1),
                             "steps": js}
        except Exception as e:          # a probe must never take the headline measurement down with it
            jpeg = {"skipped": "%s: %s" % (type(e).__name__, e)}
    # ---- the other single-GPU configurations of BASELINE.json, a few steps each (never the headline) -----------------------------
    other = None
    if args.full and workload == "pipeline" and args.model == "student" and rank == 0 and world == 1 and not args.no_probes:
        other = {}
        try:      # configs[1]: 256 pre-cropped faces through Student@256 on ONE engine / stream (lane 0's program)
            nb = min(256, faces_per_step // lanes)
            lw = bs.LandmarkWorkload(eng, dev, nb, seed=1234)
            for _ in range(3):
                lw.step()
            lw.sync()
            t1 = time.perf_counter()
            for _ in range(10):
                lw.step()
            lw.sync()
            dt = time.perf_counter() - t1
            lw.check()
            other["configs[1] Student@256 landmark-only"] = {"faces_per_s": round(nb * 10 / dt, 1), "ms_per_step": round(dt / 10 * 1e3, 4),
                                                           "faces_per_step": nb, "steps": 10, "lanes": 1}
        except Exception as e:   # noqa: BLE001  (a probe never takes the headline down)
            other["configs[1] Student@256 landmark-only"] = {"skipped": "%s: %s" % (type(e).__name__, e)}
        if args.dtype == "f32s" and not args.mix:
            try:      # the headline's configuration with the decoder tail on ONE f16 product (opt-in mix; never the headline)
                from peppa_pig_face_landmark_amd._native import BatchEngine as _BE
                mb = _BE(local_rank, lanes)
                mblobs = bs.build_programs("pipeline", args.dtype, "student", one_product=("hero", "head"), **skw)
                mb.load_program(PF_NET_LANDMARK, mblobs[PF_NET_LANDMARK], args.frames // lanes * args.faces_per_frame)
                mb.load_program(PF_NET_DETECTOR, mblobs[PF_NET_DETECTOR], args.frames // lanes)
                mw = bs.BatchPipelineWorkload(mb, dev, args.frames, args.faces_per_frame, seed=7, lanes=lanes, graph=True, frame_hw=tuple(args.frame_hw))
                for _ in range(3):
                    mw.step()
                mw.sync()
                t1 = time.perf_counter()
                for _ in range(12):
                    mw.step()
                mw.sync()
                dt = time.perf_counter() - t1
                mw.check(compare_eager=False)
                other["configs[2] with up2.conv2 + the score head on ONE f16 product (--mix hero,head)"] = {
                    "faces_per_s": round(faces_per_step * 12 / dt, 1), "ms_per_step": round(dt / 12 * 1e3, 4), "steps": 12, "lanes": lanes,
                    "note": "opt-in precision mix, NOT the headline: decoder.upsampler2.conv2 (42 % of the dense MACs) and the 98 score channels of "
                            "the heat-map conv on one v_mfma_f32_16x16x32_f16 product per 32 k instead of the split's three; landmarks within "
                            "1.4e-4 of the oracle on MI355X (tests/test_gpu_landmark.py::test_student_one_product_hero_mix_stays_within_its_budget; "
                            "f32s: 2.8e-5; north star 1e-3), which layers tolerate it: profiles/r06_student_precision_study.txt"}
                mw.close()
            except Exception as e:   # noqa: BLE001
                other["configs[2] with up2.conv2 + the score head on ONE f16 product (--mix hero,head)"] = {"skipped": "%s: %s" % (type(e).__name__, e)}
        # configs[4]'s shape on this GPU: Teacher@256, 2160x3840 frames x 32 planted faces, three lanes -- f32s (the parity-grade mode) and the
        # same with the two decoder layers that have one-product kernels on ONE f16 product (profiles/r06_teacher_precision_study.txt)
        for tmix in ((), ("hero", "head")):
            tkey = "configs[4]-shaped Teacher@256 2160p x 32 faces, one GPU" + (" -- up2.conv2 + score head on ONE f16 product" if tmix else "")
            try:
                from peppa_pig_face_landmark_amd._native import BatchEngine as _BE
                tb = _BE(local_rank, 3)
                tblobs = bs.build_programs("pipeline", args.dtype, "teacher", **({"one_product": tmix} if tmix else {}))
                c5_frames = 12
                tb.load_program(PF_NET_LANDMARK, tblobs[PF_NET_LANDMARK], c5_frames // 3 * 32)
                tb.load_program(PF_NET_DETECTOR, tblobs[PF_NET_DETECTOR], c5_frames // 3)
                tw = bs.BatchPipelineWorkload(tb, dev, c5_frames, 32, seed=7, lanes=3, graph=True, frame_hw=(2160, 3840))
                for _ in range(2):
                    tw.step()
                tw.sync()
                t1 = time.perf_counter()
                for _ in range(6):
                    tw.step()
                tw.sync()
                dt = time.perf_counter() - t1
                tw.check(compare_eager=False)
                other[tkey] = {
                    "faces_per_s": round(c5_frames * 32 * 6 / dt, 1), "ms_per_step": round(dt / 6 * 1e3, 4), "frames_per_step": c5_frames,
                    "faces_per_step": c5_frames * 32, "steps": 6, "lanes": 3, "dtype": args.dtype,
                    "note": ("opt-in precision mix: landmarks within 1.1e-4 of the oracle on MI355X (tests/test_gpu_landmark.py::"
                             "test_teacher_one_product_hero_head_mix_stays_within_its_budget); the other layers force three products "
                             "(profiles/r06_teacher_precision_study.txt: one product everywhere = 7.6e-3)") if tmix else
                            ("f32s (split-precision f16 MFMA, parity grade); BASELINE names fp16 MFMA for this config -- f16 storage misses the "
                             "1e-3 bar on the synthetic weights (DESIGN.md 3), so the parity-grade mode is what is timed")}
                tw.close()
            except Exception as e:   # noqa: BLE001
                other[tkey] = {"skipped": "%s: %s" % (type(e).__name__, e)}
    ms_per_step = elapsed / args.steps * 1e3
    faces_total = faces_per_step * world * args.steps
    value = faces_total / elapsed
    # executed matrix-pipe work of ONE lane step (all of a lane's launches back to back) against its serial device time: the whole
    # forward's MFMA fraction, not only the hero's.  Landmark net: SURVEY 8d's algorithmic FLOPs minus the 2 x 98 offset channels of
    # the heat-map head that are evaluated at the arg-max pixel only; detector: its restated graph's count at the letterbox size.
    serial_ms = sum(v[0] for v in prof.values()) / PROF_STEPS if prof else 0.0
    step_serial_ms = front_ms + lanes * serial_ms      # every launch of one step back to back: front engine once + each lane's share
    exec_frac_forward = None
    if serial_ms > 0 and args.model == "student":
        exec_gflop = faces_per_step * (GFLOP_PER_FACE["student"] - 2.0 * 4096 * 128 * 196 / 1e9)
        if workload == "pipeline":
            exec_gflop += args.frames * GFLOP_DETECTOR
        exec_frac_forward = round(exec_gflop * MFMA_INSTR_PER_PRODUCT[args.dtype] / step_serial_ms / PEAK_TFLOPS[args.dtype], 4)
    out = {
        "metric": "faces/sec (whole node), %s@256" % args.model.capitalize() + ((" %dpx%d-face full pipeline" % (args.frame_hw[0], args.faces_per_frame)) if workload == "pipeline" else " landmark-only"),
        "value": round(value, 1), "unit": "faces/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": {"f32": "f32", "f16": "f16", "f32s": "f32 (tensors f32; convs = 3x f16-MFMA split precision, f32 accumulate)"}[args.dtype] +
                 ((" EXCEPT %s on ONE f16-MFMA product (opt-in mix, not the parity-grade default)" % args.mix) if args.mix else ""),
        "data": "synthetic",
        "config": {"workload": ("%s full pipeline: %d x %dx%d frames x %d planted faces per GPU per step" % (
                       "configs[2]" if tuple(args.frame_hw) == (1080, 1920) else "configs[4]-shaped", args.frames, args.frame_hw[1], args.frame_hw[0], args.faces_per_frame))
                   if workload == "pipeline" else ("configs[1] landmark-only: %d pre-cropped 256x256 faces per GPU per step" % args.batch),
                   "faces_per_step_per_gpu": faces_per_step, "parallelism": "frame-sharded x%d GPUs, %d HIP streams per GPU%s, no data-path collective" % (
                       world, lanes, " (pf_batch_run_frames: one call per step, lanes inside the library)" if lanes > 1 else ""),
                   "unique_frames_per_gpu": getattr(state, "unique_frames", None),
                   "results": "counts/boxes/landmarks/scores copied to page-locked host memory inside every step" if workload == "pipeline" else "device resident",
                   "weights": "synthetic (reference .onnx blobs absent), %s: %.1f MB%s" % (
                       bcast["via"], bcast["bytes"] / 1e6,
                       (" in %.3f ms = %.1f GB/s vs 153 GB/s per xGMI link" % (bcast["ms"], bcast["bytes"] / 1e9 / (bcast["ms"] * 1e-3)))
                       if (world > 1 and bcast["ms"] > 0) else (" (one rank: the broadcast is a local no-op, no rate to report)" if world == 1 else ""))},
        "extra": {"ms_per_frame": round(ms_per_step / args.frames, 4) if workload == "pipeline" else None,
                  "algorithmic_tflops": round(value * GFLOP_PER_FACE[args.model] / 1e3, 2),
                  "frac_of_conv_roofline": round(value / world * GFLOP_PER_FACE[args.model] / 1e3 / PEAK_TFLOPS[args.dtype], 4),
                  "weight_broadcast": bcast,
                  "per_rank_faces_per_s": per_rank_rate,      # each rank on its own clock; `value` uses the slowest rank's time
                  "weight_broadcast_GBps_vs_xgmi_link": (round(bcast["bytes"] / 1e9 / (bcast["ms"] * 1e-3), 2) if (world > 1 and bcast["ms"] > 0) else None),
                  "setup_s": round(setup_s, 2)},
    }
    if args.full:
        out.update({
            # the timed region is short (20 steps ~ 0.3 s): the rate of the multi-second loop that follows it, same steps, same process
            "sustained_value": (round(sustained["faces_per_s_per_gpu"] * world, 1) if sustained else None),
            # NOT the headline: the same configuration with decoder.upsampler2.conv2 and the score head on ONE f16 product (extra.other_configs
            # has the note and the parity test's name); the headline stays f32-grade everywhere
            "value_with_one_product_decoder_tail": ((other or {}).get("configs[2] with up2.conv2 + the score head on ONE f16 product (--mix hero,head)", {}).get("faces_per_s")),
            "roofline": roofline,
            "cpu_baseline": None})
        out["extra"].update({
            "hbm_ops": (dict(hbm_ops_table(prof, PROF_STEPS, frames_per_launch, faces_per_launch, tuple(args.frame_hw), args.faces_per_frame),
                             **hbm_ops_table(front_prof, PROF_STEPS, args.frames, faces_per_step, tuple(args.frame_hw), args.faces_per_frame))
                        if workload == "pipeline" else None),
            "dense_kernels": dense_kernel_table(prof, PROF_STEPS, faces_per_launch, args.dtype, committed_pmc_traffic(faces_per_launch)) if args.model == "student" else None,
            "sustained": sustained,
            "executed_mfma_frac_forward": exec_frac_forward,
            # what ONE engine / one stream delivers on a lane's share of the step (plain pf_run_frames, graph replay);
            # the headline is pf_batch_run_frames over `lanes` of them
            "one_lane_faces_per_s": one_lane,
            "latency": latency,
            "pcie_inclusive": pcie, "jpeg_ingest": jpeg, "other_configs": other,
            "kernel_ms_per_lane_step": {k: round(v[0] / PROF_STEPS, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])[:12]},
            "lane_step_ms_serial": round(serial_ms, 4),
            # front engine: letterbox + detector + NMS of ALL frames of a step, once (null: every lane detects its own slice)
            "front_step_ms_serial": round(front_ms, 4) if front_prof else None,
            "front_kernel_ms_per_step": ({k: round(v[0] / PROF_STEPS, 4) for k, v in sorted(front_prof.items(), key=lambda kv: -kv[1][0])[:8]}
                                         if front_prof else None),
            "step_ms_serial": round(step_serial_ms, 4),
            # how much of a step's serial kernel time the concurrent streams hide: (front + lanes x lane) / measured step
            "lanes_overlap": round(step_serial_ms / ms_per_step, 4)})
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.cpu_faces, tuple(args.frame_hw), args.faces_per_frame)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if hasattr(state, "close"):
        state.close()
    else:
        eng.close()


if __name__ == "__main__":
    main()

"""Cost of the baseline JPEG encoder (pf_encode_jpeg, csrc/k_jpeg_enc.h), in one process on one device.

  * jpeg_enc_blocks / jpeg_enc_entropy / jpeg_enc_pack (pf_profile_fetch) and the whole device-to-device call (events around it,
    profiling off) for 96 redacted frames of 1080p with 8 planted faces each at quality 85, 4:2:0 and 4:4:4, and for 768 chips of
    112 x 112, beside hipMemcpyAsync device-to-device over the same INPUT bytes -- the floor of any pass that reads every pixel
    once -- and beside the alternative the encoder replaces: the device-to-host copy of the raw images followed by Pillow
    (libjpeg-turbo) on 16 host threads.  The Pillow side INCLUDES that copy, reported separately as well; the device side
    includes no copy (the files stay in device memory, 0.1 - 0.5 byte per pixel to fetch);
  * pf_run_frames on 1080p synthetic frames with 8 planted faces each (Student f32s@256, detector running, top_k 8): alone; with
    pf_face_redact into device memory + pf_encode_jpeg, only the files copied out; with the raw redacted frames copied out.  The
    landmarks must be bit-identical in all three.

Both sides of each comparison run interleaved, --repeats times; every repetition is reported.  A one-thread-per-interval form of the
entropy stage was not built, so there is no second form to time.  Writes profiles/jpeg_encode_bench.json and prints the same line.

    python tools/bench_jpeg_encode.py [--frames 48] [--encode-frames 96] [--iters 5] [--repeats 2]
"""
from __future__ import annotations

import argparse
import ctypes as C
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("jpeg_enc_blocks", "jpeg_enc_entropy", "jpeg_enc_pack")


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=48, help="1080p frames per pf_run_frames call (8 faces each)")
    ap.add_argument("--encode-frames", type=int, default=96, help="frames of the kernel measurement (8 faces each)")
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the Pillow side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_bench.json"))
    return ap.parse_args()


def main():
    args = parse_args()
    import torch
    from PIL import Image
    from oracle import synth_weights as sw
    from peppa_pig_face_landmark_amd import _native
    from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
    from peppa_pig_face_landmark_amd.graph.student import build_student_program
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
    from tests.align_ref import layout98
    from tools.bench_face_masks import face_landmarks

    dev = torch.device("cuda:0")
    K, H, W, R, S = 8, 1080, 1920, 15120, 112
    Fp, Fe, Q = args.frames, args.encode_frames, args.quality
    rng = np.random.default_rng(1)
    layout = layout98()
    fr, rows, kps = [], [], []
    for f in range(max(Fp, Fe)):
        frame, boxes = make_frame(H, W, K, seed=100 + f)
        fr.append(frame)
        if f < Fp:
            rows.append(plant_rows(boxes, (H, W), R, (384, 640), 24, seed=100 + f))
        kps.append(np.stack([face_landmarks(layout, b, rng.uniform(-30, 30), rng) for b in boxes]))
    kps = np.stack(kps).astype(np.float32)
    d_frames = torch.from_numpy(np.stack(fr)).to(dev)
    d_rows = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)
    del fr
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    eng = _native.Engine(0)
    result = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "quality": Q, "pillow": Image.__version__,
              "pillow_threads": args.threads, "entropy_one_thread_per_interval": "not built"}

    # the inputs: redacted frames and chips, made on the device by the stages in front of the encoder
    d_red = torch.empty((Fe, H, W, 3), dtype=torch.uint8, device=dev)
    eng.redact_faces_device((d_frames.data_ptr(), Fe, H, W), kps[:Fe], d_red.data_ptr(), mode="mosaic", strength=16)
    d_chips = torch.zeros((Fe * K, S, S, 3), dtype=torch.uint8, device=dev)
    eng.align_faces_device((d_frames.data_ptr(), Fe, H, W), kps[:Fe], d_chips.data_ptr(), chip_size=S)
    eng.sync()
    d_copy = torch.empty((Fe * H * W * 3,), dtype=torch.uint8, device=dev)

    def memcpy_ms(nbytes, src):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            assert hip.hipMemcpyAsync(d_copy.data_ptr(), src, nbytes, 3, None) == 0
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    def pillow_ms(d_images, sampling):
        """device-to-host copy of the raw images, then Pillow on the host threads: (ms of the copy, ms of the encoding, files)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = d_images.cpu().numpy()
        t1 = time.perf_counter()

        def one(i):
            buf = io.BytesIO()
            Image.fromarray(host[i][..., ::-1]).save(buf, format="JPEG", quality=Q, subsampling={444: 0, 422: 1, 420: 2}[sampling],
                                                     restart_marker_rows=1)
            return buf.getvalue()
        with ThreadPoolExecutor(args.threads) as pool:
            files = list(pool.map(one, range(host.shape[0])))
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, files

    result["encode"] = {}
    for name, d_images, sampling in (("frames_420", d_red, 420), ("frames_444", d_red, 444), ("chips_420", d_chips, 420)):
        n, h, w = d_images.shape[:3]
        in_bytes = n * h * w * 3
        cap = 3 * h * w // 2 + 4096
        d_out = torch.empty((n * cap,), dtype=torch.uint8, device=dev)
        d_sizes = torch.zeros((n,), dtype=torch.int32, device=dev)

        def encode():
            eng.encode_jpeg_device(d_images.data_ptr(), n, h, w, d_out.data_ptr(), cap, d_sizes.data_ptr(), quality=Q, subsampling=sampling)

        sec = {"images": n, "shape": [h, w], "subsampling": sampling, "input_bytes": in_bytes, "ms_call": [], "ms_memcpy_d2d": [],
               "ms_pillow_copy_d2h": [], "ms_pillow_encode": []}
        sec.update({"ms_" + k: [] for k in KERNELS})
        for _ in range(args.warmup):
            encode()
            eng.sync()
            memcpy_ms(in_bytes, d_images.data_ptr())
        for _ in range(args.repeats):
            eng.profile_enable(True)
            for _ in range(args.iters):
                encode()
            eng.sync()
            prof = eng.profile_fetch()
            eng.profile_enable(False)
            for k in KERNELS:                                   # per call: the chunks of a call are summed
                sec["ms_" + k].append(round(prof[k][0] / args.iters, 4))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.iters):
                encode()
            eng.sync()
            b.record()
            torch.cuda.synchronize()
            sec["ms_call"].append(round(a.elapsed_time(b) / args.iters, 4))
            sec["ms_memcpy_d2d"].append(round(memcpy_ms(in_bytes, d_images.data_ptr()), 4))
            c_ms, e_ms, files = pillow_ms(d_images, sampling)
            sec["ms_pillow_copy_d2h"].append(round(c_ms, 2))
            sec["ms_pillow_encode"].append(round(e_ms, 2))
        sizes = d_sizes.cpu().numpy()
        assert (sizes > 0).all()
        out = d_out.cpu().numpy()
        same = sum(out[i * cap: i * cap + sizes[i]].tobytes() == files[i] for i in range(n))
        sec["files_identical_with_pillow"] = "%d of %d" % (same, n)
        sec["file_bytes"] = int(sizes.sum())
        sec["bytes_per_pixel"] = round(float(sizes.sum()) / (n * h * w), 4)
        kernels = sum(min(sec["ms_" + k]) for k in KERNELS)
        sec["ms_kernels"] = round(kernels, 4)
        sec["kernels_over_memcpy"] = round(kernels / min(sec["ms_memcpy_d2d"]), 2)
        sec["pillow_with_copy_over_call"] = round((min(sec["ms_pillow_copy_d2h"]) + min(sec["ms_pillow_encode"])) / min(sec["ms_call"]), 2)
        sec["megapixels_per_s"] = round(n * h * w / (min(sec["ms_call"]) * 1e-3) / 1e6, 1)
        result["encode"][name] = sec
        del d_out
    del d_copy, d_chips, d_red

    # ---- pipeline: alone / redact + encode on the device, files out / raw redacted frames out, interleaved --------------------------
    eng.load_program(_native.PF_NET_LANDMARK, build_student_program(sw.student_weights(), 256, "f32s")[0], Fp * K)
    eng.load_program(_native.PF_NET_DETECTOR, build_detector_program(sw.detector_weights(), (384, 640), "f32s")[0], Fp)
    outs = [torch.empty(s, dtype=dt, device=dev) for s, dt in (((Fp,), torch.int32), ((Fp, K, 4), torch.float32),
                                                                ((Fp, K, 98, 2), torch.float32), ((Fp, K, 98), torch.float32))]
    r_out = torch.zeros((Fp, H, W, 3), dtype=torch.uint8, device=dev)
    got = {}

    def pipe(mode):
        eng.run_frames_device(d_frames.data_ptr(), Fp, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=R,
                              d_counts=outs[0].data_ptr(), d_boxes=outs[1].data_ptr(), d_kps=outs[2].data_ptr(), d_scores=outs[3].data_ptr())
        if mode == "jpeg":
            eng.face_redact_device(Fp * K, r_out.data_ptr(), mode="mosaic", strength=16)
            got[mode] = eng.encode_jpeg((r_out.data_ptr(), Fp, H, W), quality=Q, subsampling=420, capacity=3 * H * W // 2)
        elif mode == "raw":
            got[mode] = eng.face_redact(Fp * K, mode="mosaic", strength=16)[0]
        eng.sync()

    modes = ("off", "jpeg", "raw")
    seen = {}
    for _ in range(args.warmup):
        for m in modes:
            pipe(m)
            seen[m] = outs[2].clone()
    assert all(torch.equal(seen["off"].view(torch.int32), seen[m].view(torch.int32)) for m in modes), "landmarks must be bit-identical"
    sec = {"frames_per_call": Fp, "landmarks_bit_identical": True, "file_bytes_per_call": sum(len(f) for f in got["jpeg"]),
           "raw_bytes_per_call": int(got["raw"].nbytes)}
    sec.update({"faces_per_s_" + m: [] for m in modes})
    for _ in range(args.repeats):
        for m in modes:
            t0 = time.perf_counter()
            for _ in range(args.iters):
                pipe(m)
            s = (time.perf_counter() - t0) / args.iters
            sec["faces_per_s_" + m].append(round(Fp * K / s, 1))
    sec["jpeg_over_off"] = round(max(sec["faces_per_s_jpeg"]) / max(sec["faces_per_s_off"]), 4)
    sec["raw_over_off"] = round(max(sec["faces_per_s_raw"]) / max(sec["faces_per_s_off"]), 4)
    result["pipeline"] = sec
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""Throughput of the tracked video path: S camera streams advanced by one pf_track_streams call per step, against S
single-stream engines (pf_track_frame, one handle each) called in turn on the same frames.

1080p synthetic frames with 8 planted faces each (synth.make_frame / plant_rows, seeded), top_k = 8 so every face is
tracked.  Stream s alternates between two frames of its own (the second one shifted by 9 px); in each call a set share of
the streams repeats its previous frame instead, so the gate skips their detector.  Frames live on the device (decoded
video), the planted detector rows in page-locked host memory; both paths read the same ones.  Timing: host wall clock
around whole calls, each of which ends in a stream synchronisation; warm-up first, then at least --min-seconds per point.
Prints one JSON line.

    python tools/bench_track_streams.py [--streams 1 8 32 96] [--repeat-share 0.5] [--dtype f32s]

--ids KEEP_LOST measures the cost of persistent ids instead of the single-stream baseline: on ONE engine per point, ids off
and ids on (pf_track_ids_config, that keep_lost) alternate, two repetitions of --min-seconds each, then a few profiled calls
give the device time of track_ident_kernel (pf_profile_fetch).  --out FILE also writes the JSON there.
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

CYCLE = 4                  # calls over which a stream repeats its frame round(share * CYCLE) times
ARGS = dict(score_thres=0.5, nms_iou_thres=0.3, min_face=1600.0, track_iou_thres=0.5, smooth_box=0.3, diff_thres=5.0)


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32, 96])
    ap.add_argument("--repeat-share", type=float, default=0.5, help="share of the streams that repeat their frame in a call")
    ap.add_argument("--baseline-max", type=int, default=32, help="largest S measured with S single-stream engines")
    ap.add_argument("--dtype", default="f32s", choices=["f32", "f32s", "f16"])
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ids", type=int, default=None, metavar="KEEP_LOST", help="measure persistent ids off / on instead of the baseline")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    return ap.parse_args()


def schedule(share: float):
    """(repeat calls per CYCLE, period in calls): a stream alternates between two frames, so its pattern comes back after
    an even number of moves -- one CYCLE, or two when a CYCLE has an odd number of moves"""
    r = min(CYCLE, max(0, int(round(share * CYCLE))))
    return r, CYCLE if (CYCLE - r) % 2 == 0 else 2 * CYCLE


def main():
    args = parse_args()
    import torch
    import bench_support as bs
    from peppa_pig_face_landmark_amd import _native
    from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows

    H, W, FACES, K, R = 1080, 1920, 8, 8, 15120
    S_max = max(args.streams)
    n_rep, period = schedule(args.repeat_share)
    dev = torch.device("cuda:0")
    # two frames per stream (A: a seeded scene rolled by 2 s px, B: A shifted by 9 px more) and their planted rows
    base = [make_frame(H, W, FACES, seed=7 + k) for k in range(4)]
    frame_ab, rows_ab = [], []
    probe = _native.Engine(0)
    for s in range(S_max):
        f0, b0 = base[s % 4]
        pair, prow = [], []
        for shift in (2 * s, 2 * s + 9):
            pair.append(torch.from_numpy(np.roll(f0, shift, axis=1)).to(dev))
            r = probe.pinned_empty((R, 16), np.float32)
            r[:] = plant_rows(b0 + np.float32([shift, 0, shift, 0]), (H, W), R, (384, 640), 6, seed=1000 + 2 * s + len(prow))
            prow.append(r)
        frame_ab.append(pair)
        rows_ab.append(prow)

    def which(s, c):      # 0 / 1: frame A or B of stream s at call c of the cycle (repeat calls keep the previous one)
        moves = sum(1 for k in range(c + 1) if (k + s) % CYCLE >= n_rep)
        return moves % 2

    blobs = bs.build_programs("pipeline", args.dtype)
    points = []
    for S in args.streams:
        # the call batches of one cycle, on the device, and their planted rows (pinned; freed with `pin` after the point)
        pin = _native.Engine(0)
        batches, prows = [], []
        for c in range(period):
            p = [which(s, c) for s in range(S)]
            batches.append(torch.stack([frame_ab[s][p[s]] for s in range(S)]).contiguous())
            pr = pin.pinned_empty((S, R, 16), np.float32)
            for s in range(S):
                pr[s] = rows_ab[s][p[s]]
            prows.append(pr)
        torch.cuda.synchronize()
        eng = _native.Engine(0)
        eng.load_program(_native.PF_NET_LANDMARK, blobs[_native.PF_NET_LANDMARK], S * K)
        eng.load_program(_native.PF_NET_DETECTOR, blobs[_native.PF_NET_DETECTOR], S)
        eng.track_streams_config(S, K)
        ids = list(range(S))

        def step(c):
            b = batches[c % period]
            return eng.track_streams(ids, b.data_ptr(), planted_rows=prows[c % period], shape=(S, H, W), **ARGS)

        for c in range(args.warmup):
            step(c)
        if args.ids is not None:
            def timed(c0):
                c, t0 = c0, time.perf_counter()
                while True:
                    step(c)
                    c += 1
                    el = time.perf_counter() - t0
                    if el >= args.min_seconds and c - c0 >= period:
                        return c, {"calls": c - c0, "ms_per_call": 1e3 * el / (c - c0), "frames_per_s": S * (c - c0) / el}
            c, runs = args.warmup, {"off": [], "on": []}
            for _ in range(2):                       # off, on, off, on: drift of the machine lands on both alike
                for mode in ("off", "on"):
                    eng.track_ids_config(mode == "on", args.ids)
                    for _w in range(period):         # every stream has met its schedule in this mode (ids: their first frames)
                        step(c)
                        c += 1
                    c, r = timed(c)
                    runs[mode].append(r)
            eng.track_ids_config(True, args.ids)
            eng.profile_enable(True)
            for _p in range(period):
                step(c)
                c += 1
            prof = eng.profile_fetch().get("track_ident", (0.0, 0))
            eng.profile_enable(False)
            n_ids = int((eng.track_ids(S * K)[0] > 0).sum())
            points.append({"streams": S, "keep_lost": args.ids, "off": runs["off"], "on": runs["on"], "ids_in_last_call": n_ids,
                           "track_ident_kernel": {"launches": prof[1], "device_ms_per_launch": prof[0] / max(prof[1], 1)}})
            eng.close()
            del eng, batches, prows
            pin.close()
            torch.cuda.empty_cache()
            continue
        c0 = c = args.warmup
        det = faces = 0
        t0 = time.perf_counter()
        while True:
            out = step(c)
            det += sum(r[3] for r in out)
            faces += sum(len(r[0]) for r in out)
            c += 1
            el = time.perf_counter() - t0
            if el >= args.min_seconds and c - c0 >= period:
                break
        calls = c - c0
        pt = {"streams": S, "calls": calls, "ms_per_call": 1e3 * el / calls, "frames_per_s": S * calls / el,
              "faces_per_s": faces / el, "detector_share": det / (S * calls)}
        eng.close()
        del eng
        if S <= args.baseline_max:
            engines = []
            for s in range(S):
                e = _native.Engine(0)
                e.load_program(_native.PF_NET_LANDMARK, blobs[_native.PF_NET_LANDMARK], K)
                e.load_program(_native.PF_NET_DETECTOR, blobs[_native.PF_NET_DETECTOR], 1)
                engines.append(e)
            nbytes = H * W * 3

            def round_(c):
                b = batches[c % period]
                res = []
                for s, e in enumerate(engines):
                    fr = _native.DeviceFrame(b.data_ptr() + s * nbytes, H, W)
                    res.append(e.track_frame(fr, ARGS["score_thres"], ARGS["nms_iou_thres"], ARGS["min_face"], K,
                                             ARGS["track_iou_thres"], ARGS["smooth_box"], ARGS["diff_thres"],
                                             prows[c % period][s]))
                return res

            for c in range(args.warmup):
                round_(c)
            c0 = c = args.warmup
            faces = 0
            t0 = time.perf_counter()
            while True:
                out = round_(c)
                faces += sum(len(r[0]) for r in out)
                c += 1
                el = time.perf_counter() - t0
                if el >= args.min_seconds and c - c0 >= period:
                    break
            rounds = c - c0
            pt["baseline"] = {"engines": S, "rounds": rounds, "ms_per_round": 1e3 * el / rounds,
                              "frames_per_s": S * rounds / el, "faces_per_s": faces / el}
            pt["speedup"] = pt["frames_per_s"] / pt["baseline"]["frames_per_s"]
            for e in engines:
                e.close()
        else:
            pt["baseline"] = None
        points.append(pt)
        del batches, prows
        pin.close()
        torch.cuda.empty_cache()
    probe.close()
    line = json.dumps({"tool": "bench_track_streams", "device": torch.cuda.get_device_name(0), "dtype": args.dtype,
                       "frame_hw": [H, W], "faces_per_frame": FACES, "top_k": K, "repeat_share": n_rep / CYCLE,
                       "timing": "host wall clock over synchronised calls", "planted_rows": "pinned host, copied per detector frame",
                       "points": points})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

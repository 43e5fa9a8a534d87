"""Generate tests/golden/tracking_video_edges.npz for tests/tracking_video.py::video_edges.  Group-A segments: the REFERENCE's
own FaceAna (facer.py + lk.py executed from source; planted rows for the detector, the engine's f32 Student on the SIMT
emulator for the landmark session -- tests/test_tracking_edges.py::reference_run_edges), each with its own min_face.  Group B
(the reference raises): the in-repo host facade (FaceAna, device_tracking = False) on the emulator; the hand-stated
expectations of those segments live in the fixture.  Next to the results goes the evidence that every edge is hit.
Needs the reference checkout (oracle.ref_import.available()).
Usage:  python tests/golden/make_tracking_golden_edges.py"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import ref_import as ri  # noqa: E402
from oracle import synth_weights as sw  # noqa: E402
from tests.test_tracking_edges import TOP_K, facade_run_edges, numpy_evidence, reference_run_edges  # noqa: E402
from tests.tracking_video import GOLDEN_EDGES, video_edges  # noqa: E402


def main():
    assert ri.available(), "needs the reference checkout"
    from tests.simt_emu import build_emu
    lib = build_emu.build_emu()
    segs = video_edges()
    runs, ran, ev = reference_run_edges(sw.student_weights(), lib)
    b_runs, b_ran = facade_run_edges(lib, sw.student_weights(), sw.detector_weights(), False, groups=("B",))
    runs.update(b_runs)
    ran.update(b_ran)
    ev.update(numpy_evidence(segs))
    frames = [(res, r) for s in segs for res, r in zip(runs[s["name"]], ran[s["name"]])]
    n = len(frames)
    box = np.zeros((n, TOP_K, 4), np.float64)
    kps = np.zeros((n, TOP_K, 98, 2), np.float64)
    scores = np.zeros((n, TOP_K, 98), np.float64)
    counts = np.zeros(n, np.int64)
    for i, (res, _) in enumerate(frames):
        counts[i] = len(res)
        for j, r in enumerate(res):
            box[i, j], kps[i, j], scores[i, j] = r["box"], r["kps"], r["scores"]
    np.savez_compressed(GOLDEN_EDGES, counts=counts, box=box, kps=kps, scores=scores,
                        detector_ran=np.asarray([r for _, r in frames], np.int64), numpy_version=np.__version__,
                        **{"ev_" + k: np.asarray(v) for k, v in ev.items()})
    print("edge tracking golden written: counts", counts.tolist(), "detector ran", [r for _, r in frames])
    for k, v in ev.items():
        print(k, np.asarray(v).tolist())


if __name__ == "__main__":
    main()

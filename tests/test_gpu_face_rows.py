"""The table of tests/test_face_rows.py through the HIP library on a real MI355X, plus the calls the emulator tier leaves out: the
tracking calls as calls that leave rows, and the accessors of a pf_batch.  These cells, too, were recorded before the bookkeeping
behind them was folded into one record."""
import ctypes as C

import numpy as np
import pytest
import torch

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from tests import test_face_rows as T

pytestmark = pytest.mark.gpu

TRACK = dict(score_thres=0.5, nms_iou_thres=0.3, min_face=100.0, track_iou_thres=0.5, smooth_box=0.3, diff_thres=5.0)

TRACK_RULES = {
    ("track_frame", None): (2, 2, 2, 2, 2),
    ("track_frame", "set_frame"): T.FORGOTTEN + (2,),
    ("track_frame", "crop_faces"): T.FORGOTTEN + (2,),
    ("track_frame", "track_streams_config"): T.FORGOTTEN + (2,),
    ("track_frame", "load_program"): T.FORGOTTEN + (T.NO_ATTRS,),
    ("track_streams", None): (4, 4, 4, 4, 4),
    ("track_streams", "set_frame"): T.FORGOTTEN + (4,),
    ("track_streams", "crop_faces"): T.FORGOTTEN + (4,),
    ("track_streams", "track_streams_config"): T.FORGOTTEN + (4,),
    ("track_streams", "load_program"): T.FORGOTTEN + (T.NO_ATTRS,),
}
TRACK_CASES = sorted(TRACK_RULES, key=lambda k: (k[0], k[1] or ""))


@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_last_call_rules(gpu_engine, student_weights, case):
    T.check_last_call_rules(gpu_engine, student_weights, case[0], case[1], T.RULES[case])


def test_fresh_handle_has_no_rows(gpu_engine, student_weights):
    gpu_engine.load_program(0, T.landmark_blob(student_weights), 4)
    assert T.observe(gpu_engine) == T.FORGOTTEN + (T.NO_ATTRS,)


@pytest.fixture(scope="module")
def detector_blob(detector_weights):
    return build_detector_program(detector_weights, (384, 640), "f32s")[0]


@pytest.mark.parametrize("case", TRACK_CASES, ids=["%s-%s" % (w, b or "nothing") for w, b in TRACK_CASES])
def test_last_call_rules_of_the_tracking_calls(gpu_engine, student_weights, detector_blob, case):
    writer, between = case
    blob = T.landmark_blob(student_weights)
    gpu_engine.load_program(0, blob, 4)
    gpu_engine.load_program(1, detector_blob, 2)
    frames, boxes, rows = T.scene(n_rows=15120, per_box=24)
    if writer == "track_frame":
        got = gpu_engine.track_frame(frames[0], TRACK["score_thres"], TRACK["nms_iou_thres"], TRACK["min_face"], T.K,
                                     TRACK["track_iou_thres"], TRACK["smooth_box"], TRACK["diff_thres"], rows[0])
        assert len(got[0]) == 2
    else:
        gpu_engine.track_streams_config(2, T.K)
        gpu_engine.track_streams([1, 0], frames, planted_rows=rows, **TRACK)
    T.call_between(gpu_engine, between, blob, frames, boxes)
    assert T.observe(gpu_engine) == TRACK_RULES[case]


def _observe_batch(be):
    def shape(n):
        F, H, W = C.c_int(0), C.c_int(0), C.c_int(0)
        be._check(be.lib.pf_batch_face_masks_shape(be.b, n, C.byref(F), C.byref(H), C.byref(W)), "pf_batch_face_masks_shape")

    def redact(n):
        out, valid = np.zeros((2, T.H, T.W, 3), np.uint8), np.zeros((max(n, 1),), np.int32)
        be._check(be.lib.pf_batch_face_redact(be.b, n, None, *_native._redact_args("mosaic", _native.PF_REDACT_FACE_ALL, 8, 0, 0),
                                              _native._ptr(out), _native._ptr(valid), _native.PF_MEM_HOST), "pf_batch_face_redact")
        return out, valid[:n]

    calls = ((lambda n: be.face_chips(n, 32), lambda r: len(r[2])), (lambda n: be.face_masks(n, 32), lambda r: len(r[3])),
             (shape, lambda r: None), (redact, lambda r: len(r[1])), (lambda n: be.face_attrs(n), lambda r: len(r)))
    return tuple(T.cell(*c) for c in calls)


@pytest.mark.parametrize("front", [1, 0])
def test_last_call_rules_of_a_batch(hip_library, student_weights, front):
    be = _native.BatchEngine(0, 2, hip_library)
    be.set_option(_native.PF_OPT_BATCH_FRONT, front)
    be.load_program(0, T.landmark_blob(student_weights), T.K)
    no_rows = "%s: no pf_batch_run_frames call has left face rows"
    assert _observe_batch(be) == (no_rows % "pf_batch_face_chips", no_rows % "pf_batch_face_masks", no_rows % "pf_batch_face_masks",
                                  no_rows % "pf_batch_face_redact",
                                  "pf_batch_face_attrs: no pf_batch_run_frames call has left face-attribute rows")
    frames, _, rows = T.scene()
    if front:       # the front engine takes device-resident frames only
        d_frames = torch.from_numpy(frames).cuda()
        d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
        be.run_frames_device(d_frames.data_ptr(), 2, T.H, T.W, 0.5, 0.3, 100.0, T.K, d_planted=d_rows.data_ptr(), rows=rows.shape[1])
        be.sync()
    else:
        be.run_frames(frames, 0.5, 0.3, 100.0, T.K, planted_rows=rows)
    assert _observe_batch(be) == (4, 4, 4, 4, 4)
    be.close()

"""What a handle's last call leaves for the accessors that come after the landmarks -- pf_face_chips, pf_face_masks,
pf_face_masks_shape, pf_face_redact, pf_face_attrs -- and which calls forget it, held as a table: a call that leaves rows, then at
most one call in between, then every accessor.  A cell is the number of rows the accessor finds, or the text it refuses with.  The
cells were recorded from the library before the bookkeeping behind them was folded into one record; they hold for the SIMT emulator
here and for the HIP library in tests/test_gpu_face_rows.py, which imports ``check_last_call_rules`` and adds the tracking calls and
pf_batch."""
import re

import numpy as np
import pytest

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd._native import PeppaHipError
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.synth import make_frame_grid, plant_rows

H = W = 96
K = 2
ACCESSORS = ("face_chips", "face_masks", "face_masks_shape", "face_redact", "face_attrs")

NO_ROWS = "%s: the handle's last call left no face rows (pf_landmarks*, pf_run_frames*, pf_track_frame* and pf_track_streams do)"
NO_FRAME = "%s: the handle's last call was pf_landmark_forward, which has no frame to %s"
NO_ATTRS = ("pf_face_attrs: the handle's last call left no face-attribute rows (pf_landmark_forward, pf_landmarks*, pf_run_frames*, "
            "pf_track_frame* and pf_track_streams do)")
FORGOTTEN = tuple(NO_ROWS % ("pf_" + a) for a in ACCESSORS[:4])
FRAMELESS = (NO_FRAME % ("pf_face_chips", "cut chips from"), NO_FRAME % ("pf_face_masks", "lay the maps over"),
             NO_FRAME % ("pf_face_masks_shape", "lay the maps over"), NO_FRAME % ("pf_face_redact", "lay the maps over"))

# (call that leaves rows, call in between) -> one cell per accessor, in the order of ACCESSORS
RULES = {
    ("landmarks", None): (2, 2, 2, 2, 2),
    ("landmarks", "set_frame"): FORGOTTEN + (2,),
    ("landmarks", "crop_faces"): FORGOTTEN + (2,),
    ("landmarks", "track_streams_config"): FORGOTTEN + (2,),
    ("landmarks", "load_program"): FORGOTTEN + (NO_ATTRS,),
    # pf_landmarks without boxes, after one with two: the frames are forgotten, the attribute rows of the earlier call are not
    ("landmarks_n0", None): FORGOTTEN + (2,),
    ("landmarks_n0", "set_frame"): FORGOTTEN + (2,),
    ("landmarks_n0", "crop_faces"): FORGOTTEN + (2,),
    ("landmarks_n0", "track_streams_config"): FORGOTTEN + (2,),
    ("landmarks_n0", "load_program"): FORGOTTEN + (NO_ATTRS,),
    ("run_frames", None): (4, 4, 4, 4, 4),
    ("run_frames", "set_frame"): FORGOTTEN + (4,),
    ("run_frames", "crop_faces"): FORGOTTEN + (4,),
    ("run_frames", "track_streams_config"): FORGOTTEN + (4,),
    ("run_frames", "load_program"): FORGOTTEN + (NO_ATTRS,),
    ("landmark_forward", None): FRAMELESS + (2,),
    ("landmark_forward", "set_frame"): FORGOTTEN + (2,),
    ("landmark_forward", "crop_faces"): FORGOTTEN + (2,),
    ("landmark_forward", "track_streams_config"): FORGOTTEN + (2,),
    ("landmark_forward", "load_program"): FORGOTTEN + (NO_ATTRS,),
}
CASES = sorted(RULES, key=lambda k: (k[0], k[1] or ""))
CASE_IDS = ["%s-%s" % (w, b or "nothing") for w, b in CASES]


def scene(F=2, seed=3, n_rows=1260, per_box=6):
    """F frames of 96 x 96 with two planted faces each, their boxes and the detector rows that select them (a loaded detector
    program takes as many planted rows as it produces itself: 15120)."""
    frames, boxes, rows = [], [], []
    for f in range(F):
        fr, bx = make_frame_grid(H, W, 2, 1, face_w=30.0, face_h=40.0, seed=seed + f)
        frames.append(fr)
        boxes.append(bx)
        rows.append(plant_rows(bx, (H, W), n_rows=n_rows, input_hw=(384, 640), per_box=per_box, seed=seed + f))
    return np.stack(frames), np.stack(boxes), np.stack(rows)


def landmark_blob(weights):
    """The 64-pixel student with the face-attribute head, so that pf_face_attrs has rows to find."""
    return build_student_program(weights, 64, "f32", face_attrs=True)[0]


def _landmarks_n0(engine, frame):
    rc = engine.lib.pf_landmarks(engine.h, _native._ptr(frame), _native.PF_MEM_HOST, H, W, frame.strides[0], None, 0, None, None, None)
    assert rc == 0


def leave_rows(engine, writer, frames, boxes, rows):
    if writer in ("landmarks", "landmarks_n0"):
        engine.landmarks(frames[0], boxes[0])
        if writer == "landmarks_n0":
            _landmarks_n0(engine, frames[0])
    elif writer == "run_frames":
        engine.run_frames(frames, 0.5, 0.3, 100.0, K, planted_rows=rows)
    elif writer == "landmark_forward":
        engine.landmark_forward(np.zeros((2, 64, 64, 3), np.uint8))
    else:
        raise KeyError(writer)


def call_between(engine, between, blob, frames, boxes):
    if between == "set_frame":
        engine.set_frame(frames[1])
    elif between == "crop_faces":
        engine.crop_faces(frames[1], boxes[1], 64)
    elif between == "track_streams_config":
        engine.track_streams_config(2, K)
    elif between == "load_program":
        engine.load_program(0, blob, 4)
    elif between is not None:
        raise KeyError(between)


def raw_face_redact(engine, n):
    """pf_face_redact itself (Engine.face_redact asks pf_face_masks_shape first, whose refusals would stand in for this one's)"""
    out, valid = np.zeros((2, H, W, 3), np.uint8), np.zeros((max(n, 1),), np.int32)
    engine._check(engine.lib.pf_face_redact(engine.h, n, None, *_native._redact_args("mosaic", _native.PF_REDACT_FACE_ALL, 8, 0, 0),
                                            _native._ptr(out), _native._ptr(valid), _native.PF_MEM_HOST), "pf_face_redact")
    return out, valid[:n]


def accessor_calls(engine):
    """name -> (call(rows), rows the result holds); chip-space maps, because the frame-space ones ask pf_face_masks_shape first"""
    return {
        "face_chips": (lambda n: engine.face_chips(n, 32), lambda r: len(r[2])),
        "face_masks": (lambda n: engine.face_masks(n, 32), lambda r: len(r[3])),
        "face_masks_shape": (lambda n: engine.face_masks_shape(n), lambda r: None),
        "face_redact": (lambda n: raw_face_redact(engine, n), lambda r: len(r[1])),
        "face_attrs": (lambda n: engine.face_attrs(n), lambda r: len(r)),
    }


def cell(call, rows_of):
    """The rows an accessor finds -- it serves exactly that many and refuses one more -- or the text it refuses with."""
    with pytest.raises(PeppaHipError) as e:
        call(1000)
    text = str(e.value).split(" failed: ", 1)[1]
    m = re.fullmatch(r"\w+: 1000 rows asked, the last call left (\d+)", text)
    if not m:
        return text
    n = int(m.group(1))
    got = rows_of(call(n))
    assert got is None or got == n
    with pytest.raises(PeppaHipError, match="%d rows asked, the last call left %d" % (n + 1, n)):
        call(n + 1)
    return n


def observe(engine):
    calls = accessor_calls(engine)
    return tuple(cell(*calls[a]) for a in ACCESSORS)


def check_last_call_rules(engine, weights, writer, between, want):
    blob = landmark_blob(weights)
    engine.load_program(0, blob, 4)
    frames, boxes, rows = scene()
    leave_rows(engine, writer, frames, boxes, rows)
    call_between(engine, between, blob, frames, boxes)
    assert observe(engine) == want


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_last_call_rules(emu_engine, student_weights, case):
    check_last_call_rules(emu_engine, student_weights, case[0], case[1], RULES[case])


def test_fresh_handle_has_no_rows(emu_engine, student_weights):
    emu_engine.load_program(0, landmark_blob(student_weights), 4)
    assert observe(emu_engine) == FORGOTTEN + (NO_ATTRS,)

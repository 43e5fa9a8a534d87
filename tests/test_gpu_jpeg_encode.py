"""pf_encode_jpeg on a real MI355X: the cases of tests/test_jpeg_encode.py (the restatement byte for byte at every shape, content
and sampling; batches, strides and unaligned device pointers; capacity; the round trip through the project's decoder; dispatch;
refusals) through the HIP library, then the product use: pf_face_redact / pf_face_chips into device memory followed by pf_encode_jpeg
on the same stream without a synchronisation, at 1080p -- 67.5 MCU rows in 4:2:0 -- against Pillow's encoding of what the host
accessors return, and the ``jpeg`` option of the Python classes."""
import numpy as np
import pytest
import torch

from peppa_pig_face_landmark_amd import _native
from peppa_pig_face_landmark_amd.graph.detector import build_detector_program
from peppa_pig_face_landmark_amd.graph.student import build_student_program
from peppa_pig_face_landmark_amd.synth import make_frame, plant_rows
from tests import test_jpeg_encode as T
from tests.test_gpu_face_redact import H, W, _scene

pytestmark = pytest.mark.gpu


def _dev_bytes(spec):
    t = torch.from_numpy(spec).cuda() if isinstance(spec, np.ndarray) else torch.full((spec[0],), spec[1], dtype=torch.uint8, device="cuda")
    return t.data_ptr(), lambda: t.cpu().numpy()


@pytest.mark.parametrize("shape", T.SHAPES, ids=T.SHAPE_IDS)
def test_engine_is_the_restatement(gpu_engine, shape):
    T.check_shape(gpu_engine, shape)


def test_batches_and_memory(gpu_engine):
    T.check_batches(gpu_engine, _dev_bytes, gpu_engine.sync)


def test_capacity(gpu_engine):
    T.check_capacity(gpu_engine)


def test_round_trip_through_the_decoder(gpu_engine):
    T.check_round_trip(gpu_engine)


def test_repeatability_and_dispatch(gpu_engine):
    T.check_repeatability(gpu_engine)


def test_refusals(gpu_engine):
    T.check_refusals(gpu_engine)


# ---- the product use: stages into device memory, then the encoder, one stream, no synchronisation ------------------------------------

@pytest.fixture(scope="module")
def blobs(student_weights, detector_weights):
    return (build_student_program(student_weights, 128, "f32")[0], build_detector_program(detector_weights, (384, 640), "f32s")[0])


def _face_scene(F, K, seed):
    """F synthetic frames with K faces each (the scene of tests/test_gpu_align_faces.py, whose chips are valid at S = 112), the planted
    detector rows and the boxes of the first frame"""
    frames, rows, boxes0 = [], [], None
    for f in range(F):
        frame, boxes = make_frame(H, W, K, seed=seed + f)
        boxes0 = boxes if boxes0 is None else boxes0
        frames.append(frame)
        rows.append(plant_rows(boxes, (H, W), 15120, (384, 640), 24, seed=seed + f))
    return np.stack(frames), np.stack(rows), boxes0


def _files(d_out, d_sizes, cap):
    out, sizes = d_out.cpu().numpy(), d_sizes.cpu().numpy()
    assert (sizes > 0).all(), sizes
    return [out[i * cap: i * cap + sizes[i]].tobytes() for i in range(len(sizes))]


def test_redact_then_encode_on_the_device(gpu_engine, blobs):
    F, K = 2, 3
    gpu_engine.load_program(0, blobs[0], 8)
    gpu_engine.load_program(1, blobs[1], 2)
    frames, rows, _ = _scene(F, K, seed=44)
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    cap = 3 * H * W + 4096                                     # noise at 1080p: about 1 byte per pixel at quality 85
    d_red = torch.empty((F, H, W, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.full((F * cap,), 0xAB, dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros((F,), dtype=torch.int32, device="cuda")
    gpu_engine.run_frames_device(d_frames.data_ptr(), F, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=rows.shape[1])
    for sampling in (420, 444):
        gpu_engine.face_redact_device(F * K, d_red.data_ptr(), mode="mosaic", strength=16, labels=0x3FE, pad=4)
        gpu_engine.encode_jpeg_device(d_red.data_ptr(), F, H, W, d_out.data_ptr(), cap, d_sizes.data_ptr(), quality=85, subsampling=sampling)
        gpu_engine.sync()
        files = _files(d_out, d_sizes, cap)
        host = gpu_engine.face_redact(F * K, mode="mosaic", strength=16, labels=0x3FE, pad=4)[0]      # the record is still there
        assert (host != frames).any()
        for f in range(F):
            want = T.pillow_encode(host[f], 85, sampling)
            assert files[f] == want, (sampling, f, T.first_difference(files[f], want))


def test_chips_then_encode_on_the_device(gpu_engine, blobs):
    F, K, S = 2, 5, 112
    gpu_engine.load_program(0, blobs[0], F * K)
    gpu_engine.load_program(1, blobs[1], 2)
    frames, rows, _ = _face_scene(F, 4, seed=31)              # four faces in five slots: slot 4 of every frame is invalid
    d_frames = torch.from_numpy(frames).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    cap = 3 * S * S + 4096
    d_chips = torch.full((F * K, S, S, 3), 0x55, dtype=torch.uint8, device="cuda")
    d_valid = torch.zeros((F * K,), dtype=torch.int32, device="cuda")
    d_out = torch.full((F * K * cap,), 0xAB, dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros((F * K,), dtype=torch.int32, device="cuda")
    gpu_engine.run_frames_device(d_frames.data_ptr(), F, H, W, 0.5, 0.3, 1600.0, K, d_planted=d_rows.data_ptr(), rows=rows.shape[1])
    gpu_engine.face_chips_device(F * K, S, d_chips.data_ptr(), d_valid=d_valid.data_ptr())
    gpu_engine.encode_jpeg_device(d_chips.data_ptr(), F * K, S, S, d_out.data_ptr(), cap, d_sizes.data_ptr(), quality=90, subsampling=420)
    gpu_engine.sync()
    files = _files(d_out, d_sizes, cap)
    chips, _, valid = gpu_engine.face_chips(F * K, S)
    assert np.array_equal(valid, d_valid.cpu().numpy().astype(bool)) and valid.any() and not valid.reshape(F, K)[:, 4].any()
    untouched = T.pillow_encode(np.full((S, S, 3), 0x55, np.uint8), 90, 420)
    for i in range(F * K):
        want = T.pillow_encode(chips[i], 90, 420) if valid[i] else untouched      # an invalid slot's chip is left as it was
        assert files[i] == want, (i, T.first_difference(files[i], want))


# ---- the Python classes ---------------------------------------------------------------------------------------------------------

REDACT = {"mode": "mosaic", "labels": 0x3FE, "strength": 16, "pad": 6}
JPEG = {"quality": 85, "subsampling": 420}


def _check_frame(data, raw):
    """the file decodes to what Pillow makes of its own encoding of the raw frame"""
    assert isinstance(data, bytes)
    assert np.array_equal(T.pillow_decode(data), T.pillow_decode(T.pillow_encode(raw, JPEG["quality"], JPEG["subsampling"])))


def _check_results(results, plain):
    """key for key the results without the option, plus chip_jpeg"""
    n = 0
    assert len(results) == len(plain)
    for r, r0 in zip(results, plain):
        assert set(r) == set(r0) | {"chip_jpeg"}
        for key in r0:
            assert np.array_equal(r[key], r0[key]), key
        if "chip" in r:
            _check_frame(r["chip_jpeg"], r["chip"])
            n += 1
        else:
            assert r["chip_jpeg"] is None
    return n


@pytest.mark.parametrize("which", ["faceana_host_tracking", "faceana_device_tracking", "stream_tracker", "frame_batch_runner"])
def test_classes_keep_jpeg_files(hip_library, student_weights, detector_weights, which):
    from Skps import FaceAna
    from peppa_pig_face_landmark_amd.core.api.batch_runner import FrameBatchRunner
    from peppa_pig_face_landmark_amd.core.api.facer import get_cfg
    from peppa_pig_face_landmark_amd.core.api.stream_tracker import StreamTracker
    frames, rows, boxes = _face_scene(2, 4, seed=120)
    weights = {"detector": detector_weights, "keypoints": student_weights}
    cfg = get_cfg()
    cfg["Skps"]["Detect"]["topk"] = 4
    cfg["Skps"]["Engine"]["device_tracking"] = which == "faceana_device_tracking"
    out, red, red_jpeg = {}, {}, {}
    for mode, jpeg in (("off", None), ("on", JPEG), ("files", dict(JPEG, raw=False))):
        kw = dict(cfg=cfg, weights=weights, library=hip_library, redact=REDACT, face_chips=112, jpeg=jpeg)
        if which.startswith("faceana"):
            obj = FaceAna(**kw)
            obj._planted_rows = lambda: rows[0]
            if which == "faceana_host_tracking":
                obj.face_detector = lambda image: np.concatenate([boxes, np.ones((len(boxes), 1), np.float32)], 1)
            out[mode], red[mode], red_jpeg[mode] = [], [], []
            for _ in range(2):                               # a detector frame and a tracked one
                out[mode].append(obj.run(frames[0]))
                red[mode].append(obj.last_redacted)
                red_jpeg[mode].append(obj.last_redacted_jpeg)
            obj.engine.close()
        elif which == "stream_tracker":
            obj = StreamTracker(max_streams=2, **kw)
            obj._planted_rows = lambda ids, fr: rows[:len(ids)]
            r = obj.run({0: frames[0], 1: frames[1]})
            out[mode] = [r[0], r[1]]
            red[mode] = [obj.last_redacted[s] for s in (0, 1)] if obj.last_redacted is not None else [None, None]
            red_jpeg[mode] = [obj.last_redacted_jpeg[s] for s in (0, 1)] if obj.last_redacted_jpeg is not None else [None, None]
            obj.close()
        else:
            obj = FrameBatchRunner(lanes=2, frames_per_lane=1, **kw)
            obj._planted_rows = lambda fr: rows[:len(fr)]
            out[mode] = obj.run(frames)
            red[mode] = list(obj.last_redacted) if obj.last_redacted is not None else [None, None]
            red_jpeg[mode] = list(obj.last_redacted_jpeg) if obj.last_redacted_jpeg is not None else [None, None]
            obj.close()
    chips = 0
    for i in range(2):
        # off: exactly today's attributes and keys
        assert red_jpeg["off"][i] is None and red["off"][i] is not None
        assert all("chip_jpeg" not in r for r in out["off"][i])
        # on: the same raw outputs, and the files next to them
        assert np.array_equal(red["on"][i], red["off"][i])
        _check_frame(red_jpeg["on"][i], red["on"][i])
        chips += _check_results(out["on"][i], out["off"][i])
        # raw = False: the same files, no raw copies
        assert red["files"][i] is None and red_jpeg["files"][i] == red_jpeg["on"][i]
        for r, r1 in zip(out["files"][i], out["on"][i]):
            assert set(r) == set(r1) - {"chip"} and r["chip_jpeg"] == r1["chip_jpeg"]
    assert chips >= 1

"""ctypes binding of ``libpeppa_hip.so`` (C ABI: ``include/peppa_hip.h``).

No torch, no onnxruntime: numpy arrays in, numpy arrays out.  There is deliberately no CPU
fallback -- if the HIP library is missing or no GPU is visible, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import numpy as np

PF_MEM_HOST, PF_MEM_DEVICE, PF_MEM_RESIDENT, PF_MEM_HOST_PINNED = 0, 1, 2, 3
PF_MEM_ROWS_DEVICE = 0x100
PF_NET_LANDMARK, PF_NET_DETECTOR = 0, 1
PF_INPUT_U8_NHWC, PF_INPUT_F32_NCHW = 0, 1
PF_OPT_HIP_GRAPH = 1
PF_OPT_RANGE_CHECK = 2
PF_OPT_JPEG_ENTROPY, PF_OPT_JPEG_SYNC_ROUNDS = 3, 4       # entropy decoding: 0 automatic / 1 host / 2 device; sync rounds 1..10 (0 = all)
PF_OPT_BATCH_FRONT = 5      # BatchEngine.set_option only: 1 (default) detector + NMS once per call on the front engine, 0 per lane
PF_OPT_DET_TILE = 6         # testing / tuning: 0 the engine picks the det_unit / det_c3 tile, th << 16 | tw forces it (det_tile_option)
PF_COMM_ID_BYTES = 128


def det_tile_option(th: int, tw: int) -> int:
    """Value of ``PF_OPT_DET_TILE`` that forces a th x tw tile."""
    return (int(th) << 16) | int(tw)

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, "libpeppa_hip.so")

_lib_cache = {}


class PeppaHipError(RuntimeError):
    pass


def _declare(lib):
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.pf_version.restype = C.c_char_p
    lib.pf_version.argtypes = []
    lib.pf_create.argtypes = [i, C.POINTER(vp)]
    lib.pf_destroy.argtypes = [vp]
    lib.pf_destroy.restype = None
    lib.pf_last_error.argtypes = [vp]
    lib.pf_last_error.restype = C.c_char_p
    lib.pf_sync.argtypes = [vp]
    lib.pf_load_program.argtypes = [vp, i, vp, sz, i]
    lib.pf_landmark_forward.argtypes = [vp, vp, i, i, i, vp, vp, i]
    lib.pf_detector_forward.argtypes = [vp, vp, i, i, i, vp, i]
    lib.pf_read_tensor.argtypes = [vp, i, i, i, fp, sz]
    if hasattr(lib, "pf_face_attrs"):      # absent from builds that predate it (tools/compare_libs.py loads those too)
        lib.pf_face_attrs.argtypes = [vp, i, vp, i, i]
        lib.pf_face_attrs.restype = i
        lib.pf_batch_face_attrs.argtypes = [vp, i, vp, i, i]
        lib.pf_batch_face_attrs.restype = i
    if hasattr(lib, "pf_align_faces"):     # likewise
        lib.pf_align_faces.argtypes = [vp, vp, i, i, i, i, vp, i, i, vp, i, i, vp, vp, vp, i]
        lib.pf_face_chips.argtypes = [vp, i, i, vp, vp, vp, i]
        lib.pf_batch_face_chips.argtypes = [vp, i, i, vp, vp, vp, i]
        for name in ("pf_align_faces", "pf_face_chips", "pf_batch_face_chips"):
            getattr(lib, name).restype = i
    if hasattr(lib, "pf_mask_faces"):      # likewise
        lib.pf_mask_faces.argtypes = [vp, i, i, i, vp, i, i, vp, i, i, vp, vp, vp, vp, i]
        lib.pf_face_masks.argtypes = [vp, i, i, vp, vp, vp, vp, i]
        lib.pf_batch_face_masks.argtypes = [vp, i, i, vp, vp, vp, vp, i]
        lib.pf_face_masks_shape.argtypes = [vp, i, ip, ip, ip]
        lib.pf_batch_face_masks_shape.argtypes = [vp, i, ip, ip, ip]
        for name in ("pf_mask_faces", "pf_face_masks", "pf_batch_face_masks", "pf_face_masks_shape", "pf_batch_face_masks_shape"):
            getattr(lib, name).restype = i
    if hasattr(lib, "pf_redact_faces"):    # likewise
        u = C.c_uint
        lib.pf_redact_faces.argtypes = [vp, vp, i, i, i, i, vp, i, i, vp, vp, i, i, i, i, i, u, vp, vp, i]
        lib.pf_face_redact.argtypes = [vp, i, vp, i, i, i, i, u, vp, vp, i]
        lib.pf_batch_face_redact.argtypes = [vp, i, vp, i, i, i, i, u, vp, vp, i]
        for name in ("pf_redact_faces", "pf_face_redact", "pf_batch_face_redact"):
            getattr(lib, name).restype = i
    if hasattr(lib, "pf_measure_faces"):   # likewise
        lib.pf_measure_faces.argtypes = [vp, vp, i, i, i, i, vp, i, i, vp, i, i, i, vp, vp, i]
        lib.pf_face_stats.argtypes = [vp, i, i, i, vp, vp, i]
        lib.pf_batch_face_stats.argtypes = [vp, i, i, i, vp, vp, i]
        for name in ("pf_measure_faces", "pf_face_stats", "pf_batch_face_stats"):
            getattr(lib, name).restype = i
    if hasattr(lib, "pf_draw_faces"):      # likewise
        lib.pf_draw_faces.argtypes = [vp, vp, i, i, i, i, vp, i, i, vp, vp, i, vp, vp, vp, i]
        lib.pf_face_draw.argtypes = [vp, i, vp, vp, vp, vp, vp, i]
        lib.pf_batch_face_draw.argtypes = [vp, i, vp, vp, vp, vp, vp, i]
        for name in ("pf_draw_faces", "pf_face_draw", "pf_batch_face_draw"):
            getattr(lib, name).restype = i
    lib.pf_detect.argtypes = [vp, vp, i, i, i, i, f, f, fp, i, ip]
    lib.pf_landmarks.argtypes = [vp, vp, i, i, i, i, fp, i, fp, fp, ip]
    lib.pf_landmarks_f64.argtypes = [vp, vp, i, i, i, i, C.POINTER(C.c_double), i, fp, fp, ip]
    lib.pf_landmarks_f64.restype = i
    lib.pf_crop_faces_f64.argtypes = [vp, vp, i, i, i, i, C.POINTER(C.c_double), i, i, vp, ip]
    lib.pf_crop_faces_f64.restype = i
    dp = C.POINTER(C.c_double)
    lib.pf_track_frame.argtypes = [vp, vp, i, i, i, i, f, f, f, i, f, f, f, i, ip, dp, dp, fp, ip]
    lib.pf_track_frame.restype = i
    lib.pf_track_frame_planted.argtypes = [vp, vp, i, i, i, i, fp, i, f, f, f, i, f, f, f, ip, dp, dp, fp, ip]
    lib.pf_track_frame_planted.restype = i
    lib.pf_track_reset.argtypes = [vp]
    lib.pf_track_reset.restype = i
    lib.pf_track_streams_config.argtypes = [vp, i, i]
    lib.pf_track_streams_config.restype = i
    lib.pf_track_streams.argtypes = [vp, i, ip, vp, i, i, i, fp, i, f, f, f, f, f, f, ip, dp, dp, fp, ip]
    lib.pf_track_streams.restype = i
    lib.pf_track_streams_reset.argtypes = [vp, i]
    lib.pf_track_streams_reset.restype = i
    lib.pf_track_ids_config.argtypes = [vp, i, i]
    lib.pf_track_ids_config.restype = i
    lib.pf_track_ids.argtypes = [vp, i, vp, vp, i]
    lib.pf_track_ids.restype = i
    lib.pf_run_frames.argtypes = [vp, vp, i, i, i, i, f, f, f, i, vp, vp, vp, vp, i]
    lib.pf_run_frames_planted.argtypes = [vp, vp, i, i, i, i, vp, i, f, f, f, i, vp, vp, vp, vp, i]
    lib.pf_letterbox.argtypes = [vp, vp, i, i, i, i, i, i, vp, fp]
    lib.pf_nms_rows.argtypes = [vp, fp, i, f, f, f, f, f, fp, i, ip]
    lib.pf_resize.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    lib.pf_resize.restype = i
    lib.pf_crop_faces.argtypes = [vp, vp, i, i, i, i, fp, i, i, vp, ip]
    lib.pf_jpeg_info.argtypes = [vp, sz, ip, ip, ip, ip]
    lib.pf_decode_jpeg.argtypes = [vp, vp, sz, ip, ip, C.POINTER(vp), vp]
    lib.pf_decode_jpeg_batch.argtypes = [vp, i, C.POINTER(vp), C.POINTER(sz), i, ip, ip, C.POINTER(vp)]
    lib.pf_encode_jpeg.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, sz, vp, i]
    lib.pf_encode_jpeg.restype = i
    lib.pf_encode_jpeg_bound.argtypes = [i, i, i]
    lib.pf_encode_jpeg_bound.restype = sz
    lib.pf_device_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.pf_device_alloc.restype = i
    lib.pf_device_free.argtypes = [vp, vp]
    lib.pf_device_free.restype = i
    lib.pf_set_frame.argtypes = [vp, vp, i, i, i, i, C.POINTER(C.c_ulonglong), ip]
    lib.pf_forget_frames.argtypes = [vp]
    lib.pf_set_option.argtypes = [vp, i, i]
    lib.pf_profile_enable.argtypes = [vp, i]
    lib.pf_profile_fetch.argtypes = [vp, C.c_char_p, sz, fp, ip, i, ip]
    lib.pf_launch_log.argtypes = [vp, C.c_char_p, sz, ip, C.POINTER(sz)]
    lib.pf_host_alloc.argtypes = [sz, C.POINTER(vp)]
    lib.pf_host_free.argtypes = [vp]
    lib.pf_host_alloc.restype = i
    lib.pf_host_free.restype = i
    lib.pf_comm_unique_id.argtypes = [vp, sz]
    lib.pf_rccl_version.argtypes = [ip]
    lib.pf_broadcast_weights.argtypes = [vp, vp, i, i, i, vp, sz, C.POINTER(sz), i, fp]
    lib.pf_comm_destroy.argtypes = [vp]
    lib.pf_batch_create.argtypes = [i, i, C.POINTER(vp)]
    lib.pf_batch_destroy.argtypes = [vp]
    lib.pf_batch_destroy.restype = None
    lib.pf_batch_last_error.argtypes = [vp]
    lib.pf_batch_last_error.restype = C.c_char_p
    lib.pf_batch_lanes.argtypes = [vp]
    lib.pf_batch_lane.argtypes = [vp, i]
    lib.pf_batch_lane.restype = vp
    lib.pf_batch_front.argtypes = [vp]
    lib.pf_batch_front.restype = vp
    lib.pf_batch_load_program.argtypes = [vp, i, vp, sz, i]
    lib.pf_batch_set_option.argtypes = [vp, i, i]
    lib.pf_batch_sync.argtypes = [vp]
    lib.pf_batch_run_frames.argtypes = [vp, vp, i, i, i, i, vp, i, f, f, f, i, vp, vp, vp, vp, i]
    for name in ("pf_batch_create", "pf_batch_lanes", "pf_batch_load_program", "pf_batch_set_option", "pf_batch_sync", "pf_batch_run_frames"):
        getattr(lib, name).restype = i
    for name in ("pf_comm_unique_id", "pf_rccl_version", "pf_broadcast_weights", "pf_comm_destroy"):
        getattr(lib, name).restype = i
    for name in ("pf_create", "pf_sync", "pf_load_program", "pf_landmark_forward", "pf_detector_forward",
                 "pf_read_tensor", "pf_detect", "pf_landmarks", "pf_run_frames", "pf_run_frames_planted",
                 "pf_profile_enable", "pf_profile_fetch", "pf_launch_log", "pf_letterbox", "pf_nms_rows", "pf_crop_faces", "pf_set_frame", "pf_forget_frames", "pf_set_option"):
        getattr(lib, name).restype = i
    return lib


def load_library(path: Optional[str] = None):
    """dlopen the engine.  ``path`` defaults to the in-tree ``libpeppa_hip.so`` built by
    ``__graft_entry__.build()`` / ``python -m peppa_pig_face_landmark_amd.build``."""
    path = os.path.abspath(path or os.environ.get("PEPPA_HIP_LIBRARY", DEFAULT_LIBRARY))
    if path in _lib_cache:
        return _lib_cache[path]
    if not os.path.exists(path):
        raise PeppaHipError(
            f"{path} not found: build it with `python -m peppa_pig_face_landmark_amd.build` "
            "(hipcc --offload-arch=gfx950).  The engine has no CPU fallback.")
    lib = _declare(C.CDLL(path))
    _lib_cache[path] = lib
    return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


def _kps_arg(kps):
    """Landmarks as the C ABI takes them: (float32 or float64 [F,top_k,98,2], contiguous; its kps_f64 flag; F; top_k).
    [top_k,98,2] is one frame."""
    k = np.asarray(kps)
    k = np.ascontiguousarray(k, np.float64 if k.dtype == np.float64 else np.float32)
    if k.ndim == 3:
        k = k[None]
    if k.ndim != 4 or k.shape[2:] != (98, 2):
        raise ValueError("kps must be [F,top_k,98,2]")
    return k, 1 if k.dtype == np.float64 else 0, k.shape[0], k.shape[1]


# ---- host outputs of the last-call accessors, shared by Engine (pf_face_*) and BatchEngine (pf_batch_face_*) -------------------------
def _last_call_attrs(check, fn, handle, what, rows, raw):
    out = np.zeros((int(rows), 7), np.float32)
    check(fn(handle, int(rows), _ptr(out), 1 if raw else 0, PF_MEM_HOST), what)
    return out


def _last_call_chips(check, fn, handle, what, rows, chip_size, out=None):
    S, rows = int(chip_size), int(rows)
    chips, mats = out if out is not None else (np.zeros((rows, max(S, 0), max(S, 0), 3), np.uint8), np.zeros((rows, 2, 3), np.float64))
    valid = np.zeros((rows,), np.int32)
    check(fn(handle, rows, S, _ptr(chips), _ptr(mats), _ptr(valid), PF_MEM_HOST), what)
    return chips, mats, valid.astype(bool)


def _last_call_masks(check, fn, fn_shape, handle, what, rows, chip_size, owners, boxes):
    """Host-output pf_face_masks / pf_batch_face_masks: the frame-space maps take the shape the library reports for `rows`."""
    S, rows = int(chip_size), int(rows)
    valid = np.zeros((rows,), np.int32)
    if S:
        labels, own, box = np.zeros((rows, max(S, 0), max(S, 0)), np.uint8), None, None
    else:
        F, H, W = C.c_int(0), C.c_int(0), C.c_int(0)
        check(fn_shape(handle, rows, C.byref(F), C.byref(H), C.byref(W)), what)
        labels = np.zeros((F.value, H.value, W.value), np.uint8)
        own = np.zeros_like(labels) if owners else None
        box = np.zeros((rows, 4), np.int32) if boxes else None
    check(fn(handle, rows, S, _ptr(labels), _ptr(own), _ptr(box), _ptr(valid), PF_MEM_HOST), what)
    return labels, own, box, valid.astype(bool)


PF_REDACT_FILL, PF_REDACT_MOSAIC, PF_REDACT_BLUR = 0, 1, 2
PF_REDACT_BACKGROUND, PF_REDACT_FACE_ALL, PF_REDACT_BOX = 0x001, 0x1FE, 0x200
_REDACT_MODES = {"fill": PF_REDACT_FILL, "mosaic": PF_REDACT_MOSAIC, "blur": PF_REDACT_BLUR}


def _redact_args(mode, labels, strength, pad, colour):
    """The five redaction parameters as the C ABI takes them; mode is "fill" / "mosaic" / "blur" or its number, colour an int
    (the low byte is channel 0) or a (c0, c1, c2) tuple."""
    m = _REDACT_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if isinstance(m, str):
        raise ValueError("mode must be 'fill', 'mosaic' or 'blur' (got %r)" % (mode,))
    if not isinstance(colour, (int, np.integer)):
        c = [int(v) & 255 for v in colour]
        colour = c[0] | (c[1] << 8) | (c[2] << 16)
    return int(m), int(labels), int(strength), int(pad), C.c_uint(int(colour) & 0xFFFFFFFF)


def _last_call_redact(check, fn, fn_shape, handle, what, rows, select, args):
    """Host-output pf_face_redact / pf_batch_face_redact: the frames take the shape the library reports for `rows`."""
    rows = int(rows)
    F, H, W = C.c_int(0), C.c_int(0), C.c_int(0)
    check(fn_shape(handle, rows, C.byref(F), C.byref(H), C.byref(W)), what)
    out = np.zeros((F.value, H.value, W.value, 3), np.uint8)
    valid = np.zeros((rows,), np.int32)
    sel = None if select is None else np.ascontiguousarray(select, np.int32).reshape(rows)
    check(fn(handle, rows, _ptr(sel), *args, _ptr(out), _ptr(valid), PF_MEM_HOST), what)
    return out, valid.astype(bool)


PF_STATS_LABELS, PF_STATS_FIELDS = 8, 9


def _last_call_stats(check, fn, handle, what, rows, dark, bright):
    """Host-output pf_face_stats / pf_batch_face_stats."""
    rows = int(rows)
    stats = np.zeros((rows, PF_STATS_LABELS, PF_STATS_FIELDS), np.uint64)
    valid = np.zeros((rows,), np.int32)
    check(fn(handle, rows, int(dark), int(bright), _ptr(stats), _ptr(valid), PF_MEM_HOST), what)
    return stats, valid.astype(bool)


PF_DRAW_POINTS, PF_DRAW_CONTOURS, PF_DRAW_BOX = 1, 2, 4
_DRAW_WHAT = {"points": PF_DRAW_POINTS, "contours": PF_DRAW_CONTOURS, "box": PF_DRAW_BOX}


class DrawStyle(C.Structure):
    """pf_draw_style of include/peppa_hip.h."""
    _fields_ = [("what", C.c_int), ("point_radius", C.c_int), ("line_width", C.c_int), ("alpha", C.c_int), ("score_thres", C.c_float),
                ("colour_hi", C.c_uint), ("colour_lo", C.c_uint), ("colour_contour", C.c_uint), ("colour_box", C.c_uint)]


def _colour_arg(colour):
    if not isinstance(colour, (int, np.integer)):
        c = [int(v) & 255 for v in colour]
        colour = c[0] | (c[1] << 8) | (c[2] << 16)
    return int(colour) & 0xFFFFFFFF


def _draw_style(what=("points",), point_radius=2, line_width=1, alpha=256, score_thres=0.8, colour_hi=(255, 255, 255),
                colour_lo=(0, 0, 255), colour_contour=(0, 255, 0), colour_box=(255, 255, 0)):
    """The overlay's parameters as the C ABI takes them; what is the bit mask or names out of "points", "contours", "box";
    a colour is an int (the low byte is channel 0) or a (c0, c1, c2) tuple."""
    if isinstance(what, str):
        what = (what,)
    if not isinstance(what, (int, np.integer)):
        bits = 0
        for w in what:
            if w not in _DRAW_WHAT:
                raise ValueError("what holds 'points', 'contours' and 'box' (got %r)" % (w,))
            bits |= _DRAW_WHAT[w]
        what = bits
    return DrawStyle(int(what), int(point_radius), int(line_width), int(alpha), float(score_thres), _colour_arg(colour_hi),
                     _colour_arg(colour_lo), _colour_arg(colour_contour), _colour_arg(colour_box))


def _last_call_draw(check, fn, fn_shape, handle, what, rows, scores, base, style):
    """Host-output pf_face_draw / pf_batch_face_draw: the frames take the shape the library reports for `rows`."""
    rows = int(rows)
    F, H, W = C.c_int(0), C.c_int(0), C.c_int(0)
    check(fn_shape(handle, rows, C.byref(F), C.byref(H), C.byref(W)), what)
    out = np.zeros((F.value, H.value, W.value, 3), np.uint8)
    valid = np.zeros((rows,), np.int32)
    sc = None if scores is None else np.ascontiguousarray(scores, np.float32).reshape(rows, 98)
    check(fn(handle, rows, _ptr(sc), C.byref(style), _ptr(int(base)) if base else None, _ptr(out), _ptr(valid), PF_MEM_HOST), what)
    return out, valid.astype(bool)


class DeviceFrame:
    """A packed BGR uint8 frame that already lives in device memory (``Engine.imread`` / ``decode_jpeg``): accepted wherever the
    engine takes a frame.  ``shape`` mirrors the numpy array cv2.imread would have returned; ``numpy()`` is the host copy
    (for drawing).  The memory belongs to the engine and is reused by its next decode: consume the frame first (``FaceAna.run``
    copies it into its resident-frame slot on the device)."""

    def __init__(self, ptr: int, height: int, width: int, host: Optional[np.ndarray] = None):
        self.ptr, self.shape, self._host = int(ptr), (int(height), int(width), 3), host
        self.dtype = np.dtype(np.uint8)

    def numpy(self) -> np.ndarray:
        if self._host is None:
            raise PeppaHipError("this DeviceFrame was decoded without a host copy (imread(..., want_host=False))")
        return self._host


class Engine:
    """One engine == one GPU + one HIP stream (``pf_handle``)."""

    def __init__(self, device: int = 0, library: Optional[str] = None):
        self.lib = load_library(library)
        self.h = C.c_void_p()
        if self.lib.pf_create(int(device), C.byref(self.h)) != 0:
            msg = self.lib.pf_last_error(None)
            raise PeppaHipError("pf_create failed: " + (msg.decode() if msg else "unknown"))
        self.device = device
        self._programs = {}

    def pinned_empty(self, shape, dtype=np.uint8) -> np.ndarray:
        """Page-locked host array (pf_host_alloc): decode frames straight into it and pass it to run_frames* so the
        host->device copy is asynchronous.  Freed by close(); do not use the array afterwards."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        if self.lib.pf_host_alloc(nbytes, C.byref(p)) != 0 or not p.value:
            raise PeppaHipError("pf_host_alloc(%d bytes) failed" % nbytes)
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p)
        buf = (C.c_ubyte * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def run_frames_host_async(self, frames: np.ndarray, d_planted: int, rows: int, score_thres: float, iou_thres: float,
                              min_face: float, top_k: int, d_counts: int, d_boxes: int, d_kps: int, d_scores: int):
        """Host-resident frames (ideally from pinned_empty) in, device-resident results out, no synchronisation:
        the call returns after enqueueing the copy and the kernels on this engine's stream.  Planted detector rows
        (benchmark instrument) are passed as a device pointer."""
        F, H, W, _ = frames.shape
        assert frames.dtype == np.uint8 and frames.flags["C_CONTIGUOUS"]
        rc = self.lib.pf_run_frames_planted(self.h, _ptr(frames), PF_MEM_HOST | PF_MEM_ROWS_DEVICE, F, H, W,
                                            _ptr(d_planted) if d_planted else None, rows, score_thres, iou_thres,
                                            min_face, top_k, _ptr(d_counts), _ptr(d_boxes), _ptr(d_kps), _ptr(d_scores),
                                            PF_MEM_DEVICE)
        self._check(rc, "pf_run_frames_planted")

    def close(self):
        for p in getattr(self, "_pinned", []):
            self.lib.pf_host_free(p)
        self._pinned = []
        if getattr(self, "h", None) is not None and self.h:
            for ptr, _ in self.__dict__.pop("_device_buffers", {}).values():
                self.lib.pf_device_free(self.h, C.c_void_p(ptr))
            if not getattr(self, "_borrowed", False):      # a lane of a BatchEngine belongs to its pf_batch
                self.lib.pf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def version(self) -> str:
        return self.lib.pf_version().decode()

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.pf_last_error(self.h)
            raise PeppaHipError(f"{what} failed: " + (msg.decode() if msg else "unknown"))

    def sync(self):
        self._check(self.lib.pf_sync(self.h), "pf_sync")

    def load_program(self, slot: int, blob: bytes, max_batch: int):
        buf = C.create_string_buffer(blob, len(blob))
        self._check(self.lib.pf_load_program(self.h, slot, C.cast(buf, C.c_void_p), len(blob), int(max_batch)),
                    "pf_load_program")
        self._programs[slot] = max_batch

    # ---- multi-GPU: one-time RCCL broadcast of the packed programs (include/peppa_hip.h) ----------------
    @staticmethod
    def comm_unique_id(library: Optional[str] = None) -> bytes:
        """Rank 0: a fresh RCCL unique id (128 bytes) to hand to the other ranks out of band."""
        lib = load_library(library)
        buf = C.create_string_buffer(PF_COMM_ID_BYTES)
        if lib.pf_comm_unique_id(C.cast(buf, C.c_void_p), PF_COMM_ID_BYTES) != 0:
            msg = lib.pf_last_error(None)
            raise PeppaHipError("pf_comm_unique_id failed: " + (msg.decode() if msg else "unknown"))
        return buf.raw

    def rccl_version(self) -> int:
        v = C.c_int(0)
        if self.lib.pf_rccl_version(C.byref(v)) != 0:
            msg = self.lib.pf_last_error(None)
            raise PeppaHipError("pf_rccl_version failed: " + (msg.decode() if msg else "unknown"))
        return v.value

    def broadcast_weights(self, unique_id: bytes, rank: int, world: int, slot: int, blob: Optional[bytes],
                          max_batch: int, capacity: int = 64 << 20) -> Tuple[bytes, float]:
        """Collective: rank 0 passes its packed program, the other ranks pass None; every rank ends up with the
        program loaded into `slot`.  Returns (blob bytes, device milliseconds of the ncclBroadcast)."""
        assert len(unique_id) == PF_COMM_ID_BYTES
        if rank == 0:
            assert blob is not None
            capacity = len(blob)
            buf = C.create_string_buffer(blob, len(blob))
        else:
            buf = C.create_string_buffer(capacity)
        n = C.c_size_t(len(blob) if rank == 0 else 0)
        ms = C.c_float(0.0)
        idb = C.create_string_buffer(unique_id, PF_COMM_ID_BYTES)
        self._check(self.lib.pf_broadcast_weights(self.h, C.cast(idb, C.c_void_p), int(rank), int(world), int(slot),
                                                  C.cast(buf, C.c_void_p), capacity, C.byref(n), int(max_batch), C.byref(ms)),
                    "pf_broadcast_weights")
        self._programs[slot] = max_batch
        return buf.raw[:n.value], float(ms.value)

    # ---- network seams ------------------------------------------------------------------------
    def landmark_forward(self, x: np.ndarray, attrs: bool = False):
        """x: uint8 [B,S,S,3] or float32 [B,3,S,S] -> (loc_fix [B,196], score [B,98]).  ``attrs=True`` (a program built with
        ``face_attrs=True``): + the raw fc-head output [B,7] of the same faces (``face_attrs(B, raw=True)``)."""
        if x.dtype == np.uint8:
            kind, batch = PF_INPUT_U8_NHWC, x.shape[0]
        elif x.dtype == np.float32:
            kind, batch = PF_INPUT_F32_NCHW, x.shape[0]
        else:
            raise TypeError("landmark input must be uint8 NHWC or float32 NCHW")
        x = np.ascontiguousarray(x)
        loc = np.empty((batch, 196), np.float32)
        score = np.empty((batch, 98), np.float32)
        self._check(self.lib.pf_landmark_forward(self.h, _ptr(x), kind, PF_MEM_HOST, batch, _ptr(loc), _ptr(score),
                                                 PF_MEM_HOST), "pf_landmark_forward")
        if attrs:
            return loc, score, self.face_attrs(batch, raw=True)
        return loc, score

    def face_attrs(self, rows: int, raw: bool = False) -> np.ndarray:
        """Face attributes [rows, 7] of the faces of the handle's last pf_landmark_forward / pf_landmarks / pf_run_frames /
        pf_track_frame / pf_track_streams call, in that call's row order (include/peppa_hip.h pf_face_attrs).  raw=True: Net's x (pose / 90, four logits); raw=False: pose in degrees
        (about x, y, z) then P(eye 60-67 closed), P(eye 68-75 closed), P(mouth closed), P(mouth wide open)."""
        return _last_call_attrs(self._check, self.lib.pf_face_attrs, self.h, "pf_face_attrs", rows, raw)

    def face_attrs_device(self, rows: int, d_out: int, raw: bool = False):
        """Same into device memory, enqueued on the handle's stream."""
        self._check(self.lib.pf_face_attrs(self.h, int(rows), _ptr(d_out), 1 if raw else 0, PF_MEM_DEVICE), "pf_face_attrs")

    def _frames_arg(self, frames, F):
        """``frames`` of align_faces / redact_faces, which must be the ``F`` frames the landmarks belong to: (pointer, mem, F, H, W,
        the host array to keep alive over the call or None)."""
        if frames is None:
            shp = getattr(self, "_resident_shape", None)
            if shp is None:
                raise PeppaHipError("no resident frame: call set_frame() first")
            fptr, mem, nf, H, W, keep = None, PF_MEM_RESIDENT, F, shp[0], shp[1], None
        elif isinstance(frames, tuple):
            fptr, mem, (nf, H, W), keep = C.c_void_p(int(frames[0])), PF_MEM_DEVICE, (int(v) for v in frames[1:]), None
        else:
            keep = np.ascontiguousarray(frames)
            if keep.ndim == 3:
                keep = keep[None]
            if keep.dtype != np.uint8 or keep.ndim != 4 or keep.shape[3] != 3:
                raise ValueError("frames must be uint8 [F,H,W,3]")
            fptr, mem, (nf, H, W) = _ptr(keep), PF_MEM_HOST, keep.shape[:3]
        if nf != F:
            raise ValueError("%d frames, landmarks of %d" % (nf, F))
        return fptr, mem, F, H, W, keep

    # ---- aligned face chips (include/peppa_hip.h pf_align_faces / pf_face_chips) -------------------------------------------------
    def align_faces(self, frames, kps: np.ndarray, counts: Optional[np.ndarray] = None, chip_size: int = 112, out=None):
        """Similarity-warped face chips.  frames: uint8 [F,H,W,3] (or [H,W,3]), ``None`` for the resident frame of set_frame(), or
        ``(device pointer, F, H, W)``; kps: float32 or float64 [F,top_k,98,2] (or [top_k,98,2] for one frame); counts: [F] live slots
        per frame (None: all).  Returns (chips uint8 [F,top_k,S,S,3], mats float64 [F,top_k,2,3] frame -> chip, valid bool [F,top_k]);
        chips and matrices of invalid slots are left as they were (zero, or what ``out = (chips, mats)`` held)."""
        k, f64, F, K = _kps_arg(kps)
        fptr, mem, F, H, W, _keep = self._frames_arg(frames, F)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        S = int(chip_size)
        chips, mats = out if out is not None else (np.zeros((F, K, max(S, 0), max(S, 0), 3), np.uint8), np.zeros((F, K, 2, 3), np.float64))
        valid = np.zeros((F, K), np.int32)
        self._check(self.lib.pf_align_faces(self.h, fptr, mem, F, H, W, _ptr(k), f64, PF_MEM_HOST, _ptr(c), K, S, _ptr(chips), _ptr(mats),
                                            _ptr(valid), PF_MEM_HOST), "pf_align_faces")
        return chips, mats, valid.astype(bool)

    def align_faces_device(self, frames, kps: np.ndarray, d_chips: int, counts: Optional[np.ndarray] = None, chip_size: int = 112):
        """align_faces with the chips [F,top_k,S,S,3] written to device memory, enqueued on the handle's stream (no matrices, no
        valid flags: chips of invalid slots are left as they were)."""
        k, f64, F, K = _kps_arg(kps)
        fptr, mem, F, H, W, _keep = self._frames_arg(frames, F)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        self._check(self.lib.pf_align_faces(self.h, fptr, mem, F, H, W, _ptr(k), f64, PF_MEM_HOST, _ptr(c), K, int(chip_size), _ptr(int(d_chips)),
                                            None, None, PF_MEM_DEVICE), "pf_align_faces")

    def face_chips(self, rows: int, chip_size: int = 112, out=None):
        """Chips of the faces of the handle's last pf_landmarks / pf_run_frames / pf_track_frame / pf_track_streams call, in that
        call's row order (include/peppa_hip.h pf_face_chips): (chips uint8 [rows,S,S,3], mats float64 [rows,2,3], valid bool [rows])."""
        return _last_call_chips(self._check, self.lib.pf_face_chips, self.h, "pf_face_chips", rows, chip_size, out)

    def face_chips_device(self, rows: int, chip_size: int, d_chips: int, d_mats: int = 0, d_valid: int = 0):
        """Same into device memory, enqueued on the handle's stream."""
        self._check(self.lib.pf_face_chips(self.h, int(rows), int(chip_size), _ptr(d_chips), _ptr(d_mats) if d_mats else None,
                                           _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE), "pf_face_chips")

    # ---- face-region label maps (include/peppa_hip.h pf_mask_faces / pf_face_masks) ----------------------------------------------
    def mask_faces(self, kps: np.ndarray, height: int = 0, width: int = 0, counts: Optional[np.ndarray] = None, chip_size: int = 0,
                   owners: bool = True, boxes: bool = True, out=None):
        """Face-region label maps from landmarks alone.  kps: float32 or float64 [F,top_k,98,2] (or [top_k,98,2] for one frame);
        counts: [F] live slots per frame (None: all).  Frame space (``chip_size = 0``): (labels uint8 [F,height,width], owners uint8
        like labels or None, boxes int32 [F,top_k,4] or None, valid bool [F,top_k]).  Chip space: (labels uint8 [F,top_k,S,S], None,
        None, valid); maps of invalid slots, like box rows of invalid slots, are left as they were (zero, or what
        ``out = (labels, owners, boxes)`` held)."""
        k, f64, F, K = _kps_arg(kps)
        S, H, W = int(chip_size), int(height), int(width)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        if out is not None:
            labels, own, box = out
        elif S:
            labels, own, box = np.zeros((F, K, max(S, 0), max(S, 0)), np.uint8), None, None
        else:
            labels = np.zeros((F, max(H, 0), max(W, 0)), np.uint8)
            own = np.zeros_like(labels) if owners else None
            box = np.zeros((F, K, 4), np.int32) if boxes else None
        valid = np.zeros((F, K), np.int32)
        self._check(self.lib.pf_mask_faces(self.h, F, H, W, _ptr(k), f64, PF_MEM_HOST, _ptr(c), K, S,
                                           _ptr(labels), _ptr(own), _ptr(box), _ptr(valid), PF_MEM_HOST), "pf_mask_faces")
        return labels, own, box, valid.astype(bool)

    def face_masks_shape(self, rows: int):
        """(n_frames, height, width) of the frame-space maps ``rows`` rows of the handle's last pipeline call need."""
        F, H, W = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.pf_face_masks_shape(self.h, int(rows), C.byref(F), C.byref(H), C.byref(W)), "pf_face_masks_shape")
        return F.value, H.value, W.value

    def face_masks(self, rows: int, chip_size: int = 0, owners: bool = True, boxes: bool = True):
        """Label maps of the faces of the handle's last pf_landmarks / pf_run_frames / pf_track_frame / pf_track_streams call, in
        that call's row order (include/peppa_hip.h pf_face_masks).  Frame space: (labels uint8 [F,H,W], owners or None, boxes int32
        [rows,4] or None, valid bool [rows]); chip space: (labels uint8 [rows,S,S], None, None, valid)."""
        return _last_call_masks(self._check, self.lib.pf_face_masks, self.lib.pf_face_masks_shape, self.h, "pf_face_masks", rows,
                                chip_size, owners, boxes)

    def face_masks_device(self, rows: int, chip_size: int, d_labels: int, d_owners: int = 0, d_boxes: int = 0, d_valid: int = 0):
        """Same into device memory (sized by face_masks_shape in frame space), enqueued on the handle's stream."""
        self._check(self.lib.pf_face_masks(self.h, int(rows), int(chip_size), _ptr(d_labels), _ptr(d_owners) if d_owners else None,
                                           _ptr(d_boxes) if d_boxes else None, _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE),
                    "pf_face_masks")

    # ---- face redaction (include/peppa_hip.h pf_redact_faces / pf_face_redact) ----------------------------------------------------
    def redact_faces(self, frames, kps: np.ndarray, counts: Optional[np.ndarray] = None, select: Optional[np.ndarray] = None,
                     mode="mosaic", labels: int = PF_REDACT_FACE_ALL, strength: int = 16, pad: int = 0, colour=(0, 0, 0), out=None):
        """Frames with the selected face pixels filled, pixelated or box-blurred, every other pixel untouched.  frames: uint8
        [F,H,W,3] (or [H,W,3]), ``None`` for the resident frame of set_frame(), or ``(device pointer, F, H, W)``; kps: float32 or
        float64 [F,top_k,98,2] (or [top_k,98,2]); counts: [F] live slots per frame (None: all); select: [F,top_k], non-zero = the
        slot is redacted (None: all); mode "fill" / "mosaic" (strength = cell 4, 8, 16) / "blur" (strength = radius 1..32); labels:
        bit L = label L of mask_faces, bit 0 the background, 0x200 the boxes grown by ``pad``.  Returns (out uint8 [F,H,W,3], valid
        bool [F,top_k])."""
        k, f64, F, K = _kps_arg(kps)
        fptr, mem, F, H, W, _keep = self._frames_arg(frames, F)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        sel = None if select is None else np.ascontiguousarray(select, np.int32).reshape(F, K)
        if out is None:
            out = np.zeros((F, H, W, 3), np.uint8)
        valid = np.zeros((F, K), np.int32)
        self._check(self.lib.pf_redact_faces(self.h, fptr, mem, F, H, W, _ptr(k), f64, PF_MEM_HOST, _ptr(c),
                                             _ptr(sel), K, *_redact_args(mode, labels, strength, pad, colour), _ptr(out), _ptr(valid),
                                             PF_MEM_HOST), "pf_redact_faces")
        return out, valid.astype(bool)

    def redact_faces_device(self, frames, kps: np.ndarray, d_out: int, counts: Optional[np.ndarray] = None,
                            select: Optional[np.ndarray] = None, mode="mosaic", labels: int = PF_REDACT_FACE_ALL, strength: int = 16,
                            pad: int = 0, colour=(0, 0, 0)):
        """redact_faces with the frames [F,H,W,3] written to device memory, enqueued on the handle's stream."""
        k, f64, F, K = _kps_arg(kps)
        fptr, mem, F, H, W, _keep = self._frames_arg(frames, F)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        sel = None if select is None else np.ascontiguousarray(select, np.int32).reshape(F, K)
        self._check(self.lib.pf_redact_faces(self.h, fptr, mem, F, H, W, _ptr(k), f64, PF_MEM_HOST, _ptr(c), _ptr(sel), K,
                                             *_redact_args(mode, labels, strength, pad, colour), _ptr(int(d_out)), None, PF_MEM_DEVICE),
                    "pf_redact_faces")

    def face_redact(self, rows: int, select: Optional[np.ndarray] = None, mode="mosaic", labels: int = PF_REDACT_FACE_ALL,
                    strength: int = 16, pad: int = 0, colour=(0, 0, 0)):
        """The frames of the handle's last pf_landmarks / pf_run_frames / pf_track_frame / pf_track_streams call with the faces of its
        first ``rows`` rows redacted (include/peppa_hip.h pf_face_redact): (out uint8 [F,H,W,3], valid bool [rows]).  select: [rows].
        Device frames the caller handed to that call must still be alive."""
        return _last_call_redact(self._check, self.lib.pf_face_redact, self.lib.pf_face_masks_shape, self.h, "pf_face_redact", rows,
                                 select, _redact_args(mode, labels, strength, pad, colour))

    def face_redact_device(self, rows: int, d_out: int, select: Optional[np.ndarray] = None, mode="mosaic",
                           labels: int = PF_REDACT_FACE_ALL, strength: int = 16, pad: int = 0, colour=(0, 0, 0), d_valid: int = 0):
        """Same into device memory (sized by face_masks_shape), enqueued on the handle's stream."""
        sel = None if select is None else np.ascontiguousarray(select, np.int32).reshape(int(rows))
        self._check(self.lib.pf_face_redact(self.h, int(rows), _ptr(sel), *_redact_args(mode, labels, strength, pad, colour), _ptr(d_out),
                                            _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE), "pf_face_redact")

    # ---- per-face region statistics (include/peppa_hip.h pf_measure_faces / pf_face_stats) ----------------------------------------
    def measure_faces(self, frames, kps: np.ndarray, counts: Optional[np.ndarray] = None, dark: int = 16, bright: int = 240, out=None):
        """Exact integer statistics of the frame pixels each face owns, per label of mask_faces.  frames, kps and counts as for
        redact_faces; a pixel is dark iff its luma <= ``dark`` and bright iff >= ``bright``.  Returns (stats uint64 [F,top_k,8,9] --
        row L - 1 is label L; n, sum c0, sum c1, sum c2, sum Y, sum Y^2, sum Lap^2, dark pixels, bright pixels -- and valid bool
        [F,top_k]); rows of invalid slots are left as they were (zero, or what ``out`` held).  ``core.api.quality.face_quality``
        turns the sums into scores."""
        k, f64, F, K = _kps_arg(kps)
        fptr, mem, F, H, W, _keep = self._frames_arg(frames, F)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        if out is None:
            out = np.zeros((F, K, PF_STATS_LABELS, PF_STATS_FIELDS), np.uint64)
        valid = np.zeros((F, K), np.int32)
        self._check(self.lib.pf_measure_faces(self.h, fptr, mem, F, H, W, _ptr(k), f64, PF_MEM_HOST, _ptr(c), K, int(dark), int(bright),
                                              _ptr(out), _ptr(valid), PF_MEM_HOST), "pf_measure_faces")
        return out, valid.astype(bool)

    def face_stats(self, rows: int, dark: int = 16, bright: int = 240):
        """The statistics of the faces of the handle's last pf_landmarks / pf_run_frames / pf_track_frame / pf_track_streams call, in
        that call's row order (include/peppa_hip.h pf_face_stats): (stats uint64 [rows,8,9], valid bool [rows]).  Device frames the
        caller handed to that call must still be alive."""
        return _last_call_stats(self._check, self.lib.pf_face_stats, self.h, "pf_face_stats", rows, dark, bright)

    def face_stats_device(self, rows: int, d_stats: int, d_valid: int = 0, dark: int = 16, bright: int = 240):
        """Same into device memory (8-byte aligned), enqueued on the handle's stream."""
        self._check(self.lib.pf_face_stats(self.h, int(rows), int(dark), int(bright), _ptr(d_stats), _ptr(d_valid) if d_valid else None,
                                           PF_MEM_DEVICE), "pf_face_stats")

    # ---- face overlay (include/peppa_hip.h pf_draw_faces / pf_face_draw) ------------------------------------------------------------
    def draw_faces(self, frames, kps: np.ndarray, counts: Optional[np.ndarray] = None, scores: Optional[np.ndarray] = None, out=None,
                   **style):
        """Frames with the landmarks, contours and boxes of their faces drawn on, every other pixel untouched.  frames, kps and counts
        as for redact_faces; scores: float32 [F,top_k,98] (None: every point takes colour_hi); style: what=("points",) out of
        "points" / "contours" / "box", point_radius=2, line_width=1, alpha=256, score_thres=0.8, colour_hi, colour_lo, colour_contour,
        colour_box.  Returns (out uint8 [F,H,W,3], valid bool [F,top_k])."""
        st = _draw_style(**style)
        k, f64, F, K = _kps_arg(kps)
        fptr, mem, F, H, W, _keep = self._frames_arg(frames, F)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        sc = None if scores is None else np.ascontiguousarray(scores, np.float32).reshape(F, K, 98)
        if out is None:
            out = np.zeros((F, H, W, 3), np.uint8)
        valid = np.zeros((F, K), np.int32)
        self._check(self.lib.pf_draw_faces(self.h, fptr, mem, F, H, W, _ptr(k), f64, PF_MEM_HOST, _ptr(c), _ptr(sc), K, C.byref(st),
                                           _ptr(out), _ptr(valid), PF_MEM_HOST), "pf_draw_faces")
        return out, valid.astype(bool)

    def draw_faces_device(self, frames, kps: np.ndarray, d_out: int, counts: Optional[np.ndarray] = None,
                          scores: Optional[np.ndarray] = None, **style):
        """draw_faces with the frames [F,H,W,3] written to device memory, enqueued on the handle's stream."""
        st = _draw_style(**style)
        k, f64, F, K = _kps_arg(kps)
        fptr, mem, F, H, W, _keep = self._frames_arg(frames, F)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        sc = None if scores is None else np.ascontiguousarray(scores, np.float32).reshape(F, K, 98)
        self._check(self.lib.pf_draw_faces(self.h, fptr, mem, F, H, W, _ptr(k), f64, PF_MEM_HOST, _ptr(c), _ptr(sc), K, C.byref(st),
                                           _ptr(int(d_out)), None, PF_MEM_DEVICE), "pf_draw_faces")

    def face_draw(self, rows: int, scores: Optional[np.ndarray] = None, base: int = 0, **style):
        """The frames of the handle's last pf_landmarks / pf_run_frames / pf_track_frame / pf_track_streams call with the faces of its
        first ``rows`` rows drawn on (include/peppa_hip.h pf_face_draw): (out uint8 [F,H,W,3], valid bool [rows]).  scores: [rows,98];
        base: a device pointer to [F,H,W,3] frames to draw on instead (face_redact_device wrote them), 0 for the call's own."""
        return _last_call_draw(self._check, self.lib.pf_face_draw, self.lib.pf_face_masks_shape, self.h, "pf_face_draw", rows, scores,
                               base, _draw_style(**style))

    def face_draw_device(self, rows: int, d_out: int, scores: Optional[np.ndarray] = None, d_base: int = 0, d_valid: int = 0, **style):
        """Same into device memory (sized by face_masks_shape), enqueued on the handle's stream."""
        st = _draw_style(**style)
        sc = None if scores is None else np.ascontiguousarray(scores, np.float32).reshape(int(rows), 98)
        self._check(self.lib.pf_face_draw(self.h, int(rows), _ptr(sc), C.byref(st), _ptr(int(d_base)) if d_base else None, _ptr(int(d_out)),
                                          _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE), "pf_face_draw")

    def landmark_forward_device(self, d_input: int, kind: int, batch: int, d_loc: int = 0, d_score: int = 0):
        """Same on device pointers (bench): nothing crosses PCIe."""
        self._check(self.lib.pf_landmark_forward(self.h, _ptr(d_input), kind, PF_MEM_DEVICE, batch,
                                                 _ptr(d_loc) if d_loc else None, _ptr(d_score) if d_score else None,
                                                 PF_MEM_DEVICE), "pf_landmark_forward")

    def detector_forward(self, x: np.ndarray, rows: int = 15120) -> np.ndarray:
        if x.dtype == np.uint8:
            kind = PF_INPUT_U8_NHWC
        elif x.dtype == np.float32:
            kind = PF_INPUT_F32_NCHW
        else:
            raise TypeError("detector input must be uint8 NHWC or float32 NCHW")
        x = np.ascontiguousarray(x)
        batch = x.shape[0]
        out = np.empty((batch, rows, 16), np.float32)
        self._check(self.lib.pf_detector_forward(self.h, _ptr(x), kind, PF_MEM_HOST, batch, _ptr(out), PF_MEM_HOST),
                    "pf_detector_forward")
        return out

    def read_tensor(self, slot: int, tensor_id: int, batch: int, shape_hwc) -> np.ndarray:
        h, w, c = shape_hwc
        out = np.empty((batch, h, w, c), np.float32)
        self._check(self.lib.pf_read_tensor(self.h, slot, tensor_id, batch,
                                            out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "pf_read_tensor")
        return out

    # ---- video mode: resident frame + frame-difference gate ------------------------------------------
    def set_frame(self, image_bgr: np.ndarray):
        """Upload the frame once and keep it resident; returns the mean absolute difference to the
        previous resident frame exactly as FaceAna.diff_frames computes it (facer.py:111-113), or None
        when there is no previous frame of the same shape."""
        total = C.c_ulonglong(0)
        has_prev = C.c_int(0)
        if isinstance(image_bgr, DeviceFrame):
            img = image_bgr
            self._check(self.lib.pf_set_frame(self.h, C.c_void_p(img.ptr), PF_MEM_DEVICE, img.shape[0], img.shape[1], img.shape[1] * 3,
                                              C.byref(total), C.byref(has_prev)), "pf_set_frame")
        else:
            img = np.ascontiguousarray(image_bgr)
            assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
            self._check(self.lib.pf_set_frame(self.h, _ptr(img), PF_MEM_HOST, img.shape[0], img.shape[1], img.strides[0],
                                              C.byref(total), C.byref(has_prev)), "pf_set_frame")
        self._resident_shape = img.shape
        if not has_prev.value:
            return None
        return total.value / img.shape[0] / img.shape[1] / 3.0

    def forget_frames(self):
        self._check(self.lib.pf_forget_frames(self.h), "pf_forget_frames")
        self._resident_shape = None

    def _frame_args(self, image_bgr):
        """(pointer, mem, H, W, row_stride) for a host frame, or for the resident one when image is None."""
        if image_bgr is None:
            shp = getattr(self, "_resident_shape", None)
            if shp is None:
                raise PeppaHipError("no resident frame: call set_frame() first")
            return None, PF_MEM_RESIDENT, shp[0], shp[1], shp[1] * 3, None
        if isinstance(image_bgr, DeviceFrame):
            return C.c_void_p(image_bgr.ptr), PF_MEM_DEVICE, image_bgr.shape[0], image_bgr.shape[1], image_bgr.shape[1] * 3, image_bgr
        img = np.ascontiguousarray(image_bgr)
        assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
        return _ptr(img), PF_MEM_HOST, img.shape[0], img.shape[1], img.strides[0], img

    # ---- pipeline seams -----------------------------------------------------------------------
    def detect(self, image_bgr, score_thres: float, iou_thres: float, max_n: int = 1024) -> np.ndarray:
        """image_bgr: HxWx3 uint8, or None to use the frame stored by set_frame()."""
        ptr, mem, H, W, stride, _keep = self._frame_args(image_bgr)
        boxes = np.empty((max_n, 16), np.float32)
        n = C.c_int(0)
        self._check(self.lib.pf_detect(self.h, ptr, mem, H, W, stride,
                                       score_thres, iou_thres, boxes.ctypes.data_as(C.POINTER(C.c_float)), max_n,
                                       C.byref(n)), "pf_detect")
        return boxes[:n.value].copy()

    def landmarks(self, image_bgr, boxes: np.ndarray):
        """image_bgr: HxWx3 uint8, or None to use the frame stored by set_frame()."""
        ptr, mem, H, W, stride, _keep = self._frame_args(image_bgr)
        boxes = np.asarray(boxes)
        # float64 rows (tracked frames of FaceAna) keep their precision: the reference's box arithmetic is float64 then
        f64 = boxes.dtype == np.float64
        b = np.ascontiguousarray(np.asarray(boxes, np.float64 if f64 else np.float32)[:, :4])
        n = b.shape[0]
        kps = np.zeros((n, 98, 2), np.float32)
        scores = np.zeros((n, 98), np.float32)
        valid = np.zeros((n,), np.int32)
        if n:
            fn = self.lib.pf_landmarks_f64 if f64 else self.lib.pf_landmarks
            self._check(fn(self.h, ptr, mem, H, W,
                                              stride, b.ctypes.data_as(C.POINTER(C.c_double if f64 else C.c_float)), n,
                                              kps.ctypes.data_as(C.POINTER(C.c_float)),
                                              scores.ctypes.data_as(C.POINTER(C.c_float)),
                                              valid.ctypes.data_as(C.POINTER(C.c_int))), "pf_landmarks")
        return kps, scores, valid.astype(bool)

    def run_frames(self, frames: np.ndarray, score_thres: float, iou_thres: float, min_face: float, top_k: int,
                   planted_rows: Optional[np.ndarray] = None):
        fr = np.ascontiguousarray(frames)
        assert fr.dtype == np.uint8 and fr.ndim == 4 and fr.shape[3] == 3
        F, H, W, _ = fr.shape
        counts = np.zeros((F,), np.int32)
        boxes = np.zeros((F, top_k, 4), np.float32)
        kps = np.zeros((F, top_k, 98, 2), np.float32)
        scores = np.zeros((F, top_k, 98), np.float32)
        if planted_rows is None:
            rc = self.lib.pf_run_frames(self.h, _ptr(fr), PF_MEM_HOST, F, H, W, score_thres, iou_thres, min_face,
                                        top_k, _ptr(counts), _ptr(boxes), _ptr(kps), _ptr(scores), PF_MEM_HOST)
        else:
            pr = np.ascontiguousarray(planted_rows, np.float32)
            rc = self.lib.pf_run_frames_planted(self.h, _ptr(fr), PF_MEM_HOST, F, H, W, _ptr(pr), pr.shape[1],
                                                score_thres, iou_thres, min_face, top_k, _ptr(counts), _ptr(boxes),
                                                _ptr(kps), _ptr(scores), PF_MEM_HOST)
        self._check(rc, "pf_run_frames")
        return counts, boxes, kps, scores

    def run_frames_device(self, d_frames: int, F: int, H: int, W: int, score_thres: float, iou_thres: float,
                          min_face: float, top_k: int, d_planted: int = 0, rows: int = 0, d_counts: int = 0,
                          d_boxes: int = 0, d_kps: int = 0, d_scores: int = 0, out_mem: int = PF_MEM_DEVICE):
        """Device-resident frames; results to device buffers, or (out_mem = PF_MEM_HOST_PINNED) to page-locked host
        buffers from pinned_empty() -- asynchronous either way, complete after sync()."""
        rc = self.lib.pf_run_frames_planted(self.h, _ptr(d_frames), PF_MEM_DEVICE, F, H, W,
                                            _ptr(d_planted) if d_planted else None, rows, score_thres, iou_thres,
                                            min_face, top_k, _ptr(d_counts) if d_counts else None,
                                            _ptr(d_boxes) if d_boxes else None, _ptr(d_kps) if d_kps else None,
                                            _ptr(d_scores) if d_scores else None, out_mem)
        self._check(rc, "pf_run_frames_planted")

    # ---- stage-level seams -----------------------------------------------------------------------
    def letterbox(self, image_bgr: np.ndarray, out_hw=(384, 640)):
        """FaceDetector.preprocess (uint8 stage): -> (RGB uint8 [H,W,3], [scale, left, top])."""
        fptr, fmem, fh, fw, fstride, _keep = self._frame_args(image_bgr)
        out = np.empty((out_hw[0], out_hw[1], 3), np.uint8)
        info = np.zeros(3, np.float32)
        self._check(self.lib.pf_letterbox(self.h, fptr, fmem, fh, fw, fstride,
                                          out_hw[0], out_hw[1], _ptr(out), info.ctypes.data_as(C.POINTER(C.c_float))),
                    "pf_letterbox")
        return out, info

    def resize(self, image: np.ndarray, out_hw) -> np.ndarray:
        """cv2.resize(image, (out_w, out_h)) (INTER_LINEAR, uint8 HxWx3) on the GPU, bit-for-bit OpenCV's fixed point."""
        img = np.ascontiguousarray(image)
        assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
        out = np.empty((int(out_hw[0]), int(out_hw[1]), 3), np.uint8)
        self._check(self.lib.pf_resize(self.h, _ptr(img), PF_MEM_HOST, img.shape[0], img.shape[1], img.strides[0],
                                       int(out_hw[0]), int(out_hw[1]), _ptr(out)), "pf_resize")
        return out

    def jpeg_info(self, data: bytes) -> Tuple[int, int, int, int]:
        """(height, width, components, subsampling 0 | 444 | 422 | 420) of a JPEG stream the decoder accepts."""
        hh, ww, cc, ss = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        if self.lib.pf_jpeg_info(buf, len(data), C.byref(hh), C.byref(ww), C.byref(cc), C.byref(ss)) != 0:
            raise PeppaHipError("pf_jpeg_info: not a JPEG stream this decoder accepts")
        return hh.value, ww.value, cc.value, ss.value

    def decode_jpeg(self, data: bytes, want_host: bool = True):
        """cv2.imread for JPEG bytes (demo.py:76): Huffman decoding on the host, everything after it on the device.  Returns
        (device pointer of the packed BGR frame -- valid until the next decode --, height, width, host copy or None)."""
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        try:
            hh, ww, _, _ = self.jpeg_info(data)
        except PeppaHipError:      # let the decoder itself say why (its message names the unsupported feature)
            self._check(self.lib.pf_decode_jpeg(self.h, buf, len(data), None, None, None, None), "pf_decode_jpeg")
            raise
        out = np.empty((hh, ww, 3), np.uint8) if want_host else None
        d = C.c_void_p(0)
        h2, w2 = C.c_int(0), C.c_int(0)
        self._check(self.lib.pf_decode_jpeg(self.h, buf, len(data), C.byref(h2), C.byref(w2), C.byref(d),
                                            _ptr(out) if want_host else None), "pf_decode_jpeg")
        return d.value, h2.value, w2.value, out

    def decode_jpeg_batch(self, files, threads: int = 16):
        """n JPEG byte strings of one size -> (device pointer of [n][H][W][3] BGR, n, H, W) for run_frames_device: Huffman
        decoding of the files on `threads` host threads, the device stages once over the batch."""
        n = len(files)
        files = [bytes(d) for d in files]            # immutable: the pointers below stay valid for the call, no copies
        ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(d), C.c_void_p) for d in files])
        sizes = (C.c_size_t * n)(*[len(d) for d in files])
        hh, ww, d = C.c_int(0), C.c_int(0), C.c_void_p(0)
        self._check(self.lib.pf_decode_jpeg_batch(self.h, n, ptrs, sizes, int(threads), C.byref(hh), C.byref(ww), C.byref(d)),
                    "pf_decode_jpeg_batch")
        return d.value, n, hh.value, ww.value

    def run_jpeg_files(self, files, score_thres: float, iou_thres: float, min_face: float, top_k: int, threads: int = 16,
                       planted_rows: Optional[np.ndarray] = None):
        """``pf_decode_jpeg_batch`` + ``pf_run_frames`` on the decoded frames, synchronous, numpy results as ``run_frames``.

        The C ABI's batch decode is asynchronous and reports a Huffman stream the device's parallel entropy decoder could not
        synchronise (a valid file with a long stretch that never re-aligns) at the NEXT synchronising call, when the frames have
        already been consumed.  This wrapper owns the recovery the ABI leaves to its caller: the batch is decoded again with the
        host's Huffman loop (``PF_OPT_JPEG_ENTROPY`` = 1 for that one call) and the frames are run again -- no file that the
        host path decodes fails here."""
        files = [bytes(d) for d in files]
        F = len(files)
        counts = np.zeros((F,), np.int32)
        boxes = np.zeros((F, top_k, 4), np.float32)
        kps = np.zeros((F, top_k, 98, 2), np.float32)
        scores = np.zeros((F, top_k, 98), np.float32)

        pr = None if planted_rows is None else np.ascontiguousarray(planted_rows, np.float32)     # benchmark / test instrument, as run_frames

        def once():
            d, n, hh, ww = self.decode_jpeg_batch(files, threads)
            if pr is None:
                rc = self.lib.pf_run_frames(self.h, _ptr(d), PF_MEM_DEVICE, n, hh, ww, score_thres, iou_thres, min_face, top_k,
                                            _ptr(counts), _ptr(boxes), _ptr(kps), _ptr(scores), PF_MEM_HOST)
            else:
                rc = self.lib.pf_run_frames_planted(self.h, _ptr(d), PF_MEM_DEVICE, n, hh, ww, _ptr(pr), pr.shape[1], score_thres,
                                                    iou_thres, min_face, top_k, _ptr(counts), _ptr(boxes), _ptr(kps), _ptr(scores),
                                                    PF_MEM_HOST)
            self._check(rc, "pf_run_frames")
            self.sync()

        try:
            once()
        except PeppaHipError as e:
            if "did not synchronise" not in str(e):
                raise
            before = self.__dict__.get("_options", {}).get(PF_OPT_JPEG_ENTROPY, 0)
            self.set_option(PF_OPT_JPEG_ENTROPY, 1)
            try:
                once()
            finally:
                self.set_option(PF_OPT_JPEG_ENTROPY, before)
        return counts, boxes, kps, scores

    # ---- baseline JPEG encoder (include/peppa_hip.h pf_encode_jpeg) ---------------------------------------------------------------
    def encode_jpeg_bound(self, height: int, width: int, subsampling: int = 420) -> int:
        """A capacity no file of that shape exceeds (0: a shape encode_jpeg refuses)."""
        return int(self.lib.pf_encode_jpeg_bound(int(height), int(width), int(subsampling)))

    def encode_jpeg(self, images, quality: int = 90, subsampling: int = 420, capacity: Optional[int] = None) -> List[bytes]:
        """Baseline JFIF files of packed BGR images, written on the device, byte for byte what libjpeg(-turbo) writes for the same
        quality and sampling with one restart interval per MCU row.  images: uint8 [H,W,3] or [n,H,W,3] (the last axis contiguous;
        rows may be strided), a ``DeviceFrame``, or ``(device pointer, n, H, W)`` of packed images.  capacity: bytes per file slot, default 3 H W + 4096; where a file does not
        fit, the call is repeated once with ``encode_jpeg_bound``.  Returns one ``bytes`` per image."""
        if isinstance(images, DeviceFrame):
            H, W = images.shape[:2]
            ptr, mem, n, stride, keep = C.c_void_p(images.ptr), PF_MEM_DEVICE, 1, 3 * W, None
        elif isinstance(images, tuple):
            d, n, H, W = (int(v) for v in images)
            ptr, mem, stride, keep = C.c_void_p(d), PF_MEM_DEVICE, 3 * W, None
        else:
            a = np.asarray(images)
            if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
                raise ValueError("images must be uint8 [H,W,3] or [n,H,W,3]")
            if a.ndim == 3:
                a = a[None]
            n, H, W = a.shape[:3]
            if n and not (a.strides[3] == 1 and a.strides[2] == 3 and a.strides[1] >= 3 * W and a.strides[0] == H * a.strides[1]):
                a = np.ascontiguousarray(a)
            ptr, mem, stride, keep = _ptr(a), PF_MEM_HOST, (a.strides[1] if n else 3 * W), a
        cap = int(capacity) if capacity is not None else 3 * H * W + 4096
        for attempt in range(2):
            out = np.empty((max(n, 1), cap), np.uint8)
            sizes = np.zeros((max(n, 1),), np.int32)
            self._check(self.lib.pf_encode_jpeg(self.h, ptr, mem, n, H, W, int(stride), int(quality), int(subsampling), _ptr(out), cap,
                                                _ptr(sizes), PF_MEM_HOST), "pf_encode_jpeg")
            if (sizes > 0).all():
                return [out[i, :sizes[i]].tobytes() for i in range(n)]
            if attempt == 0:
                cap = self.encode_jpeg_bound(H, W, subsampling)
        raise PeppaHipError("pf_encode_jpeg: a file exceeded pf_encode_jpeg_bound (sizes %s)" % (sizes.tolist(),))

    def encode_jpeg_device(self, d_images: int, n: int, H: int, W: int, d_out: int, capacity: int, d_sizes: int, quality: int = 90,
                           subsampling: int = 420, row_stride: int = 0):
        """Same on device pointers, enqueued on the handle's stream without a read-back: file i at d_out + i * capacity, its length
        (or -(bytes needed) where it does not fit) in the int32 d_sizes[i].  row_stride 0: packed rows."""
        self._check(self.lib.pf_encode_jpeg(self.h, _ptr(int(d_images)), PF_MEM_DEVICE, int(n), int(H), int(W), int(row_stride) or 3 * int(W),
                                            int(quality), int(subsampling), _ptr(int(d_out)), int(capacity), _ptr(int(d_sizes)), PF_MEM_DEVICE),
                    "pf_encode_jpeg")

    def device_buffer(self, name: str, nbytes: int) -> int:
        """A device allocation of at least ``nbytes`` that belongs to the engine, kept under ``name`` and grown on demand
        (pf_device_alloc): where the classes keep device outputs that encode_jpeg reads.  Freed by close()."""
        bufs = self.__dict__.setdefault("_device_buffers", {})
        ptr, have = bufs.get(name, (0, 0))
        if have < nbytes:
            if ptr:
                self._check(self.lib.pf_device_free(self.h, C.c_void_p(ptr)), "pf_device_free")
                bufs.pop(name)
            p = C.c_void_p(0)
            self._check(self.lib.pf_device_alloc(self.h, int(nbytes), C.byref(p)), "pf_device_alloc")
            ptr = p.value
            bufs[name] = (ptr, int(nbytes))
        return ptr

    def imread(self, path_or_bytes, want_host: bool = True) -> "DeviceFrame":
        """cv2.imread(path) for baseline JPEG files, decoded into device memory (see decode_jpeg)."""
        data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
        d, hh, ww, host = self.decode_jpeg(bytes(data), want_host)
        return DeviceFrame(d, hh, ww, host)

    def nms_rows(self, rows: np.ndarray, scale: float, left: float, top: float, score_thres: float, iou_thres: float,
                 max_n: int = 1024) -> np.ndarray:
        """xywh2xyxy + py_nms + scale_coords on decoded rows [R,16]."""
        r = np.ascontiguousarray(rows, np.float32)
        kept = np.empty((max_n, 16), np.float32)
        n = C.c_int(0)
        self._check(self.lib.pf_nms_rows(self.h, r.ctypes.data_as(C.POINTER(C.c_float)), r.shape[0], float(scale),
                                         float(left), float(top), float(score_thres), float(iou_thres),
                                         kept.ctypes.data_as(C.POINTER(C.c_float)), max_n, C.byref(n)), "pf_nms_rows")
        return kept[:n.value].copy()

    def crop_faces(self, image_bgr: np.ndarray, boxes: np.ndarray, out_size: int = 256):
        """FaceLandmark.preprocess: -> (crops uint8 [n,S,S,3], params int32 [n,8])."""
        img = np.ascontiguousarray(image_bgr)
        f64 = np.asarray(boxes).dtype == np.float64
        b = np.ascontiguousarray(np.asarray(boxes, np.float64 if f64 else np.float32)[:, :4])
        n = b.shape[0]
        crops = np.zeros((n, out_size, out_size, 3), np.uint8)
        params = np.zeros((n, 8), np.int32)
        fn = self.lib.pf_crop_faces_f64 if f64 else self.lib.pf_crop_faces
        self._check(fn(self.h, _ptr(img), PF_MEM_HOST, img.shape[0], img.shape[1], img.strides[0],
                                           b.ctypes.data_as(C.POINTER(C.c_double if f64 else C.c_float)), n, out_size, _ptr(crops),
                                           params.ctypes.data_as(C.POINTER(C.c_int))), "pf_crop_faces")
        return crops, params

    # ---- video stream with the tracking state on the device (pf_track_frame) -----------------------------------------
    def track_frame(self, image_bgr: np.ndarray, score_thres: float, nms_iou_thres: float, min_face: float, top_k: int,
                    track_iou_thres: float = 0.5, smooth_box: float = 0.3, diff_thres: float = 5.0,
                    planted_rows: Optional[np.ndarray] = None):
        """FaceAna.run(image) for this engine's stream: returns (track boxes float64 [n,4], smoothed landmarks float64
        [n,98,2], scores float32 [n,98], detector_ran).  planted_rows (test instrument): decoded detector
        rows [R,16] that replace the detector network's own output when the gate runs the detector."""
        fptr, fmem, fh, fw, fstride, img = self._frame_args(image_bgr)
        n = C.c_int(0)
        ran = C.c_int(0)
        boxes = np.zeros((top_k, 4), np.float64)
        kps = np.zeros((top_k, 98, 2), np.float64)
        scores = np.zeros((top_k, 98), np.float32)
        outs = (C.byref(n), boxes.ctypes.data_as(C.POINTER(C.c_double)), kps.ctypes.data_as(C.POINTER(C.c_double)),
                scores.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ran))
        if planted_rows is None:
            rc = self.lib.pf_track_frame(self.h, fptr, fmem, fh, fw, fstride,
                                         float(score_thres), float(nms_iou_thres), float(min_face), int(top_k),
                                         float(track_iou_thres), float(smooth_box), float(diff_thres), 0, *outs)
        else:
            pr = np.ascontiguousarray(planted_rows, np.float32)
            rc = self.lib.pf_track_frame_planted(self.h, fptr, fmem, fh, fw, fstride,
                                                 pr.ctypes.data_as(C.POINTER(C.c_float)), pr.shape[0],
                                                 float(score_thres), float(nms_iou_thres), float(min_face), int(top_k),
                                                 float(track_iou_thres), float(smooth_box), float(diff_thres), *outs)
        self._check(rc, "pf_track_frame")
        self._resident_shape = img.shape
        k = n.value
        return boxes[:k].copy(), kps[:k].copy(), scores[:k].copy(), bool(ran.value)

    def track_reset(self):
        self._check(self.lib.pf_track_reset(self.h), "pf_track_reset")
        self._resident_shape = None

    # ---- N video streams on this engine (pf_track_streams) ----------------------------------------------------------------
    def track_streams_config(self, max_streams: int, top_k: int):
        """(Re)allocate the pool of stream slots 0 .. max_streams-1 (every stream forgotten)."""
        self._check(self.lib.pf_track_streams_config(self.h, int(max_streams), int(top_k)), "pf_track_streams_config")
        self._streams_top_k = int(top_k)

    def track_streams(self, stream_ids, frames, score_thres: float, nms_iou_thres: float, min_face: float,
                      track_iou_thres: float = 0.5, smooth_box: float = 0.3, diff_thres: float = 5.0,
                      planted_rows: Optional[np.ndarray] = None, shape=None):
        """FaceAna.run() of each listed stream on its frame.  frames: numpy uint8 [n,H,W,3], or a device pointer (int) with
        shape=(n, H, W).  planted_rows (test instrument): decoded detector rows [n,R,16], used for the frames whose gate runs
        the detector.  Returns one (boxes float64 [c,4], kps float64 [c,98,2], scores float32 [c,98], detector_ran) per frame."""
        ids = np.ascontiguousarray(stream_ids, np.int32).reshape(-1)
        if isinstance(frames, int):
            if shape is None:
                raise ValueError("a device pointer needs shape=(n, H, W)")
            n, H, W = (int(x) for x in shape)
            fptr, fmem, keep = C.c_void_p(frames), PF_MEM_DEVICE, None
        else:
            keep = np.ascontiguousarray(frames)
            if keep.dtype != np.uint8 or keep.ndim != 4 or keep.shape[3] != 3:
                raise ValueError("frames must be uint8 [n,H,W,3]")
            n, H, W = keep.shape[:3]
            fptr, fmem = _ptr(keep), PF_MEM_HOST
        if ids.shape[0] != n:
            raise ValueError("one stream id per frame")
        K = max(1, getattr(self, "_streams_top_k", 1))    # before config the engine rejects the call itself
        counts = np.zeros((n,), np.int32)
        ran = np.zeros((n,), np.int32)
        boxes = np.zeros((n, K, 4), np.float64)
        kps = np.zeros((n, K, 98, 2), np.float64)
        scores = np.zeros((n, K, 98), np.float32)
        pr, R = None, 0
        if planted_rows is not None:
            pr = np.ascontiguousarray(planted_rows, np.float32)
            R = pr.shape[1]
        rc = self.lib.pf_track_streams(self.h, n, ids.ctypes.data_as(C.POINTER(C.c_int)), fptr, fmem, H, W,
                                       pr.ctypes.data_as(C.POINTER(C.c_float)) if pr is not None else None, R,
                                       float(score_thres), float(nms_iou_thres), float(min_face), float(track_iou_thres),
                                       float(smooth_box), float(diff_thres), counts.ctypes.data_as(C.POINTER(C.c_int)),
                                       boxes.ctypes.data_as(C.POINTER(C.c_double)), kps.ctypes.data_as(C.POINTER(C.c_double)),
                                       scores.ctypes.data_as(C.POINTER(C.c_float)), ran.ctypes.data_as(C.POINTER(C.c_int)))
        self._check(rc, "pf_track_streams")
        return [(boxes[i, :c].copy(), kps[i, :c].copy(), scores[i, :c].copy(), bool(ran[i]))
                for i, c in enumerate(counts.tolist())]

    def track_streams_reset(self, stream_id: int = -1):
        self._check(self.lib.pf_track_streams_reset(self.h, int(stream_id)), "pf_track_streams_reset")

    # ---- persistent face ids of the tracking calls (include/peppa_hip.h pf_track_ids_config / pf_track_ids) -------------------------
    def track_ids_config(self, enable: bool, keep_lost: int = 0):
        """Persistent ids for ``track_frame`` and ``track_streams`` on or off (off by default); ``keep_lost``: frames (0 .. 255) an
        id that left is remembered for.  Any change forgets the ids handed out so far (they restart at 1), never the tracks."""
        self._check(self.lib.pf_track_ids_config(self.h, 1 if enable else 0, int(keep_lost)), "pf_track_ids_config")

    def track_ids(self, rows: int):
        """(ids int32 [rows], ages int32 [rows]) of the rows of the last tracking call, counted as ``face_chips`` counts them: [n]
        after ``track_frame``, [n * top_k] after ``track_streams`` (0 beyond a frame's count)."""
        ids = np.zeros((int(rows),), np.int32)
        ages = np.zeros((int(rows),), np.int32)
        self._check(self.lib.pf_track_ids(self.h, int(rows), _ptr(ids), _ptr(ages), PF_MEM_HOST), "pf_track_ids")
        return ids, ages

    def track_ids_device(self, rows: int, d_ids: int = 0, d_ages: int = 0):
        """Same into device memory (int32 [rows] each, 0 = not wanted), enqueued on the handle's stream."""
        self._check(self.lib.pf_track_ids(self.h, int(rows), _ptr(int(d_ids)) if d_ids else None, _ptr(int(d_ages)) if d_ages else None,
                                          PF_MEM_DEVICE), "pf_track_ids")

    def set_option(self, option: int, value: int):
        """PF_OPT_HIP_GRAPH (1): replay device-resident run_frames calls from a captured hipGraph."""
        self._check(self.lib.pf_set_option(self.h, int(option), int(value)), "pf_set_option")
        self.__dict__.setdefault("_options", {})[int(option)] = int(value)

    # ---- profiling ----------------------------------------------------------------------------
    def profile_enable(self, on: bool = True):
        self._check(self.lib.pf_profile_enable(self.h, 1 if on else 0), "pf_profile_enable")

    def profile_fetch(self):
        cap = 256
        names = C.create_string_buffer(16384)
        ms = (C.c_float * cap)()
        cnt = (C.c_int * cap)()
        n = C.c_int(0)
        self._check(self.lib.pf_profile_fetch(self.h, names, 16384, ms, cnt, cap, C.byref(n)), "pf_profile_fetch")
        tags = [t for t in names.value.decode().split("\n") if t]
        return {tags[k]: (float(ms[k]), int(cnt[k])) for k in range(n.value)}

    def launch_log(self):
        """Kernels launched since ``profile_enable(True)``, in order, as the launch sites spell them (template arguments included)."""
        n, need = C.c_int(0), C.c_size_t(0)
        self._check(self.lib.pf_launch_log(self.h, None, 0, C.byref(n), C.byref(need)), "pf_launch_log")
        names = C.create_string_buffer(need.value)
        self._check(self.lib.pf_launch_log(self.h, names, need.value, C.byref(n), C.byref(need)), "pf_launch_log")
        return [t for t in names.value.decode().split("\n") if t]


class BatchEngine:
    """``lanes`` engines (one HIP stream + one arena each) on ONE GPU behind one call: ``pf_batch_*`` of the C ABI.
    Every ``run_frames*`` call hands its frames to the lanes as contiguous slices; launches are asynchronous, so the lanes'
    kernels overlap on the device.  The reference has no batch path (face_landmark.py:119); this is the configuration
    ``bench.py`` measures."""

    def __init__(self, device: int = 0, lanes: int = 3, library: Optional[str] = None):
        self.lib = load_library(library)
        self.b = C.c_void_p()
        if self.lib.pf_batch_create(int(device), int(lanes), C.byref(self.b)) != 0:
            msg = self.lib.pf_batch_last_error(None)
            raise PeppaHipError("pf_batch_create failed: " + (msg.decode() if msg else "unknown"))
        self.device, self.lanes = device, int(lanes)
        self._lane_engines = {}
        self._host = Engine.__new__(Engine)          # page-locked allocations only (pf_host_alloc needs no handle)
        self._host.lib, self._host.h, self._host._borrowed = self.lib, None, True

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.pf_batch_last_error(self.b)
            raise PeppaHipError(f"{what} failed: " + (msg.decode() if msg else "unknown"))

    def lane(self, i: int) -> "Engine":
        """Lane ``i`` as an ``Engine`` (profiling, stage-level calls); the handle stays owned by the batch."""
        if i not in self._lane_engines:
            h = self.lib.pf_batch_lane(self.b, int(i))
            if not h:
                raise PeppaHipError("pf_batch_lane(%d): no such lane" % i)
            e = Engine.__new__(Engine)
            e.lib, e.h, e.device, e._programs, e._borrowed = self.lib, C.c_void_p(h), self.device, {}, True
            self._lane_engines[i] = e
        return self._lane_engines[i]

    def front(self) -> "Engine":
        """The engine that runs letterbox + detector + NMS of a whole call (``PF_OPT_BATCH_FRONT``), for profiling."""
        if "front" not in self._lane_engines:
            e = Engine.__new__(Engine)
            e.lib, e.h, e.device, e._programs, e._borrowed = self.lib, C.c_void_p(self.lib.pf_batch_front(self.b)), self.device, {}, True
            self._lane_engines["front"] = e
        return self._lane_engines["front"]

    def pinned_empty(self, shape, dtype=np.uint8) -> np.ndarray:
        return self._host.pinned_empty(shape, dtype)

    def load_program(self, slot: int, blob: bytes, max_batch_per_lane: int):
        buf = C.create_string_buffer(blob, len(blob))
        self._check(self.lib.pf_batch_load_program(self.b, slot, C.cast(buf, C.c_void_p), len(blob), int(max_batch_per_lane)),
                    "pf_batch_load_program")

    def set_option(self, option: int, value: int):
        self._check(self.lib.pf_batch_set_option(self.b, int(option), int(value)), "pf_batch_set_option")

    def sync(self):
        self._check(self.lib.pf_batch_sync(self.b), "pf_batch_sync")

    def run_frames_device(self, d_frames: int, F: int, H: int, W: int, score_thres: float, iou_thres: float, min_face: float,
                          top_k: int, d_planted: int = 0, rows: int = 0, d_counts: int = 0, d_boxes: int = 0, d_kps: int = 0,
                          d_scores: int = 0, out_mem: int = PF_MEM_DEVICE):
        """Device-resident frames in; results to device buffers or page-locked host buffers (``out_mem``), no synchronisation."""
        rc = self.lib.pf_batch_run_frames(self.b, _ptr(d_frames), PF_MEM_DEVICE, F, H, W, _ptr(d_planted) if d_planted else None,
                                          rows, score_thres, iou_thres, min_face, top_k, _ptr(d_counts) if d_counts else None,
                                          _ptr(d_boxes) if d_boxes else None, _ptr(d_kps) if d_kps else None,
                                          _ptr(d_scores) if d_scores else None, out_mem)
        self._check(rc, "pf_batch_run_frames")

    def run_frames_host_async(self, frames: np.ndarray, d_planted: int, rows: int, score_thres: float, iou_thres: float,
                              min_face: float, top_k: int, d_counts: int, d_boxes: int, d_kps: int, d_scores: int):
        """Host-resident frames (ideally from pinned_empty) in, device-resident results out, no synchronisation: every lane
        copies its slice on its own stream, so one lane's copy overlaps the others' kernels.  Planted detector rows
        (benchmark instrument) are a device pointer."""
        F, H, W, _ = frames.shape
        assert frames.dtype == np.uint8 and frames.flags["C_CONTIGUOUS"]
        rc = self.lib.pf_batch_run_frames(self.b, _ptr(frames), PF_MEM_HOST | PF_MEM_ROWS_DEVICE, F, H, W,
                                          _ptr(d_planted) if d_planted else None, rows, score_thres, iou_thres, min_face, top_k,
                                          _ptr(d_counts), _ptr(d_boxes), _ptr(d_kps), _ptr(d_scores), PF_MEM_DEVICE)
        self._check(rc, "pf_batch_run_frames")

    def run_frames(self, frames: np.ndarray, score_thres: float, iou_thres: float, min_face: float, top_k: int,
                   planted_rows: Optional[np.ndarray] = None):
        """Host frames ``[F,H,W,3]`` uint8 in, numpy results out (synchronous): counts [F], boxes [F,top_k,4],
        landmarks [F,top_k,98,2], scores [F,top_k,98]; rows of a frame beyond its count are undefined."""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W, _ = frames.shape
        counts = np.zeros((F,), np.int32)
        boxes = np.zeros((F, top_k, 4), np.float32)
        kps = np.zeros((F, top_k, 98, 2), np.float32)
        scores = np.zeros((F, top_k, 98), np.float32)
        rows, pr = 0, None
        if planted_rows is not None:
            pr = np.ascontiguousarray(planted_rows, np.float32)
            rows = pr.shape[1]
        rc = self.lib.pf_batch_run_frames(self.b, _ptr(frames), PF_MEM_HOST, F, H, W, _ptr(pr), rows, score_thres, iou_thres,
                                          min_face, top_k, _ptr(counts), _ptr(boxes), _ptr(kps), _ptr(scores), PF_MEM_HOST)
        self._check(rc, "pf_batch_run_frames")
        return counts, boxes, kps, scores

    def face_attrs(self, rows: int, raw: bool = False) -> np.ndarray:
        """Face attributes [rows, 7] of the last run_frames* call, laid out like its kps ([F * top_k]; include/peppa_hip.h
        pf_batch_face_attrs)."""
        return _last_call_attrs(self._check, self.lib.pf_batch_face_attrs, self.b, "pf_batch_face_attrs", rows, raw)

    def face_attrs_device(self, rows: int, d_out: int, raw: bool = False):
        """Same into device memory, enqueued on the lanes' streams."""
        self._check(self.lib.pf_batch_face_attrs(self.b, int(rows), _ptr(d_out), 1 if raw else 0, PF_MEM_DEVICE), "pf_batch_face_attrs")

    def face_chips(self, rows: int, chip_size: int = 112):
        """Chips of the last run_frames* call, laid out like its kps ([F * top_k]; include/peppa_hip.h pf_batch_face_chips):
        (chips uint8 [rows,S,S,3], mats float64 [rows,2,3], valid bool [rows])."""
        return _last_call_chips(self._check, self.lib.pf_batch_face_chips, self.b, "pf_batch_face_chips", rows, chip_size)

    def face_chips_device(self, rows: int, chip_size: int, d_chips: int, d_mats: int = 0, d_valid: int = 0):
        """Same into device memory, enqueued on the lanes' streams."""
        self._check(self.lib.pf_batch_face_chips(self.b, int(rows), int(chip_size), _ptr(d_chips), _ptr(d_mats) if d_mats else None,
                                                 _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE), "pf_batch_face_chips")

    def face_masks(self, rows: int, chip_size: int = 0, owners: bool = True, boxes: bool = True):
        """Label maps of the last run_frames* call (include/peppa_hip.h pf_batch_face_masks), as ``Engine.face_masks`` returns them:
        frame-space maps [F,H,W], boxes and valid laid out like its kps ([F * top_k])."""
        return _last_call_masks(self._check, self.lib.pf_batch_face_masks, self.lib.pf_batch_face_masks_shape, self.b,
                                "pf_batch_face_masks", rows, chip_size, owners, boxes)

    def face_masks_device(self, rows: int, chip_size: int, d_labels: int, d_owners: int = 0, d_boxes: int = 0, d_valid: int = 0):
        """Same into device memory, enqueued on the lanes' streams."""
        self._check(self.lib.pf_batch_face_masks(self.b, int(rows), int(chip_size), _ptr(d_labels), _ptr(d_owners) if d_owners else None,
                                                 _ptr(d_boxes) if d_boxes else None, _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE),
                    "pf_batch_face_masks")

    def redact_faces(self, frames, kps, **kw):
        """Stage-level redaction on lane 0's engine (``Engine.redact_faces``)."""
        return self.lane(0).redact_faces(frames, kps, **kw)

    def face_redact(self, rows: int, select: Optional[np.ndarray] = None, mode="mosaic", labels: int = PF_REDACT_FACE_ALL,
                    strength: int = 16, pad: int = 0, colour=(0, 0, 0)):
        """The frames of the last run_frames* call, redacted (include/peppa_hip.h pf_batch_face_redact), as ``Engine.face_redact``
        returns them: (out uint8 [F,H,W,3], valid bool [rows]); each lane writes the frames it ran."""
        return _last_call_redact(self._check, self.lib.pf_batch_face_redact, self.lib.pf_batch_face_masks_shape, self.b,
                                 "pf_batch_face_redact", rows, select, _redact_args(mode, labels, strength, pad, colour))

    def face_redact_device(self, rows: int, d_out: int, select: Optional[np.ndarray] = None, mode="mosaic",
                           labels: int = PF_REDACT_FACE_ALL, strength: int = 16, pad: int = 0, colour=(0, 0, 0), d_valid: int = 0):
        """Same into device memory, enqueued on the lanes' streams."""
        sel = None if select is None else np.ascontiguousarray(select, np.int32).reshape(int(rows))
        self._check(self.lib.pf_batch_face_redact(self.b, int(rows), _ptr(sel), *_redact_args(mode, labels, strength, pad, colour),
                                                  _ptr(d_out), _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE), "pf_batch_face_redact")

    def measure_faces(self, frames, kps, **kw):
        """Stage-level statistics on lane 0's engine (``Engine.measure_faces``)."""
        return self.lane(0).measure_faces(frames, kps, **kw)

    def face_stats(self, rows: int, dark: int = 16, bright: int = 240):
        """The statistics of the faces of the last run_frames* call (include/peppa_hip.h pf_batch_face_stats), as
        ``Engine.face_stats`` returns them; each lane measures the frames it ran."""
        return _last_call_stats(self._check, self.lib.pf_batch_face_stats, self.b, "pf_batch_face_stats", rows, dark, bright)

    def face_stats_device(self, rows: int, d_stats: int, d_valid: int = 0, dark: int = 16, bright: int = 240):
        """Same into device memory, enqueued on the lanes' streams."""
        self._check(self.lib.pf_batch_face_stats(self.b, int(rows), int(dark), int(bright), _ptr(d_stats),
                                                 _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE), "pf_batch_face_stats")

    def draw_faces(self, frames, kps, **kw):
        """Stage-level overlay on lane 0's engine (``Engine.draw_faces``)."""
        return self.lane(0).draw_faces(frames, kps, **kw)

    def face_draw(self, rows: int, scores: Optional[np.ndarray] = None, base: int = 0, **style):
        """The frames of the last run_frames* call with their faces drawn on (include/peppa_hip.h pf_batch_face_draw), as
        ``Engine.face_draw`` returns them; each lane draws the frames it ran."""
        return _last_call_draw(self._check, self.lib.pf_batch_face_draw, self.lib.pf_batch_face_masks_shape, self.b,
                               "pf_batch_face_draw", rows, scores, base, _draw_style(**style))

    def face_draw_device(self, rows: int, d_out: int, scores: Optional[np.ndarray] = None, d_base: int = 0, d_valid: int = 0, **style):
        """Same into device memory, enqueued on the lanes' streams."""
        st = _draw_style(**style)
        sc = None if scores is None else np.ascontiguousarray(scores, np.float32).reshape(int(rows), 98)
        self._check(self.lib.pf_batch_face_draw(self.b, int(rows), _ptr(sc), C.byref(st), _ptr(int(d_base)) if d_base else None,
                                                _ptr(int(d_out)), _ptr(d_valid) if d_valid else None, PF_MEM_DEVICE), "pf_batch_face_draw")

    def encode_jpeg(self, images, **kw):
        """``Engine.encode_jpeg`` on lane 0's engine."""
        return self.lane(0).encode_jpeg(images, **kw)

    def device_buffer(self, name: str, nbytes: int) -> int:
        return self.lane(0).device_buffer(name, nbytes)

    def encode_jpeg_bound(self, height: int, width: int, subsampling: int = 420) -> int:
        return self.lane(0).encode_jpeg_bound(height, width, subsampling)

    def encode_jpeg_device(self, d_images: int, n: int, H: int, W: int, d_out: int, capacity: int, d_sizes: int, **kw):
        """``Engine.encode_jpeg_device`` on lane 0's stream; images the other lanes wrote (face_redact_device, face_chips_device) need
        a ``sync()`` in front."""
        return self.lane(0).encode_jpeg_device(d_images, n, H, W, d_out, capacity, d_sizes, **kw)

    def close(self):
        self._host.close()
        for e in self._lane_engines.values():
            e.close()
        self._lane_engines = {}
        if getattr(self, "b", None) is not None and self.b:
            self.lib.pf_batch_destroy(self.b)
            self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

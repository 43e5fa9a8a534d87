"""FaceAna: the public API of the reference (Skps/core/api/facer.py:25-208) on the MI355X engine.

``FaceAna().run(image_bgr) -> [{'box': (4,), 'kps': (98,2), 'scores': (98,)}, ...]`` and
``reset()`` keep the reference's semantics, including the frame-difference gate that skips the
detector on static video (facer.py:98-118), IoU matching + EMA of boxes against the previous frame
(:144-189), top-k by area (:120-142) and One-Euro landmark smoothing.  The two network stages run
on the GPU through ``pf_detect`` / ``pf_landmarks``; the per-frame bookkeeping stays host-side
Python exactly where the reference has it."""
from __future__ import annotations

import logging
import os
import pathlib
from typing import Dict, Optional

import numpy as np
import yaml

from ... import _native
from ...logger.logger import logger
from ..smoother.ident import IdentityTracker, ids_options, spare_select
from ..smoother.lk import EmaFilter, GroupTrack
from .face_detector import FaceDetector
from .face_landmark import FaceLandmark
from .hip_model_base import run_guarded
from .quality import attach_stats, best_shots_options, stats_options


def get_cfg(path: Optional[str] = None):
    root = pathlib.Path(__file__).resolve().parents[2]
    path = path or os.path.join(root, "config", "Skps.yml")
    with open(path, encoding="UTF-8") as f:
        return yaml.safe_load(f)


def _load_weights(root, rel_path: str, what: str) -> Dict[str, np.ndarray]:
    """``model_path`` of Skps.yml -> weight dictionary.  Accepts the reference's own files --
    ``pretrained/yolov5n-0.5.onnx`` / ``pretrained/kps_student.onnx`` (Skps/config/Skps.yml:4,12; read without
    onnx / onnxruntime, weights.weights_from_onnx) -- as well as ``.npz`` archives and torch checkpoints."""
    from ...weights import load_weights
    path = rel_path if os.path.isabs(rel_path) else os.path.join(root, rel_path)
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{what} weights not found at {path}.  Put the reference's model file there (the .onnx the reference "
            "loads at onnx_model_base.py:14 works as is; so do an .npz of state_dict arrays or a .pth checkpoint) or "
            "pass FaceAna(weights={'detector': {...}, 'keypoints': {...}}).")
    return load_weights(path, what)


def _host_imread(data: bytes):
    """Host decode of an image file the device decoder refuses: BGR uint8 [H,W,3] like cv2.imread(path) (IMREAD_COLOR: alpha
    dropped, greyscale / palette expanded), or None when no host decoder can read it (cv2.imread's answer too).  Uses Pillow
    when it is installed; nothing else in the package depends on it."""
    try:
        import io
        from PIL import Image
    except ImportError:
        return None
    try:
        from PIL import ImageOps
        with Image.open(io.BytesIO(data)) as im:
            im = ImageOps.exif_transpose(im)         # cv2.imread applies the EXIF orientation (IMREAD_COLOR without IGNORE_ORIENTATION)
            if im.mode in ("I;16", "I;16B", "I;16L", "I"):      # 16-bit greyscale: cv2.imread(IMREAD_COLOR) keeps the HIGH byte
                im = im.point(lambda v: v / 256.0).convert("L")
            rgb = np.asarray(im.convert("RGB"))
    except Exception:  # noqa: BLE001  (truncated / unknown format)
        return None
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _box_iou(a, b) -> float:
    total = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])
    iw = max(0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    return inter / (total - inter)


def attach_masks(dicts, labels, owners, boxes, valid):
    """Result dict i of a frame (slot i of its maps) gets "mask_box" and "mask": the labels cropped to the slot's box, pixels another
    face owns set to 0.  An invalid slot or an empty box gets neither."""
    for i, d in enumerate(dicts):
        x0, y0, x1, y1 = (int(v) for v in boxes[i])
        if valid[i] and x1 > x0 and y1 > y0:
            d["mask_box"] = np.array([x0, y0, x1, y1], np.int32)
            d["mask"] = np.where(owners[y0:y1, x0:x1] == i + 1, labels[y0:y1, x0:x1], 0).astype(np.uint8)


def redact_options(value, eng_cfg):
    """The ``redact`` option of the classes: ``None`` -> ``Engine.redact`` of Skps.yml; a false value is off (``None`` is returned);
    a dict gives any of "mode" ("fill" / "mosaic" / "blur"), "labels", "strength", "pad", "colour" over the defaults of
    ``Engine.redact_faces``; ``True`` is those defaults."""
    if value is None:
        value = eng_cfg.get("redact", None)
    if not value:
        return None
    opts = {"mode": "mosaic", "labels": _native.PF_REDACT_FACE_ALL, "strength": 16, "pad": 0, "colour": (0, 0, 0)}
    if isinstance(value, dict):
        unknown = set(value) - set(opts)
        if unknown:
            raise ValueError("redact: unknown keys %s" % sorted(unknown))
        opts.update(value)
    return opts


def jpeg_options(value, eng_cfg):
    """The ``jpeg`` option of the classes: ``None`` -> ``Engine.jpeg`` of the configuration if present, else off (``None`` is
    returned); a quality (int) or a dict with any of "quality" (90), "subsampling" (420) and "raw" (True: the raw host copies are kept
    next to the files)."""
    if value is None:
        value = eng_cfg.get("jpeg", None)
    if value is None or value is False:
        return None
    opts = {"quality": 90, "subsampling": 420, "raw": True}
    if isinstance(value, dict):
        unknown = set(value) - set(opts)
        if unknown:
            raise ValueError("jpeg: unknown keys %s" % sorted(unknown))
        opts.update(value)
    elif value is not True:
        opts["quality"] = int(value)
    return opts


def jpeg_redacted(engine, jpeg, redact, rows, shape, source=None, sync=None):
    """The redacted frames [F,H,W,3] (``shape``) as JPEG files, redacted and encoded on the device: pf_face_redact of the last call's
    first ``rows`` rows, or -- ``source = (frames argument, landmarks)`` -- pf_redact_faces, into device memory the engine keeps,
    then pf_encode_jpeg on it; only the files come to the host.  ``sync``: called between the two where they run on different
    streams (BatchEngine)."""
    F, H, W = (int(v) for v in shape[:3])
    d = engine.device_buffer("jpeg_redacted", F * H * W * 3)
    if source is None:
        engine.face_redact_device(rows, d, **redact)
    else:
        engine.redact_faces_device(source[0], source[1], d, **redact)
    if sync is not None:
        sync()
    return engine.encode_jpeg((d, F, H, W), quality=jpeg["quality"], subsampling=jpeg["subsampling"])


def jpeg_chips(engine, jpeg, rows, S, valid, source=None, sync=None):
    """One JPEG file per valid chip of ``rows`` chips (``None`` for an invalid one), cut and encoded on the device (pf_face_chips, or
    pf_align_faces for ``source = (frames argument, landmarks)``, then pf_encode_jpeg)."""
    rows, S = int(rows), int(S)
    if rows == 0:
        return []
    d = engine.device_buffer("jpeg_chips", rows * S * S * 3)
    if source is None:
        engine.face_chips_device(rows, S, d)
    else:
        engine.align_faces_device(source[0], source[1], d, chip_size=S)
    if sync is not None:
        sync()
    files = engine.encode_jpeg((d, rows, S, S), quality=jpeg["quality"], subsampling=jpeg["subsampling"])
    return [f if v else None for f, v in zip(files, np.asarray(valid).reshape(-1))]


def draw_options(value, eng_cfg, redact):
    """The ``draw`` option of the classes: ``None`` -> ``Engine.draw`` of Skps.yml; a false value is off (``None`` is returned); a
    dict gives any of the keywords of ``Engine.draw_faces`` ("what", "point_radius", "line_width", "alpha", "score_thres",
    "colour_hi", "colour_lo", "colour_contour", "colour_box") over its defaults, plus "base": "frame" (the default) or "redacted"
    (draw over the redaction, which needs ``redact`` -- the options redact_options returned -- on); ``True`` is the defaults."""
    if value is None:
        value = eng_cfg.get("draw", None)
    if not value:
        return None
    opts = {"what": ("points",), "point_radius": 2, "line_width": 1, "alpha": 256, "score_thres": 0.8, "colour_hi": (255, 255, 255),
            "colour_lo": (0, 0, 255), "colour_contour": (0, 255, 0), "colour_box": (255, 255, 0), "base": "frame"}
    if isinstance(value, dict):
        unknown = set(value) - set(opts)
        if unknown:
            raise ValueError("draw: unknown keys %s" % sorted(unknown))
        opts.update(value)
    if opts["base"] not in ("frame", "redacted"):
        raise ValueError("draw: base must be 'frame' or 'redacted' (got %r)" % (opts["base"],))
    if opts["base"] == "redacted" and not redact:
        raise ValueError("draw: base 'redacted' needs the redact option on")
    _native._draw_style(**{k: v for k, v in opts.items() if k != "base"})      # a wrong name in "what" is refused here, not at the first frame
    return opts


def draw_overlay(engine, draw, jpeg, redact, rows, shape, scores, source=None, sync=None):
    """The frames [F,H,W,3] (``shape``) with the faces drawn on, on the device: pf_face_draw of the last call's first ``rows`` rows,
    or -- ``source = (frames argument, landmarks)`` -- pf_draw_faces; ``scores`` [rows,98] or None.  With "base": "redacted" the
    redaction (``redact``) is written to device memory the engine keeps and drawn over.  Returns (the raw frames or None when
    ``jpeg`` has "raw": False, the JPEG files or None without ``jpeg``): the files are encoded from the device output, so only they
    cross PCIe.  ``sync``: called in front of the encoder where it runs on another stream (BatchEngine)."""
    F, H, W = (int(v) for v in shape[:3])
    style = {k: v for k, v in draw.items() if k != "base"}
    d_base = 0
    if draw["base"] == "redacted":
        d_base = engine.device_buffer("draw_base", F * H * W * 3)
        if source is None:
            engine.face_redact_device(rows, d_base, **redact)
        else:
            engine.redact_faces_device(source[0], source[1], d_base, **redact)
    frames = (d_base, F, H, W) if d_base and source is not None else (source[0] if source is not None else None)
    sc = None if scores is None else np.ascontiguousarray(scores, np.float32)
    drawn = files = None
    if not jpeg or jpeg["raw"]:
        if source is None:
            drawn = engine.face_draw(rows, scores=sc, base=d_base, **style)[0]
        else:
            drawn = engine.draw_faces(frames, source[1], scores=sc, **style)[0]
    if jpeg:
        d = engine.device_buffer("jpeg_drawn", F * H * W * 3)
        if source is None:
            engine.face_draw_device(rows, d, scores=sc, d_base=d_base, **style)
        else:
            engine.draw_faces_device(frames, source[1], d, scores=sc, **style)
        if sync is not None:
            sync()
        files = engine.encode_jpeg((d, F, H, W), quality=jpeg["quality"], subsampling=jpeg["subsampling"])
    return drawn, files


def stage_options(eng_cfg, face_attributes=None, face_chips=None, face_masks=None, redact=None):
    """The four options FaceAna, StreamTracker and FrameBatchRunner share, each from its argument or, when that is ``None``, from
    ``Engine`` of Skps.yml: (face_attributes bool, face_chips int (0 = off), face_masks bool, redact dict or None)."""
    return (bool(eng_cfg.get("face_attributes", False)) if face_attributes is None else bool(face_attributes),
            int(eng_cfg.get("face_chips", 0) or 0) if face_chips is None else int(face_chips or 0),
            bool(eng_cfg.get("face_masks", False)) if face_masks is None else bool(face_masks),
            redact_options(redact, eng_cfg))


def host_frame(image) -> np.ndarray:
    """A copy of a frame as a numpy array (a DeviceFrame gives its host copy)."""
    return np.array(image.numpy() if isinstance(image, _native.DeviceFrame) else image)


class FaceAna:
    def __init__(self, verbose: bool = False, cfg: Optional[dict] = None, weights: Optional[dict] = None,
                 device: Optional[int] = None, library: Optional[str] = None, face_attributes: Optional[bool] = None,
                 face_chips: Optional[int] = None, face_masks: Optional[bool] = None, redact: Optional[dict] = None, jpeg=None, draw=None,
                 track_ids=None, spare_ids=None, face_stats=None, best_shots=None):
        """``face_stats`` (default: ``Engine.face_stats`` of the configuration if present, else off): ``True`` or
        ``{"dark": d, "bright": b}`` gives every result dict ``"stats"`` (uint64 [8,9]: per face-region label 1..8 the exact sums n,
        c0, c1, c2, Y, Y^2, Lap^2 and the dark / bright pixel counts over the frame pixels the face owns, measured on the GPU with
        the landmarks the result carries; include/peppa_hip.h pf_measure_faces) and ``"quality"`` (``quality.face_quality`` of it:
        pixels, brightness, contrast, sharpness, dark, bright, skin_bgr), in both tracking modes.  Frame space only; sharpness is per
        frame pixel and falls as a face grows; the face polygon has no forehead.  ``best_shots`` (``True`` or a dict with ``"key"`` /
        ``"min_pixels"``; needs ``track_ids`` and ``face_stats``) keeps the best-scoring result of every id in ``self.best_shots``
        (``quality.BestShots``), with its chip when ``face_chips`` is on.

        ``track_ids`` (default: ``Engine.track_ids`` of Skps.yml, off): ``True`` or ``{"keep_lost": n}`` gives every result dict
        ``"id"`` (int, from 1, stable while the face is tracked; a face absent for up to ``keep_lost`` frames comes back with its id)
        and ``"age"`` (int, frames the id has been seen), in both tracking modes (the rule: include/peppa_hip.h, "Persistent face
        ids").  Geometric identity only (IoU, no appearance): two people who swap places behind an occlusion swap ids.  ``reset()``
        forgets the ids but never reuses one.  ``spare_ids`` (a set of ids, needs ``track_ids`` and is read by ``redact``; may be
        changed between calls through the attribute): a face whose id is in the set is not redacted, every other face -- one seen
        for the first time included -- is.

        ``draw`` (default: ``Engine.draw`` of Skps.yml, off): a dict with any of the keywords of ``Engine.draw_faces`` --
        ``"what"`` (names out of "points", "contours", "box"; default the points), ``"point_radius"``, ``"line_width"``, ``"alpha"``,
        ``"score_thres"`` and the four colours -- and ``"base"`` ("frame", or "redacted" to draw over the redaction, which needs
        ``redact`` on) keeps ``last_drawn`` (uint8 [H,W,3]): the frame with the landmarks, contours and boxes of every face the
        result carries drawn on the GPU, a point white where its score exceeds the threshold and red elsewhere like the reference's
        demo; a frame without a face comes back as a copy.  With ``jpeg`` on it also keeps ``last_drawn_jpeg`` (bytes), encoded on
        the GPU from the device output of the overlay, and ``"raw": False`` drops ``last_drawn``.  The result dicts are unchanged.

        ``jpeg`` (default: ``Engine.jpeg`` of the configuration if present, else off): a quality, or a dict with any of
        ``"quality"`` (90), ``"subsampling"`` (420, 422 or 444) and ``"raw"`` (True).  With ``redact`` on it keeps
        ``last_redacted_jpeg`` (bytes: the frame ``last_redacted`` holds as a baseline JPEG file); with ``face_chips`` on every result
        gets ``"chip_jpeg"`` (bytes, ``None`` for a degenerate fit).  Both are encoded on the GPU from the device outputs of the
        redaction and of the chips (``Engine.encode_jpeg``), byte for byte what libjpeg writes with one restart interval per MCU row.
        ``"raw": False`` drops the raw host copies: ``last_redacted`` stays ``None`` -- the redacted frame then crosses PCIe only as
        its file -- and the results carry no ``"chip"``.

        ``redact`` (default: ``Engine.redact`` of Skps.yml, off): a dict with any of ``"mode"`` ("fill" / "mosaic" / "blur"),
        ``"labels"`` (bit L = face-region label L, bit 0 the background, 0x200 the face boxes grown by ``"pad"``), ``"strength"``
        (mosaic cell 4 / 8 / 16, blur radius 1..32), ``"pad"`` and ``"colour"`` keeps ``last_redacted`` (uint8 [H,W,3]): the frame
        with every face the result carries redacted on the GPU from its landmarks, every other pixel untouched; a frame without a
        face comes back as a copy.  The result dicts are unchanged.

        ``face_masks`` (default: ``Engine.face_masks`` of Skps.yml, false): every result dict also carries ``"mask_box"`` (int32
        x0, y0, x1, y1) and ``"mask"`` (uint8 [y1 - y0, x1 - x0]: the frame's face-region labels -- 1 face, 2 / 3 brows, 4 / 5 eyes,
        6 nose, 7 lips, 8 inner mouth -- cropped to the box, pixels owned by another face set to 0), filled on the GPU from the
        landmarks the result carries; a face whose box is empty or whose landmarks are not finite gets neither key.  The whole maps of
        the last frame stay reachable as ``last_label_map`` / ``last_owner_map`` (uint8 [H,W]; owner = index in the result list + 1).
        Hard edges, no feathering; the face polygon stops at the upper brow line.

        ``face_chips`` (default: ``Engine.face_chips`` of Skps.yml, 0 = off): a chip size S (a multiple of 16 in [32, 256], e.g.
        112) makes every result dict also carry ``"chip"`` (uint8 [S,S,3], BGR: the face warped onto the ArcFace five-point template
        on the GPU, cut with the landmarks the result carries) and ``"chip_matrix"`` (float64 [2,3], frame -> chip); a face whose
        fit is degenerate gets neither key.  No anti-alias pre-filter is applied when the face is larger than the chip.

        ``face_attributes`` (default: ``Engine.face_attributes`` of Skps.yml, false): every result dict also gets ``"pose"``
        (float32 [3], head pose in degrees about x, y, z -- the per-frame network output, not smoothed) and ``"attrs"`` (float32 [4],
        P(eye of points 60-67 closed), P(eye of points 68-75 closed), P(mouth closed), P(mouth wide open)) from the landmark network's
        fc head, in both tracking modes.  Needs weights with ``fc.weight`` / ``fc.bias`` (a .pth checkpoint or an .npz made from one,
        not the ONNX file)."""
        if verbose:
            logger.setLevel(logging.DEBUG)
        cfg = cfg or get_cfg()
        sk = cfg["Skps"]
        eng_cfg = sk.get("Engine", {})
        dev = int(eng_cfg.get("device", 0)) if device is None else int(device)
        dtype = eng_cfg.get("dtype", "f32")
        root = pathlib.Path(__file__).resolve().parents[2]
        weights = weights or {}
        det_w = weights.get("detector") or _load_weights(root, sk["Detect"]["model_path"], "detector")
        kps_arch = str(sk["Keypoints"].get("model", "student"))
        kps_w = weights.get("keypoints") or _load_weights(root, sk["Keypoints"]["model_path"], "teacher" if kps_arch == "teacher" else "keypoints")

        # Engine.device_tracking: keep track_box / previous landmarks / One-Euro state on the GPU (pf_track_frame) instead of
        # walking the boxes through numpy between the two networks on every frame
        self.device_tracking = bool(eng_cfg.get("device_tracking", False))
        self.face_attributes, self.face_chips, self.face_masks, self.redact = stage_options(eng_cfg, face_attributes, face_chips, face_masks, redact)
        self.last_label_map = self.last_owner_map = None
        self.last_redacted = None
        self.jpeg = jpeg_options(jpeg, eng_cfg)
        self.last_redacted_jpeg = None
        self.draw = draw_options(draw, eng_cfg, self.redact)
        self.last_drawn = self.last_drawn_jpeg = None
        self.track_ids = ids_options(track_ids, eng_cfg)
        if spare_ids is not None and not self.track_ids:
            raise ValueError("spare_ids needs track_ids on")
        self.spare_ids = set(spare_ids or ())
        self.face_stats = stats_options(face_stats, eng_cfg)
        self.best_shots = best_shots_options(best_shots, self.track_ids, self.face_stats)
        self._planted_rows = None   # test instrument: callable returning decoded detector rows that replace the detector's own
        self._det_cfg = sk["Detect"]
        self.top_k = sk["Detect"]["topk"]
        self.engine = _native.Engine(dev, library)      # one GPU, one stream, shared by both stages
        if self.track_ids and self.device_tracking:
            self.engine.track_ids_config(True, self.track_ids["keep_lost"])
        max_faces = max(int(eng_cfg.get("max_faces", 8)), int(self.top_k))
        self.face_detector = FaceDetector(sk["Detect"], det_w, engine=self.engine, dtype=dtype)
        self.face_landmark = FaceLandmark(sk["Keypoints"], kps_w, engine=self.engine, dtype=dtype, max_batch=max_faces,
                                          face_attributes=self.face_attributes)
        self.trace = GroupTrack(sk["Trace"])
        logger.info("model init done!")

        self.track_box = None
        self.previous_image = None
        self.previous_box = None
        self.diff_thres = 5
        self.min_face = sk["Detect"]["min_face"]
        self.iou_thres = sk["Trace"]["iou_thres"]
        self.alpha = sk["Trace"]["smooth_box"]
        self.filter = EmaFilter(self.alpha)
        # host tracking mode: the identity rule in numpy, fed by judge_boxs and sort_and_filter
        self._ident = IdentityTracker(self.track_ids["keep_lost"], self.iou_thres) if self.track_ids and not self.device_tracking else None
        self._judge_src = self._sel_rows = None

    def configure_track_ids(self, keep_lost: int):
        """Another ``keep_lost`` for ``track_ids``: the ids handed out so far are forgotten (they restart at 1), the tracks stay."""
        if not self.track_ids:
            raise ValueError("track_ids is off")
        self.track_ids = ids_options({"keep_lost": keep_lost}, {})
        if self.device_tracking:
            self.engine.track_ids_config(True, self.track_ids["keep_lost"])
        else:
            self._ident = IdentityTracker(self.track_ids["keep_lost"], self.iou_thres)

    def _redact_with(self, ids):
        """The redact options with the ``select`` the ids imply (``spare_ids``), or as they are without ``track_ids``."""
        if not self.redact or ids is None:
            return self.redact
        return dict(self.redact, select=spare_select(ids, self.spare_ids))

    # ---- per-frame entry ---------------------------------------------------------------------------
    def run(self, image: np.ndarray):
        # one host->device copy per frame: the frame stays resident for the gate, the detector and the
        # landmark stage; the frame-difference gate (facer.py:98-118) is evaluated on the GPU against the
        # previous resident frame (exact integer sum, same decision as the numpy code in diff_frames()).
        if self.device_tracking:
            def fn(*args):       # the attribute rows / chips of the tracked faces, compacted like kps (pf_face_attrs / pf_face_chips after pf_track_frame)
                r = self.engine.track_frame(*args)
                n = len(r[0])
                ids = self.engine.track_ids(n) if self.track_ids else None
                red = self._redact_with(ids[0] if ids else None)
                chips = self.engine.face_chips(n, self.face_chips) if self.face_chips and n else None
                jp = (jpeg_redacted(self.engine, self.jpeg, red, n, (1,) + tuple(image.shape[:2])) if self.jpeg and self.redact and n else None,
                      jpeg_chips(self.engine, self.jpeg, n, self.face_chips, chips[2]) if self.jpeg and chips is not None else None)
                over = (draw_overlay(self.engine, self.draw, self.jpeg, red, n, (1,) + tuple(image.shape[:2]), r[2])
                        if self.draw and n else None)
                return r + (self.engine.face_attrs(n) if self.face_attributes else None, chips,
                            self.engine.face_masks(n) if self.face_masks and n else None,
                            self.engine.face_redact(n, **red)[0] if self.redact and n and self._raw else None, jp, over, ids,
                            self.engine.face_stats(n, **self.face_stats) if self.face_stats and n else None)
            out = run_guarded(
                [self.face_detector.model, self.face_landmark.model], fn, image, float(self._det_cfg["score_thrs"]), float(self._det_cfg["iou_thrs"]),
                float(self.min_face), int(self.top_k), float(self.iou_thres), float(self.alpha), float(self.diff_thres),
                self._planted_rows() if self._planted_rows is not None else None)
            boxes, kps, scores = out[:3]
            self.previous_image = image
            self.track_box = boxes
            self._keep_redacted(out[7], image, out[8][0])
            self._keep_drawn(out[9], image)
            return self._with_stats(self.with_ids(self.to_dict(boxes, kps, scores, out[4], out[5], self._keep_masks(out[6], image), out[8][1],
                                                               self._raw), out[10]), out[11])
        diff = self.engine.set_frame(image)
        self.previous_image = image
        if diff is None or self.track_box is None or diff > self.diff_thres:
            boxes = self.face_detector(None)
            boxes = self.judge_boxs(self.track_box, boxes)
            self.trace.previous_landmarks_set = None     # detector ran: smoothing history is dropped
        else:
            boxes = self.track_box
            self._judge_src = [(k, 0.0) for k in range(len(boxes))]      # a gated frame: selected row q is row k of track_box
        previous_track, judge_src = self.track_box, self._judge_src      # before the hull judge below replaces both
        boxes = self.sort_and_filter(boxes)
        boxes_return = np.array(boxes)
        attrs = None
        if self.face_attributes:
            landmarks, states, attrs = self.face_landmark(None, boxes)
        else:
            landmarks, states = self.face_landmark(None, boxes)
        landmarks = self.trace.calculate(image, landmarks)
        hulls = [[np.min(l[:, 0]), np.min(l[:, 1]), np.max(l[:, 0]), np.max(l[:, 1])] for l in landmarks]
        self.track_box = self.judge_boxs(boxes_return, np.array(hulls))
        ids = None
        if self._ident is not None:      # output rows = the selected rows the landmark stage accepted, in order
            valid = self.face_landmark.last_valid if len(boxes_return) else np.zeros((0,), bool)
            src = [judge_src[self._sel_rows[q]] for q in range(len(boxes_return)) if valid[q]]
            ids = self._ident.update([j for j, _ in src], [w for _, w in src], np.asarray(self.track_box, np.float64).reshape(-1, 4),
                                     previous_track)
        red = self._redact_with(ids[0] if ids else None)      # select [top_k] is [1, top_k] of the one frame
        chips = None
        if self.face_chips and len(landmarks):      # cut with the smoothed landmarks the result carries, from the resident frame
            c, m, v = self.engine.align_faces(None, np.asarray(landmarks)[None], chip_size=self.face_chips)
            chips = (c[0], m[0], v[0])
        chip_jpeg = None
        if self.jpeg and chips is not None:
            chip_jpeg = jpeg_chips(self.engine, self.jpeg, len(landmarks), self.face_chips, chips[2], source=(None, np.asarray(landmarks)[None]))
        masks = None
        if self.face_masks and len(landmarks):      # filled from the smoothed landmarks the result carries
            masks = self.engine.mask_faces(np.asarray(landmarks)[None], image.shape[0], image.shape[1])
        redacted = red_jpeg = None
        if self.redact and len(landmarks):          # from the resident frame, with the smoothed landmarks the result carries
            if self._raw:
                redacted = self.engine.redact_faces(None, np.asarray(landmarks)[None], **red)[0]
            if self.jpeg:
                red_jpeg = jpeg_redacted(self.engine, self.jpeg, red, len(landmarks), (1,) + tuple(image.shape[:2]),
                                         source=(None, np.asarray(landmarks)[None]))
        self._keep_redacted(redacted, image, red_jpeg)
        over = None
        if self.draw and len(landmarks):            # on the resident frame, with the smoothed landmarks and the scores the result carries
            over = draw_overlay(self.engine, self.draw, self.jpeg, red, len(landmarks), (1,) + tuple(image.shape[:2]),
                                np.asarray(states), source=(None, np.asarray(landmarks)[None]))
        self._keep_drawn(over, image)
        measured = None
        if self.face_stats and len(landmarks):      # on the resident frame, with the smoothed landmarks the result carries
            st, sv = self.engine.measure_faces(None, np.asarray(landmarks)[None], **self.face_stats)
            measured = (st[0], sv[0])
        return self._with_stats(self.with_ids(self.to_dict(self.track_box, landmarks, states, attrs, chips, self._keep_masks(masks, image),
                                                           chip_jpeg, self._raw), ids), measured)

    def _with_stats(self, dicts, measured):
        """(stats [n,8,9], valid [n]) of Engine.face_stats / measure_faces -> ``"stats"`` and ``"quality"`` of the result dicts, and
        the update of ``best_shots``; ``None``: the dicts as they are."""
        if measured is not None:
            attach_stats(dicts, measured[0], measured[1])
            if self.best_shots is not None:
                self.best_shots.update(dicts)
        return dicts

    @property
    def _raw(self) -> bool:
        """Are the raw host copies kept (always without the ``jpeg`` option)?"""
        return not self.jpeg or bool(self.jpeg["raw"])

    def _keep_redacted(self, redacted, image, red_jpeg=None):
        """[1,H,W,3] of Engine.redact_faces / face_redact, or None when the frame has no face -> last_redacted; the files of
        jpeg_redacted (None: no face, the frame itself is encoded) -> last_redacted_jpeg."""
        if self.redact and self._raw:
            self.last_redacted = host_frame(image) if redacted is None else redacted[0]
        if self.redact and self.jpeg:
            self.last_redacted_jpeg = red_jpeg[0] if red_jpeg is not None else self.engine.encode_jpeg(
                image if isinstance(image, _native.DeviceFrame) else np.asarray(image), quality=self.jpeg["quality"],
                subsampling=self.jpeg["subsampling"])[0]

    def _keep_drawn(self, over, image):
        """(frames [1,H,W,3] or None, files or None) of draw_overlay, or None when the frame has no face (the frame itself is kept
        and encoded) -> last_drawn, last_drawn_jpeg."""
        if not self.draw:
            return
        if self._raw:
            self.last_drawn = host_frame(image) if over is None else over[0][0]
        if self.jpeg:
            self.last_drawn_jpeg = over[1][0] if over is not None else self.engine.encode_jpeg(
                image if isinstance(image, _native.DeviceFrame) else np.asarray(image), quality=self.jpeg["quality"],
                subsampling=self.jpeg["subsampling"])[0]

    def _keep_masks(self, masks, image):
        """(labels [1,H,W], owners, boxes, valid) of Engine.mask_faces / face_masks -> the one frame's (labels, owners, boxes [n,4],
        valid [n]), remembered as last_label_map / last_owner_map (all zero when the frame has no face)."""
        if not self.face_masks:
            return None
        if masks is None:
            self.last_label_map = np.zeros(tuple(image.shape[:2]), np.uint8)
            self.last_owner_map = self.last_label_map.copy()
            return None
        self.last_label_map, self.last_owner_map = masks[0][0], masks[1][0]
        return self.last_label_map, self.last_owner_map, masks[2].reshape(-1, 4), masks[3].reshape(-1)

    def imread(self, path_or_bytes, want_host: bool = True):
        """``cv2.imread(path)`` of the reference's demo (demo.py:76) for baseline JPEG files: the Huffman stream is decoded on
        the host, dequantisation / inverse DCT / chroma upsampling / colour conversion run on the GPU (bit-identical with
        cv2.imread's libjpeg) and the frame never exists in host memory unless asked for.  Returns a ``DeviceFrame`` that
        ``run()`` accepts like an array; ``frame.numpy()`` is the BGR array for drawing."""
        data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else None
        if data is None:
            try:
                with open(path_or_bytes, "rb") as f:
                    data = f.read()
            except OSError:
                return None                      # cv2.imread returns None for a path it cannot read
        try:
            return self.engine.imread(bytes(data), want_host)
        except _native.PeppaHipError as e:
            # Everything else cv2.imread opens (demo.py:76) -- progressive / arithmetic-coded / CMYK JPEG, PNG, BMP, ... -- is
            # decoded on the HOST, as the reference itself does for every file, and handed to run() as the numpy array
            # cv2.imread would have returned; only baseline JPEG has a device decoder (csrc/jpeg.inl).
            # NOTE the type: a host-decoded file comes back as the ndarray cv2.imread returns, not as a DeviceFrame (run() takes both)
            frame = _host_imread(bytes(data))
            if frame is None:
                logger.warning("imread: %s", e)
            return frame

    @staticmethod
    def to_dict(bboxes, kps, states, attrs=None, chips=None, masks=None, chip_jpeg=None, raw_chips=True):
        """``chip_jpeg``: one file (or None) per row, of jpeg_chips; ``raw_chips`` False: no ``"chip"`` key.  ``chips``: (chips [n,S,S,3], matrices [n,2,3], valid [n]) of the same rows (Engine.face_chips / align_faces).
        ``masks``: (labels [H,W], owners [H,W], boxes [>= n,4], valid [>= n]) of the rows' frame, row i being slot i
        (Engine.face_masks / mask_faces)."""
        out = [{"box": bboxes[i], "kps": kps[i], "scores": states[i]} for i in range(len(bboxes))]
        if attrs is not None:
            for i, d in enumerate(out):
                d["pose"] = np.asarray(attrs[i, :3], np.float32).copy()
                d["attrs"] = np.asarray(attrs[i, 3:7], np.float32).copy()
        if chips is not None:
            for i, d in enumerate(out):
                if chips[2][i]:
                    if raw_chips:
                        d["chip"] = chips[0][i].copy()
                    d["chip_matrix"] = chips[1][i].copy()
        if chip_jpeg is not None:
            for i, d in enumerate(out):
                d["chip_jpeg"] = chip_jpeg[i]
        if masks is not None:
            attach_masks(out, *masks)
        return out

    @staticmethod
    def with_ids(dicts, ids):
        """Result dict i gets ``"id"`` and ``"age"`` from (ids, ages) of the same rows; ``None``: the dicts as they are."""
        if ids is not None:
            for d, i, a in zip(dicts, ids[0], ids[1]):
                d["id"], d["age"] = int(i), int(a)
        return dicts

    def diff_frames(self, previous_frame, image) -> bool:
        """True -> run the detector (facer.py:98-118): mean absolute difference of the frames > 5."""
        if previous_frame is None:
            return True
        if previous_frame.shape != image.shape:
            return True
        diff = np.abs(previous_frame.astype(np.int16) - image.astype(np.int16)).sum(dtype=np.int64)
        return diff / previous_frame.shape[0] / previous_frame.shape[1] / 3.0 > self.diff_thres

    def sort_and_filter(self, bboxes):
        """Leaves the input row of every returned row in ``_sel_rows`` (persistent ids)."""
        self._sel_rows = []
        if len(bboxes) < 1:
            return []
        area = (bboxes[:, 2] - bboxes[:, 0]) * (bboxes[:, 3] - bboxes[:, 1])
        keep = area > self.min_face
        rows = np.flatnonzero(keep)
        area, bboxes = area[keep], bboxes[keep, :]
        if bboxes.shape[0] > self.top_k:
            # equal areas: the later row first, as the reference's argsort gives under its pinned numpy (an insertion sort at
            # these sizes) and as track_select_kernel does; newer numpy sorts float32 with SIMD networks that keep no order
            order = area.argsort(kind="stable")[-self.top_k:][::-1]
            bboxes, rows = bboxes[order], rows[order]
        self._sel_rows = [int(r) for r in rows]
        return np.array(bboxes)

    def judge_boxs(self, previuous_bboxs, now_bboxs):
        """Match each current box to the first previous box with IoU > thres and EMA-smooth it.  Leaves (previous row or -1, that
        IoU as a double) of every current row in ``_judge_src`` (persistent ids)."""
        self._judge_src = [(-1, 0.0)] * len(now_bboxs)
        if previuous_bboxs is None:
            return now_bboxs
        out = []
        for i in range(now_bboxs.shape[0]):
            for j in range(previuous_bboxs.shape[0]):
                iou = _box_iou(now_bboxs[i], previuous_bboxs[j])
                if iou > self.iou_thres:
                    out.append(self.smooth(now_bboxs[i], previuous_bboxs[j]))
                    self._judge_src[i] = (j, float(iou))
                    break
            else:
                out.append(now_bboxs[i][0:4])
        return np.array(out)

    def smooth(self, now_box, previous_box):
        return self.filter(now_box[:4], previous_box[:4])

    def reset(self):
        self.track_box = None
        self.previous_image = None
        self.previous_box = None
        if self._ident is not None:
            self._ident.reset()
        if self.device_tracking:
            self.engine.track_reset()
        self.engine.forget_frames()

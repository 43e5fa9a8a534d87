"""FrameBatchRunner: ``FaceAna.run(image)`` + ``reset()`` (Skps/core/api/facer.py:52-85, the demo's still-image loop
demo.py:76-86) over a BATCH of frames in one call.

The reference processes one frame per call and one face per session run (face_landmark.py:40-48; "batched" is a TODO at
:119).  Here the frames of a call are split over ``lanes`` engines on one GPU (``pf_batch_*`` of the C ABI: one HIP stream
and one activation arena per lane), each lane running letterbox -> detector -> NMS -> area filter / top-k -> crop ->
landmark regressor -> back-projection for its slice; the lanes' kernels overlap on the device.  Same configuration keys
as ``FaceAna`` (``Skps.yml``), same result format per frame.  No tracking state: every frame is detected afresh, which is
what ``run()`` followed by ``reset()`` computes (tracking over a video stream is ``FaceAna`` with
``Engine.device_tracking``, one stream per instance)."""
from __future__ import annotations

import pathlib
from typing import Dict, List, Optional

import numpy as np

from ... import _native
from ...logger.logger import logger
from ...graph.detector import build_detector_program
from ...graph.student import build_student_program
from ..smoother.lk import EmaFilter
from .facer import (_box_iou, _load_weights, attach_masks, draw_options, draw_overlay, get_cfg, jpeg_chips, jpeg_options, jpeg_redacted,
                    stage_options)
from .hip_model_base import _RANGE_ERR
from .quality import attach_stats, stats_options


class FrameBatchRunner:
    def __init__(self, cfg: Optional[dict] = None, weights: Optional[dict] = None, lanes: int = 3, frames_per_lane: int = 32,
                 device: Optional[int] = None, library: Optional[str] = None, graph: bool = True, top_k: Optional[int] = None,
                 face_attributes: Optional[bool] = None, face_chips: Optional[int] = None,
                 face_masks: Optional[bool] = None, redact: Optional[dict] = None, jpeg=None, draw=None, face_stats=None):
        """``face_stats`` (default: ``Engine.face_stats`` of the configuration if present, else off): the option of ``FaceAna``;
        every result dict gets ``"stats"`` and ``"quality"``, each lane measuring the frames it ran.

        ``draw`` (default: ``Engine.draw`` of Skps.yml, off): the dict of ``FaceAna``; ``last_drawn`` (uint8 [F,H,W,3]) keeps the
        frames of the last ``run`` with the faces the results carry drawn on, each lane drawing the frames it ran, and
        ``last_drawn_jpeg`` (one ``bytes`` per frame) their files with ``jpeg`` on.

        ``jpeg`` (default: ``Engine.jpeg`` of the configuration if present, else off): the option of ``FaceAna``;
        ``last_redacted_jpeg`` (one ``bytes`` per frame of the last ``run``) and ``"chip_jpeg"`` in every result dict, encoded on the
        GPU (lane 0, behind a synchronisation of the lanes); ``"raw": False`` drops ``last_redacted`` and ``"chip"``.

        ``redact`` (default: ``Engine.redact`` of Skps.yml, off): the dict of ``FaceAna``; ``last_redacted`` (uint8 [F,H,W,3])
        keeps the frames of the last ``run`` with every face the results carry redacted, a frame without a face as a copy.

        ``face_masks`` (default: ``Engine.face_masks`` of Skps.yml, false): ``"mask_box"`` and ``"mask"`` in every result dict as in
        ``FaceAna``; the whole maps of the last ``run`` stay reachable as ``last_label_maps`` / ``last_owner_maps`` (uint8 [F,H,W]).

        ``face_chips`` (default: ``Engine.face_chips`` of Skps.yml, 0 = off): a chip size adds ``"chip"`` and ``"chip_matrix"`` to
        every result dict as in ``FaceAna``.

        ``face_attributes`` (default: ``Engine.face_attributes`` of Skps.yml): every result dict also gets ``"pose"`` and
        ``"attrs"`` as in ``FaceAna``."""
        cfg = cfg or get_cfg()
        sk = cfg["Skps"]
        eng_cfg = sk.get("Engine", {})
        self.face_attributes, self.face_chips, self.face_masks, self.redact = stage_options(eng_cfg, face_attributes, face_chips, face_masks, redact)
        self.last_label_maps = self.last_owner_maps = None
        self.last_redacted = None
        self.jpeg = jpeg_options(jpeg, eng_cfg)
        self.last_redacted_jpeg = None
        self.draw = draw_options(draw, eng_cfg, self.redact)
        self.last_drawn = self.last_drawn_jpeg = None
        self.face_stats = stats_options(face_stats, eng_cfg)
        self._measured = None
        self.device = int(eng_cfg.get("device", 0)) if device is None else int(device)
        self.dtype = eng_cfg.get("dtype", "f32s")
        root = pathlib.Path(__file__).resolve().parents[2]
        weights = weights or {}
        self._det_w = weights.get("detector") or _load_weights(root, sk["Detect"]["model_path"], "detector")
        self._arch = str(sk["Keypoints"].get("model", "student"))
        self._kps_w = weights.get("keypoints") or _load_weights(root, sk["Keypoints"]["model_path"],
                                                                "teacher" if self._arch == "teacher" else "keypoints")
        self._det_shape = tuple(int(v) for v in sk["Detect"]["input_shape"][:2])
        self._kps_size = int(sk["Keypoints"]["input_shape"][0])
        self.score_thrs = float(sk["Detect"]["score_thrs"])
        self.iou_thrs = float(sk["Detect"]["iou_thrs"])
        self.min_face = float(sk["Detect"]["min_face"])
        self.top_k = int(top_k if top_k is not None else sk["Detect"]["topk"])
        self.track_iou_thres = float(sk["Trace"]["iou_thres"])
        self._box_filter = EmaFilter(float(sk["Trace"]["smooth_box"]))
        self.lanes, self.frames_per_lane = int(lanes), int(frames_per_lane)
        self._planted_rows = None    # test instrument: callable(frames [F,H,W,3]) -> decoded detector rows [F,R,16] for run()
        self.engine = _native.BatchEngine(self.device, self.lanes, library)
        self.engine.set_option(_native.PF_OPT_HIP_GRAPH, 1 if graph else 0)
        self._load(_native.PF_NET_DETECTOR, self.dtype)
        self._load(_native.PF_NET_LANDMARK, self.dtype)

    @property
    def max_frames(self) -> int:
        return self.lanes * self.frames_per_lane

    def _load(self, slot: int, dtype: str):
        if slot == _native.PF_NET_DETECTOR:
            blob, _ = build_detector_program(self._det_w, self._det_shape, dtype)
            self.engine.load_program(slot, blob, self.frames_per_lane)
        else:
            if self._arch == "teacher":
                from ...graph.teacher import build_teacher_program
                blob, _ = build_teacher_program(self._kps_w, self._kps_size, dtype, face_attrs=self.face_attributes)
            else:
                blob, _ = build_student_program(self._kps_w, self._kps_size, dtype, face_attrs=self.face_attributes)
            self.engine.load_program(slot, blob, self.frames_per_lane * self.top_k)

    def _guarded(self, fn, *args, **kw):
        """The f32s range guard (PF_OPT_RANGE_CHECK) names the program whose activations left the representable range: that
        network is reloaded on every lane with exact-f32 convolutions and the call repeated (as FaceAna does)."""
        for _ in range(3):
            try:
                return fn(*args, **kw)
            except _native.PeppaHipError as e:
                m = _RANGE_ERR.search(str(e))
                if not m:
                    raise
                logger.warning("range guard: %s -- reloading network %s as exact f32 on all %d lanes", e, m.group(1), self.lanes)
                self._load(int(m.group(1)), "f32")
        raise _native.PeppaHipError("range guard fallback did not converge")

    def run_arrays(self, frames: np.ndarray, planted_rows: Optional[np.ndarray] = None):
        """frames ``[F,H,W,3]`` BGR uint8 (F <= lanes * frames_per_lane) -> (counts [F], boxes [F,top_k,4], landmarks
        [F,top_k,98,2], scores [F,top_k,98]); rows of a frame beyond its count are undefined."""
        frames = np.asarray(frames)
        if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
            raise ValueError("frames must be uint8 [F,H,W,3]")
        if frames.shape[0] > self.max_frames:
            raise ValueError("%d frames exceed lanes * frames_per_lane = %d" % (frames.shape[0], self.max_frames))
        return self._guarded(self.engine.run_frames, frames, self.score_thrs, self.iou_thrs, self.min_face, self.top_k, planted_rows)

    def _run_with_extras(self, frames, planted_rows=None):
        """run_frames + the attribute rows, chips and / or label maps of the same call ([F][top_k] rows, like kps)."""
        r = self.engine.run_frames(frames, self.score_thrs, self.iou_thrs, self.min_face, self.top_k, planted_rows)
        F, K = r[0].shape[0], self.top_k
        attrs = self.engine.face_attrs(F * K).reshape(F, K, 7) if self.face_attributes else None
        if self.face_stats:
            st, sv = self.engine.face_stats(F * K, **self.face_stats)
            self._measured = (st.reshape(F, K, 8, 9), sv.reshape(F, K))
        chips = None
        if self.face_chips:
            c, m, v = self.engine.face_chips(F * K, self.face_chips)
            chips = (c.reshape((F, K) + c.shape[1:]), m.reshape(F, K, 2, 3), v.reshape(F, K))
        masks = None
        if self.face_masks:
            lab, own, mb, mv = self.engine.face_masks(F * K)
            masks = (lab, own, mb.reshape(F, K, 4), mv.reshape(F, K))
        raw = not self.jpeg or self.jpeg["raw"]
        redacted = self.engine.face_redact(F * K, **self.redact)[0] if self.redact and raw else None
        red_jpeg = chip_jpeg = None
        if self.jpeg and self.redact:
            red_jpeg = jpeg_redacted(self.engine, self.jpeg, self.redact, F * K, frames.shape, sync=self.engine.sync)
        if self.jpeg and chips is not None:
            files = jpeg_chips(self.engine, self.jpeg, F * K, self.face_chips, chips[2], sync=self.engine.sync)
            chip_jpeg = [files[f * K:(f + 1) * K] for f in range(F)]
        if self.draw:
            self._over = draw_overlay(self.engine, self.draw, self.jpeg, self.redact, F * K, frames.shape, r[3].reshape(-1, 98),
                                      sync=self.engine.sync)
        return r + (attrs, chips, masks, redacted, red_jpeg, chip_jpeg)

    def _returned_boxes(self, det_boxes: np.ndarray, kps: np.ndarray) -> np.ndarray:
        """The 'box' a fresh ``FaceAna.run`` hands back (facer.py:81-84): not the detector's box but the hull of the face's
        landmarks, EMA-smoothed against the first detector box it overlaps (``judge_boxs(boxes_return, hulls)``)."""
        hulls = np.array([[np.min(l[:, 0]), np.min(l[:, 1]), np.max(l[:, 0]), np.max(l[:, 1])] for l in kps])
        out = []
        for i in range(hulls.shape[0]):
            for j in range(det_boxes.shape[0]):
                if _box_iou(hulls[i], det_boxes[j]) > self.track_iou_thres:
                    out.append(self._box_filter(hulls[i][:4], det_boxes[j][:4]))
                    break
            else:
                out.append(hulls[i][0:4])
        return np.array(out)

    def run(self, frames) -> List[List[Dict[str, np.ndarray]]]:
        """Per frame what ``FaceAna.run(frame)`` returns for a fresh instance: ``[{'box', 'kps', 'scores'}, ...]`` -- 'box' is
        the smoothed landmark hull like the reference's, the detector's own box rides along as 'det_box'."""
        frames = np.stack(frames) if isinstance(frames, (list, tuple)) else np.asarray(frames)
        out: List[List[Dict[str, np.ndarray]]] = []
        all_labels, all_owners, all_redacted, all_red_jpeg = [], [], [], []
        all_drawn, all_drawn_jpeg = [], []
        raw = not self.jpeg or self.jpeg["raw"]
        for s in range(0, frames.shape[0], self.max_frames):
            chunk = frames[s:s + self.max_frames]
            attrs = chips = masks = redacted = red_jpeg = chip_jpeg = None
            planted = self._planted_rows(chunk) if self._planted_rows is not None else None
            if self.face_attributes or self.face_chips or self.face_masks or self.redact or self.draw or self.face_stats:
                if chunk.ndim != 4 or chunk.shape[-1] != 3 or chunk.dtype != np.uint8:
                    raise ValueError("frames must be uint8 [F,H,W,3]")
                counts, boxes, kps, scores, attrs, chips, masks, redacted, red_jpeg, chip_jpeg = self._guarded(self._run_with_extras, chunk, planted)
            else:
                counts, boxes, kps, scores = self.run_arrays(chunk, planted)
            for f in range(counts.shape[0]):
                n = int(counts[f])
                ret = self._returned_boxes(boxes[f, :n], kps[f, :n]) if n else np.zeros((0, 4), np.float32)
                res = [{"box": ret[i], "kps": kps[f, i], "scores": scores[f, i], "det_box": boxes[f, i]} for i in range(n)]
                if attrs is not None:           # per-frame network output, not smoothed
                    for i, d in enumerate(res):
                        d["pose"] = attrs[f, i, :3].copy()
                        d["attrs"] = attrs[f, i, 3:7].copy()
                if chips is not None:           # cut with the landmarks the result carries; a degenerate fit gets neither key
                    for i, d in enumerate(res):
                        if chips[2][f, i]:
                            if raw:
                                d["chip"] = chips[0][f, i].copy()
                            d["chip_matrix"] = chips[1][f, i].copy()
                        if chip_jpeg is not None:
                            d["chip_jpeg"] = chip_jpeg[f][i]
                if masks is not None:
                    attach_masks(res, masks[0][f], masks[1][f], masks[2][f], masks[3][f])
                if self.face_stats:
                    attach_stats(res, self._measured[0][f], self._measured[1][f])
                out.append(res)
            if masks is not None:
                all_labels.append(masks[0]); all_owners.append(masks[1])
            if self.draw:
                if self._over[0] is not None:
                    all_drawn.append(self._over[0])
                if self._over[1] is not None:
                    all_drawn_jpeg += self._over[1]
            if redacted is not None:
                all_redacted.append(redacted)
            if red_jpeg is not None:
                all_red_jpeg += red_jpeg
        if self.face_masks and all_labels:
            self.last_label_maps, self.last_owner_maps = np.concatenate(all_labels), np.concatenate(all_owners)
        if all_redacted:
            self.last_redacted = np.concatenate(all_redacted)
        if all_red_jpeg:
            self.last_redacted_jpeg = all_red_jpeg
        if all_drawn:
            self.last_drawn = np.concatenate(all_drawn)
        if all_drawn_jpeg:
            self.last_drawn_jpeg = all_drawn_jpeg
        return out

    def close(self):
        self.engine.close()

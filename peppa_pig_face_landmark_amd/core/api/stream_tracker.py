"""StreamTracker: ``FaceAna.run()`` with tracking for N camera feeds on one engine.

``StreamTracker(max_streams=N).run({stream_id: frame, ...}) -> {stream_id: [{'box', 'kps', 'scores'}, ...]}`` advances
every listed stream by one frame in one engine call (``pf_track_streams``): the frame-difference gate of all of them is
one kernel and one read-back, the detector runs once on the frames whose gate opened, the landmark stage once on all of
them, and the frame-to-frame state (track boxes, landmark sets, One-Euro filters, previous frame) of stream s stays on
the device in slot s.  Per stream the answers are those of a ``FaceAna`` with ``device_tracking`` on its own engine.
A stream absent from a call keeps its state; ``reset(stream_id)`` is ``FaceAna.reset()`` of one stream."""
from __future__ import annotations

import logging
import pathlib
from typing import Dict, Optional

import numpy as np

from ... import _native
from ...logger.logger import logger
from .facer import FaceAna, _load_weights, draw_options, draw_overlay, get_cfg, jpeg_chips, jpeg_options, jpeg_redacted, stage_options
from .quality import attach_stats, best_shots_options, stats_options
from ..smoother.ident import ids_options, spare_select
from .hip_model_base import HIPEngine, run_guarded


class StreamTracker:
    def __init__(self, cfg: Optional[dict] = None, weights: Optional[dict] = None, max_streams: int = 8,
                 device: Optional[int] = None, library: Optional[str] = None, verbose: bool = False,
                 face_attributes: Optional[bool] = None, face_chips: Optional[int] = None,
                 face_masks: Optional[bool] = None, redact: Optional[dict] = None, jpeg=None, draw=None,
                 track_ids=None, spare_ids: Optional[Dict[int, set]] = None, face_stats=None, best_shots=None):
        """``face_stats`` (default: ``Engine.face_stats`` of the configuration if present, else off) and ``best_shots``: the options
        of ``FaceAna``; every result dict gets ``"stats"`` and ``"quality"``, and ``best_shots`` (a ``BestShots``) keeps the best
        result of every (stream id, id).

        ``track_ids`` (default: ``Engine.track_ids`` of Skps.yml, off): the option of ``FaceAna``; every result dict gets
        ``"id"`` and ``"age"``.  Ids are per stream: unique across streams is (stream id, id).  ``spare_ids`` (stream id -> set of
        ids, needs ``track_ids``; may be changed between calls through the attribute): with ``redact`` on, a face of stream s whose
        id is in ``spare_ids[s]`` is not redacted, every other face is.

        ``draw`` (default: ``Engine.draw`` of Skps.yml, off): the dict of ``FaceAna``; ``last_drawn`` (stream id -> uint8 [H,W,3])
        keeps the frames of the last call with the faces the results carry drawn on, ``last_drawn_jpeg`` (stream id -> bytes) their
        files with ``jpeg`` on.

        ``jpeg`` (default: ``Engine.jpeg`` of the configuration if present, else off): the option of ``FaceAna``;
        ``last_redacted_jpeg`` (stream id -> bytes) and ``"chip_jpeg"`` in every result dict, encoded on the GPU; ``"raw": False``
        drops ``last_redacted`` and ``"chip"``.

        ``redact`` (default: ``Engine.redact`` of Skps.yml, off): the dict of ``FaceAna``; ``last_redacted`` (stream id -> uint8
        [H,W,3]) keeps the frames of the last call with every face the results carry redacted.

        ``face_masks`` (default: ``Engine.face_masks`` of Skps.yml, false): ``"mask_box"`` and ``"mask"`` in every result dict as in
        ``FaceAna``; the whole maps of the last call stay reachable as ``last_label_maps`` / ``last_owner_maps`` (stream id -> uint8
        [H,W]).

        ``face_chips`` (default: ``Engine.face_chips`` of Skps.yml, 0 = off): a chip size adds ``"chip"`` and ``"chip_matrix"`` to
        every result dict as in ``FaceAna``.

        ``face_attributes`` (default: ``Engine.face_attributes`` of Skps.yml): every result dict also gets ``"pose"`` and
        ``"attrs"`` as in ``FaceAna`` (per-frame network output, not smoothed)."""
        if verbose:
            logger.setLevel(logging.DEBUG)
        if int(max_streams) < 1:
            raise ValueError("max_streams must be >= 1")
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

        self.face_attributes, self.face_chips, self.face_masks, self.redact = stage_options(eng_cfg, face_attributes, face_chips, face_masks, redact)
        self.last_redacted: Optional[Dict[int, np.ndarray]] = None
        self.jpeg = jpeg_options(jpeg, eng_cfg)
        self.last_redacted_jpeg: Optional[Dict[int, bytes]] = None
        self.draw = draw_options(draw, eng_cfg, self.redact)
        self.last_drawn: Optional[Dict[int, np.ndarray]] = None
        self.last_drawn_jpeg: Optional[Dict[int, bytes]] = None
        self.track_ids = ids_options(track_ids, eng_cfg)
        if spare_ids is not None and not self.track_ids:
            raise ValueError("spare_ids needs track_ids on")
        self.spare_ids: Dict[int, set] = {int(s): set(v) for s, v in (spare_ids or {}).items()}
        self.face_stats = stats_options(face_stats, eng_cfg)
        self.best_shots = best_shots_options(best_shots, self.track_ids, self.face_stats)
        self.last_label_maps: Dict[int, np.ndarray] = {}
        self.last_owner_maps: Dict[int, np.ndarray] = {}
        self.max_streams = int(max_streams)
        self.top_k = int(sk["Detect"]["topk"])
        self._det_cfg = sk["Detect"]
        self.min_face = sk["Detect"]["min_face"]
        self.iou_thres = sk["Trace"]["iou_thres"]
        self.alpha = sk["Trace"]["smooth_box"]
        self.diff_thres = 5
        self._planted_rows = None    # test instrument: callable(stream_ids, frames [n,H,W,3]) -> decoded detector rows [n,R,16]
        self.engine = _native.Engine(dev, library)
        # both programs sized for a call that advances every stream: one detector frame and top_k faces per stream
        self.detector = HIPEngine(det_w, "detector", sk["Detect"]["input_shape"], dtype=dtype, max_batch=self.max_streams,
                                  engine=self.engine)
        self.landmark = HIPEngine(kps_w, "keypoints", sk["Keypoints"]["input_shape"], dtype=dtype,
                                  max_batch=self.max_streams * self.top_k, engine=self.engine, arch=kps_arch,
                                  face_attrs=self.face_attributes)
        self.engine.track_streams_config(self.max_streams, self.top_k)
        if self.track_ids:
            self.engine.track_ids_config(True, self.track_ids["keep_lost"])
        self.last_detector_ran: Dict[int, bool] = {}
        logger.info("stream tracker init done (%d streams)", self.max_streams)

    def run(self, frames: Dict[int, np.ndarray]) -> Dict[int, list]:
        """One FaceAna.run() per listed stream; all frames of a call have one size."""
        if not frames:
            return {}
        ids = [int(s) for s in frames]
        batch = np.stack([np.ascontiguousarray(frames[s]) for s in frames])
        planted = self._planted_rows(ids, batch) if self._planted_rows is not None else None
        K = self.top_k

        over = [None, None]
        measured = [None]

        def call(*args):
            r = self.engine.track_streams(*args)
            if self.face_stats:                        # the call's [n][top_k] rows, compacted like kps
                measured[0] = self.engine.face_stats(len(r) * K, **self.face_stats)
            attrs = chips = masks = redacted = red_jpeg = chip_jpeg = ident = None
            raw = not self.jpeg or self.jpeg["raw"]
            red = self.redact
            if self.track_ids:                         # ids / ages of the call's [n][top_k] rows, and the select they imply
                ident = self.engine.track_ids(len(r) * K)
                if self.redact:
                    red = dict(self.redact, select=np.concatenate(
                        [spare_select(ident[0][i * K:(i + 1) * K], self.spare_ids.get(s)) for i, s in enumerate(ids)]))
            if self.draw:                              # the scores of the call's [n][top_k] rows, compacted like kps
                sc = np.zeros((len(r), K, 98), np.float32)
                for i, (b, _, s_i, _) in enumerate(r):
                    sc[i, :len(b)] = s_i
                over[:] = draw_overlay(self.engine, self.draw, self.jpeg, red, len(r) * K, batch.shape, sc.reshape(-1, 98))
            if self.redact and raw:
                redacted = self.engine.face_redact(len(r) * K, **red)[0]      # one frame per listed stream
            if self.redact and self.jpeg:
                red_jpeg = jpeg_redacted(self.engine, self.jpeg, red, len(r) * K, batch.shape)
            if self.face_attributes:
                a = self.engine.face_attrs(len(r) * K)           # [n][top_k] rows, compacted like kps
                attrs = [a[i * K:i * K + len(b)] for i, (b, _, _, _) in enumerate(r)]
            if self.face_chips:
                c = self.engine.face_chips(len(r) * K, self.face_chips)      # the same rows
                chips = [tuple(x[i * K:i * K + len(b)] for x in c) for i, (b, _, _, _) in enumerate(r)]
                if self.jpeg:
                    files = jpeg_chips(self.engine, self.jpeg, len(r) * K, self.face_chips, c[2])
                    chip_jpeg = [files[i * K:i * K + len(b)] for i, (b, _, _, _) in enumerate(r)]
            if self.face_masks:
                lab, own, mb, mv = self.engine.face_masks(len(r) * K)        # one map per listed stream, slots = the same rows
                masks = [(lab[i], own[i], mb[i * K:(i + 1) * K], mv[i * K:(i + 1) * K]) for i in range(len(r))]
            return r, attrs, chips, masks, redacted, red_jpeg, chip_jpeg, ident
        res, attrs, chips, masks, redacted, red_jpeg, chip_jpeg, ident = run_guarded([self.detector, self.landmark], call, ids, batch,
                                 float(self._det_cfg["score_thrs"]), float(self._det_cfg["iou_thrs"]), float(self.min_face),
                                 float(self.iou_thres), float(self.alpha), float(self.diff_thres), planted)
        self.last_detector_ran = {s: ran for s, (_, _, _, ran) in zip(ids, res)}   # did the gate run the detector
        if redacted is not None:
            self.last_redacted = {s: redacted[i] for i, s in enumerate(ids)}
        if red_jpeg is not None:
            self.last_redacted_jpeg = {s: red_jpeg[i] for i, s in enumerate(ids)}
        if over[0] is not None:
            self.last_drawn = {s: over[0][i] for i, s in enumerate(ids)}
        if over[1] is not None:
            self.last_drawn_jpeg = {s: over[1][i] for i, s in enumerate(ids)}
        if masks is not None:
            self.last_label_maps = {s: m[0] for s, m in zip(ids, masks)}
            self.last_owner_maps = {s: m[1] for s, m in zip(ids, masks)}
        out = {s: FaceAna.with_ids(
                    self.to_dict(b, k, sc, attrs[i] if attrs is not None else None, chips[i] if chips is not None else None,
                                 masks[i] if masks is not None else None, chip_jpeg[i] if chip_jpeg is not None else None,
                                 not self.jpeg or self.jpeg["raw"]),
                    None if ident is None else (ident[0][i * K:(i + 1) * K], ident[1][i * K:(i + 1) * K]))
               for i, (s, (b, k, sc, _)) in enumerate(zip(ids, res))}
        if measured[0] is not None:
            for i, s in enumerate(ids):
                attach_stats(out[s], measured[0][0][i * K:(i + 1) * K], measured[0][1][i * K:(i + 1) * K])
                if self.best_shots is not None:
                    self.best_shots.update(out[s], stream=s)
        return out

    to_dict = staticmethod(FaceAna.to_dict)

    def reset(self, stream_id: Optional[int] = None):
        """FaceAna.reset() of one stream, or of every stream (None)."""
        self.engine.track_streams_reset(-1 if stream_id is None else int(stream_id))

    def close(self):
        self.engine.close()

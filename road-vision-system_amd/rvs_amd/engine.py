"""Batched per-frame hot path: S camera streams x 1 frame per step.

Reproduces the reference's per-frame call order (main_preview.py:94-109):
    proc = pipeline(raw)                 -> fused CLAHE + median (HIP), which
                                            also emits the detector's letterbox
    dets = detector.infer(proc)          -> YOLOv8 + NMS (HIP)
    dets = tracker.update(dets, ts, projector)   -> SORT + geometry (HIP)
for a stream-major batch, entirely on the device: no host round trip inside a
step.  ``results()`` converts one step's device outputs into the reference's
``Detection`` lists (the only device->host copy, ~S*max_det*6 floats).
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import load_config
from .detect.types import Detection
from .detect.weights import detector_weights, names_from_config, resolve_model
from .detect.yolo_hip import YoloEngine
from .geometry import GroundProjector, build_camera_projectors, build_projector
from .handback import Record, handback
from .io_video.sink import MultiStreamSink, record_settings
from .preprocess import PreprocessPipeline
from .track.byte_hip import MultiStreamByte, byte_thresholds
from .track.registry import BYTE_BACKENDS, backend_name
from .track.sort_hip import CameraTable, MultiStreamSort
from .vis.display_list import canvas_geometry
from .vis.overlay import OverlayRenderer


class RoadVisionEngine:
    def __init__(self, cfg: Optional[dict], n_streams: int, frame_hw, device="cuda",
                 tmax: int = 1024, projector: Optional[GroundProjector] = None,
                 weights: Optional[np.ndarray] = None, lanes: int = 1, pair: int = 1,
                 projectors: Optional[Sequence[Optional[GroundProjector]]] = None):
        """projectors: one ground projector (or None) per camera stream, as
        the reference runs one process -- one geometry.projector -- per
        camera; default: the config's geometry.cameras, when present.  It
        wins over `projector` / geometry.projector (one calibration for every
        stream).  set_camera_projector recalibrates one camera later.

        pair = P >= 2: the pipelined schedule (schedule.PipelinedRun)
        runs the forwards of P consecutive steps as one batch of P*S frames
        (the small P4 / P5 layers amortise their per-launch floor; measured
        B = 64: 20.5 us per frame against 25.0 at B = 32,
        tools/probe_batch.py).  Every stream still sees its frames in order
        in SORT, so results are those of sequential step() calls; a frame's
        results come out P - 1 steps later.

        tracking.backend "bytetrack" / "byte" / "bytetrack_hip": the tracker
        is MultiStreamByte (ByteTrack's second association on low-score
        detections, track/byte_hip.py) and the detector runs at conf =
        tracking.track_low_thresh instead of detect.conf_thres, so the low
        rows reach the tracker.  NMS never lets a lower score suppress a
        higher one and its output is score-ordered, so the rows at or above
        tracking.track_high_thresh (default: detect.conf_thres) are the rows
        the SORT configuration would see -- as long as an image has at most
        detect.max_det rows at conf = low; beyond that NMS cuts the list at
        max_det either way, and the low rows do not displace high ones (they
        sort behind them).  Every stage downstream of the tracker (hand-back,
        overlays, recording, out["dets"] / out["det_n"]) sees the rows the
        tracker kept, not the NMS output.  0 < low <= high <= 1 is required
        (ValueError).  Every other backend value builds the SORT tracker."""
        cfg = cfg if cfg is not None else load_config()
        self.cfg = cfg
        self.S = int(n_streams)
        # preview.record: checked before anything is built (a wrong container
        # or a shared path is a configuration error, not a feature to drop)
        record_cfg = record_settings(cfg, self.S)
        self.recorder = None
        self.pair = max(1, int(pair))
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        self.device = torch.device(device)
        self.pipeline = PreprocessPipeline(cfg.get("preprocess", {}) or {})
        det_cfg = cfg.get("detect", {}) or {}
        trk_cfg = cfg.get("tracking", {}) or {}
        # main_preview.py:60-70: the detector and the tracker exist only when
        # their `enabled` key is set (src/config.py defaults both to False)
        self.detect_enabled = bool(det_cfg.get("enabled", False))
        self.tracking_enabled = bool(trk_cfg.get("enabled", False))
        # tracking.backend: BYTE needs the detector's low rows (a wrong
        # threshold pair is a configuration error, not a feature to drop)
        conf_thres = float(det_cfg.get("conf_thres", 0.25))
        self.byte = self.tracking_enabled and backend_name(trk_cfg) in BYTE_BACKENDS
        if self.byte:
            low, high = byte_thresholds(trk_cfg, conf_thres)
            trk_cfg = dict(trk_cfg, track_low_thresh=low, track_high_thresh=high)
            conf_thres = low
        self.variant = resolve_model(det_cfg.get("model", "yolov8n.pt"))
        self.detector = None
        # class count and names: the checkpoint's / the config's (detect.nc,
        # detect.names); caller-supplied flat weights carry detect.nc classes
        self.nc = int(det_cfg.get("nc", 80))
        if self.detect_enabled:
            if weights is None:
                weights, self.nc = detector_weights(det_cfg, self.variant)
            self.detector = YoloEngine(
                self.variant, weights, self.S * self.pair, (self.H, self.W),
                imgsz=int(det_cfg.get("imgsz", 640)),
                conf=conf_thres,
                iou=float(det_cfg.get("iou_thres", 0.7)),
                max_det=int(det_cfg.get("max_det", 100)),
                classes_keep=[int(x) for x in det_cfg.get("classes_keep", [])],
                device=self.device, lanes=lanes, nc=self.nc)
            if self.detector.lanes > 1:
                # a multi-lane engine runs pipelined stages (schedule.PipelinedRun):
                # its forwards keep the Detect heads on the stage's own stream
                # instead of two more side streams per handle sharing the 4
                # hardware queues (r04: +3 % frames/s)
                self.detector.set_head_streams(False)
        self.max_det = self.detector.max_det if self.detector is not None else \
            int(det_cfg.get("max_det", 100))
        # main_preview.py:64-78: a tracker or projector that fails to build
        # is reported and left off (the run goes on without that feature)
        geom = cfg.get("geometry", {}) or {}
        if projectors is None and projector is None and geom.get("enabled", False):
            # geometry.cameras: one projector mapping (or null) per stream
            projectors = build_camera_projectors(geom, self.S)
        if projectors is not None:
            projectors = list(projectors)
            if len(projectors) != self.S:
                raise ValueError(f"{len(projectors)} projectors for {self.S} camera streams")
            projector = None
        self.projectors = projectors
        if projector is None and projectors is None:
            if geom.get("enabled", False):
                try:
                    projector = build_projector(geom)
                except Exception as exc:
                    warnings.warn(f"geometry projector init failed, running without it: {exc}")
                    projector = None
        self.projector = projector
        self.tracker = None
        if self.tracking_enabled and self.detector is not None:
            try:
                tracker = (MultiStreamByte if self.byte else MultiStreamSort)(
                    trk_cfg, self.S, tmax=tmax, dmax=self.max_det, device=self.device)
                if projectors is not None:
                    tracker.set_projectors(projectors)
                else:
                    tracker.set_projector(projector)
                self.tracker = tracker
            except Exception as exc:
                warnings.warn(f"tracker init failed, running without it: {exc}")
                self.tracker = None
        if self.tracker is None and self.detector is not None:
            # tracker off (main_preview.py:104-109): ids and speeds stay None,
            # each detection gets projector.distance_for_bbox when a projector exists
            self._untracked = _UntrackedMetrics(self.S, self.max_det, projector, self.device,
                                                projectors=projectors)
        self.proc = torch.empty((self.S, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        self.names = names_from_config(det_cfg, self.nc)
        # result hand-back: device staging buffer + the pinned host record of step()
        self.record = Record(self.S, self.max_det, self.device)
        self.rec_stage = torch.empty(self.record.nbytes, dtype=torch.uint8, device=self.device)
        # vis.draw (main_preview.py:113-116): the overlays of annotate() and of
        # a recording with preview.record.content "annotated" / "compare"
        draw_cfg = (cfg.get("vis") or {}).get("draw") or {}
        self.draw_det = bool(draw_cfg.get("det", True)) and self.detector is not None
        self._draw_args = (int(draw_cfg.get("thickness", 2)), float(draw_cfg.get("font_scale", 0.6)))
        self._annotators: Dict[bool, OverlayRenderer] = {}
        self._rec_overlay = None
        self._rec_n = 0
        if record_cfg is not None:
            # main_preview.py:130,137 (writer.write): every stream's frames as a
            # Motion-JPEG file, encoded on a side stream of step()
            content = record_cfg.get("content", "proc")
            hw = (self.H, self.W)
            if content == "compare":
                cmp_cfg = (cfg.get("preview") or {}).get("compare") or {}
                hw = canvas_geometry(self.H, self.W, cmp_cfg.get("layout", "h"),
                                     cmp_cfg.get("divider_px", 4))[:2]
            self.recorder = MultiStreamSink(record_cfg["paths"], hw,
                                            quality=record_cfg["quality"],
                                            sampling=record_cfg["sampling"], device=self.device)
            if content != "proc":
                # display lists rotate as deep as the sink's device buffers
                self._rec_overlay = self._overlay(content == "compare", self.recorder.nbuf + 1)
                self._rec_canvas = torch.empty((self.S, hw[0], hw[1], 3), dtype=torch.uint8,
                                               device=self.device)

    def _overlay(self, compare: bool, slots: int) -> OverlayRenderer:
        cmp_cfg = (self.cfg.get("preview") or {}).get("compare") or {}
        return OverlayRenderer(self.S, (self.H, self.W), self.max_det, self.names,
                               self._draw_args[0], self._draw_args[1], self.device,
                               compare={k: cmp_cfg[k] for k in ("layout", "divider_px", "label_raw",
                                                                "label_proc") if k in cmp_cfg}
                               if compare else None, slots=slots)

    def _record_proc(self, proc: torch.Tensor, frames: Optional[torch.Tensor] = None) -> None:
        """preview.record: queue this step's proc frames for the files.  The
        encode waits (on its own stream) for an event recorded here, behind
        the preprocess; the current stream goes on with the detector.  With
        overlays to draw the frames are queued by _record_overlay instead,
        once the step's results exist."""
        if self.recorder is None:
            return
        if self._rec_overlay is None:
            self.recorder.write(proc)
        elif not self.draw_det:
            self._record_overlay(proc, frames, None)

    def _record_overlay(self, proc: torch.Tensor, frames: Optional[torch.Tensor], res) -> None:
        """preview.record.content "annotated" / "compare": the display lists
        of this step's results `res` (dets, det_n, track_id, distance_m,
        speed_kmh; None: nothing to draw) are laid out on the current stream
        -- the next step overwrites the results -- and the raster and the
        encode run on the sink's stream behind an event recorded here; the
        current stream waits for neither."""
        ov = self._rec_overlay
        if ov.compare is None and res is None:
            self.recorder.write(proc)  # vis.draw.det false: plain proc
            return
        if ov.compare is not None and frames is None:
            raise ValueError("a compare recording needs the step's raw frames")
        slot = None
        if res is not None:
            slot = self._rec_n % ov.lists.shape[0]
            self._rec_n += 1
            ov.layout(*res, slot=slot)
        raw = frames if ov.compare is not None else None
        self.recorder.write([proc] if raw is None else [proc, raw],
                            render=lambda: ov.raster(proc, raw, out=self._rec_canvas, slot=slot))

    def annotate(self, out: Dict[str, torch.Tensor],
                 frames: Optional[torch.Tensor] = None) -> torch.Tensor:
        """What the reference shows for one step's `out`: its proc frames
        with draw_detections (vis.draw.thickness / font_scale) when
        vis.draw.det is set and the detector runs -- (S, H, W, 3) -- or, given
        the step's raw `frames`, make_canvas(frames, annotated proc) with
        preview.compare's layout, divider and labels.  A new device tensor,
        on the current stream; no FPS text.  Call it before the next step()
        overwrites the step's results."""
        compare = frames is not None
        if compare not in self._annotators:
            self._annotators[compare] = self._overlay(compare, 1)
        ov = self._annotators[compare]
        if self.draw_det and not out.get("no_detector"):
            ov.layout(out["dets"], out["det_n"], out["track_id"], out["distance_m"],
                      out["speed_kmh"], slot=0)
            return ov.raster(out["proc"], frames, slot=0)
        if not compare:
            return out["proc"].clone()
        return ov.raster(out["proc"], frames, slot=None)

    def _need_detector(self, what: str) -> None:
        if self.detector is None:
            raise ValueError(f"{what} needs the detector (detect.enabled is false); "
                             "step() runs the preprocess-only path")

    def preprocess_stage(self, frames: torch.Tensor, lb_slot: int = 0, lb_off: int = 0,
                         proc: Optional[torch.Tensor] = None):
        """pipeline(raw) + the detector's LetterBox (main_preview.py:94-99)
        for (S,H,W,3) u8 device frames -> (proc, letterboxed batch in the
        detector's letterbox slot `lb_slot`, images [lb_off, lb_off + S)).
        proc: a caller-owned buffer to fill (rvs_amd.schedule: a recorded
        schedule must not allocate per run)."""
        if self.pipeline.chain_supported:
            # any chain of the built-in ops, the gate included: one
            # stream-ordered library call (the gate is evaluated on the device)
            if self.detector is None:
                return self.pipeline.run_chain_with_letterbox(frames, out=proc)
            B = frames.shape[0]
            return self.pipeline.run_chain_with_letterbox(
                frames, self.detector.geo, self.detector.lb[lb_slot][lb_off:lb_off + B], out=proc)
        if proc is not None and _lib._recorder is not None:
            raise RuntimeError("a recorded schedule needs a preprocess chain of the built-in ops "
                               "(CLAHEDehaze / MedianDerain, at most 4): this chain has "
                               f"{self.pipeline.unsupported_op}, which runs eagerly with torch "
                               "allocations and copies")
        p = self.pipeline(frames)
        lb = None if self.detector is None else self.detector.letterbox(p, lb_slot, lb_off)
        if proc is None:
            return p, lb
        proc.copy_(p)
        return proc, lb

    def yolo_stage(self, lb: Optional[torch.Tensor], slot: int = 0, lane: int = 0,
                   part: int = 0, batch: Optional[int] = None) -> None:
        """YOLOv8 forward + decode in forward context `lane`; NMS candidates
        land in candidate slot `slot`.  part 1 / 2: the two halves of the
        forward (YoloEngine.forward_raw); part 2 continues part 1's batch
        (`batch` images, default S * pair)."""
        self._need_detector("yolo_stage")
        self.detector.forward_raw(lb, slot=slot, lane=lane, part=part,
                                  batch=batch if batch is not None else self.S * self.pair)

    def detect_stage(self, frames: torch.Tensor, slot: int = 0) -> torch.Tensor:
        self._need_detector("detect_stage")
        proc, lb = self.preprocess_stage(frames)
        self._record_proc(proc, frames)
        self.yolo_stage(lb, slot)
        return proc

    def autotune(self, frames: torch.Tensor, reps: int = 3, verify: bool = False) -> int:
        """Autotune the detector's conv kernels on one batch of these frames
        (YoloEngine.autotune; pair mode: the batch of P*S the pipelined
        forwards run, the frames repeated); call outside graph capture."""
        self._need_detector("autotune")
        for h in range(self.pair):
            self.preprocess_stage(frames, 0, h * self.S)
        lb = self.detector.lb[0][:self.S * self.pair]
        return self.detector.autotune(lb, reps=reps, verify=verify)

    def track_stage(self, ts: torch.Tensor, slot: int = 0,
                    record: Optional[Record] = None) -> Dict[str, torch.Tensor]:
        """NMS of candidate slot `slot` + SORT/geometry (main_preview.py:99-109),
        then the hand-back of the results into `record` (pinned host)."""
        self._need_detector("track_stage")
        dets, det_n = self.detector.nms(ts.shape[0], slot)
        dets, det_n, tid, dist, spd = self._tracked(dets, det_n, ts)
        out = {"dets": dets, "det_n": det_n, "track_id": tid, "distance_m": dist,
               "speed_kmh": spd}
        if record is not None:
            handback(dets, det_n, tid, dist, spd, self.rec_stage, record.host)
            record.seq += 1
            out["record"] = record
            out["seq"] = record.seq
        return out

    def track_pair_stage(self, ts_list, slot: int, records,
                         overlay=None) -> List[Dict[str, torch.Tensor]]:
        """Pair mode: NMS of the P*S images of candidate slot `slot` at once,
        then SORT + hand-back of each of the P steps in order (step h owns
        images [h*S, (h+1)*S)).  overlay: the (proc, raw frames) of each step
        of a recording that draws overlays; every step is laid out and queued
        right behind its SORT, before the next step's overwrites the results."""
        self._need_detector("track_pair_stage")
        S = self.S
        dets, det_n = self.detector.nms(S * len(ts_list), slot)
        outs = []
        for h, (ts, rec) in enumerate(zip(ts_list, records)):
            d, n, tid, dist, spd = self._tracked(dets[h * S:(h + 1) * S],
                                                 det_n[h * S:(h + 1) * S], ts)
            handback(d, n, tid, dist, spd, self.rec_stage, rec.host)
            if overlay is not None:
                self._record_overlay(overlay[h][0], overlay[h][1], (d, n, tid, dist, spd))
            outs.append({"record": rec})
        return outs

    def track_handback(self, dets: torch.Tensor, det_n: torch.Tensor, ts: torch.Tensor,
                       record: Record) -> None:
        """SORT + geometry of one step's NMS output (S images), then its
        hand-back into `record` (tracker.update + the .cpu() hand-over of
        main_preview.py:99-109)."""
        self._need_detector("track_handback")
        dets, det_n, tid, dist, spd = self._tracked(dets, det_n, ts)
        handback(dets, det_n, tid, dist, spd, self.rec_stage, record.host)

    def _tracked(self, dets: torch.Tensor, det_n: torch.Tensor, ts: torch.Tensor):
        """One step's NMS output through the tracker -> (rows, counts,
        track_id, distance_m, speed_kmh) as every later stage takes them: the
        NMS buffers themselves, or with a BYTE tracker the rows it kept (its
        workspace views, rewritten by the next update like the results)."""
        tid, dist, spd = self._metrics(dets, det_n, ts)
        if self.byte and self.tracker is not None:
            dets, det_n = self.tracker.kept_dets, self.tracker.kept_n
        return dets, det_n, tid, dist, spd

    def _metrics(self, dets: torch.Tensor, det_n: torch.Tensor, ts: torch.Tensor):
        """(track_id, distance_m, speed_kmh) of one step's NMS output:
        SortTracker.update when tracking is enabled, else the tracker-off
        branch of main_preview.py:101-109 (rv_untracked_metrics)."""
        if self.tracker is not None:
            return self.tracker.update(dets, det_n, ts)
        return self._untracked(dets, det_n)

    def step_unit(self, frames_list, ts_list, records) -> List[Dict[str, torch.Tensor]]:
        """Pair mode, sequentially on the current stream: the preprocess of
        P consecutive steps into one letterbox slot, ONE forward over their
        P*S frames, then NMS + per-step SORT + hand-back (the work of one
        pipeline unit of schedule.PipelinedRun, each launch alone)."""
        self._need_detector("step_unit")
        S = self.S
        procs = [self.preprocess_stage(f, 0, h * S)[0] for h, f in enumerate(frames_list)]
        for p, f in zip(procs, frames_list):
            self._record_proc(p, f)
        self.yolo_stage(self.detector.lb[0][:S * len(frames_list)], 0)
        draws = self._rec_overlay is not None and self.draw_det
        outs = self.track_pair_stage(ts_list, 0, records,
                                     list(zip(procs, frames_list)) if draws else None)
        for o, p in zip(outs, procs):
            o["proc"] = p
        return outs

    def step(self, frames: torch.Tensor, ts: torch.Tensor,
             record: Optional[Record] = None) -> Dict[str, torch.Tensor]:
        """frames (S,H,W,3) u8 on device, ts (S,) f64 on device.  The step's
        results end in `record` (pinned host; default: the engine's own
        record, which the next step() overwrites -- read results(out) before
        it, or pass a Record per step).  With detect.enabled false only the
        preprocess runs and every stream's list is empty (main_preview.py:97-99)."""
        if self.detector is None:
            proc, _ = self.preprocess_stage(frames)
            self._record_proc(proc, frames)
            return {"proc": proc, "no_detector": True}
        proc = self.detect_stage(frames, 0)
        out = self.track_stage(ts, 0, self.record if record is None else record)
        out["proc"] = proc
        if self._rec_overlay is not None and self.draw_det:
            self._record_overlay(proc, frames, (out["dets"], out["det_n"], out["track_id"],
                                                out["distance_m"], out["speed_kmh"]))
        return out

    def results(self, out: Dict[str, torch.Tensor]) -> List[List[Detection]]:
        """The reference's Detection lists of one step: from its host record
        (synchronises the device first), or from the device tensors."""
        if out.get("no_detector"):
            return [[] for _ in range(self.S)]
        if "record" in out:
            if "seq" in out and out["record"].seq != out["seq"]:
                raise RuntimeError("this step's record was overwritten by a later step(): call "
                                   "results(out) before the next step(), or pass step() its own "
                                   "Record")
            torch.cuda.synchronize(self.device)
            return out["record"].detections(self.names)
        d = out["dets"].cpu().numpy()
        n = out["det_n"].cpu().numpy()
        tid = out["track_id"].cpu().numpy()
        dist = out["distance_m"].cpu().numpy()
        spd = out["speed_kmh"].cpu().numpy()
        res = []
        for s in range(d.shape[0]):
            lst = []
            for i in range(int(n[s])):
                r = d[s, i]
                k = int(r[5])
                lst.append(Detection(float(r[0]), float(r[1]), float(r[2]), float(r[3]),
                                     float(r[4]), k, str(self.names[k]) if k < len(self.names) else str(k),
                                     None if tid[s, i] < 0 else int(tid[s, i]),
                                     None if np.isnan(dist[s, i]) else float(dist[s, i]),
                                     None if np.isnan(spd[s, i]) else float(spd[s, i])))
            res.append(lst)
        return res

    def set_camera_projector(self, s: int, projector: Optional[GroundProjector]) -> None:
        """Recalibrate camera stream s (None: remove its projector) for every
        later step: one stream-ordered copy into the device table on the
        current stream (MultiStreamSort.set_camera_projector, or the
        tracker-off metrics' table).  A recorded PipelinedRun reads the same
        table, so it follows the change without being recorded again -- but
        call this between its runs (after the previous run has been waited
        for), not while one is in flight: the run's SORT launches are on
        other streams and would see the copy at an undefined step.  An engine
        built with a single projector switches to a table in which every
        other camera keeps that projector; a PipelinedRun recorded before
        that switch still holds the single-projector calls."""
        if not 0 <= int(s) < self.S:
            raise IndexError(f"camera {s} outside [0, {self.S})")
        if self.tracker is not None:
            self.tracker.set_camera_projector(s, projector)
        elif self.detector is not None:
            self._untracked.set_camera_projector(s, projector)
        if self.projectors is None:
            self.projectors = [self.projector] * self.S
            self.projector = None
        self.projectors[int(s)] = projector

    def track_stats(self) -> Dict[str, np.ndarray]:
        """Per-stream SORT capacity report (MultiStreamSort.stats); empty
        arrays when tracking is off."""
        if self.tracker is None:
            z = np.zeros(self.S, np.int32)
            return {"T": z, "next_id": z.copy(), "overflow": z.copy()}
        return self.tracker.stats()

    def close(self):
        """Also finishes a recording: queued frames are written, the files are
        flushed, and a frame that could not be written is raised here."""
        if self.detector is not None:
            self.detector.close()
        if self.recorder is not None:
            recorder, self.recorder = self.recorder, None
            recorder.close()


class _UntrackedMetrics:
    """The tracker-off outputs of one step (main_preview.py:101-109):
    track_id None (-1), speed_kmh None (NaN), distance_m =
    projector.distance_for_bbox(bbox) (projector.py:49-51) with a projector,
    else None -- on the device (rv_untracked_metrics), so the step's
    hand-back record is built exactly as with the tracker."""

    def __init__(self, S: int, dmax: int, projector: Optional[GroundProjector], device,
                 projectors: Optional[Sequence[Optional[GroundProjector]]] = None):
        """projectors (length S, entries may be None): one projector per
        camera stream from a table in device memory
        (rv_untracked_metrics_cams); it wins over `projector`."""
        self.S, self.dmax = int(S), int(dmax)
        self.cams = None
        if projectors is not None:
            if len(projectors) != self.S:
                raise ValueError(f"{len(projectors)} projectors for {self.S} camera streams")
            self.cams = CameraTable(projectors, device)
            projector = None
        self._single = projector
        self.out_id = torch.empty((self.S, self.dmax), dtype=torch.int32, device=device)
        self.out_dist = torch.empty((self.S, self.dmax), dtype=torch.float64, device=device)
        self.out_speed = torch.empty((self.S, self.dmax), dtype=torch.float64, device=device)
        self._H = self._origin = None
        self._md = -1.0
        if projector is not None:
            H, origin, md = projector.device_params()
            self._H = np.ascontiguousarray(H, np.float64)
            self._origin = np.ascontiguousarray(origin, np.float32)
            self._md = float(md)

    def set_camera_projector(self, s: int, projector: Optional[GroundProjector]) -> None:
        """Recalibrate camera s (stream-ordered copy on the current stream);
        without a table yet the other cameras start from the single projector."""
        if not 0 <= int(s) < self.S:
            raise IndexError(f"camera {s} outside [0, {self.S})")
        if self.cams is None:
            self.cams = CameraTable([self._single] * self.S, self.out_id.device)
        self.cams.set(s, projector)

    def __call__(self, dets: torch.Tensor, det_n: torch.Tensor):
        S = dets.shape[0]
        if S != self.S or dets.shape[1] != self.dmax:
            raise ValueError(f"dets must be ({self.S}, {self.dmax}, 6)")
        if self.cams is not None:
            _lib.call("rv_untracked_metrics_cams", _lib.ptr(dets), _lib.ptr(det_n), S, self.dmax,
                      _lib.ptr(self.cams.dev), _lib.ptr(self.out_id), _lib.ptr(self.out_dist),
                      _lib.ptr(self.out_speed), _lib.stream_ptr())
            return self.out_id, self.out_dist, self.out_speed
        _lib.call("rv_untracked_metrics", _lib.ptr(dets), _lib.ptr(det_n), S, self.dmax,
                  self._H.ctypes.data if self._H is not None else None,
                  self._origin.ctypes.data if self._origin is not None else None, self._md,
                  _lib.ptr(self.out_id), _lib.ptr(self.out_dist), _lib.ptr(self.out_speed),
                  _lib.stream_ptr())
        return self.out_id, self.out_dist, self.out_speed

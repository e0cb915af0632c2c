"""BYTE on the GPU: ByteTrack's second association on the reference's SORT.

ByteTrack (Zhang et al., "ByteTrack: Multi-Object Tracking by Associating
Every Detection Box", ECCV 2022) keeps the low-score detections a tracker
like SORT never sees: after the high-score detections have been associated,
the low ones are offered to the tracks that are still unmatched, and the low
ones no track claims are dropped.  In fog and rain, where scores sag, a
vehicle then keeps its id and its speed history through the frames in which
its score is under ``detect.conf_thres``.

Here this is one mode of the fused SORT kernel (csrc/sort.hip, the BYTE
instances, selected by ``params6[5] = track_high_thresh > 0``):

* a row is *high* iff ``float64(conf) >= track_high_thresh``, else *low*;
  rows below ``track_low_thresh`` never reach the tracker (the detector runs
  at ``conf = track_low_thresh``; ``ByteTracker`` filters on the host);
* stage 1: the reference's greedy association of all tracks with the high
  rows at ``iou_threshold``;
* stage 2: the same greedy loop over the tracks stage 1 left unmatched whose
  ``hit_streak`` was > 0 before the frame, and the low rows, at IoU 0.5
  (ByteTrack's constant, ``RV_BYTE_SECOND_IOU``);
* new tracks come from unmatched high rows only; unmatched low rows are
  dropped; the *kept* rows (high or matched) come back compacted in input
  order with ``track_id`` / ``distance_m`` / ``speed_kmh`` indexed by kept row.

Departures from the paper: greedy association instead of the Hungarian
algorithm, no score fusion, no separate pass for unconfirmed tracks.  It is
BYTE on the reference's SORT: with every row high it is that SORT bit for bit
(tests/byte_ref.py restates the semantics).
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Optional

import numpy as np
import torch

from .. import _lib
from .._lib import call
from ..detect.types import Detection
from ..geometry import GroundProjector
from .base import Tracker
from .sort_hip import MultiStreamSort

DEFAULT_HIGH = 0.25  # detect.conf_thres of the shipped configuration
DEFAULT_LOW = 0.1


def byte_thresholds(trk_cfg: dict, conf_thres: float = DEFAULT_HIGH):
    """(track_low_thresh, track_high_thresh) of a tracking config: high
    defaults to the detector's conf_thres, low to 0.1.  ValueError unless
    0 < low <= high <= 1."""
    high = float(trk_cfg.get("track_high_thresh", conf_thres))
    low = float(trk_cfg.get("track_low_thresh", DEFAULT_LOW))
    if not (0.0 < low <= high <= 1.0):
        raise ValueError(f"tracking.track_low_thresh={low} / track_high_thresh={high}: BYTE needs "
                         "0 < low <= high <= 1")
    return low, high


def is_below(conf: float, thr: float) -> bool:
    """The kernel's class test on the f32 score: float64(conf_f32) < thr."""
    return not (np.float64(np.float32(conf)) >= np.float64(thr))


class MultiStreamByte(MultiStreamSort):
    """MultiStreamSort with the second association.  ``update`` takes every
    row at or above track_low_thresh and returns (track_id, distance_m,
    speed_kmh) indexed by *kept* row; the kept rows and their counts are
    ``kept_dets`` (S, dmax, 6) and ``kept_n`` (S,), views of the workspace at
    addresses that never change (a recorded schedule holds them), valid from
    one update until the next.  Rows at or beyond ``kept_n[s]`` are zero /
    -1 / NaN.  ``track_high_thresh = 0`` runs the plain kernel (every row is
    kept: ``kept_dets`` / ``kept_n`` are then not written)."""

    def __init__(self, cfg: dict, n_streams: int, tmax: int = 1024, dmax: int = 128,
                 device="cuda"):
        super().__init__(cfg, n_streams, tmax=tmax, dmax=dmax, device=device)
        self.track_high_thresh = float(cfg.get("track_high_thresh", DEFAULT_HIGH))
        self.track_low_thresh = float(cfg.get("track_low_thresh", DEFAULT_LOW))
        if not 0.0 <= self.track_high_thresh <= 1.0:
            raise ValueError(f"track_high_thresh={self.track_high_thresh} is not in [0, 1]")
        self.params[5] = self.track_high_thresh
        d_off, n_off = ctypes.c_size_t(), ctypes.c_size_t()
        call("rv_sort_kept_layout", self.S, self.tmax, self.dmax, ctypes.byref(d_off),
             ctypes.byref(n_off))
        nd = self.S * self.dmax * 6 * 4
        self.kept_dets = self.ws[d_off.value:d_off.value + nd].view(torch.float32).view(
            self.S, self.dmax, 6)
        self.kept_n = self.ws[n_off.value:n_off.value + self.S * 4].view(torch.int32)
        self.kept_dets.zero_()
        self.kept_n.zero_()

    def update(self, dets: torch.Tensor, counts: torch.Tensor, ts: torch.Tensor):
        """As MultiStreamSort.update; the three results are indexed by kept
        row (``kept_dets`` / ``kept_n``)."""
        self.params[5] = self.track_high_thresh
        return super().update(dets, counts, ts)

    def update_many(self, streams, timestamps) -> List[List[Detection]]:
        return update_many(self, streams, timestamps)


def _hand_out(lst: List[Detection], kept: np.ndarray, n: int, tid, dist, spd) -> List[Detection]:
    """The kept Detection objects of one stream, mutated: kept rows are a
    subsequence of the input rows, so they are matched up in order by
    content (rows of equal content are interchangeable)."""
    out, k = [], 0
    for d in lst:
        row = np.array((d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id), np.float32)
        if k < n and row.tobytes() == kept[k].tobytes():
            d.track_id = None if tid[k] < 0 else int(tid[k])
            d.distance_m = None if np.isnan(dist[k]) else float(dist[k])
            d.speed_kmh = None if np.isnan(spd[k]) else float(spd[k])
            out.append(d)
            k += 1
    if k != n:
        raise _lib.RVError(f"BYTE hand-out: {n} kept rows, {k} found among the input")
    return out


def update_many(core: MultiStreamByte, streams, timestamps) -> List[List[Detection]]:
    """ByteTracker.update for S camera streams in one launch: per stream the
    rows below track_low_thresh are removed on the host, the rest go through
    the kernel, and the kept Detection objects come back mutated."""
    S = core.S
    lists = [list(x) for x in streams]
    if len(lists) != S or len(timestamps) != S:
        raise ValueError(f"expected {S} streams and timestamps")
    rows = np.zeros((S, core.dmax, 6), np.float32)
    cnt = np.zeros(S, np.int32)
    fed = []
    for s, lst in enumerate(lists):
        for d in lst:
            d.track_id = d.distance_m = d.speed_kmh = None
        lst = [d for d in lst if not is_below(d.conf, core.track_low_thresh)]
        if len(lst) > core.dmax:
            raise ValueError(f"{len(lst)} detections exceed dmax={core.dmax}")
        cnt[s] = len(lst)
        for i, d in enumerate(lst):
            rows[s, i] = (d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id)
        fed.append(lst)
    dev = core.device
    tid, dist, spd = core.update(torch.from_numpy(rows).to(dev), torch.from_numpy(cnt).to(dev),
                                 torch.tensor([float(t) for t in timestamps], dtype=torch.float64,
                                              device=dev))
    tid, dist, spd = tid.cpu().numpy(), dist.cpu().numpy(), spd.cpu().numpy()
    if core.track_high_thresh > 0.0:
        kept, kn = core.kept_dets.cpu().numpy(), core.kept_n.cpu().numpy()
    else:  # the plain kernel: every row is kept
        kept, kn = rows, cnt
    return [_hand_out(fed[s], kept[s], int(kn[s]), tid[s], dist[s], spd[s]) for s in range(S)]


class ByteTracker(Tracker):
    """Single-stream reference API (Tracker.update) on MultiStreamByte: the
    rows below track_low_thresh are removed on the host; the kept Detection
    objects are mutated and returned, the dropped ones are not."""

    def __init__(self, cfg: dict, tmax: int = 1024, dmax: int = 128):
        self.cfg = dict(cfg)
        low, high = byte_thresholds(self.cfg)
        if not torch.cuda.is_available():
            raise RuntimeError("ByteTracker (HIP) needs an MI355X; there is no CPU fallback")
        self.cfg.update(track_low_thresh=low, track_high_thresh=high)
        self.tmax, self.dmax = tmax, dmax
        self.core = MultiStreamByte(self.cfg, 1, tmax=tmax, dmax=dmax)
        self._proj_key = None

    def update(self, detections: Iterable[Detection], timestamp: float,
               projector: Optional[GroundProjector] = None) -> List[Detection]:
        if id(projector) != self._proj_key:
            self.core.set_projector(projector)
            self._proj_key = id(projector)
        return update_many(self.core, [list(detections)], [timestamp])[0]

    def close(self) -> None:
        self.core.reset()

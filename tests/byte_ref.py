"""Pure-Python restatement of the BYTE tracker backend (rvs_amd.track.byte_hip,
the BYTE instances of csrc/sort.hip) -- TEST INFRASTRUCTURE ONLY.

BYTE (Zhang et al., "ByteTrack: Multi-Object Tracking by Associating Every
Detection Box", ECCV 2022) on the reference's SORT: ``ByteSortTracker.update``
is ``oracle.sort_ref.SortTracker.update`` built from the same pieces
(``_Track``, ``iou_matrix``, ``greedy``, the projector) with these differences
only:

1. a detection is *high* iff ``float64(conf_f32) >= track_high_thresh``, else
   *low* (rows below ``track_low_thresh`` never get here: the caller removes
   them);
2. stage 1 is the reference's greedy loop on (all tracks, list order) x (high
   detections, row order) at ``iou_threshold``; per track ``was_tracked =
   hit_streak > 0`` is taken before the frame (ByteTrack's "Tracked, not Lost");
3. stage 2 is the same greedy loop on (tracks stage 1 left unmatched with
   ``was_tracked``, list order) x (low detections, row order) at SECOND_IOU =
   0.5; a stage-2 match is an ordinary match;
4. new tracks come from unmatched high detections only, in ascending row
   order; tracks unmatched after both stages are marked missed; pruning is
   unchanged;
5. the result is the kept rows -- all high detections plus the matched low
   ones, in input order; unmatched low detections are dropped.

Departures from the paper: greedy association instead of the Hungarian
algorithm, no score fusion, no separate pass for unconfirmed tracks.  With
``track_high_thresh = 0`` every row is high and this is the reference's SORT
output for output.

``last`` holds the regime of the last update (from this restatement alone):
T, D_high, D_low, cnt1 / cnt2 (pairs at or above the threshold in the stage's
sub-matrix), n_match1, n_match2, n_dropped, n_new.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from oracle import sort_ref
from oracle.sort_ref import _Track, greedy, iou_matrix, x_to_bbox

SECOND_IOU = 0.5


def is_high(conf, high: float) -> bool:
    return bool(np.float64(np.float32(conf)) >= np.float64(high))


class ByteSortTracker(sort_ref.SortTracker):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.track_high_thresh = float(cfg.get("track_high_thresh", 0.0))
        self.last: dict = {}

    def _stage(self, tb, db, ti: List[int], di: List[int], thr: float, key: str):
        """greedy on the (ti x di) sub-matrix -> [(track, det)] in full indices."""
        self.last[key] = 0
        if not ti or not di:
            return []
        m = iou_matrix(tb[ti], db[di])
        self.last[key] = int((m.astype(np.float64) >= thr).sum())
        matches, _, _ = greedy(m, thr)
        return [(ti[a], di[b]) for a, b in matches]

    def update(self, dets: Sequence[sort_ref.Det], ts: float, proj=None):
        dets = list(dets)
        for d in dets:
            d.track_id = d.distance_m = d.speed_kmh = None
        T0 = len(self.tracks)
        was_tracked = [t.hit_streak > 0 for t in self.tracks]
        for t in self.tracks:
            t.predict(ts)
        high = [i for i, d in enumerate(dets) if is_high(d.conf, self.track_high_thresh)]
        low = [i for i in range(len(dets)) if i not in set(high)]
        self.last = {"T": T0, "D_high": len(high), "D_low": len(low)}
        tb = np.array([x_to_bbox(t.kf.x) for t in self.tracks], dtype=np.float32).reshape(-1, 4)
        db = np.array([[d.x1, d.y1, d.x2, d.y2] for d in dets], dtype=np.float32).reshape(-1, 4)
        m1 = self._stage(tb, db, list(range(T0)), high, self.iou_threshold, "cnt1")
        taken = {t for t, _ in m1}
        rest = [t for t in range(T0) if t not in taken and was_tracked[t]]
        m2 = self._stage(tb, db, rest, low, SECOND_IOU, "cnt2")
        matches = m1 + m2
        for ti, di in matches:
            t, d = self.tracks[ti], dets[di]
            bb = (d.x1, d.y1, d.x2, d.y2)
            t.update(bb, ts, d)
            if proj is not None:
                t.update_metrics(proj, bb, ts)
            d.track_id = t.id
            if t.current_distance is not None:
                d.distance_m = t.current_distance
            elif proj is not None:
                d.distance_m = proj.distance_for_bbox(bb)
            if t.current_speed is not None:
                d.speed_kmh = t.current_speed * 3.6
        matched_t = {t for t, _ in matches}
        matched_d = {d for _, d in matches}
        for ti in range(T0):
            if ti not in matched_t:
                self.tracks[ti].hit_streak = 0
        new = [i for i in high if i not in matched_d]
        for di in new:
            d = dets[di]
            bb = (d.x1, d.y1, d.x2, d.y2)
            t = _Track(self.next_id, bb, ts, self.min_hits, self.speed_window)
            t.class_id, t.confidence = d.cls_id, d.conf
            if proj is not None:
                t.update_metrics(proj, bb, ts)
                if t.current_distance is not None:
                    d.distance_m = t.current_distance
                if t.current_speed is not None:
                    d.speed_kmh = t.current_speed * 3.6
            d.track_id = t.id
            self.tracks.append(t)
            self.next_id += 1
        self.tracks = [t for t in self.tracks if float(ts) - t.last_update_ts <= self.max_staleness]
        kept = [i for i in range(len(dets)) if i in set(high) or i in matched_d]
        self.last.update(n_match1=len(m1), n_match2=len(m2), n_new=len(new),
                         n_dropped=len(dets) - len(kept), kept=kept)
        return [dets[i] for i in kept]

"""The named inputs of the SORT path tests (test_sort_cases_cpu.py,
test_sort_paths_gpu.py): every case is one batched launch -- the streams that
share a config, a projector and the pool sizes -- with the oracle's answer
(oracle/sort_ref.SortTracker, one per stream, computed once) and, from the
oracle alone, the regime every frame ran in: (T, D, cnt) as _associate saw
them (cnt = pairs with IoU >= thr, which picks the kernel's rank sort, bitonic
sort or argmax loop), the longest speed history, and whether the clamps and
the negative predicted area were reached.  test_sort_cases_cpu.py asserts the
regimes, so the GPU tests cannot silently run another path than the one a case
is named for."""
import functools
import math
import os
from typing import List, NamedTuple, Optional

import numpy as np

from conftest import GOLDEN
from oracle import sort_ref
from oracle.sort_ref import synthetic_detections

G = np.load(os.path.join(GOLDEN, "reference_sort.npz"), allow_pickle=False)
CFG = {"max_staleness": 1.2, "min_hits": 3, "iou_threshold": 0.35, "speed_window": 0.8}
GOLDEN_PROJ = (np.asarray(G["proj/H"], np.float64).reshape(3, 3),
               tuple(float(x) for x in G["proj/origin"]), float(G["proj/max_distance"]))
# w = y2 - 500: the projection of a box whose (integer) y2 is 500 is None
PARTIAL_PROJ = (np.array([[0.05, 0.0, -40.0], [0.0, 0.1, 10.0], [0.0, 1.0, -500.0]]),
                (0.0, 0.0), None)


# A speed is hypot(X1 - X0, Y1 - Y0) / dt over ground coordinates that numpy
# (a BLAS matrix-vector product, fused or not by the CPU it runs on) and the
# kernel (plain left-to-right f64) round differently: on the golden projector
# the two disagree by an ulp on a quarter of all points.  Two ulps on either
# end of a displacement of r times the coordinates are 4 * 1.1e-16 / r of the
# speed, so the rtol 1e-12 bar on speed_kmh means something only for r above
# 4.4e-4.  Every speed of every case stays above this (checked on the oracle).
MIN_REL_DISP = 5e-4


class Stream(NamedTuple):
    name: str
    frames: List[np.ndarray]  # per frame the (n, 6) f32 rows handed to the device
    ts: List[float]
    dcount: Optional[List[int]] = None  # per frame the count handed to the device (None: n)


class Case(NamedTuple):
    name: str
    cfg: dict
    proj: Optional[tuple]  # (H, origin, max_distance)
    tmax: int
    dmax: int
    streams: List[Stream]
    overflow: bool = False  # the case is about new tracks that find no free slot


def device_count(case, st, f):
    """The dcount entry the device gets for frame f of a stream."""
    return len(st.frames[f]) if st.dcount is None else int(st.dcount[f])


def rows_used(case, st, f):
    """The rows the tracker is to see: the device clamps dcount to [0, dmax]."""
    return st.frames[f][:min(max(device_count(case, st, f), 0), case.dmax)]


def oracle_projector(spec):
    return None if spec is None else sort_ref.HomographyProjector(spec[0], spec[1], spec[2])


def device_projector(spec):
    from rvs_amd.geometry import HomographyProjector
    return None if spec is None else HomographyProjector.from_matrix(spec[0], spec[1], spec[2])


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def _rows(boxes, conf=0.8, cls=2):
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return np.concatenate([b, np.full((len(b), 1), conf), np.full((len(b), 1), cls)],
                          1).astype(np.float32)


def _trim(frames, n):
    """At most n(f) rows per frame (n: an int or a function of the frame)."""
    return [fr[:(n(f) if callable(n) else n)] for f, fr in enumerate(frames)]


def crowd(n, seed, nf=30, fps=30.0, region=260.0):
    """n boxes of 140-180 px drifting (and bouncing) with their centres inside
    a `region` px square, jitter sigma 1 px: most pairs overlap.  The region
    itself moves (6, 2) px a frame, so no box ever stands still on the ground:
    a speed is a difference of ground coordinates, and one over a displacement
    of 1e-4 of the coordinates carries 1e4 times their rounding error."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, region, (n, 2))
    v = rng.uniform(-1.5, 1.5, (n, 2))
    wh = rng.uniform(140.0, 180.0, (n, 2))
    cls = rng.choice([0, 2, 3, 5, 7], n)
    frames, ts = [], []
    for f in range(nf):
        j = rng.normal(0.0, 1.0, (n, 2))
        p = c + j + 500.0 + np.array([6.0, 2.0]) * f
        rows = np.concatenate([p - wh / 2, p + wh / 2, rng.uniform(0.3, 0.95, (n, 1)),
                               cls[:, None]], 1)
        frames.append(rows[rng.permutation(n)].astype(np.float32))
        ts.append(f / fps)
        c += v
        v = np.where((c < 0.0) | (c > region), -v, v)
    return frames, ts


def _grid(n, x0, y0, cols, dx=100.0, dy=100.0, w=40.0, h=40.0):
    k = np.arange(n)
    x, y = x0 + dx * (k % cols), y0 + dy * (k // cols)
    return np.stack([x, y, x + w, y + h], 1)


BOUNDARY_TD = [(16, 32), (19, 27), (32, 32), (25, 41)]  # cnt 512, 513, 1024, 1025


def boundary_stream(T, D, seed):
    """Frame 0: T boxes that do not overlap.  Frames 1, 2: D boxes, about
    two thirds of min(T, D) of them on tracks (moved 2 px a frame), the rest
    elsewhere.  With thr = 0 every pair qualifies: cnt = T * D in frame 1."""
    rng = np.random.default_rng(seed)
    on = (2 * min(T, D)) // 3
    trk = _grid(T, 50.0, 50.0, 8)
    frames = [_rows(trk[rng.permutation(T)])]
    pick = rng.permutation(T)[:on]
    away = _grid(D - on, 1000.0, 60.0, 8)
    order = rng.permutation(D)
    for f in (1, 2):
        b = np.concatenate([trk[pick] + 2.0 * f, away + 3.0 * f])
        frames.append(_rows(b[order], conf=0.6, cls=7))
    return frames, [0.0, 1 / 30, 2 / 30]


def grid_stream(n=530, nf=4, cols=27, seed=3):
    """n boxes on a grid that never overlap, all drifting 1.5 px a frame; the
    rows in another order every frame."""
    rng = np.random.default_rng(seed)
    base = _grid(n, 20.0, 20.0, cols, dx=60.0, dy=50.0, w=40.0, h=30.0)
    frames = []
    for f in range(nf):
        b = base + np.array([1.5 * f, 0.0, 1.5 * f, 0.0])
        frames.append(_rows(b[rng.permutation(n)]))
    return frames, [f / 30.0 for f in range(nf)]


def degenerate_stream(nf=40, seed=31):
    """A normal stream plus, in every frame, a zero-area box (x1 == x2), one
    with x2 < x1, one with y2 < y1 and a 1e-4 px wide sliver: two of them
    sit on the first object of the frame, two stay where they are."""
    frames, ts = synthetic_detections(nf, seed=seed, n_obj=8, p_clutter=1.0)
    rng = np.random.default_rng(seed)
    out = []
    for fr in frames:
        x1, y1, x2, y2 = (fr[0, :4] if len(fr) else (300., 300., 400., 380.))
        extra = _rows([[x1 + 10, y1, x1 + 10, y2],          # zero area, on an object
                       [x2, y1, x1, y2],                    # x2 < x1, on an object
                       [700.0, 420.0, 760.0, 380.0],        # y2 < y1
                       [128.0, 640.0, 128.0 + 1e-4, 700.0]],  # sliver
                      conf=0.4, cls=0)
        rows = np.concatenate([fr, extra])
        out.append(rows[rng.permutation(len(rows))])
    return out, ts


def shrinking_stream(nf=40, seed=32):
    """Four normal objects and one whose box shrinks from 200 px to 4 px
    over ten frames and is then gone: its track keeps predicting with the
    learnt negative area rate while it is stale, and s + dt * ds < 0."""
    frames, ts = synthetic_detections(nf, seed=seed, n_obj=4, p_miss=0.0, p_clutter=0.0)
    out = []
    for f, fr in enumerate(frames):
        if f < 10:
            half = 0.5 * (200.0 - 196.0 * f / 9.0)
            fr = np.concatenate([fr, _rows([[1500.0 - half, 300.0 - half, 1500.0 + half,
                                             300.0 + half]], conf=0.7, cls=5)])
        out.append(fr)
    return out, ts


def duplicate_stream(nf=40, seed=33):
    """Every frame repeats three of its rows verbatim: the IoU of a track
    with a row and with its copy are the same bits on both sides, so the flat
    index decides."""
    frames, ts = synthetic_detections(nf, seed=seed, n_obj=10, p_miss=0.0, p_clutter=1.0)
    rng = np.random.default_rng(seed)
    out = []
    for fr in frames:
        rows = np.concatenate([fr, fr[:3]])
        out.append(rows[rng.permutation(len(rows))])
    return out, ts


def crossing_stream(nf=30):
    """Integer boxes moving down 2 px a frame through y2 == 500 at different
    frames (PARTIAL_PROJ: None exactly there)."""
    frames = []
    for f in range(nf):
        b = []
        for k in range(6):
            x1 = 100.0 + 220.0 * k
            y2 = 470.0 + 6.0 * k + 2.0 * f  # == 500 at f = 15 - 3k
            b.append([x1, y2 - 90.0, x1 + 120.0, y2])
        frames.append(_rows(b, conf=0.9, cls=2))
    return frames, [f / 30.0 for f in range(nf)]


def _synth_stream(name, nf, dcount=None, trim=None, ts_edit=None, **kw):
    frames, ts = synthetic_detections(nf, **kw)
    if trim is not None:
        frames = _trim(frames, trim)
    if ts_edit is not None:
        ts = ts_edit(list(ts))
    return Stream(name, frames, [float(t) for t in ts], dcount)


def _equal_ts(ts):
    for f in range(2, len(ts), 3):
        ts[f] = ts[f - 1]
    return ts


def _backward_ts(ts):
    for f in (15, 30):
        ts[f] = ts[f - 1] - 0.05
    return ts


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case."""
    # the seeds that this file chooses were chosen on the oracle alone, for
    # the regime counts and MIN_REL_DISP (test_sort_cases_cpu.py)
    out = []

    def add(name, streams, cfg=None, proj=GOLDEN_PROJ, tmax=128, dmax=32, overflow=False):
        for st in streams:
            assert all(len(fr) <= dmax for fr in st.frames), (name, st.name)
        out.append(Case(name, dict(CFG, **(cfg or {})), proj, tmax, dmax, list(streams), overflow))

    add("bitonic_thr0",
        [_synth_stream("n27", 40, seed=1, n_obj=27, p_miss=0.05, p_clutter=0.0)],
        cfg={"iou_threshold": 0.0}, tmax=64, dmax=32)
    add("bitonic_crowd",
        [Stream("n40", *crowd(40, seed=11)), Stream("n30", *crowd(30, seed=12, region=200.0))],
        cfg={"iou_threshold": 0.05}, tmax=128, dmax=48)
    add("cnt_boundaries",
        [Stream(f"{T}x{D}", *boundary_stream(T, D, seed=40 + k))
         for k, (T, D) in enumerate(BOUNDARY_TD)],
        cfg={"iou_threshold": 0.0}, tmax=64, dmax=48)
    add("hist_cap",
        [_synth_stream("fps120", 70, seed=5, n_obj=10, fps=120.0, p_clutter=1.0)])
    add("hist_window_clamp",
        [_synth_stream("fps120", 70, seed=5, n_obj=10, fps=120.0, p_clutter=1.0)],
        cfg={"speed_window": 0.01})
    nd = 128
    add("update_forms",
        [_synth_stream("le64", 40, seed=61, n_obj=40, p_clutter=2.0),
         _synth_stream("ge65", 40, seed=67, n_obj=90, p_miss=0.05, p_clutter=2.0),
         _synth_stream("64_65", 40, seed=71, n_obj=90, p_miss=0.05, p_clutter=2.0,
                       trim=lambda f: 65 if f % 3 == 1 else 64),
         _synth_stream("full", 40, seed=74, n_obj=135, p_miss=0.0, p_clutter=1.0, trim=nd,
                       dcount=[-3 if f == 20 else nd + 7 for f in range(40)])],
        tmax=1024, dmax=nd)
    add("many_tracks", [Stream("grid530", *grid_stream())], tmax=1024, dmax=576)
    add("odd_pool", [_synth_stream("n5", 80, seed=7, n_obj=5, p_clutter=1.0, trim=7)],
        tmax=100, dmax=7)
    add("time_equal_backward",
        [_synth_stream("equal", 45, seed=21, n_obj=12, ts_edit=_equal_ts),
         _synth_stream("backward", 45, seed=22, n_obj=12, ts_edit=_backward_ts)])
    add("stale_zero", [_synth_stream("ms0", 30, seed=27, n_obj=12, ts_edit=_equal_ts)],
        cfg={"max_staleness": 0.0})
    add("stale_negative", [_synth_stream("ms-1", 12, seed=24, n_obj=6)],
        cfg={"max_staleness": -1.0})
    # one frame of 7 boxes into a pool of 4: the three tracks without a slot
    # still report their ids and distances (the frame after would diverge: the
    # reference's list has no capacity)
    add("no_room", [Stream("7into4", [_rows(_grid(7, 300.0, 400.0, 4, dx=150.0))], [0.0])],
        tmax=4, dmax=8, overflow=True)
    add("box_edges",
        [Stream("degenerate", *degenerate_stream()), Stream("shrinking", *shrinking_stream()),
         Stream("duplicates", *duplicate_stream())], tmax=256, dmax=32)
    add("partial_projector", [Stream("crossing", *crossing_stream())], proj=PARTIAL_PROJ,
        tmax=64, dmax=8)
    return {c.name: c for c in out}


# ---------------------------------------------------------------------------
# the oracle's answer and the regimes
# ---------------------------------------------------------------------------
class Frame(NamedTuple):
    ids: np.ndarray    # -1 = None
    dist: np.ndarray   # NaN = None
    speed: np.ndarray  # NaN = None
    T: int             # len(tracks) after the frame
    next_id: int
    regime: dict       # T0, D, cnt, max_hist, n_speed, min_s_pred, n_dt_clamp


class Answer(NamedTuple):
    frames: List[Frame]
    x: np.ndarray     # (T, 7) final kf.x
    meta: np.ndarray  # (T, 4) id, hits, hit_streak, class_id


def _run_oracle(case, st):
    seen = {}
    greedy0, predict0 = sort_ref.greedy, sort_ref._Track.predict

    def greedy(m, thr):
        seen["cnt"] = int((m.astype(np.float64) >= thr).sum())
        seen["TD"] = m.shape
        return greedy0(m, thr)

    def predict(self, ts):
        box = predict0(self, ts)
        seen["min_s"] = min(seen.get("min_s", np.inf), float(self.kf.x[2, 0]))
        return box

    proj = oracle_projector(case.proj)
    tr = sort_ref.SortTracker(case.cfg)
    frames = []
    sort_ref.greedy, sort_ref._Track.predict = greedy, predict
    try:
        for f in range(len(st.frames)):
            seen.clear()
            rows, ts = rows_used(case, st, f), float(st.ts[f])
            T0 = len(tr.tracks)
            res = tr.update([sort_ref.Det(*map(float, r[:5]), int(r[5])) for r in rows], ts, proj)
            assert seen.get("TD", (T0, len(rows))) == (T0, len(rows))
            ids = np.array([-1 if d.track_id is None else d.track_id for d in res], np.int32)
            dist = np.array([np.nan if d.distance_m is None else d.distance_m for d in res],
                            np.float64)
            spd = np.array([np.nan if d.speed_kmh is None else d.speed_kmh for d in res],
                           np.float64)
            moved = [t for t in tr.tracks
                     if t.last_update_ts == ts and t.current_speed is not None]
            regime = {
                # the smallest ground displacement behind a speed of this frame,
                # relative to the ground coordinates it is the difference of
                "min_rel_disp": min(
                    [math.hypot(t.hist[-1][1] - t.hist[0][1], t.hist[-1][2] - t.hist[0][2]) /
                     max(map(abs, t.hist[0][1:] + t.hist[-1][1:])) for t in moved],
                    default=np.inf),
                "T0": T0, "D": len(rows), "cnt": seen.get("cnt", 0),
                "max_hist": max([len(t.hist) for t in tr.tracks], default=0),
                "n_speed": int((~np.isnan(spd)).sum()),
                "min_s_pred": seen.get("min_s", np.inf),
                # speeds of this frame whose t1 - t0 fell under the 1e-3 clamp
                "n_dt_clamp": sum(1 for t in moved if t.hist[-1][0] - t.hist[0][0] < 1e-3),
            }
            frames.append(Frame(ids, dist, spd, len(tr.tracks), tr.next_id, regime))
    finally:
        sort_ref.greedy, sort_ref._Track.predict = greedy0, predict0
    x = np.array([t.kf.x.reshape(-1) for t in tr.tracks], np.float64).reshape(-1, 7)
    meta = np.array([[t.id, t.hits, t.hit_streak, t.class_id] for t in tr.tracks],
                    np.int32).reshape(-1, 4)
    return Answer(frames, x, meta)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """One Answer per stream of the case.  Computed once per process."""
    case = cases()[name]
    return [_run_oracle(case, st) for st in case.streams]


def regimes(name, s, key, first=0):
    return [fr.regime[key] for fr in oracle(name)[s].frames[first:]]


# ---------------------------------------------------------------------------
# the device's side (used by the GPU tests only)
# ---------------------------------------------------------------------------
def batch(case, f):
    """Frame f of every stream as the device entries take it: dets (S, dmax,
    6) f32, counts (S,) i32, ts (S,) f64."""
    S = len(case.streams)
    dets = np.zeros((S, case.dmax, 6), np.float32)
    cnt = np.zeros(S, np.int32)
    ts = np.zeros(S, np.float64)
    for s, st in enumerate(case.streams):
        r = st.frames[f]
        dets[s, :len(r)] = r
        cnt[s] = device_count(case, st, f)
        ts[s] = st.ts[f]
    return dets, cnt, ts


def compare_frame(name, f, ids, dist, speed):
    """The device's (S, dmax) outputs of frame f against the oracle, at
    tests/test_sort_gpu.py's bars: ids exact, distance exact with its None
    pattern, speed rtol 1e-12 with its None pattern; rows [D, dmax) empty."""
    case = cases()[name]
    for s, st in enumerate(case.streams):
        ref = oracle(name)[s].frames[f]
        n = len(ref.ids)
        msg = f"{name}/{st.name} frame {f}"
        np.testing.assert_array_equal(ids[s, :n], ref.ids, err_msg=msg)
        np.testing.assert_array_equal(np.isnan(dist[s, :n]), np.isnan(ref.dist), err_msg=msg)
        np.testing.assert_array_equal(dist[s, :n], ref.dist, err_msg=msg)
        np.testing.assert_array_equal(np.isnan(speed[s, :n]), np.isnan(ref.speed), err_msg=msg)
        np.testing.assert_allclose(speed[s, :n], ref.speed, rtol=1e-12, equal_nan=True,
                                   err_msg=msg)
        assert (ids[s, n:] == -1).all() and np.isnan(dist[s, n:]).all() and \
            np.isnan(speed[s, n:]).all(), msg


def compare_final(name, export, stats):
    """export() / stats() after the last frame: x at rtol = atol = 1e-9; id,
    hits, streak, cls, T and next_id exact; the overflow flag 0 -- or, in a
    case about overflow (its only frame overflows), 1 with the pool holding
    the first tmax tracks of the oracle's list."""
    case = cases()[name]
    T, x, meta = export
    for s, st in enumerate(case.streams):
        ans = oracle(name)[s]
        msg = f"{name}/{st.name}"
        n = len(ans.meta)
        assert n == ans.frames[-1].T, msg
        if case.overflow:
            assert n > case.tmax and len(ans.frames) == 1, msg
            n = case.tmax
        assert int(T[s]) == n and int(stats["T"][s]) == n, msg
        assert int(stats["next_id"][s]) == ans.frames[-1].next_id, msg
        assert bool(stats["overflow"][s]) == case.overflow, msg
        np.testing.assert_array_equal(meta[s, :n], ans.meta[:n], err_msg=msg)
        assert (meta[s, n:, 0] == -1).all(), msg
        np.testing.assert_allclose(x[s, :n], ans.x[:n], rtol=1e-9, atol=1e-9, err_msg=msg)

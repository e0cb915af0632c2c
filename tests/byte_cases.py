"""The named inputs of the BYTE path tests (test_byte_cases_cpu.py,
test_byte_paths_gpu.py), in the style of tests/sort_cases.py: every case is
one batched launch -- the streams that share a config and the pool sizes --
with the reference's answer (tests/byte_ref.ByteSortTracker, one per stream,
computed once) and, from the reference alone, the regime of every frame: T,
D_high, D_low, the stage-1 and stage-2 qualifying pair counts (which pick the
kernel's rank sort, bitonic sort or argmax loop in each stage) and the counts
of stage-2 matches, dropped rows and new tracks.  test_byte_cases_cpu.py
asserts the regimes, so the GPU tests cannot silently run another path than
the one a case is named for.

The fused kernel runs 512 threads: its rank sort takes up to 512 pairs, the
bitonic sort up to 1024, the argmax loop the rest.  The sorter cases stay at
or under 256, in 513..1024 and above 1024, so they also hold for a 256-thread
build."""
import functools
import math
from typing import List, NamedTuple, Optional

import numpy as np

import sort_cases as sc
from byte_ref import ByteSortTracker
from oracle import sort_ref
from sort_cases import GOLDEN_PROJ, MIN_REL_DISP, Stream

CFG = {"max_staleness": 1.2, "min_hits": 3, "iou_threshold": 0.35, "speed_window": 0.8,
       "track_high_thresh": 0.5, "track_low_thresh": 0.1}
DT = 0.2  # seconds a frame: seven missed frames are longer than max_staleness
ALL_HIGH_THRESH = 0.2  # under every conf of tests/sort_cases.py (the smallest is 0.26)


class Case(NamedTuple):
    name: str
    cfg: dict
    proj: Optional[tuple]          # one (H, origin, max_distance) for every stream
    projs: Optional[list]          # or one per camera stream (None entries: disabled)
    tmax: int
    dmax: int
    streams: List[Stream]
    overflow: bool = False         # the last frame brings more new tracks than free slots


def stream_proj(case, s):
    return case.projs[s] if case.projs is not None else case.proj


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def sq(x, y, a=64.0):
    """A square box: a track made from it predicts exactly this box while its
    velocity is zero (s = a * a, r = 1: sqrt and quotient are exact)."""
    return [x, y, x + a, y + a]


def rows(items):
    """[(box, conf, cls)] -> (n, 6) f32."""
    return np.array([list(b) + [c, k] for b, c, k in items], np.float32).reshape(-1, 6)


def _ts(n):
    return [DT * f for f in range(n)]


def _pad(frames, n):
    return frames + [rows([])] * (n - len(frames))


def below(x):
    """The f32 one ulp under f32(x)."""
    return float(np.nextafter(np.float32(x), np.float32(0)))


def fade_stream(lo_frames=8, x0=600.0, y0=520.0, v=(14.0, 6.0), lo_to=0.15):
    """One object moving v px a frame whose score decays 0.8 -> lo_to over
    lo_frames frames (longer than max_staleness) and recovers, beside one
    that is always high."""
    confs = [0.8, 0.8, 0.8] + list(np.linspace(0.45, lo_to, lo_frames)) + [0.8, 0.8, 0.8]
    frames = []
    for f, c in enumerate(confs):
        a = [x0 + v[0] * f, y0 + v[1] * f, x0 + 120.0 + v[0] * f, y0 + 90.0 + v[1] * f]
        b = [1300.0 - 11.0 * f, 700.0 + 5.0 * f, 1440.0 - 11.0 * f, 800.0 + 5.0 * f]
        frames.append(rows([(a, c, 2), (b, 0.9, 7)]))
    return frames, _ts(len(frames))


def compaction_stream():
    """Frame 1: low-dropped, high-matched, low-matched, high-unmatched (new),
    low-matched, high-matched, low-dropped -- the first and the last row are
    dropped."""
    pos = [(100.0, 100.0), (400.0, 100.0), (700.0, 100.0), (1000.0, 100.0)]
    f0 = rows([(sq(x, y), 0.9, 2) for x, y in pos])
    f1 = rows([(sq(100.0, 600.0), 0.3, 0), (sq(102.0, 101.0), 0.7, 2), (sq(401.0, 99.0), 0.2, 3),
               (sq(1300.0, 500.0), 0.6, 5), (sq(699.0, 102.0), 0.45, 7),
               (sq(1001.0, 101.0), 0.95, 2), (sq(1500.0, 800.0), 0.11, 0)])
    f2 = rows([(sq(1302.0, 501.0), 0.4, 5), (sq(300.0, 900.0), 0.49, 0),
               (sq(104.0, 102.0), 0.3, 2), (sq(1003.0, 102.0), 0.5, 2)])
    return [f0, f1, f2], _ts(3)


def stage_order_stream():
    """Frame 1: a low row exactly on the track (IoU 1) before a high row
    shifted 16 px (IoU 0.6): stage 1 gives the track to the high row."""
    f0 = rows([(sq(200.0, 200.0), 0.9, 2)])
    f1 = rows([(sq(200.0, 200.0), 0.3, 2), (sq(216.0, 200.0), 0.8, 2)])
    f2 = rows([(sq(216.0, 200.0), 0.3, 2)])
    return [f0, f1, f2], _ts(3)


def eligibility_stream():
    """A, B at frame 0.  Frame 1: A only (B misses: streak 0) and a new C.
    Frame 2: low rows on B (not eligible: dropped) and on C (created the
    frame before: taken), high on A.  Frame 3: a high row on B (taken)."""
    A, B, C = sq(100.0, 100.0), sq(500.0, 100.0), sq(900.0, 100.0)
    f0 = rows([(A, 0.9, 2), (B, 0.9, 2)])
    f1 = rows([(A, 0.9, 2), (C, 0.9, 7)])
    f2 = rows([(B, 0.4, 2), (C, 0.4, 7), (A, 0.9, 2)])
    f3 = rows([(B, 0.9, 2), (A, 0.3, 2)])
    return [f0, f1, f2, f3], _ts(4)


def edge_stream(high):
    """Scores at, one f32 ulp under and one over f32(high) on free ground (new
    track or dropped); stage-2 IoU exactly 0.5 (the 3:1 pair of
    tests/nms_cases.py, on squares) and one f32 ulp under it (a 64 x (32 -
    2^-19) box inside the 64 x 64 track: inter / union = (2048 - 2^-13) /
    4096 in f32 and in f64)."""
    hi = float(np.float32(high))
    lo = min(0.9 * hi, below(hi))
    f0 = rows([(sq(0.0, 0.0), 0.9, 2), (sq(1000.0, 0.0, 96.0), 0.9, 2), (sq(300.0, 600.0), 0.9, 2)])
    h_under = float(np.float32(32.0) - np.float32(2.0 ** -19))
    f1 = rows([([0.0, 0.0, 64.0, h_under], lo, 2),                 # IoU 0.5 - ulp: dropped
               ([1032.0, 0.0, 1128.0, 96.0], lo, 2),               # IoU 0.5 exactly: matched
               (sq(100.0, 300.0), hi, 3),                          # conf == f32(high)
               (sq(400.0, 300.0), below(hi), 3),                   # one ulp under
               (sq(700.0, 300.0), float(np.nextafter(np.float32(hi), np.float32(1))), 3),
               (sq(301.0, 601.0), below(hi), 5)])                  # one ulp under, on a track
    return [f0, f1], _ts(2)


def ties_stream():
    """Frame 1, low rows only: one row at IoU 0.6 to tracks A and B (A, the
    first in the list, takes it); two rows at IoU 0.6 to track C (the first
    row takes it)."""
    f0 = rows([(sq(0.0, 0.0), 0.9, 2), (sq(32.0, 0.0), 0.9, 2), (sq(500.0, 0.0), 0.9, 2)])
    f1 = rows([(sq(516.0, 0.0), 0.3, 2), (sq(16.0, 0.0), 0.3, 2), (sq(484.0, 0.0), 0.3, 2)])
    f2 = rows([(sq(16.0, 0.0), 0.3, 2), (sq(32.0, 0.0), 0.9, 2)])
    return [f0, f1, f2], _ts(3)


def cluster_stream(n_trk, n_high, n_low, n_high2=0):
    """Frame 0: n_trk coincident boxes (n_trk coincident tracks).  Frame 1:
    n_high coincident high rows and n_low coincident low rows on them, all
    pairs at IoU 1: cnt1 = n_trk * n_high, cnt2 = (n_trk - min(n_trk,
    n_high)) * n_low.  Frame 2: the same 3 px on."""
    b = sq(300.0, 300.0, 80.0)
    f0 = rows([(b, 0.9, 2)] * n_trk)
    out = [f0]
    for f in (1, 2):
        m = [v + 3.0 * f for v in b]
        fr = [(m, 0.3, 7)] * (n_low // 2) + [(m, 0.8, 2)] * n_high + \
             [(m, 0.3, 7)] * (n_low - n_low // 2)
        out.append(rows(fr))
    return out, _ts(3)


def empty_stream(dmax):
    """Frame 1: every row low and on free ground (kept count 0).  Frame 2: no
    rows.  Frame 3: dcount < 0.  Frame 4: dcount > dmax with dmax rows."""
    f0 = rows([(sq(100.0, 100.0), 0.9, 2), (sq(500.0, 100.0), 0.9, 2)])
    f1 = rows([(sq(100.0, 700.0), 0.3, 2), (sq(900.0, 700.0), 0.2, 2)])
    f2 = rows([])
    f3 = rows([(sq(100.0, 100.0), 0.9, 2), (sq(500.0, 100.0), 0.3, 2)])
    full = [(sq(100.0, 100.0), 0.3, 2), (sq(500.0, 100.0), 0.9, 2)] + \
           [(sq(60.0 + 110.0 * k, 500.0), 0.3 if k % 2 else 0.7, 3) for k in range(dmax - 2)]
    f4 = rows(full)
    return Stream("empty", [f0, f1, f2, f3, f4], _ts(5), [2, 2, 0, -3, dmax + 7])


def full_pool_stream():
    """tmax = 4, dmax = 6.  Frame 0: three tracks.  Frame 1 (D = dmax): one
    high and two low rows on them and three new high rows -- one slot is
    free: two new tracks are dropped, their ids consumed, the flag set."""
    pos = [(100.0, 100.0), (400.0, 100.0), (700.0, 100.0)]
    f0 = rows([(sq(x, y), 0.9, 2) for x, y in pos])
    f1 = rows([(sq(1000.0, 500.0), 0.9, 3), (sq(401.0, 100.0), 0.3, 2), (sq(1200.0, 500.0), 0.8, 3),
               (sq(101.0, 100.0), 0.9, 2), (sq(1400.0, 500.0), 0.7, 3), (sq(700.0, 101.0), 0.2, 2)])
    return [f0, f1], _ts(2)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case."""
    out = []

    def add(name, streams, cfg=None, proj=None, projs=None, tmax=64, dmax=16, overflow=False):
        n = len(streams[0].frames)
        for st in streams:
            assert len(st.frames) == n and all(len(fr) <= dmax for fr in st.frames), (name, st.name)
        assert len(streams) <= 5
        out.append(Case(name, dict(CFG, **(cfg or {})), proj, projs, tmax, dmax, list(streams),
                        overflow))

    add("fade_recover", [Stream("fade", *fade_stream())], proj=GOLDEN_PROJ)
    add("compaction", [Stream("interleaved", *compaction_stream())])
    add("stage_order", [Stream("low_first", *stage_order_stream())])
    add("eligibility", [Stream("abc", *eligibility_stream())])
    for high in (0.25, 0.5, 0.1):
        add(f"edges_{high}", [Stream("edges", *edge_stream(high))],
            cfg={"track_high_thresh": high, "track_low_thresh": 0.05}, tmax=16, dmax=8)
    add("ties", [Stream("ties", *ties_stream())])
    add("sorters_stage1",
        [Stream("rank_12x12", *cluster_stream(12, 12, 0)),
         Stream("bitonic_28x28", *cluster_stream(28, 28, 0)),
         Stream("argmax_36x36", *cluster_stream(36, 36, 0))], tmax=64, dmax=64)
    add("sorters_stage2",
        [Stream("rank_12x12", *cluster_stream(12, 0, 12)),
         Stream("bitonic_28x28", *cluster_stream(28, 0, 28)),
         Stream("argmax_36x36", *cluster_stream(36, 0, 36)),
         Stream("rank_then_argmax", *cluster_stream(40, 4, 36)),
         Stream("argmax_then_rank", *cluster_stream(44, 36, 8))], tmax=64, dmax=64)
    add("empty_results", [empty_stream(8)], tmax=16, dmax=8)
    add("full_pool", [Stream("6into4", *full_pool_stream())], tmax=4, dmax=6, overflow=True)
    fa, fb = fade_stream(), fade_stream(x0=500.0, y0=480.0, v=(-12.0, 7.0))
    add("per_camera", [Stream("cam_on", *fa), Stream("cam_off", *fb),
                       Stream("cam_on2", *fade_stream(lo_frames=8, x0=800.0, y0=560.0,
                                                      v=(10.0, -4.0), lo_to=0.2))],
        projs=[GOLDEN_PROJ, None, GOLDEN_PROJ])
    n = len(fa[0])
    add("mixed_batch",
        [Stream("fade", *fa),
         Stream("compaction", _pad(compaction_stream()[0], n), _ts(n)),
         Stream("eligibility", _pad(eligibility_stream()[0], n), _ts(n)),
         Stream("ties", _pad(ties_stream()[0], n), _ts(n)),
         Stream("cluster", _pad(cluster_stream(12, 4, 8)[0], n), _ts(n))],
        tmax=64, dmax=16)
    return {c.name: c for c in out}


# ---------------------------------------------------------------------------
# the reference's answer and the regimes
# ---------------------------------------------------------------------------
class Frame(NamedTuple):
    kept: np.ndarray   # (n, 6) f32: the kept rows, in input order
    ids: np.ndarray    # per kept row; -1 = None
    dist: np.ndarray   # NaN = None
    speed: np.ndarray  # NaN = None
    T: int             # len(tracks) after the frame
    next_id: int
    regime: dict       # ByteSortTracker.last + min_rel_disp, n_speed


class Answer(NamedTuple):
    frames: List[Frame]
    x: np.ndarray     # (T, 7) final kf.x
    meta: np.ndarray  # (T, 4) id, hits, hit_streak, class_id


def to_dets(r):
    return [sort_ref.Det(*map(float, x[:5]), int(x[5])) for x in r]


def run_reference(cfg, proj_spec, frames_rows, ts_list, tracker=ByteSortTracker):
    """frames_rows: per frame the (n, 6) rows the tracker sees -> Answer."""
    proj = sc.oracle_projector(proj_spec)
    tr = tracker(cfg)
    frames = []
    for r, ts in zip(frames_rows, ts_list):
        ts = float(ts)
        res = tr.update(to_dets(r), ts, proj)
        kept = np.array([[d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id] for d in res],
                        np.float32).reshape(-1, 6)
        ids = np.array([-1 if d.track_id is None else d.track_id for d in res], np.int32)
        dist = np.array([np.nan if d.distance_m is None else d.distance_m for d in res], np.float64)
        spd = np.array([np.nan if d.speed_kmh is None else d.speed_kmh for d in res], np.float64)
        moved = [t for t in tr.tracks if t.last_update_ts == ts and t.current_speed is not None]
        regime = dict(getattr(tr, "last", {}))
        regime["n_speed"] = int((~np.isnan(spd)).sum())
        regime["min_rel_disp"] = min(
            [math.hypot(t.hist[-1][1] - t.hist[0][1], t.hist[-1][2] - t.hist[0][2]) /
             max(map(abs, t.hist[0][1:] + t.hist[-1][1:])) for t in moved], default=np.inf)
        frames.append(Frame(kept, ids, dist, spd, len(tr.tracks), tr.next_id, regime))
    x = np.array([t.kf.x.reshape(-1) for t in tr.tracks], np.float64).reshape(-1, 7)
    meta = np.array([[t.id, t.hits, t.hit_streak, t.class_id] for t in tr.tracks],
                    np.int32).reshape(-1, 4)
    return Answer(frames, x, meta)


@functools.lru_cache(maxsize=None)
def reference(name):
    """One Answer per stream of the case.  Computed once per process."""
    case = cases()[name]
    return [run_reference(case.cfg, stream_proj(case, s),
                          [sc.rows_used(case, st, f) for f in range(len(st.frames))], st.ts)
            for s, st in enumerate(case.streams)]


def regimes(name, s, key):
    return [fr.regime[key] for fr in reference(name)[s].frames]


# ---------------------------------------------------------------------------
# the device's side (used by the GPU tests only)
# ---------------------------------------------------------------------------
batch = sc.batch  # frame f of every stream as the device entries take it


def compare_frame(name, f, kept, kept_n, ids, dist, speed):
    """The device's kept rows (S, dmax, 6), counts (S,) and (S, dmax) outputs
    of frame f against the reference: kept rows bit for bit, count and ids
    exact, the tails zero / -1 / NaN; distance exact with its None pattern,
    speed rtol 1e-12 with its None pattern (tests/test_sort_paths_gpu.py's
    bars)."""
    case = cases()[name]
    for s, st in enumerate(case.streams):
        ref = reference(name)[s].frames[f]
        n = len(ref.ids)
        msg = f"{name}/{st.name} frame {f}"
        assert int(kept_n[s]) == n, msg
        assert kept[s, :n].tobytes() == ref.kept.tobytes(), msg
        assert not kept[s, n:].any(), msg
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
    case about overflow (its last frame overflows), 1 with the pool holding
    the first tmax tracks of the reference's list."""
    case = cases()[name]
    T, x, meta = export
    for s, st in enumerate(case.streams):
        ans = reference(name)[s]
        msg = f"{name}/{st.name}"
        n = len(ans.meta)
        assert n == ans.frames[-1].T, msg
        if case.overflow:
            assert n > case.tmax, msg
            n = case.tmax
        assert int(T[s]) == n and int(stats["T"][s]) == n, msg
        assert int(stats["next_id"][s]) == ans.frames[-1].next_id, msg
        assert bool(stats["overflow"][s]) == case.overflow, msg
        np.testing.assert_array_equal(meta[s, :n], ans.meta[:n], err_msg=msg)
        assert (meta[s, n:, 0] == -1).all(), msg
        np.testing.assert_allclose(x[s, :n], ans.x[:n], rtol=1e-9, atol=1e-9, err_msg=msg)

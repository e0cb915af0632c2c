"""The common input of the per-camera projector tests (test_cams_cpu.py,
test_cams_gpu.py): 5 camera streams x 12 frames of synthetic detections,
five different ground calibrations of which two change mid-run, and the
oracle's answer -- oracle/sort_ref.SortTracker run once per stream with that
stream's projector passed per call, as the reference does
(src/track/sort_tracker.py:212-278)."""
import functools
import os

import numpy as np

from conftest import GOLDEN
from oracle import sort_ref

G = np.load(os.path.join(GOLDEN, "reference_sort.npz"), allow_pickle=False)
CFG = {"max_staleness": 1.2, "min_hits": 3, "iou_threshold": 0.35, "speed_window": 0.8}
S, NF, DMAX, TMAX = 5, 12, 16, 64
H0 = np.asarray(G["proj/H"], np.float64).reshape(3, 3)
ORIGIN0 = tuple(float(x) for x in G["proj/origin"])
CAP0 = float(G["proj/max_distance"])
A = np.array([[0.9, 0.05, 3.0], [-0.02, 1.1, -7.0], [1e-5, 2e-4, 1.0]])

# (H, origin, max_distance) or None
CAMS = [
    (H0, ORIGIN0, CAP0),
    None,
    (A @ H0, (5.0, -2.0), None),
    (H0, (0.0, 0.0), 12.5),
    (np.diag([1.0, 1.0, 0.0]), (0.0, 0.0), None),  # w = 0: every projection is None
]
# frame -> {camera: new spec}: applied before that frame's update
CHANGES = {6: {2: (H0, (1.0, 1.0), 30.0)}, 8: {0: None}}


def cams_at(frame):
    """The five camera specs in force at `frame`."""
    cams = list(CAMS)
    for f in sorted(CHANGES):
        if f <= frame:
            for s, spec in CHANGES[f].items():
                cams[s] = spec
    return cams


def oracle_projector(spec):
    return None if spec is None else sort_ref.HomographyProjector(spec[0], spec[1], spec[2])


def device_projector(spec):
    from rvs_amd.geometry import HomographyProjector
    return None if spec is None else HomographyProjector.from_matrix(spec[0], spec[1], spec[2])


@functools.lru_cache(maxsize=None)
def streams():
    """Per stream (frames, ts) of sort_ref.synthetic_detections."""
    out = [sort_ref.synthetic_detections(NF, seed=500 + s, n_obj=6, p_clutter=1.0)
           for s in range(S)]
    assert max(len(fr) for st in out for fr in st[0]) <= 10
    return out


def batch(f):
    """Frame f of every stream as the device entries take it: dets (S, DMAX,
    6) f32, counts (S,) i32, ts (S,) f64."""
    dets = np.zeros((S, DMAX, 6), np.float32)
    cnt = np.zeros(S, np.int32)
    ts = np.zeros(S, np.float64)
    for s, (frames, t) in enumerate(streams()):
        r = frames[f]
        dets[s, :len(r)] = r
        cnt[s] = len(r)
        ts[s] = t[f]
    return dets, cnt, ts


@functools.lru_cache(maxsize=None)
def oracle():
    """out[s][f] = (ids, dist, speed) arrays of stream s, frame f (-1 / NaN =
    None), from one sort_ref.SortTracker per stream.  Computed once."""
    out = []
    for s, (frames, ts) in enumerate(streams()):
        tr = sort_ref.SortTracker(CFG)
        rows = []
        for f in range(NF):
            proj = oracle_projector(cams_at(f)[s])
            dets = [sort_ref.Det(*map(float, r[:5]), int(r[5])) for r in frames[f]]
            res = tr.update(dets, float(ts[f]), proj)
            rows.append((
                np.array([-1 if d.track_id is None else d.track_id for d in res], np.int32),
                np.array([np.nan if d.distance_m is None else d.distance_m for d in res],
                         np.float64),
                np.array([np.nan if d.speed_kmh is None else d.speed_kmh for d in res],
                         np.float64)))
        out.append(rows)
    return out


def check_non_vacuous():
    """The oracle's side of the comparison exercises what the cameras are
    there for (the counts the common input was chosen for)."""
    ora = oracle()
    for s in (0, 2, 3):
        nd = sum(int((~np.isnan(r[1])).sum()) for r in ora[s])
        ns = sum(int((~np.isnan(r[2])).sum()) for r in ora[s])
        assert nd >= 50 and ns >= 40, (s, nd, ns)
    # camera 0 after its projector was removed: matched tracks keep reporting
    assert sum(int((~np.isnan(r[1])).sum()) for r in ora[0][8:]) >= 10
    assert sum(int((r[1] == 12.5).sum()) for r in ora[3]) >= 10
    for s in (1, 4):
        assert all(np.isnan(r[1]).all() and np.isnan(r[2]).all() for r in ora[s])


def compare(got, s, f):
    """got = (ids, dist, speed) of stream s, frame f against the oracle, at
    tests/test_sort_gpu.py's bars: ids exact, distance exact with its None
    pattern, speed rtol 1e-12 with its None pattern."""
    ids, dist, spd = oracle()[s][f]
    msg = f"stream {s} frame {f}"
    np.testing.assert_array_equal(got[0], ids, err_msg=msg)
    np.testing.assert_array_equal(np.isnan(got[1]), np.isnan(dist), err_msg=msg)
    np.testing.assert_array_equal(got[1], dist, err_msg=msg)
    np.testing.assert_array_equal(np.isnan(got[2]), np.isnan(spd), err_msg=msg)
    np.testing.assert_allclose(got[2], spd, rtol=1e-12, equal_nan=True, err_msg=msg)

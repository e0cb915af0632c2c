"""The cost of the BYTE instances of the fused SORT kernel against the plain
fused entry (rv_sort_update_cams), S = 32 streams of
oracle/sort_ref.synthetic_detections loads:

  (a) all-high rows: the BYTE instance with every score at or above
      track_high_thresh (stage 2 finds nothing) against the SORT entry on the
      same rows;
  (b) a third of the scores low (rewritten under track_high_thresh) against
      the SORT entry on the same rows;
  (c) informational: an engine step at conf 0.25 (SORT) against conf 0.1
      (BYTE) -- more candidates reach NMS, so this is not the kernel's cost.

The runs of a pair are interleaved (A B A B ...), each run times K frames
with HIP events after a warm-up that brings the track count to its steady
state, and the medians are reported with the run-to-run spread (min .. max)
of each side.  Prints one JSON line.
usage: python tools/bench_byte.py [--runs 7] [--steps 30] [--no-engine]"""
import argparse
import copy
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "road-vision-system_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

S, NOBJ, DMAX, WARM = 32, 40, 100, 60
CFG = {"max_staleness": 1.2, "min_hits": 3, "iou_threshold": 0.35, "speed_window": 0.8}
HIGH = 0.25  # synthetic_detections' scores are all above it


def _load(n, low_third):
    from oracle import sort_ref
    dets = np.zeros((n, S, DMAX, 6), np.float32)
    cnt = np.zeros((n, S), np.int32)
    ts = np.zeros((n, S), np.float64)
    rng = np.random.default_rng(0)
    for s in range(S):
        fr, t = sort_ref.synthetic_detections(n, seed=s, n_obj=NOBJ, p_clutter=8.0)
        for f in range(n):
            r = fr[f][:DMAX].copy()
            if low_third and len(r):
                r[rng.uniform(size=len(r)) < 1 / 3, 4] = 0.15
            dets[f, s, :len(r)] = r
            cnt[f, s] = len(r)
            ts[f, s] = t[f]
    return dets, cnt, ts


def _tracker(dev, high):
    from rvs_amd.geometry import HomographyProjector
    from rvs_amd.track.byte_hip import MultiStreamByte
    g = np.load(os.path.join(REPO, "tests", "golden", "reference_sort.npz"), allow_pickle=False)
    proj = HomographyProjector.from_matrix(g["proj/H"], g["proj/origin"],
                                           float(g["proj/max_distance"]))
    ms = MultiStreamByte(dict(CFG, track_high_thresh=high), S, tmax=1024, dmax=DMAX, device=dev)
    ms.set_projectors([proj] * S)
    return ms


def _time_run(ms, data, steps):
    """us per frame (all S streams) over `steps` frames after the warm-up."""
    dets, cnt, ts = data
    ms.reset()
    for f in range(WARM):
        ms.update(dets[f], cnt[f], ts[f])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for f in range(WARM, WARM + steps):
        ms.update(dets[f], cnt[f], ts[f])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def _pair(dev, low_third, runs, steps):
    data = tuple(torch.from_numpy(x).to(dev) for x in _load(WARM + steps, low_third))
    sides = {"sort": _tracker(dev, 0.0), "byte": _tracker(dev, HIGH)}
    t = {k: [] for k in sides}
    for _ in range(runs):
        for k, ms in sides.items():  # interleaved
            t[k].append(_time_run(ms, data, steps))
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)}
            for k, v in t.items()}


def _engine(dev, runs, steps):
    from rvs_amd.config import load_config
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.synth import road_frames
    H, W, n = 360, 640, 8
    frames = road_frames(S, n, H, W, device=dev)
    ts = [torch.full((S,), k / 30.0, dtype=torch.float64, device=dev) for k in range(steps)]
    engs = {}
    for k, backend in (("sort_conf0.25", "sort"), ("byte_conf0.1", "bytetrack")):
        cfg = copy.deepcopy(load_config())
        cfg["tracking"]["backend"] = backend
        engs[k] = RoadVisionEngine(cfg, S, (H, W), device=dev)
    t = {k: [] for k in engs}
    for r in range(runs + 1):
        for k, eng in engs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(steps):
                eng.step(frames[i % n], ts[i])
            e1.record()
            torch.cuda.synchronize()
            if r:  # the first round warms up
                t[k].append(e0.elapsed_time(e1) * 1e3 / steps)
    for eng in engs.values():
        eng.close()
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)}
            for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-engine", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"S": S, "runs": a.runs, "steps": a.steps,
           "a_all_high": _pair(dev, False, a.runs, a.steps),
           "b_third_low": _pair(dev, True, a.runs, a.steps)}
    if not a.no_engine:
        res["c_engine_step"] = _engine(dev, a.runs, a.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

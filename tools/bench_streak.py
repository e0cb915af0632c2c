#!/usr/bin/env python3
"""Device time of the rain-streak removal (rv_streak_derain_u8) on 32 x 1080p
rainy frames: the op alone with max_len 0 and 49, the chain [StreakDerain,
CLAHEDehaze, MedianDerain] and, for comparison, the default chain
[CLAHEDehaze, MedianDerain], the last two through rv_preprocess_chain_u8 with
the letterbox.

One process, every form warmed up, device events around REPS back-to-back
calls, the forms alternated round by round; the median round of each is
reported with the spread of the rounds.  Also prints rv_streak_ws_bytes and
the bytes the kernels move per frame (from the shapes, csrc/derain.hip's tiles)
against the floor of one read and one write of the frame, and the time the
byte model would take at the HBM peak.  --kernel-stats merges the per-kernel
times of a profiler's kernel statistics (a CSV with Name, Calls and
TotalDurationNs columns) taken in a run of its own.

    python3 tools/bench_streak.py [--out profiles/streak/bench_streak.json]
"""
import argparse
import csv
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "road-vision-system_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from rvs_amd import kernels  # noqa: E402
from rvs_amd.preprocess.ops import streak_params  # noqa: E402
from rvs_amd.synth import road_frames  # noqa: E402

TILE, REJECT_W = 64, 9  # csrc/derain.hip, RV_STREAK_REJECT_W
HBM_PEAK = 8.0e12       # bytes/s, MI355X


def tile_factor(n, k, slant):
    """Bytes a line kernel's tile loads per byte it writes: the halo of n / 2
    rows and of the line's reach (+ k / 2, rounded up to 4) in columns."""
    hn = n // 2
    rxr = ((hn * abs(slant) + 2) // 4 + k // 2 + 3) // 4 * 4
    return (TILE + 2 * hn) * (TILE + 2 * rxr) / (TILE * TILE)


def byte_model(H, W, width, min_len, max_len, slant):
    """Bytes per frame each kernel asks the memory system for (halo re-reads
    included: most of them are served by the L2) and the bytes that must reach
    HBM at least once (each plane written once and read once)."""
    P = H * ((W + 15) // 16 * 16)
    k = {
        "row": {"read": 3 * H * W, "write": P},
        "erode_L": {"read": P * tile_factor(min_len, 3, slant), "write": P},
        "final": {"read": P * tile_factor(min_len, 1, slant) + P + 3 * H * W, "write": 3 * H * W},
    }
    once = 3 * H * W + P + 2 * P + 2 * P + 3 * H * W + 3 * H * W
    if max_len:
        k["erode_M"] = {"read": P * tile_factor(max_len, REJECT_W, slant), "write": P}
        k["dilate_M"] = {"read": P * tile_factor(max_len, 1, slant), "write": P}
        k["final"]["read"] += REJECT_W * P   # where S > 0 only: an upper bound
        once += 5 * P
    asked = sum(v["read"] + v["write"] for v in k.values())
    return {"kernels": {n: {a: round(b) for a, b in v.items()} for n, v in k.items()},
            "asked_bytes": round(asked), "at_least_once_bytes": round(once),
            "floor_bytes": 6 * H * W}


def rainy_frames(B, H, W, dev, p=0.02, rain_len=16, seed=0):
    """Road frames under the generator's rain model: 1-pixel streaks of slant
    -1 (column x + (y >> 2)), rain_len rows long, I' = I + (255 - I) 0.45."""
    clear = road_frames(B, 1, H, W, device=dev)[0]
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cells = torch.rand((B, H // rain_len + 1, W + H // 4 + 1), device=dev, generator=g) < p
    y = torch.arange(H, device=dev).view(H, 1)
    x = torch.arange(W, device=dev).view(1, W)
    rain = cells[:, (y // rain_len).expand(H, W), (x + (y >> 2)).expand(H, W)]
    f = clear.float()
    f = torch.where(rain.unsqueeze(-1), f + (255.0 - f) * 0.45, f)
    return f.round().clamp(0, 255).to(torch.uint8)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernel_stats(path):
    """{kernel: ms per call} of the streak kernels in a kernel-statistics CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "streak_" in name:
                short = name[name.index("streak_"):].split("(")[0].split(" ")[0]
                out[short] = round(float(row["TotalDurationNs"]) / int(row["Calls"]) * 1e-6, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=49)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "streak", "bench_streak.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_streak needs a GPU (no CPU timing is reported)")
    dev = torch.device("cuda:0")
    B, (H, W) = args.frames, args.hw
    x = rainy_frames(B, H, W, dev)
    p0 = streak_params({"slant": -1})
    pM = streak_params({"slant": -1, "max_len": args.max_len})
    geo = kernels.letterbox_geometry(H, W)
    out = torch.empty_like(x)
    lb = torch.empty((B, geo[0], geo[1], 3), dtype=torch.uint8, device=dev)
    ws_op = torch.empty(kernels.streak_ws_bytes(B, H, W, pM[2]), dtype=torch.uint8, device=dev)
    y8, med = ("clahe", "YCrCb", 8, 2.0), ("median", 3)
    chains = {"streak_clahe_median3": [("streak",) + p0, y8, med], "default": [y8, med]}
    desc = {n: kernels.chain_desc(ops) for n, ops in chains.items()}
    need = {n: kernels.preprocess_chain_ws_bytes(d, B, H, W) for n, d in desc.items()}
    ws_chain = torch.empty(max(need.values()), dtype=torch.uint8, device=dev)
    forms = {
        "op_max_len_0": lambda: kernels.streak_derain(x, *p0, out=out, ws=ws_op),
        f"op_max_len_{pM[2]}": lambda: kernels.streak_derain(x, *pM, out=out, ws=ws_op),
        "chain_streak_clahe_median3": lambda: kernels.preprocess_chain(
            x, desc["streak_clahe_median3"], geo, out=out, lb_out=lb, ws=ws_chain),
        "chain_default": lambda: kernels.preprocess_chain(x, desc["default"], geo, out=out,
                                                          lb_out=lb, ws=ws_chain),
    }
    for fn in forms.values():  # warm-up of every form
        timed(fn, 2)
    s_plane = kernels.streak_derain(x, *p0, s=True)[1]
    rounds = {n: [] for n in forms}
    for _ in range(args.rounds):
        for n, fn in forms.items():
            rounds[n].append(timed(fn, args.reps))
    res = {"what": f"ms per call of {B} x {H}x{W} frames (median of {args.rounds} rounds of "
                   f"{args.reps} calls; min and max of the rounds beside it)",
           "device": torch.cuda.get_device_name(0),
           "params": {"max_len_0": list(p0), f"max_len_{pM[2]}": list(pM)},
           "streak_pixel_share": round(float((s_plane > 0).float().mean()), 5),
           "ms": {n: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                      "max": round(max(v), 4)} for n, v in rounds.items()},
           "rv_streak_ws_bytes": {"max_len_0": kernels.streak_ws_bytes(B, H, W, 0),
                                  f"max_len_{pM[2]}": kernels.streak_ws_bytes(B, H, W, pM[2])},
           "chain_ws_bytes": need, "bytes_per_frame": {}, "model": {}}
    for tag, p in (("max_len_0", p0), (f"max_len_{pM[2]}", pM)):
        m = byte_model(H, W, p[0], p[1], p[2], p[3])
        ms = res["ms"]["op_" + tag]["median"]
        res["bytes_per_frame"][tag] = m
        res["model"][tag] = {
            "asked_GB_per_call": round(m["asked_bytes"] * B / 1e9, 3),
            "at_least_once_GB_per_call": round(m["at_least_once_bytes"] * B / 1e9, 3),
            "asked_TBps": round(m["asked_bytes"] * B / (ms * 1e-3) / 1e12, 3),
            "asked_over_floor_bytes": round(m["asked_bytes"] / m["floor_bytes"], 2),
            "ms_of_at_least_once_bytes_at_hbm_peak": round(m["at_least_once_bytes"] * B / HBM_PEAK * 1e3, 4),
            "measured_over_model": round(ms / (m["at_least_once_bytes"] * B / HBM_PEAK * 1e3), 2)}
    if args.kernel_stats:
        res["kernel_ms_per_launch"] = kernel_stats(args.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

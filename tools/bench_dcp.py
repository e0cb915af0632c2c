#!/usr/bin/env python3
"""Device time of the dark-channel dehaze (rv_dcp_dehaze_u8) on 32 x 1080p
hazy frames: the op alone, the chain [DarkChannelDehaze, MedianDerain] and,
for comparison, the default chain [CLAHEDehaze, MedianDerain], the last two
through rv_preprocess_chain_u8 with the letterbox.

One process, every form warmed up, device events around REPS back-to-back
calls, the forms alternated round by round; the median round of each is
reported with the spread of the rounds.  Also prints rv_dcp_ws_bytes and the
bytes the kernels move per frame (from the shapes, csrc/dehaze.hip's tiles)
against the floor of one read and one write of the frame.

    python3 tools/bench_dcp.py [--out profiles/dcp/bench_dcp.json]
"""
import argparse
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
from rvs_amd.preprocess.ops import dcp_params  # noqa: E402
from rvs_amd.synth import road_frames  # noqa: E402

TW, TH, BAND, SEG = 128, 32, 64, 512  # csrc/dehaze.hip


def byte_model(H, W, patch, radius):
    """Bytes per frame each kernel asks the memory system for (halo re-reads
    included: most of them are served by the L2) and the bytes that must reach
    HBM at least once (each plane written once and read once)."""
    P = H * ((W + 15) // 16 * 16)
    hp = patch // 2
    halo = (TW + 2 * hp) * (TH + 2 * hp) / (TW * TH)
    rows = (2 * radius + 1 + 2 * BAND) / BAND   # rows a column-sum thread reads per row written
    seg = (SEG + 2 * radius) / SEG
    k = {
        "min0": {"read": 3 * H * W * halo, "write": 0},
        "min1": {"read": 3 * H * W * halo, "write": (2 * P if radius else 4 * H * W)},
    }
    if radius:
        k["vsum1"] = {"read": 2 * P * rows, "write": 12 * P}
        k["hsum1"] = {"read": 12 * P * seg, "write": 8 * P}
        k["vsum2"] = {"read": 8 * P * rows, "write": 12 * P}
        k["hsum2"] = {"read": 12 * P * seg + P + 3 * H * W, "write": 3 * H * W}
    asked = sum(v["read"] + v["write"] for v in k.values())
    once = 2 * 3 * H * W + 3 * H * W + (2 * (2 + 12 + 8 + 12) * P + P if radius else 0)
    return {"kernels": {n: {a: round(b) for a, b in v.items()} for n, v in k.items()},
            "asked_bytes": round(asked), "at_least_once_bytes": round(once),
            "floor_bytes": 6 * H * W}


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dcp", "bench_dcp.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dcp needs a GPU (no CPU timing is reported)")
    dev = torch.device("cuda:0")
    B, (H, W) = args.frames, args.hw
    clear = road_frames(B, 1, H, W, device=dev)[0]
    # depth-dependent haze toward A = 230, thicker toward the top of the frame
    t = torch.exp(-1.5 * (1.0 - torch.arange(H, device=dev, dtype=torch.float32) / H))
    t = t.view(1, H, 1, 1)
    x = (clear.float() * t + 230.0 * (1.0 - t)).round().clamp(0, 255).to(torch.uint8)
    del clear
    p = dcp_params({})
    geo = kernels.letterbox_geometry(H, W)
    out = torch.empty_like(x)
    lb = torch.empty((B, geo[0], geo[1], 3), dtype=torch.uint8, device=dev)
    ws_op = torch.empty(kernels.dcp_ws_bytes(B, H, W, p[3]), dtype=torch.uint8, device=dev)
    chains = {"dcp_median3": [("dcp",) + p, ("median", 3)],
              "default": [("clahe", "YCrCb", 8, 2.0), ("median", 3)]}
    desc = {n: kernels.chain_desc(ops) for n, ops in chains.items()}
    need = {n: kernels.preprocess_chain_ws_bytes(d, B, H, W) for n, d in desc.items()}
    ws_chain = torch.empty(max(need.values()), dtype=torch.uint8, device=dev)
    forms = {
        "op": lambda: kernels.dcp_dehaze(x, *p, out=out, ws=ws_op),
        "op_radius0": lambda: kernels.dcp_dehaze(x, p[0], p[1], p[2], 0, p[4], out=out, ws=ws_op),
        "chain_dcp_median3": lambda: kernels.preprocess_chain(x, desc["dcp_median3"], geo, out=out,
                                                              lb_out=lb, ws=ws_chain),
        "chain_default": lambda: kernels.preprocess_chain(x, desc["default"], geo, out=out,
                                                          lb_out=lb, ws=ws_chain),
    }
    for fn in forms.values():  # warm-up of every form
        timed(fn, 2)
    rounds = {n: [] for n in forms}
    for _ in range(args.rounds):
        for n, fn in forms.items():
            rounds[n].append(timed(fn, args.reps))
    model = byte_model(H, W, p[0], p[3])
    res = {"what": f"ms per call of {B} x {H}x{W} frames (median of {args.rounds} rounds of "
                   f"{args.reps} calls; min and max of the rounds beside it)",
           "device": torch.cuda.get_device_name(0), "params": list(p),
           "ms": {n: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                      "max": round(max(v), 4)} for n, v in rounds.items()},
           "rv_dcp_ws_bytes": int(ws_op.numel()),
           "chain_ws_bytes": need, "bytes_per_frame": model}
    ms = res["ms"]["op"]["median"]
    res["op_asked_TBps"] = round(model["asked_bytes"] * B / (ms * 1e-3) / 1e12, 3)
    res["op_over_floor_bytes"] = round(model["asked_bytes"] / model["floor_bytes"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

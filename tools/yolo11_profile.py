"""Per-launch device time of the YOLO11n forward beside YOLOv8n's, in one
process on one device (HIP events, rv_yolo_profile_reps): batch B, HxW road
frames letterboxed at imgsz 640, both plans autotuned.

YOLO11 has no shipped calibration, so its weights are tests/yolo11_ref.py's
one-pass normalisation on two of the frames; YOLOv8n uses the shipped
synthetic weights.  Writes OUT.txt (one row per launch, in launch order) and
OUT.json; prints both totals and the attention / depthwise shares.

    B=128 H=360 W=640 OUT=profiles/r15/yolo11_profile_b128_384x640 python tools/yolo11_profile.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "road-vision-system_amd"), os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yolo11_ref as y11  # noqa: E402
import yolo_synth  # noqa: E402
from rvs_amd import _lib  # noqa: E402
from rvs_amd.detect import weights  # noqa: E402
from rvs_amd.detect.yolo_hip import YoloEngine  # noqa: E402

B = int(os.environ.get("B", 128))
H, W = int(os.environ.get("H", 360)), int(os.environ.get("W", 640))
N = int(os.environ.get("N", 5))
REPS = int(os.environ.get("REPS", 5))  # launches per event pair (event overhead)
OUT = os.environ.get("OUT", "yolo11_profile")
lib = _lib.load()


def profile(variant, flat, frames):
    eng = YoloEngine(variant, flat, B, (H, W), imgsz=640)
    lb = eng.letterbox(frames)
    for _ in range(3):
        eng.forward_raw(lb)
    eng.autotune(lb)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(N):
        eng.forward_raw(lb)
    e.record()
    torch.cuda.synchronize()
    fwd = s.elapsed_time(e) / N
    lib.rv_yolo_profile_reps(eng._h, N, REPS)
    for _ in range(N):
        eng.forward_raw(lb)
    torch.cuda.synchronize()
    n = lib.rv_yolo_num_convs(variant)
    ms, fl, by = np.zeros(n), np.zeros(n), np.zeros(n)
    cv = np.zeros(n, np.int32)
    nf = lib.rv_yolo_profile_read(eng._h, ms.ctypes.data, fl.ctypes.data, cv.ctypes.data, n)
    lib.rv_yolo_profile_bytes(eng._h, by.ctypes.data, n)
    convs, groups, cfgs = weights.conv_list(variant), weights.conv_groups(variant), eng.tuned_configs()
    rows, seen = [], set()
    for i in range(n):
        if cv[i] < 0:
            continue
        name, ci, co, k, st, act = convs[cv[i]]
        kind = "depthwise" if groups[cv[i]] > 1 else "conv"
        if i == n - 1:
            kind, name = "stem", "stem (model.0 ...)"
        elif name.endswith(".attn.qkv") and cv[i] in seen:  # the attention behind its qkv conv
            kind, name = "attention", name[:-len(".qkv")]
        seen.add(int(cv[i]))
        t = ms[i] / nf
        rows.append(dict(slot=i, kind=kind, name=name, cin=ci, cout=co, k=k, s=st, us=t * 1e3,
                         gflop=fl[i] / 1e9, tflops=fl[i] / t / 1e9, gbps=by[i] / t / 1e6,
                         cfg=list(cfgs[i]) if i < len(cfgs) else []))
    eng.close()
    return dict(variant=variant, forward_ms=fwd, launch_sum_ms=sum(r["us"] for r in rows) / 1e3,
                launches=len(rows), rows=rows)


def main():
    fr = yolo_synth.frames(H, W, 4)
    frames = torch.from_numpy(np.concatenate([fr] * ((B + 3) // 4))[:B].copy()).cuda()
    flat11 = y11.synth_weights_on(20, yolo_synth.letterboxed(H, W, 2, 640))
    res = {"B": B, "frame": [H, W], "reps": REPS, "forwards": N,
           "yolov8n": profile(0, weights.synthetic_weights(0), frames),
           "yolo11n": profile(20, flat11, frames)}
    lines = []
    for key in ("yolov8n", "yolo11n"):
        p = res[key]
        lines.append(f"== {key}: forward {p['forward_ms']:.3f} ms unprofiled; per-launch sum "
                     f"{p['launch_sum_ms']:.3f} ms over {p['launches']} launches")
        for r in p["rows"]:
            lines.append(f"{r['us']:8.1f} us {r['gflop']:7.2f} GF {r['tflops']:7.1f} TF/s {r['gbps']:7.0f} GB/s  "
                         f"{r['kind']:9s} {r['name']:26s} {r['cin']:4d}->{r['cout']:4d} k{r['k']} s{r['s']}  "
                         f"cfg {r['cfg']}")
    p = res["yolo11n"]
    for kind in ("attention", "depthwise"):
        us = sum(r["us"] for r in p["rows"] if r["kind"] == kind)
        res[kind + "_us"] = us
        lines.append(f"yolo11n {kind}: {us:.1f} us in {sum(r['kind'] == kind for r in p['rows'])} launches, "
                     f"{100 * us / (p['launch_sum_ms'] * 1e3):.1f} % of the per-launch sum")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(OUT + ".json", "w") as f:
        json.dump(res, f, indent=1)
    print("\n".join(ln for ln in lines if ln.startswith(("==", "yolo11n "))))


if __name__ == "__main__":
    main()

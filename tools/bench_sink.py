"""The JPEG encoder and the Motion-JPEG sink on S 1080p proc frames (the
benchmark's synthetic road frames through the default CLAHE + median chain):

    python3 tools/bench_sink.py [--streams 32] [--reps 30] [--out profiles/rNN/bench_sink.json]

Per quality (75, 95), 4:2:0: ms per step of the encode alone (device events
around each call, after warm-up; also its two halves, frames -> records and
records -> streams), bytes per frame, the sink's sustained frames/s into files
on a memory file system (host clock from the first write to the end of
flush()), and, where Pillow is installed, Pillow's encode rate on 16 threads.
Reported, not gated."""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "road-vision-system_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rvs_amd import _lib  # noqa: E402
from rvs_amd.io_video import MultiStreamSink  # noqa: E402
from rvs_amd.io_video.sink import default_capacity  # noqa: E402
from rvs_amd.kernels import (bgr_to_jpeg_coef, clahe_median, jpeg_coef_to_stream,  # noqa: E402
                             jpeg_encode)
from rvs_amd.synth import road_frames  # noqa: E402

H, W = 1080, 1920


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    for k in range(reps):
        ev[k].record()
        fn()
    ev[reps].record()
    torch.cuda.synchronize()
    ms = sorted(ev[k].elapsed_time(ev[k + 1]) for k in range(reps))
    return {"median_ms": round(ms[reps // 2], 4), "min_ms": round(ms[0], 4),
            "max_ms": round(ms[-1], 4)}


def pillow_rate(frames, quality, seconds=2.0):
    try:
        from PIL import Image
    except ImportError:
        return None
    import io
    from concurrent.futures import ThreadPoolExecutor
    imgs = [Image.fromarray(f[..., ::-1].copy()) for f in frames]

    def one(i):
        buf = io.BytesIO()
        imgs[i % len(imgs)].save(buf, "JPEG", quality=quality, subsampling=2)
        return buf.tell()

    with ThreadPoolExecutor(16) as pool:
        list(pool.map(one, range(32)))
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            list(pool.map(one, range(64)))
            n += 64
        return round(n / (time.perf_counter() - t0), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sink-steps", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    S = args.streams
    dev = torch.device("cuda:0")
    proc = clahe_median(road_frames(S, 1, H, W, device=dev)[0])
    host = proc.cpu().numpy()
    cap = default_capacity(W, H, "420")
    out = torch.empty((S, cap), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(_lib.load().rv_jpeg_encode_ws_bytes(S, W, H, 2)), dtype=torch.uint8,
                     device=dev)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    result = {"streams": S, "frame": [H, W], "sampling": "420", "capacity": cap,
              "workspace_bytes": ws.numel(), "reps": args.reps, "quality": {}}
    for q in (75, 95):
        r = {}
        r["encode"] = timed(lambda: jpeg_encode(proc, q, "420", out=out, ws=ws), args.reps)
        rec = bgr_to_jpeg_coef(proc, q, "420")
        r["frames_to_records"] = timed(lambda: bgr_to_jpeg_coef(proc, q, "420", out=rec), args.reps)
        r["records_to_streams"] = timed(
            lambda: jpeg_coef_to_stream(rec, W, H, "420", q, out=out, ws=ws), args.reps)
        hdr = out[:, :16].cpu().numpy().view(np.uint32)
        assert (hdr[:, 2] == 0).all(), "a frame overflowed the default capacity"
        r["bytes_per_frame"] = int(hdr[:, 1].mean())
        del rec
        with tempfile.TemporaryDirectory(dir=shm) as d:
            sink = MultiStreamSink([os.path.join(d, f"s{s}.mjpeg") for s in range(S)], (H, W),
                                   quality=q, sampling="420", device=dev)
            for _ in range(4):
                sink.write(proc)
            sink.flush()
            t0 = time.perf_counter()
            for _ in range(args.sink_steps):
                sink.write(proc)
            sink.flush()
            dt = time.perf_counter() - t0
            st = sink.stats()
            sink.close()
            r["sink"] = {"frames_per_s": round(S * args.sink_steps / dt, 1),
                         "steps": args.sink_steps, "seconds": round(dt, 3),
                         "bytes_copied_per_frame": int(sum(x["bytes_copied"] for x in st) /
                                                       sum(x["submitted"] for x in st)),
                         "memory_fs": shm is not None}
        r["pillow_16_threads_frames_per_s"] = pillow_rate(host, q)
        result["quality"][str(q)] = r
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

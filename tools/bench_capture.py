"""Capture-fed frames through the whole front end (§8(f)4; a PCIe-inclusive
rate, never the bench `value`): S camera streams, each a YUV4MPEG2 file of F
1080p frames (looped), read by the native reader threads into pinned slots,
uploaded as NV12 by MultiStreamCapture on its copy stream one batch ahead,
converted to BGR on the device, then one RoadVisionEngine step per batch
(eager launches) with the result hand-back.  Prints one JSON line: frames/s
of the capture-fed loop, the capture alone (no engine), and the
device-resident eager rate on the same engine for reference.

``--format mjpeg`` feeds the same frames as Motion-JPEG files instead (4:2:0,
quality 75, encoded here with Pillow): the reader threads entropy-decode, the
device does IDCT + upsampling + colour.  It adds the host decode rate of one
thread, the capture-only rate of the y4m path in the same run, the bytes
uploaded per frame, and event-timed figures for rv_jpeg_coef_to_bgr_u8 and
rv_nv12_to_bgr_u8 on one S-frame batch (run it under a kernel trace for the
kernel times proper)."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "road-vision-system_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import bench_config  # noqa: E402
from rvs_amd.engine import RoadVisionEngine  # noqa: E402
from rvs_amd.io_video import MultiStreamCapture, jpeg_coefficients, write_y4m  # noqa: E402
from rvs_amd.kernels import jpeg_to_bgr, nv12_to_bgr  # noqa: E402
from rvs_amd.synth import road_frames  # noqa: E402

S = int(os.environ.get("S", 32))
F = int(os.environ.get("F", 4))
K = int(os.environ.get("K", 30))
H, W = 1080, 1920


def capture_only(cap):
    for _ in range(3):
        cap.next_batch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        cap.next_batch()
    torch.cuda.synchronize()
    return S * K / (time.perf_counter() - t0)


def event_ms(fn, reps=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def mjpeg_extras(frames, tmp, y4m_paths, dev):
    """MJPEG files of the same frames plus the figures only that format has."""
    from PIL import Image
    paths, images = [], []
    for s in range(S):
        p = os.path.join(tmp, f"cam{s}.mjpeg")
        with open(p, "wb") as f:
            for k in range(F):
                buf = io.BytesIO()
                Image.fromarray(frames[k, s][..., ::-1]).save(buf, "JPEG", quality=75,
                                                              subsampling=2)
                images.append(buf.getvalue())
                f.write(images[-1])
        paths.append(p)
    t0 = time.perf_counter()
    recs = [jpeg_coefficients(i) for i in images[:32]]
    decode_fps = len(recs) / (time.perf_counter() - t0)
    batch = torch.from_numpy(np.stack([recs[i % len(recs)] for i in range(S)])).to(dev)
    out = torch.empty((S, H, W, 3), dtype=torch.uint8, device=dev)
    nv12 = torch.randint(0, 256, (S, 3 * H // 2, W), dtype=torch.uint8, device=dev)
    cap = MultiStreamCapture(y4m_paths, device=dev, loop=True, nbuf=4)
    y4m_fps = capture_only(cap)
    cap.close()
    return paths, {
        "jpeg_bytes_per_frame": int(np.mean([len(i) for i in images])),
        "record_bytes_per_frame": int(recs[0].size),
        "host_decode_fps_one_thread": round(decode_fps, 1),
        "jpeg_to_bgr_ms_per_batch_events": round(event_ms(lambda: jpeg_to_bgr(batch, W, H, out=out)), 3),
        "nv12_to_bgr_ms_per_batch_events": round(event_ms(lambda: nv12_to_bgr(nv12, out=out)), 3),
        "y4m_capture_only_fps": round(y4m_fps, 1),
        "y4m_h2d_gbs_at_capture_rate": round(y4m_fps * H * W * 1.5 / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=["y4m", "mjpeg"], default="y4m")
    fmt = ap.parse_args().format
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    frames = road_frames(S, F, H, W, device=dev).cpu().numpy()
    paths = []
    t0 = time.perf_counter()
    for s in range(S):
        p = os.path.join(tmp, f"cam{s}.y4m")
        write_y4m(p, [frames[f, s] for f in range(F)])
        paths.append(p)
    gen_s = time.perf_counter() - t0
    y4m_paths, extra = paths, {}
    if fmt == "mjpeg":
        paths, extra = mjpeg_extras(frames, tmp, y4m_paths, dev)
    eng = RoadVisionEngine(bench_config(), S, (H, W), device=dev)
    # capture alone
    cap = MultiStreamCapture(paths, device=dev, loop=True, nbuf=4)
    cap_only = capture_only(cap)
    frame_bytes = cap.frame_bytes
    # capture-fed engine steps
    for k in range(3):
        fr, ts, _ = cap.next_batch()
        eng.step(fr, ts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(K):
        fr, ts, _ = cap.next_batch()
        eng.step(fr, ts)
    torch.cuda.synchronize()
    fed = S * K / (time.perf_counter() - t0)
    pinned = cap.pinned
    cap.close()
    # device-resident eager steps on the same engine
    src = road_frames(S, 2, H, W, device=dev)
    tsd = torch.zeros(S, dtype=torch.float64, device=dev)
    for k in range(3):
        eng.step(src[k % 2], tsd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(K):
        eng.step(src[k % 2], tsd)
    torch.cuda.synchronize()
    resident = S * K / (time.perf_counter() - t0)
    eng.close()
    for p in set(paths) | set(y4m_paths):
        os.remove(p)
    metric = ("capture-fed frames/s @1080p (y4m files -> reader threads -> pinned NV12 -> "
              "H2D -> device NV12->BGR -> full chain, eager steps)")
    if fmt == "mjpeg":
        metric = ("capture-fed frames/s @1080p (mjpeg files -> reader threads: Huffman decode -> "
                  "pinned coefficient records -> H2D -> device IDCT + colour -> full chain, "
                  "eager steps)")
    print(json.dumps({
        "metric": metric,
        "value": round(fed, 1), "unit": "frames/s", "streams": S, "steps": K,
        "capture_only_fps": round(cap_only, 1), "device_resident_eager_fps": round(resident, 1),
        "pinned_slots": bool(pinned), "nv12_bytes_per_frame": H * W * 3 // 2,
        "h2d_gbs_at_capture_rate": round(cap_only * frame_bytes / 1e9, 2),
        "y4m_generation_s": round(gen_s, 1), **extra}))


if __name__ == "__main__":
    main()

"""Frame sink: the reference's ``writer.write(frame)`` (main_preview.py:130,137)
for device-resident frames.

``encode_jpeg`` is cv2.imencode(".jpg") for BGR frames on the GPU: colour
conversion, chroma downsampling, DCT, quantisation and Huffman coding all run
in HIP kernels (rv_jpeg_encode_bgr_u8), and the bytes equal what libjpeg
writes with its default settings and one restart segment per MCU row.
``VideoSink`` (one stream) and ``MultiStreamSink`` (S streams, one file each)
write Motion-JPEG files -- complete JPEG images back to back -- which
``VideoSource`` / ``MultiStreamCapture`` read back.  Only the compressed
bytes cross to the host: native writer threads over pinned rings
(rv_sink_*) copy each image once its encode has finished, without ever making
the caller's GPU stream wait.

Containers: ``.mjpeg`` / ``.mjpg`` only.  There is no MP4 / AVI muxer and no
timing in the file.  What is recorded is ``preview.record.content``: the bare
proc frames, the frames with the detection overlays, or the RAW | PROC compare
canvas; the drawing is ``rvs_amd.vis`` (rv_overlay_raster), which a sink runs
on its own stream through ``write(..., render=...)``.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream_ptr

_CONTAINERS = (".mjpeg", ".mjpg")
# preview.record.content: what a recording engine writes
RECORD_CONTENTS = ("proc", "annotated", "compare")


def _device_frames(frames, device) -> torch.Tensor:
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if not frames.is_cuda:
        frames = frames.to(torch.device(device) if device is not None else torch.device("cuda:0"))
    return frames.unsqueeze(0) if frames.dim() == 3 else frames


def stream_payloads(streams: torch.Tensor) -> List[bytes]:
    """The images of encoded device streams (kernels.jpeg_encode) as bytes:
    the headers come over first, then only each image's own bytes."""
    from ..kernels import (JPEG_STREAM_HEADER_BYTES as HB, JPEG_STREAM_MAGIC, JPEG_STREAM_OVERFLOW,
                           JPEG_STREAM_BAD_RECORD)
    hdr = streams[:, :HB].contiguous().cpu().numpy().view(np.uint32).reshape(-1, 4)
    out = []
    for s, (magic, n, flags, _) in enumerate(hdr.tolist()):
        if magic != JPEG_STREAM_MAGIC or flags & JPEG_STREAM_BAD_RECORD:
            raise _lib.RVError(f"stream {s} is not an encoded JPEG stream")
        if flags & JPEG_STREAM_OVERFLOW:
            raise _lib.RVError(f"stream {s}: the image of {n} bytes overflowed its capacity")
        out.append(streams[s, HB:HB + n].cpu().numpy().tobytes())
    return out


def encode_jpeg(frames, quality: int = 95, sampling: str = "420", device=None) -> List[bytes]:
    """cv2.imencode(".jpg", frame, [IMWRITE_JPEG_QUALITY, quality]) for one
    (H, W, 3) or a batch (S, H, W, 3) of BGR u8 frames (device tensors, or host
    arrays, which are uploaded): one complete baseline JPEG image per frame,
    encoded on the GPU."""
    from ..kernels import jpeg_encode
    x = _device_frames(frames, device)
    with torch.cuda.device(x.device):
        return stream_payloads(jpeg_encode(x, quality, sampling))


def default_capacity(W: int, H: int, sampling="420") -> int:
    """Bytes reserved per encoded frame when the caller names none: 16 header
    bytes and one byte per pixel (about three times what camera footage takes
    at quality 95), at least 64 KiB, never above the worst case
    (kernels.jpeg_stream_bound)."""
    from ..kernels import jpeg_stream_bound
    cap = (16 + max(64 << 10, int(W) * int(H)) + 4095) // 4096 * 4096
    return min(cap, jpeg_stream_bound(W, H, sampling))


class MultiStreamSink:
    """One Motion-JPEG file per stream.  write(batch) encodes (S, H, W, 3) BGR
    u8 device frames on a side stream -- ordered after the work queued so far
    on the current stream, or after `after` -- and queues every stream's image
    for its file's writer thread; it returns without waiting for the GPU
    (unless all `nbuf` slots of a ring are still being written).  An image
    larger than `capacity`, or an I/O error, is raised by the next write() and
    by close().  close() writes what is queued and flushes the files."""

    def __init__(self, paths: Sequence[str], frame_hw, quality: int = 95, sampling: str = "420",
                 device="cuda:0", nbuf: int = 4, capacity: Optional[int] = None):
        from ..kernels import jpeg_sampling_code
        self.paths = [str(p) for p in paths]
        for p in self.paths:
            if os.path.splitext(p)[1].lower() not in _CONTAINERS:
                raise ValueError(f"{p!r}: supported containers are Motion-JPEG (.mjpeg / .mjpg); "
                                 "there is no MP4 muxer")
        if not 1 <= int(quality) <= 100:
            raise ValueError(f"JPEG quality {quality} not in 1..100")
        self.S = len(self.paths)
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        self.quality, self.sampling = int(quality), sampling
        jpeg_sampling_code(sampling)
        self.device = torch.device(device)
        self.nbuf = int(nbuf)
        self.capacity = int(capacity) if capacity is not None else \
            default_capacity(self.W, self.H, sampling)
        self._handles: List[ctypes.c_void_p] = []
        self._n = 0
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(self.device)
            # a batch's device memory must outlive nbuf later writes: nbuf + 1 in rotation
            self._bufs = torch.empty((self.nbuf + 1, self.S, self.capacity), dtype=torch.uint8,
                                     device=self.device)
            self._ws = None
            try:
                for p in self.paths:
                    h = ctypes.c_void_p()
                    call("rv_sink_open", p.encode(), self.nbuf, self.capacity, ctypes.byref(h))
                    self._handles.append(h)
            except Exception:
                self._close_handles()
                raise
        self._harr = (ctypes.c_void_p * self.S)(*[h.value for h in self._handles])

    def write(self, batch, after: Optional[torch.cuda.Event] = None, render=None) -> None:
        """render: a callable that runs on the sink's stream, behind `after`,
        and returns the (S, H, W, 3) frames to encode -- the overlay raster of
        a recording engine.  `batch` is then the tensor, or the tensors, it
        reads (they are kept alive for the sink's stream)."""
        from ..kernels import jpeg_encode
        if not self._handles:
            raise RuntimeError("the sink is closed")
        inputs = [batch] if isinstance(batch, torch.Tensor) else list(batch)
        if render is None and (len(inputs) != 1 or not inputs[0].is_cuda or
                               tuple(inputs[0].shape) != (self.S, self.H, self.W, 3)):
            raise ValueError(f"expected ({self.S}, {self.H}, {self.W}, 3) uint8 frames on the GPU")
        with torch.cuda.device(self.device):
            if after is None:
                after = torch.cuda.Event()
                after.record(torch.cuda.current_stream())
            self.stream.wait_event(after)
            for t in inputs:
                t.record_stream(self.stream)
            out = self._bufs[self._n % (self.nbuf + 1)]
            with torch.cuda.stream(self.stream):
                if render is not None:
                    batch = render()
                    if tuple(batch.shape) != (self.S, self.H, self.W, 3):
                        raise ValueError(f"render() gave {tuple(batch.shape)} frames for a sink "
                                         f"of ({self.S}, {self.H}, {self.W}, 3)")
                else:
                    batch = inputs[0]
                if self._ws is None:
                    need = int(_lib.load().rv_jpeg_encode_ws_bytes(self.S, self.W, self.H,
                                                                   _code(self.sampling)))
                    self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                jpeg_encode(batch, self.quality, self.sampling, out=out, ws=self._ws)
                call("rv_sink_write_batch", self._harr, self.S, ptr(out), out.stride(0),
                     stream_ptr(self.stream))
        self._n += 1

    def stats(self) -> List[dict]:
        keys = ("submitted", "written", "bytes_written", "bytes_copied", "overflowed", "failed",
                "nbuf", "capacity")
        out = []
        for h in self._handles:
            st = (ctypes.c_int64 * 8)()
            call("rv_sink_stats", h, st)
            out.append(dict(zip(keys, [int(v) for v in st])))
        return out

    def flush(self) -> None:
        """Wait until every frame written so far is in its file."""
        for h in self._handles:
            call("rv_sink_flush", h)

    def _close_handles(self):
        first = None
        handles, self._handles = self._handles, []
        for h in handles:
            try:
                call("rv_sink_close", h)
            except _lib.RVError as exc:
                first = first or exc
        return first

    def close(self) -> None:
        with torch.cuda.device(self.device):
            exc = self._close_handles()
        self._bufs = self._ws = None
        if exc is not None:
            raise exc

    release = close


def _code(sampling) -> int:
    from ..kernels import jpeg_sampling_code
    return jpeg_sampling_code(sampling)


class VideoSink:
    """cv2.VideoWriter for one stream: write(frame) takes an (H, W, 3) BGR u8
    frame (device tensor, or a host array, which is uploaded); release()
    writes what is queued and closes the file."""

    def __init__(self, path: str, frame_hw, quality: int = 95, sampling: str = "420",
                 device="cuda:0", nbuf: int = 4, capacity: Optional[int] = None):
        self._m = MultiStreamSink([path], frame_hw, quality, sampling, device, nbuf, capacity)

    def write(self, frame) -> None:
        self._m.write(_device_frames(frame, self._m.device))

    def stats(self) -> dict:
        return self._m.stats()[0]

    def release(self) -> None:
        self._m.close()


def record_settings(cfg: Optional[dict], n_streams: int) -> Optional[dict]:
    """preview.record of a config -> None when recording is off, else
    {"paths": one file per stream, "quality", "sampling"}, plus "content" when
    it is not the default "proc".  Raises for a container other than
    Motion-JPEG, for several streams sharing a path and for a content other
    than "proc" / "annotated" / "compare"."""
    rec = ((cfg or {}).get("preview") or {}).get("record") or {}
    if not rec.get("enable", False):
        return None
    path = str(rec.get("path", ""))
    if os.path.splitext(path)[1].lower() not in _CONTAINERS:
        raise ValueError(f"preview.record.path {path!r}: supported containers are Motion-JPEG "
                         "(.mjpeg / .mjpg); there is no MP4 muxer")
    if n_streams > 1 and "{stream}" not in path:
        raise ValueError(f"preview.record.path {path!r} needs a {{stream}} field to name one file "
                         f"for each of the {n_streams} streams")
    quality = int(rec.get("quality", 95))
    if not 1 <= quality <= 100:
        raise ValueError(f"preview.record.quality {quality} not in 1..100")
    sampling = str(rec.get("sampling", "420"))
    _code(sampling)
    content = rec.get("content", "proc")
    if content not in RECORD_CONTENTS:
        raise ValueError(f"preview.record.content {content!r}: expected one of {RECORD_CONTENTS}")
    paths = [path.format(stream=s) if "{stream}" in path else path for s in range(n_streams)]
    out = {"paths": paths, "quality": quality, "sampling": sampling}
    if content != "proc":
        out["content"] = content
    return out

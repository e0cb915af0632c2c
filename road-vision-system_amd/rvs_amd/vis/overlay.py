"""Drawing on device frames: rv_overlay_layout / rv_overlay_raster behind the
reference's ``src/vis`` surface (draw_detections) and main_preview.py's
make_canvas.  The raster model is the one of include/rvhip.h; there is no
host drawing path."""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream_ptr
from . import display_list as dlist

ANNOTATE, COMPARE_H, COMPARE_V = 0, 1, 2


def _mode(layout: Optional[str]) -> int:
    if layout is None:
        return ANNOTATE
    return COMPARE_V if str(layout).lower() == "v" else COMPARE_H


def _u8_frames(x: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.uint8 or \
            x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"{what} must be (S, H, W, 3) uint8 frames on the GPU")
    return x.contiguous()


def raster(proc: torch.Tensor, raw: Optional[torch.Tensor] = None, layout: Optional[str] = None,
           divider_px: int = 0, lists: Optional[torch.Tensor] = None, dmax: int = 0,
           canvas: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rv_overlay_raster on the current stream: (S, H, W, 3) proc (and raw, for
    a canvas `layout` "h" / "v") + the streams' display lists `lists` (a uint8
    device tensor for `dmax`) + the canvas list -> out."""
    proc = _u8_frames(proc, "proc")
    S, H, W, _ = proc.shape
    mode = _mode(layout)
    if mode != ANNOTATE:
        raw = _u8_frames(raw, "raw")
        if raw.shape != proc.shape:
            raise ValueError("raw and proc must have one shape")
    oh, ow, _, _, d = dlist.canvas_geometry(H, W, layout, divider_px) if mode != ANNOTATE \
        else (H, W, 0, 0, 0)
    if out is None:
        out = torch.empty((S, oh, ow, 3), dtype=torch.uint8, device=proc.device)
    elif tuple(out.shape) != (S, oh, ow, 3) or out.dtype != torch.uint8 or not out.is_contiguous() \
            or out.device != proc.device:
        raise ValueError(f"out must be a contiguous ({S}, {oh}, {ow}, 3) uint8 tensor")
    if lists is not None and lists.numel() < S * dlist.list_bytes(dmax):
        raise ValueError(f"display lists of {lists.numel()} bytes for {S} streams, dmax {dmax}")
    with torch.cuda.device(proc.device):
        call("rv_overlay_raster", ptr(proc), ptr(raw) if mode != ANNOTATE else None, S, H, W, mode,
             d, ptr(lists), int(dmax), ptr(canvas), ptr(out), stream_ptr())
    return out


def _upload(arr: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(arr)).to(device)


def draw_detections(image, detections: Iterable, thickness: int = 2,
                    font_scale: float = 0.6) -> None:
    """The reference's draw_detections (src/vis/draw.py:25), in place: boxes,
    "ID n | class conf" and "12.3 m / 45.6 km/h" on `image`, an (H, W, 3) BGR
    u8 device tensor -- or a numpy array, which is uploaded, drawn on and
    copied back.  The display list is built on the host from the Detection
    list; the drawing is rv_overlay_raster."""
    host = image if isinstance(image, np.ndarray) else None
    dev = _upload(host, "cuda:0") if host is not None else image
    if not isinstance(dev, torch.Tensor) or dev.dim() != 3 or dev.shape[-1] != 3 or \
            dev.dtype != torch.uint8 or not dev.is_cuda:
        raise ValueError("image must be an (H, W, 3) uint8 array or GPU tensor")
    dl = dlist.detection_list(detections, int(dev.shape[0]), thickness, font_scale)
    if len(dl) == 0:
        return
    dmax = max(1, -(-(len(dl) - 8) // 5))
    lists = _upload(dl.to_bytes(dlist.capacity(dmax)), dev.device)
    drawn = raster(dev.contiguous().unsqueeze(0), lists=lists, dmax=dmax)[0]
    if host is not None:
        host[...] = drawn.cpu().numpy()
    else:
        dev.copy_(drawn)


def make_canvas(raw: torch.Tensor, proc: torch.Tensor, layout: str = "h", divider_px: int = 4,
                label_raw: str = "RAW", label_proc: str = "PROC", fps: Optional[float] = None,
                show_fps: bool = True) -> torch.Tensor:
    """main_preview.py's make_canvas for device frames, (H, W, 3) or a batch
    (S, H, W, 3): RAW | divider | PROC (or stacked, layout "v") with the
    labels.  Draw detections on `proc` first, as the reference does."""
    single = raw.dim() == 3
    r = raw.unsqueeze(0) if single else raw
    p = proc.unsqueeze(0) if single else proc
    H, W = int(r.shape[1]), int(r.shape[2])
    labels = dlist.canvas_list(H, W, layout, divider_px, label_raw, label_proc, fps, show_fps)
    canvas = _upload(labels.to_bytes(dlist.CANVAS_PRIMS), r.device)
    out = raster(p, r, "v" if str(layout).lower() == "v" else "h", divider_px, canvas=canvas)
    return out[0] if single else out


class OverlayRenderer:
    """The batched device path: one step's results -> display lists
    (``layout``, rv_overlay_layout) -> annotated frames or compare canvases
    (``raster``, rv_overlay_raster).  The two are separate calls so that they
    can sit on different streams: the lists live in `slots` rotating buffers.

    compare: None for annotated frames, else a mapping with make_canvas's
    layout / divider_px / label_raw / label_proc."""

    def __init__(self, n_streams: int, frame_hw, max_det: int, names: Sequence, thickness: int = 2,
                 font_scale: float = 0.6, device="cuda:0", compare: Optional[dict] = None,
                 slots: int = 1):
        self.S, self.dmax = int(n_streams), int(max_det)
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        self.thickness = max(1, int(thickness))
        self.k = dlist.glyph_scale(font_scale)
        if self.thickness > 33:
            raise ValueError(f"thickness {thickness}: text is drawn up to thickness 32")
        self.device = torch.device(device)
        table = dlist.names_table(names)
        self.nc = int(table.shape[0])
        self.compare = dict(compare) if compare is not None else None
        self.layout_code = None
        self.divider_px = 0
        if self.compare is not None:
            self.layout_code = "v" if str(self.compare.get("layout", "h")).lower() == "v" else "h"
            self.divider_px = max(0, int(self.compare.get("divider_px", 4)))
        self.out_hw = dlist.canvas_geometry(self.H, self.W, self.layout_code, self.divider_px)[:2] \
            if self.compare is not None else (self.H, self.W)
        self._fps_key = ()
        with torch.cuda.device(self.device):
            need = int(_lib.load().rv_overlay_ws_bytes(self.S, self.dmax))
            if need == 0:
                raise ValueError(f"{self.S} streams x {self.dmax} detections: out of range")
            self.lists = torch.zeros((max(1, int(slots)), need), dtype=torch.uint8, device=self.device)
            self.names = _upload(table if self.nc else np.zeros((1, dlist.NAME_BYTES), np.uint8),
                                 self.device)
            self._canvas = self._canvas_list(None)

    def _canvas_list(self, fps: Optional[float]) -> Optional[torch.Tensor]:
        if self.compare is None:
            return None
        labels = dlist.canvas_list(self.H, self.W, self.layout_code, self.divider_px,
                                   str(self.compare.get("label_raw", "RAW")),
                                   str(self.compare.get("label_proc", "PROC")), fps, True)
        return _upload(labels.to_bytes(dlist.CANVAS_PRIMS), self.device)

    def layout(self, dets: torch.Tensor, det_n: torch.Tensor, track_id: torch.Tensor,
               distance_m: torch.Tensor, speed_kmh: torch.Tensor, slot: int = 0) -> None:
        """Display lists of one step's device results into list slot `slot`
        (current stream)."""
        if tuple(dets.shape) != (self.S, self.dmax, 6) or dets.dtype != torch.float32:
            raise ValueError(f"dets must be ({self.S}, {self.dmax}, 6) float32")
        for t, dt, what in ((det_n, torch.int32, "det_n"), (track_id, torch.int32, "track_id"),
                            (distance_m, torch.float64, "distance_m"),
                            (speed_kmh, torch.float64, "speed_kmh")):
            if t.dtype != dt or not t.is_contiguous() or \
                    t.numel() != (self.S if what == "det_n" else self.S * self.dmax):
                raise ValueError(f"{what}: expected a contiguous {dt} tensor of this batch")
        lists = self.lists[slot]
        with torch.cuda.device(self.device):
            call("rv_overlay_layout", ptr(dets.contiguous()), ptr(det_n), ptr(track_id),
                 ptr(distance_m), ptr(speed_kmh), self.S, self.dmax, self.H, self.W,
                 ptr(self.names), self.nc, self.thickness, self.k, ptr(lists), lists.numel(),
                 stream_ptr())

    def raster(self, proc: torch.Tensor, raw: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, slot: Optional[int] = 0,
               fps: Optional[float] = None) -> torch.Tensor:
        """proc (and raw, for a compare renderer) + list slot `slot` (None:
        no detections) -> out, on the current stream.  fps: the canvas's
        "FPS: x.y" label, formatted on the host."""
        canvas = self._canvas
        if self.compare is not None and fps is not None:
            canvas = self._canvas_list(float(fps))
        return raster(proc, raw, self.layout_code, self.divider_px,
                      None if slot is None else self.lists[slot], self.dmax, canvas, out)

    def render(self, dets, det_n, track_id, distance_m, speed_kmh, proc, raw=None, out=None,
               slot: int = 0, fps: Optional[float] = None) -> torch.Tensor:
        """layout + raster on the current stream."""
        self.layout(dets, det_n, track_id, distance_m, speed_kmh, slot)
        return self.raster(proc, raw, out, slot, fps)

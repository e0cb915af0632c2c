"""Display lists on the host: the reference's draw_detections
(src/vis/draw.py:25-102) and make_canvas labels (main_preview.py:12-34) as
records of the raster model of include/rvhip.h ("Detection overlays").

Nothing here touches the GPU.  ``detection_list`` is what ``draw_detections``
uploads, and the yardstick for the device layout kernel (rv_overlay_layout):
both must produce the same bytes.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

FILL, OUTLINE, TEXT = 1, 2, 3
TEXT_BYTES = 64
HEADER_BYTES = 16
CANVAS_PRIMS = 8
NAME_BYTES = 32
MAX_TEXT_THICKNESS = 32

# rv_overlay_prim (include/rvhip.h)
PRIM = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                 ("b", "u1"), ("g", "u1"), ("r", "u1"), ("thickness", "u1"), ("scale", "u1"),
                 ("len", "u1"), ("pad", "u1", (2,)), ("text", "u1", (TEXT_BYTES,)),
                 ("reserved", "<i4")])
assert PRIM.itemsize == 96

# src/vis/draw.py:11-22
COLOR_TABLE: Tuple[Tuple[int, int, int], ...] = (
    (255, 128, 64), (0, 255, 255), (80, 175, 76), (255, 0, 255), (0, 128, 255),
    (255, 64, 64), (64, 255, 64), (128, 128, 255), (255, 200, 0), (0, 255, 128))
WHITE = (255, 255, 255)
DIVIDER = (40, 40, 40)


def glyph_scale(font_scale: float) -> int:
    """cv2's font_scale -> the bitmap font's integer scale k (0.6 -> 2: 14 px
    capitals against Hershey's 13)."""
    return max(1, min(8, int(float(font_scale) * 22 / 7 + 0.5)))


def text_size(text: str, k: int) -> Tuple[Tuple[int, int], int]:
    """cv2.getTextSize of the raster model: ((width, height), baseline)."""
    return (6 * k * len(text.encode("utf-8")), 9 * k), 2 * k


def capacity(dmax: int) -> int:
    return 5 * int(dmax) + 8


def list_bytes(dmax: int) -> int:
    return HEADER_BYTES + capacity(dmax) * PRIM.itemsize


class DisplayList:
    """Primitives in painter's order."""

    def __init__(self):
        self._rows: List[tuple] = []

    def __len__(self):
        return len(self._rows)

    def fill(self, p0, p1, color) -> None:
        self._rows.append((FILL, int(p0[0]), int(p0[1]), int(p1[0]), int(p1[1]), color, 0, 0, b""))

    def outline(self, p0, p1, color, thickness: int) -> None:
        if not 1 <= thickness <= 255:
            raise ValueError(f"outline thickness {thickness} not in 1..255")
        self._rows.append((OUTLINE, int(p0[0]), int(p0[1]), int(p1[0]), int(p1[1]), color,
                           int(thickness), 0, b""))

    def text(self, text: str, org, k: int, color, thickness: int) -> None:
        """A string at origin `org`; one record per 64 bytes of it."""
        if not 1 <= thickness <= MAX_TEXT_THICKNESS:
            raise ValueError(f"text thickness {thickness} not in 1..{MAX_TEXT_THICKNESS}")
        if not 1 <= k <= 8:
            raise ValueError(f"glyph scale {k} not in 1..8")
        data = text.encode("utf-8")
        for i in range(0, len(data), TEXT_BYTES):
            self._rows.append((TEXT, int(org[0]) + 6 * k * i, int(org[1]), 0, 0, color,
                               int(thickness), int(k), data[i:i + TEXT_BYTES]))

    def records(self) -> np.ndarray:
        out = np.zeros(len(self._rows), PRIM)
        for r, (kind, x0, y0, x1, y1, color, t, k, data) in zip(out, self._rows):
            r["kind"], r["x0"], r["y0"], r["x1"], r["y1"] = kind, x0, y0, x1, y1
            r["b"], r["g"], r["r"] = color
            r["thickness"], r["scale"], r["len"] = t, k, len(data)
            r["text"][:len(data)] = np.frombuffer(data, np.uint8)
        return out

    def to_bytes(self, cap: Optional[int] = None) -> np.ndarray:
        """The list as the device reads it: the header and the records; with
        `cap`, padded with zeros to that many records."""
        n = len(self._rows)
        if cap is not None and n > cap:
            raise ValueError(f"{n} primitives exceed the list's capacity of {cap}")
        out = np.zeros(HEADER_BYTES + (n if cap is None else cap) * PRIM.itemsize, np.uint8)
        out[:4] = np.frombuffer(np.int32(n).tobytes(), np.uint8)
        out[HEADER_BYTES:HEADER_BYTES + n * PRIM.itemsize] = self.records().view(np.uint8)
        return out


def _label_top(dl: DisplayList, text: str, topleft, color, k: int, thickness: int) -> None:
    # draw.py:59-79
    if not text:
        return
    x, y = int(max(0, topleft[0])), int(max(0, topleft[1]))
    (tw, th), baseline = text_size(text, k)
    pad = 2
    box_top = max(0, y - th - baseline - pad * 2)
    dl.fill((x, box_top), (x + tw + pad * 2, y), color)
    dl.text(text, (x + pad, max(box_top + th, pad + th)), k, WHITE, max(1, thickness - 1))


def _label_bottom(dl: DisplayList, text: str, bottomleft, color, k: int, thickness: int,
                  img_h: int) -> None:
    # draw.py:82-102
    if not text:
        return
    x, y = int(max(0, bottomleft[0])), int(max(0, bottomleft[1]))
    (tw, th), baseline = text_size(text, k)
    pad = 2
    box_top = min(max(0, y), img_h - th - baseline - pad * 2)
    box_bottom = min(img_h, box_top + th + baseline + pad * 2)
    dl.fill((x, box_top), (x + tw + pad * 2, box_bottom), color)
    dl.text(text, (x + pad, min(img_h - baseline - 1, box_top + th + baseline)), k, WHITE,
            max(1, thickness - 1))


def detection_list(detections: Iterable, img_h: int, thickness: int = 2,
                   font_scale: float = 0.6) -> DisplayList:
    """draw_detections (draw.py:25-56) for an image of `img_h` rows."""
    dl = DisplayList()
    k = glyph_scale(font_scale)
    thickness = max(1, int(thickness))
    for det in detections:
        if det is None:
            continue
        color = COLOR_TABLE[det.cls_id % len(COLOR_TABLE)]
        x1, y1, x2, y2 = map(int, [det.x1, det.y1, det.x2, det.y2])
        if x2 <= x1 or y2 <= y1:
            continue
        dl.outline((x1, y1), (x2, y2), color, thickness)
        cls_name = det.cls_name or str(det.cls_id)
        label_main = f"{cls_name} {det.conf:.2f}" if det.conf is not None else cls_name
        if det.track_id is not None:
            label_main = f"ID {det.track_id} | {label_main}"
        _label_top(dl, label_main, (x1, y1), color, k, thickness)
        metrics = []
        if det.distance_m is not None:
            metrics.append(f"{det.distance_m:.1f} m")
        if det.speed_kmh is not None:
            metrics.append(f"{det.speed_kmh:.1f} km/h")
        if metrics:
            _label_bottom(dl, " / ".join(metrics), (x1, y2 + 4), color, k, thickness, img_h)
    return dl


def canvas_geometry(h: int, w: int, layout: str = "h", divider_px: int = 4):
    """(out_h, out_w, pane_x, pane_y, divider) of make_canvas for h x w frames."""
    d = max(0, int(divider_px))
    if str(layout).lower() == "v":
        return 2 * h + d, w, 0, h + d, d
    return h, 2 * w + d, w + d, 0, d


def canvas_list(h: int, w: int, layout: str = "h", divider_px: int = 4, label_raw: str = "RAW",
                label_proc: str = "PROC", fps: Optional[float] = None,
                show_fps: bool = True) -> DisplayList:
    """The labels make_canvas (main_preview.py:17-33) puts on the canvas of
    two h x w frames: each a black thickness-3 text under a coloured
    thickness-2 one."""
    dl = DisplayList()
    k = glyph_scale(0.8)
    _, _, px, py, _ = canvas_geometry(h, w, layout, divider_px)

    def put_label(org, text, color=(50, 220, 50)):
        dl.text(text, org, k, (0, 0, 0), 3)
        dl.text(text, org, k, color, 2)

    put_label((10, 30), label_raw)
    put_label((px + 10, py + 30), label_proc, color=(0, 200, 255))
    if show_fps and fps is not None:
        put_label((10, max(60, h - 10)), f"FPS: {fps:.1f}", color=(0, 255, 255))
    if len(dl) > CANVAS_PRIMS:
        raise ValueError(f"canvas labels of {len(dl)} records exceed {CANVAS_PRIMS}: "
                         "a label is longer than 64 bytes")
    return dl


def names_table(names: Sequence, nc: Optional[int] = None) -> np.ndarray:
    """Class names -> the device table of rv_overlay_layout: (nc, 32) u8,
    NUL-terminated UTF-8.  `names` is a list or an {id: name} mapping; a
    missing or empty name draws str(class id)."""
    if isinstance(names, dict):
        n = int(nc) if nc is not None else (max(names) + 1 if names else 0)
        items = [names.get(i, "") for i in range(n)]
    else:
        items = list(names)
        n = int(nc) if nc is not None else len(items)
        items = (items + [""] * n)[:n]
    table = np.zeros((max(n, 1), NAME_BYTES), np.uint8)
    for i, name in enumerate(items):
        data = str(name if name is not None else "").encode("utf-8")
        if len(data) > NAME_BYTES - 1:
            raise ValueError(f"class name {name!r} is longer than {NAME_BYTES - 1} bytes")
        table[i, :len(data)] = np.frombuffer(data, np.uint8)
    return table[:n] if n else table[:0]

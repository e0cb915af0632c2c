"""A numpy stand-in for the cv2 calls of the reference's drawing code
(src/vis/draw.py, main_preview.py's make_canvas): rectangle, getTextSize and
putText, per the raster model of include/rvhip.h ("Detection overlays").
Sequential, one primitive at a time, written independently of the kernel: an
outline is its four edge lines, a thick text a loop over shifted copies.

The font comes from tests/golden/overlay/font.npz (Pillow's built-in bitmap
font), not from csrc/overlay_font.h: the tests check one against the other.
"""
import os

import numpy as np

FONT_HERSHEY_SIMPLEX = 0
LINE_AA = 16
LINE_8 = 8
FILLED = -1

_FONT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay",
                          "font.npz")
_font = None


def font_rows():
    """(95, 11) u8: one byte per cell row of ASCII 32..126, bit 5 = leftmost."""
    global _font
    if _font is None:
        _font = np.load(_FONT_PATH)["rows"]
        assert _font.shape == (95, 11) and _font.dtype == np.uint8
    return _font


def glyph_scale(font_scale):
    return max(1, min(8, int(font_scale * 22 / 7 + 0.5)))


def _bytes(text):
    return text.encode("utf-8") if isinstance(text, str) else bytes(text)


def fill_rect(img, x0, y0, x1, y1, color):
    H, W = img.shape[:2]
    xa, xb = max(min(x0, x1), 0), min(max(x0, x1), W - 1)
    ya, yb = max(min(y0, y1), 0), min(max(y0, y1), H - 1)
    if xa <= xb and ya <= yb:
        img[ya:yb + 1, xa:xb + 1] = np.asarray(color, np.uint8)


def outline_rect(img, x0, y0, x1, y1, color, t):
    x0, x1 = min(x0, x1), max(x0, x1)
    y0, y1 = min(y0, y1), max(y0, y1)
    a, b = t // 2, (t - 1) // 2
    fill_rect(img, x0 - a, y0 - a, x1 + b, y0 + b, color)  # top
    fill_rect(img, x0 - a, y1 - a, x1 + b, y1 + b, color)  # bottom
    fill_rect(img, x0 - a, y0 - a, x0 + b, y1 + b, color)  # left
    fill_rect(img, x1 - a, y0 - a, x1 + b, y1 + b, color)  # right


def draw_text(img, data, ox, oy, k, color, t):
    """`data` bytes at origin (ox, oy), glyph scale k, thickness t."""
    rows = font_rows()
    H, W = img.shape[:2]
    color = np.asarray(color, np.uint8)
    t = min(max(1, t), 32)
    lo, hi = (t - 1) // 2, t // 2
    top = oy - 9 * k + 1
    for i, ch in enumerate(data):
        if ch < 32 or ch > 126:
            ch = ord("?")
        for r in range(11):
            for c in range(6):
                if not (rows[ch - 32, r] >> (5 - c)) & 1:
                    continue
                bx, by = ox + 6 * k * i + k * c, top + k * r  # the bit's k x k block
                for dy in range(-lo, hi + 1):
                    for dx in range(-lo, hi + 1):
                        fill_rect(img, bx + dx, by + dy, bx + dx + k - 1, by + dy + k - 1, color)


def rectangle(img, pt1, pt2, color, thickness=1, lineType=LINE_8, shift=0):
    if thickness < 0:
        fill_rect(img, int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1]), color)
    else:
        outline_rect(img, int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1]), color,
                     max(1, int(thickness)))
    return img


def getTextSize(text, fontFace, fontScale, thickness):
    k = glyph_scale(fontScale)
    return (6 * k * len(_bytes(text)), 9 * k), 2 * k


def putText(img, text, org, fontFace, fontScale, color, thickness=1, lineType=LINE_8,
            bottomLeftOrigin=False):
    draw_text(img, _bytes(text), int(org[0]), int(org[1]), glyph_scale(fontScale), color,
              int(thickness))
    return img


def raster_records(img, records):
    """A display list's records (rvs_amd.vis.display_list.PRIM) onto img, in order."""
    for r in records:
        color = (int(r["b"]), int(r["g"]), int(r["r"]))
        x0, y0, x1, y1 = int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])
        if r["kind"] == 1:
            fill_rect(img, x0, y0, x1, y1, color)
        elif r["kind"] == 2:
            outline_rect(img, x0, y0, x1, y1, color, max(1, int(r["thickness"])))
        elif r["kind"] == 3:
            draw_text(img, bytes(r["text"][:int(r["len"])]), x0, y0, int(r["scale"]), color,
                      int(r["thickness"]))
    return img

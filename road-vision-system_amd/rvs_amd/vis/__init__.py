"""The reference's ``src/vis`` surface for device frames: detection overlays
and the RAW | PROC compare canvas, drawn by HIP kernels (csrc/overlay.hip)."""
from .display_list import (COLOR_TABLE, DisplayList, canvas_list, detection_list, glyph_scale,
                           names_table, text_size)
from .overlay import OverlayRenderer, draw_detections, make_canvas, raster

__all__ = ["COLOR_TABLE", "DisplayList", "OverlayRenderer", "canvas_list", "detection_list",
           "draw_detections", "glyph_scale", "make_canvas", "names_table", "raster", "text_size"]

"""Capture front end (src/io_video)."""
from .capture import (Frame, MultiStreamCapture, VideoSource, decode_jpeg, jpeg_coefficients,
                      jpeg_probe, jpeg_record_layout, write_y4m)

__all__ = ["Frame", "MultiStreamCapture", "VideoSource", "decode_jpeg", "jpeg_coefficients",
           "jpeg_probe", "jpeg_record_layout", "write_y4m"]

"""Capture front end (src/io_video) and the Motion-JPEG sink."""
from .capture import (Frame, MultiStreamCapture, VideoSource, decode_jpeg, jpeg_coefficients,
                      jpeg_probe, jpeg_record_layout, write_y4m)
from .sink import MultiStreamSink, VideoSink, encode_jpeg, record_settings

__all__ = ["Frame", "MultiStreamCapture", "VideoSource", "decode_jpeg", "jpeg_coefficients",
           "jpeg_probe", "jpeg_record_layout", "write_y4m", "MultiStreamSink", "VideoSink",
           "encode_jpeg", "record_settings"]

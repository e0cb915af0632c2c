"""Tracker factory (mirrors src/track/registry.py:10-14): 'sort' (the
reference's name) and 'sort_hip' build the gfx950 SORT tracker; 'bytetrack',
'byte' and 'bytetrack_hip' build the same tracker with ByteTrack's second
association on low-score detections (track/byte_hip.py)."""
from typing import Any, Dict

from .base import Tracker

SORT_BACKENDS = ("sort", "sort_hip")
BYTE_BACKENDS = ("bytetrack", "byte", "bytetrack_hip")


def backend_name(cfg: Dict[str, Any]) -> str:
    return str(cfg.get("backend") or "sort").lower()


def build_tracker(cfg: Dict[str, Any]) -> Tracker:
    backend = backend_name(cfg)
    if backend in SORT_BACKENDS:
        from .sort_hip import SortTracker
        return SortTracker(cfg)
    if backend in BYTE_BACKENDS:
        from .byte_hip import ByteTracker
        return ByteTracker(cfg)
    raise ValueError(f"unknown tracker backend: {backend}")

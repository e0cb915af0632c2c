"""HIP preprocess ops (drop-in for src/preprocess/ops/*.py and ops_cuda/*.py).

``CLAHEDehaze`` restates clahe_dehaze.py:13-32 and ``MedianDerain`` restates
median_derain.py:10-14 on the gfx950 kernels of csrc/clahe.hip and median.hip.  Parameter
parsing follows the reference line by line (grid clamp, ksize normalisation).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import kernels
from .base import PreprocessOp


def clahe_params(params):
    """(space, clip_limit, grid) exactly as clahe_dehaze.py:14-17 parses them."""
    space = str(params.get("space", "YCrCb")).upper()
    clip_limit = float(params.get("clip_limit", 2.0))
    grid = int(params.get("tile_grid", 8))
    grid = max(2, grid)
    return space, clip_limit, grid


def median_ksize(params):
    """ksize normalisation of median_derain.py:11-13."""
    k = int(params.get("ksize", 3))
    if k % 2 == 0:
        k += 1
    k = max(3, min(k, 9))
    return k


def dcp_params(params):
    """(patch, wq, tq, radius, eq): DarkChannelDehaze's parameters as the
    integers rv_dcp_dehaze_u8 takes.  patch odd in [3, 31]; omega in 1/256;
    t_min in 1/255; refine_radius in [0, 64] (0: no refinement); eps (on
    gray in [0, 1]) in 1/65025."""
    p = int(params.get("patch", 15))
    if p % 2 == 0:
        p += 1
    p = max(3, min(p, 31))
    wq = min(256, max(1, int(float(params.get("omega", 0.95)) * 256 + 0.5)))
    tq = min(255, max(1, int(float(params.get("t_min", 0.1)) * 255 + 0.5)))
    r = min(64, max(0, int(params.get("refine_radius", 40))))
    eq = min(1 << 20, max(1, int(float(params.get("eps", 1e-3)) * 65025 + 0.5)))
    return p, wq, tq, r, eq


def streak_params(params):
    """(width, min_len, max_len, slant, thr): StreakDerain's parameters as the
    integers rv_streak_derain_u8 takes.  width odd in [3, 15]; min_len odd in
    [3, 33]; max_len 0 (off) or odd in [min_len + 2, 97]; slant in [-4, 4]
    quarter pixels of x per row; thresh in [1, 255].  An even size goes up to
    the next odd one."""
    def odd(v, lo, hi):
        v = int(v)
        if v % 2 == 0:
            v += 1
        return max(lo, min(v, hi))
    w = odd(params.get("width", 3), 3, 15)
    lo = odd(params.get("min_len", 9), 3, 33)
    hi = int(params.get("max_len", 0))
    hi = 0 if hi <= 0 else odd(hi, lo + 2, 97)
    slant = max(-4, min(int(params.get("slant", 0)), 4))
    thr = max(1, min(int(params.get("thresh", 20)), 255))
    return w, lo, hi, slant, thr


def _to_device(image):
    """np.ndarray (H,W,3) u8 -> (device tensor, was_numpy)."""
    if isinstance(image, torch.Tensor):
        return image, False
    arr = np.ascontiguousarray(image)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"expected BGR uint8 (H,W,3), got {arr.shape} {arr.dtype}")
    return torch.from_numpy(arr).cuda(), True


def _back(t, was_numpy):
    return t.cpu().numpy() if was_numpy else t


class CLAHEDehaze(PreprocessOp):
    """CLAHE on the luma channel, HIP kernels: YCrCb (default) or LAB
    (clahe_dehaze.py:21-30; any space other than "LAB" takes YCrCb)."""

    def __init__(self, **params):
        super().__init__(**params)
        self.space, self.clip_limit, self.grid = clahe_params(self.params)
        self._ws = None

    def __call__(self, image):
        x, was_np = _to_device(image)
        B = 1 if x.dim() == 3 else x.shape[0]
        need = kernels.clahe_ws_bytes(B, self.grid)
        if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        fn = kernels.clahe_lab if self.space == "LAB" else kernels.clahe_ycrcb
        out = fn(x, self.grid, self.clip_limit, ws=self._ws)
        return _back(out, was_np)


class MedianDerain(PreprocessOp):
    """Exact k x k median, replicated borders, HIP kernel."""

    def __init__(self, **params):
        super().__init__(**params)
        self.k = median_ksize(self.params)

    def __call__(self, image):
        x, was_np = _to_device(image)
        return _back(kernels.median(x, self.k), was_np)


class DarkChannelDehaze(PreprocessOp):
    """Dark-channel-prior dehaze (He, Sun, Tang): the inverse of the fog model
    I = J t + A (1 - t) that augment.fog synthesises, with a guided-filter
    refinement of the transmission; integer arithmetic, HIP kernels
    (csrc/dehaze.hip).  params: patch, omega, t_min, refine_radius, eps."""

    def __init__(self, **params):
        super().__init__(**params)
        self.patch, self.wq, self.tq, self.radius, self.eq = dcp_params(self.params)
        self._ws = None

    def __call__(self, image):
        x, was_np = _to_device(image)
        B = 1 if x.dim() == 3 else x.shape[0]
        need = kernels.dcp_ws_bytes(B, x.shape[-3], x.shape[-2], self.radius)
        if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
            self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
        out = kernels.dcp_dehaze(x, self.patch, self.wq, self.tq, self.radius, self.eq,
                                 ws=self._ws)
        return _back(out, was_np)


class StreakDerain(PreprocessOp):
    """Directional rain-streak removal, HIP kernels (csrc/derain.hip), integer
    arithmetic: a horizontal white top-hat of the gray finds bright runs
    narrower than `width`, an opening along a line of `slant` quarter pixels
    of x per row keeps those at least `min_len` rows long, and the pixel is
    recovered by the exact inverse of the rain model I' = I + (255 - I) a; a
    rain-free frame comes back byte for byte.  params: width (3), min_len (9),
    max_len (0), slant (0), thresh (20).  augment.fog's streaks are slant -1.

    Measured on tests/streak_ref.py with the oracle's rain: on
    noisy frames without thin structures, max_len 0 brings the frame to
    42-56 dB of the rain-free one (rainy 26-36 dB, its 3x3 median 30-33 dB).
    max_len > 0 keeps structures at least that long along the slant (lane
    markings, poles): on frames with thin bright lines max_len 49 is about
    5 dB better than 0 at rain_p 0.01 and 2 dB better to 2 dB worse at 0.03,
    and without such lines it costs 6 to 11 dB, because dense rain forms
    false long chains; hence the default 0.  A slant of the wrong sign gains
    under 1.6 dB: the direction is a parameter, not estimated.  A chain may
    hold two ops with different slants."""

    def __init__(self, **params):
        super().__init__(**params)
        self.width, self.min_len, self.max_len, self.slant, self.thr = streak_params(self.params)
        self._ws = None

    def __call__(self, image):
        x, was_np = _to_device(image)
        B = 1 if x.dim() == 3 else x.shape[0]
        need = kernels.streak_ws_bytes(B, x.shape[-3], x.shape[-2], self.max_len)
        if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
            self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
        out = kernels.streak_derain(x, self.width, self.min_len, self.max_len, self.slant,
                                    self.thr, ws=self._ws)
        return _back(out, was_np)


# The reference registers its OpenCV-CUDA variants under these names
# (src/preprocess/registry.py:19-23); on MI355X they are the same HIP ops.
HIPCLAHEDehaze = CLAHEDehaze
HIPMedianDerain = MedianDerain
CUDACLAHEDehaze = CLAHEDehaze
CUDAMedianDerain = MedianDerain
DCPDehaze = DarkChannelDehaze
HIPDarkChannelDehaze = DarkChannelDehaze
HIPStreakDerain = StreakDerain

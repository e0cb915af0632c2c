"""PreprocessPipeline (mirrors src/preprocess/pipeline.py:7-45).

Same config keys and control flow as the reference: ``enabled``, ``chain``
(list of {name, params}), ``auto_gate`` {enable_low_contrast_gate,
contrast_thresh}.  When the chain is exactly [CLAHEDehaze(YCrCb),
MedianDerain] -- configs/default.yaml:21-31 -- it runs the fused HIP pass
(rv_clahe_median_u8), which is bit-identical to running the two ops in turn.

Every chain made of the built-in ops (at most four of them, in any order)
also has a host descriptor (``chain_desc``): ``run_chain_with_letterbox`` runs
it, the low-contrast gate and the detector's LetterBox through
rv_preprocess_chain_u8 -- stream-ordered launches only, the gate evaluated on
the device -- which is what a recorded schedule needs.
"""
from __future__ import annotations

from typing import Any, Dict

import numpy as np
import torch

from .. import kernels
from .ops import (CLAHEDehaze, DarkChannelDehaze, MedianDerain, StreakDerain, _back,
                  _to_device)
from .registry import get_op_class


class PreprocessPipeline:
    def __init__(self, config: Dict[str, Any]):
        self.enabled = bool(config.get("enabled", True))
        self.chain_cfg = config.get("chain", []) or []
        self.auto_gate_cfg = config.get("auto_gate", {}) or {}
        self.ops = []
        for node in self.chain_cfg:
            name = node.get("name")
            params = node.get("params", {})
            cls = get_op_class(name)
            self.ops.append(cls(**params))
        # the fused CLAHE+median passes are YCrCb-only; a LAB chain runs op by op
        self._fused = (len(self.ops) == 2 and isinstance(self.ops[0], CLAHEDehaze)
                       and self.ops[0].space != "LAB" and isinstance(self.ops[1], MedianDerain))
        self._ws = None
        # host descriptor of the chain for rv_preprocess_chain_u8; None when
        # the chain holds an op the library does not know (unsupported_op
        # names it) or more ops than the descriptor has room for
        self.chain_desc, self.unsupported_op = self._build_desc()
        self._chain_ws = None

    def _build_desc(self):
        ops = []
        for node, op in zip(self.chain_cfg, self.ops):
            if type(op) is CLAHEDehaze:
                ops.append(("clahe", op.space, op.grid, op.clip_limit))
            elif type(op) is MedianDerain:
                ops.append(("median", op.k))
            elif type(op) is DarkChannelDehaze:
                ops.append(("dcp", op.patch, op.wq, op.tq, op.radius, op.eq))
            elif type(op) is StreakDerain:
                ops.append(("streak", op.width, op.min_len, op.max_len, op.slant, op.thr))
            else:
                return None, str(node.get("name"))
        if len(ops) > kernels.CHAIN_MAX_OPS:
            return None, f"{len(ops)} ops (the chain descriptor holds {kernels.CHAIN_MAX_OPS})"
        return kernels.chain_desc(ops, self.enabled, self._gate_enabled(),
                                  float(self.auto_gate_cfg.get("contrast_thresh", 20.0))), None

    @property
    def chain_supported(self) -> bool:
        return self.chain_desc is not None

    def chain_route(self, H: int, W: int, geo=None) -> int:
        """kernels.ROUTE_* of this chain on H x W frames (a host query)."""
        return kernels.preprocess_chain_route(self.chain_desc, H, W, geo)

    def run_chain_with_letterbox(self, x: torch.Tensor, geo=None, lb_out: torch.Tensor = None,
                                 out: torch.Tensor = None):
        """(B,H,W,3) device frames -> (proc, letterboxed proc) for any
        supported chain, the gate included, without a host read or an
        allocation once the workspace has its size; byte-identical to
        self(x) followed by the detector's letterbox.  geo None: (proc, None)."""
        if self.chain_desc is None:
            raise ValueError(f"preprocess chain not supported by rv_preprocess_chain_u8: "
                             f"{self.unsupported_op}")
        B, H, W = x.shape[0], x.shape[1], x.shape[2]
        need = kernels.preprocess_chain_ws_bytes(self.chain_desc, B, H, W, x.stride(1))
        if self._chain_ws is None or self._chain_ws.numel() < need or \
                self._chain_ws.device != x.device:
            self._chain_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
        return kernels.preprocess_chain(x, self.chain_desc, geo, out=out, lb_out=lb_out,
                                        ws=self._chain_ws)

    def _gate_enabled(self) -> bool:
        return bool(self.auto_gate_cfg.get("enable_low_contrast_gate", False))

    def low_contrast_mask(self, frames: torch.Tensor) -> torch.Tensor:
        """Per-frame `span < contrast_thresh` (pipeline.py:24-30) on device."""
        thresh = float(self.auto_gate_cfg.get("contrast_thresh", 20.0))
        span = kernels.gray_span(frames)
        return span.float() < thresh

    def _run_chain(self, x: torch.Tensor) -> torch.Tensor:
        if self._fused:
            clahe, med = self.ops
            B = 1 if x.dim() == 3 else x.shape[0]
            need = kernels.clahe_ws_bytes(B, clahe.grid)
            if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
            if kernels.clahe_median_fits(x, clahe.grid, med.k):
                return kernels.clahe_median(x, clahe.grid, clahe.clip_limit, med.k, ws=self._ws)
            # very fine grids: the LUT window exceeds LDS; the unfused pair
            # gives the identical result.
        out = x
        for op in self.ops:
            out = op(out)
        return out

    def __call__(self, image, ts: float = None):
        if not self.enabled or not self.ops:
            return image
        x, was_np = _to_device(image)
        if self._gate_enabled():
            low = self.low_contrast_mask(x)
            if x.dim() == 3:
                if not bool(low[0]):
                    return image  # contrast is sufficient -> skip the chain
                return _back(self._run_chain(x), was_np)
            # per frame, as the reference's per-frame loop does: only the
            # low-contrast frames run the chain (gathered into one batch, one
            # host read of the gate); the others pass through unchanged
            sel = torch.nonzero(low).flatten()
            n = int(sel.numel())
            if n == 0:
                return image
            if n == x.shape[0]:
                return _back(self._run_chain(x), was_np)
            out = x.clone()
            out.index_copy_(0, sel, self._run_chain(x.index_select(0, sel).contiguous()))
            return _back(out, was_np)
        return _back(self._run_chain(x), was_np)

"""Functional torch-tensor front end over the C ABI (include/rvhip.h).

Every function takes device-resident uint8 BGR frames shaped (B, H, W, 3)
(or (H, W, 3)), launches on the current torch stream and returns device
tensors.  Nothing here copies to the host or synchronises.
"""
from __future__ import annotations

import ctypes
import struct
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr


def _frames(x: torch.Tensor) -> Tuple[torch.Tensor, int, int, int, int]:
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[-1] != 3 or x.dtype != torch.uint8:
        raise ValueError(f"expected uint8 frames (B,H,W,3), got {tuple(x.shape)} {x.dtype}")
    if not x.is_cuda:
        raise ValueError("frames must be on the GPU (HIP path has no CPU fallback)")
    B, H, W, _ = x.shape
    if not (x.stride(3) == 1 and x.stride(2) == 3 and x.stride(0) == H * x.stride(1)):
        x = x.contiguous()
    pitch = x.stride(1)
    return x, B, H, W, pitch


def _like(x: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    """Output frames with the same (B, H, pitch) layout as the input: the ABI
    takes one pitch for both."""
    if out is None:
        return torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    if out.shape != x.shape or out.stride() != x.stride():
        raise ValueError("out must have the input's shape and strides")
    return out


def clahe_ws_bytes(B: int, tiles: int) -> int:
    return int(_lib.load().rv_clahe_ws_bytes(B, tiles))


def _workspace(ws: Optional[torch.Tensor], need: int, device) -> torch.Tensor:
    """ws if it holds `need` bytes, else a new buffer that does."""
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    return ws


def clahe_ycrcb(frames: torch.Tensor, tiles: int = 8, clip: float = 2.0,
                out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    x, B, H, W, pitch = _frames(frames)
    out = _like(x, out)
    ws = _workspace(ws, clahe_ws_bytes(B, tiles), x.device)
    call("rv_clahe_ycrcb_u8", ptr(x), ptr(out), B, H, W, pitch, int(tiles), float(clip),
         ptr(ws), ws.numel(), stream_ptr())
    return out if frames.dim() == 4 else out[0]


_lab_ready = set()  # devices whose Lab tables are uploaded


def _lab_tables(device) -> None:
    """The Lab tables, uploaded once per device: synchronous, so it happens
    before anything records."""
    if device not in _lab_ready:
        with torch.cuda.device(device):
            call("rv_lab_init")
        _lab_ready.add(device)


def clahe_lab(frames: torch.Tensor, tiles: int = 8, clip: float = 2.0,
              out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    """CLAHEDehaze space='LAB' (clahe_dehaze.py:21-25) on device frames."""
    x, B, H, W, pitch = _frames(frames)
    out = _like(x, out)
    ws = _workspace(ws, clahe_ws_bytes(B, tiles), x.device)
    _lab_tables(x.device)
    call("rv_clahe_lab_u8", ptr(x), ptr(out), B, H, W, pitch, int(tiles), float(clip),
         ptr(ws), ws.numel(), stream_ptr())
    return out if frames.dim() == 4 else out[0]


def nv12_to_bgr(nv12: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed NV12 frames (B, 3H/2, W) u8 on device (Y rows, then interleaved
    U,V rows) -> (B, H, W, 3) BGR, cv2.COLOR_YUV2BGR_NV12 bit for bit."""
    if nv12.dim() == 2:
        return nv12_to_bgr(nv12.unsqueeze(0), None if out is None else out.unsqueeze(0))[0]
    if nv12.dim() != 3 or nv12.dtype != torch.uint8 or not nv12.is_cuda:
        raise ValueError("expected packed NV12 uint8 (B, 3H/2, W) on the GPU")
    nv12 = nv12.contiguous()
    B, R, W = nv12.shape
    if R % 3 or (2 * R // 3) % 2 or W % 2:
        raise ValueError(f"NV12 rows {R} / width {W}: need 3H/2 rows with H, W even")
    H = 2 * R // 3
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=nv12.device)
    elif out.shape != (B, H, W, 3) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (B, H, W, 3) uint8 tensor")
    fs = R * W
    call("rv_nv12_to_bgr_u8", ptr(nv12), nv12.data_ptr() + H * W, W, W, fs, fs, ptr(out), B, H, W,
         3 * W, stream_ptr())
    return out


def jpeg_to_bgr(records: torch.Tensor, W: int, H: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """JPEG coefficient records (S, record bytes) u8 on device (what
    rv_jpeg_decode_coef and the MJPEG readers produce for W x H images; the
    records' sampling and quant tables may differ) -> (S, H, W, 3) BGR, bit
    for bit libjpeg's default decode in this sense: identical to libjpeg where
    its own builds agree (the 16-bit-safe domain, libjpeg16_safe in
    tests/jpeg_ref.py, which every encoder output of 8-bit pixels lies in), and
    a plain clamp beyond it.  Example: one grey block, DC only, quant entry
    255: a quantised DC of 32 decodes to 255 everywhere; 33 (8415 * 4 leaves
    int16) to 255 here and to 0 in libjpeg-turbo's SIMD build.
    A 1-D record gives one (H, W, 3) frame."""
    if records.dim() == 1:
        return jpeg_to_bgr(records.unsqueeze(0), W, H,
                           None if out is None else out.unsqueeze(0))[0]
    if records.dim() != 2 or records.dtype != torch.uint8 or not records.is_cuda:
        raise ValueError("expected JPEG coefficient records, uint8 (S, bytes), on the GPU")
    S = records.shape[0]
    stride = records.stride(0) if S > 1 else records.shape[1] // 16 * 16
    if records.stride(1) != 1 or stride % 16 or records.data_ptr() % 16:
        raise ValueError("records must be rows of bytes, 16-byte aligned with a 16-byte stride")
    if out is None:
        out = torch.empty((S, H, W, 3), dtype=torch.uint8, device=records.device)
    elif out.shape != (S, H, W, 3) or not out.is_contiguous() or out.dtype != torch.uint8:
        raise ValueError("out must be a contiguous (S, H, W, 3) uint8 tensor")
    call("rv_jpeg_coef_to_bgr_u8", ptr(records), stride, S, int(W), int(H), ptr(out),
         stream_ptr())
    return out


JPEG_SAMPLING = {"444": 0, "422": 1, "420": 2}
JPEG_STREAM_MAGIC, JPEG_STREAM_HEADER_BYTES = 0x534A5652, 16
JPEG_STREAM_OVERFLOW, JPEG_STREAM_BAD_RECORD = 1, 2


def jpeg_sampling_code(sampling) -> int:
    """"444" / "422" / "420" (or the RV_JPEG_* code itself) -> RV_JPEG_* code."""
    if isinstance(sampling, str):
        if sampling not in JPEG_SAMPLING:
            raise ValueError(f"JPEG sampling {sampling!r}: expected '444', '422' or '420'")
        return JPEG_SAMPLING[sampling]
    return int(sampling)


def jpeg_stream_bound(W: int, H: int, sampling) -> int:
    """Worst-case bytes of one encoded stream (rv_jpeg_stream_bound)."""
    n = int(_lib.load().rv_jpeg_stream_bound(int(W), int(H), jpeg_sampling_code(sampling)))
    if n == 0:
        raise ValueError(f"no JPEG stream bound for {W}x{H}, sampling {sampling!r}")
    return n


def jpeg_file_header(W: int, H: int, sampling, quality: int, restart_interval: int) -> bytes:
    """SOI .. SOS of a W x H image at `quality` (rv_jpeg_write_header, host)."""
    buf = ctypes.create_string_buffer(640)
    n = ctypes.c_size_t(0)
    call("rv_jpeg_write_header", int(W), int(H), jpeg_sampling_code(sampling), int(quality),
         int(restart_interval), ctypes.addressof(buf), 640, ctypes.addressof(n))
    return buf.raw[:n.value]


def bgr_to_jpeg_coef(frames: torch.Tensor, quality: int = 95, sampling="420",
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(S, H, W, 3) BGR u8 frames on device -> (S, record bytes) quantised DCT
    coefficient records (the layout jpeg_to_bgr reads), libjpeg's default
    forward path bit for bit."""
    x, S, H, W, pitch = _frames(frames)
    if pitch != 3 * W:
        x = x.contiguous()
    samp = jpeg_sampling_code(sampling)
    n = int(_lib.load().rv_jpeg_record_bytes(W, H, samp))
    if out is None:
        out = torch.empty((S, n), dtype=torch.uint8, device=x.device)
    elif out.shape != (S, n) or not out.is_contiguous() or out.dtype != torch.uint8:
        raise ValueError(f"out must be a contiguous ({S}, {n}) uint8 tensor")
    call("rv_jpeg_bgr_to_coef_u8", ptr(x), S, H, W, samp, int(quality), ptr(out), n, stream_ptr())
    return out


def _jpeg_streams(S, W, H, samp, capacity, out, device):
    stride = jpeg_stream_bound(W, H, samp) if out is None else out.stride(0)
    if out is None:
        out = torch.empty((S, stride), dtype=torch.uint8, device=device)
    elif out.dim() != 2 or out.shape[0] != S or out.stride(1) != 1 or out.dtype != torch.uint8:
        raise ValueError("out must be (S, stride) uint8 rows")
    cap = out.shape[1] if capacity is None else int(capacity)
    return out, stride, cap


def jpeg_coef_to_stream(records: torch.Tensor, W: int, H: int, sampling, quality: int,
                        capacity: Optional[int] = None, out: Optional[torch.Tensor] = None,
                        ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device coefficient records of W x H images (from bgr_to_jpeg_coef at
    `quality`) -> (S, stride) u8 streams: a 16-byte header {magic, image bytes,
    flags, segments} and the complete JPEG image.  At most `capacity` bytes of
    each stream are written."""
    samp = jpeg_sampling_code(sampling)
    if records.dim() != 2 or records.dtype != torch.uint8 or not records.is_cuda:
        raise ValueError("expected JPEG coefficient records, uint8 (S, bytes), on the GPU")
    S = records.shape[0]
    rstride = records.stride(0) if S > 1 else records.shape[1] // 16 * 16
    out, stride, cap = _jpeg_streams(S, W, H, samp, capacity, out, records.device)
    ws = _workspace(ws, int(_lib.load().rv_jpeg_stream_ws_bytes(S, W, H, samp)), records.device)
    fh = (1 if samp == 0 else 2) * 8
    hdr = jpeg_file_header(W, H, samp, quality, (W + fh - 1) // fh)
    call("rv_jpeg_coef_to_stream", ptr(records), rstride, S, int(W), int(H), samp, hdr, len(hdr),
         ptr(ws), ws.numel(), ptr(out), stride, cap, stream_ptr())
    return out


def jpeg_encode(frames: torch.Tensor, quality: int = 95, sampling="420",
                capacity: Optional[int] = None, out: Optional[torch.Tensor] = None,
                ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(S, H, W, 3) BGR u8 frames on device -> (S, stride) u8 streams
    (rv_jpeg_encode_bgr_u8; see jpeg_coef_to_stream).  Nothing is read back."""
    x, S, H, W, pitch = _frames(frames)
    if pitch != 3 * W:
        x = x.contiguous()
    samp = jpeg_sampling_code(sampling)
    out, stride, cap = _jpeg_streams(S, W, H, samp, capacity, out, x.device)
    ws = _workspace(ws, int(_lib.load().rv_jpeg_encode_ws_bytes(S, W, H, samp)), x.device)
    call("rv_jpeg_encode_bgr_u8", ptr(x), S, H, W, samp, int(quality), ptr(ws), ws.numel(),
         ptr(out), stride, cap, stream_ptr())
    return out


def median(frames: torch.Tensor, k: int = 3, out: Optional[torch.Tensor] = None):
    x, B, H, W, pitch = _frames(frames)
    out = _like(x, out)
    call("rv_median_u8c3", ptr(x), ptr(out), B, H, W, pitch, int(k), stream_ptr())
    return out if frames.dim() == 4 else out[0]


def clahe_median(frames: torch.Tensor, tiles: int = 8, clip: float = 2.0, k: int = 3,
                 out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    x, B, H, W, pitch = _frames(frames)
    out = _like(x, out)
    ws = _workspace(ws, clahe_ws_bytes(B, tiles), x.device)
    call("rv_clahe_median_u8", ptr(x), ptr(out), B, H, W, pitch, int(tiles), float(clip),
         int(k), ptr(ws), ws.numel(), stream_ptr())
    return out if frames.dim() == 4 else out[0]


def clahe_median_letterbox(frames: torch.Tensor, tiles: int, clip: float, k: int, geo,
                           out: Optional[torch.Tensor] = None,
                           lb_out: Optional[torch.Tensor] = None,
                           ws: Optional[torch.Tensor] = None):
    """Fused CLAHE + median + LetterBox: returns (proc, letterboxed)."""
    x, B, H, W, pitch = _frames(frames)
    out = _like(x, out)
    if lb_out is None:
        lb_out = torch.empty((B, geo[0], geo[1], 3), dtype=torch.uint8, device=x.device)
    ws = _workspace(ws, clahe_ws_bytes(B, tiles), x.device)
    call("rv_clahe_median_letterbox_u8", ptr(x), ptr(out), B, H, W, pitch, int(tiles),
         float(clip), int(k), ptr(ws), ws.numel(), ptr(lb_out), _lib.int_array(geo), stream_ptr())
    return (out if frames.dim() == 4 else out[0]), lb_out


def clahe_median_letterbox_fits(H: int, W: int, tiles: int, k: int, geo) -> bool:
    return bool(_lib.load().rv_clahe_median_letterbox_fits(H, W, int(tiles), int(k),
                                                           _lib.int_array(geo)))


def clahe_median_fits(frames: torch.Tensor, tiles: int, k: int) -> bool:
    H, W = frames.shape[-3], frames.shape[-2]
    return bool(_lib.load().rv_clahe_median_fits(H, W, int(tiles), int(k)))


def dcp_ws_bytes(B: int, H: int, W: int, radius: int) -> int:
    """Workspace bytes of rv_dcp_dehaze_u8 (0 for a bad shape or radius)."""
    return int(_lib.load().rv_dcp_ws_bytes(int(B), int(H), int(W), int(radius)))


def dcp_dehaze(frames: torch.Tensor, patch: int = 15, wq: int = 243, tq: int = 26,
               radius: int = 40, eq: int = 65, out: Optional[torch.Tensor] = None,
               ws: Optional[torch.Tensor] = None, air: bool = False, t: bool = False):
    """Dark-channel-prior dehaze (rv_dcp_dehaze_u8) of device frames with the
    normalised parameters of preprocess.ops.dcp_params (the defaults are that
    function's).  Returns the frames; with air and/or t also the (B, 5) int32
    {A_b, A_g, A_r, L, cnt} and the (B, H, W) uint8 transmission, in that
    order."""
    x, B, H, W, pitch = _frames(frames)
    out = _like(x, out)
    ws = _workspace(ws, dcp_ws_bytes(B, H, W, radius), x.device)
    air_t = torch.empty((B, 5), dtype=torch.int32, device=x.device) if air else None
    t_t = torch.empty((B, H, W), dtype=torch.uint8, device=x.device) if t else None
    call("rv_dcp_dehaze_u8", ptr(x), ptr(out), B, H, W, pitch, int(patch), int(wq), int(tq),
         int(radius), int(eq), ptr(ws), ws.numel(), ptr(air_t), ptr(t_t), stream_ptr())
    single = frames.dim() != 4
    res = [out[0] if single else out]
    if air:
        res.append(air_t[0] if single else air_t)
    if t:
        res.append(t_t[0] if single else t_t)
    return res[0] if len(res) == 1 else tuple(res)


def streak_ws_bytes(B: int, H: int, W: int, max_len: int) -> int:
    """Workspace bytes of rv_streak_derain_u8 (0 for a bad shape or max_len)."""
    return int(_lib.load().rv_streak_ws_bytes(int(B), int(H), int(W), int(max_len)))


def streak_derain(frames: torch.Tensor, width: int = 3, min_len: int = 9, max_len: int = 0,
                  slant: int = 0, thr: int = 20, out: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None, s: bool = False):
    """Directional rain-streak removal (rv_streak_derain_u8) of device frames
    with the normalised parameters of preprocess.ops.streak_params (the
    defaults are that function's).  Returns the frames; with s also the
    (B, H, W) uint8 streak plane S."""
    x, B, H, W, pitch = _frames(frames)
    out = _like(x, out)
    ws = _workspace(ws, streak_ws_bytes(B, H, W, max_len), x.device)
    s_t = torch.empty((B, H, W), dtype=torch.uint8, device=x.device) if s else None
    call("rv_streak_derain_u8", ptr(x), ptr(out), B, H, W, pitch, int(width), int(min_len),
         int(max_len), int(slant), int(thr), ptr(ws), ws.numel(), ptr(s_t), stream_ptr())
    single = frames.dim() != 4
    res = out[0] if single else out
    if s:
        return res, (s_t[0] if single else s_t)
    return res


CHAIN_DESC_BYTES = 120  # sizeof(rv_chain_desc), include/rvhip.h
CHAIN_MAX_OPS = 4
ROUTE_FUSED, ROUTE_FUSED_GATED, ROUTE_OPS = 0, 1, 2  # RV_CHAIN_ROUTE_*


def chain_desc(ops, enabled: bool = True, gate_on: bool = False, contrast_thresh: float = 20.0):
    """The host descriptor (rv_chain_desc) of a preprocess chain.  ops: a list
    of ("clahe", space, tiles, clip), ("median", k), ("dcp", patch, wq, tq,
    radius, eq) and ("streak", width, min_len, max_len, slant, thr) tuples
    holding the normalised parameters (preprocess.ops.clahe_params /
    median_ksize / dcp_params / streak_params).
    Nothing is validated here: the library checks the descriptor (n_ops,
    tiles, k, ...) and answers RV_EINVAL."""
    ops = list(ops)
    blob = struct.pack("<iiiid", int(bool(enabled)), len(ops), int(bool(gate_on)), 0,
                       float(contrast_thresh))
    for op in (ops + [("median", 0)] * CHAIN_MAX_OPS)[:CHAIN_MAX_OPS]:
        if op[0] == "clahe":
            _, space, tiles, clip = op
            blob += struct.pack("<iiiid", 0, 1 if str(space).upper() == "LAB" else 0, int(tiles), 0,
                                float(clip))
        elif op[0] == "median":
            blob += struct.pack("<iiiid", 1, 0, 0, int(op[1]), 0.0)
        elif op[0] == "dcp":
            _, patch, wq, tq, radius, eq = op
            blob += struct.pack("<iiiiii", 2, int(tq), int(radius), int(patch), int(wq), int(eq))
        elif op[0] == "streak":
            _, width, min_len, max_len, slant, thr = op
            blob += struct.pack("<iiiiii", 4, int(thr), int(min_len), int(width), int(max_len),
                                int(slant))
        else:
            raise ValueError(f"chain op {op[0]!r}: expected 'clahe', 'median', 'dcp' or 'streak'")
    assert len(blob) == CHAIN_DESC_BYTES
    return (ctypes.c_uint8 * CHAIN_DESC_BYTES).from_buffer_copy(blob)


def preprocess_chain_route(desc, H: int, W: int, geo=None) -> int:
    """Which route rv_preprocess_chain_u8 takes (ROUTE_*); a host query."""
    st = int(_lib.load().rv_preprocess_chain_route(
        desc, int(H), int(W), None if geo is None else _lib.int_array(geo)))
    if st < 0:
        _lib.check(st, "rv_preprocess_chain_route")
    return st


def preprocess_chain_ws_bytes(desc, B: int, H: int, W: int, pitch: Optional[int] = None) -> int:
    """Workspace bytes of rv_preprocess_chain_u8 (0 for a bad descriptor); a
    host query.  pitch: bytes per frame row (default 3 * W)."""
    return int(_lib.load().rv_preprocess_chain_ws_bytes(
        desc, int(B), int(H), int(W), 3 * int(W) if pitch is None else int(pitch)))


def desc_is_identity(desc) -> bool:
    """True for a disabled or empty chain: proc = raw for every frame."""
    enabled, n_ops = struct.unpack_from("<ii", bytes(desc), 0)
    return not enabled or n_ops == 0


def _desc_has_lab(desc) -> bool:
    b = bytes(desc)
    n = min(struct.unpack_from("<i", b, 4)[0], CHAIN_MAX_OPS)
    return any(struct.unpack_from("<ii", b, 24 + 24 * i) == (0, 1) for i in range(max(n, 0)))


def preprocess_chain(frames: torch.Tensor, desc, geo=None, out: Optional[torch.Tensor] = None,
                     lb_out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    """pipeline(raw) + LetterBox of any built-in chain (rv_preprocess_chain_u8):
    returns (proc, letterboxed proc), or (proc, None) when geo is None.
    Stream-ordered launches only: the low-contrast gate is evaluated on the
    device.  A disabled or empty chain called without `out` returns the
    input frames themselves as proc (no copy), as the pipeline does."""
    x, B, H, W, pitch = _frames(frames)
    if out is None and desc_is_identity(desc):
        if geo is None:
            return frames, None
        out, proc = None, frames
    else:
        out = proc = _like(x, out)
        if frames.dim() != 4:
            proc = out[0]
    if geo is None:
        if lb_out is not None:
            raise ValueError("lb_out needs the letterbox geometry (geo)")
    elif lb_out is None:
        lb_out = torch.empty((B, geo[0], geo[1], 3), dtype=torch.uint8, device=x.device)
    ws = _workspace(ws, preprocess_chain_ws_bytes(desc, B, H, W, pitch), x.device)
    if _desc_has_lab(desc):
        _lab_tables(x.device)
    call("rv_preprocess_chain_u8", ptr(x), ptr(out), B, H, W, pitch, desc, ptr(ws), ws.numel(),
         ptr(lb_out), None if geo is None else _lib.int_array(geo), stream_ptr())
    return proc, lb_out


def gray_span(frames: torch.Tensor) -> torch.Tensor:
    x, B, H, W, pitch = _frames(frames)
    ws = torch.empty(2 * B, dtype=torch.int32, device=x.device)
    span = torch.empty(B, dtype=torch.int32, device=x.device)
    call("rv_gray_span_u8", ptr(x), B, H, W, pitch, ptr(ws), ptr(span), stream_ptr())
    return span


def letterbox_geometry(H: int, W: int, imgsz: int = 640, stride: int = 32):
    geo = _lib.int_array([0] * 6)
    call("rv_letterbox_geometry", H, W, imgsz, stride, geo)
    return tuple(int(v) for v in geo)


def letterbox(frames: torch.Tensor, geo, out: Optional[torch.Tensor] = None):
    x, B, H, W, pitch = _frames(frames)
    oh, ow = geo[0], geo[1]
    if out is None:
        out = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=x.device)
    call("rv_letterbox_u8", ptr(x), ptr(out), B, H, W, pitch, _lib.int_array(geo), stream_ptr())
    return out

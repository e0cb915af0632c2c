"""The named inputs of the preprocess path tests (test_preprocess_cases_cpu.py,
test_preprocess_paths_gpu.py): every case is one call of one entry of
csrc/preprocess.hip on named frames, with the oracle's answer (oracle.cpu,
computed once per process and shared, read-only) and, from the host side
alone, the kernel path the call takes (path_of: the path predicates of
the library restated in Python, each citing the function it mirrors; the CPU
test holds them to the library's own host queries) and the regime the data
is in (clahe_stats, unclamped_crcb, unsaturated_bgr, split_share: numpy on
the oracle's planes).  test_preprocess_cases_cpu.py asserts paths and
regimes, so the GPU test cannot silently run another path than the one a
case is named for.

A frame is named by a spec tuple -- ("noise", seed), ("flat", v),
("flat_split", y, num, den), ("checker", a, b), ("checker3",),
("two_level", seed), ("lattice",), ("blocks",), ("road", seed),
("ramp_extremes", seed, where, lo, hi) -- and a case holds one spec per
batch element.  A layout is "contig" (a fresh (B, H, W, 3) tensor) or one of
"in_mis" / "out_mis" / "both_mis": input and output are views of
(B, H, W + PAD_COLS, 3) buffers, an aligned one starting at column 0 and a
misaligned one at column 1 (3 bytes past the allocation base)."""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

from conftest import road_frame
from oracle import cpu

PAD_COLS = 5
IN_FILL, OUT_FILL = 7, 9          # what the padding columns of the wide buffers hold
ROUTE_FUSED, ROUTE_FUSED_GATED, ROUTE_OPS = 0, 1, 2   # RV_CHAIN_ROUTE_* (include/rvhip.h)
ROUTES = {ROUTE_FUSED: "fused", ROUTE_FUSED_GATED: "fused_gated", ROUTE_OPS: "ops"}
KS = (3, 5, 7, 9)
CHECKERS = [(127, 128), (0, 255), (254, 255), (0, 1)]
# ("checker3",): per channel (a, b, phase) -- three different pairs, the green
# channel in the opposite phase: a channel mix-up in the byte permutes shows
CHECKER3 = [(127, 128, 0), (0, 255, 1), (254, 255, 0)]
MEDIAN_SHAPES = [(1, 1), (1, 7), (2, 3), (7, 1), (31, 127), (32, 128), (33, 129), (15, 127),
                 (16, 128), (17, 129), (70, 130)]
LAYOUTS = ("in_mis", "out_mis", "both_mis")
LB_IMGSZ = 64
# shape -> (eligible for the fused letterbox, its form)
LETTERBOX = {
    (64, 128): (True, "half-weight blend, 2:1"),
    (96, 192): (True, "copy form, 3:1"),
    (192, 384): (True, "blend across several blocks, 6:1"),
    (64, 64): (True, "identity"),
    (40, 64): (True, "scale 1, pad rows"),
    (20, 32): (False, "upscale"),
    (100, 160): (False, "taps straddle a block"),
}


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def lattice():
    """512 x 512: every colour of the 64^3 lattice with channel levels
    round(i 255 / 63) once, in a fixed random pixel order."""
    lv = np.rint(np.arange(64) * 255.0 / 63.0).astype(np.uint8)
    idx = np.random.default_rng(64).permutation(64 ** 3)
    return _ro(np.stack([lv[idx & 63], lv[(idx >> 6) & 63], lv[idx >> 12]], -1).reshape(512, 512, 3))


@functools.lru_cache(maxsize=None)
def blocks():
    """256 x 256: every colour of the 16^3 lattice (levels 17 i, the cube
    corners among them) as one 4 x 4 block, the blocks in a fixed random
    order.  A 3 x 3 window inside a block holds one colour, so a median behind
    the CLAHE cannot hide what the colour arithmetic did to it (on the
    lattice a wrong pixel stands alone among 8 others and is filtered out)."""
    idx = np.random.default_rng(16).permutation(16 ** 3).reshape(64, 64)
    col = np.stack([idx & 15, (idx >> 4) & 15, idx >> 8], -1) * 17
    return _ro(np.repeat(np.repeat(col, 4, 0), 4, 1))


def gray_of(img):
    """cv2 BGR2GRAY / the Y of BGR2YCrCb, 14-bit fixed point (common.h bgr_to_y)."""
    i = np.asarray(img).astype(np.int64)
    return (i[..., 0] * 1868 + i[..., 1] * 9617 + i[..., 2] * 4899 + 8192) >> 14


def extremes_at(where, H, W):
    """(position of the minimum, position of the maximum) of ramp_extremes."""
    return {"first_last": ((0, 0), (H - 1, W - 1)),
            "last_first": ((H - 1, W - 1), (0, 0)),
            "ragged_row": ((H // 2, W - 1), (H - 1, W - 1))}[where]


@functools.lru_cache(maxsize=None)
def make_frame(spec, H, W):
    kind = spec[0]
    if kind == "noise":
        f = np.random.default_rng(spec[1]).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "two_level":
        f = np.random.default_rng(spec[1]).integers(0, 2, (H, W, 3), dtype=np.uint8) * 255
    elif kind == "checker":
        par = (np.arange(H)[:, None] + np.arange(W)[None, :]) & 1
        f = np.repeat(np.where(par == 0, spec[1], spec[2])[..., None], 3, 2)
    elif kind == "checker3":
        par = (np.arange(H)[:, None] + np.arange(W)[None, :]) & 1
        f = np.stack([np.where((par + ph) & 1 == 0, a, b) for a, b, ph in CHECKER3], -1)
    elif kind == "flat":
        f = np.empty((H, W, 3), np.uint8)
        f[:] = spec[1]
    elif kind == "flat_split":   # gray y left of column W num / den, y + 1 from there on
        _, y, num, den = spec
        assert y % 2 == 0 and y < 255
        f = np.full((H, W, 3), y, np.uint8)
        f[:, W * num // den:] = y + 1
    elif kind == "lattice":      # the first H W pixels of the lattice (all of it at 512 x 512)
        f = lattice().reshape(-1, 3)[:H * W].reshape(H, W, 3)
    elif kind == "blocks":
        assert (H, W) == (256, 256)
        f = blocks()
    elif kind == "road":
        f = road_frame(H, W, seed=spec[1])
    elif kind == "ramp_extremes":
        _, seed, where, lo, hi = spec
        f = np.clip(road_frame(H, W, seed=seed), 4, 251)  # gray 4 .. 251 everywhere ...
        pmin, pmax = extremes_at(where, H, W)
        f[pmin], f[pmax] = lo, hi                            # ... but at the two planted pixels
    else:
        raise ValueError(spec)
    return _ro(f)


def frames_of(case):
    return np.stack([make_frame(s, case.H, case.W) for s in case.frame])


# ---------------------------------------------------------------------------
# the path predicates of csrc/{clahe,median,preprocess}.hip, restated
# ---------------------------------------------------------------------------
kBW, kBH, kLutWinMax = 128, 16, 48                 # median.hip: median_tile_kernel
kM3W, kM3H, kM3TW, kM3TH, kCellMax = 128, 32, 136, 34, 16   # median.hip: med3_kernel


class Geo(NamedTuple):
    tiles: int
    tw: int
    th: int
    clip_limit: int


def make_geo(H, W, tiles, clip=0.0):
    """clahe.h: make_geo."""
    if W % tiles == 0 and H % tiles == 0:
        tw, th = W // tiles, H // tiles
    else:
        tw, th = (W + tiles - W % tiles) // tiles, (H + tiles - H % tiles) // tiles
    lim = max(int(clip * (tw * th) / 256), 1) if clip > 0.0 else 0
    return Geo(tiles, tw, th, lim)


def clahe_packed_ok(g):
    """clahe.hip: clahe_packed_ok."""
    per_thread = 4 * (((g.tw // 4) * g.th + 255) // 256) + (g.tw * g.th + 255) // 256
    return 8 * per_thread <= 65535


def med3_cells(g):
    """median.hip: med3_cells."""
    ncx = min((kM3TW + g.tw - 1) // g.tw + 2, g.tiles + 1)
    ncy = min((kM3TH + g.th - 1) // g.th + 2, g.tiles + 1)
    return ncx * ncy


def med3_cells_fit(g):
    """median.hip: med3_cells_fit."""
    return med3_cells(g) <= kCellMax


def lut_window_fits(g, K):
    """median.hip: lut_window_fits."""
    R = K // 2
    cols = (kBW + 2 * R - 1) // g.tw + 3
    rows = (kBH + 2 * R - 1) // g.th + 3
    return min(cols, g.tiles) * min(rows, g.tiles) <= kLutWinMax


def clahe_median_fits(H, W, tiles, k):
    """median.hip: clahe_median_fuses (rv_clahe_median_fits)."""
    g = make_geo(H, W, tiles)
    return (k == 3 and med3_cells_fit(g)) or lut_window_fits(g, k)


def lut_loader(H, W, g, pitch, base):
    """clahe.hip: clahe_lut_body, the LUT loader's `inside` and `vec`, over the
    whole grid: 'vec' when every tile loads dwords, 'mixed' when only the
    tiles inside the frame do, else 'scalar'.  (A frame's base is in + b H
    pitch and a tile's x0 = tx tw: both keep the alignment when pitch % 4 ==
    0 and tw % 4 == 0.)"""
    if g.tw % 4 or pitch % 4 or base % 4:
        return "scalar"
    inside = sum(1 for ty in range(g.tiles) for tx in range(g.tiles)
                 if (tx + 1) * g.tw <= W and (ty + 1) * g.th <= H)
    return "vec" if inside == g.tiles ** 2 else ("mixed" if inside else "scalar")


def dword_io(pitch, *bases):
    """median.hip: launch_med3_as (in and out); preprocess.hip: launch_gray_span (in)."""
    return "vec" if pitch % 4 == 0 and all(b % 4 == 0 for b in bases) else "scalar"


def _f32(v):
    return np.asarray(v, np.float32)


def lb_taps(n_dst, scale, n, vertical):
    """lbgeo.h: lb_tap_x / lb_tap_y for every destination index:
    (s0, s1) after the zero-weight redirection, and w1."""
    d = np.arange(n_dst, dtype=np.float64)
    f = _f32((d + 0.5) * scale - 0.5)
    s = np.floor(f).astype(np.int64)
    f = _f32(f - _f32(s))
    if not vertical:
        f = np.where(s < 0, _f32(0), f)
        s = np.maximum(s, 0)
    w0 = np.clip(np.rint(_f32(_f32(_f32(1) - f) * _f32(2048))), -32768, 32767).astype(np.int64)
    w1 = np.clip(np.rint(_f32(f * _f32(2048))), -32768, 32767).astype(np.int64)
    s0, s1 = np.clip(s, 0, n - 1), np.clip(s + 1, 0, n - 1)
    if not vertical:
        edge = s >= n - 1
        s0, s1 = np.where(edge, n - 1, s0), np.where(edge, n - 1, s1)
        w0, w1 = np.where(edge, 2048, w0), np.where(edge, 0, w1)
    s1 = np.where(w1 == 0, s0, s1)
    s0 = np.where(w0 == 0, s1, s0)
    return s0, s1, w1


def lbgeo_ok(geo):
    """lbgeo.h: lbgeo_from's consistency test."""
    oh, ow, nh, nw, top, left = geo
    return nh > 0 and nw > 0 and top >= 0 and left >= 0 and top + nh <= oh and left + nw <= ow


def med3_lb_fits(geo, H, W):
    """median.hip: med3_lb_fits."""
    _, _, nh, nw, _, _ = geo
    if nw > W or nh > H:
        return False
    x0, x1, _ = lb_taps(nw, 1.0 / (nw / W), W, False)
    y0, y1, _ = lb_taps(nh, 1.0 / (nh / H), H, True)
    return bool((x0 // kM3W == x1 // kM3W).all() and (y0 // kM3H == y1 // kM3H).all())


def lb_is_copy(geo, H, W):
    """median.hip: lb_is_copy."""
    _, _, nh, nw, _, _ = geo
    return bool((lb_taps(nw, 1.0 / (nw / W), W, False)[2] == 0).all() and
                (lb_taps(nh, 1.0 / (nh / H), H, True)[2] == 0).all())


def letterbox_fits(H, W, tiles, k, geo):
    """preprocess.hip: rv_clahe_median_letterbox_fits."""
    return k == 3 and lbgeo_ok(geo) and med3_cells_fit(make_geo(H, W, tiles)) and \
        med3_lb_fits(geo, H, W)


def chain_passes(ops, H, W):
    """preprocess.hip: make_plan, the passes: ('clahe', space, tiles,
    clip), ('median', k) or ('clahe_median', tiles, clip, k)."""
    out, i = [], 0
    while i < len(ops):
        o = ops[i]
        if o[0] == "clahe" and o[1] == "YCrCb" and i + 1 < len(ops) and ops[i + 1][0] == "median" \
                and clahe_median_fits(H, W, o[2], ops[i + 1][1]):
            out.append(("clahe_median", o[2], o[3], ops[i + 1][1]))
            i += 2
        else:
            out.append(o)
            i += 1
    return out


def chain_route(ops, enabled, gate, H, W, geo=None):
    """preprocess.hip: make_plan, the route."""
    if not enabled or not ops:
        return ROUTE_OPS
    p = chain_passes(ops, H, W)
    if len(p) == 1 and p[0][0] == "clahe_median" and p[0][3] == 3 and \
            med3_cells_fit(make_geo(H, W, p[0][1])) and (geo is None or med3_lb_fits(geo, H, W)):
        return ROUTE_FUSED_GATED if gate else ROUTE_FUSED
    return ROUTE_OPS


class Path(NamedTuple):
    hist: Optional[str]      # packed16 | packed_wide | u32
    loader: Optional[str]    # vec | mixed | scalar (the LUT kernel's histogram loads)
    applier: Optional[str]   # apply | med3 | tile<K>
    io: Optional[str]        # vec | scalar: dword loads / stores of med3 and gray span
    route: Optional[str]     # fused | fused_gated | ops (chains only)


def path_of(entry, H, W, tiles=0, k=0, pitch=None, base_offset=0, gate=False, geo=None):
    """What runs for one call.  entry: clahe_ycrcb, clahe_lab, median,
    clahe_median, clahe_median_letterbox, gray_span, or chain (the chain
    [CLAHE(YCrCb, tiles), median k]).  base_offset: bytes past 4-byte
    alignment of the input, or (input, output).  A clahe_median call the
    library refuses (rv_clahe_median_fits) has no applier."""
    pitch = 3 * W if pitch is None else pitch
    bi, bo = base_offset if isinstance(base_offset, tuple) else (base_offset, base_offset)
    if entry == "gray_span":
        return Path(None, None, None, dword_io(pitch, bi), None)
    if entry == "median":
        return Path(None, None, "med3" if k == 3 else f"tile<{k}>",
                    dword_io(pitch, bi, bo) if k == 3 else None, None)
    g = make_geo(H, W, tiles)
    hist = "u32" if not clahe_packed_ok(g) else ("packed16" if g.tw * g.th <= 65535 else "packed_wide")
    loader = lut_loader(H, W, g, pitch, bi)
    if entry in ("clahe_ycrcb", "clahe_lab"):
        return Path(hist, loader, "apply", None, None)
    if k == 3 and med3_cells_fit(g):
        applier = "med3"
    else:
        applier = f"tile<{k}>" if lut_window_fits(g, k) else None
    io = dword_io(pitch, bi, bo) if applier == "med3" else None
    if entry in ("clahe_median", "clahe_median_letterbox"):
        return Path(hist, loader, applier, io, None)
    assert entry == "chain", entry
    ops = [("clahe", "YCrCb", tiles, 2.0), ("median", k)]
    return Path(hist, loader, applier, io, ROUTES[chain_route(ops, True, gate, H, W, geo)])


# ---------------------------------------------------------------------------
# regimes, from the oracle's planes alone
# ---------------------------------------------------------------------------
def luma_plane(img, space="YCrCb"):
    return np.ascontiguousarray((cpu.bgr2lab(img) if space == "LAB" else cpu.bgr2ycrcb(img))[..., 0])


def clahe_stats(plane, tiles, clip):
    """cv::CLAHE (8UC1) restated in numpy after
    test_oracle_preprocess._clahe_numpy, with what the redistribution did:
    {clip_limit, batch, residual, max_bin (tiles, tiles), bins (the number of
    nonempty bins), out}.  `out` must equal cpu.clahe_u8c1."""
    H, W = plane.shape
    g = make_geo(H, W, tiles, clip)
    ext = plane
    if g.tw * tiles != W or g.th * tiles != H:
        ext = np.pad(plane, ((0, g.th * tiles - H), (0, g.tw * tiles - W)), mode="reflect")
    area = g.tw * g.th
    scale = np.float32(255) / np.float32(area)
    lut = np.zeros((tiles, tiles, 256), np.uint8)
    batch, residual, max_bin, bins = (np.zeros((tiles, tiles), np.int64) for _ in range(4))
    for ty in range(tiles):
        for tx in range(tiles):
            t = ext[ty * g.th:(ty + 1) * g.th, tx * g.tw:(tx + 1) * g.tw]
            h = np.bincount(t.ravel(), minlength=256).astype(np.int64)
            max_bin[ty, tx], bins[ty, tx] = h.max(), (h > 0).sum()
            if g.clip_limit > 0:
                clipped = int(np.maximum(h - g.clip_limit, 0).sum())
                h = np.minimum(h, g.clip_limit)
                batch[ty, tx], residual[ty, tx] = clipped // 256, clipped % 256
                h += clipped // 256
                if clipped % 256:
                    step = max(256 // (clipped % 256), 1)
                    h[np.arange(0, 256, step)[:clipped % 256]] += 1
            lut[ty, tx] = np.clip(np.rint(np.cumsum(h).astype(np.float32) * scale), 0, 255)
    one, half = np.float32(1), np.float32(0.5)
    xs = np.arange(W, dtype=np.float32) * (one / np.float32(g.tw)) - half
    ys = np.arange(H, dtype=np.float32) * (one / np.float32(g.th)) - half
    tx1, ty1 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    xa, ya = xs - tx1.astype(np.float32), ys - ty1.astype(np.float32)
    xa1, ya1 = one - xa, one - ya
    tx2, ty2 = np.minimum(tx1 + 1, tiles - 1), np.minimum(ty1 + 1, tiles - 1)
    tx1, ty1 = np.maximum(tx1, 0), np.maximum(ty1, 0)
    out = np.empty_like(plane)
    for y in range(H):
        v = plane[y].astype(int)
        top = lut[ty1[y], tx1, v].astype(np.float32) * xa1 + lut[ty1[y], tx2, v].astype(np.float32) * xa
        bot = lut[ty2[y], tx1, v].astype(np.float32) * xa1 + lut[ty2[y], tx2, v].astype(np.float32) * xa
        res = top * ya1[y] + bot * ya[y]
        assert res.dtype == np.float32
        out[y] = np.clip(np.rint(res), 0, 255)
    return {"clip_limit": g.clip_limit, "batch": batch, "residual": residual, "max_bin": max_bin,
            "bins": bins, "out": out}


@functools.lru_cache(maxsize=None)
def stats_of(spec, H, W, space, tiles, clip):
    return clahe_stats(luma_plane(make_frame(spec, H, W), space), tiles, clip)


def unclamped_crcb(img):
    """Cr and Cb of BGR2YCrCb before saturate_cast (common.h bgr_to_ycrcb)."""
    i = np.asarray(img).astype(np.int64)
    Y = gray_of(img)
    return ((i[..., 2] - Y) * 11682 + (128 << 14) + 8192) >> 14, \
        ((i[..., 0] - Y) * 9241 + (128 << 14) + 8192) >> 14


def unsaturated_bgr(img, tiles, clip):
    """YCrCb2BGR of the oracle's CLAHE'd luma before saturate_cast (H, W, 3)."""
    ycc = cpu.bgr2ycrcb(img).astype(np.int64)
    y2 = cpu.clahe_u8c1(np.ascontiguousarray(ycc[..., 0].astype(np.uint8)), tiles, clip).astype(np.int64)
    dcr, dcb = ycc[..., 1] - 128, ycc[..., 2] - 128
    return np.stack([y2 + ((dcb * 29049 + 8192) >> 14),
                     y2 + ((dcb * -5636 + dcr * -11698 + 8192) >> 14),
                     y2 + ((dcr * 22987 + 8192) >> 14)], -1)


def interior_windows(img, k):
    """(H - k + 1, W - k + 1, 3, k k): the windows that touch no border."""
    w = np.lib.stride_tricks.sliding_window_view(img, (k, k), axis=(0, 1))
    return w.reshape(w.shape[:3] + (k * k,))


def split_share(img, k):
    """Share of interior windows (per channel) whose two most frequent values
    split k k into (k k + 1) / 2 and (k k - 1) / 2."""
    w = np.sort(interior_windows(img, k), -1)
    n = k * k
    if w.size == 0:
        return 0.0
    two = (np.diff(w, axis=-1) != 0).sum(-1) == 1
    lo = (w == w[..., :1]).sum(-1)
    return float((two & ((lo == n // 2) | (lo == n // 2 + 1))).mean())


# ---------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    group: str               # clahe | colour | median | layout | span | chain | letterbox
    frame: Tuple[tuple, ...]  # one frame spec per batch element
    H: int
    W: int
    entry: str
    tiles: int
    clip: float
    k: int
    layout: str
    expect_path: Path
    gate: bool = False
    imgsz: int = 0            # letterbox geometry (0: none)
    tag: str = ""             # which regime the CPU test holds the case to

    @property
    def B(self):
        return len(self.frame)


def spec_name(s):
    return "_".join(str(v) for v in s)


def pitch_base(layout, W):
    """(pitch, (input base, output base)) of a layout."""
    if layout == "contig":
        return 3 * W, (0, 0)
    return 3 * (W + PAD_COLS), {"in_mis": (3, 0), "out_mis": (0, 3), "both_mis": (3, 3)}[layout]


def case_geo(case):
    return cpu.letterbox_geometry(case.H, case.W, case.imgsz, 32) if case.imgsz else None


def P(hist=None, loader=None, applier=None, io=None, route=None):
    return Path(hist, loader, applier, io, route)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case.  expect_path is written by hand from the geometry; the
    CPU test compares it with path_of."""
    out = []

    def add(group, frame, H, W, entry, tiles, clip, k, path, layout="contig", tag="", **kw):
        frame = tuple(frame) if isinstance(frame[0], tuple) else (frame,)
        name = f"{group}/{entry}/{'+'.join(spec_name(s) for s in frame)}/{H}x{W}/t{tiles}c{clip:g}k{k}"
        name += ("/" + layout if layout != "contig" else "") + ("/gate" if kw.get("gate") else "")
        name += f"/lb{kw['imgsz']}" if kw.get("imgsz") else ""
        out.append(Case(name, group, frame, H, W, entry, tiles, float(clip), k, layout, path,
                        tag=tag, **kw))

    def clahe3(group, frame, H, W, tiles, clip, hist, loader, applier="med3", tag=""):
        """clahe_ycrcb, clahe_lab and (where the library takes it) clahe_median k = 3."""
        add(group, frame, H, W, "clahe_ycrcb", tiles, clip, 0, P(hist, loader, "apply"), tag=tag)
        add(group, frame, H, W, "clahe_lab", tiles, clip, 0, P(hist, loader, "apply"), tag=tag)
        if applier:
            add(group, frame, H, W, "clahe_median", tiles, clip, 3,
                P(hist, loader, applier, ("vec" if W % 4 == 0 else "scalar") if applier == "med3" else None),
                tag=tag)

    noise, road = ("noise", 11), ("road", 12)
    split, split_q = ("flat_split", 100, 1, 2), ("flat_split", 100, 1, 4)
    flat = ("flat", 77)

    # --- CLAHE histogram and LUT
    # u32: 1024 x 1024 at tiles = 1 is one tile of 1 048 576 pixels
    for fr in (noise, split, road, (("noise", 13), split)):
        clahe3("clahe", fr, 1024, 1024, 1, 2.0, "u32", "vec", tag="flat" if fr == split else "")
    # packed_wide, the largest packed tile: 1023 x 1024 at tiles = 1
    for fr in (split, noise):
        clahe3("clahe", fr, 1023, 1024, 1, 2.0, "packed_wide", "vec", tag="flat" if fr == split else "")
    # packed_wide, the smallest: 512 x 514 at tiles = 2, tiles of 257 x 256 = 65 792
    # (split after column 256 / after column 1: the left tiles hold both bins of
    # the pair, 65 536 pixels in the even / in the odd one)
    for fr in (flat, split, ("flat_split", 100, 256, 514), ("flat_split", 100, 1, 514)):
        for clip in (2.0, 0.0):
            clahe3("clahe", fr, 512, 514, 2, clip, "packed_wide", "scalar",
                   tag="flat_redistribute" if clip else "flat_clip0")
    # packed16 at its carry-free bound: 510 x 512 at tiles = 2, tiles of 256 x 255 = 65 280
    for fr in (split, split_q):
        clahe3("clahe", fr, 510, 512, 2, 2.0, "packed16", "vec", tag="flat16")
    # loader steps: groups = 1; groups = 257 (dr = 0); groups = 129
    clahe3("clahe", noise, 32, 32, 8, 2.0, "packed16", "vec", applier=None)
    clahe3("clahe", noise, 16, 2056, 2, 2.0, "packed16", "vec")
    clahe3("clahe", noise, 260, 516, 2, 2.0, "packed16", "scalar")
    clahe3("clahe", noise, 260, 1032, 2, 2.0, "packed_wide", "vec")
    # grid extremes
    clahe3("clahe", noise, 64, 128, 1, 2.0, "packed16", "vec")
    clahe3("clahe", noise, 64, 128, 2, 2.0, "packed16", "vec")
    clahe3("clahe", noise, 64, 128, 64, 2.0, "packed16", "scalar", applier=None)
    clahe3("clahe", noise, 3, 5, 8, 2.0, "packed16", "scalar", applier=None)
    clahe3("clahe", noise, 1, 1, 8, 2.0, "packed16", "scalar", applier=None)
    clahe3("clahe", noise, 1, 7, 3, 40.0, "packed16", "scalar", applier="med3")
    # redistribution
    clahe3("clahe", road, 128, 256, 8, 2.0, "packed16", "vec", applier="tile<3>", tag="road_clip2")
    clahe3("clahe", road, 128, 256, 8, 40.0, "packed16", "vec", applier="tile<3>", tag="road_clip40")
    clahe3("clahe", noise, 128, 256, 8, 2.0, "packed16", "vec", applier="tile<3>", tag="noise_clip2")

    # --- colour: the lattice through every applier
    lat = ("lattice",)
    add("colour", lat, 512, 512, "clahe_ycrcb", 8, 2.0, 0, P("packed16", "vec", "apply"))
    add("colour", lat, 512, 512, "clahe_ycrcb", 8, 0.0, 0, P("packed16", "vec", "apply"))
    add("colour", lat, 512, 512, "clahe_lab", 8, 2.0, 0, P("packed16", "vec", "apply"))
    add("colour", lat, 512, 512, "clahe_median", 2, 2.0, 3, P("packed_wide", "vec", "med3", "vec"))
    add("colour", lat, 512, 512, "clahe_median", 8, 2.0, 3, P("packed16", "vec", "med3", "vec"))
    add("colour", lat, 512, 512, "clahe_median", 16, 2.0, 3, P("packed16", "vec", "tile<3>"))
    add("colour", lat, 512, 512, "clahe_median", 8, 2.0, 5, P("packed16", "vec", "tile<5>"))
    # ... and every saturated colour in 4 x 4 blocks, which a median lets through
    blk = ("blocks",)
    add("colour", blk, 256, 256, "clahe_ycrcb", 4, 2.0, 0, P("packed16", "vec", "apply"))
    add("colour", blk, 256, 256, "clahe_lab", 4, 2.0, 0, P("packed16", "vec", "apply"))
    add("colour", blk, 256, 256, "clahe_median", 2, 2.0, 3, P("packed16", "vec", "med3", "vec"))
    add("colour", blk, 256, 256, "clahe_median", 4, 2.0, 3, P("packed16", "vec", "med3", "vec"))
    add("colour", blk, 256, 256, "clahe_median", 8, 2.0, 3, P("packed16", "vec", "tile<3>"))
    add("colour", blk, 256, 256, "clahe_median", 8, 2.0, 5, P("packed16", "vec", "tile<5>"))
    add("colour", blk, 256, 256, "clahe_median", 4, 0.0, 3, P("packed16", "vec", "med3", "vec"))

    # --- median: rank boundaries on every kernel, with and without CLAHE in front
    med_frames = [("checker", a, b) for a, b in CHECKERS] + [("checker3",), ("two_level", 21),
                                                             ("noise", 22)]
    for fr in med_frames:
        for H, W in MEDIAN_SHAPES:
            for k in KS:
                io = ("vec" if W % 4 == 0 else "scalar") if k == 3 else None
                ap = "med3" if k == 3 else f"tile<{k}>"
                add("median", fr, H, W, "median", 0, 0.0, k, P(None, None, ap, io))
                # tiles = 2: a tile is at most 65 x 35, the LUT window is the whole grid
                add("median", fr, H, W, "clahe_median", 2, 2.0, k,
                    P("packed16", "vec" if W % 8 == 0 and H % 2 == 0 else "scalar", ap, io))
    # batches of different frames through the XCD tile remap of med3_kernel:
    # 3 blocks (fewer than 8) and 2 x 3 x 3 = 18 blocks (no multiple of 8)
    mix = (("noise", 23), ("two_level", 24), ("checker3",))
    for H, W, io, ld in [(32, 128, "vec", "vec"), (70, 130, "scalar", "scalar")]:
        add("median", mix, H, W, "median", 0, 0.0, 3, P(None, None, "med3", io))
        add("median", mix, H, W, "clahe_median", 2, 2.0, 3, P("packed16", ld, "med3", io))
        add("median", mix, H, W, "median", 0, 0.0, 5, P(None, None, "tile<5>"))

    # --- layouts: every entry on views that start one pixel into a wider buffer
    # (70 x 131 at tiles = 3: tiles of 44 x 24, so the aligned loader is vector
    # on the four tiles inside the frame)
    for lay in LAYOUTS:
        ld = "mixed" if lay == "out_mis" else "scalar"
        add("layout", noise, 70, 131, "clahe_ycrcb", 3, 2.0, 0, P("packed16", ld, "apply"), lay)
        add("layout", noise, 70, 131, "clahe_lab", 3, 2.0, 0, P("packed16", ld, "apply"), lay)
        add("layout", noise, 70, 131, "median", 0, 0.0, 3, P(None, None, "med3", "scalar"), lay)
        add("layout", noise, 70, 131, "median", 0, 0.0, 5, P(None, None, "tile<5>"), lay)
        add("layout", noise, 70, 131, "clahe_median", 3, 2.0, 3,
            P("packed16", ld, "med3", "scalar"), lay)
        add("layout", noise, 70, 131, "clahe_median", 3, 2.0, 5, P("packed16", ld, "tile<5>"), lay)
        # imgsz 131: scale 1 with pad rows, the one letterbox a 131-wide frame's taps fit
        add("layout", noise, 70, 131, "clahe_median_letterbox", 3, 2.0, 3,
            P("packed16", ld, "med3", "scalar"), lay, imgsz=131)
        add("layout", (noise, ("noise", 14)), 70, 131, "chain", 3, 2.0, 3,
            P("packed16", ld, "med3", "scalar", "fused"), lay, imgsz=131)
        add("layout", (flat, noise), 70, 131, "chain", 3, 2.0, 5,
            P("packed16", ld, "tile<5>", None, "ops"), lay, gate=True, imgsz=131)
    # gray span reads only: "out_mis" is the aligned view of the wide buffer
    add("layout", noise, 70, 131, "gray_span", 0, 0.0, 0, P(io="scalar"), "in_mis")
    add("layout", noise, 70, 131, "gray_span", 0, 0.0, 0, P(io="vec"), "out_mis")

    # --- gray span
    ext = tuple(("ramp_extremes", 30 + b, w, b, 255 - b)
                for b, w in enumerate(("first_last", "last_first", "ragged_row")))
    for H, W in [(64, 96), (37, 91), (300, 2000)]:
        add("span", ext, H, W, "gray_span", 0, 0.0, 0, P(io="vec" if W % 4 == 0 else "scalar"),
            tag="extremes")
    add("span", ext, 37, 91, "gray_span", 0, 0.0, 0, P(io="scalar"), "in_mis", tag="extremes")
    add("span", (flat, ("flat", (3, 200, 90))), 64, 96, "gray_span", 0, 0.0, 0, P(io="vec"),
        tag="span0")
    add("span", ("checker", 0, 255), 37, 91, "gray_span", 0, 0.0, 0, P(io="scalar"), tag="span255")

    # --- chain and gate: a flat frame (span 0: processed), noise and colour (both pass)
    gated = (flat, ("noise", 15), lat)
    add("chain", gated, 64, 256, "chain", 8, 2.0, 5, P("packed16", "vec", "tile<5>", None, "ops"),
        gate=True, imgsz=640)
    add("chain", gated, 64, 128, "chain", 2, 2.0, 3,
        P("packed16", "vec", "med3", "vec", "fused_gated"), gate=True, imgsz=LB_IMGSZ)
    add("chain", gated, 64, 128, "chain", 2, 2.0, 3,
        P("packed16", "vec", "med3", "vec", "fused_gated"), gate=True)

    # --- fused letterbox on crafted content
    for (H, W), (ok, _) in LETTERBOX.items():
        for fr in (("noise", 16), ("two_level", 17)):
            path = P("packed16", "vec", "med3", "vec")
            if ok:
                add("letterbox", (fr, flat), H, W, "clahe_median_letterbox", 2, 2.0, 3, path,
                    imgsz=LB_IMGSZ)
            add("letterbox", (fr, flat), H, W, "chain", 2, 2.0, 3,
                path._replace(route="fused" if ok else "ops"), imgsz=LB_IMGSZ)
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


def group(*names):
    return [n for n, c in cases().items() if c.group in names]


# ---------------------------------------------------------------------------
# the oracle's answers (computed once per process, shared, read-only)
# ---------------------------------------------------------------------------
def chain_ops(case):
    return (("clahe", "YCrCb", case.tiles, case.clip), ("median", case.k))


def case_ops(case):
    return {"clahe_ycrcb": (("clahe", "YCrCb", case.tiles, case.clip),),
            "clahe_lab": (("clahe", "LAB", case.tiles, case.clip),),
            "median": (("median", case.k),)}.get(case.entry, chain_ops(case))


@functools.lru_cache(maxsize=None)
def ref(spec, H, W, ops):
    """The oracle's chain `ops` on one frame; prefixes are shared."""
    if not ops:
        return make_frame(spec, H, W)
    src, op = ref(spec, H, W, ops[:-1]), ops[-1]
    if op[0] == "median":
        return _ro(cpu.median(src, op[1]))
    return _ro((cpu.clahe_lab if op[1] == "LAB" else cpu.clahe_ycrcb)(src, op[2], op[3]))


def span_of(img):
    g = gray_of(img)
    return int(g.max() - g.min())


GATE_THRESH = 20.0


class Answer(NamedTuple):
    proc: Optional[np.ndarray]   # (B, H, W, 3)
    lb: Optional[np.ndarray]     # (B, out_h, out_w, 3)
    span: Optional[np.ndarray]   # (B,)


@functools.lru_cache(maxsize=None)
def oracle(name):
    case = cases()[name]
    if case.entry == "gray_span":
        return Answer(None, None, np.array([span_of(make_frame(s, case.H, case.W)) for s in case.frame]))
    proc = []
    for s in case.frame:
        raw = make_frame(s, case.H, case.W)
        passes = case.gate and not float(span_of(raw)) < GATE_THRESH
        proc.append(raw if passes else ref(s, case.H, case.W, case_ops(case)))
    geo = case_geo(case)
    lb = None if geo is None else _ro(np.stack([cpu.letterbox(p, geo) for p in proc]))
    return Answer(_ro(np.stack(proc)), lb, None)


# ---------------------------------------------------------------------------
# the device's side (used by the GPU tests only)
# ---------------------------------------------------------------------------
class Device(NamedTuple):
    proc: Optional[np.ndarray]
    lb: Optional[np.ndarray]
    span: Optional[np.ndarray]
    x: object                # the input frames on the device, as handed to the entry
    out: object              # the output view (None: the entry allocated it)


def device_frames(case, cuda):
    """(input, out or None, check): the tensors of the case's layout; check()
    asserts the input came back unchanged and no padding column was written."""
    import torch
    host = frames_of(case)
    B, H, W = host.shape[:3]
    if case.layout == "contig":
        x = torch.from_numpy(host).to(cuda)
        return x, None, lambda: np.testing.assert_array_equal(x.cpu().numpy(), host)
    _, (bi, bo) = pitch_base(case.layout, W)
    wide = torch.full((B, H, W + PAD_COLS, 3), IN_FILL, dtype=torch.uint8, device=cuda)
    owide = torch.full((B, H, W + PAD_COLS, 3), OUT_FILL, dtype=torch.uint8, device=cuda)
    ci, co = bi // 3, bo // 3
    x, out = wide[:, :, ci:ci + W], owide[:, :, co:co + W]
    x.copy_(torch.from_numpy(host).to(cuda))
    assert x.data_ptr() % 4 == bi % 4 and out.data_ptr() % 4 == bo % 4 and x.stride(1) % 4 == 0

    def check():
        np.testing.assert_array_equal(x.cpu().numpy(), host)
        w, o = wide.cpu().numpy(), owide.cpu().numpy()
        assert (w[:, :, :ci] == IN_FILL).all() and (w[:, :, ci + W:] == IN_FILL).all()
        assert (o[:, :, :co] == OUT_FILL).all() and (o[:, :, co + W:] == OUT_FILL).all()
    return x, out, check


def chain_desc(case):
    from rvs_amd import kernels
    return kernels.chain_desc(chain_ops(case), gate_on=case.gate, contrast_thresh=GATE_THRESH)


def device_run(case, cuda):
    """One call of the case's entry."""
    from rvs_amd import kernels
    x, out, check = device_frames(case, cuda)
    geo = case_geo(case)
    proc = lb = span = None
    e = case.entry
    if e == "gray_span":
        span = kernels.gray_span(x)
    elif e == "clahe_ycrcb":
        proc = kernels.clahe_ycrcb(x, case.tiles, case.clip, out=out)
    elif e == "clahe_lab":
        proc = kernels.clahe_lab(x, case.tiles, case.clip, out=out)
    elif e == "median":
        proc = kernels.median(x, case.k, out=out)
    elif e == "clahe_median":
        proc = kernels.clahe_median(x, case.tiles, case.clip, case.k, out=out)
    elif e == "clahe_median_letterbox":
        proc, lb = kernels.clahe_median_letterbox(x, case.tiles, case.clip, case.k, geo, out=out)
    else:
        proc, lb = kernels.preprocess_chain(x, chain_desc(case), geo, out=out)
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    dv = Device(host(proc), host(lb), host(span), x, out)
    check()
    return dv


def compare(case, dv):
    """The device's bytes against the oracle's."""
    ans = oracle(case.name)
    for got, want, what in [(dv.proc, ans.proc, "proc"), (dv.lb, ans.lb, "letterbox"),
                            (dv.span, ans.span, "span")]:
        assert (got is None) == (want is None), (case.name, what)
        if want is not None:
            assert got.shape == want.shape, (case.name, what, got.shape, want.shape)
            np.testing.assert_array_equal(got, want, err_msg=f"{case.name} {what}")

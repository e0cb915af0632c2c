"""Named cases of the fog generator (csrc/augment.hip), shared by
tests/test_fog_cases_cpu.py (no GPU: proves on the oracle that every case
takes the path and meets the regime it is named for) and
tests/test_fog_paths_gpu.py (holds rv_fog_full_u8 / rv_fog_rain_u8 to the
oracle on every case, bytes and stages).

What is restated here, as plain functions, from augment.hip:
  * the path predicates (vector / scalar apply, rblocks and nblk with their
    caps, grid_lds, the row-pass segment count, fog_lum's block count, the
    per-band early return, the airlight regime);
  * the full chain's workspace layout, so a test can read the per-frame
    scalars and planes a call leaves behind with no new entry point;
  * the regions of a frame a confined fault would sit in (the last row-pass
    segment, the 256-column seams, tile edges, the border ring, the rows of
    an active depth band).

No case exceeds 260 x 520.  The 4096-block cap of the core's apply kernel
needs more than 4096 * 256 pixel groups (over a million), which no test of
a few seconds on the oracle can afford; it stays unpinned ("Fog
generator").
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from conftest import road_frame
from oracle import fog_ref

F = np.float32

# --- geometries and the paths each is named for -----------------------------
GEOMS = {
    # the API minimum: fog_lum one block; every 64 x 16 tile of fog_tbil /
    # fog_fade meets a border; fog_sep_v 2 x 2 blocks; the middle depth band
    # has 64 pixels (< 100) and is skipped
    "min": (64, 64),
    # a second sep_h segment 44 pixels wide, W % 4 == 0
    "seg": (72, 300),
    # odd W: the tbil pair tail, a second sep_h segment 3 pixels wide, the
    # scalar apply of the core
    "odd": (67, 259),
    # 135 200 pixels: nblk capped at 512 (17 blocks make a second trip),
    # rblocks capped at 256, three sep_h segments (the last 8 wide), fog_lum
    # 8 blocks
    "big": (260, 520),
}

# constants of augment.hip
K_GRID_LDS, K_RANGE_BLOCKS, K_FULL_NBLK, K_AIR_PER_BLOCK = 2048, 256, 512, 2048
K_TAB = dict(glow_a=0, glow_b=32, band=64, cw=160, sw=416, tbil=480, stride=576)
K_SEP_RMAX = 31


def ceil_div(a, b):
    return -(-a // b)


def band_rows(h):
    return max(10, int(0.12 * h))


def quantile_rank(n, q=0.9):
    """np.quantile's 'linear' virtual index for an f32 array: (k, t)."""
    vi = F(n - 1) * F(q)
    k = int(np.floor(vi))
    return k, F(vi - F(k))


# --- path predicates ---------------------------------------------------------
def core_vector(w, pitch):
    """rv_fog_rain_u8 runs fog_apply_kernel<4> (three dword loads per thread)."""
    return w % 4 == 0 and pitch % 4 == 0


def rblocks(h, w):
    return min(K_RANGE_BLOCKS, ceil_div(h * w, 256))


def nblk(h, w):
    return min(K_FULL_NBLK, ceil_div(h * w, 256))


def second_trip_blocks(h, w):
    """Blocks of fog_t / fog_scatter whose grid-stride loop runs a second
    time."""
    n = nblk(h, w)
    return max(0, min(n, ceil_div(h * w - n * 256, 256)))


def grid_stride(h, w, scale_ratio=0.18, n_oct=2):
    octs, _ = fog_ref.octaves(h, w, scale_ratio, n_oct)
    return sum((gh + 1) * (gw + 1) for gh, gw, _ in octs)


def grid_lds(h, w, scale_ratio=0.18, n_oct=2):
    return grid_stride(h, w, scale_ratio, n_oct) <= K_GRID_LDS


def sep_h_segments(w):
    """(segments of the row pass, width of the last)."""
    n = ceil_div(w, 256)
    return n, w - 256 * (n - 1)


def lum_blocks(h, w):
    return ceil_div(band_rows(h) * w, K_AIR_PER_BLOCK)


def bands_returning_early(params):
    """Per depth band: fog_sep_h / fog_sep_v<BAND> return at once for this
    frame (its drawn kernel size fp[13 + band] is <= 1)."""
    return [int(params[13 + i]) <= 1 for i in range(3)]


def airlight_regime(lum):
    """(same, with_eq, all) of fog_airfin for a band's f32 luminance: the two
    order statistics around the rank are one key; the keys equal to the
    selected one are in the mask; the mask holds under 100 pixels so the
    whole band is averaged."""
    s = np.sort(lum.ravel())
    n = s.size
    k, _ = quantile_rank(n)
    same = bool(s[k] == s[min(k + 1, n - 1)])
    thr = np.quantile(lum, 0.9)
    with_eq = bool(thr <= s[k])
    return same, with_eq, bool((lum >= thr).sum() < 100)


def select_state(lum):
    """(selected key, eq, residual rank) the radix select must end with."""
    keys = np.sort(lum.ravel().astype(F).view(np.uint32))
    k, _ = quantile_rank(keys.size)
    key = keys[k]
    return int(key), int((keys == key).sum()), int(k - (keys < key).sum())


# --- workspace layout of rv_fog_full_u8 ---------------------------------------
WS_ORDER = ("range", "part", "air", "ascale", "gthr", "tab", "hist", "st", "keys", "apart",
            "gpart", "t0", "tf", "h1", "tmp", "h2")
ST_BYTES = 128  # AirState: five u32, three pad, twelve f64


def ws_layout(b, h, w):
    """{name: (byte offset, byte size)} and the total, each start rounded up
    to 256 bytes, in augment.hip's order."""
    px = b * h * w
    size = dict(range=b * 2 * 4, part=b * 2 * K_RANGE_BLOCKS * 4, air=b * 4 * 4, ascale=b * 4,
                gthr=b * 4, tab=b * K_TAB["stride"] * 4, hist=b * 2048 * 4, st=b * ST_BYTES,
                keys=b * band_rows(h) * w * 4, apart=b * K_FULL_NBLK * 8,
                gpart=b * K_FULL_NBLK * 2 * 8, t0=px * 4, tf=px * 4, h1=px * 16, tmp=px * 16,
                h2=px * 16)
    off, out = 0, {}
    for name in WS_ORDER:
        off = (off + 255) & ~255
        out[name] = (off, size[name])
        off += size[name]
    return out, off


def ws_read(ws, b, h, w):
    """The stages a full call left in its workspace (ws: u8 numpy copy)."""
    lay, total = ws_layout(b, h, w)
    assert ws.size >= total

    def arr(name, dtype, shape):
        o, n = lay[name]
        return ws[o:o + n].view(dtype).reshape(shape)
    st = arr("st", np.uint8, (b, ST_BYTES))
    return dict(range=arr("range", F, (b, 2)), air=arr("air", F, (b, 4)),
                ascale=arr("ascale", F, (b,)), gthr=arr("gthr", F, (b,)),
                tab=arr("tab", F, (b, K_TAB["stride"])),
                st_u32=st[:, :32].copy().view(np.uint32).reshape(b, 8),
                st_sum=st[:, 32:].copy().view(np.float64).reshape(b, 12),
                keys=arr("keys", np.uint32, (b, band_rows(h), w)),
                t0=arr("t0", F, (b, h, w)), tf=arr("tf", F, (b, h, w)))


# --- frames ----------------------------------------------------------------------
def sky_frame(h, w, seed, lo=150, hi=250):
    """road_frame with the top band_h + 4 rows replaced by random u8 in
    [lo, hi): a sky bright enough that the image airlight is not clipped."""
    img = road_frame(h, w, seed)
    rows = band_rows(h) + 4
    rng = np.random.default_rng(seed + 1000)
    img[:rows] = rng.integers(lo, hi, size=(rows, w, 3), dtype=np.uint8)
    return img


def band_frame(h, w, seed, levels):
    """road_frame whose airlight band holds exactly `levels`: [(count, (b, g,
    r))], counts summing to band_h * w, in a seeded shuffle so every level is
    spread over the band (and over fog_lum's blocks)."""
    img = road_frame(h, w, seed)
    n = band_rows(h) * w
    assert sum(c for c, _ in levels) == n
    px = np.concatenate([np.tile(np.array(col, np.uint8), (c, 1)) for c, col in levels])
    px = px[np.random.default_rng(seed + 2000).permutation(n)]
    img[:band_rows(h)] = px.reshape(band_rows(h), w, 3)
    return img


# two colours whose luminance keys (0x3f47cb20, 0x3f47cb60) share their top 22
# bits: the third radix pass (low 10 bits) decides between them
LOWBITS_A, LOWBITS_B = (248, 162, 253), (155, 231, 153)
DARK, MID, HIGH = (60, 60, 60), (180, 180, 180), (230, 230, 230)


def _frame(spec, h, w):
    kind, seed = spec[0], spec[1]
    n = band_rows(h) * w
    k, _ = quantile_rank(n)
    if kind == "road":        # dark band: a + tint < 0.7, the lower clip
        return road_frame(h, w, seed)
    if kind == "sky":         # unclipped airlight
        return sky_frame(h, w, seed)
    if kind == "overbright":  # a + tint > 1 with the forced positive tint: the upper clip
        return sky_frame(h, w, seed, 250, 256)
    if kind == "constant":    # every key equal: same, with_eq, min_gt never written
        return band_frame(h, w, seed, [(n, (200, 190, 180))])
    if kind == "straddle":    # s[k] and s[k+1] on different levels: lerp, thr > a
        return band_frame(h, w, seed, [(k + 1, (90, 90, 90)), (n - k - 1, (200, 210, 220))])
    if kind == "mask100":     # exactly 100 pixels at or above the threshold
        return band_frame(h, w, seed, [(n - 100, DARK), (60, MID), (40, HIGH)])
    if kind == "mask99":      # exactly 99: the whole band is averaged
        return band_frame(h, w, seed, [(n - 99, DARK), (59, MID), (40, HIGH)])
    if kind == "lowbits_a":   # the quantile is key A ...
        return band_frame(h, w, seed, [(k - 99, DARK), (105, LOWBITS_A), (n - k - 6, LOWBITS_B)])
    if kind == "lowbits_b":   # ... or key B, 64 ulps above it
        return band_frame(h, w, seed, [(k - 99, DARK), (95, LOWBITS_A), (n - k + 4, LOWBITS_B)])
    raise KeyError(kind)


# --- cases -----------------------------------------------------------------------
@dataclass
class Case:
    name: str
    geom: str
    frames: tuple                 # ((kind, seed), ...), one per frame of the batch
    kw: dict = field(default_factory=dict)      # FogSynthesizer options
    force: tuple = ()             # per-frame dict of forced draw values
    pad_cols: int = 0             # run through a column-sliced view: pitch = 3 (W + pad)
    claims: tuple = ()            # the paths this case is named for
    twin: str = ""                # the case whose frames, draws and options this one repeats
    seed: int = 21

    @property
    def hw(self):
        return GEOMS[self.geom]

    @property
    def batch(self):
        return len(self.frames)


# DECOY: the frame's switch fp[12] is 0 but a non-zero noise plane is handed over
# for it; the device must not read it
ON, OFF, DECOY = dict(noise=True), dict(noise=False), dict(noise=False, decoy=True)
G1, GP = dict(gamma=1.0), dict(gamma=0.97)

CASES = [
    # every airlight regime in one batch at the API minimum
    Case("min_bands", "min",
         (("sky", 1), ("constant", 2), ("mask100", 3), ("mask99", 4), ("overbright", 5),
          ("road", 6)),
         kw=dict(level="heavy"),
         force=({**ON, **G1}, {**DECOY, **GP}, {**OFF, **G1}, {**OFF, **G1},
                {**ON, **GP, "tint_a": (0.02, 0.015, 0.02)}, {**OFF, **G1}),
         claims=("lum_one_block", "air_unclipped", "air_constant", "air_mask100", "air_mask99",
                 "air_upper_clip", "air_lower_clip", "mid_band_skipped", "gamma_1", "gamma_pow",
                 "noise_on", "noise_off", "rain_0", "core_vector", "glow_unclipped")),
    Case("seg_bands", "seg", (("straddle", 7), ("lowbits_a", 8), ("lowbits_b", 9)),
         kw=dict(level="heavy"), force=({**OFF, **G1}, {**OFF, **G1}, {**OFF, **G1}),
         claims=("air_straddle", "air_lowbits", "sep_h_second_segment")),
    Case("odd_sky", "odd", (("sky", 10), ("road", 11)), kw=dict(level="heavy", rain_p=0.004),
         force=({**ON, **GP}, {**OFF, **G1}),
         claims=("tbil_pair_tail", "sep_h_narrow_segment", "core_scalar", "rain_0.004")),
    Case("odd_sky_pitch", "odd", (("sky", 10), ("road", 11)),
         kw=dict(level="heavy", rain_p=0.004), force=({**ON, **GP}, {**OFF, **G1}), pad_cols=5, twin="odd_sky",
         claims=("pitch_padded", "tbil_pair_tail")),
    Case("seg_pitch_scalar", "seg", (("sky", 12),), kw=dict(level="medium"), force=(GP,),
         pad_cols=1, claims=("pitch_padded", "core_scalar_by_pitch")),
    Case("big_sky", "big", (("sky", 13),), kw=dict(level="heavy", rain_p=0.004, rain_len=5),
         force=({**ON, **GP},),
         claims=("nblk_capped", "rblocks_capped", "sep_h_three_segments", "lum_multi_block",
                 "rain_len_5")),
    Case("min_oct1", "min", (("sky", 14),), kw=dict(perlin_octaves=1, rain_p=1.0),
         force=({**OFF, **G1},), claims=("n_oct_1", "rain_saturated")),
    Case("min_oct4_lds", "min", (("sky", 15),),
         kw=dict(perlin_octaves=4, perlin_scale_ratio=0.05, level="heavy"),
         force=({**ON, **G1},), claims=("n_oct_4", "grid_lds")),
    Case("seg_oct4_global", "seg", (("sky", 16),),
         kw=dict(perlin_octaves=4, perlin_scale_ratio=0.05, level="heavy"),
         force=({**OFF, **GP},), claims=("n_oct_4", "grid_global")),
    Case("seg_blur8", "seg", (("sky", 17),), kw=dict(level="heavy", depth_blur_max=8.0),
         force=({**OFF, **G1},), claims=("two_bands",)),
    Case("seg_blur14", "seg", (("sky", 18),), kw=dict(level="heavy", depth_blur_max=14.0),
         force=({**OFF, **G1, "beta": 0.22},), claims=("two_bands", "rad_13")),
    Case("min_noedge", "min", (("sky", 19),), kw=dict(level="heavy", edge_guided=False),
         force=({**OFF, **G1},), claims=("edge_guided_off",)),
    # one batch whose frames differ in every draw-dependent branch
    Case("seg_mixed3", "seg", (("sky", 20), ("sky", 21), ("sky", 22)),
         kw=dict(level="heavy", depth_blur_max=5.0, rain_p=0.004, rain_len=5),
         force=({**ON, **G1, "glow": 0.2, "cdrop": 0.08, "beta": 0.02},
                {**DECOY, **GP, "glow": 2.0, "cdrop": 0.26, "beta": 0.3},
                {**ON, **G1, "glow": 0.45, "cdrop": 0.15, "beta": 0.6}),
         claims=("mixed_batch",)),
]
BY_NAME = {c.name: c for c in CASES}

_OPT = dict(perlin_octaves="n_oct", perlin_scale_ratio="scale_ratio", depth_blur_max="depth_blur_max",
            edge_guided="edge_guided", rain_p="rain_p", rain_len="rain_len",
            global_veil="global_veil", horizon_softness="softness_ratio")


def oracle_options(case, full=True):
    opt = {_OPT[k]: v for k, v in case.kw.items() if k in _OPT}
    if not full:
        opt.pop("depth_blur_max", None)
        opt.pop("edge_guided", None)
    return opt


def build_frames(case):
    h, w = case.hw
    return np.stack([_frame(s, h, w) for s in case.frames])


def _forced_noise(case, i, h, w):
    return np.random.RandomState(case.seed * 100 + i).normal(0, 0.0035, size=(h, w, 3)).astype(F)


def _draw_args(case):
    kw = case.kw
    return dict(level=kw.get("level", "medium"), mor=kw.get("mor"),
                scale_ratio=kw.get("perlin_scale_ratio", 0.18), n_oct=kw.get("perlin_octaves", 2),
                rain=kw.get("rain_p", 0) > 0)


def oracle_draws(case, full=True):
    """The oracle's per-frame draws with the case's forced values edited in."""
    h, w = case.hw
    rng = np.random.RandomState(case.seed)
    out = []
    for i in range(case.batch):
        fc = case.force[i] if i < len(case.force) else {}
        if not full:
            prm = fog_ref.draw(rng, h, w, **_draw_args(case))
            if "gamma" in fc:
                prm["gamma"] = F(fc["gamma"])
            out.append(prm)
            continue
        prm = fog_ref.draw_full(rng, h, w, **_draw_args(case))
        for key in ("gamma", "glow", "cdrop", "beta"):
            if key in fc:
                prm[key] = float(fc[key])
        if "tint_a" in fc:
            prm["tint_a"] = np.array(fc["tint_a"], F)
        if "noise" in fc:
            prm["noise"] = _forced_noise(case, i, h, w) if fc["noise"] else None
        out.append(prm)
    return out


def device_draws(case, device="cpu", full=True):
    """(FogSynthesizer, its per-frame draws with the same forced values):
    the (params, grids[, noise]) tuples the public draws= argument takes.
    A decoy frame carries a noise plane with its switch off."""
    from rvs_amd.augment import FogSynthesizer, band_radii
    h, w = case.hw
    syn = FogSynthesizer(seed=case.seed, device=device, filters=full, **case.kw)
    out = []
    for i in range(case.batch):
        fc = case.force[i] if i < len(case.force) else {}
        d = syn.draw(h, w)
        p = d[0].copy()
        if "gamma" in fc:
            p[8] = fc["gamma"]
        if not full:
            out.append((p, d[1]))
            continue
        nz = d[2]
        if "noise" in fc:
            nz = _forced_noise(case, i, h, w) if fc["noise"] else None
            if fc.get("decoy"):
                nz = _forced_noise(case, i + 50, h, w) * F(10)
            p[12] = 1.0 if fc["noise"] else 0.0
        if "tint_a" in fc:
            p[1:4] = fc["tint_a"]
        if "glow" in fc:
            g = float(fc["glow"])
            p[10], p[16] = g, int(9 + 20 * g) | 1
            p[17] = int(max(7, (h + w) * (0.003 + 0.01 * g))) | 1
        if "cdrop" in fc:
            p[11], p[18] = fc["cdrop"], int(5 + float(fc["cdrop"]) * 20) | 1
        if "beta" in fc:
            fs = syn._full_scene(h, w)
            p[0] = fc["beta"]
            p[13:16] = band_radii(fs["depth"], fs["bands"], float(fc["beta"]),
                                  syn.depth_blur_max)
        out.append((p, d[1], nz))
    return syn, out


@lru_cache(maxsize=None)
def oracle_full(name):
    """fog_stages_full per frame of a case, computed once per session.  A
    padded-pitch case shares its unpadded twin's frames and draws, hence its
    result."""
    case = BY_NAME[name]
    if case.twin:
        return oracle_full(case.twin)
    frames = build_frames(case)
    return [fog_ref.fog_stages_full(frames[i], prm, **oracle_options(case))
            for i, prm in enumerate(oracle_draws(case))]


@lru_cache(maxsize=None)
def oracle_core(name):
    case = BY_NAME[name]
    if case.twin:
        return oracle_core(case.twin)
    frames = build_frames(case)
    return [fog_ref.fog_frame(frames[i], prm, **oracle_options(case, full=False))
            for i, prm in enumerate(oracle_draws(case, full=False))]


# --- regions of the byte comparison ---------------------------------------------
def _near_multiples(n, pitch, r):
    i = np.arange(n)
    m = np.zeros(n, bool)
    for e in range(pitch, n, pitch):
        m |= (i >= e - r) & (i < e + r)
    return m


def regions(h, w, st=None):
    """{name: (h, w) bool mask}.  `st` (a frame's oracle stages) gives the
    filter radii and the active depth bands; without it (the core) only the
    geometry regions are returned.  A radius is capped at a quarter of the
    tile pitch so that a region never becomes the whole frame."""
    out = {}
    full = np.ones((h, w), bool)
    segs, _ = sep_h_segments(w)
    rad = 4
    if st is not None:
        rad = max([st["glow_k"] // 2, st["glow_k2"] // 2] + [r // 2 for _, r in st["bands"]])
    if segs > 1:
        out["last_segment"] = full & (np.arange(w) >= 256 * (segs - 1))[None, :]
        out["seam_256"] = full & _near_multiples(w, 256, rad)[None, :]
    out["tile64_cols"] = full & _near_multiples(w, 64, min(rad, 16))[None, :]
    out["tile16_rows"] = full & _near_multiples(h, 16, min(rad, 4))[:, None]
    out["tile32_cols"] = full & _near_multiples(w, 32, min(rad, 8))[None, :]
    out["tile32_rows"] = full & _near_multiples(h, 32, min(rad, 8))[:, None]
    ring = np.ones((h, w), bool)
    b = min(rad, 8)
    ring[b:h - b, b:w - b] = False
    out["border"] = ring
    if st is not None:
        depth, _ = fog_ref.depth_and_sky(h, w)
        edges = (0.0, 0.33, 0.66, 1.0)
        for i, _r in st["bands"]:
            rows = ((depth >= F(0) if i == 0 else depth >= edges[i]) &
                    (depth < edges[i + 1])).any(axis=1)
            out[f"band{i}_rows"] = full & rows[:, None]
    return {k: v for k, v in out.items() if v.any()}


def byte_report(got, ref, regs, dmax, share):
    """Failures (strings) of the per-frame and per-region byte bars: no
    |d| > dmax; per frame at least 1 - share exact; per region of N values at
    most max(ceil(share N), 2) inexact."""
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    bad = []
    exact = float((d == 0).mean())
    print(f"  frame: max |d| {d.max()}, exact {exact:.5f}")
    if d.max() > dmax:
        bad.append(f"max |d| {d.max()} > {dmax}")
    if exact < 1 - share:
        bad.append(f"exact share {exact:.5f} < {1 - share}")
    for name, m in regs.items():
        n = int(m.sum()) * 3
        inexact = int((d[m] != 0).sum())
        allow = max(math.ceil(share * n), 2)
        print(f"  {name}: {inexact} of {n} inexact (allowed {allow})")
        if inexact > allow:
            bad.append(f"{name}: {inexact} of {n} inexact > {allow}")
    return bad

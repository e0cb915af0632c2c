"""The fog cases (tests/fog_cases.py) take the paths they are named for.

No GPU: every check runs on the oracle (oracle/fog_ref.py), on the host
draw (rvs_amd/augment/fog.py) and on the restated predicates.  If a case
stops meeting its regime (a frame builder, a preset or a constant of
augment.hip changes), this file fails, not the GPU parity test silently
losing its coverage.
"""
import numpy as np
import pytest

import fog_cases as fc
from oracle import fog_ref

F = np.float32


def _frame_of(case, kind):
    return [i for i, s in enumerate(case.frames) if s[0] == kind][0]


def _regime(case, st, kind):
    return fc.airlight_regime(st[_frame_of(case, kind)]["lum"])


def _band_pixels(h, w, band):
    from rvs_amd.augment import depth_band_map, fog_depth
    return int((depth_band_map(fog_depth(h, w)) == band).sum())


def _lowbits(case, st):
    ka = fc.select_state(st[_frame_of(case, "lowbits_a")]["lum"])[0]
    kb = fc.select_state(st[_frame_of(case, "lowbits_b")]["lum"])[0]
    return ka != kb and ka >> 10 == kb >> 10 and (ka, kb) == (0x3f47cb20, 0x3f47cb60)


def _inside(st, prm):
    v = st["a_rgb_raw"] + prm["tint_a"]
    return bool(((v > 0.7) & (v < 1.0)).all() and np.array_equal(st["a_rgb"], v))


# claim -> predicate(case, per-frame stages, per-frame oracle draws, per-frame device draws)
PATHS = {
    "lum_one_block": lambda c, st, pr, dd: fc.lum_blocks(*c.hw) == 1,
    "lum_multi_block": lambda c, st, pr, dd: fc.lum_blocks(*c.hw) == 8,
    "air_unclipped": lambda c, st, pr, dd: _inside(st[_frame_of(c, "sky")],
                                                   pr[_frame_of(c, "sky")]),
    "air_constant": lambda c, st, pr, dd: _regime(c, st, "constant") == (True, True, False) and
    np.unique(st[_frame_of(c, "constant")]["lum"]).size == 1,
    "air_straddle": lambda c, st, pr, dd: _regime(c, st, "straddle") == (False, False, False),
    "air_mask100": lambda c, st, pr, dd: st[_frame_of(c, "mask100")]["mask_count"] == 100 and
    _regime(c, st, "mask100") == (True, True, False) and
    _inside(st[_frame_of(c, "mask100")], pr[_frame_of(c, "mask100")]),
    "air_mask99": lambda c, st, pr, dd: st[_frame_of(c, "mask99")]["mask_count"] == 99 and
    _regime(c, st, "mask99") == (True, True, True),
    "air_upper_clip": lambda c, st, pr, dd: bool(
        (st[_frame_of(c, "overbright")]["a_rgb"] == 1.0).all() and
        (st[_frame_of(c, "overbright")]["a_rgb_raw"] + pr[_frame_of(c, "overbright")]["tint_a"]
         > 1.0).all()),
    "air_lower_clip": lambda c, st, pr, dd: bool(
        (st[_frame_of(c, "road")]["a_rgb"] == F(0.7)).all() and
        (st[_frame_of(c, "road")]["a_rgb_raw"] + pr[_frame_of(c, "road")]["tint_a"] < 0.7).all()),
    "air_lowbits": lambda c, st, pr, dd: _lowbits(c, st),
    "mid_band_skipped": lambda c, st, pr, dd: _band_pixels(*c.hw, 1) == 64 and
    all(1 not in [b for b, _ in s["bands"]] for s in st),
    "gamma_1": lambda c, st, pr, dd: any(d[0][8] == 1.0 and p["gamma"] == 1.0
                                         for d, p in zip(dd, pr)),
    "gamma_pow": lambda c, st, pr, dd: any(d[0][8] != 1.0 and p["gamma"] != 1.0
                                           for d, p in zip(dd, pr)),
    "noise_on": lambda c, st, pr, dd: any(d[0][12] == 1.0 and d[2] is not None and
                                          p["noise"] is not None for d, p in zip(dd, pr)),
    # off twice: no plane at all, and a non-zero decoy plane behind a switch that is off
    "noise_off": lambda c, st, pr, dd: any(d[0][12] == 0.0 and d[2] is None and
                                           p["noise"] is None for d, p in zip(dd, pr)) and
    any(d[0][12] == 0.0 and d[2] is not None and np.abs(d[2]).max() > 0.05 and
        p["noise"] is None for d, p in zip(dd, pr)),
    "rain_0": lambda c, st, pr, dd: c.kw.get("rain_p", 0.0) == 0.0,
    "rain_0.004": lambda c, st, pr, dd: c.kw["rain_p"] == 0.004 and c.kw.get("rain_len", 16) == 16,
    "rain_len_5": lambda c, st, pr, dd: c.kw["rain_p"] == 0.004 and c.kw["rain_len"] == 5,
    # rain_thresh saturates at 2^32 - 1: every hash but that one value streaks
    "rain_saturated": lambda c, st, pr, dd: c.kw["rain_p"] == 1.0 and
    min(float(F(c.kw["rain_p"])) * 4294967296.0, 4294967295.0) == 4294967295.0,
    "sep_h_second_segment": lambda c, st, pr, dd: fc.sep_h_segments(c.hw[1]) == (2, 44) and
    c.hw[1] % 4 == 0,
    "sep_h_narrow_segment": lambda c, st, pr, dd: fc.sep_h_segments(c.hw[1]) == (2, 3),
    "sep_h_three_segments": lambda c, st, pr, dd: fc.sep_h_segments(c.hw[1]) == (3, 8),
    "tbil_pair_tail": lambda c, st, pr, dd: c.hw[1] % 2 == 1,
    "core_vector": lambda c, st, pr, dd: fc.core_vector(c.hw[1], 3 * (c.hw[1] + c.pad_cols)),
    "core_scalar": lambda c, st, pr, dd: c.hw[1] % 4 != 0 and
    not fc.core_vector(c.hw[1], 3 * c.hw[1]),
    "core_scalar_by_pitch": lambda c, st, pr, dd: c.hw[1] % 4 == 0 and
    not fc.core_vector(c.hw[1], 3 * (c.hw[1] + c.pad_cols)),
    "pitch_padded": lambda c, st, pr, dd: c.pad_cols > 0,
    "nblk_capped": lambda c, st, pr, dd: fc.ceil_div(c.hw[0] * c.hw[1], 256) > fc.nblk(*c.hw)
    == 512 and fc.second_trip_blocks(*c.hw) == 17,
    "rblocks_capped": lambda c, st, pr, dd: fc.ceil_div(c.hw[0] * c.hw[1], 256) >
    fc.rblocks(*c.hw) == 256,
    "n_oct_1": lambda c, st, pr, dd: c.kw["perlin_octaves"] == 1 and len(pr[0]["grids"]) == 1,
    "n_oct_4": lambda c, st, pr, dd: c.kw["perlin_octaves"] == 4 and len(pr[0]["grids"]) == 4,
    "grid_lds": lambda c, st, pr, dd: fc.grid_stride(*c.hw, 0.05, 4) == 1484 == dd[0][1].size and
    fc.grid_lds(*c.hw, 0.05, 4),
    "grid_global": lambda c, st, pr, dd: fc.grid_stride(*c.hw, 0.05, 4) == 7506 == dd[0][1].size
    and not fc.grid_lds(*c.hw, 0.05, 4),
    "two_bands": lambda c, st, pr, dd: [b for b, _ in st[0]["bands"]] == [1, 2] and
    min(r for _, r in st[0]["bands"]) > 1,
    "rad_13": lambda c, st, pr, dd: max(r for _, r in st[0]["bands"]) == 13,
    "edge_guided_off": lambda c, st, pr, dd: c.kw["edge_guided"] is False and
    st[0]["t"] is st[0]["t0"],
    "glow_unclipped": lambda c, st, pr, dd: 0.65 < st[0]["glow_thr_raw"] < 0.9 and
    st[0]["glow_thr"] == st[0]["glow_thr_raw"],
    "mixed_batch": lambda c, st, pr, dd: [d[0][12] for d in dd] == [1.0, 0.0, 1.0] and
    [d[0][8] == 1.0 for d in dd] == [True, False, True] and dd[1][2] is not None and
    len({int(d[0][16]) for d in dd}) == 3 and len({int(d[0][17]) for d in dd}) >= 2 and
    len({int(d[0][18]) for d in dd}) == 3 and
    len({tuple(b for b, _ in s["bands"]) for s in st}) >= 2 and
    len({tuple(s["bands"]) for s in st}) == 3,
}


@pytest.fixture(scope="module", params=fc.CASES, ids=lambda c: c.name)
def case_data(request):
    c = request.param
    _, dd = fc.device_draws(c)
    return c, fc.oracle_full(c.name), fc.oracle_draws(c), dd


def test_every_path_is_claimed():
    claimed = {p for c in fc.CASES for p in c.claims}
    assert claimed == set(PATHS), (set(PATHS) - claimed, claimed - set(PATHS))
    assert {c.geom for c in fc.CASES} == set(fc.GEOMS)
    assert max(h * w for h, w in fc.GEOMS.values()) == 260 * 520


def test_case_takes_its_paths(case_data):
    c, st, pr, dd = case_data
    assert c.claims
    for claim in c.claims:
        assert PATHS[claim](c, st, pr, dd), f"{c.name} no longer takes {claim}"


def test_forced_draws_agree(case_data):
    """The draw tuples handed to the device carry the values the oracle's
    dict carries, forced ones included, and the filter sizes derived from
    them are the ones the oracle uses."""
    c, st, pr, dd = case_data
    for i, (s, p, d) in enumerate(zip(st, pr, dd)):
        q, grids, nz = d
        want = c.force[i] if i < len(c.force) else {}
        for key, slot in (("gamma", 8), ("glow", 10), ("cdrop", 11), ("beta", 0)):
            if key in want:
                assert p[key] == want[key] and q[slot] == F(want[key])
        assert q[0] == F(p["beta"]) and q[4] == F(p["a_target"]) and q[8] == F(p["gamma"])
        np.testing.assert_array_equal(q[1:4], p["tint_a"])
        np.testing.assert_array_equal(q[5:8], p["tint"])
        assert int(q[9]) == p["rain_seed"]
        assert q[10] == F(p["glow"]) and q[11] == F(p["cdrop"])
        assert q[12] == (p["noise"] is not None) and (nz is not None or p["noise"] is None)
        if p["noise"] is not None:
            np.testing.assert_array_equal(nz, p["noise"])
        else:
            assert nz is None or want.get("decoy")
        np.testing.assert_array_equal(grids, np.concatenate([g.ravel() for g in p["grids"]]))
        assert (int(q[16]), int(q[17]), int(q[18])) == (s["glow_k"], s["glow_k2"], s["fade_d"])
        assert [(b, int(q[13 + b])) for b in range(3) if q[13 + b] > 0] == s["bands"]
        assert fc.bands_returning_early(q) == [b not in dict(s["bands"]) for b in range(3)]
        assert max(s["glow_k"], s["glow_k2"]) <= 2 * fc.K_SEP_RMAX + 1 and s["fade_d"] <= 15
        # the hard glow mask is neither empty nor everything
        assert 0.01 < s["glow_share"] < 0.99, s["glow_share"]


def test_predicates_at_the_named_geometries():
    assert [fc.lum_blocks(*fc.GEOMS[g]) for g in ("min", "seg", "odd", "big")] == [1, 2, 2, 8]
    assert [fc.nblk(*fc.GEOMS[g]) for g in ("min", "seg", "odd", "big")] == [16, 85, 68, 512]
    assert [fc.rblocks(*fc.GEOMS[g]) for g in ("min", "seg", "odd", "big")] == [16, 85, 68, 256]
    assert [fc.second_trip_blocks(*fc.GEOMS[g]) for g in ("min", "seg", "big")] == [0, 0, 17]
    assert fc.quantile_rank(640)[0] == 575 and fc.quantile_rank(3000)[0] == 2699
    assert fc.band_rows(64) == 10 and fc.band_rows(260) == 31
    assert fc.grid_stride(64, 64) > 0 and fc.grid_lds(64, 64) and fc.grid_lds(260, 520)
    # fog_sep_v at the minimum is 2 x 2 blocks; every 64 x 16 tile meets a border
    assert (fc.ceil_div(64, 32), fc.ceil_div(64, 32)) == (2, 2) and fc.ceil_div(64, 64) == 1
    from rvs_amd.augment import quantile_consts
    for n in (640, 3000, 2590, 16120):
        k, t = quantile_consts(n)
        assert (k, F(t)) == fc.quantile_rank(n)


def test_workspace_layout_matches_the_library():
    """The restated layout's total equals rv_fog_full_ws_bytes over a grid of
    geometries; the GPU test reads the stages through this layout."""
    from rvs_amd import _lib
    lib = _lib.load()
    for b in (1, 2, 3, 6, 16):
        for h, w in list(fc.GEOMS.values()) + [(65, 97), (128, 128), (360, 641), (1280, 1280)]:
            lay, total = fc.ws_layout(b, h, w)
            assert total == lib.rv_fog_full_ws_bytes(b, h, w), (b, h, w)
            assert all(o % 256 == 0 for o, _ in lay.values())
    lay, _ = fc.ws_layout(2, 64, 64)
    assert lay["st"][1] == 2 * 128 and lay["tab"][1] == 2 * 576 * 4
    assert list(lay) == list(fc.WS_ORDER)


def _frame_full_before_stages(img, prm, depth_blur_max=3.5, edge_guided=True, scale_ratio=0.18,
                              n_oct=2, rain_p=0.0, rain_len=16):
    """fog_frame_full as it read before fog_stages_full existed (default
    scene ratios), from the oracle's public pieces."""
    h, w = img.shape[:2]
    x = img.astype(F) / 255.0
    depth, sw = fog_ref.depth_and_sky(h, w)
    octs, norm = fog_ref.octaves(h, w, scale_ratio, n_oct)
    nz = fog_ref.noise(h, w, prm["grids"], octs, norm)
    nn = (nz - nz.min()) / max(F(1e-6), nz.max() - nz.min())
    beta_map = (prm["beta"] * (F(0.85) + F(0.35) * nn)).astype(F)
    a_rgb = np.clip(fog_ref.airlight_rgb(x) + prm["tint_a"], 0.7, 1.0)
    vg = np.linspace(1.0, 0.85, h, dtype=F)[:, None, None]
    xg = np.linspace(0.95, 1.05, w, dtype=F)[None, :, None]
    amap = vg * a_rgb[None, None, :] * xg
    for c in range(3):
        amap[:, :, c] = fog_ref.bilateral_f32(amap[:, :, c], 33, 12, 12)
    amap = np.clip(amap, 0.7, 1.0)
    scale = prm["a_target"] / max(1e-6, amap.mean())
    amap = np.clip(amap * scale, 0.75, 1.0)
    t = np.clip(np.exp(-beta_map * depth), 0.05, 1.0)
    if edge_guided:
        t = np.clip(fog_ref.bilateral_f32(t, 17, 12, 12), 0.05, 1.0)
    t3 = t[..., None]
    hazy = x * t3 + amap * (1.0 - t3)
    gv = (0.06 * (0.6 + 0.4 * sw))[:, None, None]
    hazy = np.clip(hazy * (1.0 - gv) + amap * gv, 0, 1)
    hazy = fog_ref.glow(hazy, prm["glow"])
    hazy = fog_ref.depth_blur(hazy, depth, prm["beta"], depth_blur_max)
    hazy = fog_ref.contrast_fade(hazy, prm["cdrop"])
    hazy = np.clip(hazy * prm["tint"][None, None, :], 0, 1)
    if prm["gamma"] != 1.0:
        hazy = np.clip(hazy ** prm["gamma"], 0, 1)
    if prm["noise"] is not None:
        hazy = np.clip(hazy + prm["noise"], 0, 1)
    if rain_p > 0:
        thr = np.uint32(min(float(np.float32(rain_p)) * 4294967296.0, 4294967295.0))
        yi, xi = np.arange(h)[:, None], np.arange(w)[None, :]
        col = (xi + (yi >> 2)).astype(np.uint32)
        seg = np.broadcast_to((yi // int(rain_len)).astype(np.uint32), col.shape)
        hsh = fog_ref._lowbias32(np.uint32(prm["rain_seed"]) ^ fog_ref._lowbias32(
            col * np.uint32(0x9E3779B1) + fog_ref._lowbias32(seg)))
        hazy = np.where((hsh < thr)[..., None], hazy + (F(1) - hazy) * F(0.45), hazy)
    return (hazy * 255.0 + 0.5).astype(np.uint8)


@pytest.mark.parametrize("name,frame", [("min_oct1", 0), ("seg_mixed3", 1), ("odd_sky", 0)])
def test_stages_and_frame_are_one_computation(name, frame):
    """fog_frame_full is fog_stages_full's `out`, and both equal the function
    as it read before the stages were returned, on three shapes."""
    c = fc.BY_NAME[name]
    img, prm = fc.build_frames(c)[frame], fc.oracle_draws(c)[frame]
    opt = fc.oracle_options(c)
    st = fc.oracle_full(name)[frame]
    np.testing.assert_array_equal(fog_ref.fog_frame_full(img, prm, **opt), st["out"])
    np.testing.assert_array_equal(_frame_full_before_stages(img, prm, **opt), st["out"])
    for key in ("noise_min", "noise_max", "lum", "thr", "mask_count", "a_rgb_raw", "a_rgb",
                "amap_mean", "amap_scale", "t0", "t", "glow_thr", "glow_thr_raw", "glow_share",
                "glow_k", "glow_k2", "kernels", "bands", "fade_d", "out"):
        assert key in st
    assert st["t0"].dtype == F and st["t"].dtype == F and st["lum"].dtype == F


def test_sky_band_makes_the_airlight_observable():
    """With the dark road band every frame runs at a = 0.7 whatever the
    kernels computed; with the sky band more than half of the output bytes
    below the band change (heavy fog), so a wrong airlight changes the bytes."""
    c = fc.BY_NAME["min_oct4_lds"]
    h, w = c.hw
    prm, opt = fc.oracle_draws(c)[0], fc.oracle_options(c)
    seed = c.frames[0][1]
    from conftest import road_frame
    dark = fog_ref.fog_stages_full(road_frame(h, w, seed), prm, **opt)
    sky = fc.oracle_full(c.name)[0]
    assert (dark["a_rgb"] == F(0.7)).all() and (sky["a_rgb"] > 0.75).all()
    rows = fc.band_rows(h) + 4
    assert np.array_equal(road_frame(h, w, seed)[rows:], fc.sky_frame(h, w, seed)[rows:])
    assert (dark["out"][rows:] != sky["out"][rows:]).mean() > 0.5


@pytest.mark.parametrize("name,frame", [("min_bands", 0), ("seg_blur14", 0), ("odd_sky", 1)])
def test_stage_planes_show_a_misplaced_tap(name, frame):
    """The t0 / tf planes vary enough that reading a neighbour instead of the
    pixel itself breaks the plane bar (5e-5): at least 5 % of the elements
    differ from the plane shifted by one pixel, in x and in y, by more than
    ten times the bar.  One frame per geometry up to 72 x 300 (beta 0.12 to
    0.22); at 260 x 520 the planes are too smooth in x for this (0.3 %), and
    the byte regions carry that geometry."""
    st = fc.oracle_full(name)[frame]
    for key in ("t0", "t"):
        p = st[key]
        sx = float((np.abs(p[:, 1:] - p[:, :-1]) > 5e-4).mean())
        sy = float((np.abs(p[1:] - p[:-1]) > 5e-4).mean())
        print(f"{name} {key}: x share {sx:.3f}, y share {sy:.3f}")
        assert sx >= 0.05 and sy >= 0.05


def test_regions_cover_their_names():
    for g, (h, w) in fc.GEOMS.items():
        st = fc.oracle_full({"min": "min_oct1", "seg": "seg_blur14", "odd": "odd_sky",
                             "big": "big_sky"}[g])[0]
        regs = fc.regions(h, w, st)
        segs, last = fc.sep_h_segments(w)
        assert ("last_segment" in regs) == (segs > 1)
        if segs > 1:
            assert regs["last_segment"].sum() == h * last
            assert regs["seam_256"][:, 255].all() and regs["seam_256"][:, 256].all()
        assert regs["border"][0].all() and regs["border"][:, -1].all()
        assert not regs["border"][h // 2, w // 2]
        for b, _ in st["bands"]:
            assert 0 < regs[f"band{b}_rows"].sum() < h * w
        assert all(0 < m.sum() < h * w for m in regs.values())
    assert set(fc.regions(72, 300, fc.oracle_full("seg_blur14")[0])) >= {"band1_rows",
                                                                        "band2_rows"}

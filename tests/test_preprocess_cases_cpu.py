"""The cases of tests/preprocess_cases.py run the kernel paths and reach the
data regimes they are named for -- from the host predicates and the oracle
alone, no GPU.  These are conditions on the inputs, not tolerances: were one
to fail, test_preprocess_paths_gpu.py would be comparing some other path of
csrc/preprocess.hip than it says.  The restated predicates are held to the
library's own host queries (rv_clahe_median_fits,
rv_clahe_median_letterbox_fits, rv_preprocess_chain_route), so they cannot
drift from the source they cite."""
import ctypes

import numpy as np
import pytest
import scipy.ndimage

import preprocess_cases as pc
from oracle import cpu


def _path(case):
    pitch, base = pc.pitch_base(case.layout, case.W)
    return pc.path_of(case.entry, case.H, case.W, case.tiles, case.k, pitch, base, case.gate,
                      pc.case_geo(case))


def _tagged(tag):
    got = [c for c in pc.cases().values() if c.tag == tag]
    assert got, tag
    return got


# ---------------------------------------------------------------------------
# paths
# ---------------------------------------------------------------------------
def test_every_case_takes_the_path_it_is_named_for():
    wrong = {n: (_path(c), c.expect_path) for n, c in pc.cases().items() if _path(c) != c.expect_path}
    assert not wrong, wrong


def test_every_value_of_every_axis_is_covered():
    paths = [c.expect_path for c in pc.cases().values()]
    assert {p.hist for p in paths} == {None, "packed16", "packed_wide", "u32"}
    assert {p.loader for p in paths} == {None, "vec", "mixed", "scalar"}
    assert {p.applier for p in paths} == {None, "apply", "med3", "tile<3>", "tile<5>", "tile<7>",
                                          "tile<9>"}
    assert {p.io for p in paths} == {None, "vec", "scalar"}
    assert {p.route for p in paths} == {None, "fused", "fused_gated", "ops"}
    # ... and the ones that meet: every histogram form under both loaders that
    # reach it, the three YCrCb appliers behind CLAHE, med3 with and without dwords
    # on a misaligned base, the 16-byte copy of the gated op-by-op route
    combos = {(p.hist, p.loader) for p in paths}
    assert {("u32", "vec"), ("packed_wide", "vec"), ("packed_wide", "scalar"), ("packed16", "vec"),
            ("packed16", "scalar"), ("packed16", "mixed")} <= combos
    behind_clahe = {p.applier for c in pc.cases().values() for p in [c.expect_path]
                    if c.entry == "clahe_median"}
    assert behind_clahe >= {"med3", "tile<3>", "tile<5>", "tile<7>", "tile<9>"}
    mis = {(c.entry, c.layout) for c in pc.cases().values() if c.layout != "contig"}
    entries = {"clahe_ycrcb", "clahe_lab", "median", "clahe_median", "clahe_median_letterbox",
               "chain"}
    assert mis >= {(e, lay) for e in entries for lay in pc.LAYOUTS}
    assert ("gray_span", "in_mis") in mis
    gated_ops = [c for c in pc.cases().values() if c.gate and c.expect_path.route == "ops"]
    assert any(c.layout == "contig" and (3 * c.W) % 16 == 0 for c in gated_ops)  # uint4 copies
    assert any(c.layout != "contig" for c in gated_ops)                           # byte copies


def test_geometries_named_in_the_table():
    """The tile sizes the histogram and loader cases are named for."""
    g = pc.make_geo
    assert g(1024, 1024, 1)[1:3] == (1024, 1024) and not pc.clahe_packed_ok(g(1024, 1024, 1))
    big = g(1023, 1024, 1)
    assert pc.clahe_packed_ok(big) and 8 * (4 * 1023 + 4092) == 65472 <= 65535
    assert g(512, 514, 2)[1:3] == (257, 256) and 257 * 256 == 65792 > 65535
    assert g(510, 512, 2)[1:3] == (256, 255) and 256 * 255 == 65280 <= 65535
    # groups of four pixels per tile row: 1; 257 (dr = 256 // groups = 0); 129 .. 255
    assert g(32, 32, 8).tw // 4 == 1
    assert g(16, 2056, 2).tw // 4 == 257 and pc.clahe_packed_ok(g(16, 2056, 2))
    assert 129 <= g(260, 1032, 2).tw // 4 <= 255
    # the grid is larger than the frame: reflect101 folds more than once on the
    # rows of 3 x 5 (5 padded rows, 2 to fold over) and on both axes of 1 x 1
    assert g(3, 5, 8)[1:3] == (1, 1) and 8 - 3 > 3 - 1 and g(1, 1, 8)[1:3] == (1, 1)
    # median_tile_kernel<3, true> is reached (tiles = 16 at 512 x 512) ...
    assert not pc.med3_cells_fit(g(512, 512, 16)) and pc.lut_window_fits(g(512, 512, 16), 3)
    # ... and every batch grid of med3_kernel named: fewer than 8 blocks, no multiple of 8
    blocks = lambda H, W, B: -(-W // 128) * -(-H // 32) * B  # noqa: E731
    assert blocks(32, 128, 3) == 3 and blocks(70, 130, 3) == 18


def _lib():
    from rvs_amd import _lib
    return _lib.load()


def _shapes():
    step = list(range(1, 301, 23)) + [300]
    table = {(c.H, c.W) for c in pc.cases().values()}
    return sorted({(h, w) for h in step for w in step} | table)


def test_restated_fits_agree_with_the_library():
    lib = _lib()
    tiles = list(range(1, 65))
    n = yes = 0
    for H, W in _shapes():
        for t in tiles if H * W < 10 ** 5 else (1, 2, 8, 64):
            for k in pc.KS:
                want = bool(lib.rv_clahe_median_fits(H, W, t, k))
                assert want == pc.clahe_median_fits(H, W, t, k), (H, W, t, k)
                n, yes = n + 1, yes + want
    assert n > 50000 and 0.1 < yes / n < 0.9, (n, yes)
    assert not lib.rv_clahe_median_fits(64, 64, 0, 3) and not lib.rv_clahe_median_fits(64, 64, 65, 3)


def test_restated_letterbox_and_route_agree_with_the_library():
    from rvs_amd import _lib, kernels
    lib = _lib.load()
    n = 0
    for H, W in _shapes():
        for imgsz in (64, 131, 640):
            geo = cpu.letterbox_geometry(H, W, imgsz, 32)
            arr = _lib.int_array([0] * 6)
            assert lib.rv_letterbox_geometry(H, W, imgsz, 32, arr) == 0 and tuple(arr) == geo
            if not pc.lbgeo_ok(geo):
                continue
            for t in (1, 2, 3, 8, 16, 64):
                for k in (3, 5):
                    want = bool(lib.rv_clahe_median_letterbox_fits(H, W, t, k, _lib.int_array(geo)))
                    assert pc.letterbox_fits(H, W, t, k, geo) == want, (H, W, imgsz, t, k)
                    if t == 1:
                        continue  # a chain's CLAHE takes tiles 2 .. 64
                    ops = [("clahe", "YCrCb", t, 2.0), ("median", k)]
                    for gate in (False, True):
                        desc = kernels.chain_desc(ops, gate_on=gate)
                        for g in (geo, None):
                            assert kernels.preprocess_chain_route(desc, H, W, g) == \
                                pc.chain_route(ops, True, gate, H, W, g), (H, W, imgsz, t, k, gate, g)
                            n += 1
    assert n > 10000
    # other chains: one op, the ops the other way round, Lab, disabled, empty
    for ops, enabled in [([("median", 3)], True), ([("median", 3), ("clahe", "YCrCb", 8, 2.0)], True),
                         ([("clahe", "LAB", 2, 2.0), ("median", 3)], True),
                         ([("clahe", "YCrCb", 2, 2.0), ("median", 3)], False), ([], True)]:
        desc = kernels.chain_desc(ops, enabled=enabled)
        assert kernels.preprocess_chain_route(desc, 64, 128) == pc.ROUTE_OPS == \
            pc.chain_route(ops, enabled, False, 64, 128)


def test_letterbox_forms():
    """The fused letterbox cases have the form they are named for."""
    for (H, W), (ok, form) in pc.LETTERBOX.items():
        geo = cpu.letterbox_geometry(H, W, pc.LB_IMGSZ, 32)
        oh, ow, nh, nw, top, left = geo
        assert pc.letterbox_fits(H, W, 2, 3, geo) == ok, (H, W, form)
        assert bool(_lib().rv_clahe_median_letterbox_fits(H, W, 2, 3, (ctypes.c_int * 6)(*geo))) == ok
        x0, x1, wx = pc.lb_taps(nw, 1.0 / (nw / W), W, False)
        y0, y1, wy = pc.lb_taps(nh, 1.0 / (nh / H), H, True)
        if form.startswith("half-weight"):
            assert (W / nw, H / nh) == (2, 2) and (wx == 1024).all() and (wy == 1024).all()
        elif form.startswith("copy"):
            assert (W / nw, H / nh) == (3, 3) and pc.lb_is_copy(geo, H, W)
            assert (x0 == 3 * np.arange(nw) + 1).all()
        elif form.startswith("blend across"):
            assert (W / nw, H / nh) == (6, 6) and (wx == 1024).all() and not pc.lb_is_copy(geo, H, W)
            assert -(-W // 128) * -(-H // 32) == 18
        elif form == "identity":
            assert geo == (H, W, H, W, 0, 0) and pc.lb_is_copy(geo, H, W)
        elif form.startswith("scale 1"):
            assert (nh, nw) == (H, W) and top > 0 and oh > H
        elif form == "upscale":
            assert nw > W and nh > H
        else:
            assert nw <= W and nh <= H  # a downscale, but some tap pair lies in two blocks
            assert (x0 // 128 != x1 // 128).any() or (y0 // 32 != y1 // 32).any()
    # the layout cases' letterbox: scale 1 on a frame two blocks wide
    assert pc.letterbox_fits(70, 131, 3, 3, cpu.letterbox_geometry(70, 131, 131, 32))


# ---------------------------------------------------------------------------
# CLAHE regimes
# ---------------------------------------------------------------------------
def _stats(case):
    space = "LAB" if case.entry == "clahe_lab" else "YCrCb"
    return [pc.stats_of(s, case.H, case.W, space, case.tiles, case.clip) for s in case.frame]


def test_clahe_restatement_agrees_with_the_oracle_on_every_case():
    seen = set()
    for c in pc.cases().values():
        if c.group not in ("clahe", "colour") or c.entry == "clahe_median":
            continue
        space = "LAB" if c.entry == "clahe_lab" else "YCrCb"
        for s in c.frame:
            key = (s, c.H, c.W, space, c.tiles, c.clip)
            if key in seen:
                continue
            seen.add(key)
            plane = pc.luma_plane(pc.make_frame(s, c.H, c.W), space)
            np.testing.assert_array_equal(pc.stats_of(*key)["out"], cpu.clahe_u8c1(plane, c.tiles, c.clip),
                                          err_msg=c.name)
    assert len(seen) > 40


def test_flat_cases_have_a_bin_above_65535():
    for tag in ("flat", "flat_redistribute", "flat_clip0"):
        for c in _tagged(tag):
            for st in _stats(c):
                assert st["max_bin"].min() > 65535, c.name
    # the packed16 bound: one bin holds all 65 280 pixels of a tile, 255 short of a carry
    for c in _tagged("flat16"):
        for st in _stats(c):
            assert st["max_bin"].max() == 65280, c.name
    assert any((st["max_bin"] == 65280).all() for c in _tagged("flat16") for st in _stats(c))


def test_flat_split_is_an_even_odd_pair():
    """The two bins share a half-word pair of the packed histogram; with the
    split at a quarter of the width the left tiles hold both."""
    for c in pc.cases().values():
        for s in c.frame:
            if s[0] != "flat_split" or c.entry == "clahe_lab":
                continue
            plane = pc.luma_plane(pc.make_frame(s, c.H, c.W))
            vals = np.unique(plane)
            assert vals.tolist() == [s[1], s[1] + 1] and vals[0] % 2 == 0 and vals[0] >> 1 == vals[1] >> 1
            st = pc.stats_of(s, c.H, c.W, "YCrCb", c.tiles, c.clip)
            if 0 < c.W * s[2] // s[3] < pc.make_geo(c.H, c.W, c.tiles).tw:
                assert st["bins"][0, 0] == 2, c.name   # one tile counts both halves of a word
    # 512 x 514 at tiles = 2: 65 536 pixels in the even bin beside 256 in the odd one, and
    # the other way round -- a carry out of either half lands in a bin that is in use
    for num, big in [(256, 100), (1, 101)]:
        plane = pc.luma_plane(pc.make_frame(("flat_split", 100, num, 514), 512, 514))
        h = np.bincount(plane[:256, :257].ravel(), minlength=256)
        assert h[big] == 65536 and h[big ^ 1] == 256
    # 510 x 512 at tiles = 2, split at a quarter: 128 and 128 columns of 255 rows in tile (0, 0)
    st = pc.stats_of(("flat_split", 100, 1, 4), 510, 512, "YCrCb", 2, 2.0)
    assert st["max_bin"][0, 0] == 128 * 255 and st["bins"].tolist() == [[2, 1], [2, 1]]


def test_redistribution_regimes():
    for c in _tagged("flat_redistribute"):   # 512 x 514, clip 2: batch > 0, residual > 128
        for st in _stats(c):
            assert st["clip_limit"] == int(2.0 * 65792 / 256) == 514
            assert (st["batch"] > 0).all() and (st["residual"] > 128).all(), (c.name, st["residual"])
    for c in _tagged("flat_clip0"):
        assert all(st["clip_limit"] == 0 for st in _stats(c))
    assert any(c.clip == 0.0 for c in pc.cases().values() if c.group == "colour")
    for c in _tagged("road_clip2"):          # every class of residual: step 1, step 2, step >= 3
        if c.entry == "clahe_lab":
            continue
        r = _stats(c)[0]["residual"]
        assert (r > 128).any() and ((r >= 86) & (r <= 128)).any() and ((r > 0) & (r < 86)).any(), r
    for c in _tagged("road_clip40"):
        for st in _stats(c):
            assert st["clip_limit"] == 80 and (st["residual"] == 0).all() and (st["batch"] == 0).all()
    for c in _tagged("noise_clip2"):         # spread histograms: no batch, small residuals
        for st in _stats(c):
            assert (st["batch"] == 0).all() and (st["residual"] < 86).all() and (st["residual"] > 0).any()


# ---------------------------------------------------------------------------
# colour regimes
# ---------------------------------------------------------------------------
def test_lattice_holds_every_colour_and_saturates():
    lat = pc.lattice()
    assert lat.shape == (512, 512, 3)
    flat = lat.reshape(-1, 3).astype(np.int64)
    assert len(np.unique(flat[:, 0] << 16 | flat[:, 1] << 8 | flat[:, 2])) == 64 ** 3
    for corner in [(b, g, r) for b in (0, 255) for g in (0, 255) for r in (0, 255)]:
        assert (lat == corner).all(-1).any(), corner
    cr, cb = pc.unclamped_crcb(lat)
    assert cr.max() == 256 and (cr > 255).any() and cb.max() >= 255, (cr.max(), cb.max())
    assert cr.min() >= 0 and cb.min() >= 0
    # pure red is the pixel that does it
    assert pc.unclamped_crcb(np.array([[[0, 0, 255]]], np.uint8))[0][0, 0] == 256
    u = pc.unsaturated_bgr(lat, 8, 2.0)
    low, high = (u < 0).any(-1).mean(), (u > 255).any(-1).mean()
    print(f"lattice after CLAHE: {low:.3f} of the pixels below 0, {high:.3f} above 255")
    assert low >= 0.10 and high >= 0.10, (low, high)
    # every tile's histogram is mixed: all 8 x 8 tiles hold (nearly) every luma
    assert pc.stats_of(("lattice",), 512, 512, "YCrCb", 8, 2.0)["bins"].min() > 200


def test_blocks_carry_the_saturated_colours_through_a_median():
    """On the lattice a saturating pixel stands alone in its 3 x 3 window and
    a median behind the CLAHE filters it out; in `blocks` the four inner pixels
    of every 4 x 4 block come through the oracle's median as the CLAHE made
    them, the saturating ones included."""
    blk = pc.blocks()
    assert blk.shape == (256, 256, 3) and len(np.unique(blk.reshape(-1, 3), axis=0)) == 16 ** 3
    assert (blk.reshape(64, 4, 64, 4, 3) == blk[::4, ::4][:, None, :, None]).all()
    cr, _ = pc.unclamped_crcb(blk)
    red = (blk == (0, 0, 255)).all(-1)
    assert red.sum() == 16 and (cr[red] == 256).all() and (cr[~red] <= 255).all()
    yy, xx = np.mgrid[:256, :256]
    inner = np.isin(yy % 4, (1, 2)) & np.isin(xx % 4, (1, 2))
    for c in pc.cases().values():
        if c.frame != (("blocks",),) or c.entry != "clahe_median" or c.clip == 0.0:
            continue
        clahe = pc.ref(("blocks",), 256, 256, (("clahe", "YCrCb", c.tiles, c.clip),))
        same = (pc.oracle(c.name).proc[0] == clahe).all(-1)
        u = pc.unsaturated_bgr(blk, c.tiles, c.clip)
        low, high = (u < 0).any(-1), (u > 255).any(-1)
        assert low.mean() >= 0.10 and high.mean() >= 0.10, (c.name, low.mean(), high.mean())
        if c.k == 3:
            assert same[inner].mean() > 0.99 and same[inner & (low | high)].all(), c.name
            assert same[inner & red].all() and (inner & red).sum() == 4, c.name


# ---------------------------------------------------------------------------
# median regimes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", pc.KS)
def test_checker_windows_split_at_the_rank(k):
    H, W = 40, 50
    r = k // 2
    border = np.ones((H, W), bool)
    border[r:H - r, r:W - r] = False
    for spec in [("checker", a, b) for a, b in pc.CHECKERS] + [("checker3",)]:
        img = pc.make_frame(spec, H, W)
        assert pc.split_share(img, k) == 1.0, spec
        win = pc.interior_windows(img, k)
        centre = img[r:H - r, r:W - r]
        assert ((win == centre[..., None]).sum(-1) == (k * k + 1) // 2).all(), spec
        out = cpu.median(img, k)
        np.testing.assert_array_equal(out[r:H - r, r:W - r], centre)
        changed = (out != img).any(-1)
        share = changed[border].mean()
        print(f"{spec} k={k}: the oracle changes {share:.3f} of the border pixels")
        assert share > 0 and not changed[~border].any(), spec
    # full-range and two-level noise: (nearly) no window is such a split, every value is met
    assert pc.split_share(pc.make_frame(("noise", 22), H, W), k) < 0.01
    two = pc.make_frame(("two_level", 21), 70, 130)
    assert set(np.unique(two)) == {0, 255}
    if k == 3:   # p = 1/2: 2 C(9, 4) / 2^9 = 0.49 of the windows split 5 : 4
        assert 0.4 < pc.split_share(two, k) < 0.6


def test_median_oracle_is_scipy_on_every_case():
    seen = set()
    for c in pc.cases().values():
        if c.entry != "median":
            continue
        for s in c.frame:
            if (s, c.H, c.W, c.k) in seen:
                continue
            seen.add((s, c.H, c.W, c.k))
            img = pc.make_frame(s, c.H, c.W)
            want = scipy.ndimage.median_filter(img, size=(c.k, c.k, 1), mode="nearest")
            np.testing.assert_array_equal(pc.ref(s, c.H, c.W, (("median", c.k),)), want, err_msg=c.name)
    assert len(seen) >= 7 * len(pc.MEDIAN_SHAPES) * 4


def test_median_cases_behind_clahe_are_accepted():
    for c in pc.cases().values():
        if c.entry == "clahe_median":
            assert pc.clahe_median_fits(c.H, c.W, c.tiles, c.k), c.name
    # ... and the geometries left out of the table are the refused ones
    for H, W, t in [(32, 32, 8), (64, 128, 64), (3, 5, 8), (1, 1, 8)]:
        assert not pc.clahe_median_fits(H, W, t, 3)


# ---------------------------------------------------------------------------
# gray span and gate regimes
# ---------------------------------------------------------------------------
def test_planted_extremes():
    for c in _tagged("extremes"):
        for b, s in enumerate(c.frame):
            g = pc.gray_of(pc.make_frame(s, c.H, c.W))
            pmin, pmax = pc.extremes_at(s[2], c.H, c.W)
            assert (g == g.min()).sum() == 1 and (g == g.max()).sum() == 1, c.name
            assert np.unravel_index(g.argmin(), g.shape) == pmin, c.name
            assert np.unravel_index(g.argmax(), g.shape) == pmax, c.name
            assert (g.min(), g.max()) == (s[3], s[4]) and pc.oracle(c.name).span[b] == s[4] - s[3]
        assert len({s[2] for s in c.frame}) == 3
        assert pc.oracle(c.name).span.tolist() == [255, 253, 251]
    wheres = {(c.H, c.W): c for c in _tagged("extremes")}
    assert (37, 91) in wheres and 91 % 4 != 0           # the ragged right edge
    H, W = 300, 2000                                   # more than 64 blocks of work a frame
    assert H * ((W + 3) // 4) > 64 * 256 * 8
    assert all(pc.oracle(c.name).span.tolist() == [0, 0] for c in _tagged("span0"))
    assert all(pc.oracle(c.name).span.tolist() == [255] for c in _tagged("span255"))


def test_gated_batches_mix_processed_and_passed_frames():
    for c in pc.cases().values():
        if not c.gate:
            continue
        spans = [pc.span_of(pc.make_frame(s, c.H, c.W)) for s in c.frame]
        low = [float(v) < pc.GATE_THRESH for v in spans]
        assert low[0] and spans[0] == 0 and not any(low[1:]), (c.name, spans)
        ans = pc.oracle(c.name)
        for b, s in enumerate(c.frame):
            raw = pc.make_frame(s, c.H, c.W)
            assert (ans.proc[b] == raw).all() != low[b], c.name   # the chain changes a flat frame

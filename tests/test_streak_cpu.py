"""The rain-streak removal without a GPU: the properties of tests/streak_ref.py,
its efficacy on the oracle's own rain, the regime of every case of
streak_cases.py, the parameter normalisation, the chain descriptor (the
existing chains unmoved, kind 3 still refused), the host queries, and both
entries answering a bad argument before any HIP call.

Efficacy, measured on the reference (seeds 0..5 at 96 x 160 and 270 x 480,
rain_p 0.01 and 0.03, slant -1, max_len 0; PSNR to the rain-free frame):
derained 41.8 .. 55.8 dB, rainy 26.3 .. 36.2 dB, 3 x 3 median of the rainy
frame 30.0 .. 33.1 dB; the smallest gain is 14.4 dB over the rainy frame and
10.6 dB over its median, so the bars are 7.2 and 5.3 dB.  slant +1 gains at
most 1.6 dB over the rainy frame."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import streak_cases as C
from streak_ref import gray, offset, streak_ref
from oracle import cpu, fog_ref

DEFAULT = [("clahe", "YCrCb", 8, 2.0), ("median", 3)]
DCP = ("dcp", 15, 243, 26, 40, 65)
ST = ("streak", 3, 9, 0, -1, 20)
GAIN_RAINY, GAIN_MEDIAN = 14.4 / 2, 10.6 / 2  # half the smallest measured gains, dB


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    m = float((d * d).mean())
    return 99.0 if m == 0 else 10 * np.log10(255.0 * 255.0 / m)


# ---------------------------------------------------------------- properties

PROP = [("rain_default", (3, 9, 0, -1, 20)), ("thr_1", (5, 5, 0, 3, 1)),
        ("reject_long", (3, 9, 49, -1, 20)), ("noise_L3", (3, 3, 0, -1, 1)),
        ("sparse_L3_M5", (3, 3, 5, 3, 1)), ("slant_4", (3, 33, 97, 4, 20)),
        ("den_1", (3, 9, 0, -2, 20))]


@pytest.mark.parametrize("name,prm", PROP)
def test_output_never_exceeds_the_input(name, prm):
    img = C.frame(name)
    out, S, d = streak_ref(img, *prm, detail=True)
    assert (out <= img).all()
    assert (d["T0"] >= 0).all()
    assert np.array_equal(out[S == 0], img[S == 0])


def test_a_frame_under_the_threshold_is_unchanged():
    for name in ("rain_free", "flat_128", "flat_white", "thr_255_miss"):
        img = C.frame(name)
        p = C.params(name)
        out, S, d = C.reference(name)
        if name != "rain_free":      # rain_free: a few noise peaks pass thr, none is 9 long
            assert int(d["T0"].max()) < p[4]
        assert not S.any() and np.array_equal(out, img)
    img = C.road(60, 80, 3)
    thr = int(streak_ref(img, 3, 3, 0, 0, 1, detail=True)[2]["T0"].max()) + 1
    out, S = streak_ref(img, 3, 3, 0, 0, thr)
    assert thr > 1 and not S.any() and np.array_equal(out, img)


@pytest.mark.parametrize("name,prm", PROP)
def test_mirror_equivariance(name, prm):
    img = C.frame(name)
    w, L, M, slant, thr = prm
    out, S = streak_ref(img, *prm)
    fx = np.ascontiguousarray(img[:, ::-1])
    fy = np.ascontiguousarray(img[::-1])
    ox, Sx = streak_ref(fx, w, L, M, -slant, thr)
    oy, Sy = streak_ref(fy, w, L, M, -slant, thr)
    assert np.array_equal(ox, out[:, ::-1]) and np.array_equal(Sx, S[:, ::-1])
    assert np.array_equal(oy, out[::-1]) and np.array_equal(Sy, S[::-1])


def test_offsets_are_odd_in_j():
    for slant in range(-4, 5):
        for j in range(0, 49):
            assert offset(-j, slant) == -offset(j, slant)
            assert offset(j, -slant) == -offset(j, slant)
        assert abs(offset(48, slant)) == 12 * abs(slant)
    assert [offset(j, -1) for j in range(0, 8)] == [0, 0, -1, -1, -1, -1, -2, -2]


@pytest.mark.parametrize("slant", [-4, -1, 0, 1, 3])
@pytest.mark.parametrize("v", [0, 90, 200])
def test_exact_inversion_on_a_flat_gray_frame(slant, v):
    """On a flat frame of B = G = R = v a streak of the model reads s in every
    channel, its gray is s exactly ((16384 s + 8192) >> 14), so T = s - v and
    den = 255 - s; where S = T the recovery is s - (T den + (den >> 1)) / den
    = s - T = v with no rounding left.  S = T on every pixel of a streak at
    least min_len long that follows the op's own line: the erosion's line
    through any of its pixels stays within one column of it, which hmax_3
    covers, and the dilation restores the ends from the streak's own centre
    line."""
    H, W, L = 80, 90, 9
    clean = C.flat(H, W, v)
    img = clean
    spots = [(40, 45, 9), (20, 20, 15), (60, 70, 33), (0, 30, 17), (79, 60, 17), (40, 0, 21),
             (40, 89, 21), (30, 55, 120)]
    for i, (y, x, n) in enumerate(spots):
        img = C.add_streak(img, y, x, n, slant, 115 if i & 1 else 70)
    assert (img != clean).any()
    out, S = streak_ref(img, 3, L, 0, slant, 10)
    assert np.array_equal(S > 0, img[..., 0] != clean[..., 0])
    assert np.array_equal(out, clean)
    # a streak shorter than min_len stays
    short = C.add_streak(clean, 40, 45, L - 2, slant, 115)
    out, S = streak_ref(short, 3, L, 0, slant, 10)
    assert not S.any() and np.array_equal(out, short)


@pytest.mark.parametrize("slant", [-1, 0, 2])
def test_a_two_pixel_line_over_the_full_height(slant):
    H, W = 120, 100
    base = C.flat(H, W, 90)   # flat gray: the inversion is exact (see above)
    img = C.add_streak(base, H // 2, 50, 4 * H, slant, 150, width=2)
    line = (img != base).any(axis=2)
    assert line.sum(axis=1).min() == 2 and line.sum() == 2 * H
    out0, S0 = streak_ref(img, 5, 9, 0, slant, 20)
    assert np.array_equal(S0 > 0, line)
    assert np.array_equal(out0, base)                               # erased
    out1, S1 = streak_ref(img, 5, 9, 49, slant, 20)
    assert not S1.any() and np.array_equal(out1, img)               # untouched


# ------------------------------------------------------------------ efficacy

@functools.lru_cache(maxsize=None)
def _rain_set(H, W, seed):
    """(rain-free, {rain_p: rainy}) through the oracle's generator."""
    base = C.road(H, W, seed)
    prm = fog_ref.draw(np.random.RandomState(seed), H, W, level="light", rain=True)
    return tuple(fog_ref.fog_frame(base, prm, rain_p=rp) for rp in (0.0, 0.01, 0.03))


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("shape", [(96, 160), (270, 480)])
def test_efficacy_on_the_oracles_rain(shape, seed):
    clean, r1, r3 = _rain_set(*shape, seed)
    out, S = streak_ref(clean, 3, 9, 0, -1, 20)
    assert np.array_equal(out, clean) and not S.any()    # rain_p 0: byte-identical
    for rainy in (r1, r3):
        assert (rainy != clean).any()
        good = psnr(streak_ref(rainy, 3, 9, 0, -1, 20)[0], clean)
        wrong = psnr(streak_ref(rainy, 3, 9, 0, 1, 20)[0], clean)
        p_rain, p_med = psnr(rainy, clean), psnr(cpu.median(rainy, 3), clean)
        print(f"{shape} seed {seed}: rainy {p_rain:.2f} median {p_med:.2f} "
              f"slant -1 {good:.2f} slant +1 {wrong:.2f} dB")
        assert good > p_rain + GAIN_RAINY
        assert good > p_med + GAIN_MEDIAN
        assert wrong < good


# ------------------------------------------------------------ named regimes

def test_cases_cover_the_parameter_ranges():
    ps = [C.params(n) for n in C.CASES]
    assert {3, 15} <= {p[0] for p in ps}
    assert {3, 33} <= {p[1] for p in ps}
    assert {0, 5, 97} <= {p[2] for p in ps}
    assert set(range(-4, 5)) <= {p[3] for p in ps}
    assert {1, 255} <= {p[4] for p in ps}
    for s in (-4, -1, 0, 1, 4):
        assert C.params(f"slant_{s}") == (3, 33, 97, s, 20)
    shapes = {C.frame(n).shape[:2] for n in C.CASES}
    assert {(1, 1), (1, 40), (40, 1), (3, 5), (16, 16), (63, 63), (64, 64), (65, 65),
            (9, 255), (9, 256), (9, 257), (3, 1023), (3, 1024), (3, 1025)} <= shapes


def test_each_case_meets_its_regime():
    S = {n: C.reference(n)[1] for n in C.CASES}
    R = {n: C.reference(n)[2]["R"] for n in C.CASES}
    for n in C.CASES:
        out, s, d = C.reference(n)
        assert out.dtype == np.uint8 and out.shape == C.frame(n).shape and s.shape == out.shape[:2]
    # dense and sparse responses
    for n in ("noise_L3", "noise_w15", "seg_9x255", "seg_9x256", "seg_9x257", "seg_5x530",
              "seg_3x1023", "seg_3x1024", "seg_3x1025"):
        assert (S[n] > 0).mean() > 0.2, n
    # frames smaller than the windows still answer (clipped windows)
    for n in ("size_1x40", "size_3x5_M0", "size_16x16_M0", "size_20x90"):
        assert S[n].any(), n
    for n in ("size_3x5", "size_16x16", "size_20x90_M"):
        assert not S[n].any() and (R[n] > 0).any(), n
    # max_len cases: some streaks rejected, some kept
    for n in ("sparse_L3_M5", "sparse_L5_M9", "tail_66x67", "reject_long", "slant_-4", "slant_-1",
              "slant_0", "slant_1", "slant_4", "slant_3_noise", "slant_-3", "tile_64x64",
              "tile_65x65", "tile_129x127"):
        p = C.params(n)
        s0 = streak_ref(C.frame(n), p[0], p[1], 0, p[3], p[4])[1]
        assert S[n].any() and ((s0 > 0) & (S[n] == 0)).any(), n
        assert (R[n] > 0).any() and (R[n] == 0).any(), n
    # thresholds: 255 passes only g = 255 over a black ground
    assert S["thr_255"].any() and set(np.unique(S["thr_255"])) == {0, 255}
    assert not S["thr_255_miss"].any()
    assert C.reference("thr_1")[2]["T"][C.reference("thr_1")[2]["T"] > 0].min() == 1
    # den = 1 where g = 255, also on a pixel that is not white
    for n in ("den_1", "batch_saturated", "thr_255"):
        img, g = C.frame(n), gray(C.frame(n))
        hit = (g == 255) & (S[n] > 0)
        assert hit.any() and (hit & (img[..., 0] == 251)).any(), n
        assert (C.reference(n)[0][hit & (img[..., 0] == 251)][:, 0] == 0).all()  # clamps at 0
    # width: 3-pixel streaks pass width 15 and not width 3
    assert (S["w15_wide_streaks"] > 0).sum() > 2 * (S["w3_wide_streaks"] > 0).sum() > 0
    # streaks across the tile edges and at the four borders
    for s in (-4, -1, 0, 1, 4):
        t = C.reference(f"slant_{s}")[2]["T"] > 0
        assert t[0].any() and t[-1].any() and t[:, 0].any() and t[:, -1].any()
        assert t[63:66, 60:69].any() and t[120:130, 118:130].any()
    t = C.reference("seg_40x270")[2]["T"] > 0
    assert t[:, 255].any() and t[:, 256].any()
    s = C.reference("seg_12x1040")[1] > 0
    assert s[:, 1022].any() and s[:, 1024].any() and s[:, 1026].any()


# ------------------------------------------------- parameters and descriptor

def test_parameter_normalisation():
    from rvs_amd.preprocess.ops import streak_params
    assert streak_params({}) == (3, 9, 0, 0, 20)
    assert streak_params({"width": 4})[0] == 5 and streak_params({"width": 0})[0] == 3
    assert streak_params({"width": 99})[0] == 15 and streak_params({"width": 16})[0] == 15
    assert streak_params({"min_len": 10})[1] == 11 and streak_params({"min_len": 1})[1] == 3
    assert streak_params({"min_len": 34})[1] == 33 and streak_params({"min_len": 200})[1] == 33
    assert streak_params({"max_len": 0})[2] == 0 and streak_params({"max_len": -5})[2] == 0
    assert streak_params({"max_len": 48})[2] == 49 and streak_params({"max_len": 500})[2] == 97
    assert streak_params({"max_len": 5})[2] == 11          # above min_len 9
    assert streak_params({"min_len": 33, "max_len": 33})[2] == 35
    assert streak_params({"slant": -9})[3] == -4 and streak_params({"slant": 7})[3] == 4
    assert streak_params({"slant": -1})[3] == -1
    assert streak_params({"thresh": 0})[4] == 1 and streak_params({"thresh": 999})[4] == 255


def test_registry_names():
    from rvs_amd.preprocess import ops, registry
    for name in ("StreakDerain", "HIPStreakDerain"):
        assert registry.get_op_class(name) is ops.StreakDerain
    assert ops.HIPStreakDerain is ops.StreakDerain
    op = ops.StreakDerain(width=6, min_len=12, max_len=48, slant=-1, thresh=15)
    assert (op.width, op.min_len, op.max_len, op.slant, op.thr) == (7, 13, 49, -1, 15)
    for word in ("max_len", "slant", "dB"):
        assert word in ops.StreakDerain.__doc__


def test_descriptor_bytes():
    from rvs_amd import kernels as K
    d = bytes(K.chain_desc([("streak", 5, 11, 49, -1, 17), ("median", 5)], True, True, 12.5))
    assert len(d) == K.CHAIN_DESC_BYTES == 120
    assert struct.unpack_from("<iiiid", d, 0) == (1, 2, 1, 0, 12.5)
    # {kind, thr, min_len, width} then {max_len, slant} in the bytes of clip
    assert struct.unpack_from("<iiiiii", d, 24) == (4, 17, 11, 5, 49, -1)
    assert struct.unpack_from("<iiiid", d, 48) == (1, 0, 0, 5, 0.0)
    # the existing chains keep every byte
    want = struct.pack("<iiiid", 1, 2, 0, 0, 20.0) + struct.pack("<iiiid", 0, 0, 8, 0, 2.0) + \
        struct.pack("<iiiid", 1, 0, 0, 3, 0.0) + struct.pack("<iiiid", 1, 0, 0, 0, 0.0) * 2
    assert bytes(K.chain_desc(DEFAULT)) == want
    lab = bytes(K.chain_desc([("clahe", "LAB", 4, 3.5)], False, True, 7.0))
    assert lab == struct.pack("<iiiid", 0, 1, 1, 0, 7.0) + struct.pack("<iiiid", 0, 1, 4, 0, 3.5) + \
        struct.pack("<iiiid", 1, 0, 0, 0, 0.0) * 3
    dcp = bytes(K.chain_desc([DCP]))
    assert struct.unpack_from("<iiiiii", dcp, 24) == (2, 26, 40, 15, 243, 65)


def _pipe(chain, **kw):
    from rvs_amd.preprocess import PreprocessPipeline
    cfg = {"enabled": True, "chain": chain}
    cfg.update(kw)
    return PreprocessPipeline(cfg)


def test_pipeline_maps_the_op_into_the_descriptor():
    from rvs_amd import kernels as K
    p = _pipe([{"name": "StreakDerain", "params": {"width": 4, "min_len": 12, "max_len": 48,
                                                  "slant": -1, "thresh": 17}},
               {"name": "CLAHEDehaze", "params": {}}, {"name": "MedianDerain", "params": {}}])
    assert p.chain_supported and p.unsupported_op is None and not p._fused
    d = bytes(p.chain_desc)
    assert struct.unpack_from("<iiiiii", d, 24) == (4, 17, 13, 5, 49, -1)
    assert p.chain_route(1080, 1920, K.letterbox_geometry(1080, 1920)) == K.ROUTE_OPS
    two = _pipe([{"name": "StreakDerain", "params": {"slant": -1}},
                 {"name": "HIPStreakDerain", "params": {"slant": 1}}])
    assert two.chain_supported
    d = bytes(two.chain_desc)
    assert struct.unpack_from("<i", d, 24 + 20)[0] == -1 and struct.unpack_from("<i", d, 48 + 20)[0] == 1
    five = _pipe([{"name": "StreakDerain", "params": {}}] * 5)
    assert not five.chain_supported
    # the default configuration does not hold the op
    from rvs_amd.config import load_config
    names = [n["name"] for n in load_config()["preprocess"]["chain"]]
    assert names == ["CLAHEDehaze", "MedianDerain"]


def test_routes_and_workspaces():
    from rvs_amd import kernels as K
    geo = K.letterbox_geometry(360, 640)
    big = ("streak", 3, 33, 97, 4, 20)
    chains = [[ST], [ST, ("median", 3)], [("clahe", "YCrCb", 8, 2.0), ST], DEFAULT + [ST],
              [ST] + DEFAULT, [ST, big], [DCP, ST], [ST] * 4]
    for ops in chains:
        for gate in (False, True):
            d = K.chain_desc(ops, gate_on=gate)
            assert K.preprocess_chain_route(d, 360, 640, geo) == K.ROUTE_OPS, ops
            assert K.preprocess_chain_route(d, 360, 640) == K.ROUTE_OPS, ops
            sizes = [K.preprocess_chain_ws_bytes(d, B, 90, 130) for B in (1, 2, 3, 8)]
            assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4, ops
    for m in (0, 11, 97):
        sizes = [K.streak_ws_bytes(B, 90, 130, m) for B in (1, 2, 3, 8)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4
        assert K.preprocess_chain_ws_bytes(K.chain_desc([("streak", 3, 9, m, 0, 20)]), 3, 90, 130) \
            >= K.streak_ws_bytes(3, 90, 130, m)
    # two planes of pitch-16 rows, four with max_len
    assert K.streak_ws_bytes(1, 90, 130, 0) >= 2 * 90 * 144
    assert K.streak_ws_bytes(2, 90, 130, 49) == 2 * K.streak_ws_bytes(2, 90, 130, 0)
    # a chain of two streak ops takes the larger one's region once
    one = K.preprocess_chain_ws_bytes(K.chain_desc([big]), 3, 90, 130)
    two = K.preprocess_chain_ws_bytes(K.chain_desc([ST, big]), 3, 90, 130)
    assert two - one == (3 * 90 * 390 + 255) // 256 * 256     # the scratch batch only
    # with a DCP op both regions are there
    both = K.preprocess_chain_ws_bytes(K.chain_desc([DCP, ST]), 3, 90, 130)
    assert both >= K.dcp_ws_bytes(3, 90, 130, 40) + K.streak_ws_bytes(3, 90, 130, 0) + 3 * 90 * 390
    # the existing chains' workspaces do not move
    assert K.preprocess_chain_ws_bytes(K.chain_desc(DEFAULT), 3, 130, 257) == K.clahe_ws_bytes(3, 8)
    assert K.preprocess_chain_ws_bytes(K.chain_desc([DCP]), 3, 90, 130) == \
        (K.dcp_ws_bytes(3, 90, 130, 40) + 255) // 256 * 256
    # bad shapes
    assert K.streak_ws_bytes(0, 90, 130, 0) == 0 and K.streak_ws_bytes(1, 90, 130, 98) == 0
    assert K.streak_ws_bytes(1, 0, 130, 0) == 0 and K.streak_ws_bytes(1, 90, 130, -1) == 0


def _streak(lib, in_=4096, out=1 << 20, B=2, H=64, W=64, pitch=None, width=3, min_len=9,
            max_len=0, slant=0, thr=20, ws=1 << 24, ws_bytes=1 << 30, s=None):
    return lib.rv_streak_derain_u8(in_, out, B, H, W, 3 * W if pitch is None else pitch, width,
                                   min_len, max_len, slant, thr, ws, ws_bytes, s, None)


def test_op_argument_errors_touch_no_device():
    """RV_EINVAL (-1000) with a message before any HIP call: the pointers are
    made-up integers."""
    from rvs_amd import _lib as L, kernels as K
    lib = L.load()
    assert lib.rv_abi_version() >= 14
    bad = [(dict(width=4), b"width"), (dict(width=1), b"width"), (dict(width=17), b"width"),
           (dict(min_len=1), b"min_len"), (dict(min_len=10), b"min_len"),
           (dict(min_len=35), b"min_len"), (dict(max_len=9), b"max_len"),
           (dict(max_len=7), b"max_len"), (dict(max_len=12), b"max_len"),
           (dict(max_len=99), b"max_len"), (dict(max_len=-1), b"max_len"),
           (dict(slant=5), b"slant"), (dict(slant=-5), b"slant"),
           (dict(thr=0), b"thr"), (dict(thr=256), b"thr"),
           (dict(pitch=3 * 64 - 1), b"pitch"), (dict(out=4096), b"alias"),
           (dict(in_=None), b"null"), (dict(out=None), b"null"),
           (dict(H=0), b"shape"), (dict(W=-1), b"shape"), (dict(B=-1), b"shape"),
           (dict(B=65536), b"shape"), (dict(ws=None), b"workspace"),
           (dict(ws=(1 << 24) + 8), b"aligned")]
    for kw, word in bad:
        assert _streak(lib, **kw) == -1000, kw
        assert word in lib.rv_last_error(), (kw, lib.rv_last_error())
    for m in (0, 49):
        need = K.streak_ws_bytes(2, 64, 64, m)
        assert need > 0
        assert _streak(lib, max_len=m, ws_bytes=need - 1) == -1000       # one byte short
        assert b"workspace" in lib.rv_last_error()
        # a well-formed call on an empty batch returns RV_OK without launching
        assert _streak(lib, max_len=m, B=0, ws_bytes=need) == 0
    assert _streak(lib, B=0, ws=None, ws_bytes=0) == 0


def test_chain_argument_errors_touch_no_device():
    from rvs_amd import _lib as L, kernels as K
    lib = L.load()
    geo = K.letterbox_geometry(64, 64)

    def call(desc, ws_bytes=1 << 30, in_=4096, out=1 << 20, ws=1 << 24, B=2, H=64, W=64,
             pitch=None):
        return lib.rv_preprocess_chain_u8(in_, out, B, H, W, 3 * W if pitch is None else pitch,
                                          desc, ws, ws_bytes, 1 << 22, L.int_array(geo), None)

    bad = [(("streak", 4, 9, 0, 0, 20), b"width"), (("streak", 3, 35, 0, 0, 20), b"min_len"),
           (("streak", 3, 9, 9, 0, 20), b"max_len"), (("streak", 3, 9, 99, 0, 20), b"max_len"),
           (("streak", 3, 9, 0, 5, 20), b"slant"), (("streak", 3, 9, 0, 0, 0), b"thr"),
           (("streak", 3, 9, 0, 0, 256), b"thr")]
    for op, word in bad:
        for ops in ([op], [("median", 3), op]):
            desc = K.chain_desc(ops)
            assert call(desc) == -1000, op
            assert word in lib.rv_last_error(), (op, lib.rv_last_error())
            assert b"streak" in lib.rv_last_error()
            assert lib.rv_preprocess_chain_route(desc, 64, 64, L.int_array(geo)) == -1000
            assert lib.rv_preprocess_chain_ws_bytes(desc, 2, 64, 64, 192) == 0
    ok = K.chain_desc([ST, ("median", 3)])
    need = K.preprocess_chain_ws_bytes(ok, 2, 64, 64)
    assert need > K.streak_ws_bytes(2, 64, 64, 0)
    assert call(ok, ws_bytes=need - 1) == -1000
    assert b"workspace" in lib.rv_last_error()
    assert call(ok, pitch=3 * 64 - 1) == -1000
    assert b"pitch" in lib.rv_last_error()
    assert call(ok, out=4096) == -1000                  # in == out
    assert call(ok, out=None) == -1000
    assert call(ok, ws_bytes=need, B=0) == 0
    # kind 3 is still nobody's
    raw = bytearray(bytes(K.chain_desc([ST])))
    struct.pack_into("<i", raw, 24, 3)
    unknown = (ctypes.c_uint8 * 120).from_buffer_copy(bytes(raw))
    assert call(unknown) == -1000 and b"unknown kind 3" in lib.rv_last_error()
    struct.pack_into("<i", raw, 24, 5)
    unknown = (ctypes.c_uint8 * 120).from_buffer_copy(bytes(raw))
    assert call(unknown) == -1000 and b"unknown kind 5" in lib.rv_last_error()

"""The dark-channel dehaze without a GPU: every case of dcp_cases.py is in the
regime it is named for (on tests/dcp_ref.py alone), the parameters normalise
as documented, the chain descriptor carries the op without moving a byte of
the existing chains, the host queries know it, and both entries answer a bad
argument before any HIP call."""
import struct

import numpy as np
import pytest

import dcp_cases as C

DEFAULT = [("clahe", "YCrCb", 8, 2.0), ("median", 3)]
DCP = ("dcp", 15, 243, 26, 40, 65)


def test_quantile_cases_pick_the_named_level():
    air = C.reference("quantile_exact")[2]
    assert (air[3], air[4]) == (255, 10)
    air = C.reference("quantile_ties")[2]
    assert air[3] == 254 and air[4] > 10
    d = C.reference("quantile_ties")[3]["d"]
    assert int((d == 255).sum()) == 9
    for name, v in (("flat_black", 0), ("flat_white", 255), ("flat_128", 128)):
        out, t, air, _ = C.reference(name)
        assert air[4] == 20 * 24 and air[3] == v
        assert list(air[:3]) == [max(1, v)] * 3  # A clamps to 1 on black


def test_gcheck_needs_more_than_a_double():
    num = C.reference("gcheck")[3]["num"]
    assert int(np.abs(num).max()) << 14 > 1 << 53
    assert int(np.abs(num).max()) << 14 < 1 << 62


def test_halves_exercises_the_t_min_clamp():
    p = C.params("halves")
    t = C.reference("halves")[3]["t"]
    share = float(np.mean(t < p[2]))
    assert 0.45 < share < 0.55, share


def test_regimes_across_the_set():
    aq_neg = aq_pos = d_neg = d_pos = t_out = False
    for name in C.CASES:
        out, t, air, info = C.reference(name)
        assert out.dtype == np.uint8 and out.shape == C.frame(name).shape
        if "aq" in info:
            aq_neg |= bool((info["aq"] < 0).any())
            aq_pos |= bool((info["aq"] > 0).any())
            assert int(np.abs(info["aq"]).max()) < 1 << 20       # 63.75 * 2^14
            assert int(np.abs(info["bq"]).max()) < 1 << 31
            t_out |= bool(((info["t_raw"] < 0) | (info["t_raw"] > 255)).any())
        d_neg |= bool((info["diff"] < 0).any())
        d_pos |= bool((info["diff"] > 0).any())
    assert aq_neg and aq_pos and d_neg and d_pos and t_out


def test_cases_cover_the_parameter_ranges():
    ps = [C.params(n) for n in C.CASES]
    assert {3, 15, 31} <= {p[0] for p in ps}
    assert {1, 256} <= {p[1] for p in ps}
    assert {0, 1, 8, 40, 64} <= {p[3] for p in ps}
    assert {1, 1 << 20} <= {p[4] for p in ps}
    shapes = {C.frame(n).shape[:2] for n in C.CASES}
    assert {(1, 1), (1, 40), (40, 1), (3, 5), (16, 16)} <= shapes


def test_hazy_error_to_the_clear_scene_falls():
    clear = C.scene(120, 200, 1).astype(np.int64)
    before = np.abs(C.frame("hazy").astype(np.int64) - clear).mean()
    after = np.abs(C.reference("hazy")[0].astype(np.int64) - clear).mean()
    assert after < 0.5 * before, (before, after)


def test_parameter_normalisation():
    from rvs_amd.preprocess.ops import dcp_params
    assert dcp_params({}) == (15, 243, 26, 40, 65)
    assert dcp_params({"patch": 4})[0] == 5 and dcp_params({"patch": 14})[0] == 15
    assert dcp_params({"patch": 1})[0] == 3 and dcp_params({"patch": 0})[0] == 3
    assert dcp_params({"patch": 99})[0] == 31 and dcp_params({"patch": 32})[0] == 31
    assert dcp_params({"omega": 0.0})[1] == 1 and dcp_params({"omega": 7.0})[1] == 256
    assert dcp_params({"omega": 1.0})[1] == 256 and dcp_params({"omega": 0.5})[1] == 128
    assert dcp_params({"t_min": 0.0})[2] == 1 and dcp_params({"t_min": 3.0})[2] == 255
    assert dcp_params({"t_min": 0.2})[2] == 51
    assert dcp_params({"refine_radius": -3})[3] == 0 and dcp_params({"refine_radius": 65})[3] == 64
    assert dcp_params({"eps": 0.0})[4] == 1 and dcp_params({"eps": 1e9})[4] == 1 << 20
    assert dcp_params({"eps": 0.01})[4] == 650


def test_registry_names():
    from rvs_amd.preprocess import ops, registry
    for name in ("DarkChannelDehaze", "DCPDehaze", "HIPDarkChannelDehaze"):
        assert registry.get_op_class(name) is ops.DarkChannelDehaze
    op = ops.DarkChannelDehaze(patch=8, refine_radius=100)
    assert (op.patch, op.wq, op.tq, op.radius, op.eq) == (9, 243, 26, 64, 65)


def test_descriptor_bytes():
    from rvs_amd import kernels as K
    d = bytes(K.chain_desc([DCP, ("median", 5)], True, True, 12.5))
    assert len(d) == K.CHAIN_DESC_BYTES == 120
    assert struct.unpack_from("<iiiid", d, 0) == (1, 2, 1, 0, 12.5)
    # {kind, tq, radius, patch} then {wq, eq} in the bytes of clip
    assert struct.unpack_from("<iiiiii", d, 24) == (2, 26, 40, 15, 243, 65)
    assert struct.unpack_from("<iiiid", d, 48) == (1, 0, 0, 5, 0.0)
    # the existing chains keep every byte
    want = struct.pack("<iiiid", 1, 2, 0, 0, 20.0) + struct.pack("<iiiid", 0, 0, 8, 0, 2.0) + \
        struct.pack("<iiiid", 1, 0, 0, 3, 0.0) + struct.pack("<iiiid", 1, 0, 0, 0, 0.0) * 2
    assert bytes(K.chain_desc(DEFAULT)) == want
    lab = bytes(K.chain_desc([("clahe", "LAB", 4, 3.5)], False, True, 7.0))
    assert lab == struct.pack("<iiiid", 0, 1, 1, 0, 7.0) + struct.pack("<iiiid", 0, 1, 4, 0, 3.5) + \
        struct.pack("<iiiid", 1, 0, 0, 0, 0.0) * 3


def _pipe(chain, **kw):
    from rvs_amd.preprocess import PreprocessPipeline
    cfg = {"enabled": True, "chain": chain}
    cfg.update(kw)
    return PreprocessPipeline(cfg)


def test_pipeline_maps_the_op_into_the_descriptor():
    from rvs_amd import kernels as K
    p = _pipe([{"name": "DarkChannelDehaze", "params": {"patch": 6, "omega": 0.5, "t_min": 0.2,
                                                       "refine_radius": 9, "eps": 0.01}},
               {"name": "MedianDerain", "params": {}}])
    assert p.chain_supported and p.unsupported_op is None and not p._fused
    d = bytes(p.chain_desc)
    assert struct.unpack_from("<iiiiii", d, 24) == (2, 51, 9, 7, 128, 650)
    assert p.chain_route(1080, 1920, K.letterbox_geometry(1080, 1920)) == K.ROUTE_OPS
    four = _pipe([{"name": "DCPDehaze", "params": {}}] * 4)
    assert four.chain_supported
    five = _pipe([{"name": "HIPDarkChannelDehaze", "params": {}}] * 5)
    assert not five.chain_supported
    # the default configuration does not hold the op
    from rvs_amd.config import load_config
    names = [n["name"] for n in load_config()["preprocess"]["chain"]]
    assert names == ["CLAHEDehaze", "MedianDerain"]


def test_routes_and_workspaces():
    from rvs_amd import kernels as K
    geo = K.letterbox_geometry(360, 640)
    chains = [[DCP], [DCP, ("median", 3)], [("clahe", "YCrCb", 8, 2.0), DCP],
              DEFAULT + [DCP], [DCP] + DEFAULT, [DCP] * 4]
    for ops in chains:
        for gate in (False, True):
            d = K.chain_desc(ops, gate_on=gate)
            assert K.preprocess_chain_route(d, 360, 640, geo) == K.ROUTE_OPS, ops
            assert K.preprocess_chain_route(d, 360, 640) == K.ROUTE_OPS, ops
            sizes = [K.preprocess_chain_ws_bytes(d, B, 90, 130) for B in (1, 2, 3, 8)]
            assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4, ops
    for r in (0, 1, 40, 64):
        sizes = [K.dcp_ws_bytes(B, 90, 130, r) for B in (1, 2, 3, 8)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4
        assert K.preprocess_chain_ws_bytes(K.chain_desc([("dcp", 15, 243, 26, r, 65)]), 3, 90, 130) \
            >= K.dcp_ws_bytes(3, 90, 130, r)
    assert K.dcp_ws_bytes(2, 90, 130, 40) > K.dcp_ws_bytes(2, 90, 130, 0)
    # the default chains' workspaces do not move
    assert K.preprocess_chain_ws_bytes(K.chain_desc(DEFAULT), 3, 130, 257) == K.clahe_ws_bytes(3, 8)
    # bad shapes and frames of more than 2^24 pixels
    assert K.dcp_ws_bytes(0, 90, 130, 40) == 0 and K.dcp_ws_bytes(1, 90, 130, 65) == 0
    assert K.dcp_ws_bytes(1, 4097, 4096, 40) == 0 and K.dcp_ws_bytes(1, 4096, 4096, 0) > 0
    assert K.preprocess_chain_ws_bytes(K.chain_desc([DCP]), 1, 4097, 4096) == 0


def _dcp(lib, in_=4096, out=1 << 20, B=2, H=64, W=64, pitch=None, patch=15, wq=243, tq=26,
         radius=40, eq=65, ws=1 << 24, ws_bytes=1 << 30, air=None, t=None):
    return lib.rv_dcp_dehaze_u8(in_, out, B, H, W, 3 * W if pitch is None else pitch, patch, wq,
                                tq, radius, eq, ws, ws_bytes, air, t, None)


def test_op_argument_errors_touch_no_device():
    """RV_EINVAL (-1000) with a message before any HIP call: the pointers are
    made-up integers."""
    from rvs_amd import _lib as L, kernels as K
    lib = L.load()
    assert lib.rv_abi_version() >= 12
    bad = [(dict(patch=4), b"patch"), (dict(patch=1), b"patch"), (dict(patch=33), b"patch"),
           (dict(radius=65), b"radius"), (dict(radius=-1), b"radius"),
           (dict(wq=0), b"wq"), (dict(wq=257), b"wq"), (dict(tq=0), b"tq"), (dict(tq=256), b"tq"),
           (dict(eq=0), b"eq"), (dict(eq=(1 << 20) + 1), b"eq"),
           (dict(pitch=3 * 64 - 1), b"pitch"), (dict(out=4096), b"alias"),
           (dict(in_=None), b"null"), (dict(out=None), b"null"),
           (dict(H=0), b"shape"), (dict(W=-1), b"shape"), (dict(B=-1), b"shape"),
           (dict(H=4097, W=4096), b"2^24"), (dict(ws=None), b"workspace"),
           (dict(ws=(1 << 24) + 8), b"aligned")]
    for kw, word in bad:
        assert _dcp(lib, **kw) == -1000, kw
        assert word in lib.rv_last_error(), (kw, lib.rv_last_error())
    need = K.dcp_ws_bytes(2, 64, 64, 40)
    assert need > 0
    assert _dcp(lib, ws_bytes=need - 1) == -1000       # one byte short
    assert b"workspace" in lib.rv_last_error()
    # a well-formed call on an empty batch returns RV_OK without launching
    assert _dcp(lib, B=0, ws_bytes=need) == 0
    assert _dcp(lib, B=0, ws=None, ws_bytes=0) == 0


def test_chain_argument_errors_touch_no_device():
    from rvs_amd import _lib as L, kernels as K
    lib = L.load()
    geo = K.letterbox_geometry(64, 64)

    def call(desc, ws_bytes=1 << 30, in_=4096, out=1 << 20, ws=1 << 24, B=2, H=64, W=64,
             pitch=None):
        return lib.rv_preprocess_chain_u8(in_, out, B, H, W, 3 * W if pitch is None else pitch,
                                          desc, ws, ws_bytes, 1 << 22, L.int_array(geo), None)

    bad = [(("dcp", 4, 243, 26, 40, 65), b"patch"), (("dcp", 15, 243, 26, 65, 65), b"radius"),
           (("dcp", 15, 0, 26, 40, 65), b"wq"), (("dcp", 15, 243, 0, 40, 65), b"tq"),
           (("dcp", 15, 243, 26, 40, 0), b"eq"), (("dcp", 15, 243, 26, 40, (1 << 20) + 1), b"eq")]
    for op, word in bad:
        for ops in ([op], [("median", 3), op]):
            desc = K.chain_desc(ops)
            assert call(desc) == -1000, op
            assert word in lib.rv_last_error(), (op, lib.rv_last_error())
            assert lib.rv_preprocess_chain_route(desc, 64, 64, L.int_array(geo)) == -1000
            assert lib.rv_preprocess_chain_ws_bytes(desc, 2, 64, 64, 192) == 0
    ok = K.chain_desc([DCP, ("median", 3)])
    need = K.preprocess_chain_ws_bytes(ok, 2, 64, 64)
    assert need > K.dcp_ws_bytes(2, 64, 64, 40)
    assert call(ok, ws_bytes=need - 1) == -1000
    assert b"workspace" in lib.rv_last_error()
    assert call(ok, pitch=3 * 64 - 1) == -1000
    assert b"pitch" in lib.rv_last_error()
    assert call(ok, out=4096) == -1000                  # in == out
    assert call(ok, out=None) == -1000
    big_geo = K.letterbox_geometry(4097, 4096)
    assert lib.rv_preprocess_chain_u8(4096, 1 << 20, 1, 4097, 4096, 3 * 4096, ok, 1 << 24,
                                      1 << 40, 1 << 22, L.int_array(big_geo), None) == -1000
    assert b"2^24" in lib.rv_last_error()
    assert call(ok, ws_bytes=need, B=0) == 0
    # a kind nobody defines is still refused
    raw = bytearray(bytes(K.chain_desc([DCP])))
    struct.pack_into("<i", raw, 24, 3)
    import ctypes
    unknown = (ctypes.c_uint8 * 120).from_buffer_copy(bytes(raw))
    assert call(unknown) == -1000 and b"unknown kind" in lib.rv_last_error()

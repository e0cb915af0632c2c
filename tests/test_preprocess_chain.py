"""rv_preprocess_chain_u8 without a GPU: the header declares the entry and
its two host queries, the route query picks the fused forms exactly where
they apply, argument errors are answered before any HIP call, and
PreprocessPipeline builds the descriptor with the reference's parameter
normalisation (clahe_dehaze.py:14-17, median_derain.py:11-13)."""
import os
import re
import struct

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "rvhip.h")
DEFAULT = [("clahe", "YCrCb", 8, 2.0), ("median", 3)]


def _lib():
    from rvs_amd import _lib as L
    return L, L.load()


def test_header_declares_chain_entries():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("rv_preprocess_chain_u8", "rv_preprocess_chain_ws_bytes",
                 "rv_preprocess_chain_route"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
    L, lib = _lib()
    for name in ("rv_preprocess_chain_u8", "rv_preprocess_chain_ws_bytes",
                 "rv_preprocess_chain_route"):
        assert hasattr(lib, name) and name in L._SIGS
    from rvs_amd import kernels, schedule
    m = re.search(r"#define RV_CHAIN_DESC_BYTES (\d+)", txt)
    assert int(m.group(1)) == kernels.CHAIN_DESC_BYTES == len(bytes(kernels.chain_desc(DEFAULT)))
    op, si, host = schedule._OPS["rv_preprocess_chain_u8"]
    assert host == {6: kernels.CHAIN_DESC_BYTES, 10: 24}  # descriptor and geo go by value
    assert "rv_preprocess_chain_u8" in L._RECORDABLE


def test_descriptor_layout():
    from rvs_amd import kernels
    d = bytes(kernels.chain_desc([("clahe", "lab", 4, 3.5), ("median", 7)], True, True, 20.5))
    assert struct.unpack_from("<iiiid", d, 0) == (1, 2, 1, 0, 20.5)
    assert struct.unpack_from("<iiiid", d, 24) == (0, 1, 4, 0, 3.5)
    assert struct.unpack_from("<iiiid", d, 48) == (1, 0, 0, 7, 0.0)


def test_routes():
    from rvs_amd import kernels
    K = kernels
    geo = K.letterbox_geometry(1080, 1920)
    route = K.preprocess_chain_route
    assert route(K.chain_desc(DEFAULT), 1080, 1920, geo) == K.ROUTE_FUSED
    assert route(K.chain_desc(DEFAULT, gate_on=True), 1080, 1920, geo) == K.ROUTE_FUSED_GATED
    # without a letterbox the same chains still take the single pass
    assert route(K.chain_desc(DEFAULT), 1080, 1920) == K.ROUTE_FUSED
    assert route(K.chain_desc(DEFAULT, gate_on=True), 1080, 1920) == K.ROUTE_FUSED_GATED
    for gate in (False, True):
        for ops, enabled in [([("clahe", "YCrCb", 8, 2.0), ("median", 5)], True),
                             ([("clahe", "LAB", 8, 2.0), ("median", 3)], True),
                             (DEFAULT, False),
                             ([], True),
                             ([("median", 3)], True),
                             ([("clahe", "YCrCb", 8, 2.0)], True),
                             ([("median", 3), ("clahe", "YCrCb", 8, 2.0)], True),
                             (DEFAULT + DEFAULT, True)]:
            d = K.chain_desc(ops, enabled=enabled, gate_on=gate)
            assert route(d, 1080, 1920, geo) == K.ROUTE_OPS, (ops, enabled, gate)
    # (37, 91): the letterbox upscales, which the fused pass does not emit
    g2 = K.letterbox_geometry(37, 91)
    assert g2[2] > 37 and g2[3] > 91
    assert not K.clahe_median_letterbox_fits(37, 91, 8, 3, g2)
    assert route(K.chain_desc(DEFAULT), 37, 91, g2) == K.ROUTE_OPS
    assert route(K.chain_desc(DEFAULT, gate_on=True), 37, 91, g2) == K.ROUTE_OPS
    # the route agrees with rv_clahe_median_letterbox_fits on the default chain
    for H, W in [(720, 1280), (360, 640), (130, 257), (45, 61), (700, 500)]:
        g = K.letterbox_geometry(H, W)
        fits = K.clahe_median_letterbox_fits(H, W, 8, 3, g)
        assert (route(K.chain_desc(DEFAULT), H, W, g) == K.ROUTE_FUSED) == fits, (H, W)


def test_workspace_sizes():
    from rvs_amd import kernels
    K = kernels
    B, H, W = 3, 130, 257
    lut = K.clahe_ws_bytes(B, 8)
    ws = K.preprocess_chain_ws_bytes
    assert ws(K.chain_desc(DEFAULT), B, H, W) == lut          # one pass: LUTs only
    assert ws(K.chain_desc([("median", 5)]), B, H, W) == 0     # nothing to keep
    assert ws(K.chain_desc(DEFAULT, enabled=False), B, H, W) == 0
    gated = ws(K.chain_desc(DEFAULT, gate_on=True), B, H, W)
    assert lut + 3 * B * 4 <= gated <= lut + 256              # + 2 B gate ints + B flags
    frames = B * H * 3 * W
    two = ws(K.chain_desc([("clahe", "LAB", 8, 2.0), ("median", 3)]), B, H, W)
    assert lut + frames <= two <= lut + frames + 256           # + one scratch batch
    four = ws(K.chain_desc([("median", 3), ("clahe", "LAB", 4, 2.0)] * 2), B, H, W)
    assert four <= K.clahe_ws_bytes(B, 4) + frames + 512       # still one scratch batch
    wide = ws(K.chain_desc([("median", 3), ("median", 5)]), B, H, W, 3 * W + 21)
    assert B * H * (3 * W + 21) <= wide <= B * H * (3 * W + 21) + 256
    assert ws(K.chain_desc(DEFAULT * 3), B, H, W) == 0         # bad descriptor


def _call(lib, desc, ws_bytes, lb, geo, in_=4096, out=1 << 16, ws=1 << 20, B=2, H=64, W=64):
    from rvs_amd import _lib as L
    return lib.rv_preprocess_chain_u8(in_, out, B, H, W, 3 * W, desc, ws, ws_bytes, lb,
                                      None if geo is None else L.int_array(geo), None)


def test_argument_errors_touch_no_device():
    """Every check answers RV_EINVAL (-1000) with a message before any HIP
    call: the pointers below are made-up integers."""
    from rvs_amd import kernels
    K = kernels
    L, lib = _lib()
    geo = K.letterbox_geometry(64, 64)
    big = 1 << 24
    bad = [
        (K.chain_desc(DEFAULT * 2 + [("median", 3)]), b"n_ops"),                # n_ops = 5
        (K.chain_desc([("clahe", "YCrCb", 8, 2.0), ("median", 4)]), b"k=4"),
        (K.chain_desc([("clahe", "YCrCb", 1, 2.0), ("median", 3)]), b"tiles"),
    ]
    for desc, word in bad:
        assert _call(lib, desc, big, 1 << 22, geo) == -1000
        assert word in lib.rv_last_error(), lib.rv_last_error()
        assert lib.rv_preprocess_chain_route(desc, 64, 64, L.int_array(geo)) == -1000
        assert lib.rv_preprocess_chain_ws_bytes(desc, 2, 64, 64, 192) == 0
        with pytest.raises(L.RVError):
            K.preprocess_chain_route(desc, 64, 64, geo)
    ok = K.chain_desc(DEFAULT)
    assert _call(lib, ok, big, 1 << 22, None) == -1000          # lb_out without geo
    assert b"geo" in lib.rv_last_error()
    assert _call(lib, ok, big, None, geo) == -1000              # geo without lb_out
    need = K.preprocess_chain_ws_bytes(ok, 2, 64, 64)
    assert need > 0
    assert _call(lib, ok, need - 1, 1 << 22, geo) == -1000      # workspace too small
    assert b"workspace" in lib.rv_last_error()
    assert _call(lib, ok, need, 1 << 22, geo, ws=None) == -1000
    assert _call(lib, None, big, 1 << 22, geo) == -1000         # null descriptor
    assert _call(lib, ok, big, 1 << 22, geo, in_=None) == -1000
    assert _call(lib, ok, big, 1 << 22, geo, out=4096) == -1000  # in == out
    assert _call(lib, ok, big, 1 << 22, geo, ws=4096 + 64) == -1000  # ws inside the frames
    # out may be NULL ("proc is the input") for a disabled or empty chain only
    assert _call(lib, ok, big, 1 << 22, geo, out=None) == -1000
    assert b"null" in lib.rv_last_error()
    # a well-formed call on an empty batch returns RV_OK without launching
    assert _call(lib, ok, big, 1 << 22, geo, B=0) == 0
    assert _call(lib, K.chain_desc(DEFAULT, enabled=False), 0, 1 << 22, geo, out=None, ws=None,
                 B=0) == 0
    assert _call(lib, K.chain_desc([]), 0, 1 << 22, geo, out=None, ws=None, B=0) == 0


def _pipe(chain, **kw):
    from rvs_amd.preprocess import PreprocessPipeline
    cfg = {"enabled": True, "chain": chain}
    cfg.update(kw)
    return PreprocessPipeline(cfg)


def _ops(desc):
    b = bytes(desc)
    n = struct.unpack_from("<i", b, 4)[0]
    return [struct.unpack_from("<iiiid", b, 24 + 24 * i) for i in range(n)]


def test_pipeline_descriptor_normalises_like_the_reference():
    p = _pipe([{"name": "CLAHEDehaze", "params": {"space": "lab", "clip_limit": 3.0,
                                                  "tile_grid": 1}},
               {"name": "MedianDerain", "params": {"ksize": 4}}],
              auto_gate={"enable_low_contrast_gate": True, "contrast_thresh": 17.5})
    assert p.chain_supported and p.unsupported_op is None
    assert struct.unpack_from("<iiiid", bytes(p.chain_desc), 0) == (1, 2, 1, 0, 17.5)
    assert _ops(p.chain_desc) == [(0, 1, 2, 0, 3.0), (1, 0, 0, 5, 0.0)]  # LAB, grid 2; k 5
    assert not p._fused
    q = _pipe([{"name": "CUDAMedianDerain", "params": {"ksize": 12}},
               {"name": "HIPCLAHEDehaze", "params": {}}], enabled=False)
    assert struct.unpack_from("<iiiid", bytes(q.chain_desc), 0) == (0, 2, 0, 0, 20.0)
    assert _ops(q.chain_desc) == [(1, 0, 0, 9, 0.0), (0, 0, 8, 0, 2.0)]
    assert _ops(_pipe([]).chain_desc) == []
    from rvs_amd import kernels
    d = _pipe([{"name": "CLAHEDehaze", "params": {}}, {"name": "MedianDerain", "params": {}}])
    assert d._fused
    assert d.chain_route(1080, 1920, kernels.letterbox_geometry(1080, 1920)) == kernels.ROUTE_FUSED


def test_pipeline_reports_unsupported_chains():
    from rvs_amd.preprocess import registry
    from rvs_amd.preprocess.base import PreprocessOp
    from rvs_amd.preprocess.ops import MedianDerain

    class Invert(PreprocessOp):
        def __call__(self, image):
            return 255 - image

    class MyMedian(MedianDerain):  # a subclass may change __call__: not the built-in op
        pass

    registry.REGISTRY["Invert"] = Invert
    registry.REGISTRY["MyMedian"] = MyMedian
    try:
        p = _pipe([{"name": "MedianDerain", "params": {}}, {"name": "Invert", "params": {}}])
        assert not p.chain_supported and p.chain_desc is None and p.unsupported_op == "Invert"
        assert _pipe([{"name": "MyMedian", "params": {}}]).unsupported_op == "MyMedian"
        with pytest.raises(ValueError, match="Invert"):
            p.run_chain_with_letterbox(None)
    finally:
        del registry.REGISTRY["Invert"], registry.REGISTRY["MyMedian"]
    five = _pipe([{"name": "MedianDerain", "params": {}}] * 5)
    assert not five.chain_supported and "5 ops" in five.unsupported_op
    with pytest.raises(KeyError):
        _pipe([{"name": "NoSuchOp", "params": {}}])

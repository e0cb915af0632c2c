"""YOLOv5u's model.0 on the GPU: k6 s2 p2 from the u8 letterbox on i8 MFMAs
(stem.hip conv0k6_kernel), C0 = 16 (YOLOv5nu) and 80 (YOLOv5xu).

Crafted letterbox tensors go straight to forward_raw (no frames); X0 is read
back from the workspace.  Geometries: 64x96 B=1 and 160x224 B=3 (X0 widths 48
and 112: ragged last 64-pixel tiles, several blocks), and 32x32 B=1 (one
partial tile).  Only model.0 has weights; every other conv is zero.

Bar (the project's conv0 bar, tests/test_yolo_variants_gpu.py): against the
float64 conv (stride 2, padding 2) of the RGB image / 255, at most 1.01 bf16
ulp + 1e-6 for more than 0.9999 of the elements and at most 2 ulp + 1e-5 for
all.
"""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolov5u_ref as v5
from test_yolo_layers_gpu import bf16_to_f32, ulp_bf16

pytestmark = pytest.mark.gpu

CASES = [(v, H, W, B) for v in (5, 9) for H, W, B in ((64, 96, 1), (160, 224, 3), (32, 32, 1))]
_BLOBS = {}


def _blob(variant, tag, make):
    """Packed blob of a flat array whose only non-zero conv is model.0 =
    make() -> (w (C0, 3, 6, 6), b (C0,)); cached per (variant, tag)."""
    from rvs_amd.detect import weights
    if (variant, tag) not in _BLOBS:
        w, b = make()
        flat = np.zeros(v5.TOTALS[variant][1], np.float32)
        flat[:w.size] = w.ravel()
        flat[w.size:w.size + b.size] = b
        # model.1 (k3 s2, C0 -> c2): fixed random weights, so that X1 means
        # something in the fused-stem test; X0 does not depend on them
        c0, c1 = w.shape[0], v5.widths(variant)[0][1]
        rng = np.random.default_rng(99)
        o = w.size + b.size
        flat[o:o + c1 * c0 * 9] = rng.normal(0, 1 / np.sqrt(c0 * 9), c1 * c0 * 9)
        flat[o + c1 * c0 * 9:o + c1 * c0 * 9 + c1] = rng.normal(0, 0.5, c1)
        _BLOBS[(variant, tag)] = (torch.from_numpy(weights.pack(variant, flat)), w.astype(np.float32),
                                  b.astype(np.float32))
    return _BLOBS[(variant, tag)]


def _c0(variant):
    return v5.widths(variant)[0][0]


def _random_wb(variant, seed=0):
    rng = np.random.default_rng([variant, seed])
    c0 = _c0(variant)
    return (rng.normal(0, 0.25, (c0, 3, 6, 6)).astype(np.float32),
            rng.normal(0, 0.5, c0).astype(np.float32))


def _positive_wb(variant):
    rng = np.random.default_rng(variant)
    c0 = _c0(variant)
    return (rng.uniform(0.01, 0.08, (c0, 3, 6, 6)).astype(np.float32),
            rng.normal(0, 0.5, c0).astype(np.float32))


def _onehot_wb(variant, st):
    """Tap t = C0 * st + o (t < 108, (ch, ky, kx) order) is weight 1 of channel o."""
    c0 = _c0(variant)
    w = np.zeros((c0, 108), np.float32)
    for o in range(c0):
        if c0 * st + o < 108:
            w[o, c0 * st + o] = 1.0
    return w.reshape(c0, 3, 6, 6), np.zeros(c0, np.float32)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "v%d-%dx%d-b%d" % c)
def stem(request, cuda):
    from rvs_amd import _lib
    from rvs_amd.detect.yolo_hip import YoloEngine
    variant, H, W, B = request.param
    blob0, _, _ = _blob(variant, "zero", lambda: (np.zeros((_c0(variant), 3, 6, 6)), np.zeros(_c0(variant))))
    eng = YoloEngine(variant, np.zeros(v5.TOTALS[variant][1], np.float32), B, (H, W),
                     imgsz=max(H, W), device=cuda)
    assert (eng.in_h, eng.in_w) == (H, W) and eng.packed.numel() == blob0.numel()
    lib = _lib.load()
    info = (ctypes.c_int * 4)()
    off = ctypes.c_size_t()
    lib.rv_yolo_buffer_info(eng._h, B, 0, info, ctypes.byref(off))
    name = ctypes.create_string_buffer(64)
    lib.rv_yolo_buffer_name(eng._h, 0, name, 64)
    c0 = _c0(variant)
    assert name.value == b"X0" and tuple(info) == (H // 2, W // 2, c0, 0)
    raw = torch.empty((B, 84, eng.A), dtype=torch.float32, device=cuda)

    def x0(blob, lb):
        """X0 (B, H/2, W/2, C0) f32 of the unfused raw forward on letterbox lb."""
        eng.packed.copy_(blob)
        n = B * (H // 2) * (W // 2) * c0
        eng.ws[off.value:off.value + 2 * n].fill_(0xFF)  # NaN bf16: every element must be written
        eng.forward_raw(torch.from_numpy(np.ascontiguousarray(lb)).to(cuda), raw)
        torch.cuda.synchronize()
        u16 = eng.ws[off.value:off.value + 2 * n].cpu().numpy().view(np.uint16)
        return bf16_to_f32(u16).reshape(B, H // 2, W // 2, c0)

    def x1(blob, lb, fused):
        """(X1 (B, H/4, W/4, c2) as bf16 bits, X0 as bits) of a raw forward
        with the fused stem (production kernel sequence) or the unfused pair."""
        eng.packed.copy_(blob)
        eng.set_stem6_fused(True)
        eng.set_raw_fused(fused)
        eng.ws.fill_(0xFF)
        eng.forward_raw(torch.from_numpy(np.ascontiguousarray(lb)).to(cuda), raw)
        torch.cuda.synchronize()
        eng.set_raw_fused(False)
        out = []
        for i, (name, bh, bw, C, es, boff) in enumerate(eng.buffers(B)[:2]):
            assert name == ("X0", "X1")[i] and es == 2
            out.append(eng.ws[boff:boff + 2 * B * bh * bw * C].cpu().numpy().view(np.uint16)
                       .reshape(B, bh, bw, C))
        return out[1], out[0]

    yield types.SimpleNamespace(variant=variant, H=H, W=W, B=B, c0=c0, x0=x0, x1=x1, eng=eng)
    eng.close()


def _ref(lb, w, b):
    x = torch.from_numpy(np.ascontiguousarray(lb[..., ::-1].transpose(0, 3, 1, 2))).double() / 255
    y = F.silu(F.conv2d(x, torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=2,
                        padding=2))
    return y.numpy().transpose(0, 2, 3, 1)


def _check(got, y, what):
    assert got.shape == y.shape, what
    assert np.isfinite(got).all(), what
    d = np.abs(got - y)
    frac = float((d <= ulp_bf16(y) * 1.01 + 1e-6).mean())
    print(f"{what}: within 1.01 ulp {frac:.6f}, max dev / ulp {float((d / ulp_bf16(y)).max()):.3f}")
    assert frac > 0.9999, what
    assert (d <= 2 * ulp_bf16(y) + 1e-5).all(), what


def _image(s, seed):
    return np.random.default_rng(seed).integers(0, 256, (s.B, s.H, s.W, 3), dtype=np.uint8)


def test_random_input_against_float64(stem):
    blob, w, b = _blob(stem.variant, "random", lambda: _random_wb(stem.variant))
    lb = _image(stem, 1)
    _check(stem.x0(blob, lb), _ref(lb, w, b), "random")


def test_one_hot_taps(stem):
    """Each of the 108 (ch, ky, kx) taps alone in one output channel: tap
    t = C0 * set + o is weight 1 of channel o (7 sets for C0 = 16, 2 for 80).
    Pins the tap order and the BGR -> RGB flip."""
    c0 = stem.c0
    lb = _image(stem, 2)
    for st in range((108 + c0 - 1) // c0):
        blob, w, b = _blob(stem.variant, f"onehot{st}", lambda: _onehot_wb(stem.variant, st))
        got = stem.x0(blob, lb)
        _check(got, _ref(lb, w, b), f"one-hot set {st}")
        # the tap itself, not only the conv: channel o is SiLU(pixel / 255)
        # of RGB channel c at (2Y - 2 + ky, 2X - 2 + kx), zero outside
        pad = np.zeros((stem.B, stem.H + 4, stem.W + 4, 3))
        pad[:, 2:-2, 2:-2] = lb[..., ::-1] / 255.0
        for o in range(c0):
            t = c0 * st + o
            if t >= 108:
                assert not got[..., o].any()
                continue
            c, ky, kx = np.unravel_index(t, (3, 6, 6))
            v = pad[:, ky:ky + stem.H:2, kx:kx + stem.W:2, c]
            y = v / (1 + np.exp(-v))
            assert (np.abs(got[..., o] - y) <= 2 * ulp_bf16(y) + 1e-5).all(), (st, o)


def test_extreme_inputs(stem):
    """All-255 input under all-positive weights (the largest accumulators) and
    all-zero input (bias only, in every pixel)."""
    blob, w, b = _blob(stem.variant, "positive", lambda: _positive_wb(stem.variant))
    shape = (stem.B, stem.H, stem.W, 3)
    lb = np.full(shape, 255, np.uint8)
    _check(stem.x0(blob, lb), _ref(lb, w, b), "all-255")
    lb = np.zeros(shape, np.uint8)
    got = stem.x0(blob, lb)
    _check(got, _ref(lb, w, b), "all-zero")
    assert (got == got[0, 0, 0]).all()  # bias only: one value per channel


def test_single_pixels_and_zero_padding(stem):
    """A black image with one 255 pixel at each corner and at (1, 1), under
    random weights: zero padding on all four sides and no bleed from the
    neighbouring row or image (B = 3: the previous image is all 255).  Outside
    the pixel's receptive field X0 is bit for bit the all-black image's."""
    blob, w, b = _blob(stem.variant, "random", lambda: _random_wb(stem.variant))
    H, W, B = stem.H, stem.W, stem.B
    img = 1 if B == 3 else 0
    for (py, px) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (1, 1)):
        lb = np.zeros((B, H, W, 3), np.uint8)
        if B == 3:
            lb[0] = 255
        lb[img, py, px] = 255
        got = stem.x0(blob, lb)
        _check(got, _ref(lb, w, b), f"pixel ({py}, {px})")
        black = got[B - 1] if B == 3 else None
        if black is None:
            z = np.zeros_like(lb)
            black = stem.x0(blob, z)[0]
        # X0 (Y, X) sees rows 2Y - 2 .. 2Y + 3, columns 2X - 2 .. 2X + 3
        Y, X = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing="ij")
        seen = (2 * Y - 2 <= py) & (py <= 2 * Y + 3) & (2 * X - 2 <= px) & (px <= 2 * X + 3)
        assert 1 <= seen.sum() <= 9
        np.testing.assert_array_equal(got[img][~seen].view(np.uint32), black[~seen].view(np.uint32))
        assert (got[img][seen] != black[seen]).any()


@pytest.mark.parametrize("stem", [c for c in CASES if c[0] == 5], indirect=True,
                         ids=lambda c: "v%d-%dx%d-b%d" % c)
def test_fused_stem_x1_is_bit_identical(stem):
    """YOLOv5nu's fused stem (conv0-k6 + model.1, the P1 map in LDS) against
    the unfused pair on all of the above inputs: X1 bit for bit.  The fused run
    leaves X0 untouched, which shows that it is the fused kernel that ran."""
    H, W, B = stem.H, stem.W, stem.B
    rnd = _blob(5, "random", lambda: _random_wb(5))[0]
    pos = _blob(5, "positive", lambda: _positive_wb(5))[0]
    cases = [("random", rnd, _image(stem, 1)),
             ("all-255", pos, np.full((B, H, W, 3), 255, np.uint8)),
             ("all-zero", pos, np.zeros((B, H, W, 3), np.uint8))]
    for st in range(7):
        cases.append((f"one-hot {st}", _blob(5, f"onehot{st}", lambda: _onehot_wb(5, st))[0], _image(stem, 2)))
    for (py, px) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (1, 1)):
        lb = np.zeros((B, H, W, 3), np.uint8)
        if B == 3:
            lb[0] = 255
        lb[B // 2, py, px] = 255
        cases.append((f"pixel ({py}, {px})", rnd, lb))
    for what, blob, lb in cases:
        unf, x0u = stem.x1(blob, lb, fused=False)
        fus, x0f = stem.x1(blob, lb, fused=True)
        assert (x0f == 0xFFFF).all() and not (x0u == 0xFFFF).any(), what
        assert not (unf == 0xFFFF).any(), what
        np.testing.assert_array_equal(fus, unf, err_msg=what)

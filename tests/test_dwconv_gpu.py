"""rv_dwconv3x3_bf16 (csrc/dwconv.hip: YOLO11's DWConv 3x3 and the attention's
positional conv) against a float64 depthwise conv on the same bf16 inputs and
weights.

Bar, every element: |gpu - ref| <= 1 bf16 ulp of |ref| (ulp_bf16, x 1.01 for
the binade edge) + 1e-3 of the case's RMS for cancellation near zero -- the
conv bar of tests/test_yolo_layers_gpu.py without its allowance of stragglers
(9 f32 products per output leave no room for any).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RV_EINVAL = -1000


def ulp_bf16(x):
    a = np.abs(x).astype(np.float32)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 7)


def bf(x, dev):
    return torch.as_tensor(np.asarray(x, np.float32)).to(dev).to(torch.bfloat16)


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def dwconv(lib, xw, C, in_co, gw, gs, w, bias, outw, out_co, resw, res_co, act):
    """One launch on wide NHWC tensors; returns the status."""
    from rvs_amd import _lib
    B, H, W, in_cs = xw.shape
    st = lib.rv_dwconv3x3_bf16(xw.data_ptr(), B, H, W, C, in_cs, in_co, gw, gs, w.data_ptr(),
                               bias.data_ptr(), outw.data_ptr(), outw.shape[-1], out_co,
                               0 if resw is None else resw.data_ptr(),
                               0 if resw is None else resw.shape[-1], res_co, act,
                               _lib.stream_ptr())
    torch.cuda.synchronize()
    return st


def logical_channels(C, in_co, gw, gs):
    c = np.arange(C)
    return in_co + c if gw == 0 else in_co + (c // gw) * gs + c % gw


def reference(xw, C, in_co, gw, gs, w, bias, resw, res_co, act):
    x = f64(xw)[..., logical_channels(C, in_co, gw, gs)]
    wt = torch.from_numpy(f64(w).T.reshape(C, 1, 3, 3).copy())
    y = F.conv2d(torch.from_numpy(x.transpose(0, 3, 1, 2).copy()), wt,
                 torch.from_numpy(bias.cpu().numpy().astype(np.float64)), padding=1, groups=C)
    if act:
        y = F.silu(y)
    y = y.numpy().transpose(0, 2, 3, 1)
    if resw is not None:
        y = y + f64(resw)[..., res_co:res_co + C]
    return y


def assert_close(got, ref, what):
    rms = float(np.sqrt(np.mean(ref ** 2))) + 1e-12
    d = np.abs(got - ref)
    tol = ulp_bf16(ref) * 1.01 + 1e-3 * rms
    bad = d > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} beyond 1 bf16 ulp, worst "
                           f"{float((d / tol).max()):.2f} x the bar at {np.argwhere(bad)[0].tolist()}")


@pytest.fixture(scope="module")
def lib(cuda):
    from rvs_amd import _lib
    return _lib.load()


def run_case(lib, cuda, rng, B, H, W, C, act, res, w=None, what=""):
    x = bf(rng.normal(0, 1, (B, H, W, C)), cuda)
    w = bf(rng.normal(0, 0.4, (9, C)), cuda) if w is None else w
    bias = torch.as_tensor(rng.normal(0, 0.3, C).astype(np.float32)).to(cuda)
    r = bf(rng.normal(0, 1, (B, H, W, C)), cuda) if res else None
    out = torch.zeros((B, H, W, C), dtype=torch.bfloat16, device=cuda)
    assert dwconv(lib, x, C, 0, 0, 0, w, bias, out, 0, r, 0, act) == 0
    assert_close(f64(out), reference(x, C, 0, 0, 0, w, bias, r, 0, act),
                 f"{what} {H}x{W} C={C} act={act} res={res}")


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7), (20, 20)])
@pytest.mark.parametrize("C", [8, 64, 80, 104])
def test_maps_and_channel_counts(lib, cuda, H, W, C):
    """Maps from one pixel (every tap but the centre is padding) to 20x20
    (three 8-row strips; at C = 104, 260 threads: two workgroups per row
    strip), SiLU and residual on and off."""
    rng = np.random.default_rng(1000 * H + 10 * W + C)
    for act in (0, 1):
        for res in (False, True):
            run_case(lib, cuda, rng, 2, H, W, C, act, res)


@pytest.mark.parametrize("tap", range(9))
def test_every_tap_alone(lib, cuda, tap):
    """Only tap (ky, kx) non-zero: the output is the input shifted by it."""
    rng = np.random.default_rng(tap)
    C = 16
    w = np.zeros((9, C), np.float32)
    w[tap] = rng.normal(0, 1, C)
    for H, W in ((5, 7), (9, 4)):  # 9 rows: the shift crosses the strip boundary at row 8
        run_case(lib, cuda, rng, 1, H, W, C, 0, False, w=bf(w, cuda), what=f"tap {tap}")


def test_borders_and_corners_count_their_taps(lib, cuda):
    """Ones in, ones as weights, no bias: the output is the number of taps
    inside the map -- 4 in the corners, 6 on the edges, 9 inside -- exactly."""
    C = 8
    for H, W in ((3, 3), (8, 9), (17, 5), (1, 6), (6, 1)):
        x = torch.ones((2, H, W, C), dtype=torch.bfloat16, device=cuda)
        w = torch.ones((9, C), dtype=torch.bfloat16, device=cuda)
        bias = torch.zeros(C, dtype=torch.float32, device=cuda)
        out = torch.zeros_like(x)
        assert dwconv(lib, x, C, 0, 0, 0, w, bias, out, 0, None, 0, 0) == 0
        ny = np.minimum(np.arange(H) + 1, H - 1) - np.maximum(np.arange(H) - 1, 0) + 1
        nx = np.minimum(np.arange(W) + 1, W - 1) - np.maximum(np.arange(W) - 1, 0) + 1
        want = np.broadcast_to((ny[:, None] * nx[None, :])[None, :, :, None], (2, H, W, C))
        np.testing.assert_array_equal(f64(out), want, err_msg=f"{H}x{W}")


@pytest.mark.parametrize("act,res", [(0, True), (1, False)])
def test_head_strided_view_reads_v_only_and_writes_its_slice_only(lib, cuda, act, res):
    """The attention's pe: v of a qkv map (64 channels of every 128 from 64)
    as the input, NaN in every channel and tensor element outside the views,
    the output a slice of a wider tensor framed by canaries."""
    rng = np.random.default_rng(5)
    B, H, W, heads = 2, 5, 7, 2
    C = 64 * heads
    qkv = rng.normal(0, 1, (B, H, W, 128 * heads + 8)).astype(np.float32)
    keep = np.zeros(qkv.shape[-1], bool)
    keep[logical_channels(C, 64, 64, 128)] = True
    qkv[..., ~keep] = np.nan
    qkv = bf(qkv, cuda)
    rw = rng.normal(0, 1, (B, H, W, C + 16)).astype(np.float32)
    rw[..., :8] = np.nan
    rw[..., 8 + C:] = np.nan
    rw = bf(rw, cuda) if res else None
    w = bf(rng.normal(0, 0.4, (9, C)), cuda)
    bias = torch.as_tensor(rng.normal(0, 0.3, C).astype(np.float32)).to(cuda)
    outw = torch.full((B, H, W, C + 24), 7.0, dtype=torch.bfloat16, device=cuda)
    assert dwconv(lib, qkv, C, 64, 64, 128, w, bias, outw, 16, rw, 8, act) == 0
    o = f64(outw)
    assert np.isfinite(o).all(), "a channel outside the view was read"
    np.testing.assert_array_equal(o[..., :16], 7.0)
    np.testing.assert_array_equal(o[..., 16 + C:], 7.0)
    assert_close(o[..., 16:16 + C], reference(qkv, C, 64, 64, 128, w, bias, rw, 8, act), "v view")


def test_argument_contract(lib, cuda):
    """Every unsupported argument is refused with RV_EINVAL and nothing is written."""
    B, H, W, C = 1, 4, 4, 16
    x = torch.zeros((B, H, W, 32), dtype=torch.bfloat16, device=cuda)
    w = torch.ones((9, C), dtype=torch.bfloat16, device=cuda)
    bias = torch.ones(C, dtype=torch.float32, device=cuda)
    out = torch.full((B, H, W, 32), 7.0, dtype=torch.bfloat16, device=cuda)
    from rvs_amd import _lib
    s = _lib.stream_ptr()
    X, Wp, Bp, O = x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr()
    #        in B  H  W  C  cs  co gw gs  w   b   out cs  co res cs co act
    good = [X, B, H, W, C, 32, 0, 0, 0, Wp, Bp, O, 32, 0, 0, 0, 0, 1, s]
    assert lib.rv_dwconv3x3_bf16(*good) == 0
    torch.cuda.synchronize()
    assert (out[..., :C].float() != 7.0).all() and (out[..., C:].float() == 7.0).all()
    out.fill_(7.0)
    bad = {
        "null in": {0: 0}, "null w": {9: 0}, "null bias": {10: 0}, "null out": {11: 0},
        "B 0": {1: 0}, "H 0": {2: 0}, "W 0": {3: 0}, "C 0": {4: 0}, "C 12": {4: 12},
        "in_cs 12": {5: 12}, "in_cs odd": {5: 36}, "in_co 4": {6: 4}, "in_co past": {6: 24},
        "in_co < 0": {6: -8}, "gw 12": {7: 12, 8: 16}, "gw not dividing": {4: 24, 7: 16, 8: 16},
        "gs < gw": {7: 8, 8: 0}, "gs 12": {7: 8, 8: 12}, "groups past cs": {7: 8, 8: 32},
        "gs without gw": {8: 8}, "in misaligned": {0: X + 2}, "w misaligned": {9: Wp + 2},
        "bias misaligned": {10: Bp + 4}, "out misaligned": {11: O + 8},
        "out_cs 12": {12: 12}, "out_co 4": {13: 4}, "out_co past": {13: 24},
        "res_cs 8": {14: X, 15: 8}, "res_co 4": {14: X, 16: 4}, "res misaligned": {14: X + 4, 15: 32},
        "res_co past": {14: X, 15: 32, 16: 24},
    }
    for what, ch in bad.items():
        a = list(good)
        for k, v in ch.items():
            a[k] = v
        assert lib.rv_dwconv3x3_bf16(*a) == RV_EINVAL, what
        assert lib.rv_last_error(), what
    torch.cuda.synchronize()
    assert (out.float() == 7.0).all(), "a refused call wrote"

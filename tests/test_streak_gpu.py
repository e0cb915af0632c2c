"""The rain-streak kernels (csrc/derain.hip) against tests/streak_ref.py, bit
for bit on the frames and on the streak plane S: every case of
streak_cases.py, a batch, a pitch above 3 W, strided views, the op through the
pipeline and through rv_preprocess_chain_u8 with its letterbox and gate."""
import functools

import numpy as np
import pytest

import streak_cases as C
from streak_ref import streak_ref
from oracle import cpu

pytestmark = pytest.mark.gpu

DEFAULT_P = (3, 9, 0, -1, 20)  # streak_params(dict(slant=-1))


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_matches_reference(cuda, name):
    from rvs_amd import kernels
    want_out, want_s, _ = C.reference(name)
    x = _dev(C.frame(name), cuda)
    out, s = kernels.streak_derain(x, *C.params(name), s=True)
    np.testing.assert_array_equal(s.cpu().numpy(), want_s, err_msg="S")
    np.testing.assert_array_equal(out.cpu().numpy(), want_out, err_msg="out")
    np.testing.assert_array_equal(x.cpu().numpy(), C.frame(name))  # input untouched


def test_batch_mixes_rain_free_rainy_and_saturated(cuda):
    from rvs_amd import kernels
    assert all(C.params(n) == DEFAULT_P for n in C.BATCH)
    x = _dev(np.stack([C.frame(n) for n in C.BATCH]), cuda)
    out, s = kernels.streak_derain(x, *DEFAULT_P, s=True)
    counts = [int((C.reference(n)[1] > 0).sum()) for n in C.BATCH]
    assert counts[0] == 0 and counts[1] > 0 and counts[2] > 0
    for b, n in enumerate(C.BATCH):
        np.testing.assert_array_equal(s[b].cpu().numpy(), C.reference(n)[1], err_msg=n)
        np.testing.assert_array_equal(out[b].cpu().numpy(), C.reference(n)[0], err_msg=n)
    again = kernels.streak_derain(x, *DEFAULT_P)
    np.testing.assert_array_equal(again.cpu().numpy(), out.cpu().numpy())  # two runs, same bytes


@pytest.mark.parametrize("max_len", [0, 97])
def test_odd_width_with_a_pitch_above_3w(cuda, max_len):
    """W = 67 in rows of 3 * 67 + 5 bytes: no row but the first is aligned."""
    import torch
    from rvs_amd import _lib, kernels
    img = C.frame("tail_66x67")
    H, W = img.shape[:2]
    prm = (3, 3, max_len, -4, 1)
    want_out, want_s = streak_ref(img, *prm)
    pitch = 3 * W + 5
    src = torch.full((2, H, pitch), 7, dtype=torch.uint8, device=cuda)
    dst = torch.full((2, H, pitch), 9, dtype=torch.uint8, device=cuda)
    src[:, :, :3 * W] = _dev(np.stack([img, img[::-1]]).reshape(2, H, 3 * W), cuda)
    s = torch.empty((2, H, W), dtype=torch.uint8, device=cuda)
    ws = torch.empty(kernels.streak_ws_bytes(2, H, W, max_len), dtype=torch.uint8, device=cuda)
    kernels.call("rv_streak_derain_u8", kernels.ptr(src), kernels.ptr(dst), 2, H, W, pitch, *prm,
                 kernels.ptr(ws), ws.numel(), kernels.ptr(s), kernels.stream_ptr())
    host = dst.cpu().numpy()
    np.testing.assert_array_equal(host[0, :, :3 * W].reshape(H, W, 3), want_out)
    np.testing.assert_array_equal(s[0].cpu().numpy(), want_s)
    flip_out, flip_s = streak_ref(np.ascontiguousarray(img[::-1]), *prm)
    np.testing.assert_array_equal(host[1, :, :3 * W].reshape(H, W, 3), flip_out)
    np.testing.assert_array_equal(s[1].cpu().numpy(), flip_s)
    assert (host[:, :, 3 * W:] == 9).all()              # the padding bytes keep their fill


@pytest.mark.parametrize("view_in,view_out", [(True, False), (False, True), (True, True)])
def test_views_one_pixel_into_a_wider_buffer(cuda, view_in, view_out):
    """The ABI takes one pitch for both, so a view on one side means the same
    (B, H, W + 2) layout on the other; the data starts at pixel 1 or pixel 0."""
    import torch
    from rvs_amd import kernels
    names = ["tail_40x254", "tail_40x254"]  # W + 2 = 256
    img = np.stack([C.frame(n) for n in names])
    B, H, W = img.shape[:3]
    src = torch.full((B, H, W + 2, 3), 7, dtype=torch.uint8, device=cuda)
    dst = torch.full((B, H, W + 2, 3), 9, dtype=torch.uint8, device=cuda)
    si, so = (1 if view_in else 0), (1 if view_out else 0)
    src[:, :, si:si + W] = _dev(img, cuda)
    xin, xout = src[:, :, si:si + W], dst[:, :, so:so + W]
    got = kernels.streak_derain(xin, *C.params(names[0]), out=xout)
    assert got.data_ptr() == xout.data_ptr()
    host = dst.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(host[b, :, so:so + W], C.reference(names[b])[0])
    pad = np.ones(W + 2, bool)
    pad[so:so + W] = False
    assert (host[:, :, pad] == 9).all()                 # the padding columns keep their fill
    spad = np.ones(W + 2, bool)
    spad[si:si + W] = False
    assert (src.cpu().numpy()[:, :, spad] == 7).all()


def test_op_through_the_pipeline(cuda):
    from rvs_amd.preprocess import PreprocessPipeline
    pipe = PreprocessPipeline({"enabled": True, "chain": [
        {"name": "StreakDerain", "params": dict(C.CASES["rain_default"][1])}]})
    got = pipe(np.array(C.frame("rain_default")))
    assert isinstance(got, np.ndarray)
    np.testing.assert_array_equal(got, C.reference("rain_default")[0])
    x = _dev(np.stack([C.frame(n) for n in C.BATCH]), cuda)
    out = pipe(x)
    assert out.is_cuda
    for b, n in enumerate(C.BATCH):
        np.testing.assert_array_equal(out[b].cpu().numpy(), C.reference(n)[0], err_msg=n)


Y8 = ("clahe", "YCrCb", 8, 2.0)
ST = ("streak",) + DEFAULT_P
ST_POS = ("streak", 3, 9, 49, 1, 20)
CHAINS = {
    "alone": [ST],
    "first_of_four": [ST, Y8, ("median", 3), ("median", 5)],
    "last_of_four": [("median", 5), Y8, ("median", 3), ST],
    "two_slants": [ST, ST_POS],
}


@functools.lru_cache(maxsize=None)
def _chain_ref(name, frame_name):
    out = C.frame(frame_name)
    for op in CHAINS[name]:
        if op[0] == "median":
            out = cpu.median(out, op[1])
        elif op[0] == "clahe":
            out = cpu.clahe_ycrcb(out, op[2], op[3])
        else:
            out = streak_ref(out, *op[1:])[0]
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_with_letterbox_matches_the_composition(cuda, name):
    from rvs_amd import kernels
    x = _dev(np.stack([C.frame(n) for n in C.BATCH]), cuda)
    H, W = x.shape[1:3]
    geo = kernels.letterbox_geometry(H, W)
    desc = kernels.chain_desc(CHAINS[name])
    assert kernels.preprocess_chain_route(desc, H, W, geo) == kernels.ROUTE_OPS
    proc, lb = kernels.preprocess_chain(x, desc, geo)
    proc, lb = proc.cpu().numpy(), lb.cpu().numpy()
    for b, n in enumerate(C.BATCH):
        want = _chain_ref(name, n)
        np.testing.assert_array_equal(proc[b], want, err_msg=f"proc {n}")
        np.testing.assert_array_equal(lb[b], cpu.letterbox(want, geo), err_msg=f"lb {n}")
    assert not np.array_equal(_chain_ref(name, "rain_default"), C.frame("rain_default"))
    p2, lb2 = kernels.preprocess_chain(x, desc, geo)
    np.testing.assert_array_equal(p2.cpu().numpy(), proc)
    np.testing.assert_array_equal(lb2.cpu().numpy(), lb)


def test_gated_chain_runs_the_low_contrast_frames_only(cuda):
    """Two frames under the gate's span and two over it, interleaved: the op
    runs on the first kind only, and the others come back raw."""
    from rvs_amd import kernels
    low = C.add_streak(C.add_streak(C.flat(96, 160, 200), 40, 30, 31, -1, 60), 50, 100, 21, -1, 60)
    low2 = C.add_streak(C.flat(96, 160, 180), 48, 80, 200, -1, 50)
    frames = [C.frame("rain_default"), low, C.frame("batch_saturated"), low2]
    span = [int(g.max() - g.min()) for g in
            [(f.astype(np.int32) * [1868, 9617, 4899]).sum(axis=2) + 8192 >> 14 for f in frames]]
    assert [s < 20 for s in span] == [False, True, False, True]
    x = _dev(np.stack(frames), cuda)
    H, W = x.shape[1:3]
    geo = kernels.letterbox_geometry(H, W)
    prm = (3, 9, 0, -1, 5)
    desc = kernels.chain_desc([("streak",) + prm, ("median", 3)], gate_on=True, contrast_thresh=20.0)
    proc, lb = kernels.preprocess_chain(x, desc, geo)
    proc, lb = proc.cpu().numpy(), lb.cpu().numpy()
    want = [f if s >= 20 else cpu.median(streak_ref(f, *prm)[0], 3) for f, s in zip(frames, span)]
    assert not np.array_equal(streak_ref(low, *prm)[0], low)
    assert not np.array_equal(streak_ref(low2, *prm)[0], low2)
    for b in range(4):
        np.testing.assert_array_equal(proc[b], want[b], err_msg=f"proc {b}")
        np.testing.assert_array_equal(lb[b], cpu.letterbox(want[b], geo), err_msg=f"lb {b}")

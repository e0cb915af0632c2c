"""The dark-channel dehaze kernels (csrc/dehaze.hip) against tests/dcp_ref.py,
bit for bit: the frames, the transmission plane and the airlight of every
case of dcp_cases.py, a batch, strided views, the op through the pipeline and
the chain through rv_preprocess_chain_u8 with its letterbox and gate."""
import functools

import numpy as np
import pytest

import dcp_cases as C
from dcp_ref import dcp_ref
from oracle import cpu

pytestmark = pytest.mark.gpu

DEFAULT_P = (15, 243, 26, 40, 65)


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_matches_reference(cuda, name):
    from rvs_amd import kernels
    want_out, want_t, want_air, _ = C.reference(name)
    x = _dev(C.frame(name), cuda)
    out, air, t = kernels.dcp_dehaze(x, *C.params(name), air=True, t=True)
    np.testing.assert_array_equal(air.cpu().numpy(), want_air, err_msg="air {A_b,A_g,A_r,L,cnt}")
    np.testing.assert_array_equal(t.cpu().numpy(), want_t, err_msg="t")
    np.testing.assert_array_equal(out.cpu().numpy(), want_out, err_msg="out")
    np.testing.assert_array_equal(x.cpu().numpy(), C.frame(name))  # input untouched


BATCH = ["patch_15", "noise_full", "radius_40"]  # three 70 x 150 frames, default parameters


def test_batch_of_three_has_a_per_frame_airlight(cuda):
    from rvs_amd import kernels
    assert all(C.params(n) == DEFAULT_P for n in BATCH)
    x = _dev(np.stack([C.frame(n) for n in BATCH]), cuda)
    out, air, t = kernels.dcp_dehaze(x, *DEFAULT_P, air=True, t=True)
    airs = [C.reference(n)[2] for n in BATCH]
    assert len({tuple(a) for a in airs}) == 3
    for b, n in enumerate(BATCH):
        np.testing.assert_array_equal(air[b].cpu().numpy(), airs[b], err_msg=n)
        np.testing.assert_array_equal(t[b].cpu().numpy(), C.reference(n)[1], err_msg=n)
        np.testing.assert_array_equal(out[b].cpu().numpy(), C.reference(n)[0], err_msg=n)
    again = kernels.dcp_dehaze(x, *DEFAULT_P)
    np.testing.assert_array_equal(again.cpu().numpy(), out.cpu().numpy())  # two runs, same bytes


@pytest.mark.parametrize("view_in,view_out", [(True, False), (False, True), (True, True)])
def test_views_one_pixel_into_a_wider_buffer(cuda, view_in, view_out):
    """The ABI takes one pitch for both, so a view on one side means the same
    (B, H, W + 2) layout on the other; the data starts at pixel 1 or pixel 0."""
    import torch
    from rvs_amd import kernels
    names = ["tail_40x254"] * 2  # W + 2 = 256: a 16-byte pitch
    img = np.stack([C.frame(n) for n in names])
    B, H, W = img.shape[:3]
    src = torch.full((B, H, W + 2, 3), 7, dtype=torch.uint8, device=cuda)
    dst = torch.full((B, H, W + 2, 3), 9, dtype=torch.uint8, device=cuda)
    si, so = (1 if view_in else 0), (1 if view_out else 0)
    src[:, :, si:si + W] = _dev(img, cuda)
    xin, xout = src[:, :, si:si + W], dst[:, :, so:so + W]
    got = kernels.dcp_dehaze(xin, *C.params(names[0]), out=xout)
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
        {"name": "DarkChannelDehaze", "params": dict(C.CASES["hazy"][1])}]})
    got = pipe(np.array(C.frame("hazy")))
    assert isinstance(got, np.ndarray)
    np.testing.assert_array_equal(got, C.reference("hazy")[0])
    x = _dev(np.stack([C.frame(n) for n in BATCH]), cuda)
    out = pipe(x)
    assert out.is_cuda
    for b, n in enumerate(BATCH):
        np.testing.assert_array_equal(out[b].cpu().numpy(), C.reference(n)[0], err_msg=n)


Y8 = ("clahe", "YCrCb", 8, 2.0)
DCP = ("dcp",) + DEFAULT_P
CHAINS = {"dcp": [DCP], "dcp_median3": [DCP, ("median", 3)], "clahe_dcp": [Y8, DCP]}


@functools.lru_cache(maxsize=None)
def _chain_ref(name, frame_name):
    out = C.frame(frame_name)
    for op in CHAINS[name]:
        if op[0] == "median":
            out = cpu.median(out, op[1])
        elif op[0] == "clahe":
            out = cpu.clahe_ycrcb(out, op[2], op[3])
        else:
            out = dcp_ref(out, *op[1:])[0]
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_with_letterbox_matches_the_composition(cuda, name):
    from rvs_amd import kernels
    x = _dev(np.stack([C.frame(n) for n in BATCH]), cuda)
    H, W = x.shape[1:3]
    geo = kernels.letterbox_geometry(H, W)
    desc = kernels.chain_desc(CHAINS[name])
    assert kernels.preprocess_chain_route(desc, H, W, geo) == kernels.ROUTE_OPS
    proc, lb = kernels.preprocess_chain(x, desc, geo)
    proc, lb = proc.cpu().numpy(), lb.cpu().numpy()
    for b, n in enumerate(BATCH):
        want = _chain_ref(name, n)
        np.testing.assert_array_equal(proc[b], want, err_msg=f"proc {n}")
        np.testing.assert_array_equal(lb[b], cpu.letterbox(want, geo), err_msg=f"lb {n}")
    p2, lb2 = kernels.preprocess_chain(x, desc, geo)
    np.testing.assert_array_equal(p2.cpu().numpy(), proc)
    np.testing.assert_array_equal(lb2.cpu().numpy(), lb)


def test_gated_chain_runs_the_low_contrast_frame_only(cuda):
    from rvs_amd import kernels
    low = (90 + (C.frame("patch_15").astype(np.int32) - 90) // 16).clip(0, 255).astype(np.uint8)
    frames = [C.frame("noise_full"), low, C.frame("radius_40")]
    span = [int(g.max() - g.min()) for g in
            [(f.astype(np.int32) * [1868, 9617, 4899]).sum(axis=2) + 8192 >> 14 for f in frames]]
    assert [s < 20 for s in span] == [False, True, False]
    x = _dev(np.stack(frames), cuda)
    H, W = x.shape[1:3]
    geo = kernels.letterbox_geometry(H, W)
    desc = kernels.chain_desc([DCP], gate_on=True, contrast_thresh=20.0)
    proc, lb = kernels.preprocess_chain(x, desc, geo)
    proc, lb = proc.cpu().numpy(), lb.cpu().numpy()
    want = [frames[0], dcp_ref(low, *DEFAULT_P)[0], frames[2]]
    assert not np.array_equal(want[1], low)
    for b in range(3):
        np.testing.assert_array_equal(proc[b], want[b], err_msg=f"proc {b}")
        np.testing.assert_array_equal(lb[b], cpu.letterbox(want[b], geo), err_msg=f"lb {b}")

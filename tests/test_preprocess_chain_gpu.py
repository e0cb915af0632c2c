"""rv_preprocess_chain_u8 on the GPU: every built-in chain, the device-side
low-contrast gate and the LetterBox against the CPU oracle and against the
same chain made of the eager calls, bit-exact (uint8 work).  B = 3 frames;
the shapes are the smallest that reach each edge: (45, 61) is smaller than
one block, has an odd width (byte path), reflect-padded CLAHE tiles and an
upscaling letterbox; (130, 257) is one or two pixels past the 128 / 32 block
edges; (360, 640) has scale 1 and 12 / 12 pad rows; (720, 1280) is the exact
2:1 downscale the fused letterbox emits."""
import functools

import numpy as np
import pytest

from conftest import road_frame
from oracle import cpu

pytestmark = pytest.mark.gpu

B = 3
SMALL = [(45, 61), (130, 257)]
SHAPES = SMALL + [(360, 640), (720, 1280)]
Y8 = ("clahe", "YCrCb", 8, 2.0)
LAB8 = ("clahe", "LAB", 8, 2.0)
# name -> (ops, enabled)
CHAINS = {
    "default": ([Y8, ("median", 3)], True),
    "k5": ([Y8, ("median", 5)], True),
    "k9": ([Y8, ("median", 9)], True),
    "lab_k3": ([LAB8, ("median", 3)], True),
    "median3": ([("median", 3)], True),
    "clahe": ([Y8], True),
    "median3_clahe": ([("median", 3), Y8], True),
    "disabled": ([Y8, ("median", 3)], False),
    "empty": ([], True),
}
CASES = [(n, s) for n in CHAINS for s in (SMALL if n == "k9" else SHAPES)]


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def cpu_gray_span(img):
    """cv2.cvtColor BGR2GRAY (14-bit) max - min (pipeline.py:24-30)."""
    i = img.astype(np.int32)
    g = (i[..., 0] * 1868 + i[..., 1] * 9617 + i[..., 2] * 4899 + 8192) >> 14
    return int(g.max() - g.min())


@functools.lru_cache(maxsize=None)
def _frame(H, W, kind, seed):
    """kind 'road': a road frame (span far above 20); 'low': squeezed to a
    span below 20; 'span20': squeezed, plus one gray pixel that makes the
    span exactly 20."""
    f = road_frame(H, W, seed=seed)
    if kind != "road":
        f = (90 + (f.astype(np.int32) - 90) // 16).clip(0, 255).astype(np.uint8)
    if kind == "span20":
        i = f.astype(np.int32)
        g = (i[..., 0] * 1868 + i[..., 1] * 9617 + i[..., 2] * 4899 + 8192) >> 14
        assert g.max() - g.min() < 20
        f = f.copy()
        f[H // 2, W // 2] = g.min() + 20  # B = G = R = v has gray exactly v
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _chain_ref(H, W, kind, seed, name):
    """The oracle's chain on one frame (computed once, shared, read-only)."""
    ops, enabled = CHAINS[name]
    out = _frame(H, W, kind, seed)
    if enabled:
        for op in ops:
            if op[0] == "median":
                out = cpu.median(out, op[1])
            elif op[1] == "LAB":
                out = cpu.clahe_lab(out, op[2], op[3])
            else:
                out = cpu.clahe_ycrcb(out, op[2], op[3])
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def _eager_chain(x, name):
    from rvs_amd import kernels
    ops, enabled = CHAINS[name]
    if enabled:
        for op in ops:
            if op[0] == "median":
                x = kernels.median(x, op[1])
            elif op[1] == "LAB":
                x = kernels.clahe_lab(x, op[2], op[3])
            else:
                x = kernels.clahe_ycrcb(x, op[2], op[3])
    return x


def _desc(name, gate_on=False, thresh=20.0):
    from rvs_amd import kernels
    ops, enabled = CHAINS[name]
    return kernels.chain_desc(ops, enabled=enabled, gate_on=gate_on, contrast_thresh=thresh)


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in CASES])
def test_chain_matches_oracle_and_eager_calls(cuda, name, shape):
    from rvs_amd import kernels
    H, W = shape
    spec = [("road", 100 + b) for b in range(B)]
    x = _dev(np.stack([_frame(H, W, k, s) for k, s in spec]), cuda)
    geo = kernels.letterbox_geometry(H, W)
    desc = _desc(name)
    fused = name == "default" and kernels.clahe_median_letterbox_fits(H, W, 8, 3, geo)
    assert kernels.preprocess_chain_route(desc, H, W, geo) == \
        (kernels.ROUTE_FUSED if fused else kernels.ROUTE_OPS)
    proc, lb = kernels.preprocess_chain(x, desc, geo)
    proc, lb = proc.cpu().numpy(), lb.cpu().numpy()
    assert lb.shape == (B, geo[0], geo[1], 3)
    for b, (k, s) in enumerate(spec):
        want = _chain_ref(H, W, k, s, name)
        np.testing.assert_array_equal(proc[b], want, err_msg=f"proc frame {b}")
        np.testing.assert_array_equal(lb[b], cpu.letterbox(want, geo), err_msg=f"lb frame {b}")
    eager = _eager_chain(x, name)
    np.testing.assert_array_equal(proc, eager.cpu().numpy())
    np.testing.assert_array_equal(lb, kernels.letterbox(eager, geo).cpu().numpy())
    if fused:  # route A is the fused entry's launches: the same bytes
        p2, lb2 = kernels.clahe_median_letterbox(x, 8, 2.0, 3, geo)
        np.testing.assert_array_equal(proc, p2.cpu().numpy())
        np.testing.assert_array_equal(lb, lb2.cpu().numpy())


BATCHES = {
    "mixed": [("low", 40), ("road", 41), ("low", 42)],
    "all_pass": [("road", 43), ("road", 44), ("road", 45)],
    "all_low": [("low", 46), ("low", 47), ("low", 48)],
    "span20": [("span20", 49), ("road", 50), ("low", 51)],
}
# low-contrast (chain runs) per frame at each threshold: a span of exactly 20
# passes at 20.0 (20 < 20.0 is false) and is processed at 20.5
LOW = {
    ("mixed", 20.0): [True, False, True], ("mixed", 20.5): [True, False, True],
    ("all_pass", 20.0): [False] * 3, ("all_pass", 20.5): [False] * 3,
    ("all_low", 20.0): [True] * 3, ("all_low", 20.5): [True] * 3,
    ("span20", 20.0): [False, False, True], ("span20", 20.5): [True, False, True],
}
GATED = [("default", (720, 1280)), ("default", (130, 257)), ("k5", (130, 257))]


@pytest.mark.parametrize("thresh", [20.0, 20.5])
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("name,shape", GATED, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in GATED])
def test_gate_on_device(cuda, name, shape, batch, thresh):
    """The gate runs on the device: low-contrast frames run the chain, the
    others come out as raw -- in proc and in the letterbox -- in one call.

    The default chain at (720, 1280) is the gate-aware fused pass
    (ROUTE_FUSED_GATED).  At (130, 257) the detector's letterbox upscales and
    the CLAHE cells of a block do not fit the fused pass, so by the route
    rules the gated default chain runs op by op there, like k = 5."""
    from rvs_amd import kernels
    H, W = shape
    spec = BATCHES[batch]
    frames = [_frame(H, W, k, s) for k, s in spec]
    spans = [cpu_gray_span(f) for f in frames]
    low = [float(s) < thresh for s in spans]
    assert low == LOW[(batch, thresh)], spans  # the fixture has the intended pattern
    if batch == "span20":
        assert spans[0] == 20
    geo = kernels.letterbox_geometry(H, W)
    desc = _desc(name, gate_on=True, thresh=thresh)
    want_route = kernels.ROUTE_FUSED_GATED if (name, shape) == ("default", (720, 1280)) \
        else kernels.ROUTE_OPS
    assert kernels.preprocess_chain_route(desc, H, W, geo) == want_route
    x = _dev(np.stack(frames), cuda)
    proc, lb = kernels.preprocess_chain(x, desc, geo)
    proc, lb = proc.cpu().numpy(), lb.cpu().numpy()
    for b, (k, s) in enumerate(spec):
        want = _chain_ref(H, W, k, s, name) if low[b] else frames[b]
        np.testing.assert_array_equal(proc[b], want, err_msg=f"proc frame {b} low={low[b]}")
        np.testing.assert_array_equal(lb[b], cpu.letterbox(want, geo),
                                      err_msg=f"lb frame {b} low={low[b]}")
    np.testing.assert_array_equal(x.cpu().numpy(), np.stack(frames))  # the input is untouched


@pytest.mark.parametrize("name,shape,gate", [("default", (720, 1280), False),
                                             ("default", (720, 1280), True),
                                             ("lab_k3", (130, 257), True)])
def test_proc_only_without_letterbox(cuda, name, shape, gate):
    from rvs_amd import kernels
    H, W = shape
    spec = BATCHES["mixed"]
    frames = [_frame(H, W, k, s) for k, s in spec]
    low = [cpu_gray_span(f) < 20.0 for f in frames]
    assert low == [True, False, True]
    proc, lb = kernels.preprocess_chain(_dev(np.stack(frames), cuda), _desc(name, gate_on=gate))
    assert lb is None
    for b, (k, s) in enumerate(spec):
        want = _chain_ref(H, W, k, s, name) if (low[b] or not gate) else frames[b]
        np.testing.assert_array_equal(proc[b].cpu().numpy(), want, err_msg=f"frame {b}")


@pytest.mark.parametrize("name", ["disabled", "empty"])
def test_identity_chain_without_out_returns_the_input(cuda, name):
    """No `out`: proc is the input tensor itself (as the pipeline returns it)
    and only the letterbox is produced; with `out`, proc is a copy."""
    from rvs_amd import kernels
    H, W = 130, 257
    frames = np.stack([_frame(H, W, "road", 100 + b) for b in range(B)])
    x = _dev(frames, cuda)
    geo = kernels.letterbox_geometry(H, W)
    proc, lb = kernels.preprocess_chain(x, _desc(name, gate_on=True), geo)
    assert proc is x
    for b in range(B):
        np.testing.assert_array_equal(lb[b].cpu().numpy(), cpu.letterbox(frames[b], geo))
    assert kernels.preprocess_chain(x, _desc(name))[0] is x
    import torch
    out = torch.zeros_like(x)
    proc, lb2 = kernels.preprocess_chain(x, _desc(name), geo, out=out)
    assert proc is out
    np.testing.assert_array_equal(out.cpu().numpy(), frames)
    np.testing.assert_array_equal(lb2.cpu().numpy(), lb.cpu().numpy())


@pytest.mark.parametrize("name,gate", [("median3_clahe", True), ("default", False),
                                       ("disabled", False)])
def test_padded_pitch(cuda, name, gate):
    """Frames that are a (B, H, W, 3) view of a (B, H, W + 7, 3) buffer: the
    row pitch is 3 W + 21 (no multiple of 16), proc keeps the view's layout
    and the two-pass chain's scratch batch uses the same pitch."""
    import torch
    from rvs_amd import kernels
    H, W = 130, 257
    spec = BATCHES["mixed"]
    frames = [_frame(H, W, k, s) for k, s in spec]
    low = [cpu_gray_span(f) < 20.0 for f in frames]
    assert low == [True, False, True]
    wide = torch.full((B, H, W + 7, 3), 7, dtype=torch.uint8, device=cuda)
    wide[:, :, :W] = _dev(np.stack(frames), cuda)
    view = wide[:, :, :W]
    out_wide = torch.full((B, H, W + 7, 3), 9, dtype=torch.uint8, device=cuda)
    geo = kernels.letterbox_geometry(H, W)
    proc, lb = kernels.preprocess_chain(view, _desc(name, gate_on=gate), geo,
                                        out=out_wide[:, :, :W])
    assert proc.stride() == view.stride()
    for b, (k, s) in enumerate(spec):
        want = _chain_ref(H, W, k, s, name) if (low[b] or not gate) else frames[b]
        np.testing.assert_array_equal(proc[b].cpu().numpy(), want, err_msg=f"frame {b}")
        np.testing.assert_array_equal(lb[b].cpu().numpy(), cpu.letterbox(want, geo))
    # the padding columns of both buffers are never written
    assert bool((out_wide[:, :, W:] == 9).all()) and bool((wide[:, :, W:] == 7).all())


def test_pipeline_runs_chain_without_host_gate(cuda):
    """PreprocessPipeline.run_chain_with_letterbox == pipeline(x) followed by
    the letterbox, gate on (ksize 4 -> 5, as the existing pipeline test)."""
    from rvs_amd import kernels
    from rvs_amd.preprocess import PreprocessPipeline
    cfg = {"enabled": True,
           "chain": [{"name": "CLAHEDehaze", "params": {"space": "YCrCb", "clip_limit": 2.0,
                                                         "tile_grid": 8}},
                     {"name": "MedianDerain", "params": {"ksize": 4}}],
           "auto_gate": {"enable_low_contrast_gate": True, "contrast_thresh": 20.0}}
    p = PreprocessPipeline(cfg)
    H, W = 130, 257
    spec = BATCHES["mixed"]
    x = _dev(np.stack([_frame(H, W, k, s) for k, s in spec]), cuda)
    geo = kernels.letterbox_geometry(H, W)
    proc, lb = p.run_chain_with_letterbox(x, geo)
    eager = p(x)  # the host-read gate of __call__
    np.testing.assert_array_equal(proc.cpu().numpy(), eager.cpu().numpy())
    np.testing.assert_array_equal(lb.cpu().numpy(), kernels.letterbox(eager, geo).cpu().numpy())
    for b, (k, s) in enumerate(spec):
        want = _chain_ref(H, W, k, s, "k5") if k == "low" else _frame(H, W, k, s)
        np.testing.assert_array_equal(proc[b].cpu().numpy(), want)

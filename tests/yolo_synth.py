"""Test-local synthetic YOLOv8 weights for any variant (n, s, m, l, x).

The package ships calibration arrays (rvs_amd/detect/data/synthetic_calib.npz)
for the variants its benchmarks run, n and m.  The layer tests of the other
plans need weights that keep every conv's pre-activation at O(1) too -- He-normal
weights alone vanish or explode through 60+ convs --, but no shipped data:
synth_weights() normalises rvs_amd.detect.weights.base_weights by the rule of
tests/golden/make_yolo_scales.py (per output channel: pre-activation std 1,
mean drawn from U(1, 2) for the SiLU convs; DFL logits std 0.7; class logits
std 1 with a +3 prior on the road classes and a common shift that makes
`target_cand` of the anchors pass conf 0.25) in ONE pass of the f32 CPU oracle
on the test's own letterboxed input: YoloRef.conv is hooked so that each conv
is normalised when the forward first reaches it, and the forward continues
with the normalised output (the script restarts the forward per conv, which is
quadratic in the number of convs).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conftest import road_frame
from oracle import cpu, yolo_ref

ROAD = (0, 2, 3, 5, 7)
MU = (1.0, 2.0)
BOX_STD, CLS_STD, ROAD_PRIOR, CONF = 0.7, 1.0, 3.0, 0.25


def _is_head(n, branch):
    return n.startswith(f"model.22.{branch}.") and n.endswith(".2")


class _Normalising(yolo_ref.YoloRef):
    """YoloRef whose conv() rescales its own weights on first use."""

    def __init__(self, variant, flat, seed):
        super().__init__(variant, flat)
        self.seed = seed
        self.order = {n: i for i, (n, *_rest) in enumerate(self.specs)}
        self.done = set()
        self.cls_logits = []

    def conv(self, n, x, res=None):
        if n in self.done:
            return super().conv(n, x, res)
        w, b, s, k, act = self.p[n]
        y = F.conv2d(x, w, b, stride=s, padding=k // 2)
        co = w.shape[0]
        target = BOX_STD if _is_head(n, "cv2") else CLS_STD if _is_head(n, "cv3") else 1.0
        sc = (target / y.std((0, 2, 3)).clamp_min(1e-6)).float()
        mu = torch.zeros(co)
        if act:
            mu = torch.from_numpy(np.random.default_rng([self.seed, self.order[n]])
                                  .uniform(MU[0], MU[1], co).astype(np.float32))
        shift = mu - y.mean((0, 2, 3)) * sc
        if _is_head(n, "cv3"):
            shift[list(ROAD)] += ROAD_PRIOR
        self.p[n] = (w * sc.view(-1, 1, 1, 1), b * sc + shift, s, k, act)
        self.done.add(n)
        # conv is linear in (w, b): the normalised conv's output without a second conv
        y = y * sc.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if _is_head(n, "cv3"):
            self.cls_logits.append(y.flatten(2))
        y = F.silu(y) if act else y
        return y if res is None else res + y


def frames(H, W, B, seed0=30):
    """(B, H, W, 3) u8: preprocessed (CLAHE + median) synthetic road frames."""
    return np.stack([cpu.median(cpu.clahe_ycrcb(road_frame(H, W, seed=seed0 + b)), 3)
                     for b in range(B)])


def letterboxed(H, W, B, imgsz, seed0=30):
    """(B, in_h, in_w, 3) u8: frames(), letterboxed on the CPU."""
    geo = cpu.letterbox_geometry(H, W, imgsz)
    return np.stack([cpu.letterbox(f, geo) for f in frames(H, W, B, seed0)])


def synth_weights_on(variant, lb, seed=1, target_cand=0.04):
    """Flat f32 weights (conv_specs order: weight[cout][cin][k][k], bias[cout]
    per conv) of `variant`, normalised on the letterboxed BGR u8 batch `lb`."""
    from rvs_amd.detect.weights import base_weights
    specs, _ = yolo_ref.conv_specs(variant)
    rng = np.random.default_rng(seed)
    flat = []
    for i, (n, ci, co, k, s, act) in enumerate(specs):
        w, b = base_weights(rng, seed, i, ci, co, k, 0.0)
        flat += [w.ravel(), b]
    m = _Normalising(variant, np.concatenate(flat), seed)
    del flat
    with torch.no_grad():
        m.forward(yolo_ref.preprocess(lb))
    assert len(m.done) == len(specs) and len(m.cls_logits) == 3
    # class logit shift: the (1 - target_cand) quantile of the per-anchor max
    # class logit lands on logit(conf); adding a constant to the last conv's
    # bias moves every logit by it, so no second forward is needed
    best = torch.cat(m.cls_logits, 2).max(1).values.numpy().ravel()
    delta = np.float32(np.log(CONF / (1 - CONF)) - np.quantile(best, 1 - target_cand))
    out = []
    for n, ci, co, k, s, act in specs:
        w, b = m.p[n][0], m.p[n][1]
        if _is_head(n, "cv3"):
            b = b + delta
        out += [w.numpy().ravel(), b.numpy().ravel()]
    return np.concatenate(out).astype(np.float32)


@functools.lru_cache(maxsize=4)
def synth_case(variant, H, W, B, imgsz, seed=1):
    """(flat weights, preprocessed frames (B, H, W, 3) u8) of a test geometry,
    normalised on those frames' letterbox; cached, treat as read-only."""
    flat = synth_weights_on(variant, letterboxed(H, W, B, imgsz), seed)
    flat.setflags(write=False)
    fr = frames(H, W, B)
    fr.setflags(write=False)
    return flat, fr


def split_params(variant, flat):
    """{conv name: (weight (cout, cin, k, k), bias (cout,))} views of flat."""
    specs, _ = yolo_ref.conv_specs(variant)
    params, off = {}, 0
    for n, ci, co, k, s, act in specs:
        nw = co * ci * k * k
        params[n] = (flat[off:off + nw].reshape(co, ci, k, k), flat[off + nw:off + nw + co])
        off += nw + co
    assert off == flat.size
    return specs, params


def oracle_stats(variant, flat, lb):
    """From the f32 oracle alone: ({SiLU conv: (min, max) over its channels
    of the pre-activation std}, fraction of anchors whose best class score passes conf)."""
    m = yolo_ref.YoloRef(variant, flat)
    stds = {}
    orig = m.conv

    def conv(n, x, res=None):
        w, b, s, k, act = m.p[n]
        if act:
            sd = F.conv2d(x, w, b, stride=s, padding=k // 2).std((0, 2, 3))
            stds[n] = (float(sd.min()), float(sd.max()))
        return orig(n, x, res)

    m.conv = conv
    with torch.no_grad():
        raw = m.forward(yolo_ref.preprocess(lb)).numpy()
    return stds, float((raw[:, 4:].max(1) > CONF).mean())

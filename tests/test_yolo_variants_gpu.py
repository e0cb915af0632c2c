"""The YOLOv8 s, l and x plans (and n, m at the same small geometries)
against float64, layer by layer.

Geometry: 160x224 frames at imgsz 224, batch 2 (P3 / P4 / P5 = 20x28, 10x14,
5x7: P5 odd in both dimensions, all three smaller than most pixel tiles) and
64x96 at imgsz 96, batch 1 (P5 = 2x3).  Weights: tests/yolo_synth.py,
normalised on the case's own letterboxed input (the package ships
calibration for n and m only).

Per case: (a) every conv recomputed in float64 from the GPU's own inputs
(test_yolo_layers_gpu.check_every_conv and its bars: 1.01 bf16 ulp + 1e-3 RMS
for all but < 1e-4 of the elements, none beyond 2 ulp + 1e-2 RMS, f32 head
logits to 1e-4 RMS + 1e-5 |ref|), model.0 against the float64 conv; (b) SPPF
pools exact, decode from the GPU's own head logits (xywh 2e-3 px, scores
1e-6), candidate count equal to the count from raw; (c) the production launch
list (fused chains, chained cv1) bit-identical to one launch per conv;
(d) every tile configuration bit-identical (autotune verify) and the tuned
forward's raw equal to the default's; (e) every conv launch has patch / direct
kernel configurations, i.e. none drops to the generic fallback kernel.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolo_synth
from test_yolo_layers_gpu import Introspect, _zero_candidate_launches, check_every_conv, ulp_bf16

pytestmark = pytest.mark.gpu

GEOMETRIES = [(160, 224, 2), (64, 96, 1)]
CASES = [(v, H, W, B) for v in (1, 3, 4, 0, 2) for H, W, B in GEOMETRIES]
NC, REG = 80, 16


def _engine(cuda, p):
    from rvs_amd.detect.yolo_hip import YoloEngine
    eng = YoloEngine(p.variant, p.flat, p.B, (p.H, p.W), imgsz=max(p.H, p.W), device=cuda)
    assert (eng.in_h, eng.in_w) == (p.H, p.W)
    return eng, eng.letterbox(torch.from_numpy(p.frames.copy()).to(cuda))


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "v%d-%dx%d-b%d" % c)
def plan(request, cuda):
    """One case: its weights and frames, and (lazily, shared by the tests that
    only read it) the default raw forward with every activation kept."""
    variant, H, W, B = request.param
    flat, fr = yolo_synth.synth_case(variant, H, W, B, max(H, W))
    p = types.SimpleNamespace(variant=variant, H=H, W=W, B=B, flat=flat, frames=fr, fwd=None)

    def forward():
        if p.fwd is None:
            eng, lb = _engine(cuda, p)
            raw = torch.empty((B, 4 + NC, eng.A), dtype=torch.float32, device=cuda)
            eng.forward_raw(lb, raw)
            ins = Introspect(eng, B)
            specs, params = yolo_synth.split_params(variant, flat)
            p.fwd = types.SimpleNamespace(eng=eng, ins=ins, specs=specs, params=params,
                                          lb=lb.cpu().numpy(), raw=raw.cpu().numpy())
        return p.fwd

    p.forward = forward
    yield p
    if p.fwd is not None:
        p.fwd.eng.close()


def test_every_conv_layerwise(plan):
    f = plan.forward()
    assert len(f.ins.recs) == len(f.specs) - 1  # every conv but model.0
    # model.0: k3 s2 from the u8 letterbox, its own kernel outside the trace
    w, b = f.params["model.0"]
    x = torch.from_numpy(f.lb[..., ::-1].transpose(0, 3, 1, 2).copy()).double() / 255
    y = F.silu(F.conv2d(x, torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=2,
                        padding=1)).numpy().transpose(0, 2, 3, 1)
    got = f.ins.view(0)
    assert got.shape == y.shape
    d = np.abs(got - y)
    assert (d <= ulp_bf16(y) * 1.01 + 1e-6).mean() > 0.9999 and (d <= 2 * ulp_bf16(y) + 1e-5).all()
    worst = check_every_conv(f.ins, f.specs, f.params)
    print(f"variant {plan.variant} {plan.H}x{plan.W} B={plan.B} worst layers: {worst}")


def test_sppf_decode_and_candidates(plan):
    f = plan.forward()
    eng, ins, raw, B = f.eng, f.ins, f.raw, plan.B
    names = [n for n, *_ in eng.buffers(B)]
    # SPPF: channels [c, 2c), [2c, 3c), [3c, 4c) are the 5 / 9 / 13 max pools of [0, c)
    s = ins.view(names.index("SP"))
    assert s.shape[1:3] == (plan.H // 32, plan.W // 32) and s.shape[-1] % 4 == 0
    c = s.shape[-1] // 4
    t = torch.from_numpy(np.ascontiguousarray(s[..., :c].transpose(0, 3, 1, 2)))
    p1 = F.max_pool2d(t, 5, 1, 2)
    p2 = F.max_pool2d(p1, 5, 1, 2)
    p3 = F.max_pool2d(p2, 5, 1, 2)
    for j, p in enumerate((p1, p2, p3)):
        np.testing.assert_array_equal(s[..., (j + 1) * c:(j + 2) * c], p.numpy().transpose(0, 2, 3, 1))
    # decode from the GPU's own f32 head logits
    outs, anc, st = [], [], []
    for lvl in range(3):
        v = ins.view(names.index(f"HD{lvl}"))
        assert v.dtype == np.float32 and v.shape[-1] == 4 * REG + NC
        h, w = v.shape[1:3]
        assert (h, w) == (plan.H // (8 << lvl), plan.W // (8 << lvl))
        outs.append(v.reshape(B, h * w, -1).transpose(0, 2, 1))
        sy, sx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        anc.append(np.stack([sx.ravel(), sy.ravel()]))
        st.append(np.full(h * w, 8.0 * 2 ** lvl))
    y = np.concatenate(outs, 2).astype(np.float64)
    A = y.shape[2]
    assert A == eng.A
    box = y[:, :4 * REG].reshape(B, 4, REG, A)
    e = np.exp(box - box.max(2, keepdims=True))
    dist = (e / e.sum(2, keepdims=True) * np.arange(REG).reshape(1, 1, REG, 1)).sum(2)
    an = np.concatenate(anc, 1)[None]
    s_ = np.concatenate(st)[None]
    x1y1, x2y2 = an - dist[:, :2], an + dist[:, 2:]
    xywh = np.concatenate([(x1y1 + x2y2) / 2, x2y2 - x1y1], 1) * s_[:, None]
    np.testing.assert_allclose(raw[:, :4], xywh, rtol=0, atol=2e-3)
    np.testing.assert_allclose(raw[:, 4:], 1 / (1 + np.exp(-y[:, 4 * REG:])), rtol=0, atol=1e-6)
    # candidates: every anchor whose best score passes conf, none else --
    # and the weights make both outcomes occur
    seg = eng.seg_n[0].view(-1)[:B * eng.nseg].view(B, eng.nseg).cpu().numpy()
    expect = (raw[:, 4:].max(1) > 0.25).sum(1)
    print(f"variant {plan.variant} {plan.H}x{plan.W}: candidates {expect.tolist()} of {A} anchors")
    np.testing.assert_array_equal(seg.sum(1), expect)
    assert 0 < expect.sum() < B * A


def _candidate_rows(eng, slot, B):
    """Per (image, segment) the valid candidate rows as sorted bit patterns
    (rows of one segment are appended in no fixed order)."""
    seg = eng.seg_n[slot].view(-1)[:B * eng.nseg].view(B, eng.nseg).cpu().numpy().copy()
    rows = eng.cand[slot].cpu().numpy().view(np.uint32)
    out = []
    for b in range(B):
        for s in range(eng.nseg):
            r = rows[b, 64 * s:64 * s + min(int(seg[b, s]), 64)]
            out.append(r[np.lexsort(r.T[::-1])])
    return seg, out


def test_production_launches_match_one_launch_per_conv(plan, cuda):
    """The default launch list (fused C2f chains, model.3 + model.4.cv1
    chained; per-tap k order in the width-16 chain) against one launch per
    conv: raw prediction, candidate counts and candidate rows bit-identical."""
    eng, lb = _engine(cuda, plan)
    B = plan.B
    eng.set_raw_fused(True)
    eng.set_c2f_tap_pairs(False)
    res, launches = [], []
    for slot in (0, 1):
        if slot == 1:
            eng.set_fuse_c2f(0)
            eng.set_fuse_cv1(False)
        raw = torch.full((B, 4 + NC, eng.A), float("nan"), dtype=torch.float32, device=cuda)
        eng.seg_n[slot].fill_(-7)
        eng.forward_raw(lb, raw, slot=slot)
        torch.cuda.synchronize()
        res.append((raw.cpu().numpy(),) + _candidate_rows(eng, slot, B))
        launches.append(_zero_candidate_launches(eng))
    # (launches without a conv configuration, launches): what the default
    # list fuses follows from the widths -- the C2f chains take hidden widths
    # 16 and 32 (n's model.2; s's model.2, whatever the width-32 default says
    # for n's model.4 / model.15), the chained cv1 a 64-channel model.3 (n);
    # m, l and x run one launch per conv either way.  The one-launch-per-conv
    # list has a configuration for every launch.
    assert launches[1][0] == 0
    if plan.variant in (0, 1):
        assert launches[0][0] >= 1 and launches[0][1] < launches[1][1], launches
    else:
        assert launches[0] == launches[1], launches
    (r0, s0, c0), (r1, s1, c1) = res
    assert np.isfinite(r0).all() and (s0 >= 0).all() and s0.sum() > 0
    np.testing.assert_array_equal(r0, r1)
    np.testing.assert_array_equal(s0, s1)
    for a, b in zip(c0, c1):
        np.testing.assert_array_equal(a, b)
    eng.close()


def test_every_tile_configuration_is_bit_identical(plan, cuda):
    """rv_yolo_autotune with verify: every valid kernel configuration of
    every conv launch reproduces the default configuration's output bits,
    and the tuned forward the default forward's raw prediction."""
    eng, lb = _engine(cuda, plan)
    raw0 = torch.full((plan.B, 4 + NC, eng.A), float("nan"), dtype=torch.float32, device=cuda)
    eng.forward_raw(lb, raw0)
    assert eng.autotune(lb, reps=1, verify=True) == 0
    cfgs = eng.tuned_configs()
    assert len(cfgs) > 0 and all(c[0] >= 0 for c in cfgs)
    ncand = [len(eng.conv_candidates(i)) for i in range(len(cfgs))]
    assert sum(ncand) > 0  # a plan with no candidates cannot pass vacuously
    raw1 = torch.full_like(raw0, float("nan"))
    eng.forward_raw(lb, raw1)
    r0 = raw0.cpu().numpy()
    assert np.isfinite(r0).all()
    np.testing.assert_array_equal(raw1.cpu().numpy(), r0)
    print(f"variant {plan.variant} {plan.H}x{plan.W}: {len(cfgs)} launches, "
          f"{sum(ncand)} configurations verified")
    eng.close()


# Conv launches that legitimately have no patch / direct configuration
# (conv name per variant): none.  DESIGN.md "Parity" records any entry.
NO_CONFIGURATION = {0: (), 1: (), 2: (), 3: (), 4: ()}


def test_no_conv_falls_back_to_the_generic_kernel(plan):
    """Every conv launch of the one-launch-per-conv forward has at least one
    patch / direct kernel configuration (rv_yolo_conv_candidates), so
    launch_conv never drops it to conv_mfma_kernel unnoticed.  The 1x1 convs
    with a virtual concat input are exempt (the direct kernel is their only
    kernel and launch_conv fails without it); the forward checked here has no
    fused chain."""
    f = plan.forward()
    lib, h = f.ins.lib, f.eng._h
    # launches in trace order; the head's last 1x1 stage (f32 logits) runs
    # inside the decode kernel and is no conv launch
    launched = [r for r in f.ins.recs if not f.ins.bufs[r[8]][3]]
    assert len(launched) == len(f.ins.recs) - 6
    assert lib.rv_yolo_conv_candidates(h, len(launched), None, 0) < 0  # one past the last launch
    missing = []
    for idx, r in enumerate(launched):
        n = lib.rv_yolo_conv_candidates(h, idx, None, 0)
        assert n >= 0
        name = f.specs[r[0]][0]
        if n == 0 and r[20] < 0 and name not in NO_CONFIGURATION[plan.variant]:
            missing.append((name, r[4:8].tolist()))
    assert not missing, f"no kernel configuration (generic fallback): {missing}"

"""The YOLO11 plans (variants 20..24: n, s, m, l, x) on the GPU, modelled on
tests/test_yolov5u_gpu.py and tests/test_yolo_variants_gpu.py, whose helpers
and assertions this file uses.

Geometry: 160x224 and 64x96 at batch 2 (P5 = 5x7 = 35 and 2x3 = 6 tokens);
YOLO11n also at 256x320 (P5 = 8x10 = 80 tokens: more than one 32-key tile of
the attention kernel, with a partial last one).  Weights: tests/yolo11_ref.py's
one-pass normalisation on the case's own letterbox.

Per case: every dense conv in float64 from the GPU's own inputs
(check_every_conv, unchanged bars; model.0 against the float64 k3 s2 conv);
every depthwise conv likewise under the same bars; every attention launch
against the float64 softmax attention on the GPU's own qkv map, |d| <= 2^-7 A
(the bar of tests/test_psa_attention_gpu.py); the WIRING -- each conv's and
attention's input and residual views resolved, through the trace records, to
the launches that wrote those channel slices, equal to the graph
yolo11_ref.expected_producers states; SPPF pools exact, decode from the GPU's
own logits, candidate counts from raw; the production launch list against one
launch per op; every tile configuration bit-identical under autotune verify
(the autotuner skips the depthwise and attention launches and keeps its
per-index alignment); no dense conv without a patch / direct configuration.
Then class counts 1, 70 and 128 on YOLO11n, the detector from an .npz
state_dict, and the pipelined engine.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_yolo_variants_gpu as tv
import yolo11_ref as y11
from conftest import road_frame
from oracle import yolo_ref
from test_yolo_layers_gpu import Introspect, check_every_conv, round_bf16, ulp_bf16

pytestmark = pytest.mark.gpu

GEOMETRIES = [(160, 224, 2), (64, 96, 2)]
CASES = [(v, H, W, B) for v in (20, 21, 22, 23, 24) for H, W, B in GEOMETRIES] + [(20, 256, 320, 2)]
NC, REG = 80, 16


def attn_records(eng):
    from rvs_amd import _lib
    lib = _lib.load()
    n = lib.rv_yolo_attn_trace(eng._h, None, 0)
    recs = np.zeros(n * 9, np.int32)
    assert lib.rv_yolo_attn_trace(eng._h, recs.ctypes.data, n) == n
    return recs.reshape(n, 9)


def _forward(cuda, variant, flat, frames, B, H, W, nc):
    from rvs_amd.detect.yolo_hip import YoloEngine
    eng = YoloEngine(variant, flat, B, (H, W), imgsz=max(H, W), device=cuda, nc=nc)
    assert (eng.in_h, eng.in_w) == (H, W)
    lb = eng.letterbox(torch.from_numpy(frames.copy()).to(cuda))
    raw = torch.full((B, 4 + nc, eng.A), float("nan"), dtype=torch.float32, device=cuda)
    eng.forward_raw(lb, raw)
    ins = Introspect(eng, B)
    specs, params = y11.split_params(variant, flat, nc)
    return types.SimpleNamespace(eng=eng, ins=ins, specs=specs, params=params, attn=attn_records(eng),
                                 dw=y11.conv_specs(variant, nc)[1]["dw"],
                                 lb=lb.cpu().numpy(), raw=raw.cpu().numpy())


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "v%d-%dx%d-b%d" % c)
def plan(request, cuda):
    """One case: its weights and frames, and (lazily, shared by the tests that
    only read it) the default raw forward with every activation kept."""
    variant, H, W, B = request.param
    flat, fr, _ = y11.synth_case(variant, H, W, B)
    p = types.SimpleNamespace(variant=variant, H=H, W=W, B=B, flat=flat, frames=fr, fwd=None)

    def forward():
        if p.fwd is None:
            p.fwd = _forward(cuda, variant, flat, fr, B, H, W, NC)
        return p.fwd

    p.forward = forward
    yield p
    if p.fwd is not None:
        p.fwd.eng.close()


def _check_model0(f):
    """model.0: k3 s2 from the u8 letterbox, its own kernel outside the trace."""
    w, b = f.params["model.0"]
    x = torch.from_numpy(f.lb[..., ::-1].transpose(0, 3, 1, 2).copy()).double() / 255
    y = F.silu(F.conv2d(x, torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=2,
                        padding=1)).numpy().transpose(0, 2, 3, 1)
    got = f.ins.view(0)
    assert got.shape == y.shape
    d = np.abs(got - y)
    assert (d <= ulp_bf16(y) * 1.01 + 1e-6).mean() > 0.9999 and (d <= 2 * ulp_bf16(y) + 1e-5).all()


def _dense_only(f):
    """f.ins restricted to the dense conv records (what check_every_conv computes)."""
    recs = np.array([r for r in f.ins.recs if f.specs[r[0]][0] not in f.dw])
    return types.SimpleNamespace(recs=recs, view=f.ins.view, bufs=f.ins.bufs)


def check_every_depthwise(f):
    """Every depthwise record in float64 on the GPU's own input, bf16 weights:
    the bars of check_every_conv.  The record's virtual-concat fields carry the
    input's group form (in2 cs = group stride, split = group width)."""
    n = 0
    for r in f.ins.recs:
        name, cin, cout, k, s, act = f.specs[r[0]]
        if name not in f.dw:
            continue
        (_c, inb, incs, inco, Hin, Win, Ho, Wo, o0, o0cs, o0co, up0, o1, o1cs, o1co, up1,
         rb, rcs, rco, in_up, in2b, gs, in2co, gw) = r.tolist()
        assert (k, s, cin, Ho, Wo, up0, o1, in_up, in2b) == (3, 1, cout, Hin, Win, 0, -1, 0, -1), name
        c = np.arange(cout)
        ch = inco + c if gw == 0 else inco + (c // gw) * gs + c % gw
        x = f.ins.view(inb)[..., ch]
        w, b = f.params[name]
        assert w.shape == (cout, 1, 3, 3)
        y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).double(),
                     torch.from_numpy(round_bf16(w)).double(), torch.from_numpy(b).double(),
                     padding=1, groups=cout)
        y = (F.silu(y) if act else y).numpy().transpose(0, 2, 3, 1)
        if rb >= 0:
            y = y + f.ins.view(rb)[..., rco:rco + cout]
        got = f.ins.view(o0)[..., o0co:o0co + cout]
        rms = float(np.sqrt(np.mean(y ** 2))) + 1e-12
        d = np.abs(got.astype(np.float64) - y)
        frac = float((d > ulp_bf16(y) * 1.01 + 1e-3 * rms).mean())
        assert frac < 1e-4, f"{name}: {frac:.2e} of elements beyond 1 ulp"
        assert (d <= 2 * ulp_bf16(y) + 1e-2 * rms).all(), f"{name}: max dev {d.max()}"
        n += 1
    return n


def check_every_attention(f, B):
    """Every attention launch against the float64 softmax attention on the
    GPU's own bf16 qkv map: |got - ref| <= 2^-7 sum_j P_ij |v_jd| everywhere."""
    worst = 0.0
    for qb, qcs, qco, heads, H, W, ob, ocs, oco in f.attn.tolist():
        N = H * W
        qkv = f.ins.view(qb).astype(np.float64)
        assert qkv.shape == (B, H, W, qcs) and qco + 128 * heads <= qcs
        qkv = qkv[..., qco:qco + 128 * heads].reshape(B, N, heads, 128)
        q, k, v = qkv[..., :32], qkv[..., 32:64], qkv[..., 64:]
        S = np.einsum("bihc,bjhc->bhij", q, k) * 32.0 ** -0.5
        P = np.exp(S - S.max(-1, keepdims=True))
        P /= P.sum(-1, keepdims=True)
        ref = np.einsum("bhij,bjhd->bihd", P, v)
        A = np.einsum("bhij,bjhd->bihd", P, np.abs(v))
        got = f.ins.view(ob).astype(np.float64)
        assert got.shape[-1] == ocs
        got = got[..., oco:oco + 64 * heads].reshape(B, N, heads, 64)
        d = np.abs(got - ref)
        assert (d <= 2.0 ** -7 * A).all(), f"attention at {H}x{W}: worst {(d / A).max() * 128:.2f} x the bar"
        worst = max(worst, float((d / np.maximum(A, 1e-300)).max() * 128))
    return len(f.attn), worst


def test_every_layer(plan):
    f = plan.forward()
    meta = y11.conv_specs(plan.variant)[1]
    assert len(f.ins.recs) == len(f.specs) - 1  # every conv but model.0
    assert np.isfinite(f.raw).all()
    _check_model0(f)
    worst = check_every_conv(_dense_only(f), f.specs, f.params)
    assert check_every_depthwise(f) == len(f.dw) == y11.TOTALS[plan.variant][1]
    n, aw = check_every_attention(f, plan.B)
    assert n == meta["rep"]
    assert all(r[3] == meta["heads"] and (r[4], r[5]) == (plan.H // 32, plan.W // 32) for r in f.attn)
    print(f"variant {plan.variant} {plan.H}x{plan.W} B={plan.B} worst layers: {worst}; "
          f"attention worst {aw:.3f} x 2^-7 A")


def resolve_producers(f, names):
    """{op name: ([(producer, upsampled?)], residual producer)} from the conv
    and attention records: every view an op reads is matched, channel by
    channel, with the output views (same buffer, same pixel stride, same map
    size) that cover it.  A read of exactly the first / second half of one
    write is tagged y11.FIRST / y11.HALF, the v channels of a qkv map y11.V;
    any other partial read fails.  Channels no op writes are SPPF's pools
    (buffer SP only); buffer 0 (X0) is model.0's, which has no record."""
    ins, specs = f.ins, f.specs
    writes = {}  # buffer -> [(channel offset, width, pixel stride, producer, Ho, Wo)]
    c0 = specs[0][2]
    writes[0] = [(0, c0, c0, specs[0][0], ins.bufs[0][0], ins.bufs[0][1])]
    qkv_of = {}
    for r in ins.recs:
        name, cout = specs[r[0]][0], specs[r[0]][2]
        if name.endswith(".attn.qkv"):
            qkv_of[int(r[8])] = name
        for ob, ocs, oco, up in ((r[8], r[9], r[10], r[11]), (r[12], r[13], r[14], r[15])):
            if ob >= 0:
                assert not up, f"{name}: no YOLO11 conv writes an upsampled copy"
                writes.setdefault(int(ob), []).append((int(oco), cout, int(ocs), name, int(r[6]), int(r[7])))
    attn_names = []
    for qb, qcs, qco, heads, H, W, ob, ocs, oco in f.attn.tolist():
        attn_names.append(qkv_of[qb][:-len(".qkv")])
        writes.setdefault(ob, []).append((oco, 64 * heads, ocs, attn_names[-1], H, W))
    for b, ws in writes.items():  # nothing overwritten inside a forward
        ws.sort()
        for a, c in zip(ws, ws[1:]):
            assert a[0] + a[1] <= c[0], f"buffer {names[b]}: {a[3]} and {c[3]} overlap"

    def cover(buf, co, width, cs, H, W, who):
        out, at = [], co
        for (o, w, wcs, name, Ho, Wo) in writes.get(int(buf), []):
            if o + w <= co or o >= co + width:
                continue
            assert wcs == cs, f"{who}: pixel stride {cs} but {name} wrote with {wcs}"
            assert (Ho, Wo) == (H, W), f"{who}: map {H}x{W} but {name} wrote {Ho}x{Wo}"
            lo = max(o, co)
            if lo > at:
                assert names[buf] == "SP", f"{who}: channels [{at}, {lo}) of {names[buf]} unwritten"
                out.append(y11.POOL)
            if o >= co and o + w <= co + width:
                out.append(name)
            elif (co, width) == (o + w // 2, w // 2):
                out.append(name + y11.HALF)
            elif (co, width) == (o, w // 2):
                out.append(name + y11.FIRST)
            else:
                raise AssertionError(f"{who}: reads [{co}, {co + width}) of {name}'s [{o}, {o + w})")
            at = min(o + w, co + width)
        if at < co + width:
            assert names[buf] == "SP", f"{who}: channels [{at}, {co + width}) of {names[buf]} unwritten"
            out.append(y11.POOL)
        return out

    got = {}
    for r in ins.recs:
        (ci_, inb, incs, inco, Hin, Win, Ho, Wo, o0, o0cs, o0co, up0, o1, o1cs, o1co, up1,
         rb, rcs, rco, in_up, in2b, in2cs, in2co, split) = r.tolist()
        name, cin, cout = specs[ci_][:3]
        if name in f.dw and split > 0:  # the group form: v of a qkv map
            assert name.endswith(".attn.pe") and (split, in2cs, inco) == (64, 128, 64)
            (o, w, wcs, src, ho, wo), = writes[inb]
            assert (o, w, wcs, ho, wo) == (0, 2 * cin, incs, Hin, Win) and src == qkv_of[inb]
            srcs = [(src + y11.V, False)]
        elif in2b >= 0:
            h1, w1 = (Hin // 2, Win // 2) if in_up else (Hin, Win)
            srcs = [(p, bool(in_up)) for p in cover(inb, inco, split, incs, h1, w1, name)]
            srcs += [(p, False) for p in cover(in2b, in2co, cin - split, in2cs, Hin, Win, name)]
        else:
            assert not in_up
            srcs = [(p, False) for p in cover(inb, inco, cin, incs, Hin, Win, name)]
        res = None
        if rb >= 0:
            rs = cover(rb, rco, cout, rcs, Ho, Wo, name + " (residual)")
            assert len(rs) == 1
            res = rs[0]
        assert name not in got
        got[name] = (srcs, res)
    for an, (qb, qcs, qco, heads, H, W, ob, ocs, oco) in zip(attn_names, f.attn.tolist()):
        got[an] = ([(p, False) for p in cover(qb, qco, 128 * heads, qcs, H, W, an)], None)
    return got


def test_wiring_is_the_yolo11_graph(plan):
    f = plan.forward()
    names = [n for n, *_ in f.eng.buffers(plan.B)]
    got = resolve_producers(f, names)
    want = y11.expected_producers(plan.variant)
    assert want.pop("model.0") == ([("input", False)], None)
    assert set(got) == set(want)
    for n in want:
        assert got[n] == want[n], f"{n}: reads {got[n]}, the graph says {want[n]}"
    # both Upsample + Concat pairs are virtual inputs of the conv that reads them
    for n in ("model.13.cv1", "model.16.cv1"):
        assert [u for _, u in got[n][0]] == [True, False], n
    assert sum(u for srcs, _ in got.values() for _, u in srcs) == 2


def test_sppf_decode_and_candidates(plan):
    tv.test_sppf_decode_and_candidates(plan)


def _launch_kinds(f):
    """The launch list of the traced forward, in launch order: one launch per
    conv record that writes a map (the head's last 1x1 stage runs inside the
    decode), plus the attention launch right behind its qkv conv."""
    kinds = []
    for r in f.ins.recs:
        name = f.specs[r[0]][0]
        if f.ins.bufs[r[8]][3]:
            continue
        kinds.append(("dw" if name in f.dw else "conv", name, r))
        if name.endswith(".attn.qkv"):
            kinds.append(("attn", name[:-len(".qkv")], None))
    return kinds


def test_production_launches_match_one_launch_per_op(plan, cuda):
    """The default launch list against the one-launch-per-op list (every
    fusing option off): raw prediction, candidate counts and candidate rows
    bit-identical, and -- no YOLO11 launch is fused -- the same launch list."""
    eng, lb = tv._engine(cuda, plan)
    B = plan.B
    eng.set_raw_fused(True)
    res, launches = [], []
    for slot in (0, 1):
        if slot == 1:
            eng.set_fuse_c2f(0)
            eng.set_fuse_cv1(False)
            eng.set_head_sparse(0)
        raw = torch.full((B, 4 + NC, eng.A), float("nan"), dtype=torch.float32, device=cuda)
        eng.seg_n[slot].fill_(-7)
        eng.forward_raw(lb, raw, slot=slot)
        torch.cuda.synchronize()
        assert eng.head_form() == 1  # raw_out: never the sparse form 3
        res.append((raw.cpu().numpy(),) + tv._candidate_rows(eng, slot, B))
        launches.append(tv._zero_candidate_launches(eng))
    kinds = _launch_kinds(plan.forward())
    others = sum(k != "conv" for k, _, _ in kinds)
    assert launches[0] == launches[1] == (others, len(kinds)), (launches, others, len(kinds))
    (r0, s0, c0), (r1, s1, c1) = res
    assert np.isfinite(r0).all() and (s0 >= 0).all() and s0.sum() > 0
    np.testing.assert_array_equal(r0, r1)
    np.testing.assert_array_equal(s0, s1)
    for a, b in zip(c0, c1):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(r0, plan.forward().raw)  # and the traced forward's
    # sparse asked for, candidates only: still the dense head (forms 1 / 2)
    eng.set_head_sparse(1)
    eng.forward_raw(lb, None, slot=1)
    torch.cuda.synchronize()
    assert eng.head_form() == (2 if plan.variant == 20 else 1)  # form 2: 64-wide box, 80-wide class branch
    s2, c2 = tv._candidate_rows(eng, 1, B)
    np.testing.assert_array_equal(s2, s0)
    for a, b in zip(c2, c0):
        np.testing.assert_array_equal(a, b)
    eng.close()


def test_every_tile_configuration_is_bit_identical(plan, cuda):
    tv.test_every_tile_configuration_is_bit_identical(plan, cuda)


def test_no_dense_conv_falls_back_to_the_generic_kernel(plan):
    """Every dense conv launch has at least one patch / direct configuration
    (no exemptions: the 8-channel convs of YOLO11n's model.2 included); the
    depthwise and attention launches, which the conv launcher never sees,
    report none and keep their launch index."""
    f = plan.forward()
    lib, h = f.ins.lib, f.eng._h
    kinds = _launch_kinds(f)
    assert len(kinds) == len(f.ins.recs) - 6 + len(f.attn)
    assert lib.rv_yolo_conv_candidates(h, len(kinds), None, 0) < 0  # one past the last launch
    missing = []
    for idx, (kind, name, r) in enumerate(kinds):
        n = lib.rv_yolo_conv_candidates(h, idx, None, 0)
        if kind != "conv":
            assert n == 0, (name, n)
        elif n <= 0 and r[20] < 0:
            missing.append((name, r[4:8].tolist()))
    assert not missing, f"no kernel configuration (generic fallback): {missing}"


@pytest.mark.parametrize("nc,form", [(1, 2), (70, 1), (128, 1)])
def test_custom_class_counts_on_yolo11n(cuda, nc, form):
    """nc = 1 (c3d 64), 70 (c3d 70 run 72 wide) and 128 (c3d 100 run 104 wide):
    layer-wise, zero padding channels (the second depthwise conv's included),
    decode from the GPU's own logits, candidates, and the decode form of the
    forward without raw."""
    H, W, B = 64, 96, 2
    flat, fr, _ = y11.synth_case(20, H, W, B, nc=nc)
    f = _forward(cuda, 20, flat, fr, B, H, W, nc)
    eng, ins, raw = f.eng, f.ins, f.raw
    assert eng.nc == nc and len(ins.recs) == len(f.specs) - 1
    _check_model0(f)
    check_every_conv(_dense_only(f), f.specs, f.params)
    assert check_every_depthwise(f) == 7
    assert check_every_attention(f, B)[0] == 1
    dims = {n: (ci, co) for n, ci, co, *_ in f.specs}
    c2d, c3d = dims["model.23.cv2.0.0"][1], dims["model.23.cv3.0.0.1"][1]
    assert (c2d, c3d) == (64, y11.N_TOTALS[nc][1])
    c3p, hcs = (c3d + 7) // 8 * 8, (4 * REG + nc + 3) // 4 * 4
    names, padded = [], 0
    for i, (name, bh, bw, C, es, off) in enumerate(eng.buffers(B)):
        names.append(name)
        if name[:2] in ("DA", "DB"):
            assert (C, es) == (c2d + c3p, 2), name
            pad = ins.raw_u16(i)[..., c2d + c3d:]
        elif name[:2] == "DW" and name[-1] == "b":
            assert (C, es) == (c3p, 2), name
            pad = ins.raw_u16(i)[..., c3d:]
        elif name[:2] == "HD":
            assert (C, es) == (hcs, 4), name
            pad = ins.view(i)[..., 4 * REG + nc:].view(np.uint32)
        else:
            continue
        padded += pad.size
        assert not pad.any(), f"{name}: padding channels not zero"
    assert (padded > 0) == (c3p != c3d or hcs != 4 * REG + nc)
    outs, anc, st = [], [], []
    for lvl in range(3):
        v = ins.view(names.index(f"HD{lvl}"))[..., :4 * REG + nc]
        h, w = v.shape[1:3]
        assert v.dtype == np.float32 and (h, w) == (H // (8 << lvl), W // (8 << lvl))
        outs.append(v.reshape(B, h * w, -1).transpose(0, 2, 1))
        sy, sx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        anc.append(np.stack([sx.ravel(), sy.ravel()]))
        st.append(np.full(h * w, 8.0 * 2 ** lvl))
    y = np.concatenate(outs, 2).astype(np.float64)
    A = y.shape[2]
    assert A == eng.A and raw.shape == (B, 4 + nc, A) and np.isfinite(raw).all()
    box = y[:, :4 * REG].reshape(B, 4, REG, A)
    e = np.exp(box - box.max(2, keepdims=True))
    dist = (e / e.sum(2, keepdims=True) * np.arange(REG).reshape(1, 1, REG, 1)).sum(2)
    an = np.concatenate(anc, 1)[None]
    s_ = np.concatenate(st)[None]
    x1y1, x2y2 = an - dist[:, :2], an + dist[:, 2:]
    xywh = np.concatenate([(x1y1 + x2y2) / 2, x2y2 - x1y1], 1) * s_[:, None]
    np.testing.assert_allclose(raw[:, :4], xywh, rtol=0, atol=2e-3)
    np.testing.assert_allclose(raw[:, 4:], 1 / (1 + np.exp(-y[:, 4 * REG:])), rtol=0, atol=1e-6)
    seg = eng.seg_n[0].view(-1)[:B * eng.nseg].view(B, eng.nseg).cpu().numpy()
    expect = (raw[:, 4:].max(1) > 0.25).sum(1)
    print(f"YOLO11n nc {nc}: candidates {expect.tolist()} of {A} anchors")
    np.testing.assert_array_equal(seg.sum(1), expect)
    assert 0 < expect.sum() < B * A
    # without raw: the fixed decode forms, the same candidates
    lb = torch.from_numpy(f.lb).to(cuda)
    eng.seg_n[1].fill_(-7)
    eng.forward_raw(lb, None, slot=1)
    torch.cuda.synchronize()
    assert eng.head_form() == form
    seg1 = eng.seg_n[1].view(-1)[:B * eng.nseg].view(B, eng.nseg).cpu().numpy()
    np.testing.assert_array_equal(seg1, seg)
    eng.close()


def _npz_state_dict(path, variant, flat):
    np.savez(path, **y11.state_dict(variant, flat, fused=True, nested=True))
    return path


def _rows(dets):
    return np.array([[d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id] for d in dets],
                    np.float32).reshape(-1, 6)


def test_detector_from_a_state_dict_file(cuda, tmp_path):
    """build_detector with detect.model yolo11n.pt and an .npz state_dict on a
    480x640 road frame: Detections, bit for bit yolo_ref.postprocess of the
    GPU's own raw prediction."""
    from rvs_amd.detect.registry import build_detector
    from rvs_amd.detect.types import Detection
    H, W = 480, 640
    flat, fr, _ = y11.synth_case(20, H, W, 1)
    path = _npz_state_dict(str(tmp_path / "yolo11n.npz"), 20, flat)
    det = build_detector({"backend": "hip", "model": "yolo11n.pt", "weights": path, "imgsz": 640,
                          "classes_keep": []})
    assert det.variant == 20 and det.nc == 80
    np.testing.assert_array_equal(det.flat, flat)
    out = det.infer(fr[0])
    assert len(out) > 0 and all(isinstance(d, Detection) for d in out)
    eng = det.engine(H, W)
    eng.set_raw_fused(True)
    raw = torch.full((1, 84, eng.A), float("nan"), dtype=torch.float32, device=cuda)
    eng.forward_raw(eng.letterbox(torch.from_numpy(fr.copy()).to(cuda)), raw, candidates=False)
    ref = yolo_ref.postprocess(raw.cpu().numpy(), (eng.in_h, eng.in_w), (H, W))
    np.testing.assert_array_equal(_rows(out), ref[0])
    det.close()


def test_pipelined_engine_matches_the_standalone_detector(cuda, tmp_path):
    """A two-stream engine at 160x224 with detect.model yolo11n.pt: a plain
    step and two pipelined steps (forward parts 3, 4 and 2 on two lanes) hand
    back the detections the standalone detector gives on the same preprocessed
    frames (the comparison of tests/test_engine_gpu.py: the row values)."""
    from rvs_amd.config import load_config
    from rvs_amd.detect.yolo_hip import YOLOHip
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.schedule import PipelinedRun
    S, H, W = 2, 160, 224
    flat, proc_ref, _ = y11.synth_case(20, H, W, S)
    path = _npz_state_dict(str(tmp_path / "yolo11n.npz"), 20, flat)
    cfg = load_config()
    cfg["detect"].update(enabled=True, model="yolo11n.pt", weights=path, imgsz=max(H, W))
    frames = torch.from_numpy(np.stack([road_frame(H, W, seed=30 + b) for b in range(S)])).to(cuda)
    ts = [torch.full((S,), f / 30.0, dtype=torch.float64, device=cuda) for f in range(3)]
    det = YOLOHip(dict(cfg["detect"]))
    seq = RoadVisionEngine(cfg, S, (H, W), device=cuda)
    assert seq.variant == 20
    out = seq.step(frames, ts[0])
    np.testing.assert_array_equal(out["proc"].cpu().numpy(), proc_ref)  # yolo_synth.frames
    want = [_rows(d) for d in det.infer_batch(out["proc"])]
    assert sum(len(w) for w in want) > 0
    for s, dets in enumerate(seq.results(out)):
        np.testing.assert_array_equal(_rows(dets), want[s])
    pip = RoadVisionEngine(cfg, S, (H, W), device=cuda, lanes=2, pair=1)
    pip.step(frames, ts[0])
    run = PipelinedRun(pip, [frames, frames], ts[1:])
    run.run()
    torch.cuda.synchronize()
    assert len(run.outs) == 2
    for o in run.outs:
        for s, dets in enumerate(pip.results(o)):
            np.testing.assert_array_equal(_rows(dets), want[s])
    run.close()
    for e in (seq, pip):
        e.close()
    det.close()

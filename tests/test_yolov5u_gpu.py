"""The YOLOv5u plans (variants 5..9: n, s, m, l, x) on the GPU, modelled on
tests/test_yolo_variants_gpu.py, whose helpers and assertions this file uses.

Geometry: 160x224 batch 2 and 64x96 batch 1 (P5 = 5x7 and 2x3).  Weights:
tests/yolov5u_ref.py's one-pass normalisation on the case's own letterbox.

Per case: every conv in float64 from the GPU's own inputs (check_every_conv,
unchanged bars; model.0 against the float64 k6 s2 p2 conv); the WIRING -- each
conv's input and residual views resolved, through the trace records, to the
convs that wrote those channel slices, equal to the graph
yolov5u_ref.expected_producers states; SPPF pools exact, decode from the GPU's
own logits, candidate counts from raw; the production launch list
bit-identical to one launch per conv; every tile configuration bit-identical
under autotune verify; no conv launch without a patch / direct configuration.
Then class counts 3 and 70 on YOLOv5nu, the detector from an .npz state_dict,
and the pipelined engine.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_yolo_variants_gpu as tv
import yolo_synth
import yolov5u_ref as v5
from conftest import road_frame
from oracle import yolo_ref
from test_yolo_layers_gpu import Introspect, check_every_conv, ulp_bf16

pytestmark = pytest.mark.gpu

CASES = [(v, H, W, B) for v in (5, 6, 7, 8, 9) for H, W, B in tv.GEOMETRIES]
NC, REG = 80, 16


def _forward(cuda, variant, flat, frames, B, H, W, nc):
    from rvs_amd.detect.yolo_hip import YoloEngine
    eng = YoloEngine(variant, flat, B, (H, W), imgsz=max(H, W), device=cuda, nc=nc)
    assert (eng.in_h, eng.in_w) == (H, W)
    lb = eng.letterbox(torch.from_numpy(frames.copy()).to(cuda))
    raw = torch.full((B, 4 + nc, eng.A), float("nan"), dtype=torch.float32, device=cuda)
    eng.forward_raw(lb, raw)
    ins = Introspect(eng, B)
    specs, params = v5.split_params(variant, flat, nc)
    return types.SimpleNamespace(eng=eng, ins=ins, specs=specs, params=params,
                                 lb=lb.cpu().numpy(), raw=raw.cpu().numpy())


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "v%d-%dx%d-b%d" % c)
def plan(request, cuda):
    """One case: its weights and frames, and (lazily, shared by the tests that
    only read it) the default raw forward with every activation kept."""
    variant, H, W, B = request.param
    flat, fr, _ = v5.synth_case(variant, H, W, B)
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
    """model.0: k6 s2 p2 from the u8 letterbox, its own kernel outside the trace."""
    w, b = f.params["model.0"]
    x = torch.from_numpy(f.lb[..., ::-1].transpose(0, 3, 1, 2).copy()).double() / 255
    y = F.silu(F.conv2d(x, torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=2,
                        padding=2)).numpy().transpose(0, 2, 3, 1)
    got = f.ins.view(0)
    assert got.shape == y.shape
    d = np.abs(got - y)
    assert (d <= ulp_bf16(y) * 1.01 + 1e-6).mean() > 0.9999 and (d <= 2 * ulp_bf16(y) + 1e-5).all()


def test_every_conv_layerwise(plan):
    f = plan.forward()
    assert len(f.ins.recs) == len(f.specs) - 1  # every conv but model.0
    assert np.isfinite(f.raw).all()
    _check_model0(f)
    worst = check_every_conv(f.ins, f.specs, f.params)
    print(f"variant {plan.variant} {plan.H}x{plan.W} B={plan.B} worst layers: {worst}")


def resolve_producers(ins, specs, names):
    """{conv name: ([(producer, upsampled?)], residual producer)} from the
    trace records: every view a conv reads is matched, channel by channel,
    with the conv output views (same buffer, same pixel stride, same map size)
    that cover it.  Channels no conv writes are SPPF's pools (buffer SP only);
    buffer 0 (X0) is model.0's, which has no record."""
    writes = {}  # buffer -> [(channel offset, width, pixel stride, producer, Ho, Wo)]
    c0 = specs[0][2]
    writes[0] = [(0, c0, c0, specs[0][0], ins.bufs[0][0], ins.bufs[0][1])]
    for r in ins.recs:
        name, cout = specs[r[0]][0], specs[r[0]][2]
        Ho, Wo = int(r[6]), int(r[7])
        for ob, ocs, oco, up in ((r[8], r[9], r[10], r[11]), (r[12], r[13], r[14], r[15])):
            if ob >= 0:
                assert not up, f"{name}: no YOLOv5u conv writes an upsampled copy"
                writes.setdefault(int(ob), []).append((int(oco), cout, int(ocs), name, Ho, Wo))
    for b, ws in writes.items():  # nothing overwritten inside a forward
        ws.sort()
        for a, c in zip(ws, ws[1:]):
            assert a[0] + a[1] <= c[0], f"buffer {names[b]}: {a[3]} and {c[3]} overlap"

    def cover(buf, co, width, cs, H, W, who):
        out, at = [], co
        for (o, w, wcs, name, Ho, Wo) in writes.get(int(buf), []):
            if o + w <= co or o >= co + width:
                continue
            assert o >= co and o + w <= co + width, f"{who}: reads part of {name}'s output"
            assert wcs == cs, f"{who}: pixel stride {cs} but {name} wrote with {wcs}"
            assert (Ho, Wo) == (H, W), f"{who}: map {H}x{W} but {name} wrote {Ho}x{Wo}"
            if o > at:
                assert names[buf] == "SP", f"{who}: channels [{at}, {o}) of {names[buf]} unwritten"
                out.append(v5.POOL)
            out.append(name)
            at = o + w
        if at < co + width:
            assert names[buf] == "SP", f"{who}: channels [{at}, {co + width}) of {names[buf]} unwritten"
            out.append(v5.POOL)
        return out

    got = {}
    for r in ins.recs:
        (ci_, inb, incs, inco, Hin, Win, Ho, Wo, o0, o0cs, o0co, up0, o1, o1cs, o1co, up1,
         rb, rcs, rco, in_up, in2b, in2cs, in2co, split) = r.tolist()
        name, cin, cout = specs[ci_][:3]
        if in2b >= 0:
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
    return got


def test_wiring_is_the_yolov5_graph(plan):
    f = plan.forward()
    names = [n for n, *_ in f.eng.buffers(plan.B)]
    got = resolve_producers(f.ins, f.specs, names)
    want = v5.expected_producers(plan.variant)
    assert want.pop("model.0") == ([("input", False)], None)
    assert set(got) == set(want)
    for n in want:
        assert got[n] == want[n], f"{n}: reads {got[n]}, the graph says {want[n]}"
    # both Upsample + Concat pairs are virtual inputs of the two convs that read them
    for n in ("model.13.cv1", "model.13.cv2", "model.17.cv1", "model.17.cv2"):
        assert [u for _, u in got[n][0]] == [True, False], n
    assert sum(u for srcs, _ in got.values() for _, u in srcs) == 4


def test_sppf_decode_and_candidates(plan):
    tv.test_sppf_decode_and_candidates(plan)


def test_production_launches_match_one_launch_per_conv(plan, cuda):
    tv.test_production_launches_match_one_launch_per_conv(plan, cuda)


def test_every_tile_configuration_is_bit_identical(plan, cuda):
    tv.test_every_tile_configuration_is_bit_identical(plan, cuda)


def test_no_conv_falls_back_to_the_generic_kernel(plan):
    """As tests/test_yolo_variants_gpu.py: every conv launch has at least one
    patch / direct configuration; no exemptions for any YOLOv5u variant."""
    f = plan.forward()
    lib, h = f.ins.lib, f.eng._h
    launched = [r for r in f.ins.recs if not f.ins.bufs[r[8]][3]]
    assert len(launched) == len(f.ins.recs) - 6
    assert lib.rv_yolo_conv_candidates(h, len(launched), None, 0) < 0  # one past the last launch
    missing = []
    for idx, r in enumerate(launched):
        n = lib.rv_yolo_conv_candidates(h, idx, None, 0)
        assert n >= 0
        if n == 0 and r[20] < 0:
            missing.append((f.specs[r[0]][0], r[4:8].tolist()))
    assert not missing, f"no kernel configuration (generic fallback): {missing}"


@pytest.mark.parametrize("nc,form", [(3, 2), (70, 1)])
def test_custom_class_counts_on_yolov5nu(cuda, nc, form):
    """nc = 3 (one class fragment) and nc = 70 (c3d = 70 run 72 wide) as
    tests/test_nc_gpu.py checks them for YOLOv8n: layer-wise, zero padding
    channels, decode from the GPU's own logits, candidates, and the decode
    form of the forward without raw."""
    H, W, B = 64, 96, 1
    flat, fr, _ = v5.synth_case(5, H, W, B, nc=nc)
    f = _forward(cuda, 5, flat, fr, B, H, W, nc)
    eng, ins, raw = f.eng, f.ins, f.raw
    assert eng.nc == nc and len(ins.recs) == len(f.specs) - 1
    _check_model0(f)
    check_every_conv(ins, f.specs, f.params)
    dims = {n: (ci, co) for n, ci, co, *_ in f.specs}
    c2d, c3d = dims["model.24.cv2.0.0"][1], dims["model.24.cv3.0.0"][1]
    assert (c2d, c3d) == (64, max(64, min(nc, 100)))
    c3p, hcs = (c3d + 7) // 8 * 8, (4 * REG + nc + 3) // 4 * 4
    names, padded = [], 0
    for i, (name, bh, bw, C, es, off) in enumerate(eng.buffers(B)):
        names.append(name)
        if name[:2] in ("DA", "DB"):
            assert (C, es) == (c2d + c3p, 2), name
            pad = ins.raw_u16(i)[..., c2d + c3d:]
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
    print(f"YOLOv5nu nc {nc}: candidates {expect.tolist()} of {A} anchors")
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
    sd = v5.state_dict(variant, flat, fused=True, nested=True)
    np.savez(path, **sd)
    return path


def _rows(dets):
    return np.array([[d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id] for d in dets],
                    np.float32).reshape(-1, 6)


def test_detector_from_a_state_dict_file(cuda, tmp_path):
    """build_detector with detect.model yolov5n.pt and an .npz state_dict on a
    480x640 road frame: Detections, bit for bit yolo_ref.postprocess of the
    GPU's own raw prediction."""
    from rvs_amd.detect.registry import build_detector
    from rvs_amd.detect.types import Detection
    H, W = 480, 640
    flat, fr, _ = v5.synth_case(5, H, W, 1)
    path = _npz_state_dict(str(tmp_path / "yolov5nu.npz"), 5, flat)
    det = build_detector({"backend": "hip", "model": "yolov5n.pt", "weights": path, "imgsz": 640,
                          "classes_keep": []})
    assert det.variant == 5 and det.nc == 80
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
    """A two-stream engine at 160x224 with detect.model yolov5nu.pt: a plain
    step and two pipelined steps (forward parts 3, 4 and 2 on two lanes) hand
    back the detections the standalone detector gives on the same preprocessed
    frames (the comparison of tests/test_engine_gpu.py: the row values)."""
    from rvs_amd.config import load_config
    from rvs_amd.detect.yolo_hip import YOLOHip
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.schedule import PipelinedRun
    S, H, W = 2, 160, 224
    flat, proc_ref, _ = v5.synth_case(5, H, W, S)
    path = _npz_state_dict(str(tmp_path / "yolov5nu.npz"), 5, flat)
    cfg = load_config()
    cfg["detect"].update(enabled=True, model="yolov5nu.pt", weights=path, imgsz=max(H, W))
    frames = torch.from_numpy(np.stack([road_frame(H, W, seed=30 + b) for b in range(S)])).to(cuda)
    ts = [torch.full((S,), f / 30.0, dtype=torch.float64, device=cuda) for f in range(3)]
    det = YOLOHip(dict(cfg["detect"]))
    seq = RoadVisionEngine(cfg, S, (H, W), device=cuda)
    assert seq.variant == 5
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

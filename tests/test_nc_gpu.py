"""YOLOv8 plans with a custom class count on the GPU, layer by layer.

Geometries as in test_yolo_variants_gpu.py (160x224 batch 2, 64x96 batch 1:
every tile tail occurs).  Weights: tests/yolo_synth.py's one-pass
normalisation over the conv list of tests/yolo_nc.py, the road-class prior on
the road ids below nc; the quantile shift puts about 4 % of the anchors above
conf on the f32 oracle for every nc (printed per case).

Bars (test_yolo_layers_gpu.check_every_conv / test_yolo_variants_gpu.py):
bf16 maps 1.01 ulp + 1e-3 RMS for all but < 1e-4 of the elements, none beyond
2 ulp + 1e-2 RMS; f32 head logits 1e-4 RMS + 1e-5 |ref|; decoded xywh 2e-3 px,
scores 1e-6; everything else bit for bit.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import yolo_nc
import yolo_synth
from oracle import yolo_ref
from test_yolo_layers_gpu import Introspect, _zero_candidate_launches, check_every_conv

pytestmark = pytest.mark.gpu

REG, CONF = 16, 0.25
BIG, SMALL = (160, 224, 2), (64, 96, 1)
# (variant, nc, geometry, decode form of the forward without raw)
CASES = [(0, 1, SMALL, 2),    # one class fragment, logits rows of 65 padded to 68
         (0, 4, BIG, 2),      # the typical fine-tune
         (0, 17, SMALL, 2),   # partial second fragment
         (0, 64, SMALL, 2),   # four full fragments: the last register-resident count
         (0, 70, SMALL, 1),   # c3d = 70 run 72 wide
         (0, 100, BIG, 1),    # c3d = 100 run 104 wide, 7 fragments: the second class pass
         (1, 4, SMALL, 1),    # s: class branch 128 wide
         (1, 100, SMALL, 1),  # second pass on a wide head
         (4, 17, SMALL, 1),   # x: box branch 80 wide
         (0, 128, SMALL, 1)]  # the largest count: 8 fragments, the 49 KB logits tile


def _engine(cuda, p, **kw):
    from rvs_amd.detect.yolo_hip import YoloEngine
    eng = YoloEngine(p.variant, p.flat, p.B, (p.H, p.W), imgsz=max(p.H, p.W), device=cuda, nc=p.nc,
                     **kw)
    assert (eng.in_h, eng.in_w) == (p.H, p.W) and eng.nc == p.nc
    assert eng._h and eng.head_form() == -1
    return eng, eng.letterbox(torch.from_numpy(p.frames.copy()).to(cuda))


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "v%d-nc%d-%dx%d-b%d" % (c[:2] + c[2]))
def plan(request, cuda):
    """One case: weights, frames and (lazily, shared by the tests that only
    read it) the default raw forward with every activation kept."""
    variant, nc, (H, W, B), form = request.param
    with pytest.MonkeyPatch.context() as mp:
        yolo_nc.patched(mp, nc)
        lb = yolo_synth.letterboxed(H, W, B, max(H, W))
        flat = yolo_synth.synth_weights_on(variant, lb)
        _, frac = yolo_synth.oracle_stats(variant, flat, lb)
    print(f"variant {variant} nc {nc} {H}x{W}: f32 oracle, {frac:.4f} of the anchors pass conf")
    assert 0.0 < frac < 1.0
    flat.setflags(write=False)
    p = types.SimpleNamespace(variant=variant, nc=nc, H=H, W=W, B=B, form=form, flat=flat,
                              frames=yolo_synth.frames(H, W, B), fwd=None)

    def forward():
        if p.fwd is None:
            eng, lb_ = _engine(cuda, p)
            raw = torch.full((B, 4 + nc, eng.A), float("nan"), dtype=torch.float32, device=cuda)
            eng.forward_raw(lb_, raw)
            ins = Introspect(eng, B)
            specs, params = yolo_nc.split(variant, nc, flat)
            p.fwd = types.SimpleNamespace(eng=eng, ins=ins, specs=specs, params=params,
                                          raw=raw.cpu().numpy())
        return p.fwd

    p.forward = forward
    yield p
    if p.fwd is not None:
        p.fwd.eng.close()


def _segments(eng, slot, B):
    """(counts (B, nseg), rows (B, cap, 8) as i32 bit patterns) of a candidate slot."""
    seg = eng.seg_n[slot].view(-1)[:B * eng.nseg].view(B, eng.nseg).cpu().numpy().copy()
    return seg, eng.cand[slot][:B].cpu().numpy().view(np.int32).copy()


def _valid_rows(seg, rows):
    return [rows[b, 64 * s:64 * s + int(seg[b, s])] for b in range(seg.shape[0])
            for s in range(seg.shape[1])]


def test_every_conv_and_zero_padding(plan):
    """Every conv in float64 from the GPU's own inputs (state_dict shapes: the
    padding is invisible to them), and every padding channel exactly zero."""
    f = plan.forward()
    assert len(f.ins.recs) == len(f.specs) - 1  # every conv but model.0
    worst = check_every_conv(f.ins, f.specs, f.params)
    print(f"variant {plan.variant} nc {plan.nc}: worst layers {worst}")
    dims = {n: (ci, co) for n, ci, co, *_ in f.specs}
    c2d, c3d = dims["model.22.cv2.0.0"][1], dims["model.22.cv3.0.0"][1]
    assert c3d == yolo_nc.c3d_of(plan.variant, plan.nc)
    c3p, hcs = (c3d + 7) // 8 * 8, (4 * REG + plan.nc + 3) // 4 * 4
    padded = 0
    for i, (name, H, W, C, es, off) in enumerate(f.eng.buffers(plan.B)):
        if name[:2] in ("DA", "DB"):
            assert (C, es) == (c2d + c3p, 2), name
            pad = f.ins.raw_u16(i)[..., c2d + c3d:]
        elif name[:2] == "HD":
            assert (C, es) == (hcs, 4), name
            pad = f.ins.view(i)[..., 4 * REG + plan.nc:].view(np.uint32)
        else:  # nothing else depends on nc
            continue
        padded += pad.size
        assert not pad.any(), f"{name}: padding channels not zero"
    assert (padded > 0) == (c3p != c3d or hcs != 4 * REG + plan.nc)


def test_decode_and_candidates(plan):
    f = plan.forward()
    eng, ins, raw, B, nc = f.eng, f.ins, f.raw, plan.B, plan.nc
    names = [n for n, *_ in eng.buffers(B)]
    outs, anc, st = [], [], []
    for lvl in range(3):
        v = ins.view(names.index(f"HD{lvl}"))[..., :4 * REG + nc]
        h, w = v.shape[1:3]
        assert v.dtype == np.float32 and (h, w) == (plan.H // (8 << lvl), plan.W // (8 << lvl))
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
    seg, rows = _segments(eng, 0, B)
    expect = (raw[:, 4:].max(1) > CONF).sum(1)
    print(f"variant {plan.variant} nc {nc}: candidates {expect.tolist()} of {A} anchors")
    np.testing.assert_array_equal(seg.sum(1), expect)
    assert 0 < expect.sum() < B * A
    best = raw[:, 4:].argmax(1)
    for b in range(B):
        for r in _valid_rows(seg[b:b + 1], rows[b:b + 1]):
            assert ((r[:, 5] >= 0) & (r[:, 5] < nc)).all()
            np.testing.assert_array_equal(r[:, 5], best[b, r[:, 6]])  # the first maximum


def test_candidates_identical_with_and_without_raw(plan, cuda):
    """The production launch list with a raw output (LDS class scan, form 1)
    and without (the case's form): candidate counts, rows and order are the
    same bits, and rv_yolo_head_form tells the two kernels apart."""
    eng, lb = _engine(cuda, plan)
    B = plan.B
    eng.set_raw_fused(True)
    got = []
    for slot, with_raw in ((0, True), (1, False)):
        eng.cand[slot].fill_(float("nan"))
        eng.seg_n[slot].fill_(-7)
        raw = torch.full((B, 4 + plan.nc, eng.A), float("nan"), dtype=torch.float32,
                         device=cuda) if with_raw else None
        eng.forward_raw(lb, raw, slot=slot)
        torch.cuda.synchronize()
        assert eng.head_form() == (1 if with_raw else plan.form)
        got.append(_segments(eng, slot, B))
    (s0, r0), (s1, r1) = got
    assert (s0 >= 0).all() and 0 < s0.sum() < B * eng.A
    np.testing.assert_array_equal(s0, s1)
    for a, b in zip(_valid_rows(s0, r0), _valid_rows(s1, r1)):
        np.testing.assert_array_equal(a, b)
    eng.close()


def test_launch_lists_and_tile_configurations(plan, cuda):
    """The production launch list (fused chains, chained cv1) against one
    launch per conv: raw and candidates bit-identical; no launch of the
    one-per-conv list lacks a patch / direct configuration (none drops to the
    generic kernel); autotune with verify finds every configuration
    bit-identical and the tuned forward reproduces raw."""
    eng, lb = _engine(cuda, plan)
    B = plan.B
    eng.set_raw_fused(True)
    eng.set_c2f_tap_pairs(False)
    res, launches = [], []
    for slot in (0, 1):
        if slot == 1:
            eng.set_fuse_c2f(0)
            eng.set_fuse_cv1(False)
        raw = torch.full((B, 4 + plan.nc, eng.A), float("nan"), dtype=torch.float32, device=cuda)
        eng.seg_n[slot].fill_(-7)
        eng.forward_raw(lb, raw, slot=slot)
        torch.cuda.synchronize()
        res.append((raw.cpu().numpy(),) + _segments(eng, slot, B))
        launches.append(_zero_candidate_launches(eng))
    assert launches[1][0] == 0, launches
    if plan.variant in (0, 1):
        assert launches[0][0] >= 1 and launches[0][1] < launches[1][1], launches
    (r0, s0, c0), (r1, s1, c1) = res
    assert np.isfinite(r0).all() and (s0 >= 0).all() and s0.sum() > 0
    np.testing.assert_array_equal(r0, r1)
    np.testing.assert_array_equal(s0, s1)
    for a, b in zip(_valid_rows(s0, c0), _valid_rows(s1, c1)):
        np.testing.assert_array_equal(a, b)
    assert eng.autotune(lb, reps=1, verify=True) == 0
    cfgs = eng.tuned_configs()
    assert len(cfgs) > 0 and all(c[0] >= 0 for c in cfgs)
    raw2 = torch.full((B, 4 + plan.nc, eng.A), float("nan"), dtype=torch.float32, device=cuda)
    eng.forward_raw(lb, raw2)
    np.testing.assert_array_equal(raw2.cpu().numpy(), r0)
    eng.close()


def test_run_and_nms_equal_the_oracle_postprocess(plan, cuda):
    """engine.run (no raw: the case's decode form) + NMS + class filter against
    yolo_ref.postprocess on the GPU's own raw, bit for bit; classes_keep mixes
    ids below nc, the last id, and ids at and above nc (which never match)."""
    nc = plan.nc
    keep = sorted({0, 2, nc - 1, nc, nc + 3, 127})
    eng, lb = _engine(cuda, plan, classes_keep=keep)
    eng.set_raw_fused(True)
    raw = torch.full((plan.B, 4 + nc, eng.A), float("nan"), dtype=torch.float32, device=cuda)
    eng.forward_raw(lb, raw, slot=1)
    raw = raw.cpu().numpy()
    dets, n = eng.run(torch.from_numpy(plan.frames.copy()).to(cuda))
    assert eng.head_form() == plan.form
    dets, n = dets.cpu().numpy(), n.cpu().numpy()
    total = 0
    for kp in (keep, ()):
        ref = yolo_ref.postprocess(raw, (eng.in_h, eng.in_w), (plan.H, plan.W), classes_keep=kp)
        if kp == ():
            e2, _ = _engine(cuda, plan)
            dets, n = e2.run(torch.from_numpy(plan.frames.copy()).to(cuda))
            dets, n = dets.cpu().numpy(), n.cpu().numpy()
            e2.close()
        for b in range(plan.B):
            np.testing.assert_array_equal(dets[b, :n[b]], ref[b])
            assert (ref[b][:, 5] < nc).all()
            total += len(ref[b])
    assert total > 0
    eng.close()


def test_detector_and_engine_carry_names(cuda, tmp_path):
    """YOLOv8n with 4 classes from a state_dict file named in detect.weights:
    YOLOHip.infer returns Detections named from detect.names, and a two-stream
    RoadVisionEngine step gives the same lists through the host record and
    through the device tensors."""
    from rvs_amd.config import load_config
    from rvs_amd.detect.yolo_hip import YOLOHip
    from rvs_amd.engine import RoadVisionEngine
    variant, nc, (H, W, B) = 0, 4, BIG
    with pytest.MonkeyPatch.context() as mp:
        yolo_nc.patched(mp, nc)
        flat = yolo_synth.synth_weights_on(variant, yolo_synth.letterboxed(H, W, B, max(H, W)))
    specs, params = yolo_nc.split(variant, nc, flat)
    sd = {}
    for n, ci, co, k, s, act in specs:
        sd["model." + n + (".conv.weight" if act else ".weight")] = params[n][0]
        sd["model." + n + (".conv.bias" if act else ".bias")] = params[n][1]
    path = str(tmp_path / "yolov8n_4cls.npz")
    np.savez(path, **sd)
    names = {0: "car", 1: "truck", 2: "bus", 3: "person"}
    frames = yolo_synth.frames(H, W, B)
    det = YOLOHip({"model": "yolov8n.pt", "weights": path, "names": names, "imgsz": max(H, W),
                   "classes_keep": []})
    assert det.nc == nc and det.names == [names[k] for k in range(nc)]
    np.testing.assert_array_equal(det.flat, flat)
    out = det.infer(frames[0])
    assert len(out) > 0 and all(0 <= d.cls_id < nc and d.cls_name == names[d.cls_id] for d in out)
    assert det.engine(H, W).head_form() == 2
    batch = det.infer_batch(torch.from_numpy(frames.copy()).to(cuda))
    assert len(batch) == B and len(batch[0]) > 0
    assert all(d.cls_name == names[d.cls_id] for lst in batch for d in lst)
    det.close()
    cfg = load_config()
    cfg["detect"].update(enabled=True, model="yolov8n.pt", weights=path, names=names,
                         imgsz=max(H, W), classes_keep=[0, 2, 3, 5, 7])
    eng = RoadVisionEngine(cfg, B, (H, W), device=cuda)
    assert eng.nc == nc and eng.detector.nc == nc and eng.names == [names[k] for k in range(nc)]
    fr = torch.from_numpy(frames.copy()).to(cuda)
    for f in range(2):
        step = eng.step(fr, torch.full((B,), f / 30.0, dtype=torch.float64, device=cuda))
    a = eng.results(step)
    b = eng.results({k: v for k, v in step.items() if k != "record"})
    key = lambda r: [[(d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id, d.cls_name, d.track_id,  # noqa
                       d.distance_m, d.speed_kmh) for d in s] for s in r]
    assert key(a) == key(b) and sum(len(s) for s in a) > 0
    assert all(d.cls_id in (0, 2, 3) and d.cls_name == names[d.cls_id] for s in a for d in s)
    eng.close()


def test_fp8_with_a_custom_class_count_is_refused(cuda):
    from rvs_amd import _lib
    lib = _lib.load()
    packed = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    h = ctypes.c_void_p()
    st = lib.rv_yolo_create3(0, 1, 4, _lib.ptr(packed), 1, 64, 96, ctypes.byref(h))
    assert st == -1000 and not h
    msg = lib.rv_last_error().decode()
    assert "fp8" in msg and "nc = 80 only" in msg and "nc = 4" in msg

"""Live conv profiling (rv_yolo_profile*): slots, FLOP counts, byte counts,
event intervals, reps and switching off.

YOLOv8n bf16 at 64x96, batch 1 (the small geometry of
test_yolo_variants_gpu.py).  A raw forward with default options runs every
conv but model.0 as its own launch, so launch index i is profile slot i; a
candidate forward runs the fused stem (slot num_convs - 1, conv 0), the
chained model.3 + model.4.cv1 and the fused model.2 chain, so a slot covers
several convs and only the FLOP total is pinned.  FLOP counts are integers
below 2^53, hence compared exactly.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import yolo_synth

pytestmark = pytest.mark.gpu

VARIANT, H, W, B = 0, 64, 96, 1


@pytest.fixture(scope="module")
def ctx(cuda):
    from rvs_amd import _lib
    from rvs_amd.detect.yolo_hip import YoloEngine
    flat, fr = yolo_synth.synth_case(VARIANT, H, W, B, max(H, W))
    eng = YoloEngine(VARIANT, flat, B, (H, W), imgsz=max(H, W), device=cuda)
    assert (eng.in_h, eng.in_w) == (H, W)
    lib = _lib.load()
    nconv = lib.rv_yolo_num_convs(VARIANT)
    specs = []
    for i in range(nconv):
        info = (ctypes.c_int * 5)()
        name = ctypes.create_string_buffer(64)
        assert lib.rv_yolo_conv_info(VARIANT, i, info, name, 64) == 0
        specs.append((name.value.decode(),) + tuple(info))  # name, cin, cout, k, s, act
    c = types.SimpleNamespace(eng=eng, lib=lib, h=eng._h, nconv=nconv, specs=specs,
                              lb=eng.letterbox(torch.from_numpy(fr.copy()).to(cuda)))
    c.raw = lambda: torch.full((B, 84, eng.A), float("nan"), dtype=torch.float32, device=cuda)
    yield c
    eng.close()


def _trace(c):
    n = c.lib.rv_yolo_trace(c.h, None, 0)
    recs = np.zeros(n * 24, np.int32)
    c.lib.rv_yolo_trace(c.h, recs.ctypes.data, n)
    return recs.reshape(n, 24)


def _read(c):
    """(recorded forwards, ms, flops, conv, bytes), one entry per slot."""
    n = c.nconv
    ms, fl, by = np.full(n, -1.0), np.full(n, -1.0), np.full(n, -1.0)
    cv = np.full(n, -2, np.int32)
    nf = c.lib.rv_yolo_profile_read(c.h, ms.ctypes.data, fl.ctypes.data, cv.ctypes.data, n)
    if nf > 0:
        assert c.lib.rv_yolo_profile_bytes(c.h, by.ctypes.data, n) == n
    return nf, ms, fl, cv, by


def _flops(c, idx, Ho, Wo):
    _, cin, cout, k, _, _ = c.specs[idx]
    return 2 * B * Ho * Wo * cout * cin * k * k


def _raw_forwards(c, n_fwd, reps):
    assert c.lib.rv_yolo_profile_reps(c.h, n_fwd, reps) == 0
    raw = c.raw()
    for _ in range(n_fwd):
        c.eng.forward_raw(c.lb, raw, candidates=False)
    torch.cuda.synchronize()
    return raw.cpu().numpy()


def test_raw_forward_one_slot_per_launch(ctx):
    c = ctx
    _raw_forwards(c, 2, 1)
    nf, ms, fl, cv, by = _read(c)
    assert nf == 2
    recs = _trace(c)
    assert len(recs) == c.nconv - 1  # every conv but model.0
    rec_of = {int(r[0]): r for r in recs}
    slots = np.flatnonzero(cv >= 0)
    # the six Detect .2 stages are traced but run inside the decode
    assert len(slots) == len(recs) - 6
    assert sorted(cv[slots].tolist()) == sorted(
        i for i in range(1, c.nconv)
        if not (c.specs[i][0].startswith("model.22.") and c.specs[i][0].endswith(".2")))
    for i in slots:
        r = rec_of[int(cv[i])]
        assert fl[i] == _flops(c, int(cv[i]), int(r[6]), int(r[7])), c.specs[cv[i]][0]
        assert ms[i] > 0 and by[i] > 0, c.specs[cv[i]][0]


def test_candidate_forward_stem_slot_flops_and_intervals(ctx):
    c = ctx
    n_fwd = 2
    assert c.lib.rv_yolo_profile_reps(c.h, n_fwd, 1) == 0
    for _ in range(n_fwd):
        c.eng.forward_raw(c.lb)
    torch.cuda.synchronize()
    nf, ms, fl, cv, by = _read(c)
    assert nf == n_fwd
    slots = np.flatnonzero(cv >= 0)
    assert cv[c.nconv - 1] == 0  # the fused stem: last slot, conv 0
    assert len(slots) < c.nconv - 6  # fused launches: fewer slots than convs
    assert (ms[slots] > 0).all() and (by[slots] > 0).all()
    c1 = c.specs[0][2]
    want = 2 * B * (H // 2) * (W // 2) * c1 * 27
    rec_of = {int(r[0]): r for r in _trace(c)}
    for i in range(1, c.nconv):
        n = c.specs[i][0]
        if n.startswith("model.22.") and n.endswith(".2"):
            continue
        want += _flops(c, i, int(rec_of[i][6]), int(rec_of[i][7]))
    assert fl[slots].sum() == want
    # intervals: forward by forward, slot by slot; the stem's slot is the last
    # but is issued first
    cap = n_fwd * c.nconv
    t0, t1 = np.full(cap, -1.0), np.full(cap, -1.0)
    k = c.lib.rv_yolo_profile_times(c.h, c.h, t0.ctypes.data, t1.ctypes.data, cap)
    assert k == n_fwd * len(slots)
    t0 = np.roll(t0[:k].reshape(n_fwd, -1), 1, axis=1).ravel()
    t1 = np.roll(t1[:k].reshape(n_fwd, -1), 1, axis=1).ravel()
    assert (t1 >= t0).all()
    # profiled forwards keep the heads on one stream: issue order is time order
    assert (np.diff(t0) >= 0).all() and (np.diff(t1) >= 0).all()


def test_reps_and_switching_off_leave_counts_and_output_alone(ctx):
    c = ctx
    _raw_forwards(c, 1, 1)
    _, _, fl1, cv1, by1 = _read(c)
    raw3 = _raw_forwards(c, 1, 3)
    nf, ms3, fl3, cv3, by3 = _read(c)
    assert nf == 1
    np.testing.assert_array_equal(cv3, cv1)
    np.testing.assert_array_equal(fl3, fl1)
    np.testing.assert_array_equal(by3, by1)
    assert (ms3[cv3 >= 0] > 0).all()
    # off: nothing to read, and the unprofiled forward computes the same bits
    assert c.lib.rv_yolo_profile(c.h, 0) == 0
    assert _read(c)[0] == 0
    raw = c.raw()
    c.eng.forward_raw(c.lb, raw, candidates=False)
    r0 = raw.cpu().numpy()
    assert np.isfinite(r0).all()
    np.testing.assert_array_equal(raw3, r0)
    assert _read(c)[0] == 0

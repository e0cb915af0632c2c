"""The cases of tests/nms_cases.py reach the paths of csrc/nms.hip they are
named for -- from the oracle alone, no GPU.  These are conditions on the
inputs, not tolerances: were one to fail, test_nms_paths_gpu.py would be
comparing some other path of the kernel than it says.  The kernel rank-sorts
up to 1024 candidates and runs the bitonic network beyond, keeps the keys in
LDS up to 4096 candidates and in the workspace beyond, walks the sorted list
in chunks of 64 and tests a chunk against the kept list with 16 waves, wave w
taking the kept boxes w, w + 16, ..."""
import numpy as np
import pytest

import nms_cases as nm
from oracle import yolo_ref

f32 = np.float32
CASES = nm.cases()


def _reg(name, b=0):
    return nm.oracle(name).regime[b]


def _sorted_rows(name, b=0):
    """(box, score, cls) of image b in sorted order, after the max_nms cut."""
    box, score, cls, _ = nm.oracle(name).cand[b]
    o = _reg(name, b)["order"]
    return box[o], score[o], cls[o]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_oracle(name):
    """greedy_regime keeps what cpu.nms keeps, and its rows are postprocess's."""
    case, ans = CASES[name], nm.oracle(name)
    assert case.B == len(ans.out) >= 1
    for b in range(case.B):
        r = ans.regime[b]
        np.testing.assert_array_equal(r["kept"], r["keep_ref"])
        assert r["survivors_after"] == min(r["survivors"], case.p["max_det"])
        _, score, cls = _sorted_rows(name, b)
        ok = np.ones(len(r["kept"]), bool)
        if case.p["classes_keep"]:
            ok = np.isin(cls[r["kept"]], case.p["classes_keep"])
        np.testing.assert_array_equal(ans.out[b][:, 4], score[r["kept"]][ok])
        np.testing.assert_array_equal(ans.out[b][:, 5], cls[r["kept"]][ok].astype(f32))
        assert np.isfinite(ans.out[b]).all()  # no poison row ever reaches the oracle


def test_layouts_fit_the_entry():
    for name, case in CASES.items():
        assert 0 < case.nseg <= 1024 and case.nseg * 64 <= case.cap <= 65536, name
        assert 0 < case.p["max_det"] <= 1024 and case.p["max_nms"] > 0, name
        if case.raw is not None:
            A = case.raw.shape[2]
            assert case.raw.shape == (case.B, 4 + case.nc, A) and A < 65536, name
            assert case.nseg == -(-A // 64), name
        else:
            assert case.cand.shape == (case.B, case.cap, 8), name
            assert case.seg_n.shape == (case.B, case.nseg), name
            for b in range(case.B):
                used = np.clip(case.seg_n[b], 0, 64)
                assert _reg(name, b)["n"] == used.sum(), name


def test_sort_and_key_store_boundaries():
    assert nm.SORT_SIZES == [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097]
    for n in nm.SORT_SIZES:
        name = f"sort_n{n}"
        r = _reg(name)
        assert r["n"] == r["n_cut"] == n and r["max_tie"] == min(n, 1), name
        assert CASES[name].p["max_det"] == 1024
        # the kept boxes reach the last chunk: a sort error anywhere shows
        assert r["last_kept"] >= min(n, 1024) - 1 - 63 * (n > 1025), (name, r["last_kept"])
        if n > 1025:
            assert r["last_kept"] >= n - 64 and r["survivors"] < 1024
            assert r["cross_chunk"] > 30 and r["in_chunk"] > 1000
        else:
            assert r["survivors"] == n  # spread: every box survives
    # ragged A (a last segment that is not full) on the chunk and the sorter boundary
    assert CASES["sort_n65"].raw.shape[2] % 64 and CASES["sort_n1025"].raw.shape[2] % 64
    # anchor order is not score order: the sort has work to do
    for n in (64, 1024, 4097):
        o = _reg(f"sort_n{n}")["order"]
        assert (np.diff(o) < 0).sum() > n // 4


def test_full_layout():
    case, r = CASES["sort_full_65536"], _reg("sort_full_65536")
    assert (case.cap, case.nseg) == (65536, 1024) and (case.seg_n == 64).all()
    assert r["n"] == r["n_cut"] == 65536 and r["max_tie"] == 1
    assert r["last_kept"] >= 65536 - 128 and 900 < r["survivors"] < 1024
    assert (np.diff(r["order"]) < 0).sum() > 30000  # slot order is not score order
    assert r["suppressor_residues"] == set(range(16))


def _reversed_ties(name):
    """The oracle's rows when ties are resolved in reverse anchor order."""
    case = CASES[name]
    raw = case.oracle_raw[0][:, ::-1]
    return nm.postprocess(case, [np.ascontiguousarray(raw)])[0]


def test_ties_under_each_sorter():
    for name, n, lo, hi in [("ties_n300", 300, 0, 1024), ("ties_n3000", 3000, 1024, 4096),
                            ("ties_n6000", 6000, 4096, 65536)]:
        r = _reg(name)
        assert r["n"] == n and lo < n <= hi
        box, score, cls, _ = nm.oracle(name).cand[0]
        assert len(np.unique(score)) == 8 and r["max_tie"] >= n // 10
        rows = np.concatenate([box, score[:, None], cls[:, None].astype(f32)], 1)
        assert n - len(np.unique(rows, axis=0)) >= n // 20  # exact duplicate rows
        assert r["last_kept"] >= n - 300 and r["survivors"] < 1024
        # the order among equal scores decides the result
        assert nm.oracle(name).out[0].tobytes() != _reversed_ties(name).tobytes()
    r = _reg("ties_all_equal_1500")
    assert r["max_tie"] == r["n"] == 1500 and r["survivors"] == 1500
    # output order == anchor order
    np.testing.assert_array_equal(r["order"][r["kept"]], np.arange(1024))


def test_max_nms():
    assert [(_reg(n)["n"], _reg(n)["n_cut"]) for n in
            ("max_nms_1", "max_nms_100_in_tie", "max_nms_n_minus_1", "max_nms_n",
             "max_nms_4500_of_5000")] == [(200, 1), (400, 100), (333, 332), (333, 333),
                                          (5000, 4500)]
    assert 332 % 64 and 4500 % 64 and 5000 > 4096
    r = _reg("max_nms_100_in_tie")
    assert r["cut_in_tie"] and r["max_tie"] >= 40
    assert nm.oracle("max_nms_100_in_tie").out[0].tobytes() != \
        _reversed_ties("max_nms_100_in_tie").tobytes()
    # the cut changes the answer everywhere but at max_nms == n
    for name in ("max_nms_1", "max_nms_100_in_tie", "max_nms_n_minus_1", "max_nms_n",
                 "max_nms_4500_of_5000"):
        case = CASES[name]
        uncut = nm.postprocess(case, max_nms=30000)[0]
        assert (len(uncut) == len(nm.oracle(name).out[0])) == (name == "max_nms_n"), name
        assert len(nm.oracle(name).out[0]) < case.p["max_det"]  # max_det hides nothing
    assert _reg("max_nms_4500_of_5000")["last_kept"] >= 4500 - 64


def test_chains():
    for name, chunk_of in [("chain_in_chunk", (0, 0, 0)), ("chain_across_chunks", (0, 1, 1))]:
        case, r = CASES[name], _reg(name)
        assert case.p["iou"] == 0.5
        kept = set(r["kept"].tolist())
        box, _, cls = _sorted_rows(name)
        for a, b, c in case.note["chains"]:
            assert a in kept and b not in kept and c in kept, (name, a, b, c)
            assert (a // 64, b // 64, c // 64) == chunk_of
            np.testing.assert_array_equal(box[b] - box[a], [3, 0, 3, 0])
            np.testing.assert_array_equal(box[c] - box[b], [3, 0, 3, 0])
            assert cls[a] == cls[b] == cls[c]
    assert CASES["chain_in_chunk"].note["chains"] == [(0, 1, 2), (30, 31, 32), (61, 62, 63)]
    assert _reg("chain_in_chunk")["in_chunk"] == 3 and _reg("chain_in_chunk")["cross_chunk"] == 0
    assert _reg("chain_across_chunks")["cross_chunk"] == 1
    assert _reg("chain_across_chunks")["in_chunk"] == 0  # b is gone before it meets c


def test_kept_growth():
    r = _reg("kept_growth")
    assert r["n"] == 384 and r["survivors"] == 120
    # 20 new kept boxes per chunk: 0, 20, 40, 60, 80, 100 at the chunk starts
    kept = r["kept"]
    assert [int((kept < 64 * c).sum()) for c in range(6)] == [0, 20, 40, 60, 80, 100]
    assert r["max_kept_at_chunk_start"] == 100 > 48
    assert r["suppressor_residues"] == set(range(16))
    assert r["cross_chunk"] == 220 and r["in_chunk"] == 44


def test_class_offsets():
    r = _reg("classes_never_meet")
    box, _, cls = _sorted_rows("classes_never_meet")
    assert r["survivors"] == 8 and (box == box[0]).all() and sorted(cls) == list(range(8))
    r = _reg("class_126_127")
    box, _, cls = _sorted_rows("class_126_127")
    assert set(cls.tolist()) == {126, 127} and CASES["class_126_127"].p["max_wh"] == 7680.0
    off = (cls.astype(f32) * f32(7680.0))[:, None]
    assert off.max() == 975360.0
    assert (((box + off) - off) != box).mean() > 0.5  # the offset box loses low bits
    assert np.abs((box + off) - off - box).max() <= 1 / 32
    assert 40 < r["survivors"] < 150 and r["in_chunk"] + r["cross_chunk"] > 50


def test_degenerate_boxes():
    r = _reg("degenerate_boxes")
    box, _, _ = _sorted_rows("degenerate_boxes")
    kept = set(r["kept"].tolist())
    for k in range(4):  # degenerate, normal, degenerate again, the normal box's copy
        assert {4 * k, 4 * k + 1, 4 * k + 2} <= kept and 4 * k + 3 not in kept
        np.testing.assert_array_equal(box[4 * k + 1], box[4 * k + 3])
    w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    assert (w[0], w[8]) == (0, 0) and (h[4], h[8]) == (0, 0) and w[12] == -6 and h[12] == 30
    assert r["in_chunk"] == 4 and r["survivors"] == 60


def test_max_det():
    r = _reg("max_det_1")
    assert (r["survivors"], r["survivors_after"]) == (200, 1)
    r = _reg("max_det_7_mid_chunk")
    assert r["survivors"] > 7 == r["survivors_after"] and r["mid_chunk"]
    assert 6 < r["last_kept"] < 63  # a box was suppressed before the limit was reached
    r = _reg("max_det_64_chunk_end")
    assert r["survivors"] > 64 == r["survivors_after"] and r["last_kept"] == 63 and not r["mid_chunk"]
    r = _reg("max_det_100")
    assert r["survivors"] == 300 and r["survivors_after"] == 100
    assert (r["kept"] < 128).sum() == 100 and r["last_kept"] == 99 and r["mid_chunk"]
    for name, lds in [("max_det_1024_lds", True), ("max_det_1024_ws", False)]:
        r = _reg(name)
        assert (r["n"] <= 4096) == lds and r["n"] > 1024
        assert r["survivors"] > 1024 == r["survivors_after"] == CASES[name].p["max_det"]
        assert r["max_kept_at_chunk_start"] == 960


def test_class_filter():
    case = CASES["class_mask_four_words"]
    assert case.nc == 128 and case.p["classes_keep"] == (3, 40, 70, 127)
    assert sorted({c >> 5 for c in case.p["classes_keep"]}) == [0, 1, 2, 3]
    out = nm.oracle(case.name).out[0]
    _, _, cls = _sorted_rows(case.name)
    assert set(out[:, 5].astype(int).tolist()) == {3, 40, 70, 127}
    assert {2, 35, 41, 69, 96, 126} <= set(cls.tolist())  # neighbours of the kept bits are there
    case, r = CASES["filter_after_max_det"], _reg("filter_after_max_det")
    out = nm.oracle(case.name).out[0]
    assert case.p["max_det"] == 50 and r["survivors"] == 300 > 50
    assert 0 < len(out) < 10 and (out[:, 5] == 1).all()
    # filtering before max_det would give more rows
    assert (_sorted_rows(case.name)[2] == 1).sum() >= 20
    assert sum(1 for c in CASES.values() if not c.p["classes_keep"]) >= 40  # keep-all is the rule


def _pair_iou(box, cls, i, j, max_wh=7680.0):
    b = box + (cls.astype(f32) * f32(max_wh))[:, None]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = max(f32(0), min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]))
    h = max(f32(0), min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
    ovr = (w * h) / (area[i] + area[j] - w * h)
    assert ovr.dtype == f32
    return ovr


@pytest.mark.parametrize("key", list(nm.THRESHOLDS))
def test_iou_at_the_threshold(key):
    thr = nm.THRESHOLDS[key]
    name = f"iou_at_{key}"
    case = CASES[name]
    assert case.p["iou"] == thr and case.B == 3 and nm.THR_CLASSES == [0, 5, 79]
    # f32(thr) above the double: equality suppresses in the reference
    above = float(f32(thr)) > thr
    assert above == (key in ("0.6", "0.3"))
    for b, c in enumerate(nm.THR_CLASSES):
        box, score, cls = _sorted_rows(name, b)
        assert (cls == c).all() and len(cls) == 6
        lo, eq, hi = (_pair_iou(box, cls, 2 * k, 2 * k + 1) for k in range(3))
        assert eq == f32(thr) and eq.tobytes() == f32(thr).tobytes()
        assert lo < f32(thr) < hi and hi - lo < 1e-3
        r = nm.oracle(name).regime[b]
        assert r["at_threshold"] == 1
        assert r["kept"].tolist() == ([0, 1, 2, 4] if above else [0, 1, 2, 3, 4])
    # the discriminating fact behind the f32 threshold argument: rounding the
    # threshold to the nearest f32 changes the reference's answer at 0.6 and 0.3
    a = nm.postprocess(case, iou=thr)
    n = nm.postprocess(case, iou=float(f32(thr)))
    for b in range(3):
        assert (a[b].tobytes() != n[b].tobytes()) == above
        assert len(n[b]) == 5 and len(a[b]) == (4 if above else 5)
    # and the product's conversion does not: the largest f32 not above the double
    from rvs_amd.detect.yolo_hip import iou_threshold_f32
    r32 = iou_threshold_f32(thr)
    assert f32(r32) == r32 <= thr < float(np.nextafter(f32(r32), f32(2)))
    for b in range(3):
        assert nm.postprocess(case, iou=r32)[b].tobytes() == a[b].tobytes()


def test_iou_threshold_conversion():
    from rvs_amd.detect.yolo_hip import iou_threshold_f32
    rng = np.random.default_rng(5)
    for t in [0.0, 1.0, 0.5, 0.25, 0.7, 0.6, 0.3, 0.45, 0.1, 1e-30, 0.9999999999] + \
            list(rng.uniform(0, 1, 200)):
        r = iou_threshold_f32(t)
        assert f32(r) == r and r <= t and float(np.nextafter(f32(r), f32(np.inf))) > t, t
    assert iou_threshold_f32(0.7) == float(f32(0.7))  # rounds down already: unchanged
    assert iou_threshold_f32(0.6) == float(np.nextafter(f32(0.6), f32(0)))


def test_scale_boxes():
    want = {"scale_landscape": ((1080, 1920), (384, 640), 1 / 3, 0, 12),
            "scale_portrait": ((1920, 1080), (640, 384), 1 / 3, 12, 0),
            "scale_square_640": ((640, 640), (640, 640), 1.0, 0, 0),
            "scale_square_1280": ((1280, 1280), (640, 640), 0.5, 0, 0)}
    for name, (hw0, hw1, gain, px, py) in want.items():
        p = CASES[name].p
        assert (p["img0_hw"], p["img1_hw"]) == (hw0, hw1)
        g, pad = yolo_ref.scale_boxes_params(hw1, hw0)
        assert (g, pad) == (gain, (px, py)), name
        out = nm.oracle(name).out[0]
        assert len(out) == 40
        # clipped at every edge, and boxes that are not clipped at all
        assert (out[:, 0] == 0).sum() >= 2 and (out[:, 1] == 0).sum() >= 2
        assert (out[:, 2] == hw0[1]).sum() >= 2 and (out[:, 3] == hw0[0]).sum() >= 2
        inside = (out[:, 0] > 0) & (out[:, 1] > 0) & (out[:, 2] < hw0[1]) & (out[:, 3] < hw0[0])
        assert inside.sum() >= 10
        assert ((out[:, 0] == out[:, 2]) | (out[:, 1] == out[:, 3])).sum() >= 2  # wholly outside


def test_candidate_kernel_inputs():
    names = [n for n in CASES if n.startswith("cand_")]
    shapes = [(CASES[n].nc, CASES[n].raw.shape[2], CASES[n].B) for n in names]
    assert shapes == [(1, 64, 3), (80, 100, 3), (128, 128, 3), (1, 5040, 1), (80, 5040, 3),
                      (128, 5040, 1)]
    assert CASES["cand_nc80_A100"].cap > 64 * CASES["cand_nc80_A100"].nseg  # cap is free
    for name in names:
        case = CASES[name]
        nc, conf = case.nc, f32(case.p["conf"])
        for b in range(case.B):
            raw = case.raw[b]
            box, score, cls, anchor = nm.oracle(name).cand[b]
            at = {int(a): k for k, a in enumerate(anchor)}
            assert raw[4:, 1].max() == conf and 1 not in at      # == conf: rejected
            assert (raw[4:, 5] == conf).all() and 5 not in at
            k = at[2]                                            # nextafter(conf): accepted
            assert score[k] == np.nextafter(conf, f32(1)) and cls[k] == nc - 1
            k = at[3]                                            # two classes tie: the lower id
            assert (raw[4:, 3] == f32(0.625)).sum() == min(nc, 2) and cls[k] == nc // 3
            assert 0.2 < len(anchor) / raw.shape[1] < 0.45
            assert len(set((anchor // 64).tolist())) == case.nseg  # every segment has rows
            if nc > 1:
                assert len(set(cls.tolist())) > min(nc, 20) // 2


def test_segmented_layouts():
    assert [CASES[n].nseg for n in ("slots_nseg1", "slots_nseg65", "slots_nseg1024")] == [1, 65, 1024]
    assert CASES["slots_nseg1"].seg_n.tolist() == [[17], [0], [64]]
    for name in ("slots_nseg65", "slots_nseg1024"):
        s = CASES[name].seg_n
        assert s[0, :7].tolist() == [0, 64, 1, 0, 17, 64, 0]
        assert {0, 1, 64} <= set(s.ravel().tolist())
    assert _reg("slots_nseg1024")["n"] > 4096 and _reg("slots_nseg1024")["last_kept"] > 24000
    case = CASES["slots_count_clamp"]
    s = case.seg_n[0].tolist()
    assert 70 in s and -3 in s and min(s) < -(1 << 30) and max(s) > 1 << 30
    assert _reg(case.name)["n"] == 64 + 0 + 5 + 64 + 0 + 64 + 9
    # every unused slot of every hand-built layout is poison, and there are many
    for name, case in CASES.items():
        if case.cand is None:
            continue
        for b in range(case.B):
            used = np.zeros(case.cap, bool)
            for j, u in enumerate(np.clip(case.seg_n[b], 0, 64)):
                used[64 * j:64 * j + u] = True
            assert np.isinf(case.cand[b, ~used, 4]).all() and np.isfinite(case.cand[b, used]).all()
            anchor = case.cand.view(np.int32)[b, used, 6]
            assert len(set(anchor.tolist())) == len(anchor) and (anchor < 65536).all()
            assert (anchor >= 0).all() and (name == "slots_anchor_order" or (np.diff(anchor) > 0).all())
        assert name == "sort_full_65536" or np.isinf(case.cand[..., 4]).sum() >= 47


def test_anchor_order_is_not_slot_order():
    """Ties resolve by the anchor field: with the rows taken in slot order
    instead, the reference's answer is another one."""
    case, r = CASES["slots_anchor_order"], _reg("slots_anchor_order")
    assert r["max_tie"] >= 100 and r["n"] > 1024
    used = np.isfinite(case.cand[0, :, 4])
    anchor = case.cand.view(np.int32)[0, used, 6]
    assert (np.diff(anchor) < 0).sum() > r["n"] // 4
    by_slot = case.oracle_raw[0][:, np.argsort(np.argsort(anchor))]  # row of rank k, slot by slot
    np.testing.assert_array_equal(by_slot[:4].T[:, 0] - by_slot[2] / f32(2), case.cand[0, used, 0])
    assert nm.postprocess(case, [np.ascontiguousarray(by_slot)])[0].tobytes() != \
        nm.oracle(case.name).out[0].tobytes()


def test_mixed_batch():
    case = CASES["mixed_batch"]
    assert [r["n"] for r in nm.oracle("mixed_batch").regime] == nm.MIXED_N == \
        [0, 5000, 37, 6000, 1500, 4096]
    assert case.B == 6 and case.raw.shape[2] == 6400
    # empty, workspace, rank, workspace, LDS bitonic, LDS bitonic at its limit
    assert [(n > 1024) + (n > 4096) for n in nm.MIXED_N] == [0, 2, 0, 2, 1, 1]
    for b in (1, 3, 4, 5):
        r = _reg("mixed_batch", b)
        assert r["last_kept"] >= r["n"] - 64 and r["survivors"] < 1024


def test_engine_passes_the_converted_threshold(monkeypatch):
    """YoloEngine.nms -- the one place that reaches rv_nms_postprocess -- hands
    over iou_threshold_f32(iou), also after the attribute was changed."""
    import torch
    from rvs_amd.detect import yolo_hip
    seen = []
    monkeypatch.setattr(yolo_hip, "call", lambda name, *a: seen.append((name, a)) or 0)
    monkeypatch.setattr(yolo_hip, "stream_ptr", lambda: 0)
    eng = object.__new__(yolo_hip.YoloEngine)
    z = torch.zeros((1, 2, 8))
    eng.cand = eng.seg_n = eng.dets_s = eng.det_n_s = eng.cand_n_s = eng.nms_ws_s = z
    eng.scale5, eng.keep, eng.cap, eng._nseg_cur = z, None, 64, 1
    eng.max_det, eng.max_nms, eng.max_wh = 100, 30000, 7680.0
    eng.iou, eng._iou_arg = 0.7, (0.7, yolo_hip.iou_threshold_f32(0.7))
    for thr in (0.7, 0.6, 0.3, 0.5):
        eng.iou = thr
        eng.nms(1)
        name, a = seen[-1]
        assert name == "rv_nms_postprocess" and a[5] == yolo_hip.iou_threshold_f32(thr) <= thr
    assert seen[1][1][5] < float(f32(0.6)) and seen[0][1][5] == float(f32(0.7))

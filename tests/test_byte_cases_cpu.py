"""The BYTE cases (tests/byte_cases.py) run the regimes they are named for,
proved from the reference restatement alone (tests/byte_ref.py); the
restatement with every row high is oracle/sort_ref.SortTracker; and the host
side of the feature: the workspace layout query, the params6[5] argument
contract, the configuration keys, the registry names and the header.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import byte_cases as bc
import sort_cases as sc
from byte_ref import ByteSortTracker
from conftest import REPO
from oracle import sort_ref

HEADER = os.path.join(REPO, "include", "rvhip.h")
RANK_MAX, KEY_CAP = 256, 1024  # see byte_cases' docstring (bitonic: 513..1024)


def reg(name, s, f):
    return bc.reference(name)[s].frames[f].regime


def ids(name, s, f):
    return bc.reference(name)[s].frames[f].ids.tolist()


def _sort_at_high(case, st):
    """The same rows through the reference's SORT as the SORT configuration
    would see them: only the rows at or above the high threshold."""
    high = case.cfg["track_high_thresh"]
    fr = [r[np.float64(r[:, 4]) >= high] for r in (sc.rows_used(case, st, f)
                                                   for f in range(len(st.frames)))]
    return bc.run_reference(case.cfg, None, fr, st.ts, tracker=sort_ref.SortTracker)


def test_every_frame_of_every_case_is_consistent():
    for name, case in bc.cases().items():
        assert case.tmax <= 64 and case.dmax <= 64 and len(case.streams) <= 5, name
        for s, st in enumerate(case.streams):
            for f, fr in enumerate(bc.reference(name)[s].frames):
                r, n = fr.regime, len(sc.rows_used(case, st, f))
                assert r["D_high"] + r["D_low"] == n
                assert len(fr.ids) == n - r["n_dropped"] == r["D_high"] + r["n_match2"]
                assert r["n_new"] == r["D_high"] - r["n_match1"]
                assert (fr.ids >= 1).all()  # every kept row has a track
                if stream_has_proj(case, s):
                    assert r["min_rel_disp"] > sc.MIN_REL_DISP, (name, st.name, f)


def stream_has_proj(case, s):
    return bc.stream_proj(case, s) is not None


def test_fade_and_recover_keeps_id_and_speed_history():
    name = "fade_recover"
    case = bc.cases()[name]
    fr = bc.reference(name)[0].frames
    low = [f for f in range(len(fr)) if fr[f].regime["D_low"] == 1]
    assert len(low) == 8 and (low[-1] - low[0] + 2) * bc.DT > case.cfg["max_staleness"]
    assert all(fr[f].regime["n_match2"] == 1 for f in low)
    assert all(ids(name, 0, f) == [1, 2] for f in range(len(fr)))
    assert all(fr[f].T == 2 for f in range(len(fr))) and fr[-1].next_id == 3
    # an unbroken speed history: a speed and a distance in every frame after the first
    assert all(not np.isnan(fr[f].speed).any() and not np.isnan(fr[f].dist).any()
               for f in range(1, len(fr)))
    # the same rows through the reference's SORT at the high threshold: a new id
    ans = _sort_at_high(case, case.streams[0])
    first = [int(x) for x in ans.frames[0].ids]
    last = [int(x) for x in ans.frames[-1].ids]
    assert first == [1, 2] and last == [3, 2] and np.isnan(ans.frames[low[-1] + 1].speed[0])


def test_compaction_regime():
    r = reg("compaction", 0, 1)
    assert (r["D_high"], r["D_low"], r["n_match1"], r["n_match2"], r["n_dropped"],
            r["n_new"]) == (3, 4, 2, 2, 2, 1)
    assert r["kept"] == [1, 2, 3, 4, 5]  # the first and the last of 7 rows are dropped
    assert ids("compaction", 0, 1) == [1, 2, 5, 3, 4]
    r = reg("compaction", 0, 2)
    assert r["n_dropped"] == 1 and r["n_match2"] == 2 and r["n_match1"] == 1


def test_stage_order_differs_from_a_single_stage():
    name = "stage_order"
    case = bc.cases()[name]
    r = reg(name, 0, 1)
    assert (r["n_match1"], r["n_match2"], r["n_dropped"], r["kept"]) == (1, 0, 1, [1])
    assert ids(name, 0, 1) == [1]
    # one association over all rows gives the track to the low row (IoU 1 > 0.6)
    st = case.streams[0]
    single = bc.run_reference(case.cfg, None, st.frames, st.ts, tracker=sort_ref.SortTracker)
    assert single.frames[1].ids.tolist() == [1, 2]
    # the frame after: the track is where the high row was
    assert reg(name, 0, 2)["n_match2"] == 1


def test_eligibility_regime():
    name = "eligibility"
    assert ids(name, 0, 1) == [1, 3]
    r = reg(name, 0, 2)  # rows: low on B (streak 0), low on C (streak 1), high on A
    assert (r["cnt2"], r["n_match2"], r["n_dropped"], r["kept"]) == (1, 1, 1, [1, 2])
    assert ids(name, 0, 2) == [3, 1]
    r = reg(name, 0, 3)  # high on B: taken; low on A: taken in stage 2
    assert (r["n_match1"], r["n_match2"], r["n_new"]) == (1, 1, 0) and ids(name, 0, 3) == [2, 1]
    # without the eligibility rule B would have taken its low row
    st = bc.cases()[name].streams[0]
    m = sort_ref.iou_matrix(st.frames[0][1:2, :4], st.frames[2][0:1, :4])
    assert float(m[0, 0]) >= 0.5


@pytest.mark.parametrize("high", [0.25, 0.5, 0.1])
def test_threshold_edges(high):
    name = f"edges_{high}"
    st = bc.cases()[name].streams[0]
    conf = st.frames[1][:, 4]
    h32 = np.float32(high)
    assert conf[2] == h32 and conf[3] == np.nextafter(h32, np.float32(0)) and conf[3] < h32
    assert (np.float64(h32) >= high) and not (np.float64(conf[3]) >= high)
    if high == 0.1:
        assert np.float64(h32) != high  # not representable: f32(0.1) > 0.1
    r = reg(name, 0, 1)
    # kept: the exact-0.5 row, conf == high, one ulp over, and the low row on a track
    assert r["kept"] == [1, 2, 4, 5] and r["D_high"] == 2 and r["n_new"] == 2
    assert ids(name, 0, 1) == [2, 4, 5, 3]
    tb = st.frames[0][:, :4]
    m = sort_ref.iou_matrix(tb[:2], st.frames[1][:2, :4])
    assert m[1, 1] == np.float32(0.5) and m[0, 0] == np.nextafter(np.float32(0.5), np.float32(0))
    assert r["cnt2"] == 2


def test_ties_regime():
    name = "ties"
    st = bc.cases()[name].streams[0]
    m = sort_ref.iou_matrix(st.frames[0][:, :4], st.frames[1][:, :4])
    assert m[0, 1] == m[1, 1] >= 0.5 and m[2, 0] == m[2, 2] >= 0.5
    r = reg(name, 0, 1)
    assert (r["cnt2"], r["n_match2"], r["kept"]) == (4, 2, [0, 1])
    assert ids(name, 0, 1) == [3, 1]


def test_every_sorter_in_every_stage():
    def sorter(cnt):
        return "rank" if 0 < cnt <= RANK_MAX else "bitonic" if 512 < cnt <= KEY_CAP else \
            "argmax" if cnt > KEY_CAP else None
    want1 = ["rank", "bitonic", "argmax"]
    for s, w in enumerate(want1):
        for f in (1, 2):
            r = reg("sorters_stage1", s, f)
            assert sorter(r["cnt1"]) == w and r["cnt2"] == 0
    want2 = [(None, "rank"), (None, "bitonic"), (None, "argmax"), ("rank", "argmax"),
             ("argmax", "rank")]
    for s, (w1, w2) in enumerate(want2):
        r = reg("sorters_stage2", s, 1)
        assert (sorter(r["cnt1"]), sorter(r["cnt2"])) == (w1, w2), s
        assert r["n_dropped"] == 0 and r["n_new"] == 0
    assert max(max(bc.regimes(n, s, "T")) for n in ("sorters_stage1", "sorters_stage2")
               for s in range(3)) <= 64


def test_empty_and_overflow_regimes():
    name = "empty_results"
    case = bc.cases()[name]
    st = case.streams[0]
    assert reg(name, 0, 1)["D_high"] == 0 and len(ids(name, 0, 1)) == 0
    assert reg(name, 0, 1)["n_dropped"] == 2
    assert len(sc.rows_used(case, st, 2)) == 0
    assert st.dcount[3] < 0 and len(sc.rows_used(case, st, 3)) == 0
    assert st.dcount[4] > case.dmax and len(sc.rows_used(case, st, 4)) == case.dmax
    # (both tracks missed three frames: neither is eligible for a low row)
    assert reg(name, 0, 4)["n_dropped"] > 0 and reg(name, 0, 4)["n_match1"] == 1
    assert reg(name, 0, 4)["n_match2"] == 0 and reg(name, 0, 4)["n_new"] > 0
    name = "full_pool"
    case = bc.cases()[name]
    r = reg(name, 0, 1)
    assert case.overflow and r["T"] + r["n_new"] > case.tmax and r["n_match2"] == 2
    assert len(sc.rows_used(case, case.streams[0], 1)) == case.dmax


def test_per_camera_and_mixed_batch_regimes():
    name = "per_camera"
    case = bc.cases()[name]
    assert [p is None for p in case.projs] == [False, True, False]
    for s in (0, 2):
        fr = bc.reference(name)[s].frames
        low = [f for f in range(len(fr)) if fr[f].regime["n_match2"] == 1]
        assert len(low) == 8
        assert all(not np.isnan(fr[f].speed[0]) and not np.isnan(fr[f].dist[0]) for f in low)
    assert all(np.isnan(fr.dist).all() for fr in bc.reference(name)[1].frames)
    name = "mixed_batch"
    assert len(bc.cases()[name].streams) == 5
    tot = {k: sum(sum(bc.regimes(name, s, k)) for s in range(5))
           for k in ("n_match1", "n_match2", "n_dropped", "n_new")}
    assert all(v > 0 for v in tot.values()), tot


@pytest.mark.parametrize("name", list(sc.cases()))
def test_all_high_is_the_reference_sort(name):
    """ByteSortTracker with every row high equals oracle.sort_ref.SortTracker
    output for output on the streams of tests/sort_cases.py."""
    case = sc.cases()[name]
    cfg = dict(case.cfg, track_high_thresh=bc.ALL_HIGH_THRESH)
    for s, st in enumerate(case.streams):
        fr = [sc.rows_used(case, st, f) for f in range(len(st.frames))]
        assert min((float(r[:, 4].min()) for r in fr if len(r)), default=1.0) >= bc.ALL_HIGH_THRESH
        got = bc.run_reference(cfg, case.proj, fr, st.ts)
        ref = sc.oracle(name)[s]
        for f, (a, b) in enumerate(zip(got.frames, ref.frames)):
            assert a.kept.tobytes() == fr[f].tobytes()
            assert a.ids.tobytes() == b.ids.tobytes() and a.dist.tobytes() == b.dist.tobytes()
            assert a.speed.tobytes() == b.speed.tobytes() and (a.T, a.next_id) == (b.T, b.next_id)
        assert got.x.tobytes() == ref.x.tobytes() and got.meta.tobytes() == ref.meta.tobytes()


def test_high_zero_is_sort_too():
    case = bc.cases()["compaction"]
    st = case.streams[0]
    a = bc.run_reference(dict(case.cfg, track_high_thresh=0.0), None, st.frames, st.ts)
    b = bc.run_reference(case.cfg, None, st.frames, st.ts, tracker=sort_ref.SortTracker)
    assert all(x.ids.tobytes() == y.ids.tobytes() for x, y in zip(a.frames, b.frames))
    assert a.x.tobytes() == b.x.tobytes()


# ---------------------------------------------------------------------------
# the host side of the library
# ---------------------------------------------------------------------------
def _lib():
    from rvs_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("S,tmax,dmax", [(1, 1, 1), (2, 64, 16), (5, 64, 64), (32, 1024, 100),
                                         (3, 100, 7)])
def test_kept_layout_agrees_with_the_workspace(S, tmax, dmax):
    lib = _lib()
    d, n = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.rv_sort_kept_layout(S, tmax, dmax, ctypes.byref(d), ctypes.byref(n)) == 0
    total = lib.rv_sort_ws_bytes(S, tmax, dmax)
    assert d.value % 256 == 0 and n.value % 256 == 0
    # behind M, the predicted boxes, last_update_ts and the jobs; disjoint; inside
    before = S * tmax * dmax * 4 + S * tmax * 16 + S * tmax * 8 + S * dmax * 8
    assert d.value >= before
    assert d.value + S * dmax * 24 <= n.value and n.value + S * 4 <= total
    assert total - n.value < 256 + S * 4


def test_kept_layout_argument_errors():
    lib = _lib()
    d, n = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.rv_sort_kept_layout(0, 8, 8, ctypes.byref(d), ctypes.byref(n)) == -1000
    assert lib.rv_sort_kept_layout(2, 8, 8, None, ctypes.byref(n)) == -1000
    assert b"null" in lib.rv_last_error()


def _sort_call(lib, params, cams_entry, **kw):
    p, ok = ctypes.c_void_p, 4096  # non-null, aligned, never dereferenced
    a = dict(wsb=1 << 30, dmax=4)
    a.update(kw)
    par = p(params.ctypes.data) if params is not None else p(ok)
    if cams_entry:
        return lib.rv_sort_update_cams(p(ok), p(ok), 2, 8, p(ok), p(ok), a["dmax"], p(ok), par,
                                       p(ok), p(ok), a["wsb"], p(ok), p(ok), p(ok), None)
    return lib.rv_sort_update(p(ok), p(ok), 2, 8, p(ok), p(ok), a["dmax"], p(ok), par, None, None,
                              p(ok), a["wsb"], p(ok), p(ok), p(ok), None)


@pytest.mark.parametrize("cams_entry", [False, True])
def test_params6_high_threshold_contract(cams_entry):
    """params6[5] outside [0, 1] or NaN is RV_EINVAL before any HIP call, and
    params6 is not read before the other arguments have passed."""
    lib = _lib()
    assert lib.rv_abi_version() >= 13
    for bad in (-0.01, 1.5, float("nan"), float("inf")):
        par = np.array([1.2, 3, 0.35, 0.8, -1.0, bad], np.float64)
        assert _sort_call(lib, par, cams_entry) == -1000
        assert b"track_high_thresh" in lib.rv_last_error()
    # a pointer that must not be dereferenced: the other checks come first
    assert _sort_call(lib, None, cams_entry, wsb=16) == -1000
    assert b"workspace" in lib.rv_last_error()
    assert _sort_call(lib, None, cams_entry, dmax=5000) == -1000
    assert b"sizes" in lib.rv_last_error()


def test_three_launch_form_refuses_byte():
    """RV_SORT_FUSED=0 (read once per process) with params6[5] > 0: RV_EINVAL
    with a text, before any HIP call."""
    code = ("import ctypes, numpy as np\n"
            "from rvs_amd import _lib\n"
            "lib = _lib.load(); p = ctypes.c_void_p; ok = 4096\n"
            "par = np.array([1.2, 3, 0.35, 0.8, -1.0, 0.5], np.float64)\n"
            "st = lib.rv_sort_update(p(ok), p(ok), 2, 8, p(ok), p(ok), 4, p(ok), "
            "p(par.ctypes.data), None, None, p(ok), 1 << 30, p(ok), p(ok), p(ok), None)\n"
            "print(st, lib.rv_last_error().decode())\n")
    env = dict(os.environ, RV_SORT_FUSED="0",
               PYTHONPATH=os.pathsep.join([os.path.join(REPO, "road-vision-system_amd"), REPO]))
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    r = subprocess.run(py + ["-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("-1000 ") and "fused" in r.stdout and "RV_SORT_FUSED" in r.stdout


def test_header_and_signatures_agree():
    from rvs_amd import _lib, schedule
    hdr = open(HEADER).read()
    assert re.search(r"int rv_sort_kept_layout\(int S, int tmax, int dmax, size_t\* dets_off, "
                     r"size_t\* n_off\);", hdr)
    assert re.search(r"#define RV_BYTE_SECOND_IOU 0\.5\b", hdr)
    res, args = _lib._SIGS["rv_sort_kept_layout"]
    assert res is ctypes.c_int and args == [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    assert "track_high_thresh" in hdr
    # no new entry point carries the update, no new schedule op: the mode
    # travels in the 48-byte copy of params6
    assert len(schedule._OPS) == 11
    assert schedule._OPS["rv_sort_update"][2][8] == 48
    assert schedule._OPS["rv_sort_update_cams"][2][8] == 48
    import byte_ref
    assert byte_ref.SECOND_IOU == 0.5


# ---------------------------------------------------------------------------
# configuration and registry
# ---------------------------------------------------------------------------
def _engine_cfg(**trk):
    from rvs_amd.config import load_config
    cfg = load_config()
    cfg["detect"]["enabled"] = False  # no detector: the engine builds on a CPU device
    cfg["tracking"].update(enabled=True, **trk)
    return cfg


@pytest.mark.parametrize("trk", [dict(track_low_thresh=0.0), dict(track_low_thresh=-0.1),
                                 dict(track_low_thresh=0.3), dict(track_high_thresh=1.01),
                                 dict(track_high_thresh=0.05),
                                 dict(track_low_thresh=float("nan"))])
def test_engine_refuses_bad_thresholds(trk):
    import warnings
    from rvs_amd.engine import RoadVisionEngine
    for backend in ("bytetrack", "byte", "bytetrack_hip", "ByteTrack"):
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # a ValueError, not the "init failed" warning
            with pytest.raises(ValueError, match="track_low_thresh"):
                RoadVisionEngine(_engine_cfg(backend=backend, **trk), 2, (64, 64), device="cpu")
    # the SORT backend does not read the keys
    RoadVisionEngine(_engine_cfg(backend="sort", **trk), 2, (64, 64), device="cpu")


def test_threshold_defaults():
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.track.byte_hip import byte_thresholds
    assert byte_thresholds({}, 0.25) == (0.1, 0.25)
    assert byte_thresholds({"track_high_thresh": 0.6}, 0.25) == (0.1, 0.6)
    assert byte_thresholds({"track_low_thresh": 0.2, "track_high_thresh": 0.2}) == (0.2, 0.2)
    eng = RoadVisionEngine(_engine_cfg(backend="bytetrack"), 2, (64, 64), device="cpu")
    assert eng.byte and eng.tracker is None  # detect off: nothing to track
    eng = RoadVisionEngine(_engine_cfg(backend="sort"), 2, (64, 64), device="cpu")
    assert not eng.byte
    # configs/default.yaml and config.py keep their values
    from rvs_amd.config import _DEFAULTS, load_config
    assert "track_high_thresh" not in load_config()["tracking"]
    assert "track_low_thresh" not in _DEFAULTS["tracking"]
    assert load_config()["tracking"]["backend"] == "sort"


def test_build_tracker_names():
    import torch
    from rvs_amd.track.registry import build_tracker
    for name in ("bytetrack", "byte", "bytetrack_hip", "BYTE"):
        if torch.cuda.is_available():
            from rvs_amd.track.byte_hip import ByteTracker
            assert isinstance(build_tracker({"backend": name}), ByteTracker)
        else:
            with pytest.raises(RuntimeError, match="ByteTracker"):
                build_tracker({"backend": name})
    with pytest.raises(ValueError, match="unknown tracker backend"):
        build_tracker({"backend": "deepsort"})
    with pytest.raises(ValueError, match="track_low_thresh"):
        build_tracker({"backend": "byte", "track_low_thresh": 0.9, "track_high_thresh": 0.5})

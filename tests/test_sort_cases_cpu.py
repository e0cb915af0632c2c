"""The cases of tests/sort_cases.py reach the regimes they are named for --
from the oracle alone, no GPU.  These are conditions on the inputs, not
tolerances: were one to fail, test_sort_paths_gpu.py would be comparing some
other path of the kernel than it says.  The fused kernel runs 512 threads and
keeps at most 1024 sorted pairs: cnt <= 512 is the rank sort, 512 < cnt <=
1024 the bitonic sort, above that the argmax loop; a frame with D <= 64 takes
the row-parallel Kalman update, D > 64 the per-lane one."""
import numpy as np

import sort_cases as sc


def _r(name, s, key, first=0):
    return sc.regimes(name, s, key, first)


def test_every_frame_fits_the_pools():
    """Tracks and detections fit tmax and dmax in every case but the one
    about overflow, and every stream of a case has the same number of frames."""
    assert [n for n, c in sc.cases().items() if c.overflow] == ["no_room"]
    for name, case in sc.cases().items():
        assert len({len(st.frames) for st in case.streams}) == 1, name
        for s, st in enumerate(case.streams):
            assert len(st.frames) == len(st.ts), name
            ans = sc.oracle(name)[s]
            assert case.overflow or max(fr.T for fr in ans.frames) <= case.tmax, name
            assert max(_r(name, s, "D")) <= case.dmax, name


def test_every_speed_is_well_conditioned():
    """sort_cases.MIN_REL_DISP: no speed is a difference of ground coordinates
    so close that the oracle's own rounding shows at the rtol 1e-12 bar."""
    worst = {}
    for name, case in sc.cases().items():
        for s, st in enumerate(case.streams):
            worst[f"{name}/{st.name}"] = min(_r(name, s, "min_rel_disp"))
    print(worst)
    assert min(worst.values()) >= sc.MIN_REL_DISP == 5e-4, worst


def test_bitonic_thr0():
    cnt = _r("bitonic_thr0", 0, "cnt", first=1)
    assert len(cnt) == 39 and all(512 < c <= 1024 for c in cnt), cnt
    assert (min(cnt), max(cnt)) == (598, 729)


def test_bitonic_crowd():
    c40 = _r("bitonic_crowd", 0, "cnt", first=1)
    c30 = _r("bitonic_crowd", 1, "cnt", first=1)
    assert len(c40) == 29 and all(512 < c <= 1024 for c in c40), c40
    assert len(c30) == 29 and all(512 < c <= 1024 for c in c30), c30
    assert (min(c40), max(c40)) == (804, 871) and (min(c30), max(c30)) == (625, 711)
    assert sc.cases()["bitonic_crowd"].cfg["iou_threshold"] == 0.05
    # the pairs are dense: every detection meets 20+ tracks above the threshold
    assert min(c40) / 40 > 20 and min(c30) / 30 > 20


def test_cnt_boundaries():
    got = [_r("cnt_boundaries", s, "cnt")[1] for s in range(4)]
    assert got == [512, 513, 1024, 1025]
    assert [(_r("cnt_boundaries", s, "T0")[1], _r("cnt_boundaries", s, "D")[1])
            for s in range(4)] == sc.BOUNDARY_TD
    # the third frame updates matched tracks again
    for s in range(4):
        ans = sc.oracle("cnt_boundaries")[s]
        assert len(ans.frames) == 3 and (ans.meta[:, 1] == 3).sum() >= 10


def test_hist_cap():
    assert max(_r("hist_cap", 0, "max_hist")) == 32
    assert sum(_r("hist_cap", 0, "n_speed")) == 611  # >= 500
    # 31 frames at 120 fps are 0.26 s: the 0.8 s window never drops an entry
    # before the cap does
    assert sc.cases()["hist_cap"].cfg["speed_window"] == 0.8


def test_hist_window_clamp():
    """speed_window = 0.01 is clamped to 0.05 s = 6 frames at 120 fps:
    without the clamp one entry would be kept and every speed be None."""
    assert sc.cases()["hist_window_clamp"].cfg["speed_window"] == 0.01
    assert max(_r("hist_window_clamp", 0, "max_hist")) == 7
    assert sum(_r("hist_window_clamp", 0, "n_speed")) == 611


def test_update_forms():
    name = "update_forms"
    case = sc.cases()[name]
    assert case.dmax == 128 and [st.name for st in case.streams] == ["le64", "ge65", "64_65",
                                                                     "full"]
    assert all(len(st.frames) == 40 for st in case.streams)
    assert max(_r(name, 0, "D")) <= 64
    assert min(_r(name, 1, "D")) >= 65
    assert sum(_r(name, 1, "n_speed")) >= 1000
    d = _r(name, 2, "D")
    assert set(d) == {64, 65} and d.count(64) >= 10 and d.count(65) >= 10
    full = case.streams[3]
    assert all(len(fr) == 128 for fr in full.frames)
    assert sorted(set(full.dcount)) == [-3, 135] and full.dcount.count(-3) == 1
    d = _r(name, 3, "D")
    assert d[20] == 0 and d.count(128) == 39
    # the empty frame comes while tracks are alive and they survive it
    assert _r(name, 3, "T0")[20] >= 128 and sc.oracle(name)[3].frames[20].T >= 128


def test_many_tracks():
    assert _r("many_tracks", 0, "T0", first=1) == [530, 530, 530]
    assert _r("many_tracks", 0, "cnt", first=1) == [530, 530, 530]  # no box meets another's
    assert [fr.T for fr in sc.oracle("many_tracks")[0].frames] == [530] * 4
    case = sc.cases()["many_tracks"]
    assert (case.tmax, case.dmax) == (1024, 576)


def test_odd_pool():
    case = sc.cases()["odd_pool"]
    assert (case.tmax, case.dmax) == (100, 7) and len(case.streams[0].frames) == 80
    d = _r("odd_pool", 0, "D")
    assert max(d) == 7 and d.count(7) >= 10  # frames that fill every row
    assert sc.oracle("odd_pool")[0].frames[-1].next_id - 1 >= 64  # more than one wave of slots


def test_time_edges():
    name = "time_equal_backward"
    eq, back = sc.cases()[name].streams
    assert sum(1 for f in range(1, 45) if eq.ts[f] == eq.ts[f - 1]) == 15
    dts = np.diff(back.ts)
    assert (dts < 0).sum() == 2 and np.allclose(dts[dts < 0], -0.05)
    # a track born in one frame and matched in the next at the same timestamp:
    # the speed's t1 - t0 = 0 takes the 1e-3 clamp
    assert sum(_r(name, 0, "n_dt_clamp")) >= 2
    assert sum(_r(name, 0, "n_speed")) >= 400 and sum(_r(name, 1, "n_speed")) >= 400
    # max_staleness = 0: tracks live on only while matched (or the time stands still)
    assert sc.cases()["stale_zero"].cfg["max_staleness"] == 0.0
    assert max(_r("stale_zero", 0, "T0")) <= 21 and sum(_r("stale_zero", 0, "n_speed")) >= 250
    assert sum(_r("stale_zero", 0, "n_dt_clamp")) >= 10
    ans = sc.oracle("stale_zero")[0]
    assert ans.frames[-1].next_id - 1 >= 80  # 4x the live tracks: slots reused all the time


def test_stale_negative_reports_distances_of_tracks_that_are_gone():
    assert sc.cases()["stale_negative"].cfg["max_staleness"] == -1.0
    ans = sc.oracle("stale_negative")[0]
    assert all(fr.T == 0 for fr in ans.frames) and len(ans.meta) == 0
    # every detection starts a track that is pruned in the same frame
    gone = sum(int((~np.isnan(fr.dist)).sum()) for fr in ans.frames)
    assert gone >= 20 and gone == 86
    assert all(np.isnan(fr.speed).all() and (fr.ids > 0).all() for fr in ans.frames)


def test_no_room():
    """7 new tracks for 4 slots, every one with a distance in the oracle."""
    case, ans = sc.cases()["no_room"], sc.oracle("no_room")[0]
    assert case.tmax == 4 and len(ans.frames) == 1
    fr = ans.frames[0]
    assert fr.T == 7 and list(fr.ids) == [1, 2, 3, 4, 5, 6, 7] and not np.isnan(fr.dist).any()


def test_box_edges():
    name = "box_edges"
    deg, shr, dup = sc.cases()[name].streams
    for fr in deg.frames:
        x1, y1, x2, y2 = fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3]
        assert (x1 == x2).sum() >= 1 and (x2 < x1).sum() >= 1 and (y2 < y1).sum() >= 1
        assert ((x2 - x1 > 0) & (x2 - x1 < 2e-4)).sum() == 1
    assert min(_r(name, 1, "min_s_pred")) < 0  # the shrinking track's predicted area
    assert sum(1 for v in _r(name, 1, "min_s_pred") if v < 0) >= 3
    for fr in dup.frames:
        _, counts = np.unique(fr, axis=0, return_counts=True)
        assert (counts == 2).sum() == 3
    # the copies take part: a copy that loses the tie starts a track of its own
    assert sc.oracle(name)[2].frames[-1].next_id - 1 >= 40


def test_partial_projector():
    """One track has None and non-None distances over its life, and a
    non-None speed after a None frame (its history skips that frame)."""
    ans = sc.oracle("partial_projector")[0]
    y2 = np.concatenate([fr[:, 3] for fr in sc.cases()["partial_projector"].streams[0].frames])
    assert (y2 == np.round(y2)).all() and (y2 == 500).sum() == 6
    life = {}
    for fr in ans.frames:
        for i, d, v in zip(fr.ids, fr.dist, fr.speed):
            life.setdefault(int(i), []).append((np.isnan(d), np.isnan(v)))
    assert len(life) == 6
    n_ok = 0
    for seq in life.values():
        none_at = [k for k, (dn, _) in enumerate(seq) if dn]
        assert len(none_at) == 1 and seq[none_at[0]][1]  # speed None with the distance
        after = seq[none_at[0] + 1:]
        n_ok += bool(after) and not after[0][0] and not after[0][1]
    assert n_ok >= 5

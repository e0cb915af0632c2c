"""Per-camera ground projectors on the device: rv_sort_update_cams (both
launch forms), rv_untracked_metrics_cams, rv_homography_project_cams, the
two recorded-schedule ops and the engine's geometry.cameras, against
oracle/sort_ref run once per stream with that stream's projector passed per
call.  Bars as tests/test_sort_gpu.py: ids exact, distance_m exact, speed_kmh
rtol 1e-12, None patterns equal (cams_common.compare)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cams_common as cc
from conftest import REPO
from oracle import sort_ref

pytestmark = pytest.mark.gpu

IMG = [[560, 1000], [1360, 1000], [1160, 620], [760, 620]]


def _dev(cuda, *arrs):
    return [torch.from_numpy(a).to(cuda) for a in arrs]


def _host(t):
    return tuple(x.cpu().numpy() for x in t)


def _bytes_equal(a, b, what):
    """Byte equality (NaN payloads included) of two tuples of arrays."""
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)


def _tracker(cuda):
    from rvs_amd.track.sort_hip import MultiStreamSort
    return MultiStreamSort(cc.CFG, cc.S, tmax=cc.TMAX, dmax=cc.DMAX, device=cuda)


def test_sort_update_cams_vs_oracle(cuda):
    """set_projectors / set_camera_projector over the common input: every
    stream equals the reference tracker called with that stream's projector
    as of that frame -- the removed projector's tracks keep reporting, the
    recalibrated camera's history spans both calibrations."""
    cc.check_non_vacuous()
    ms = _tracker(cuda)
    ms.set_projectors([cc.device_projector(c) for c in cc.CAMS])
    for f in range(cc.NF):
        for s, spec in cc.CHANGES.get(f, {}).items():
            ms.set_camera_projector(s, cc.device_projector(spec))
        dets, cnt, ts = cc.batch(f)
        i, d, v = _host(ms.update(*_dev(cuda, dets, cnt, ts)))
        for s in range(cc.S):
            n = cnt[s]
            cc.compare((i[s, :n], d[s, :n], v[s, :n]), s, f)
            assert (i[s, n:] == -1).all() and np.isnan(d[s, n:]).all() and np.isnan(v[s, n:]).all()
    assert ms.stats()["overflow"].sum() == 0


def test_sort_update_cams_three_launch_form():
    """The same test in a fresh process with RV_SORT_FUSED=0 (the switch is
    read once per process): the table is then read by the update kernel."""
    env = dict(os.environ, RV_SORT_FUSED="0")
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    r = subprocess.run(py + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "-x",
                        os.path.join(REPO, "tests", "test_cams_gpu.py") +
                        "::test_sort_update_cams_vs_oracle"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _run_all(cuda, update):
    """12 frames through update(f, dets, cnt, ts) -> per-frame host outputs."""
    outs = []
    for f in range(cc.NF):
        outs.append(_host(update(*_dev(cuda, *cc.batch(f)))))
    return outs


def _cams_call(ms, cams_ptr):
    """MultiStreamSort.update through rv_sort_update_cams with a raw table
    pointer (0 = NULL)."""
    from rvs_amd._lib import call, ptr, stream_ptr

    def update(dets, cnt, ts):
        ms.params[:4] = [ms.max_staleness, ms.min_hits, ms.iou_threshold, ms.speed_window]
        st = ms.state[0]
        call("rv_sort_update_cams", ptr(st), ptr(st), ms.S, ms.tmax, ptr(dets), ptr(cnt), ms.dmax,
             ptr(ts), ms.params.ctypes.data, cams_ptr, ptr(ms.ws), ms.ws_bytes, ptr(ms.out_id),
             ptr(ms.out_dist), ptr(ms.out_speed), stream_ptr())
        return ms.out_id, ms.out_dist, ms.out_speed
    return update


def test_same_projector_in_every_entry_equals_the_single_projector_entry(cuda):
    proj = cc.device_projector(cc.CAMS[0])
    a, b = _tracker(cuda), _tracker(cuda)
    a.set_projector(proj)
    b.set_projectors([proj] * cc.S)
    assert b.cams is not None and a.cams is None
    oa, ob = _run_all(cuda, a.update), _run_all(cuda, b.update)
    for f in range(cc.NF):
        _bytes_equal(oa[f], ob[f], f"frame {f}")
    _bytes_equal(a.export(), b.export(), "state")
    assert sum(int((~np.isnan(o[1])).sum()) for o in oa) >= 250  # 5 streams of distances
    assert sum(int((~np.isnan(o[2])).sum()) for o in oa) >= 200
    # set_projector drops the table again
    b.set_projector(proj)
    assert b.cams is None


def test_null_table_equals_no_projector(cuda):
    a, b = _tracker(cuda), _tracker(cuda)
    a.set_projector(None)
    oa, ob = _run_all(cuda, a.update), _run_all(cuda, _cams_call(b, None))
    for f in range(cc.NF):
        _bytes_equal(oa[f], ob[f], f"frame {f}")
        assert np.isnan(ob[f][1]).all() and np.isnan(ob[f][2]).all()
    _bytes_equal(a.export(), b.export(), "state")
    assert sum(int((o[0] >= 0).sum()) for o in ob) >= 300  # ids were handed out


def _boxes(rng, n):
    x1 = rng.uniform(0, 1800, n)
    y1 = rng.uniform(150, 900, n)
    w = rng.uniform(20, 200, n)
    h = rng.uniform(20, 180, n)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


def test_untracked_metrics_cams_vs_oracle(cuda):
    from rvs_amd.engine import _UntrackedMetrics
    rng = np.random.default_rng(7)
    det_n = np.array([cc.DMAX, 0, 7, cc.DMAX, 3], np.int32)
    dets = np.zeros((cc.S, cc.DMAX, 6), np.float32)
    dets[..., :4] = _boxes(rng, cc.S * cc.DMAX).reshape(cc.S, cc.DMAX, 4)  # rows >= det_n too
    dets[..., 4] = 0.5
    d_dev, n_dev = _dev(cuda, dets, det_n)
    um = _UntrackedMetrics(cc.S, cc.DMAX, None, cuda,
                           projectors=[cc.device_projector(c) for c in cc.CAMS])
    i, d, v = _host(um(d_dev, n_dev))
    assert (i == -1).all() and np.isnan(v).all()
    n_val = 0
    for s, spec in enumerate(cc.CAMS):
        proj = cc.oracle_projector(spec)
        for k in range(cc.DMAX):
            ref = None if (proj is None or k >= det_n[s]) else proj.distance_for_bbox(dets[s, k, :4])
            if ref is None:
                assert np.isnan(d[s, k]), (s, k)
            else:
                assert d[s, k] == ref, (s, k, d[s, k], ref)
                n_val += 1
    assert n_val >= 7 + 2 * cc.DMAX - 2 and (d[3] == 12.5).sum() >= 3
    # rows >= det_n[s]: as the single-projector entry writes them
    one = _UntrackedMetrics(cc.S, cc.DMAX, cc.device_projector(cc.CAMS[0]), cuda)
    i1, d1, v1 = _host(one(d_dev, n_dev))
    for s in range(cc.S):
        n = det_n[s]
        _bytes_equal((i[s, n:], d[s, n:], v[s, n:]), (i1[s, n:], d1[s, n:], v1[s, n:]), f"tail {s}")
    _bytes_equal((d[0],), (d1[0],), "camera 0 is the single projector")
    # one recalibration: camera 1 gets camera 3's projector
    um.set_camera_projector(1, cc.device_projector(cc.CAMS[3]))
    det_n2 = np.array([cc.DMAX, 5, 7, cc.DMAX, 3], np.int32)
    i, d2, v = _host(um(d_dev, _dev(cuda, det_n2)[0]))
    p3 = cc.oracle_projector(cc.CAMS[3])
    assert [d2[1, k] for k in range(5)] == [p3.distance_for_bbox(dets[1, k, :4]) for k in range(5)]
    assert np.isnan(d2[1, 5:]).all()


def test_homography_project_cams_vs_oracle(cuda):
    from rvs_amd.track.sort_hip import CameraTable, project_boxes_cams
    rng = np.random.default_rng(11)
    n = 301  # more than one block, not a multiple of it
    boxes = _boxes(rng, n)
    cam = rng.integers(0, cc.S, n).astype(np.int32)
    cam[17], cam[190] = -1, cc.S  # outside [0, S): NaN, no entry read
    cam[:5] = np.arange(5)
    tab = CameraTable([cc.device_projector(c) for c in cc.CAMS], cuda)
    xy, dist = _host(project_boxes_cams(tab.dev, *_dev(cuda, boxes, cam)))
    got_xy, ref_xy = [], []
    n_val = 0
    for k in range(n):
        spec = cc.CAMS[cam[k]] if 0 <= cam[k] < cc.S else None
        proj = cc.oracle_projector(spec)
        pt = None if proj is None else proj.project_bbox(boxes[k])
        if pt is None:
            assert np.isnan(xy[k]).all() and np.isnan(dist[k]), (k, cam[k])
            continue
        n_val += 1
        assert not np.isnan(xy[k]).any(), k
        got_xy.append(xy[k])
        ref_xy.append(pt)
        ref = proj.distance(pt)
        assert dist[k] == ref, (k, cam[k], dist[k], ref)
    got_xy, ref_xy = np.array(got_xy), np.array(ref_xy, np.float64)
    print("project_cams: valid", n_val, "max abs xy error", np.abs(got_xy - ref_xy).max(),
          "max |xy|", np.abs(ref_xy).max())
    assert n_val >= 100
    # f64 ground points, the bar of tests/test_track_ops_gpu.py for the
    # single-projector entry: each coordinate is a 3-term f64 dot product of
    # terms up to ~1e3 (H rows x pixel coordinates) over w, summed in another
    # order than numpy's -- a few 1e-13 absolute where the terms cancel, 1e-12
    # relative elsewhere
    np.testing.assert_allclose(got_xy, ref_xy, rtol=1e-12, atol=1e-12)
    assert np.isnan(xy[17]).all() and np.isnan(xy[190]).all()
    assert np.isnan(dist[17]) and np.isnan(dist[190])


def test_recorded_schedule_reads_the_table_on_every_run(cuda):
    """One RV_SCHED_SORT_UPDATE_CAMS and one RV_SCHED_UNTRACKED_CAMS node,
    recorded once; camera 3's entry is overwritten between two runs and the
    second run follows it: both runs equal the eager calls with the table of
    that time."""
    from rvs_amd.engine import _UntrackedMetrics
    from rvs_amd.schedule import Schedule
    projs = [cc.device_projector(c) for c in cc.CAMS]
    new3 = cc.device_projector(cc.CAMS[0])
    d0, c0, t0 = cc.batch(0)
    dets, cnt, ts = _dev(cuda, d0, c0, t0)  # the nodes' fixed input buffers

    def pair():
        ms = _tracker(cuda)
        ms.set_projectors(projs)
        return ms, _UntrackedMetrics(cc.S, cc.DMAX, None, cuda, projectors=projs)
    (ms_r, um_r), (ms_e, um_e), (ms_o, um_o) = pair(), pair(), pair()

    sched = Schedule()
    with sched.recording():
        ms_r.update(dets, cnt, ts)
        um_r(dets, cnt)
    assert sched.num_nodes() == 2

    def eager(ms, um):
        return _host(ms.update(dets, cnt, ts)) + _host(um(dets, cnt))

    def recorded():
        sched.run()
        torch.cuda.synchronize()
        return _host((ms_r.out_id, ms_r.out_dist, ms_r.out_speed)) + \
            _host((um_r.out_id, um_r.out_dist, um_r.out_speed))

    _bytes_equal(recorded(), eager(ms_e, um_e), "run 1")
    eager(ms_o, um_o)
    # frame 1 into the same buffers, camera 3 recalibrated: stream-ordered copies
    d1, c1, t1 = cc.batch(1)
    for dst, src in ((dets, d1), (cnt, c1), (ts, t1)):
        dst.copy_(torch.from_numpy(src))
    for ms, um in ((ms_r, um_r), (ms_e, um_e)):
        ms.set_camera_projector(3, new3)
        um.set_camera_projector(3, new3)
    got = recorded()
    _bytes_equal(got, eager(ms_e, um_e), "run 2")
    old = eager(ms_o, um_o)  # the table as it was recorded
    n3 = c1[3]
    assert n3 >= 3 and not np.array_equal(got[1][3, :n3], old[1][3, :n3])
    assert not np.array_equal(got[4][3, :n3], old[4][3, :n3])
    for s in (0, 1, 2, 4):  # the other cameras are untouched
        _bytes_equal(tuple(x[s] for x in got), tuple(x[s] for x in old), f"stream {s}")
    p = cc.oracle_projector(cc.CAMS[0])
    assert [got[4][3, k] for k in range(n3)] == [p.distance_for_bbox(d1[3, k, :4]) for k in range(n3)]
    sched.close()


def _camera_mapping(spec):
    """A geometry.cameras entry whose fitted homography is (close to) the
    spec's: four image points and their ground points under it."""
    p = sort_ref.HomographyProjector(spec[0])
    return {"type": "homography", "image_points": IMG,
            "world_points": [list(p.project_point(x, y)) for x, y in IMG],
            "origin": [float(v) for v in spec[1]], "max_distance": spec[2]}


def _key(lst):
    return [(d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id, d.cls_name, d.track_id, d.distance_m,
             d.speed_kmh) for d in lst]


@pytest.mark.parametrize("tracking", [True, False])
def test_engine_cameras_equal_one_engine_per_camera(cuda, tracking):
    """geometry.cameras = [camera 0, null, camera 3] on one S = 3 engine
    against the reference's arrangement: one single-stream engine per camera,
    each with its own geometry.projector (none for the null camera)."""
    from rvs_amd.config import load_config
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.synth import road_frames
    S, H, W, K = 3, 360, 640, 3
    cams = [_camera_mapping(cc.CAMS[0]), None, _camera_mapping(cc.CAMS[3])]
    base = load_config()
    base["tracking"]["enabled"] = tracking
    cfg = copy.deepcopy(base)
    cfg["geometry"]["enabled"] = True
    cfg["geometry"]["cameras"] = cams
    frames = road_frames(S, K, H, W, device=cuda)
    ts = [torch.full((1,), k / 30.0, dtype=torch.float64, device=cuda) for k in range(K)]
    eng = RoadVisionEngine(cfg, S, (H, W), device=cuda)
    assert (eng.tracker is not None) == tracking
    assert (eng.tracker.cams if tracking else eng._untracked.cams) is not None
    multi = [eng.results(eng.step(frames[k], ts[k].expand(S).contiguous())) for k in range(K)]
    eng.close()
    n_dist = 0
    for s in range(S):
        c1 = copy.deepcopy(base)
        if cams[s] is not None:
            c1["geometry"]["enabled"] = True
            c1["geometry"]["projector"] = cams[s]
        one = RoadVisionEngine(c1, 1, (H, W), device=cuda)
        assert (one.projector is None) == (cams[s] is None) and one.projectors is None
        for k in range(K):
            res = one.results(one.step(frames[k][s:s + 1], ts[k]))
            assert _key(res[0]) == _key(multi[k][s]), (s, k)
            n_dist += sum(d.distance_m is not None for d in res[0])
            if cams[s] is None:
                assert all(d.distance_m is None and d.speed_kmh is None for d in res[0])
        one.close()
    assert sum(len(x) for r in multi for x in r) >= 9 and n_dist >= 3

"""Every path of the BYTE instances of the fused SORT kernel (csrc/sort.hip)
against tests/byte_ref.ByteSortTracker on the named cases of
tests/byte_cases.py, through MultiStreamByte on both entries: rv_sort_update
with a host projector and rv_sort_update_cams with the per-camera table.
test_byte_cases_cpu.py proves from the reference alone that every case runs
the path it is named for.

Exact: the kept rows (bit for bit), the kept count, ids, the zero / -1 / NaN
tails and rv_sort_stats.  State, distance and speed at the bars of
tests/test_sort_paths_gpu.py: distance exact with its None pattern, speed rtol
1e-12 with its None pattern, x at rtol = atol = 1e-9, id / hits / streak / cls /
T / next_id exact."""
import numpy as np
import pytest
import torch

import byte_cases as bc
import sort_cases as sc

pytestmark = pytest.mark.gpu


def _tracker(case, cuda, cams, cls=None, cfg=None):
    from rvs_amd.track.byte_hip import MultiStreamByte
    ms = (cls or MultiStreamByte)(cfg or case.cfg, len(case.streams), tmax=case.tmax,
                                  dmax=case.dmax, device=cuda)
    projs = getattr(case, "projs", None)
    if projs is not None:
        ms.set_projectors([sc.device_projector(p) for p in projs])
    elif cams:
        ms.set_projectors([sc.device_projector(case.proj)] * len(case.streams))
    else:
        ms.set_projector(sc.device_projector(case.proj))
    return ms


def _frames(case, cuda, ms):
    """Every frame through ms.update -> per frame the host copies of (kept
    rows, kept counts, ids, dist, speed); the inputs must come back untouched."""
    for f in range(len(case.streams[0].frames)):
        host = sc.batch(case, f)
        dev = [torch.from_numpy(a).to(cuda) for a in host]
        out = ms.update(*dev)
        assert dev[0].cpu().numpy().tobytes() == host[0].tobytes()
        yield f, host, tuple(x.cpu().numpy() for x in (ms.kept_dets, ms.kept_n) + tuple(out))


# (a per-camera case has no single-projector form)
ENTRIES = [(n, c) for n, k in bc.cases().items() for c in (False, True) if c or k.projs is None]


@pytest.mark.parametrize("name,cams", ENTRIES,
                         ids=[f"{n}-{'camera_table' if c else 'host_projector'}"
                              for n, c in ENTRIES])
def test_case_vs_reference(cuda, name, cams):
    case = bc.cases()[name]
    ms = _tracker(case, cuda, cams)
    # garbage in the outputs and the kept regions: every row must be written
    ms.kept_dets.fill_(7.0)
    ms.kept_n.fill_(-9)
    ms.out_id.fill_(77)
    for f, _, got in _frames(case, cuda, ms):
        bc.compare_frame(name, f, *got)
    bc.compare_final(name, ms.export(), ms.stats())


@pytest.mark.parametrize("cams", [False, True], ids=["host_projector", "camera_table"])
@pytest.mark.parametrize("name", list(sc.cases()))
def test_all_high_sort_cases(cuda, name, cams):
    """Every case of tests/sort_cases.py with every conf at or above high > 0:
    the BYTE instances give the SORT oracle's answer, and keep every row."""
    case = sc.cases()[name]
    ms = _tracker(case, cuda, cams, cfg=dict(case.cfg, track_high_thresh=bc.ALL_HIGH_THRESH))
    for f, (dets, cnt, _), (kept, kn, ids, dist, speed) in _frames(case, cuda, ms):
        n = np.clip(cnt, 0, case.dmax)
        np.testing.assert_array_equal(kn, n)
        for s in range(len(case.streams)):
            assert kept[s, :n[s]].tobytes() == dets[s, :n[s]].tobytes(), (name, f, s)
            assert not kept[s, n[s]:].any()
        sc.compare_frame(name, f, ids, dist, speed)
    sc.compare_final(name, ms.export(), ms.stats())


@pytest.mark.parametrize("name", ["compaction", "fade_recover", "sorters_stage2"])
def test_high_zero_is_multistreamsort(cuda, name):
    """track_high_thresh = 0 through MultiStreamByte launches the plain
    instance: bit-identical to MultiStreamSort on the same rows."""
    from rvs_amd.track.sort_hip import MultiStreamSort
    case = bc.cases()[name]
    cfg = dict(case.cfg, track_high_thresh=0.0)
    a = _tracker(case, cuda, False, cfg=cfg)
    b = _tracker(case, cuda, False, cls=MultiStreamSort, cfg=cfg)
    assert a.params[5] == 0.0
    for f in range(len(case.streams[0].frames)):
        dev = [torch.from_numpy(x).to(cuda) for x in sc.batch(case, f)]
        oa = [x.cpu().numpy().tobytes() for x in a.update(*dev)]
        ob = [x.cpu().numpy().tobytes() for x in b.update(*dev)]
        assert oa == ob, f
    for x, y in zip(a.export(), b.export()):
        assert x.tobytes() == y.tobytes()
    sa, sb = a.stats(), b.stats()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)


def _detections(r):
    from rvs_amd.detect.types import Detection
    return [Detection(*map(float, x[:5]), int(x[5]), "") for x in r]


def _same_lists(got, ref_frame, rows_in, msg):
    """The returned Detection objects against the reference's kept list."""
    assert len(got) == len(ref_frame.ids), msg
    rows = np.array([[d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id] for d in got],
                    np.float32).reshape(-1, 6)
    assert rows.tobytes() == ref_frame.kept.tobytes(), msg
    assert [d.track_id for d in got] == ref_frame.ids.tolist(), msg
    dist = np.array([np.nan if d.distance_m is None else d.distance_m for d in got], np.float64)
    spd = np.array([np.nan if d.speed_kmh is None else d.speed_kmh for d in got], np.float64)
    np.testing.assert_array_equal(dist, ref_frame.dist, err_msg=msg)
    np.testing.assert_allclose(spd, ref_frame.speed, rtol=1e-12, equal_nan=True, err_msg=msg)


@pytest.mark.parametrize("name", ["fade_recover", "compaction", "eligibility", "edges_0.1"])
def test_byte_tracker_update(cuda, name):
    """ByteTracker.update (the reference's single-stream API) returns the
    reference's kept lists: the same objects, mutated."""
    from rvs_amd.track.byte_hip import ByteTracker
    case = bc.cases()[name]
    st = case.streams[0]
    trk = ByteTracker(case.cfg, tmax=case.tmax, dmax=case.dmax)
    proj = sc.device_projector(case.proj)
    for f in range(len(st.frames)):
        dets = _detections(sc.rows_used(case, st, f))
        got = trk.update(dets, st.ts[f], proj)
        assert all(any(g is d for d in dets) for g in got)
        _same_lists(got, bc.reference(name)[0].frames[f], st.frames[f], f"{name} frame {f}")
        assert all(d.track_id is None for d in dets if not any(g is d for g in got))
    trk.close()


def test_update_many_and_low_filter(cuda):
    """update_many over the S = 5 mixed batch returns the reference's kept
    lists; rows below track_low_thresh are removed on the host."""
    from rvs_amd.track.byte_hip import MultiStreamByte
    name = "mixed_batch"
    case = bc.cases()[name]
    ms = MultiStreamByte(case.cfg, len(case.streams), tmax=case.tmax, dmax=case.dmax, device=cuda)
    ms.set_projector(None)
    junk = np.array([[5000.0, 5000.0, 5050.0, 5050.0, 0.05, 0]], np.float32)  # below low = 0.1
    for f in range(len(case.streams[0].frames)):
        lists = [_detections(np.concatenate([junk, sc.rows_used(case, st, f)]))
                 for st in case.streams]
        got = ms.update_many(lists, [st.ts[f] for st in case.streams])
        for s, st in enumerate(case.streams):
            assert all(g is not lists[s][0] for g in got[s])
            _same_lists(got[s], bc.reference(name)[s].frames[f], st.frames[f],
                        f"{name}/{st.name} frame {f}")

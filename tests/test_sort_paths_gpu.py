"""Every path of the SORT kernel (csrc/sort.hip) against oracle/sort_ref on
the named cases of tests/sort_cases.py: the three association strategies and
the counts where one hands over to the next, both Kalman update forms, the
speed history's cap and clamps, timing / box / table-size edges, the
ping-pong state buffers -- in the fused launch form and, in a child process,
the three-launch form.  test_sort_cases_cpu.py proves from the oracle alone
that every case runs the path it is named for.

Bars as tests/test_sort_gpu.py, on every frame of every stream: ids exact,
distance_m exact with its None pattern, speed_kmh rtol 1e-12 with its None
pattern, rows [D, dmax) empty; after the last frame x at rtol = atol = 1e-9,
id / hits / streak / cls / T / next_id exact, no overflow (but in `no_room`,
whose one frame brings more new tracks than the pool has slots)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sort_cases as sc
from conftest import REPO

pytestmark = pytest.mark.gpu


def _tracker(case, cuda):
    from rvs_amd.track.sort_hip import MultiStreamSort
    ms = MultiStreamSort(case.cfg, len(case.streams), tmax=case.tmax, dmax=case.dmax, device=cuda)
    ms.set_projector(sc.device_projector(case.proj))
    return ms


def _run(case, cuda, ms, update=None):
    """Every frame through update(dets, cnt, ts) -> per-frame host outputs."""
    update = update or ms.update
    outs = []
    for f in range(len(case.streams[0].frames)):
        dev = [torch.from_numpy(a).to(cuda) for a in sc.batch(case, f)]
        outs.append(tuple(x.cpu().numpy() for x in update(*dev)))
    return outs


@pytest.mark.parametrize("name", list(sc.cases()))
def test_case_vs_oracle(cuda, name):
    case = sc.cases()[name]
    ms = _tracker(case, cuda)
    for f, (ids, dist, speed) in enumerate(_run(case, cuda, ms)):
        sc.compare_frame(name, f, ids, dist, speed)
    sc.compare_final(name, ms.export(), ms.stats())


def _pingpong_call(ms, other):
    """MultiStreamSort.update through the raw rv_sort_update with two state
    buffers: state_in = the current one, state_out = the other, then swap."""
    from rvs_amd._lib import call, ptr, stream_ptr
    ms.state = [ms.state[0], other]

    def update(dets, cnt, ts):
        ms.params[:4] = [ms.max_staleness, ms.min_hits, ms.iou_threshold, ms.speed_window]
        src, dst = ms.state[ms.cur], ms.state[1 - ms.cur]
        call("rv_sort_update", ptr(src), ptr(dst), ms.S, ms.tmax, ptr(dets), ptr(cnt), ms.dmax,
             ptr(ts), ms.params.ctypes.data, ms._H.ctypes.data, ms._origin.ctypes.data,
             ptr(ms.ws), ms.ws_bytes, ptr(ms.out_id), ptr(ms.out_dist), ptr(ms.out_speed),
             stream_ptr())
        ms.cur = 1 - ms.cur  # export() / stats() read state[cur]
        return ms.out_id, ms.out_dist, ms.out_speed
    return update


def test_pingpong_state_buffers_equal_in_place(cuda):
    """state_in != state_out, alternating: outputs and the final state are
    the in-place run's, byte for byte (NaN payloads included)."""
    name = "bitonic_crowd"
    case = sc.cases()[name]
    a, b = _tracker(case, cuda), _tracker(case, cuda)
    other = torch.full_like(b.state[0], 0xA5)  # state_out starts as garbage
    oa, ob = _run(case, cuda, a), _run(case, cuda, b, _pingpong_call(b, other))
    assert len(oa) == 30 and b.cur == 0 and b.state[0].data_ptr() != b.state[1].data_ptr()
    for f in range(len(oa)):
        for k in range(3):
            assert oa[f][k].tobytes() == ob[f][k].tobytes(), (f, k)
    for k, (x, y) in enumerate(zip(a.export(), b.export())):
        assert x.tobytes() == y.tobytes(), k
    sa, sb = a.stats(), b.stats()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    # and the ping-pong run is the oracle's as well
    sc.compare_final(name, b.export(), sb)


def test_three_launch_form():
    """The tests above in a fresh process with RV_SORT_FUSED=0 (the switch is
    read once per process).  There the association runs 1024 threads: cnt =
    1024 is a rank sort, 1025 the argmax loop; the Kalman update is always
    the per-lane form.  The expectations are the same."""
    env = dict(os.environ, RV_SORT_FUSED="0")
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    r = subprocess.run(py + ["-m", "pytest", "-q", "-p", "no:cacheprovider", "-x",
                             os.path.join(REPO, "tests", "test_sort_paths_gpu.py"),
                             "-k", "not three_launch_form"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    n = len(sc.cases()) + 1
    assert r.returncode == 0 and f"{n} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]

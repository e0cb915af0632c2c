"""A chain holding StreakDerain on the engine, in the manner of
test_engine_dcp_gpu.py at small shapes: preprocess_stage() gives the proc and
letterbox bytes of the ops applied one by one (tests/streak_ref.py, then the
oracle's CLAHE and median), sequential step() calls give the same proc, and
PipelinedRun, recorded (native) and eager, replays the chain twice with the
same proc and the same detections."""
import copy

import numpy as np
import pytest
import torch

import streak_cases as C
from streak_ref import streak_ref
from oracle import cpu

pytestmark = pytest.mark.gpu

S, K = 2, 4
CHAIN = [{"name": "StreakDerain", "params": {"slant": -1, "max_len": 49}},
         {"name": "CLAHEDehaze", "params": {"tile_grid": 8, "clip_limit": 2.0}},
         {"name": "StreakDerain", "params": {"slant": 1, "thresh": 30}},
         {"name": "MedianDerain", "params": {"ksize": 3}}]


def _cfg(H, W):
    from rvs_amd.config import load_config
    cfg = copy.deepcopy(load_config())
    cfg["detect"]["weights"] = "synthetic"
    cfg["detect"]["imgsz"] = max(H, W)
    cfg["detect"]["conf_thres"] = 0.001  # the synthetic weights score low
    cfg["detect"]["classes_keep"] = []
    cfg["preprocess"]["chain"] = copy.deepcopy(CHAIN)
    return cfg


def _want(f):
    out = streak_ref(f, 3, 9, 49, -1, 20)[0]
    out = cpu.clahe_ycrcb(out, 8, 2.0)
    out = streak_ref(np.ascontiguousarray(out), 3, 9, 0, 1, 30)[0]
    return cpu.median(out, 3)


def _key(res):
    return [[(d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id, d.track_id, d.distance_m, d.speed_kmh)
             for d in s] for s in res]


@pytest.mark.parametrize("H,W", [(64, 96), (160, 224)])
def test_engine_runs_a_chain_with_the_streak_op(cuda, H, W):
    from rvs_amd import kernels
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.preprocess.ops import streak_params
    from rvs_amd.schedule import PipelinedRun
    assert streak_params(CHAIN[0]["params"]) == (3, 9, 49, -1, 20)
    assert streak_params(CHAIN[2]["params"]) == (3, 9, 0, 1, 30)
    cfg = _cfg(H, W)
    host = np.stack([np.stack([C.rainy(C.road(H, W, 10 * k + s), -1, 100 + 10 * k + s, 30,
                                       (9, 17, 33, 4 * H)) for s in range(S)]) for k in range(K)])
    frames = torch.from_numpy(host).to(cuda)
    ts = [torch.full((S,), k / 30.0, dtype=torch.float64, device=cuda) for k in range(K)]
    want_proc = [np.stack([_want(host[k, s]) for s in range(S)]) for k in range(K)]
    assert not np.array_equal(streak_ref(host[0, 0], 3, 9, 49, -1, 20)[0], host[0, 0])

    seq = RoadVisionEngine(cfg, S, (H, W), device=cuda)
    geo = seq.detector.geo
    assert seq.pipeline.chain_supported
    assert seq.pipeline.chain_route(H, W, geo) == kernels.ROUTE_OPS
    proc, lb = seq.preprocess_stage(frames[0])
    np.testing.assert_array_equal(proc.cpu().numpy(), want_proc[0], err_msg="proc")
    for s in range(S):
        np.testing.assert_array_equal(lb[s].cpu().numpy(), cpu.letterbox(want_proc[0][s], geo),
                                      err_msg=f"letterbox {s}")
    seq_res = []
    for r in range(2):
        for k in range(K):
            out = seq.step(frames[k], ts[k])
            seq_res.append(_key(seq.results(out)))
            np.testing.assert_array_equal(out["proc"].cpu().numpy(), want_proc[k],
                                          err_msg=f"step() proc {k}")
    assert sum(len(s) for r in seq_res for s in r) > 0  # the comparison saw detections

    for mode in ("native", "eager"):
        pip = RoadVisionEngine(cfg, S, (H, W), device=cuda, lanes=2, pair=2)
        run = PipelinedRun(pip, [frames[k] for k in range(K)], ts, mode=mode)
        if mode == "native":
            assert run.sched.num_nodes() > 0
        for r in range(2):  # the second run replays the recorded descriptor
            run.run()
            torch.cuda.synchronize()
            for k, o in enumerate(run.outs):
                np.testing.assert_array_equal(o["proc"].cpu().numpy(), want_proc[k],
                                              err_msg=f"{mode} run {r} proc {k}")
                assert _key(pip.results(o)) == seq_res[r * K + k], f"{mode} run {r} step {k}"
        run.close()
        pip.close()
    np.testing.assert_array_equal(frames.cpu().numpy(), host)  # inputs untouched
    seq.close()

"""The BYTE tracker backend on the engine, in the manner of
test_engine_dcp_gpu.py: a BYTE engine's per-step records equal
tests/byte_ref.ByteSortTracker fed with the NMS rows of a tracking-off engine
at the same conf = track_low_thresh (the rows the hand-back, the overlays and
the sink see are the rows the tracker kept), and a recorded PipelinedRun
equals eager step() calls record for record while the eager engine records
`annotated` overlays.

LOW / HIGH were chosen from the scores the shipped synthetic weights give on
these frames (the best row of an image scores 0.41 to 0.69, about 30 rows
reach 0.3, and under 0.18 an image runs into max_det = 100): over the run low
rows are both matched in the second association (13) and dropped (166), and
no image reaches max_det.  The test asserts that regime and fails if the
weights or the frames stop giving it."""
import copy

import numpy as np
import pytest
import torch

import byte_cases as bc
import sort_cases as sc

pytestmark = pytest.mark.gpu

S, H, W, K = 2, 360, 640, 6
LOW, HIGH = 0.3, 0.38


def _cfg(backend="bytetrack", tracking=True):
    from rvs_amd.config import load_config
    cfg = copy.deepcopy(load_config())
    cfg["tracking"]["enabled"] = tracking
    cfg["tracking"]["backend"] = backend
    cfg["tracking"]["track_low_thresh"] = LOW
    cfg["tracking"]["track_high_thresh"] = HIGH
    return cfg


def _key(res):
    return [[(d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id, d.track_id, d.distance_m, d.speed_kmh)
             for d in s] for s in res]


def _inputs(cuda):
    from rvs_amd.synth import road_frames
    frames = road_frames(S, K, H, W, device=cuda)
    ts = [torch.full((S,), k / 30.0, dtype=torch.float64, device=cuda) for k in range(K)]
    return frames, ts


def test_engine_records_equal_the_reference_on_the_nms_rows(cuda):
    from rvs_amd.engine import RoadVisionEngine
    frames, ts = _inputs(cuda)
    # the NMS rows at conf = LOW: a tracking-off engine
    cfg = _cfg(tracking=False)
    cfg["detect"]["conf_thres"] = LOW
    off = RoadVisionEngine(cfg, S, (H, W), device=cuda)
    rows = []
    for k in range(K):
        out = off.step(frames[k], ts[k])
        d, n = out["dets"].cpu().numpy(), out["det_n"].cpu().numpy()
        rows.append([d[s, :n[s]].copy() for s in range(S)])
    off.close()
    assert all(len(r) < off.max_det for fr in rows for r in fr)  # the max_det caveat
    refs = [bc.run_reference(dict(_cfg()["tracking"]), None, [rows[k][s] for k in range(K)],
                             [k / 30.0 for k in range(K)]) for s in range(S)]
    tot = {k: sum(fr.regime[k] for a in refs for fr in a.frames) for k in ("n_match2", "n_dropped")}
    assert tot["n_match2"] >= 1 and tot["n_dropped"] >= 1, tot

    eng = RoadVisionEngine(_cfg(), S, (H, W), device=cuda)
    assert eng.byte and eng.detector.conf == pytest.approx(LOW)
    for k in range(K):
        out = eng.step(frames[k], ts[k])
        res = eng.results(out)
        n = out["det_n"].cpu().numpy()
        for s in range(S):
            ref = refs[s].frames[k]
            got = np.array([[d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id] for d in res[s]],
                           np.float32).reshape(-1, 6)
            assert int(n[s]) == len(ref.ids), (k, s)
            assert got.tobytes() == ref.kept.tobytes(), (k, s)
            assert [d.track_id for d in res[s]] == ref.ids.tolist(), (k, s)
            assert all(d.distance_m is None and d.speed_kmh is None for d in res[s])
    st = eng.track_stats()
    assert [int(x) for x in st["next_id"]] == [a.frames[-1].next_id for a in refs]
    eng.close()


def test_recorded_pipeline_equals_eager_steps(cuda, tmp_path):
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.schedule import PipelinedRun
    frames, ts = _inputs(cuda)
    cfg = _cfg()
    cfg["geometry"]["enabled"] = True
    cfg["geometry"]["projector"]["image_points"] = [[186, 333], [453, 333], [386, 206], [253, 206]]
    cfg["geometry"]["projector"]["world_points"] = [[-3.5, 5.0], [3.5, 5.0], [3.5, 30.0],
                                                    [-3.5, 30.0]]
    rec = copy.deepcopy(cfg)
    rec["preview"]["record"] = {"enable": True, "path": str(tmp_path / "b{stream}.mjpeg"),
                                "content": "annotated"}
    seq = RoadVisionEngine(rec, S, (H, W), device=cuda)
    assert seq.byte and seq._rec_overlay is not None
    seq_res, kept_n = [], 0
    for k in range(K):
        out = seq.step(frames[k], ts[k])
        assert out["dets"].data_ptr() == seq.tracker.kept_dets.data_ptr()
        seq_res.append(_key(seq.results(out)))
        kept_n += int(out["det_n"].sum())
    seq.close()
    assert kept_n > 0
    assert all((tmp_path / f"b{s}.mjpeg").stat().st_size > 0 for s in range(S))

    pip = RoadVisionEngine(cfg, S, (H, W), device=cuda, lanes=2, pair=2)
    run = PipelinedRun(pip, [frames[k] for k in range(K)], ts, mode="native")
    for r in range(2):  # the second run replays the recorded schedule on new tracker state
        pip.tracker.reset()
        run.run()
        torch.cuda.synchronize()
        for k, o in enumerate(run.outs):
            assert _key(pip.results(o)) == seq_res[k], f"run {r} step {k}"
    run.close()
    pip.close()

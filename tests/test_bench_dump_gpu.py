"""bench.py's plain run and --dump-outputs on the GPU, at 2 camera streams:
a plain run times exactly --steps steps and runs none of the --full legs;
the dump holds the last timed step's hand-back (float32 / float64 arrays,
rows past a stream's detection count zeroed) and the seeded proc sample; the
same arguments give the same dump, whether the steps are issued by the
native launch list, eagerly, or as sequential step() calls."""
import gc
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, K, W = 2, 4, 1
NAMES = ["det_count", "boxes_xyxy", "conf", "cls_id", "track_id", "distance_m", "speed_kmh",
         "proc_sample_index", "proc_sample"]
F64 = {"track_id", "distance_m", "speed_kmh", "proc_sample_index"}


_DONE = {}


def _run(tmp_path, capfd, tag, *extra):
    """One bench.main run with --dump-outputs (each `tag` runs once per module)."""
    import bench
    if tag in _DONE:
        return _DONE[tag]
    out = tmp_path / tag
    try:
        rc = bench.main(["--gpus", "1", "--streams", str(S), "--steps", str(K), "--warmup", str(W),
                         "--no-autotune", "--dump-outputs", str(out), *extra])
    finally:
        gc.unfreeze()  # BenchJob.prepare froze the collector's generations
    assert rc == 0
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in NAMES)
    _DONE[tag] = json.loads(lines[0]), {n: np.load(out / (n + ".npy")) for n in NAMES}
    return _DONE[tag]


@pytest.fixture(scope="module")
def runs(tmp_path_factory, cuda):
    return tmp_path_factory.mktemp("bench_dump")


def test_plain_run_line_and_dump(runs, capfd):
    import bench
    d, a = _run(runs, capfd, "native")
    # the line: K timed steps, ms_per_step their mean, value the frame rate
    assert d["steps"] == K and d["warmup"] == W and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["dtype"] == "bf16" and d["metric"] == bench.METRIC
    assert abs(d["ms_per_step"] - d["elapsed_s"] / K * 1e3) < 1e-3
    assert abs(d["value"] - S * K / d["elapsed_s"]) < 1e-3 * d["value"]
    # none of the --full legs ran
    for k in ("device_only", "pair1", "secondary", "cpu_baseline", "steady_state_ms_per_step"):
        assert k not in d
    assert d["roofline"] is None
    # the dump: dtypes, shapes, padding
    for n, v in a.items():
        assert v.dtype == (np.float64 if n in F64 else np.float32), n
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    dmax = a["conf"].shape[1]
    assert a["det_count"].shape == (S,) and a["boxes_xyxy"].shape == (S, dmax, 4)
    n = a["det_count"].astype(int)
    assert n.sum() > 0 and n.max() <= dmax  # the synthetic frames give detections
    valid = np.arange(dmax)[None, :] < n[:, None]
    for k in ("conf", "cls_id", "track_id", "distance_m", "speed_kmh"):
        assert a[k].shape == (S, dmax) and not a[k][~valid].any(), k
    assert not a["boxes_xyxy"][~valid].any()
    assert (a["conf"][valid] > 0).all() and (a["conf"][valid] <= 1).all()
    b = a["boxes_xyxy"][valid]
    assert (b[:, 2] >= b[:, 0]).all() and (b[:, 3] >= b[:, 1]).all()
    assert b.min() >= 0 and b[:, 2].max() <= bench.W and b[:, 3].max() <= bench.H
    assert (a["track_id"][valid] >= -1).all() and (a["track_id"][valid] >= 0).any()
    assert all(np.isfinite(v).all() for v in a.values())
    # the proc sample: sorted flat indices into (S, H, W, 3), u8 values
    i, p = a["proc_sample_index"], a["proc_sample"]
    assert i.shape == p.shape == (min(bench.DUMP_PROC_SAMPLES, S * bench.H * bench.W * 3),)
    assert (np.diff(i) >= 0).all() and i[0] >= 0 and i[-1] < S * bench.H * bench.W * 3
    assert (p == np.round(p)).all() and p.min() >= 0 and p.max() <= 255 and p.std() > 1


def test_dump_is_reproducible(runs, capfd):
    """The same arguments: the same inputs, so the same outputs -- here from
    the same schedule issued eagerly instead of by the native launch list,
    and from plain sequential step() calls (whose results the pipeline
    reproduces exactly: test_engine_gpu)."""
    _, a = _run(runs, capfd, "native")
    for mode in ("eager", "sequential"):
        _, b = _run(runs, capfd, mode, "--exec", mode)
        for n in NAMES:
            np.testing.assert_array_equal(a[n], b[n], err_msg=f"{mode}: {n}")


def test_long_run_holds_a_bounded_frame_pool(runs, capfd, monkeypatch):
    """More steps than bench.FRAME_POOL: the run generates FRAME_POOL frames
    and plays them back and forth, and the schedule's steps share FRAME_POOL
    proc buffers -- the results stay those of sequential step() calls over
    the same frames, and the proc sample is the last step's."""
    import bench
    monkeypatch.setattr(bench, "FRAME_POOL", 6)
    pool = bench.FramePool(list(range(6)))
    assert [pool[i] for i in range(13)] == [0, 1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2]
    d, a = _run(runs, capfd, "long", "--steps", "20")
    _, b = _run(runs, capfd, "long_seq", "--steps", "20", "--exec", "sequential")
    assert d["steps"] == 20 and abs(d["ms_per_step"] - d["elapsed_s"] / 20 * 1e3) < 1e-3
    for n in NAMES:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
    assert a["det_count"].sum() > 0

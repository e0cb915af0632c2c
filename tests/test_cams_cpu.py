"""Per-camera ground projectors, the parts that need no GPU: the table
layout, pack_cam_table, geometry.cameras parsing, rank_cameras, the argument
checks of the three *_cams entries (they return before any HIP call) and the
recorded-schedule tables of the two new ops."""
import copy
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import cams_common as cc
from conftest import REPO

HEADER = os.path.join(REPO, "include", "rvhip.h")
IMG = [[560, 1000], [1360, 1000], [1160, 620], [760, 620]]
WLD = [[-3.5, 5.0], [3.5, 5.0], [3.5, 30.0], [-3.5, 30.0]]


def _header_int(name):
    m = re.search(r"#define %s (\d+)" % name, open(HEADER).read())
    assert m, name
    return int(m.group(1))


def test_layout_matches_header():
    from rvs_amd import geometry
    nbytes = _header_int("RV_CAM_PROJ_BYTES")
    dt = geometry.CAM_PROJ_DTYPE
    assert nbytes == 96 == geometry.RV_CAM_PROJ_BYTES == dt.itemsize

    class C(ctypes.Structure):  # the header's struct, field by field
        _fields_ = [("H", ctypes.c_double * 9), ("max_distance", ctypes.c_double),
                    ("origin", ctypes.c_float * 2), ("enabled", ctypes.c_int32),
                    ("reserved", ctypes.c_int32)]
    assert ctypes.sizeof(C) == nbytes
    for name, _ in C._fields_:
        assert dt.fields[name][1] == getattr(C, name).offset, name
    assert dt.fields["H"][0].shape == (9,) and dt.fields["H"][0].base == np.float64
    assert dt.fields["origin"][0].shape == (2,) and dt.fields["origin"][0].base == np.float32
    assert dt.fields["enabled"][0] == np.int32 and dt.fields["max_distance"][0] == np.float64


def test_pack_cam_table_round_trip():
    from rvs_amd.geometry import pack_cam_table
    projs = [cc.device_projector(c) for c in cc.CAMS]
    tab = pack_cam_table(projs)
    assert tab.shape == (cc.S,) and tab.nbytes == cc.S * 96
    raw = tab.view(np.uint8).reshape(cc.S, 96)
    for s, spec in enumerate(cc.CAMS):
        H = raw[s, :72].view(np.float64)
        md = raw[s, 72:80].view(np.float64)[0]
        origin = raw[s, 80:88].view(np.float32)
        enabled, reserved = raw[s, 88:96].view(np.int32)
        assert reserved == 0
        if spec is None:
            assert enabled == 0 and md == -1.0 and not H.any() and not origin.any()
            continue
        assert enabled == 1
        np.testing.assert_array_equal(H, np.asarray(spec[0], np.float64).ravel())
        np.testing.assert_array_equal(origin, np.asarray(spec[1], np.float32))
        assert md == (-1.0 if spec[2] is None else spec[2])
    assert tab["max_distance"][2] == -1.0  # max_distance=None
    assert pack_cam_table([]).shape == (0,)


def _cfg(n_cameras=None):
    from rvs_amd.config import load_config
    cfg = copy.deepcopy(load_config())
    cfg["detect"]["enabled"] = False
    cfg["geometry"]["enabled"] = True
    cfg["geometry"]["projector"]["image_points"] = IMG
    cfg["geometry"]["projector"]["world_points"] = WLD
    if n_cameras is not None:
        cam = {"type": "homography", "image_points": IMG, "world_points": WLD,
               "origin": [1.0, 2.0], "max_distance": 40.0}
        cfg["geometry"]["cameras"] = [copy.deepcopy(cam) for _ in range(n_cameras)]
    return cfg


def test_config_cameras_win_over_projector_and_null_entries():
    from rvs_amd.engine import RoadVisionEngine
    cfg = _cfg(3)
    cfg["geometry"]["cameras"][1] = None
    cfg["geometry"]["cameras"][2]["max_distance"] = None
    eng = RoadVisionEngine(cfg, 3, (64, 64), device="cpu")
    assert eng.projector is None and len(eng.projectors) == 3
    assert eng.projectors[1] is None
    H, origin, md = eng.projectors[0].device_params()
    assert md == 40.0 and list(origin) == [1.0, 2.0]
    assert eng.projectors[2].device_params()[2] == -1.0
    # the same mapping as geometry.projector builds the same homography
    from rvs_amd.geometry import build_projector
    np.testing.assert_array_equal(H, build_projector(cfg["geometry"]).device_params()[0])


def test_config_cameras_yaml_round_trip(tmp_path):
    """geometry.cameras as a user writes it: a YAML list with a null entry."""
    import yaml
    from rvs_amd.config import load_config
    from rvs_amd.geometry import build_camera_projectors
    cam = {"type": "homography", "image_points": IMG, "world_points": WLD}
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump({"geometry": {"enabled": True, "cameras": [cam, None]}}))
    geom = load_config(str(p))["geometry"]
    projs = build_camera_projectors(geom, 2)
    assert projs[1] is None and projs[0].device_params()[2] == -1.0
    assert list(projs[0].device_params()[1]) == [0.0, 0.0]


def test_config_camera_that_fails_to_build_warns_and_is_none():
    from rvs_amd.engine import RoadVisionEngine
    cfg = _cfg(2)
    cfg["geometry"]["cameras"][0]["image_points"] = [[0, 0], [1, 1]]
    with pytest.warns(UserWarning, match="camera 0.*at least 4 image points"):
        eng = RoadVisionEngine(cfg, 2, (64, 64), device="cpu")
    assert eng.projectors[0] is None and eng.projectors[1] is not None
    cfg = _cfg(2)
    cfg["geometry"]["cameras"][1]["type"] = "lidar"
    with pytest.warns(UserWarning, match="camera 1.*unknown projector type"):
        eng = RoadVisionEngine(cfg, 2, (64, 64), device="cpu")
    assert eng.projectors == [eng.projectors[0], None] and eng.projectors[0] is not None


def test_config_cameras_wrong_length_raises():
    from rvs_amd.engine import RoadVisionEngine
    with pytest.raises(ValueError, match="cameras"):
        RoadVisionEngine(_cfg(2), 3, (64, 64), device="cpu")
    with pytest.raises(ValueError, match="projectors"):
        RoadVisionEngine(_cfg(), 3, (64, 64), device="cpu", projectors=[None, None])


def test_without_cameras_the_projector_is_todays():
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.geometry import build_projector
    cfg = _cfg()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng = RoadVisionEngine(cfg, 2, (64, 64), device="cpu")
    assert eng.projectors is None
    np.testing.assert_array_equal(eng.projector.device_params()[0],
                                  build_projector(cfg["geometry"]).device_params()[0])
    # cameras are read only when geometry.enabled
    cfg = _cfg(2)
    cfg["geometry"]["enabled"] = False
    eng = RoadVisionEngine(cfg, 2, (64, 64), device="cpu")
    assert eng.projectors is None and eng.projector is None


def test_rank_cameras_against_partition():
    from rvs_amd.shard import partition, rank_cameras
    cams = [f"cam{i}" for i in range(256)]
    parts = partition(256, 8)
    got = [rank_cameras(cams, 32, r) for r in range(8)]
    for r, ids in enumerate(parts):
        assert got[r] == [cams[i] for i in ids] and len(got[r]) == 32
    assert sum(got, []) == cams
    with pytest.raises(ValueError, match="cameras"):
        rank_cameras(cams[:255], 32, 7)
    with pytest.raises(ValueError):
        rank_cameras(cams, 32, -1)


def test_argument_errors_of_the_cams_entries():
    """Bad arguments return RV_EINVAL with a text before any HIP call."""
    from rvs_amd import _lib
    lib = _lib.load()
    assert lib.rv_abi_version() >= 9
    p = ctypes.c_void_p
    ok = 4096  # any non-null, 8-byte aligned value: never dereferenced here

    def sort(**kw):
        a = dict(si=ok, so=ok, S=2, tmax=8, dets=ok, dc=ok, dmax=4, ts=ok, par=ok, cams=ok,
                 ws=ok, wsb=1 << 30, oi=ok, od=ok, osp=ok)
        a.update(kw)
        return lib.rv_sort_update_cams(p(a["si"]), p(a["so"]), a["S"], a["tmax"], p(a["dets"]),
                                       p(a["dc"]), a["dmax"], p(a["ts"]), p(a["par"]),
                                       p(a["cams"]), p(a["ws"]), a["wsb"], p(a["oi"]),
                                       p(a["od"]), p(a["osp"]), None)
    assert sort(si=None) == -1000 and b"null" in lib.rv_last_error()
    assert sort(dets=None) == -1000 and b"null" in lib.rv_last_error()
    assert sort(par=None) == -1000
    assert sort(S=0) == -1000 and b"sizes" in lib.rv_last_error()
    assert sort(dmax=5000) == -1000
    assert sort(wsb=16) == -1000 and b"workspace" in lib.rv_last_error()
    assert sort(cams=ok + 4) == -1000 and b"aligned" in lib.rv_last_error()

    def untracked(dets=ok, n=ok, S=2, dmax=4, cams=ok, oi=ok, od=ok, osp=ok):
        return lib.rv_untracked_metrics_cams(p(dets), p(n), S, dmax, p(cams), p(oi), p(od),
                                             p(osp), None)
    assert untracked(dets=None) == -1000 and b"null" in lib.rv_last_error()
    assert untracked(od=None) == -1000
    assert untracked(S=-1) == -1000 and b"shape" in lib.rv_last_error()
    assert untracked(dmax=0) == -1000
    assert untracked(cams=ok + 2) == -1000 and b"aligned" in lib.rv_last_error()
    assert untracked(S=0) == 0  # nothing to do, nothing launched

    def project(cams=ok, S=2, boxes=ok, cam=ok, n=3, xy=ok, dist=ok):
        return lib.rv_homography_project_cams(p(cams), S, p(boxes), p(cam), n, p(xy), p(dist),
                                              None)
    assert project(cams=None) == -1000 and b"null" in lib.rv_last_error()
    assert project(cam=None) == -1000
    assert project(xy=None) == -1000
    assert project(S=0) == -1000 and b"shape" in lib.rv_last_error()
    assert project(n=-1) == -1000
    assert project(cams=ok + 4) == -1000 and b"aligned" in lib.rv_last_error()
    assert project(n=0, boxes=None, cam=None) == 0


def test_schedule_tables_of_the_new_ops_agree():
    from rvs_amd import _lib, schedule
    hdr = open(HEADER).read()
    ids = {m.group(1): (int(m.group(2)), m.group(3)) for m in
           re.finditer(r"#define (RV_SCHED_\w+) (\d+)\s*/\* (rv_\w+) \*/", hdr)}
    assert ids["RV_SCHED_SORT_UPDATE_CAMS"] == (9, "rv_sort_update_cams")
    assert ids["RV_SCHED_UNTRACKED_CAMS"] == (10, "rv_untracked_metrics_cams")
    assert _header_int("RV_SCHED_NUM_OPS") == 11 == len(schedule._OPS)
    src = open(os.path.join(REPO, "road-vision-system_amd", "csrc", "sched.hip")).read()
    specs = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in
             re.finditer(r"/\* (RV_SCHED_\w+) \*/ \{(\d+), (\d+)\}", src)}
    for macro, (op, name) in ids.items():
        if not macro.endswith("_CAMS"):
            continue
        assert re.search(r"case %s:" % macro, src), macro
        pop, si, host = schedule._OPS[name]
        assert pop == op and name in _lib._RECORDABLE
        argtypes = _lib._SIGS[name][1]
        assert argtypes[si] is ctypes.c_void_p and si == len(argtypes) - 1
        assert specs[macro] == (len(argtypes) - 1, 0), macro  # no float-class argument
    # cams is a device pointer: an integer slot, not a host array copied at record time
    assert schedule._OPS["rv_sort_update_cams"][2] == {8: 48}
    assert schedule._OPS["rv_untracked_metrics_cams"][2] == {}


def test_common_input_is_not_vacuous():
    cc.check_non_vacuous()
    ora = cc.oracle()
    n0 = sum(len(r[0]) for r in ora[0])
    nd0 = sum(int((~np.isnan(r[1])).sum()) for r in ora[0])
    assert (n0, nd0) == (74, 73)

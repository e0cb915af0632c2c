"""Shared by the overlay tests: the goldens of tests/golden/overlay (the
reference's drawing code over tests/cv2_standin.py, make_overlay_golden.py),
read once and never written."""
import functools
import os

import numpy as np

from conftest import GOLDEN

ODIR = os.path.join(GOLDEN, "overlay")


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(ODIR, "cases.npz"))
    out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def draw_cases():
    return sorted(k[:-len("/thickness")] for k in golden() if k.endswith("/thickness"))


def canvas_cases():
    return sorted(k[:-len("/layout")] for k in golden() if k.endswith("/layout"))


def background(case):
    g = golden()
    return g["bg_%dx%d" % tuple(g[case + "/hw"])]


def raw_frame(case):
    g = golden()
    return g["raw_%dx%d" % tuple(g[case + "/hw"])]


def detections(case):
    """The case's inputs as the package's Detection list."""
    from rvs_amd.detect.types import Detection
    g = golden()
    out = []
    for r, name, tid, dist, spd in zip(g[case + "/dets"], g[case + "/names"], g[case + "/track_id"],
                                       g[case + "/distance_m"], g[case + "/speed_kmh"]):
        out.append(Detection(float(r[0]), float(r[1]), float(r[2]), float(r[3]), float(r[4]),
                             int(r[5]), str(name), None if tid < 0 else int(tid),
                             None if np.isnan(dist) else float(dist),
                             None if np.isnan(spd) else float(spd)))
    return out


def params(case):
    g = golden()
    return int(g[case + "/thickness"]), float(g[case + "/font_scale"])


def canvas_params(case):
    g = golden()
    fps = float(g[case + "/fps"])
    return dict(layout=str(g[case + "/layout"]), divider_px=int(g[case + "/divider_px"]),
                label_raw=str(g[case + "/labels"][0]), label_proc=str(g[case + "/labels"][1]),
                fps=None if np.isnan(fps) else fps), str(g[case + "/case"])

"""Generate the overlay goldens from the REFERENCE's own drawing code (run
where /root/reference is mounted read-only and Pillow is installed).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_overlay_golden.py

tests/cv2_standin.py is put in sys.modules["cv2"], and the reference's
src/vis/draw.py and main_preview.py are imported unmodified: which detections
are drawn, their order, colours, label strings and every coordinate come from
the reference; only cv2.rectangle / getTextSize / putText are the stand-in's
raster model (include/rvhip.h, "Detection overlays").  main_preview imports
the whole application at module level; every module it cannot import here
(the detector's and tracker's third-party packages, cv2-backed capture) gets
an empty stand-in that make_canvas never calls into.

Output, data only: tests/golden/overlay/font.npz (Pillow's built-in bitmap
font, written first because the stand-in draws with it) and
tests/golden/overlay/cases.npz (inputs and the reference's images).
"""
import importlib
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.dont_write_bytecode = True
sys.path.insert(0, TESTS)

import numpy as np  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "overlay")


def write_font():
    from PIL import ImageFont
    font = ImageFont.load_default_imagefont()
    rows = np.zeros((95, 11), np.uint8)
    for c in range(32, 127):
        m = font.getmask(chr(c))
        assert m.size == (6, 11), (c, m.size)
        a = np.array(m, np.uint8).reshape(11, 6)
        assert set(np.unique(a)) <= {0, 255}
        for r in range(11):
            rows[c - 32, r] = sum(1 << (5 - x) for x in range(6) if a[r, x])
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "font.npz"), rows=rows)


def import_reference():
    import cv2_standin
    sys.modules["cv2"] = cv2_standin
    sys.path.insert(0, REF)
    for _ in range(64):  # a stand-in for every module the application cannot import here
        try:
            draw = importlib.import_module("src.vis.draw")
            preview = importlib.import_module("main_preview")
            break
        except ImportError as exc:
            while not getattr(exc, "name", None) and exc.__cause__ is not None:
                exc = exc.__cause__  # sort_tracker.py re-raises filterpy's ImportError
            if not getattr(exc, "name", None) or exc.name.startswith("src") or \
                    exc.name == "main_preview":
                raise
            mod = types.ModuleType(exc.name)
            mod.__path__ = []
            mod.__getattr__ = lambda name: type(name, (), {})
            sys.modules[exc.name] = mod
            for k in [k for k in sys.modules if k.startswith("src") or k == "main_preview"]:
                del sys.modules[k]
    else:
        raise RuntimeError("could not import the reference")
    from src.detect.types import Detection
    return draw, preview, Detection


def background(h, w, seed):
    """Four-level noise: any pixel left uncovered, or covered wrongly, shows,
    and the file stays small."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 4, (h, w, 3)) * 60 + 17).astype(np.uint8)


def f32(v):
    return float(np.float32(v))


# (x1, y1, x2, y2, conf, cls_id, cls_name, track_id, distance_m, speed_kmh)
def det(x1, y1, x2, y2, conf, cls, name, tid=None, dist=None, spd=None):
    return (f32(x1), f32(y1), f32(x2), f32(y2), f32(conf), int(cls), name, tid, dist, spd)


A, B, C = (37, 91), (64, 96), (72, 136)
LONG = "articulated-lorry-with-trailers"  # 31 characters
assert len(LONG) == 31

DRAW_CASES = {
    # boxes on every image edge and beyond it, thin lines, smallest glyphs
    "edges_t1_k1": (A, 1, 0.3, [
        det(0, 0, 20.9, 12.2, 0.875, 0, "person", 1, 3.25, None),
        det(70.5, 5, 90, 20, 0.5, 2, "car"),
        det(30, 25.7, 60, 36, 0.125, 3, "motorcycle", None, None, 12.35),
        det(-5.5, -3.2, 10, 8, 0.995, 5, "bus", 7, 0.05, 0.25),
        det(85, 30, 95.5, 40, 0.375, 7, "truck"),
    ]),
    # top label clamped at the top, bottom label clamped at the bottom, text off the right edge
    "clamps_t2_k2": (B, 2, 0.6, [
        det(4, 5, 40, 30, 0.66, 2, "car", 12, 10.0, 36.6),
        det(50, 30, 90, 60, 0.71, 7, "truck", 2147483647, 999.95, -0.04),
        det(70, 40, 94, 63.9, 0.3, 0, "person", None, 2.675, None),
    ]),
    # a later detection covers an earlier label; a degenerate box between two valid ones
    "overlap_t3_k1": (B, 3, 0.3, [
        det(10, 20, 50, 50, 0.9, 13, "", 3, 5.5, 20.0),
        det(30, 30, 30.5, 40, 0.8, 2, "car", 4, 1.0, 1.0),
        det(40, 45, 20, 60, 0.8, 2, "car", 5, 1.0, 1.0),
        det(8, 12, 60, 40, 0.45, 27, "voiture électrique", None, None, 88.85),
    ]),
    "big_t5_k3": (C, 5, 1.0, [
        det(20, 40, 100, 60, 1.0, 1, "bicycle", 0, 0.35, None),
        det(60.2, 10.9, 130, 35, 0.0, 11, LONG, 42, None, None),
    ]),
    "names_t2_k1": (C, 2, 0.3, [
        det(2, 30, 134, 50, 0.005, 9, LONG, 2147483647, 123456.75, 250.25),
        det(40, 52, 90, 66, 0.55, 10, "café 猫", 8, 1e9 - 0.04, -12.25),
        det(100, 2, 120, 20, 0.25, 4, "", None, 7.0, None),
    ]),
    "empty": (A, 2, 0.6, []),
    # third cases of the two smaller frames, for batches of three different streams
    "mixed_t1_k2": (B, 1, 0.6, [
        det(20, 28, 70, 44, 0.5, 6, "train", 9, None, 3.05),
        det(0, 50, 95, 63, 0.95, 0, "person", None, 0.15, None),
    ]),
    "small_frame_t3_k2": (A, 3, 0.6, [
        det(10, 12, 80, 30, 0.33, 5, "bus", 21, 15.0, 50.05),
        det(60, 2, 89.5, 36.5, 0.6, 15, "", None, None, None),
    ]),
}

# (frame, layout, divider_px, fps, label_raw, label_proc, draw case whose detections go on proc)
CANVAS_CASES = {
    "h_d4_fps": (B, "h", 4, 23.456, "RAW", "PROC", "clamps_t2_k2"),
    "h_d0": (B, "h", 0, None, "RAW", "PROC", None),
    "v_d4": (B, "v", 4, None, "RAW", "PROC", "overlap_t3_k1"),
    "v_d0_fps": (A, "v", 0, 9.95, "IN", "OUT", "edges_t1_k1"),
    "h_d3_odd": (A, "h", 3, 30.0, "RAW", "PROC", "edges_t1_k1"),
}


def main():
    write_font()
    draw, preview, Detection = import_reference()
    out = {}
    seeds = {A: 1, B: 2, C: 3}
    for hw in (A, B, C):
        out["bg_%dx%d" % hw] = background(hw[0], hw[1], seeds[hw])
        out["raw_%dx%d" % hw] = background(hw[0], hw[1], 10 + seeds[hw])

    def detections(rows):
        return [Detection(*r) for r in rows]

    for name, (hw, t, fs, rows) in DRAW_CASES.items():
        img = out["bg_%dx%d" % hw].copy()
        draw.draw_detections(img, detections(rows), thickness=t, font_scale=fs)
        n = len(rows)
        out[name + "/hw"] = np.array(hw, np.int32)
        out[name + "/thickness"] = np.int32(t)
        out[name + "/font_scale"] = np.float64(fs)
        out[name + "/dets"] = np.array([r[:6] for r in rows], np.float64).reshape(n, 6)
        out[name + "/names"] = np.array([r[6] for r in rows], dtype="U40")
        out[name + "/track_id"] = np.array([-1 if r[7] is None else r[7] for r in rows], np.int64)
        out[name + "/distance_m"] = np.array([np.nan if r[8] is None else r[8] for r in rows],
                                             np.float64)
        out[name + "/speed_kmh"] = np.array([np.nan if r[9] is None else r[9] for r in rows],
                                            np.float64)
        out[name + "/image"] = img
    for name, (hw, layout, d, fps, lr, lp, case) in CANVAS_CASES.items():
        raw = out["raw_%dx%d" % hw]
        proc = out["bg_%dx%d" % hw].copy()
        if case is not None:
            chw, t, fs, rows = DRAW_CASES[case]
            assert chw == hw
            draw.draw_detections(proc, detections(rows), thickness=t, font_scale=fs)
        canvas = preview.make_canvas(raw, proc, layout=layout, divider_px=d, label_raw=lr,
                                     label_proc=lp, fps=fps, show_fps=True)
        out["canvas_" + name + "/hw"] = np.array(hw, np.int32)
        out["canvas_" + name + "/layout"] = np.array(layout)
        out["canvas_" + name + "/divider_px"] = np.int32(d)
        out["canvas_" + name + "/fps"] = np.float64(np.nan if fps is None else fps)
        out["canvas_" + name + "/labels"] = np.array([lr, lp])
        out["canvas_" + name + "/case"] = np.array(case or "")
        out["canvas_" + name + "/image"] = np.ascontiguousarray(canvas)
    np.savez_compressed(os.path.join(OUT, "cases.npz"), **out)
    size = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("wrote", OUT, size, "bytes")


if __name__ == "__main__":
    main()

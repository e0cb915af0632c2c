"""Detection overlays, host side: the raster model of tests/cv2_standin.py
pixel by pixel, the font table of csrc/overlay_font.h against its fixture and
Pillow, the package's display-list builder against the reference's images
(tests/golden/overlay), and preview.record.content.  No GPU calls."""
import os
import re

import numpy as np
import pytest

import cv2_standin as cv2s
import overlay_common as oc
from conftest import PKG

C = (9, 8, 7)


def _img(h=8, w=8):
    return np.zeros((h, w, 3), np.uint8)


def _mask(img):
    return (img == np.array(C, np.uint8)).all(-1)


def _rows(*rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


def test_outline_t1_is_the_one_pixel_frame():
    img = _img()
    cv2s.rectangle(img, (2, 1), (5, 4), C, 1)
    assert np.array_equal(_mask(img), _rows("........",
                                            "..####..",
                                            "..#..#..",
                                            "..#..#..",
                                            "..####..",
                                            "........",
                                            "........",
                                            "........"))


def test_outline_t2_grows_up_and_left():
    """t = 2: a = 1, b = 0, each edge at c covers c-1 .. c."""
    img = _img()
    cv2s.rectangle(img, (2, 2), (6, 5), C, 2)
    assert np.array_equal(_mask(img), _rows("........",
                                            ".######.",
                                            ".######.",
                                            ".##..##.",
                                            ".######.",
                                            ".######.",
                                            "........",
                                            "........"))


def test_outline_t3_is_centred_and_clipped():
    """t = 3: a = b = 1; the frame of (1,1)-(6,6) reaches the image edge."""
    img = _img()
    cv2s.rectangle(img, (1, 1), (6, 6), C, 3)
    assert np.array_equal(_mask(img), _rows("########",
                                            "########",
                                            "########",
                                            "###..###",
                                            "###..###",
                                            "########",
                                            "########",
                                            "########"))
    img = _img()
    cv2s.rectangle(img, (-1, 5), (3, 9), C, 3)  # mostly outside: nothing is written out of bounds
    assert np.array_equal(_mask(img), _rows("........",
                                            "........",
                                            "........",
                                            "........",
                                            "#####...",
                                            "#####...",
                                            "#####...",
                                            "#.###..."))


def test_filled_rectangle_is_inclusive_and_order_free():
    a, b = _img(), _img()
    cv2s.rectangle(a, (1, 2), (3, 3), C, -1)
    cv2s.rectangle(b, (3, 3), (1, 2), C, -1)
    assert np.array_equal(a, b) and _mask(a).sum() == 6 and _mask(a)[2:4, 1:4].all()


# Pillow's "A" cell: rows 3..8 above the baseline
A_CELL = _rows("......",
               "......",
               "......",
               "####..",
               ".###..",
               ".#.#..",
               "#####.",
               "##.##.",
               "##.###",
               "......",
               "......")


def test_one_glyph_k1():
    """Origin (1, 9): cell row r is y = oy - 9 + 1 + r, so row 8 ends at y = oy."""
    img = _img(12, 8)
    cv2s.putText(img, "A", (1, 9), cv2s.FONT_HERSHEY_SIMPLEX, 0.3, C, 1, cv2s.LINE_AA)
    want = np.zeros((12, 8), bool)
    want[1:12, 1:7] = A_CELL
    assert np.array_equal(_mask(img), want)
    assert cv2s.getTextSize("A", 0, 0.3, 1) == ((6, 9), 2)


def test_one_glyph_k2_paints_2x2_blocks():
    img = _img(24, 14)
    cv2s.putText(img, "A", (1, 18), cv2s.FONT_HERSHEY_SIMPLEX, 0.6, C, 1)
    want = np.zeros((24, 14), bool)
    want[1:23, 1:13] = np.kron(A_CELL, np.ones((2, 2), bool))
    assert np.array_equal(_mask(img), want)
    assert cv2s.getTextSize("AB", 0, 0.6, 3) == ((24, 18), 4)


def test_thickness_2_dilates_right_and_down():
    """t = 2: shifts dx, dy in [0, 1]; '.' is two pixels of cell row 8."""
    img = _img(12, 8)
    cv2s.putText(img, ".", (0, 9), 0, 0.3, C, 2)
    thin = _img(12, 8)
    cv2s.putText(thin, ".", (0, 9), 0, 0.3, C, 1)
    m = _mask(thin)
    want = m.copy()
    want[:, 1:] |= m[:, :-1]
    want[1:, :] |= want[:-1, :].copy()
    assert np.array_equal(_mask(img), want) and m.sum() * 2 < want.sum()
    # t = 3 is centred: one pixel on every side
    img3 = _img(12, 8)
    cv2s.putText(img3, ".", (0, 9), 0, 0.3, C, 3)
    ys, xs = np.nonzero(m)
    want3 = np.zeros_like(m)
    want3[ys.min() - 1:ys.max() + 2, max(0, xs.min() - 1):xs.max() + 2] = True
    assert np.array_equal(_mask(img3), want3)


def test_bytes_outside_ascii_are_question_marks():
    a, b = _img(12, 20), _img(12, 20)
    cv2s.putText(a, "é\x07", (0, 9), 0, 0.3, C, 1)  # two UTF-8 bytes and a control byte
    cv2s.putText(b, "???", (0, 9), 0, 0.3, C, 1)
    assert np.array_equal(a, b)


def _header_table():
    txt = open(os.path.join(PKG, "csrc", "overlay_font.h")).read()
    body = txt[txt.index("RV_OVERLAY_FONT_TABLE"):]
    vals = [int(v, 16) for v in re.findall(r"0x([0-9a-fA-F]{2})", body)]
    return np.array(vals, np.uint8).reshape(95, 11)


def test_font_header_equals_the_fixture():
    assert np.array_equal(_header_table(), cv2s.font_rows())
    assert int(cv2s.font_rows().max()) < 64  # six columns


def test_font_fixture_equals_pillow():
    ImageFont = pytest.importorskip("PIL.ImageFont")
    font = ImageFont.load_default_imagefont()
    rows = cv2s.font_rows()
    for c in range(32, 127):
        m = font.getmask(chr(c))
        assert m.size == (6, 11)
        a = np.array(m, np.uint8).reshape(11, 6) > 0
        got = (rows[c - 32][:, None] >> (5 - np.arange(6))[None, :]) & 1
        assert np.array_equal(got.astype(bool), a), chr(c)


def test_glyph_scale():
    from rvs_amd.vis import glyph_scale
    assert [glyph_scale(f) for f in (0.3, 0.6, 0.8, 1.0, 0.01, 9.0)] == [1, 2, 3, 3, 1, 8]
    assert all(glyph_scale(f) == cv2s.glyph_scale(f) for f in np.linspace(0.05, 3.0, 60))


@pytest.mark.parametrize("case", oc.draw_cases())
def test_host_builder_equals_the_reference(case):
    """The package's display list (our restatement of draw.py), rastered by
    the stand-in, against the image the reference's draw_detections made."""
    from rvs_amd.vis import detection_list
    t, fs = oc.params(case)
    img = oc.background(case).copy()
    dl = detection_list(oc.detections(case), img.shape[0], t, fs)
    cv2s.raster_records(img, dl.records())
    assert np.array_equal(img, oc.golden()[case + "/image"])
    if case == "empty":
        assert len(dl) == 0 and np.array_equal(img, oc.background(case))


@pytest.mark.parametrize("case", oc.canvas_cases())
def test_host_canvas_equals_the_reference(case):
    from rvs_amd.vis import canvas_list, detection_list
    from rvs_amd.vis.display_list import canvas_geometry
    kw, dcase = oc.canvas_params(case)
    raw, proc = oc.raw_frame(case), oc.background(case).copy()
    h, w = proc.shape[:2]
    if dcase:
        t, fs = oc.params(dcase)
        cv2s.raster_records(proc, detection_list(oc.detections(dcase), h, t, fs).records())
    oh, ow, px, py, d = canvas_geometry(h, w, kw["layout"], kw["divider_px"])
    canvas = np.full((oh, ow, 3), 40, np.uint8)
    canvas[:h, :w] = raw
    canvas[py:py + h, px:px + w] = proc
    cv2s.raster_records(canvas, canvas_list(h, w, **kw).records())
    want = oc.golden()[case + "/image"]
    assert canvas.shape == want.shape and np.array_equal(canvas, want)


def test_host_builder_skips_none_and_takes_conf_none():
    from rvs_amd.detect.types import Detection
    from rvs_amd.vis import detection_list
    d = Detection(3.0, 20.0, 30.0, 40.0, 0.5, 2, "car", 5, 1.25, None)
    a = detection_list([None, d, None], 64).to_bytes()
    b = detection_list([d], 64).to_bytes()
    assert np.array_equal(a, b)
    d2 = Detection(3.0, 20.0, 30.0, 40.0, None, 2, "", None, None, None)
    recs = detection_list([d2], 64).records()
    assert len(recs) == 3 and bytes(recs[2]["text"][:recs[2]["len"]]) == b"2"
    assert bytes(detection_list([d], 64).records()[4]["text"][:6]) == b"1.2 m\0"  # 1.25: half to even


def test_long_text_is_split_and_names_are_bounded():
    from rvs_amd.vis import DisplayList, names_table
    dl = DisplayList()
    dl.text("x" * 70, (5, 20), 2, (1, 2, 3), 1)
    recs = dl.records()
    assert [int(r["len"]) for r in recs] == [64, 6] and int(recs[1]["x0"]) == 5 + 12 * 64
    assert names_table(["a" * 31]).shape == (1, 32)
    with pytest.raises(ValueError):
        names_table(["a" * 32])
    assert bytes(names_table({1: "car"}, 3)[1, :4]) == b"car\0"


def _cfg(**record):
    from rvs_amd.config import load_config
    cfg = load_config()
    cfg["preview"]["record"] = dict(cfg["preview"]["record"], enable=True, path="o{stream}.mjpeg",
                                    **record)
    return cfg


def test_record_settings_content():
    from rvs_amd.config import load_config
    from rvs_amd.io_video import record_settings
    assert load_config()["preview"]["record"]["content"] == "proc"
    assert "content" not in record_settings(_cfg(), 2)  # the default: today's settings
    assert "content" not in record_settings(_cfg(content="proc"), 2)
    for content in ("annotated", "compare"):
        assert record_settings(_cfg(content=content), 2)["content"] == content
    for bad in ("canvas", "", None, 1):
        with pytest.raises(ValueError, match="content"):
            record_settings(_cfg(content=bad), 2)
    cfg = _cfg(content="raw")
    cfg["preview"]["record"]["enable"] = False
    assert record_settings(cfg, 2) is None  # off: nothing is checked, as for the path

"""The host half of the JPEG encoder (rv_jpeg_quant_tables,
rv_jpeg_write_header, rv_jpeg_encode_coef) against files Pillow wrote, and the
handling of preview.record in the configuration.  No GPU calls."""
import ctypes
import glob
import os
import types

import numpy as np
import pytest

import jpeg_ref
from conftest import GOLDEN

JDIR = os.path.join(GOLDEN, "jpeg")
EDIR = os.path.join(GOLDEN, "jpeg_enc")
# stills that use the Annex K Huffman tables, written out in full
OLD = sorted(p for p in glob.glob(os.path.join(JDIR, "*.jpg"))
             if not any(t in os.path.basename(p) for t in ("_opt", "_nodht", "reject_")))
NEW = sorted(glob.glob(os.path.join(EDIR, "*.jpg")))
RV_EINVAL = -1000


def _restart_interval(data):
    segs, _ = jpeg_ref.segments(data)
    ri = [(data[o] << 8) | data[o + 1] for m, o, n in segs if m == 0xDD]
    return ri[0] if ri else 0


def _encode_coef(rec, ri, cap):
    from rvs_amd import _lib
    out = np.full(cap + 8, 0xA5, np.uint8)
    n = ctypes.c_size_t(0)
    st = _lib.load().rv_jpeg_encode_coef(rec.ctypes.data, rec.size, ri, out.ctypes.data, cap,
                                         ctypes.addressof(n))
    assert (out[cap:] == 0xA5).all(), "bytes behind the capacity were written"
    return st, out[:min(n.value, cap)].tobytes(), n.value


def test_the_fixture_sets_are_there():
    assert len(OLD) >= 30 and len(NEW) == 33
    names = " ".join(os.path.basename(p) for p in NEW)
    for shape in ("1x1", "8x8", "16x16", "17x33", "24x24", "37x91", "9x250", "130x24", "72x136",
                  "9x1100"):
        for s in ("444", "422", "420"):
            assert f"{shape}_{s}_" in names
    assert any("gray" in p for p in OLD) and any("rst2" in p for p in OLD)
    z = np.load(os.path.join(EDIR, "input.npz"))
    assert {n + ".jpg" for n in z.files if not n.startswith("clip_")} == \
        {os.path.basename(p) for p in NEW}
    clip = open(os.path.join(EDIR, "clip_40x56_420_q90.mjpeg"), "rb").read()
    assert len(jpeg_ref.split_frames(clip)) == 5 and z["clip_40x56_420_q90"].shape == (5, 40, 56, 3)


@pytest.mark.parametrize("path", OLD + NEW, ids=os.path.basename)
def test_encode_of_decode_is_the_file(path):
    """rv_jpeg_encode_coef(rv_jpeg_decode_coef(file), the file's restart
    interval) == file: header, Huffman coding, stuffing, padding, RSTm, EOI."""
    from rvs_amd.io_video import jpeg_coefficients
    data = open(path, "rb").read()
    rec = jpeg_coefficients(data)
    st, got, n = _encode_coef(rec, _restart_interval(data), len(data))
    assert st == 0 and n == len(data)
    assert got == data


def test_encode_coef_refuses_what_it_cannot_write():
    from rvs_amd import _lib
    from rvs_amd.io_video import jpeg_coefficients
    lib = _lib.load()
    data = open(os.path.join(EDIR, "17x33_422_q75_noise.jpg"), "rb").read()
    rec = jpeg_coefficients(data)
    ri = _restart_interval(data)
    st, _, n = _encode_coef(rec, ri, len(data) - 1)      # one byte short
    assert st == RV_EINVAL and n == len(data) and b"bytes" in lib.rv_last_error()
    st, _, _ = _encode_coef(rec, ri, 0)
    assert st == RV_EINVAL
    bad = rec.copy()
    bad[:4] = 0
    assert _encode_coef(bad, ri, len(data))[0] == RV_EINVAL
    assert b"record" in lib.rv_last_error()
    lay = __import__("rvs_amd.io_video", fromlist=["x"]).jpeg_record_layout(33, 17, 1)
    big = rec.copy()
    big[lay["coef_offset"][0] + 2:lay["coef_offset"][0] + 4] = (0x7F, 0x7F)  # an AC value of 32639
    assert _encode_coef(big, ri, 1 << 16)[0] == RV_EINVAL
    assert b"no baseline code" in lib.rv_last_error()
    assert _encode_coef(rec[:rec.size - 16].copy(), ri, len(data))[0] == RV_EINVAL
    # without a restart interval the same record still decodes to itself
    st, plain, n = _encode_coef(rec, 0, len(data))
    assert st == 0 and b"\xff\xdd" not in plain[:700]
    np.testing.assert_array_equal(jpeg_coefficients(plain), rec)


@pytest.mark.parametrize("q", [1, 25, 49, 50, 51, 75, 95, 100])
def test_quant_tables_and_header_equal_pillows(q):
    from rvs_amd import _lib
    from rvs_amd.kernels import jpeg_file_header
    lib = _lib.load()
    want = np.load(os.path.join(EDIR, "dqt.npz"))[f"q{q}"]
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    assert lib.rv_jpeg_quant_tables(q, luma.ctypes.data, chroma.ctypes.data) == 0
    for t, tab in enumerate((luma, chroma)):
        assert want[t, 0] == t
        np.testing.assert_array_equal(tab[jpeg_ref.ZIGZAG], want[t, 1:])
    hdr = jpeg_file_header(8, 8, "420", q, 1)
    segs, end = jpeg_ref.segments(hdr + b"\x00")
    assert end == len(hdr)
    got = [hdr[o:o + n] for m, o, n in segs if m == 0xDB]
    assert got == [want[0].tobytes(), want[1].tobytes()]


def test_quality_and_sampling_are_checked():
    from rvs_amd import _lib
    lib = _lib.load()
    t = np.zeros(64, np.uint16)
    for q in (0, 101, -5):
        assert lib.rv_jpeg_quant_tables(q, t.ctypes.data, t.ctypes.data) == RV_EINVAL
    assert lib.rv_jpeg_stream_bound(16, 16, 3) == 0 and lib.rv_jpeg_stream_bound(0, 16, 2) == 0
    # the bound of rvhip.h: 16 + 640 + blocks x 416 + MCU rows x 4 + 2, rounded up to 16
    raw = 16 + 640 + (12 * 8 + 2 * 6 * 4) * 416 + 4 * 4 + 2
    assert lib.rv_jpeg_stream_bound(91, 50, 2) == (raw + 15) // 16 * 16
    # grey is refused by the device entries before any launch (a non-null pointer is enough)
    st = lib.rv_jpeg_bgr_to_coef_u8(16, 1, 8, 8, 3, 75, 16, 1 << 20, None)
    assert st == RV_EINVAL and b"4:4:4, 4:2:2 or 4:2:0" in lib.rv_last_error()


def _cfg(**record):
    from rvs_amd.config import load_config
    cfg = load_config()
    cfg["preview"]["record"] = dict(cfg["preview"]["record"], **record)
    return cfg


def test_record_settings():
    from rvs_amd.io_video import record_settings
    assert record_settings(_cfg(), 4) is None                       # the default: off
    assert record_settings(_cfg(enable=False, path="x.mp4"), 4) is None
    got = record_settings(_cfg(enable=True, path="out/cam{stream}.mjpeg"), 3)
    assert got == {"paths": ["out/cam0.mjpeg", "out/cam1.mjpeg", "out/cam2.mjpeg"],
                   "quality": 95, "sampling": "420"}
    got = record_settings(_cfg(enable=True, path="one.MJPG", quality=80, sampling="444", fps=25), 1)
    assert got == {"paths": ["one.MJPG"], "quality": 80, "sampling": "444"}


def test_engine_refuses_a_recording_it_cannot_write():
    """Raised at construction, before anything touches a device."""
    from rvs_amd.engine import RoadVisionEngine
    with pytest.raises(ValueError, match=r"Motion-JPEG \(\.mjpeg / \.mjpg\).*no MP4 muxer"):
        RoadVisionEngine(_cfg(enable=True, path="out_compare.mp4"), 1, (40, 56), device="cpu")
    with pytest.raises(ValueError, match=r"\{stream\}"):
        RoadVisionEngine(_cfg(enable=True, path="out.mjpeg"), 2, (40, 56), device="cpu")
    with pytest.raises(ValueError, match="quality"):
        RoadVisionEngine(_cfg(enable=True, path="o{stream}.mjpeg", quality=0), 2, (40, 56),
                         device="cpu")
    with pytest.raises(ValueError, match="sampling"):
        RoadVisionEngine(_cfg(enable=True, path="o{stream}.mjpeg", sampling="411"), 2, (40, 56),
                         device="cpu")


def test_pipelined_run_refuses_a_recording_engine():
    from rvs_amd.schedule import PipelinedRun
    eng = types.SimpleNamespace(recorder=object(), detector=None, pair=1)
    with pytest.raises(RuntimeError, match=r"recording runs with step\(\)"):
        PipelinedRun(eng, [], [])

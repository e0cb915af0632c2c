"""Baseline JPEG on the host (rv_jpeg_probe / rv_jpeg_decode_coef, the
RV_CAP_MJPEG reader): marker parse and Huffman decode against the numpy
restatement tests/jpeg_ref.py on the Pillow-encoded fixtures of
tests/golden/jpeg; the rejected stream kinds; truncation.  No GPU calls."""
import ctypes
import glob
import os
import time

import numpy as np
import pytest

import jpeg_ref
from conftest import GOLDEN

JDIR = os.path.join(GOLDEN, "jpeg")
STILLS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(JDIR, "*.jpg"))
                if not os.path.basename(p).startswith("reject_"))
STREAMS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(JDIR, "*.mjpeg")))
RV_EINVAL = -1000


def _data(name):
    return open(os.path.join(JDIR, name), "rb").read()


def _named(prefix):
    """The fixture whose name starts with `prefix` (shape_sampling_)."""
    return [n for n in STILLS if n.startswith(prefix)][0]


def _images(name):
    d = _data(name)
    return jpeg_ref.split_frames(d) if name.endswith(".mjpeg") else [d]


def _check_record(rec, ref):
    """A coefficient record against jpeg_ref.parse's output, through the
    layout entry (no offsets known here)."""
    from rvs_amd.io_video import jpeg_record_layout
    lay = jpeg_record_layout(ref["W"], ref["H"], ref["sampling"])
    assert lay["record_bytes"] == rec.size and lay["ncomp"] == ref["ncomp"]
    hdr = rec[:32].view(np.int32)
    assert list(hdr[1:5]) == [ref["W"], ref["H"], ref["sampling"], ref["ncomp"]]
    nc = ref["ncomp"]
    qt = rec[lay["qt_offset"]:lay["qt_offset"] + 128 * nc].view(np.uint16).reshape(nc, 64)
    np.testing.assert_array_equal(qt, ref["qt"])
    for c in range(nc):
        bh, bw = lay["blocks_h"][c], lay["blocks_w"][c]
        assert ref["coef"][c].shape == (bh, bw, 64)
        o = lay["coef_offset"][c]
        got = rec[o:o + bh * bw * 128].view(np.int16).reshape(bh, bw, 64)
        np.testing.assert_array_equal(got, ref["coef"][c])
    assert lay["coef_offset"][nc - 1] + lay["blocks_h"][nc - 1] * lay["blocks_w"][nc - 1] * 128 \
        == rec.size


def test_fixture_set_covers_the_cases():
    names = " ".join(STILLS)
    for shape in ("1x1", "8x8", "16x16", "17x33", "37x91", "48x64", "50x70", "9x250"):
        for s in ("444", "422", "420", "gray"):
            assert f"{shape}_{s}_" in names
    for tag in ("_q30_", "_q100_", "_noise", "_smooth", "_rst2", "_opt", "_nodht"):
        assert tag in names
    assert len(STREAMS) == 2
    exp = np.load(os.path.join(JDIR, "expected.npz"))
    assert set(exp.files) == set(STILLS) | set(STREAMS)
    assert b"\xff\xc4" not in _data("48x64_420_q75_nodht.jpg")[:400]


@pytest.mark.parametrize("name", STILLS + STREAMS)
def test_probe_and_coefficients_equal_the_restatement(name):
    from rvs_amd.io_video import jpeg_coefficients, jpeg_probe
    for img in _images(name):
        ref = jpeg_ref.parse(img)
        assert jpeg_probe(img) == {k: ref[k] for k in ("W", "H", "sampling", "ncomp")}
        _check_record(jpeg_coefficients(img), ref)
    if name.endswith(".jpg"):
        H, W = map(int, name.split("_")[0].split("x"))
        assert (ref["H"], ref["W"]) == (H, W)
        assert ref["sampling"] == {"444": 0, "422": 1, "420": 2, "gray": 3}[name.split("_")[1]]


def _reader(path, nbuf=3, loop=False):
    from rvs_amd.io_video.capture import RV_CAP_MJPEG, _Reader
    return _Reader(str(path), RV_CAP_MJPEG, 0, 0, nbuf, loop)


def _slot(r, ptr):
    return np.ctypeslib.as_array((ctypes.c_uint8 * r.frame_bytes).from_address(ptr)).copy()


@pytest.mark.parametrize("name", STREAMS)
def test_mjpeg_reader_hands_out_records_in_order(name):
    imgs = _images(name)
    refs = [jpeg_ref.parse(i) for i in imgs]
    r = _reader(os.path.join(JDIR, name), nbuf=2)  # fewer slots than frames: the ring wraps
    assert (r.W, r.H) == (refs[0]["W"], refs[0]["H"])
    assert r.jpeg["sampling"] == refs[0]["sampling"] and r.jpeg["record_bytes"] == r.frame_bytes
    t_prev = 0.0
    for i, ref in enumerate(refs):
        ptr, ts, idx, slot = r.next()
        assert idx == i and ts >= t_prev and abs(ts - time.time()) < 60
        t_prev = ts
        _check_record(_slot(r, ptr), ref)
        r.release(slot)
    assert r.next() is None and r.next() is None
    r.close()
    if len({tuple(ref["qt"].ravel()) for ref in refs}) == 1:
        assert "padded" in name   # the 5-frame stream changes its quant tables per frame


def test_mjpeg_reader_loops_and_jpg_is_one_frame(tmp_path):
    name = "40x56_420_5frames.mjpeg"
    refs = [jpeg_ref.parse(i) for i in _images(name)]
    r = _reader(os.path.join(JDIR, name), nbuf=3, loop=True)
    for k in range(12):
        ptr, ts, idx, slot = r.next()
        assert idx == k
        _check_record(_slot(r, ptr), refs[k % 5])
        r.release(slot)
    r.close()
    r = _reader(os.path.join(JDIR, "37x91_420_q75_opt.jpg"))
    ptr, ts, idx, slot = r.next()
    _check_record(_slot(r, ptr), jpeg_ref.parse(_data("37x91_420_q75_opt.jpg")))
    r.release(slot)
    assert r.next() is None
    r.close()
    # a truncated last image ends the stream, as a truncated y4m frame does
    d = _data(name)
    cut = tmp_path / "cut.mjpeg"
    cut.write_bytes(d[:len(d) - 40])
    r = _reader(cut)
    n = 0
    while (got := r.next()) is not None:
        r.release(got[3])
        n += 1
    assert n == 4
    r.close()


def test_size_or_sampling_change_in_mid_stream_is_a_named_error(tmp_path):
    from rvs_amd import _lib
    same, other_size, other_samp = _named("16x16_420_"), _named("17x33_420_"), _named("16x16_422_")
    for other in (other_size, other_samp):
        p = tmp_path / f"change_{other}.mjpeg"
        p.write_bytes(_data(same) + _data(same) + _data(other) + _data(same))
        r = _reader(p)
        for i in range(2):
            r.release(r.next()[3])
        with pytest.raises(_lib.RVError, match=r"frame 2.*size or sampling changed"):
            r.next()
        r.close()


def _sof_offset(d):
    segs, _ = jpeg_ref.segments(d)
    return [o for m, o, n in segs if m == 0xC0][0]


def _with(d, off, val):
    b = bytearray(d)
    b[off:off + len(val)] = val
    return bytes(b)


def _rejected():
    """(label, bytes, cause the error must name) for each stream kind the
    decoder refuses; all but the progressive file are header edits."""
    base = _data(_named("16x16_420_"))
    segs, scan = jpeg_ref.segments(base)
    sof = _sof_offset(base)
    dqt = [o for m, o, n in segs if m == 0xDB][0]
    out = [("progressive", _data("reject_progressive.jpg"), "progressive")]
    for marker, cause in ((0xC1, "extended"), (0xC3, "lossless"), (0xC9, "arithmetic")):
        out.append((cause, _with(base, sof - 3, bytes([marker])), cause))
    out.append(("12-bit", _with(base, sof, b"\x0c"), "12-bit"))
    out.append(("16-bit quant", _with(base, dqt, bytes([0x10 | base[dqt]])), "16-bit quant"))
    # four components: SOF0 rewritten with a fourth entry
    body = bytes([8]) + base[sof + 1:sof + 5] + bytes([4]) + base[sof + 6:sof + 15] + b"\x04\x11\x00"
    four = base[:sof - 2] + (len(body) + 2).to_bytes(2, "big") + body + base[sof + 15:]
    out.append(("4 components", four, "4 components"))
    out.append(("4:4:0", _with(base, sof + 7, b"\x12"), "sampling factors"))
    out.append(("4:1:1", _with(base, sof + 7, b"\x41"), "sampling factors"))
    # multi-scan baseline: the scan header announces one component of three
    sos = [o for m, o, n in segs if m == 0xDA][0]
    one = base[:sos - 2] + (8).to_bytes(2, "big") + b"\x01" + base[sos + 1:sos + 3] + \
        base[sos + 7:sos + 10] + base[scan:]
    out.append(("multi-scan", one, "multi-scan"))
    return out


@pytest.mark.parametrize("case", _rejected(), ids=lambda c: c[0])
def test_rejected_stream_kinds_name_their_cause(case):
    from rvs_amd import _lib
    lib = _lib.load()
    _, data, cause = case
    rec = np.zeros(1 << 16, np.uint8)
    st = lib.rv_jpeg_decode_coef(data, len(data), rec.ctypes.data, rec.size)
    assert st == RV_EINVAL
    assert cause.encode() in lib.rv_last_error(), lib.rv_last_error()
    if cause != "multi-scan" and cause != "16-bit quant":   # known from the frame header alone
        info = (ctypes.c_int * 4)()
        assert lib.rv_jpeg_probe(data, len(data), info) == RV_EINVAL
        assert cause.encode() in lib.rv_last_error()


def test_corrupt_entropy_data_is_einval():
    from rvs_amd import _lib
    lib = _lib.load()
    rec = np.zeros(1 << 16, np.uint8)

    def status(d):
        st = lib.rv_jpeg_decode_coef(d, len(d), rec.ctypes.data, rec.size)
        return st, lib.rv_last_error().decode()

    good = _data("37x91_420_q75_rst2.jpg")
    assert status(good)[0] == 0
    # a missing restart marker
    k = good.index(b"\xff\xd1")
    st, msg = status(good[:k] + good[k + 2:])
    assert st == RV_EINVAL and "RST" in msg, msg
    # restart markers out of order
    st, msg = status(good[:k] + b"\xff\xd3" + good[k + 2:])
    assert st == RV_EINVAL and "RST1" in msg, msg
    # a segment length that runs past the end of the file
    segs, scan = jpeg_ref.segments(good)
    o = segs[0][1]
    st, msg = status(_with(good, o - 2, b"\xff\xf0"))
    assert st == RV_EINVAL
    # a code that is in no table / a run past coefficient 63: all-ones entropy data
    base = _data("48x64_420_q75_nodht.jpg")
    segs, scan = jpeg_ref.segments(base)
    st, msg = status(base[:scan] + b"\xff\x00" * 64 + b"\xff\xd9")
    assert st == RV_EINVAL and ("not in the" in msg or "coefficient 63" in msg), msg
    # a DHT whose only AC code is a 15-zero run with a value: the run passes 63
    dht_ac = bytes([0x10, 1] + [0] * 15 + [0xF1])
    dht_dc = bytes([0x00, 1] + [0] * 15 + [0x00])
    seg = lambda m, b: bytes([0xFF, m]) + (len(b) + 2).to_bytes(2, "big") + b
    gray = _data(_named("8x8_gray_"))
    segs, scan = jpeg_ref.segments(gray)
    sos = [o for m, o, n in segs if m == 0xDA][0]
    hdr = b"".join(gray[o - 4:o + n] for m, o, n in segs if m not in (0xC4, 0xDA))
    run = b"\xff\xd8" + hdr + seg(0xC4, dht_dc) + seg(0xC4, dht_ac) + gray[sos - 4:scan] + \
        b"\x00" * 16 + b"\xff\xd9"
    st, msg = status(run)
    assert st == RV_EINVAL and "coefficient 63" in msg, msg
    # a record buffer that is too small
    st = lib.rv_jpeg_decode_coef(good, len(good), rec.ctypes.data, 64)
    assert st == RV_EINVAL and b"bytes" in lib.rv_last_error()


@pytest.mark.parametrize("prefix", ["37x91_420_q75_rst2", "50x70_444_q30", "17x33_gray_q75_opt"])
def test_truncation_is_an_error_never_a_crash(prefix, tmp_path):
    from rvs_amd import _lib
    lib = _lib.load()
    d = _data(_named(prefix))
    rec = np.zeros(1 << 17, np.uint8)
    info = (ctypes.c_int * 4)()
    for k in np.linspace(0, len(d) - 1, 20).astype(int):
        cut = d[:k]
        exact = ctypes.create_string_buffer(cut, max(len(cut), 1))  # no bytes past the cut
        assert lib.rv_jpeg_decode_coef(exact, len(cut), rec.ctypes.data, rec.size) == RV_EINVAL
        assert lib.rv_jpeg_probe(exact, len(cut), info) in (0, RV_EINVAL)
        # as the only image of a stream: an open error; behind a whole image: end of stream
        p = tmp_path / f"cut{k}.mjpeg"
        p.write_bytes(d + cut)
        r = _reader(p)
        r.release(r.next()[3])
        assert r.next() is None
        r.close()
        p.write_bytes(cut)
        with pytest.raises(_lib.RVError):
            _reader(p)


def test_other_containers_stay_unsupported(tmp_path):
    from rvs_amd.io_video import VideoSource
    with pytest.raises(ValueError, match="unsupported"):
        VideoSource(str(tmp_path / "clip.mp4"))
    with pytest.raises(ValueError, match="unsupported"):
        VideoSource(str(tmp_path / "clip.avi"))

"""Writes tests/golden/jpeg/: small JPEG / Motion-JPEG fixtures encoded with
Pillow (libjpeg-turbo) and expected.npz, the RGB pixels Pillow decodes from
them.  Every fixture is also decoded with tests/jpeg_ref.py and must agree
with Pillow byte for byte before anything is written.

    python tests/golden/make_jpeg_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref  # noqa: E402

OUT = os.path.join(HERE, "jpeg")
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 91), (48, 64), (50, 70), (9, 250)]
SAMPLINGS = ["444", "422", "420", "gray"]


def content(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([40 + 170 * x / max(W - 1, 1), 30 + 200 * y / max(H - 1, 1),
                    128 + 100 * np.sin(x / 7.0) * np.cos(y / 5.0)], axis=-1)
    return np.clip(img + rng.normal(0, 2, img.shape), 0, 255).astype(np.uint8)


def encode(rgb, sampling, quality, **kw):
    buf = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(rgb[..., 1]).save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(rgb).save(buf, "JPEG", quality=quality,
                                  subsampling={"444": 0, "422": 1, "420": 2}[sampling], **kw)
    return buf.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def strip_dht(data):
    segs, start = jpeg_ref.segments(data)
    out = bytearray(data[:2])
    for m, o, n in segs:
        if m != 0xC4:
            out += data[o - 4:o + n]
    return bytes(out) + data[start:]


def main():
    os.makedirs(OUT, exist_ok=True)
    files, expected = {}, {}
    for hi, (H, W) in enumerate(SHAPES):
        for si, s in enumerate(SAMPLINGS):  # each sampling meets both qualities and contents
            q = (30, 100)[(si + hi) % 2]
            kind = ("noise", "smooth")[(si // 2 + hi // 2) % 2]
            files[f"{H}x{W}_{s}_q{q}_{kind}.jpg"] = encode(content(kind, H, W, 4 * hi + si), s, q)
    # the chroma plane is at most two samples wide: libjpeg replicates there
    files["6x4_420_q90_noise.jpg"] = encode(content("noise", 6, 4, 90), "420", 90)
    files["5x3_422_q90_noise.jpg"] = encode(content("noise", 5, 3, 91), "422", 90)
    # more than one 128 x 64 kernel tile: down, and both ways (the chroma halo crosses tiles)
    files["130x24_420_q50_smooth.jpg"] = encode(content("smooth", 130, 24, 92), "420", 50)
    files["72x136_420_q75_noise.jpg"] = encode(content("noise", 72, 136, 93), "420", 75)
    files["72x136_444_q50_smooth.jpg"] = encode(content("smooth", 72, 136, 94), "444", 50)
    files["37x91_420_q75_rst2.jpg"] = encode(content("smooth", 37, 91, 100), "420", 75,
                                             restart_marker_blocks=2)
    files["50x70_444_q75_rst2.jpg"] = encode(content("noise", 50, 70, 101), "444", 75,
                                             restart_marker_blocks=2)
    files["37x91_420_q75_opt.jpg"] = encode(content("noise", 37, 91, 102), "420", 75, optimize=True)
    files["17x33_gray_q75_opt.jpg"] = encode(content("smooth", 17, 33, 103), "gray", 75,
                                             optimize=True)
    plain = encode(content("smooth", 48, 64, 104), "420", 75)
    files["48x64_420_q75_nodht.jpg"] = strip_dht(plain)
    assert b"\xff\xc4" not in files["48x64_420_q75_nodht.jpg"][:600]
    expected["48x64_420_q75_nodht.jpg"] = pillow_rgb(plain)
    # the Annex K tables restated in jpeg_ref are the ones Pillow writes
    j = jpeg_ref.segments(plain)[0]
    dht = b"".join(plain[o:o + n] for m, o, n in j if m == 0xC4)
    for tc_th, (counts, syms) in ((0x00, jpeg_ref.STD_DC_LUMA), (0x10, jpeg_ref.STD_AC_LUMA),
                                  (0x01, jpeg_ref.STD_DC_CHROMA), (0x11, jpeg_ref.STD_AC_CHROMA)):
        assert bytes([tc_th] + counts + syms) in dht, hex(tc_th)

    frames = [encode(content("smooth", 40, 56, 200 + f), "420", q)
              for f, q in enumerate((30, 50, 75, 90, 100))]
    files["40x56_420_5frames.mjpeg"] = b"".join(frames)
    pad = [encode(content("noise", 24, 40, 300 + f), "422", 80) for f in range(3)]
    files["24x40_422_padded.mjpeg"] = (b"\x00" * 5 + pad[0] + b"\x00" * 7 + pad[1] +
                                       b"\xff\xff\x00pad\xff" + pad[2] + b"\x00\x00")
    # a stream the decoder must reject (tests/test_jpeg_cpu.py)
    files["reject_progressive.jpg"] = encode(content("smooth", 16, 16, 400), "420", 75,
                                             progressive=True)

    for name, data in files.items():
        if name.startswith("reject_"):
            continue
        parts = jpeg_ref.split_frames(data) if name.endswith(".mjpeg") else [data]
        if name not in expected:
            want = [pillow_rgb(p) for p in parts]
            expected[name] = np.stack(want) if name.endswith(".mjpeg") else want[0]
        got = [jpeg_ref.decode_rgb(p) for p in parts]
        got = np.stack(got) if name.endswith(".mjpeg") else got[0]
        assert got.shape == expected[name].shape, name
        assert np.array_equal(got, expected[name]), \
            f"{name}: numpy restatement differs from Pillow at {np.argwhere(got != expected[name])[:4]}"
    total = 0
    for name, data in files.items():
        assert len(data) < 100 * 1024
        total += len(data)
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)
    print(f"{len(files)} fixtures, {total} bytes, "
          f"npz {os.path.getsize(os.path.join(OUT, 'expected.npz'))} bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/jpeg_enc/: fixtures for the JPEG encoder.  input.npz
holds the RGB pixels, each NAME.jpg is what Pillow (libjpeg-turbo) writes for
them with quality=q, subsampling=s, restart_marker_rows=1, decoded.npz is
what Pillow decodes from that file (RGB), and dqt.npz holds the DQT segments
Pillow writes at eight qualities.  The set as a whole must contain the
entropy coder's special cases; that is asserted with tests/jpeg_ref.py before
anything is written.

    python tests/golden/make_jpeg_enc_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref  # noqa: E402

OUT = os.path.join(HERE, "jpeg_enc")
# 17x33: odd both ways, a dummy luma block under 4:2:0 / 4:2:2.  24x24: the
# chroma planes of 4:2:0 end inside an MCU row.  9x250: many MCUs in a segment.
# 130x24: more than eight segments.  9x1100: more than 256 blocks in a segment
# for every sampling (the entropy kernel codes 256 blocks at a time).
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 33), (24, 24), (37, 91), (9, 250), (130, 24), (72, 136),
          (9, 1100)]
SAMPLINGS = ["444", "422", "420"]
QUALITIES = [30, 75, 100]
KINDS = ["noise", "smooth", "flat"]


def content(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (H, W, 3)).copy()
    if kind == "blocks":  # black and white 8x8 squares: the largest DC differences
        y, x = np.mgrid[0:H, 0:W]
        return np.repeat((((x // 8 + y // 8) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([40 + 170 * x / max(W - 1, 1), 30 + 200 * y / max(H - 1, 1),
                    128 + 100 * np.sin(x / 7.0) * np.cos(y / 5.0)], axis=-1)
    return np.clip(img + rng.normal(0, 2, img.shape), 0, 255).astype(np.uint8)


def encode(rgb, sampling, quality):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, restart_marker_rows=1,
                              subsampling={"444": 0, "422": 1, "420": 2}[sampling])
    return buf.getvalue()


def features(data):
    """Which of the entropy coder's special cases one fixture contains."""
    j = jpeg_ref.parse(data)
    _, scan = jpeg_ref.segments(data)
    body = data[scan:]
    out = set()
    if b"\xff\x00" in body:
        out.add("stuffed FF 00")
    if body.count(b"\xff\xd0") >= 2:
        out.add("wrapped RSTm")
    h, v = j["hv"][0]
    mx = j["coef"][0].shape[1] // h
    for c, (ch, cv) in enumerate(j["hv"]):
        plane = j["coef"][c]
        zz = plane[:, :, jpeg_ref.ZIGZAG].astype(np.int64)
        if (zz[:, :, 63] != 0).any():
            out.add("coefficient 63")
        if (zz[:, :, 1:] == 0).all(axis=2).any():
            out.add("EOB only")
        nz = zz[:, :, 1:] != 0
        for by, bx in zip(*np.nonzero(nz.any(axis=2))):
            k = np.nonzero(nz[by, bx])[0]
            if np.diff(np.concatenate([[-1], k])).max() > 16:
                out.add("ZRL")
                break
        # DC differences in MCU order, the predictor reset at each MCU row
        for row in range(plane.shape[0] // cv):
            dc = plane[row * cv:(row + 1) * cv, :, 0].astype(np.int64)
            order = dc.reshape(cv, mx, ch).transpose(1, 0, 2).reshape(-1)
            if np.abs(np.diff(np.concatenate([[0], order]))).max() >= 1024:
                out.add("DC category 11")
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    files, inputs = {}, {}
    for hi, (H, W) in enumerate(SHAPES):
        for si, s in enumerate(SAMPLINGS):  # each sampling meets every quality and content
            q = QUALITIES[(si + hi) % 3]
            kind = KINDS[(2 * si + hi + hi // 3) % 3]
            name = f"{H}x{W}_{s}_q{q}_{kind}"
            inputs[name] = content(kind, H, W, 3 * hi + si)
    for si, s in enumerate(SAMPLINGS):
        inputs[f"16x48_{s}_q100_blocks"] = content("blocks", 16, 48, 0)
    for name, rgb in inputs.items():
        _, s, q, _ = name.split("_")
        files[name] = encode(rgb, s, int(q[1:]))

    for s in SAMPLINGS:
        mine = [n for n in files if f"_{s}_" in n]
        assert {n.split("_")[2] for n in mine} >= {"q30", "q75", "q100"}, s
        assert {n.split("_")[3] for n in mine} >= set(KINDS), s
    seen = set()
    decoded = {}
    for name, data in files.items():
        assert len(data) < 100 * 1024, name
        segs, _ = jpeg_ref.segments(data)
        assert [m for m, _, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD,
                                           0xDA], name
        seen |= features(data)
        decoded[name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    need = {"stuffed FF 00", "ZRL", "DC category 11", "coefficient 63", "EOB only", "wrapped RSTm"}
    assert seen >= need, need - seen

    for name, data in files.items():
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
    # five frames of one size, sampling and quality whose lengths differ: a
    # batch in one call, and what a sink writes (the images back to back)
    clip = np.stack([content(("smooth", "noise", "flat", "smooth", "blocks")[f], 40, 56, 500 + f)
                     for f in range(5)])
    images = [encode(fr, "420", 90) for fr in clip]
    assert len({len(i) for i in images}) == 5
    inputs["clip_40x56_420_q90"] = clip
    with open(os.path.join(OUT, "clip_40x56_420_q90.mjpeg"), "wb") as f:
        f.write(b"".join(images))
    np.savez_compressed(os.path.join(OUT, "input.npz"), **inputs)
    np.savez_compressed(os.path.join(OUT, "decoded.npz"), **decoded)
    # the DQT payloads (table index, then 64 entries in zigzag order) Pillow writes per quality
    dqt = {}
    for q in (1, 25, 49, 50, 51, 75, 95, 100):
        data = encode(content("smooth", 8, 8, 0), "420", q)
        segs, _ = jpeg_ref.segments(data)
        dqt[f"q{q}"] = np.stack([np.frombuffer(data[o:o + n], np.uint8)
                                 for m, o, n in segs if m == 0xDB])
        assert dqt[f"q{q}"].shape == (2, 65)
    np.savez_compressed(os.path.join(OUT, "dqt.npz"), **dqt)
    print(f"{len(files)} fixtures, {sum(map(len, files.values()))} bytes; "
          f"input.npz {os.path.getsize(os.path.join(OUT, 'input.npz'))}, "
          f"decoded.npz {os.path.getsize(os.path.join(OUT, 'decoded.npz'))} bytes")


if __name__ == "__main__":
    main()

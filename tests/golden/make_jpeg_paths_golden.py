"""Writes tests/golden/jpeg_paths/pillow_sha256.json: per decoder case of
tests/jpeg_cases.py (all but beyond16) the SHA-256 of the RGB pixels Pillow
(libjpeg-turbo) decodes from the file the host coder (rv_jpeg_encode_coef)
writes for the case's coefficient record.  basis gives Cb and Cr different
quant tables, which the host coder refuses; its files get their header from
this script (three DQT segments) and their scan from jpeg_ref.entropy_encode.
Nothing is written unless tests/jpeg_ref.py decodes every file as Pillow does.

It also checks the domain of jpeg_ref.libjpeg16_safe against Pillow on random
single grey blocks with products up to 32000: every block it calls safe must
decode as the restatement does.  Needs the built library and Pillow.

    python tests/golden/make_jpeg_paths_golden.py
"""
import ctypes
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(REPO, "road-vision-system_amd")]
import jpeg_cases  # noqa: E402
import jpeg_ref  # noqa: E402

OUT = os.path.join(HERE, "jpeg_paths")


def host_file(j):
    from rvs_amd import _lib
    rec = jpeg_ref.record(j)
    out = np.zeros(700 + 2 * rec.size, np.uint8)
    n = ctypes.c_size_t(0)
    st = _lib.load().rv_jpeg_encode_coef(rec.ctypes.data, rec.size, 0, out.ctypes.data, out.size,
                                         ctypes.addressof(n))
    assert st == 0, _lib.load().rv_last_error()
    return out[:n.value].tobytes()


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def script_file(j):
    """A baseline file with one quant table per component."""
    nc = j["ncomp"]
    out = b"\xff\xd8"
    for c in range(nc):
        out += _seg(0xDB, bytes([c]) + bytes(int(v) for v in j["qt"][c][jpeg_ref.ZIGZAG]))
    sof = bytes([8]) + j["H"].to_bytes(2, "big") + j["W"].to_bytes(2, "big") + bytes([nc])
    for c, (h, v) in enumerate(j["hv"]):
        sof += bytes([c + 1, (h << 4) | v, c])
    out += _seg(0xC0, sof)
    for tc_th, (counts, syms) in ((0x00, jpeg_ref.STD_DC_LUMA), (0x10, jpeg_ref.STD_AC_LUMA),
                                  (0x01, jpeg_ref.STD_DC_CHROMA), (0x11, jpeg_ref.STD_AC_CHROMA)):
        out += _seg(0xC4, bytes([tc_th] + counts + syms))
    sos = bytes([nc]) + b"".join(bytes([c + 1, 0x00 if c == 0 else 0x11]) for c in range(nc))
    out += _seg(0xDA, sos + bytes([0, 63, 0]))
    return out + jpeg_ref.entropy_encode(j, 0)[0]


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def check_domain(n=1438, seed=7):
    rng = np.random.default_rng(seed)
    safe_n = unsafe_differ = unsafe_n = 0
    for _ in range(n):
        q = rng.integers(1, 256, 64)
        blk = np.zeros(64, np.int16)
        lim = int(rng.choice([1000, 4000, 8000, 32000]))
        for pos in rng.choice(64, int(rng.integers(1, 9)), replace=False):
            blk[pos] = int(rng.integers(-lim, lim + 1)) // int(q[pos])
        blk[1:] = np.clip(blk[1:], -1023, 1023)
        blk[0] = np.clip(blk[0], -1024, 1023)
        j = jpeg_cases.blank(8, 8, jpeg_ref.SGRAY, [q] * 3)
        j["coef"][0][0, 0] = blk
        same = np.array_equal(pillow_rgb(host_file(j)), jpeg_ref.to_rgb(j))
        if jpeg_ref.libjpeg16_safe(blk, q):
            assert same, f"a block inside the 16-bit-safe domain decodes differently: {blk} {q}"
            safe_n += 1
        else:
            unsafe_n += 1
            unsafe_differ += not same
    print(f"domain: {safe_n} safe blocks all identical; {unsafe_differ} of {unsafe_n} unsafe differ")
    assert safe_n > 100 and unsafe_differ > 100


def main():
    check_domain()
    digests = {}
    for k, j in jpeg_cases.decoder_cases(include_beyond=False).items():
        shared = j["ncomp"] == 1 or np.array_equal(j["qt"][1], j["qt"][2])
        data = host_file(j) if shared else script_file(j)
        back = jpeg_ref.parse(data)
        assert all(np.array_equal(a, b) for a, b in zip(back["coef"], j["coef"])), k
        assert np.array_equal(back["qt"], j["qt"]), k
        want, got = pillow_rgb(data), jpeg_ref.to_rgb(j)
        assert want.shape == got.shape, k
        assert np.array_equal(want, got), \
            f"{k}: numpy restatement differs from Pillow at {np.argwhere(got != want)[:4]}"
        digests[k] = hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest()
    # the block of the table in DESIGN.md: the restatement clamps, Pillow's libjpeg does not
    j = jpeg_cases.beyond16(jpeg_ref.SGRAY)
    one = jpeg_cases.blank(8, 8, jpeg_ref.SGRAY, j["qt"])
    one["coef"][0][0, 0] = j["coef"][0][0, 0]
    print("DC 33 x quant 255: restatement", jpeg_ref.to_rgb(one)[0, 0, 0], "Pillow",
          pillow_rgb(host_file(one))[0, 0, 0])
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "pillow_sha256.json"), "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests")


if __name__ == "__main__":
    main()

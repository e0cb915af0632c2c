"""Baseline JPEG in numpy: the independent checker of the native decoder.

Marker parse, Huffman decode and the integer arithmetic of libjpeg's default
decode path (islow IDCT, fancy chroma upsampling, 16-bit fixed-point
YCbCr -> RGB), restated from the JPEG standard (ITU-T T.81) and libjpeg's
published arithmetic.  Slow and plain on purpose; only for small fixtures.

The way back, for the hand-built cases of tests/jpeg_cases.py: record() (the
coefficient record of include/rvhip.h), entropy_encode() (the inverse of
parse()'s scan loop), and the two predicates that bound the decoder's claim:
libjpeg16_safe() (where libjpeg's own builds agree) and int32_safe().
"""
import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
    13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
    52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

S444, S422, S420, SGRAY = 0, 1, 2, 3
_YSAMP = {(1, 1): S444, (2, 1): S422, (2, 2): S420}

# T.81 Annex K.3 typical Huffman tables: (counts per code length 1..16, symbols)
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])


def _huff_table(counts, symbols):
    """{(length, code): symbol} of a canonical Huffman table."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


def segments(data):
    """[(marker, payload offset, payload length)] of the header segments up to
    and including SOS; the offset after the SOS header is where entropy data
    starts."""
    assert data[0] == 0xFF and data[1] == 0xD8
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        while data[p + 1] == 0xFF:
            p += 1
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        out.append((m, p + 4, n - 2))
        p += 2 + n
        if m == 0xDA:
            return out, p


def split_frames(data):
    """The JPEG images (SOI .. EOI) of a Motion-JPEG byte string, in order."""
    frames, p, n = [], 0, len(data)
    while True:
        while p + 1 < n and not (data[p] == 0xFF and data[p + 1] == 0xD8):
            p += 1
        if p + 1 >= n:
            return frames
        _, q = segments(data[p:])
        q += p
        while not (data[q] == 0xFF and data[q + 1] == 0xD9):
            q += 1
        frames.append(bytes(data[p:q + 2]))
        p = q + 2


class _Bits:
    def __init__(self, data, p):
        self.d, self.p, self.acc, self.n = data, p, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.d[self.p]
            self.p += 1
            if b == 0xFF:
                assert self.d[self.p] == 0, "marker inside entropy data"
                self.p += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise ValueError("Huffman code not in table")

    def restart(self, k):
        self.n = 0
        assert self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xD0 + (k & 7), "missing RSTn"
        self.p += 2


def _extend(v, s):
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def parse(data):
    """One baseline JPEG image -> dict: W, H, ncomp, sampling, qt (ncomp, 64)
    u16 in natural order, coef: per component an (blocks_h, blocks_w, 64)
    int16 array of quantised coefficients in natural order (MCU-padded)."""
    data = bytes(data)
    segs, p = segments(data)
    qts, huff = {}, {(0, 0): _huff_table(*STD_DC_LUMA), (0, 1): _huff_table(*STD_DC_CHROMA),
                     (1, 0): _huff_table(*STD_AC_LUMA), (1, 1): _huff_table(*STD_AC_CHROMA)}
    ri, comps, scan = 0, None, None
    for m, o, n in segs:
        b = data[o:o + n]
        if m == 0xDB:
            while b:
                assert b[0] >> 4 == 0
                q = np.zeros(64, np.uint16)
                q[ZIGZAG] = np.frombuffer(b[1:65], np.uint8)
                qts[b[0] & 15] = q
                b = b[65:]
        elif m == 0xC4:
            while b:
                counts = list(b[1:17])
                ns = sum(counts)
                huff[(b[0] >> 4, b[0] & 15)] = _huff_table(counts, list(b[17:17 + ns]))
                b = b[17 + ns:]
        elif m == 0xC0:
            assert b[0] == 8
            H, W = (b[1] << 8) | b[2], (b[3] << 8) | b[4]
            comps = [(b[6 + 3 * i], b[7 + 3 * i] >> 4, b[7 + 3 * i] & 15, b[8 + 3 * i])
                     for i in range(b[5])]
        elif m == 0xDD:
            ri = (b[0] << 8) | b[1]
        elif m == 0xDA:
            assert b[0] == len(comps)
            scan = [(b[2 + 2 * i] >> 4, b[2 + 2 * i] & 15) for i in range(b[0])]
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, hex(m)
    nc = len(comps)
    if nc == 1:
        sampling, hv = SGRAY, [(1, 1)]
    else:
        sampling = _YSAMP[(comps[0][1], comps[0][2])]
        assert comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1)
        hv = [c[1:3] for c in comps]
    hmax, vmax = hv[0]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    coef = [np.zeros((my * v, mx * h, 64), np.int16) for h, v in hv]
    br, pred, done = _Bits(data, p), [0] * nc, 0
    for mcu in range(mx * my):
        if ri and mcu and mcu % ri == 0:
            br.restart(done)
            done += 1
            pred = [0] * nc
        for c, (h, v) in enumerate(hv):
            for j in range(h * v):
                blk = coef[c][(mcu // mx) * v + j // h, (mcu % mx) * h + j % h]
                s = br.symbol(huff[(0, scan[c][0])])
                pred[c] += _extend(br.bits(s), s)
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs = br.symbol(huff[(1, scan[c][1])])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                    k += 1
    qt = np.stack([qts[c[3]] for c in comps])
    return dict(W=W, H=H, ncomp=nc, sampling=sampling, qt=qt, coef=coef, hv=hv)


def _idct_1d(i, s, seen=None):
    """libjpeg jidctint (islow) butterfly over the leading axis of eight.
    `seen`, a list, collects every intermediate value (for int32_safe)."""
    def k(x):
        if seen is not None:
            seen.append(x)
        return x
    i = [x.astype(np.int64) for x in i]
    z1 = k(k(i[2] + i[6]) * 4433)
    t2 = k(z1 - k(i[6] * 15137))
    t3 = k(z1 + k(i[2] * 6270))
    t0 = k(k(i[0] + i[4]) << 13)
    t1 = k(k(i[0] - i[4]) << 13)
    t10, t13, t11, t12 = k(t0 + t3), k(t0 - t3), k(t1 + t2), k(t1 - t2)
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = k(a0 + a3), k(a1 + a2), k(a0 + a2), k(a1 + a3)
    z5 = k(k(z3 + z4) * 9633)
    a0, a1, a2, a3 = k(a0 * 2446), k(a1 * 16819), k(a2 * 25172), k(a3 * 12299)
    z1, z2 = k(z1 * -7373), k(z2 * -20995)
    z3, z4 = k(k(z3 * -16069) + z5), k(k(z4 * -3196) + z5)
    a0, a1, a2, a3 = (k(a0 + k(z1 + z3)), k(a1 + k(z2 + z4)), k(a2 + k(z2 + z3)),
                      k(a3 + k(z1 + z4)))
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return [k(k(o) + (1 << (s - 1))) >> s for o in out]


def idct_samples(coef, q, seen=None):
    """(..., 64) quantised coefficients -> (..., 8, 8) samples [v, u] before
    the clamp to 0..255."""
    coef = np.asarray(coef)
    d = (coef.astype(np.int64) * np.asarray(q).astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    if seen is not None:
        seen.append(d)
    cols = _idct_1d([d[..., v, :] for v in range(8)], 11, seen)  # down each column
    ws = np.stack(cols, axis=-2)                                 # (..., v, u)
    rows = _idct_1d([ws[..., :, u] for u in range(8)], 18, seen)  # along each row
    return np.stack(rows, axis=-1) + 128


def idct_plane(coef, q):
    """(bh, bw, 64) quantised coefficients -> (8 bh, 8 bw) u8 samples."""
    bh, bw, _ = coef.shape
    px = np.clip(idct_samples(coef, q), 0, 255)
    return px.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw).astype(np.int64)


def _fits(x, bits):
    lim = 1 << (bits - 1)
    x = np.asarray(x)
    return ((x >= -lim) & (x < lim)).reshape(x.shape[0], -1).all(axis=1)


def libjpeg16_safe(coef, q):
    """Per block of (..., 64) coefficients: does it stay where every libjpeg
    build decodes the same samples as a plain clamp?  libjpeg-turbo's SIMD
    islow IDCT keeps 16-bit lanes for the dequantised coefficients, for the
    sums it forms before widening (in0 +- in4, in7 + in3, in5 + in1, in both
    passes) and for the workspace between the passes; the C build wraps out of
    range samples through a mask table.  Inside these bounds they all agree."""
    coef = np.asarray(coef)
    c = coef.reshape(-1, 64).astype(np.int64)
    d = (c * np.asarray(q).astype(np.int64).reshape(1, 64)).reshape(-1, 8, 8)
    ok = _fits(d, 16)
    ws = np.stack(_idct_1d([d[:, v, :] for v in range(8)], 11), axis=1)
    ok &= _fits(ws, 16)
    for i in ([d[:, v, :] for v in range(8)], [ws[:, :, u] for u in range(8)]):
        for x in (i[0] + i[4], i[0] - i[4], i[7] + i[3], i[5] + i[1]):
            ok &= _fits(x, 16)
    return ok.reshape(coef.shape[:-1])


def int32_safe(coef, q):
    """Per block: does every intermediate of the restatement (products, sums,
    the rounding add) fit int32?  The kernel computes in int."""
    coef = np.asarray(coef)
    seen = []
    idct_samples(coef.reshape(-1, 64), q, seen)
    ok = np.ones(coef.reshape(-1, 64).shape[0], bool)
    for x in seen:
        ok &= _fits(x, 32)
    return ok.reshape(coef.shape[:-1])


def _up_h2v1(p):
    prev = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    nxt = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + prev + 1) >> 2
    out[:, 1::2] = (3 * p + nxt + 2) >> 2
    return out


def _up_h2v2(p):
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    dn = np.concatenate([p[1:], p[-1:]], axis=0)
    s = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    s[0::2] = 3 * p + up
    s[1::2] = 3 * p + dn
    prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    nxt = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (3 * s + prev + 8) >> 4
    out[:, 1::2] = (3 * s + nxt + 7) >> 4
    return out


def full_planes(j):
    """parse() output -> the components as (H, W) int64 planes at full
    resolution: IDCT, clamp, crop, chroma upsampling."""
    W, H = j["W"], j["H"]
    hmax, vmax = j["hv"][0]
    planes = []
    for c, (h, v) in enumerate(j["hv"]):
        dh, dw = -(-H * v // vmax), -(-W * h // hmax)
        p = idct_plane(j["coef"][c], j["qt"][c])[:dh, :dw]      # crop before upsampling
        fh, fv = hmax // h, vmax // v
        if fh == 2 and dw <= 2:     # libjpeg replicates instead when the plane is <= 2 wide
            p = np.repeat(np.repeat(p, fv, axis=0), 2, axis=1)
        elif (fh, fv) == (2, 1):
            p = _up_h2v1(p)
        elif (fh, fv) == (2, 2):
            p = _up_h2v2(p)
        planes.append(p[:H, :W])
    return planes


def ycc_to_rgb_unclamped(y, cb, cr):
    """(..., 3) int64 R, G, B of libjpeg's 16-bit fixed-point conversion,
    before the clamp to 0..255."""
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.stack([r, g, b], axis=-1)


def to_rgb(j):
    """parse() output -> (H, W, 3) RGB u8."""
    planes = full_planes(j)
    if len(planes) == 1:
        return np.repeat(planes[0][:, :, None], 3, axis=2).astype(np.uint8)
    return np.clip(ycc_to_rgb_unclamped(*planes), 0, 255).astype(np.uint8)


def decode_rgb(data):
    return to_rgb(parse(data))


# ---- the way back: coefficient records and the entropy coder --------------

RECORD_MAGIC = 0x46434A52  # "RJCF", include/rvhip.h


def record(j):
    """parse() output -> the coefficient record of include/rvhip.h as a u8
    array: int32[8] {magic, W, H, sampling, ncomp, 0, 0, 0}, u16 quant tables
    in natural order, then per component its int16 block grid."""
    nc = len(j["coef"])
    parts = [np.array([RECORD_MAGIC, j["W"], j["H"], j["sampling"], nc, 0, 0, 0], "<i4").view(np.uint8),
             np.ascontiguousarray(j["qt"], "<u2").reshape(-1).view(np.uint8)]
    assert parts[1].size == nc * 128
    parts += [np.ascontiguousarray(c, "<i2").reshape(-1).view(np.uint8) for c in j["coef"]]
    return np.concatenate(parts)


def _huff_enc(counts, symbols):
    """{symbol: (code, length)} of a canonical Huffman table."""
    return {sym: (code, length) for (length, code), sym in _huff_table(counts, symbols).items()}


_ENC_DC = (_huff_enc(*STD_DC_LUMA), _huff_enc(*STD_DC_CHROMA))
_ENC_AC = (_huff_enc(*STD_AC_LUMA), _huff_enc(*STD_AC_CHROMA))


def _value_bits(v):
    """(size category, the category's value bits) of a coefficient (T.81 F.1.2)."""
    s = abs(v).bit_length()
    return s, (v if v >= 0 else v - 1) & ((1 << s) - 1)


def block_code(blk, pred, t):
    """(bits as an int, bit count) of one block in natural order, coded with
    the Annex K tables of class t (0 luma, 1 chroma) after DC prediction pred."""
    s, vb = _value_bits(int(blk[0]) - pred)
    assert s <= 11, "DC difference without a baseline code"
    code, n = _ENC_DC[t][s]
    acc, bits = (code << s) | vb, n + s
    run = 0
    for v in blk[ZIGZAG[1:]].tolist():
        if v == 0:
            run += 1
            continue
        while run >= 16:
            code, n = _ENC_AC[t][0xF0]
            acc, bits = (acc << n) | code, bits + n
            run -= 16
        s, vb = _value_bits(v)
        assert s <= 10, "AC coefficient without a baseline code"
        code, n = _ENC_AC[t][(run << 4) | s]
        acc, bits = (acc << (n + s)) | (code << s) | vb, bits + n + s
        run = 0
    if run:
        code, n = _ENC_AC[t][0]
        acc, bits = (acc << n) | code, bits + n
    return acc, bits


def scan_order(j, rows_per_restart=1):
    """The blocks of the interleaved scan as [(component, by, bx)], one list
    per restart segment of rows_per_restart MCU rows (0: a single segment)."""
    hv = j["hv"]
    my, mx = j["coef"][0].shape[0] // hv[0][1], j["coef"][0].shape[1] // hv[0][0]
    rows = []
    for yy in range(my):
        row = []
        for xx in range(mx):
            for c, (h, v) in enumerate(hv):
                row += [(c, yy * v + k // h, xx * h + k % h) for k in range(h * v)]
        rows.append(row)
    n = rows_per_restart or my
    return [sum(rows[k:k + n], []) for k in range(0, my, n)]


def encode_segment(j, blocks):
    """One restart segment (a scan_order() list) -> (its bytes before stuffing,
    padded with 1-bits to a whole byte; the bit count of every block)."""
    acc, total, counts, pred = 0, 0, [], [0] * len(j["coef"])
    for c, by, bx in blocks:
        blk = j["coef"][c][by, bx]
        a, n = block_code(blk, pred[c], 0 if c == 0 else 1)
        pred[c] = int(blk[0])
        acc, total = (acc << n) | a, total + n
        counts.append(n)
    pad = -total % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((total + pad) // 8, "big"), counts


def entropy_encode(j, rows_per_restart=1):
    """The inverse of parse()'s scan loop: parse() output -> (the bytes that
    follow the SOS header up to and including EOI, per restart segment a dict
    {block_bits, raw_bytes, stuffed_bytes, raw}).  Annex K tables, MCU order
    with the dummy blocks as stored, DC prediction reset per segment, 1-bit
    padding, 0x00 after every 0xFF, RSTm between segments."""
    out, info = bytearray(), []
    segs = scan_order(j, rows_per_restart)
    for k, blocks in enumerate(segs):
        raw, counts = encode_segment(j, blocks)
        stuffed = raw.replace(b"\xff", b"\xff\x00")
        out += stuffed
        out += bytes([0xFF, 0xD0 + (k & 7) if k + 1 < len(segs) else 0xD9])
        info.append(dict(block_bits=counts, raw_bytes=len(raw), stuffed_bytes=len(stuffed), raw=raw))
    return bytes(out), info

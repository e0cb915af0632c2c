"""Named inputs that pin every path of the JPEG kernels: hand-built
coefficient records for csrc/jpeg.hip (decoder cases) and for the entropy and
compact kernels of csrc/jpeg_enc.hip (stream cases).

Every case is a dict in the form jpeg_ref.parse() returns, built from a seed;
nothing is read from disk.  Every block carries a DC of its own, a function of
(component, bx, by), so a read from the wrong block shows -- except where a
case dictates the DC (saturate's flat blocks, sizes, maxbits), which says so.
tests/test_jpeg_cases_cpu.py proves from the reference side alone which path
each case runs; tests/test_jpeg_paths_gpu.py runs them on the kernels.

What could not be reached is listed in UNREACHED, never dropped silently.
"""
import functools

import numpy as np

import jpeg_ref
from jpeg_ref import S420, S422, S444, SGRAY, ZIGZAG

NAMES = {S444: "444", S422: "422", S420: "420", SGRAY: "gray"}
HV = {S444: [(1, 1)] * 3, S422: [(2, 1), (1, 1), (1, 1)], S420: [(2, 2), (1, 1), (1, 1)],
      SGRAY: [(1, 1)]}
ALL = (S444, S422, S420, SGRAY)
COLOUR = (S444, S422, S420)
SUBSAMPLED = (S422, S420)
TILE_W, TILE_H = 128, 64            # the decode kernel's tile, pixels
CHUNK = 256                         # blocks the entropy kernel codes at a time
PASS_BYTES = 1024                   # raw bytes per pass of the compact kernel


def max_block_bits(t):
    """The longest block the Annex K tables of class t (0 luma, 1 chroma) can
    code, by dynamic programming over the position of the next non-zero
    coefficient: the longest DC code plus the longest run / size sequence."""
    ac, dc = jpeg_ref._ENC_AC[t], jpeg_ref._ENC_DC[t]
    best = [0] * 65
    for k in range(63, 0, -1):
        b = ac[0][1]                                        # EOB here
        for p in range(k, 64):
            r = p - k
            sym = max(ac[((r % 16) << 4) | s][1] + s for s in range(1, 11))
            b = max(b, (r // 16) * ac[0xF0][1] + sym + best[p + 1])
        best[k] = b
    return max(dc[s][1] + s for s in range(12)) + best[1]


# 1658 and 1408: a block of +-1023 everywhere behind a DC difference of +-2047
BLOCK_BITS_MAX = (max_block_bits(0), max_block_bits(1))

UNREACHED = {
    "maxbits: chroma blocks of 1660 bits":
        "1660 bits (an 11-bit DC code, 11 value bits, 63 x (16 + 10)) bounds any block, but the "
        "Annex K chroma table codes run 0 / size 10 in 12 bits and its 16-bit codes all have a "
        "run, so the longest chroma block is 1408 bits (max_block_bits); luma reaches its 1658",
    "basis at 64 x 128 for 4:2:2 / 4:2:0":
        "a 64 x 128 image has 64 / 32 chroma blocks; the image grows to 64 x 256 / 128 x 256 "
        "so that every component still holds all 128 basis blocks",
    "tiles 4:2:2 reads above / below":
        "4:2:2 has no vertical chroma filter, so no pixel reads a chroma row of another tile; "
        "its tile borders downwards are still crossed by every tiles case with H > 64",
    "chunks of exactly 255 / 256 / 257 / 512 blocks":
        "a segment is a whole number of MCUs of 3 (4:4:4), 4 (4:2:2) or 6 (4:2:0) blocks; the "
        "nearest counts are used: 255 258 513 516 / 252 256 260 512 516 / 252 258 510 516",
    "rows: RST index wrap at 9 rows":
        "nine MCU rows write RST0..RST7 once; the index first wraps with a tenth row, which is "
        "added to the issue's 1, 8, 9 and 257",
    "pillow digest of beyond16":
        "libjpeg builds disagree there by construction; the expected value is the clamp",
}


def blank(W, H, samp, qt):
    """An all-zero parse()-style dict; qt: (3, 64) tables in natural order."""
    hv = HV[samp]
    hmax, vmax = hv[0]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    coef = [np.zeros((my * v, mx * h, 64), np.int16) for h, v in hv]
    return dict(W=W, H=H, ncomp=len(hv), sampling=samp,
                qt=np.array(qt, np.uint16)[:len(hv)].copy(), coef=coef, hv=list(hv))


def own(c, shape, seed=0):
    """The signature of every block of a (bh, bw) grid: -8..8, and it differs
    between horizontal, vertical and diagonal neighbours and between components."""
    by, bx = np.mgrid[0:shape[0], 0:shape[1]]
    return (11 * c + 5 * bx + 3 * by + seed) % 17 - 8


def _table(c, dc=None):
    k = np.arange(64)
    q = 2 + 3 * ((7 * k) % 64) + c      # 2..193: all 192 entries of the three tables differ
    if dc is not None:
        q[0] = dc
    return q


QT3 = np.stack([_table(c) for c in range(3)])
# stream cases: Cb and Cr share a table, as the file format of the host coder wants
STREAM_QT = np.stack([1 + np.arange(64), 3 + 2 * np.arange(64), 3 + 2 * np.arange(64)])
STREAM_QUALITY = 75                 # the header of the device stream; the scan does not depend on it


def textured(W, H, samp, seed=0):
    """Every block: its own DC (levels up to +-48) and the three lowest AC
    terms with signs that change from block to block."""
    j = blank(W, H, samp, QT3)
    for c, g in enumerate(j["coef"]):
        q = j["qt"][c].astype(int)
        o = own(c, g.shape[:2], seed)
        g[..., 0] = o * (48 // q[0])
        by, bx = np.mgrid[0:g.shape[0], 0:g.shape[1]]
        for n, (pos, amp) in enumerate(((1, 96), (8, 96), (9, 64))):
            sign = 1 - 2 * (((bx * (n + 1) + by * (3 - n) + c + seed) >> (n & 1)) & 1)
            g[..., pos] = sign * max(1, amp // q[pos])
    return j


# ---- decoder cases -----------------------------------------------------------

BASIS_SIZE = {S444: (64, 128), SGRAY: (64, 128), S422: (64, 256), S420: (128, 256)}


@functools.lru_cache(None)
def basis(samp):
    """Block i of a component holds entry perm[i % 128] of {coefficient k
    positive, coefficient k negative}, k = 0..63, on top of its own DC; the
    product with the quant entry is about 1100 (clamps) or 240 (does not)."""
    H, W = BASIS_SIZE[samp]
    j = blank(W, H, samp, QT3)
    rng = np.random.default_rng(1000 + samp)
    for c, g in enumerate(j["coef"]):
        q = j["qt"][c].astype(int)
        flat = g.reshape(-1, 64)
        assert flat.shape[0] >= 128
        perm = rng.permutation(128)
        flat[:, 0] = own(c, g.shape[:2]).reshape(-1) * (40 // q[0])
        for i in range(flat.shape[0]):
            e = int(perm[i % 128])
            k, neg = e % 64, e >= 64
            target = 1100 if (k + (k >> 3) + c + i // 128) & 1 else 240
            v = max(1, target // q[k])
            flat[i, k] = -v if neg else v      # k = 0: the basis term replaces the signature
    j["perm_seed"] = 1000 + samp
    return j


TILE_SIZES = ((63, 127), (64, 128), (65, 129), (128, 256), (129, 257), (192, 384))


@functools.lru_cache(None)
def tiles(samp, H, W):
    return textured(W, H, samp, seed=H + W)


NARROW_W, NARROW_H = tuple(range(1, 10)), (1, 2, 3, 16, 17)


@functools.lru_cache(None)
def narrow(samp, H, W):
    return textured(W, H, samp, seed=3 * H + W)


STORE_SIZES = ((5, 13), (7, 10), (3, 7), (4, 8))
STORE_FRAMES, STORE_BUFFER, PREFILL = 3, 4, 0xA5


@functools.lru_cache(None)
def stores(samp, H, W):
    """Three frames of one size: 3 W is odd or even and H W 3 is or is not a
    multiple of four, so rows and frame bases meet every store alignment."""
    return tuple(textured(W, H, samp, seed=7 * f + 1) for f in range(STORE_FRAMES))


SAT_LEVELS = (0, 128, 255)
SAT_FLAT, SAT_HEAVY = 27, 13


@functools.lru_cache(None)
def saturate(samp):
    """MCU m < 27 is flat: its components decode to the m-th element of
    {0, 128, 255}^3 (DC -128, 0, 128 at quant 8; 128 * 8 / 8 + 128 = 256 clamps
    to 255).  These blocks carry the DC the case dictates, not their own.
    The 13 MCUs behind them are AC-heavy: random coefficients in every
    position whose samples leave 0..255 on both sides."""
    nc = len(HV[samp])
    fh, fv = HV[samp][0]
    flat_n = SAT_FLAT if nc == 3 else 3
    n = flat_n + SAT_HEAVY
    qt = np.stack([_table(c, dc=8) for c in range(3)])
    j = blank(8 * fh * n, 8 * fv, samp, qt)
    rng = np.random.default_rng(2000 + samp)
    for c, g in enumerate(j["coef"]):
        q = j["qt"][c].astype(int)
        h, v = j["hv"][c]
        o = own(c, g.shape[:2])
        for by in range(g.shape[0]):
            for bx in range(g.shape[1]):
                m = bx // h
                if m < flat_n:
                    digit = (m // 3 ** (2 - c)) % 3 if nc == 3 else m
                    g[by, bx, 0] = (-128, 0, 128)[digit]
                    continue
                while True:
                    blk = np.zeros(64, np.int16)
                    blk[0] = o[by, bx] * 4
                    lim = 300 // q[1:]
                    blk[1:] = rng.integers(-lim, lim + 1)
                    s = jpeg_ref.idct_samples(blk, q)
                    if jpeg_ref.libjpeg16_safe(blk, q) and s.min() < 0 and s.max() > 255:
                        break
                g[by, bx] = blk
    j["flat_mcus"] = flat_n
    return j


BEYOND_BLOCKS = 16


@functools.lru_cache(None)
def beyond16(samp):
    """Blocks outside libjpeg's 16-bit-safe domain and inside int32: MCU 0 is
    the block with a quantised DC of 33 at quant 255 and nothing else; the
    others hold one to three large terms on top of their own DC."""
    fh, fv = HV[samp][0]
    qt = np.stack([255 - ((3 * np.arange(64) + c) % 60) for c in range(3)])
    qt[:, 0] = 255
    j = blank(8 * fh * BEYOND_BLOCKS, 8 * fv, samp, qt)
    rng = np.random.default_rng(3000 + samp)
    for c, g in enumerate(j["coef"]):
        q = j["qt"][c].astype(int)
        h, v = j["hv"][c]
        o = own(c, g.shape[:2])
        for by in range(g.shape[0]):
            for bx in range(g.shape[1]):
                if bx // h == 0:
                    g[by, bx, 0] = 33
                    continue
                while True:
                    blk = np.zeros(64, np.int16)
                    blk[0] = o[by, bx]
                    for pos in rng.choice(np.arange(1, 64), int(rng.integers(1, 4)), replace=False):
                        blk[pos] = int(rng.integers(40, 120)) * (1 - 2 * int(rng.integers(0, 2)))
                    if not jpeg_ref.libjpeg16_safe(blk, q) and jpeg_ref.int32_safe(blk, q):
                        break
                g[by, bx] = blk
    return j


MIXED_SIZE, MIXED_BROKEN = (129, 257), 1    # (H, W); the record whose magic word is broken


@functools.lru_cache(None)
def mixed_batch():
    H, W = MIXED_SIZE
    return tuple(tiles(s, H, W) for s in ALL)


def decoder_cases(include_beyond=True):
    """{id: case} of every single-image decoder case."""
    out = {}
    for s in ALL:
        n = NAMES[s]
        out[f"basis-{n}"] = basis(s)
        for H, W in TILE_SIZES:
            out[f"tiles-{n}-{H}x{W}"] = tiles(s, H, W)
        if s in SUBSAMPLED:
            for H in NARROW_H:
                for W in NARROW_W:
                    out[f"narrow-{n}-{H}x{W}"] = narrow(s, H, W)
        for H, W in STORE_SIZES:
            for f, j in enumerate(stores(s, H, W)):
                out[f"stores-{n}-{H}x{W}-f{f}"] = j
        out[f"saturate-{n}"] = saturate(s)
        if include_beyond:
            out[f"beyond16-{n}"] = beyond16(s)
    return out


# ---- stream cases ------------------------------------------------------------

def sparse(W, H, samp, seed=0, density=1):
    """Own DC (times three) and `density` small AC terms in every block."""
    j = blank(W, H, samp, STREAM_QT)
    for c, g in enumerate(j["coef"]):
        o = own(c, g.shape[:2], seed)
        g[..., 0] = 3 * o
        by, bx = np.mgrid[0:g.shape[0], 0:g.shape[1]]
        for d in range(density):
            pos = ZIGZAG[1 + (bx + 2 * by + c + 5 * d + seed) % 11 + 11 * d]
            np.put_along_axis(g, pos[..., None], (((bx + by + d) % 5) - 2)[..., None].astype(np.int16),
                              axis=2)
    return j


def coding_sequences(j):
    """Per component the blocks [(by, bx)] in the order the scan codes them,
    split by restart segment (one MCU row each)."""
    out = [[] for _ in j["coef"]]
    for seg in jpeg_ref.scan_order(j):
        per = [[] for _ in j["coef"]]
        for c, by, bx in seg:
            per[c].append((by, bx))
        for c, p in enumerate(per):
            out[c].append(p)
    return out


AC_VALUES = sorted({s * v for s in (1, -1) for k in range(1, 10) for v in (1, 2 ** k - 1, 2 ** k)}
                   | {1023, -1023})
DC_DIFFS = sorted({s * v for s in (1, -1) for k in range(1, 12) for v in (2 ** k - 1, 2 ** k)
                   if v <= 2047})


@functools.lru_cache(None)
def sizes(samp):
    """12 x 7 MCUs.  The DCs are dictated: blocks 2n and 2n + 1 of a component
    (coding order, never across a segment) differ by DC_DIFFS[n].  Every
    block holds five of AC_VALUES."""
    fh, fv = HV[samp][0]
    j = blank(12 * 8 * fh, 7 * 8 * fv, samp, STREAM_QT)
    for c, rows in enumerate(coding_sequences(j)):
        n = 0
        for row in rows:
            assert len(row) % 2 == 0
            for by, bx in row:
                d = DC_DIFFS[(n // 2) % len(DC_DIFFS)]
                p = -((d + 1) // 2) if d > 0 else (-d) // 2
                blk = j["coef"][c][by, bx]
                blk[0] = p + d if n & 1 else p
                for i in range(5):
                    blk[ZIGZAG[1 + 3 * i + (n % 3)]] = AC_VALUES[(5 * n + i) % len(AC_VALUES)]
                n += 1
    return j


RUNS = (0, 1, 14, 15, 16, 17, 31, 32, 33, 47, 48, 62)


def run_patterns():
    """{zig-zag position: value} per pattern."""
    pats = []
    for r in RUNS:
        pats.append({r + 1: 3})
        if r + 2 <= 63:
            pats.append({1: -2, r + 2: 5})
    pats.append({60: 1, 61: -1, 62: 2, 63: -7})         # dense up to and including 63
    pats.append({k: (-1) ** k * (1 + k % 3) for k in range(1, 64)})
    pats.append({})                                     # all zero: DC and EOB alone
    pats.append({63: -1})                               # only position 63 (a run of 62)
    return pats


@functools.lru_cache(None)
def runs(samp):
    """7 x 4 MCUs; block n of a component (coding order) holds pattern n."""
    fh, fv = HV[samp][0]
    j = blank(7 * 8 * fh, 4 * 8 * fv, samp, STREAM_QT)
    pats = run_patterns()
    for c, rows in enumerate(coding_sequences(j)):
        o = own(c, j["coef"][c].shape[:2])
        n = 0
        for row in rows:
            for by, bx in row:
                blk = j["coef"][c][by, bx]
                blk[0] = 3 * o[by, bx]
                for pos, v in pats[n % len(pats)].items():
                    blk[ZIGZAG[pos]] = v
                n += 1
    return j


MAXBITS_SIZE = {S444: (8, 688), S422: (8, 1040), S420: (16, 688)}   # 258, 260, 258 blocks


@functools.lru_cache(None)
def maxbits(samp):
    """One MCU row of at least 258 blocks, each the longest block baseline can
    code: every AC +-1023, the DC dictated, alternating -1024 / 1023."""
    H, W = MAXBITS_SIZE[samp]
    j = blank(W, H, samp, STREAM_QT)
    ac = np.where(np.arange(63) % 3 == 1, -1023, 1023)
    for c, rows in enumerate(coding_sequences(j)):
        for n, (by, bx) in enumerate(rows[0]):
            blk = j["coef"][c][by, bx]
            blk[0] = 1023 if n & 1 else -1024
            blk[ZIGZAG[1:]] = ac if (n + c) & 1 else -ac
    return j


CHUNK_WIDTHS = {S444: (680, 688, 1368, 1376), S422: (1008, 1024, 1040, 2048, 2064),
                S420: (672, 688, 1360, 1376)}
CHUNK_ROWS = 10
_FILL = (0, 1, -2, 5, -9, 17, -40, 70, -130, 300, -600, 1023)


def _tune_bits(j, blocks, counts, slot, ok, rng):
    """Put filler values into zig-zag positions 1..4 of block `slot` of the
    segment until ok(counts) holds; the DC stays, so no other block changes."""
    c, by, bx = blocks[slot]
    blk = j["coef"][c][by, bx]
    pred = 0
    for c2, by2, bx2 in blocks[:slot]:
        if c2 == c:
            pred = int(j["coef"][c2][by2, bx2, 0])
    for _ in range(20000):
        if ok(counts):
            return
        blk[ZIGZAG[1:5]] = rng.choice(_FILL, 4)
        counts[slot] = jpeg_ref.block_code(blk, pred, 0 if c == 0 else 1)[1]
    raise AssertionError("no filler reaches the regime")


def chunk_targets(row, nblk):
    """(condition on the bits before block 256, condition on the segment's
    bits) of MCU row `row`; None: whatever comes."""
    first = None
    if nblk > CHUNK:
        first = (lambda b: b % 32 == 0) if row % 2 == 0 else (lambda b: b % 32 != 0)
    if row == 0:
        return first, None
    if row == 1:
        return first, lambda t: t % 32 == 0
    if row == 2:
        return first, lambda t: t % 8 == 0 and t % 32 != 0
    return first, lambda t, pad=row - 2: (-t) % 8 == pad


@functools.lru_cache(None)
def chunks(samp, W):
    """Ten segments of sparse blocks.  The first block's fillers set the bit
    offset at the 256-block chunk boundary (0 mod 32 in even rows, something
    else in odd rows), the last block's set the segment's total: row 1 a whole
    number of words, row 2 whole bytes but not words, rows 3..9 pads of 1..7."""
    fv = HV[samp][0][1]
    j = sparse(W, CHUNK_ROWS * 8 * fv, samp, seed=W)
    rng = np.random.default_rng(4000 + 10 * W + samp)
    for row, blocks in enumerate(jpeg_ref.scan_order(j)):
        counts = jpeg_ref.encode_segment(j, blocks)[1]
        first, total = chunk_targets(row, len(blocks))
        if first:
            _tune_bits(j, blocks, counts, 0, lambda n: first(sum(n[:CHUNK])), rng)
        if total:
            _tune_bits(j, blocks, counts, len(blocks) - 1, lambda n: total(sum(n)), rng)
    return j


def _tune_raw(j, blocks, ok, rng):
    """Fill blocks 0, 1 and 2 of the segment at random (block 0 sparse values,
    blocks 1 and 2 a run of 1023s) until ok(raw bytes) holds."""
    b0, b1, b2 = (j["coef"][c][y, x] for c, y, x in blocks[:3])
    for _ in range(50000):
        b0[ZIGZAG[1:]] = 0
        k = int(rng.integers(0, 30))
        b0[ZIGZAG[rng.choice(np.arange(1, 64), k, replace=False)]] = rng.choice(_FILL, k)
        b1[ZIGZAG[1:]] = 0
        b1[ZIGZAG[1:1 + int(rng.integers(0, 64))]] = 1023
        b2[ZIGZAG[1:]] = 0
        b2[ZIGZAG[1:1 + int(rng.integers(0, 64))]] = 1023
        if ok(jpeg_ref.encode_segment(j, blocks)[0]):
            return
    raise AssertionError("no filler reaches the regime")


@functools.lru_cache(None)
def stuffing(samp):
    """4 x 4 MCUs.  Row 0 and row 3: every block all +1023, whose ten value
    bits of ones run into the leading ones of the next code; row 0 is
    tuned so that raw byte 1023, the last of the compact kernel's first pass,
    is 0xFF.  Rows 1 and 2 are exactly 1024 and 1025 raw bytes long and end in
    a 1023 at position 63, so their padded last byte is 0xFF."""
    fh, fv = HV[samp][0]
    j = sparse(4 * 8 * fh, 4 * 8 * fv, samp, seed=9)
    rng = np.random.default_rng(5000 + samp)
    segs = jpeg_ref.scan_order(j)
    for row, blocks in enumerate(segs):
        for n, (c, by, bx) in enumerate(blocks):
            j["coef"][c][by, bx][ZIGZAG[1:]] = 1023 if row in (0, 3) else 0
        if row in (1, 2):
            c, by, bx = blocks[-1]
            j["coef"][c][by, bx, 63] = 1023
            for c, by, bx in blocks[3:-1]:      # all 1023 while 300 bits and more stay for the tuning
                j["coef"][c][by, bx][ZIGZAG[1:]] = 1023
                if len(jpeg_ref.encode_segment(j, blocks)[0]) > PASS_BYTES - 38:
                    j["coef"][c][by, bx][ZIGZAG[1:]] = 0
                    break
    _tune_raw(j, segs[0], lambda r: len(r) > PASS_BYTES and r[PASS_BYTES - 1] == 0xFF, rng)
    _tune_raw(j, segs[1], lambda r: len(r) == PASS_BYTES and r[-1] == 0xFF, rng)
    _tune_raw(j, segs[2], lambda r: len(r) == PASS_BYTES + 1 and r[-1] == 0xFF, rng)
    return j


ROW_COUNTS = (1, 8, 9, 10, 257)


@functools.lru_cache(None)
def rows(samp, n):
    """n MCU rows of one MCU: W = 8 (4:4:4) or 16, H = 8 n or 16 n."""
    fh, fv = HV[samp][0]
    return sparse(8 * fh, 8 * fv * n, samp, seed=n, density=2)


BATCH_WIDTH = {S444: 688, S422: 1040, S420: 688}
BATCH_BROKEN = 1


@functools.lru_cache(None)
def batch(samp):
    """Three records of one size, two segments of more than 256 blocks each,
    with 1, 3 and 5 AC terms per block: three stream lengths."""
    fv = HV[samp][0][1]
    return tuple(sparse(BATCH_WIDTH[samp], 2 * 8 * fv, samp, seed=f, density=1 + 2 * f)
                 for f in range(3))


def stream_cases():
    """{id: case} of every single-image stream case."""
    out = {}
    for s in COLOUR:
        n = NAMES[s]
        out[f"sizes-{n}"] = sizes(s)
        out[f"runs-{n}"] = runs(s)
        out[f"maxbits-{n}"] = maxbits(s)
        for W in CHUNK_WIDTHS[s]:
            out[f"chunks-{n}-w{W}"] = chunks(s, W)
        out[f"stuffing-{n}"] = stuffing(s)
        for r in ROW_COUNTS:
            out[f"rows-{n}-{r}"] = rows(s, r)
        for f, j in enumerate(batch(s)):
            out[f"batch-{n}-f{f}"] = j
    return out

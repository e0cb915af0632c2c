"""tests/jpeg_cases.py from the reference side alone: which path of the JPEG
kernels every case runs (each regime with a count above zero), that the
decoder cases lie where libjpeg's builds agree (and beyond16 does not), that
the reference entropy coder, parse() and the host coder agree on every stream
case, and that the restatement decodes the decoder cases as Pillow did
(tests/golden/jpeg_paths/pillow_sha256.json).  No GPU calls, no Pillow."""
import ctypes
import glob
import hashlib
import json
import os

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_ref
from conftest import GOLDEN
from jpeg_ref import S420, S422, S444, SGRAY, ZIGZAG

FIXTURES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg"))
                  if "reject_" not in os.path.basename(p))


@pytest.fixture(scope="module")
def decoder_cases():
    return jc.decoder_cases()


@pytest.fixture(scope="module")
def stream_cases():
    return jc.stream_cases()


@pytest.fixture(scope="module")
def coded(stream_cases):
    """id -> (scan bytes, per-segment info) of the reference coder; made once."""
    return {k: jpeg_ref.entropy_encode(j) for k, j in stream_cases.items()}


def _of(cases, name, samp):
    pre = f"{name}-{jc.NAMES[samp]}"
    return {k: v for k, v in cases.items() if k == pre or k.startswith(pre + "-")}


# ---- jpeg_ref additions ------------------------------------------------------

def test_record_has_the_layout_of_the_library():
    from rvs_amd.io_video import jpeg_record_layout
    for samp in jc.ALL:
        for H, W in ((1, 1), (17, 33), (129, 257)):
            j = jc.textured(W, H, samp, seed=5)
            lay = jpeg_record_layout(W, H, samp)
            rec = jpeg_ref.record(j)
            assert rec.dtype == np.uint8 and rec.size == lay["record_bytes"]
            assert list(rec[:32].view("<i4")) == [0x46434A52, W, H, samp, lay["ncomp"], 0, 0, 0]
            nc = lay["ncomp"]
            qt = rec[lay["qt_offset"]:lay["qt_offset"] + 128 * nc].view("<u2").reshape(nc, 64)
            np.testing.assert_array_equal(qt, j["qt"])
            for c in range(nc):
                bh, bw = lay["blocks_h"][c], lay["blocks_w"][c]
                assert j["coef"][c].shape == (bh, bw, 64)
                o = lay["coef_offset"][c]
                np.testing.assert_array_equal(
                    rec[o:o + bh * bw * 128].view("<i2").reshape(bh, bw, 64), j["coef"][c])


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_record_of_parse_is_what_the_host_decoder_writes(path):
    from rvs_amd.io_video import jpeg_coefficients
    data = open(path, "rb").read()
    np.testing.assert_array_equal(jpeg_ref.record(jpeg_ref.parse(data)), jpeg_coefficients(data))


def test_the_domain_predicates_on_the_known_blocks():
    """Quantised DC 32 and 33 at quant 255: 8160 * 4 fits int16, 8415 * 4 does
    not (the pass-1 workspace); the restatement clamps both to 255."""
    q = np.ones(64, np.uint16)
    q[0] = 255
    for dc, safe in ((32, True), (33, False), (-32, True), (-33, False)):
        blk = np.zeros(64, np.int16)
        blk[0] = dc
        assert bool(jpeg_ref.libjpeg16_safe(blk, q)) == safe
        assert bool(jpeg_ref.int32_safe(blk, q))
        assert (np.clip(jpeg_ref.idct_samples(blk, q), 0, 255) == (255 if dc > 0 else 0)).all()
    blk = np.zeros((2, 64), np.int16)
    blk[0, 1] = 129                      # the product 129 * 255 leaves int16
    blk[1, 0] = 32767                    # (in0 + in4) << 13 leaves int32
    assert list(jpeg_ref.libjpeg16_safe(blk, q.astype(int) * 0 + 255)) == [False, False]
    assert list(jpeg_ref.int32_safe(blk, q.astype(int) * 0 + 255)) == [True, False]
    for path in FIXTURES[:8]:            # every encoder output of 8-bit pixels is inside
        j = jpeg_ref.parse(open(path, "rb").read())
        for c, g in enumerate(j["coef"]):
            assert jpeg_ref.libjpeg16_safe(g, j["qt"][c]).all()


# ---- decoder cases -----------------------------------------------------------

def test_decoder_cases_lie_inside_the_libjpeg_domain_and_beyond16_outside(decoder_cases):
    inside = outside = 0
    for k, j in decoder_cases.items():
        for c, g in enumerate(j["coef"]):
            safe = jpeg_ref.libjpeg16_safe(g, j["qt"][c])
            if k.startswith("beyond16"):
                assert not safe.any(), k
                assert jpeg_ref.int32_safe(g, j["qt"][c]).all(), k
                outside += safe.size
            else:
                assert safe.all(), k
                inside += safe.size
    assert inside > 0 and outside >= 4 * jc.BEYOND_BLOCKS
    for samp in jc.ALL:                  # the block of the issue's table leads every beyond16 case
        j = jc.beyond16(samp)
        blk = j["coef"][0][0, 0]
        assert blk[0] == 33 and not blk[1:].any() and j["qt"][0][0] == 255


def test_every_block_carries_its_own_dc(decoder_cases):
    """tiles, narrow and stores: horizontal and vertical neighbours never share
    a DC, nor do the components of one position."""
    seen = 0
    for k, j in decoder_cases.items():
        if not k.startswith(("tiles", "narrow", "stores")):
            continue
        for g in j["coef"]:
            dc = g[..., 0]
            assert (dc[:, 1:] != dc[:, :-1]).all() and (dc[1:] != dc[:-1]).all(), k
            seen += dc.size
        if j["ncomp"] == 3:
            assert (j["coef"][1][..., 0] != j["coef"][2][..., 0]).all(), k
    assert seen > 0


def test_basis_holds_every_coefficient_with_both_signs_on_both_sides_of_the_clamp():
    assert len(set(jc.QT3.reshape(-1).tolist())) == 192 and jc.QT3.max() <= 255
    for samp in jc.ALL:
        j = jc.basis(samp)
        assert (j["H"], j["W"]) == jc.BASIS_SIZE[samp]
        orders = []
        for c, g in enumerate(j["coef"]):
            flat = g.reshape(-1, 64).astype(int)
            assert flat.shape[0] >= 128
            terms = []
            for blk in flat:
                nz = [k for k in np.flatnonzero(blk) if k != 0]
                assert len(nz) <= 1
                k = nz[0] if nz else 0
                terms.append((k, int(np.sign(blk[k]))))
            assert set(terms[:128]) == {(k, s) for k in range(64) for s in (1, -1)}
            orders.append(terms[:128])
            s = jpeg_ref.idct_samples(flat, j["qt"][c]).reshape(len(flat), -1)
            clamps = (s.min(axis=1) < 0) | (s.max(axis=1) > 255)
            assert clamps.sum() > 0 and (~clamps).sum() > 0
            assert (s.min(axis=1) < 0).sum() > 0 and (s.max(axis=1) > 255).sum() > 0
        assert all(orders[0] != o for o in orders[1:]) and (len(orders) < 3 or orders[1] != orders[2])


def _halo_reads(H, W, samp):
    """Pixels whose triangle filter reads a chroma sample that the tile to the
    {left, right, above, below} owns, from the geometry alone."""
    fh, fv = jc.HV[samp][0]
    dw, dh = -(-W // fh), -(-H // fv)
    y, x = np.mgrid[0:H, 0:W]
    out = dict(left=0, right=0, above=0, below=0)
    if fh == 2 and dw > 2:
        cx = x >> 1
        nb = np.clip(np.where(x & 1, cx + 1, cx - 1), 0, dw - 1)
        owner, tile = nb // (jc.TILE_W // 2), x // jc.TILE_W
        out["left"], out["right"] = int((owner < tile).sum()), int((owner > tile).sum())
    if fv == 2:
        cy = y >> 1
        nb = np.clip(np.where(y & 1, cy + 1, cy - 1), 0, dh - 1)
        owner, tile = nb // (jc.TILE_H // 2), y // jc.TILE_H
        out["above"], out["below"] = int((owner < tile).sum()), int((owner > tile).sum())
    return out


def test_tiles_read_their_halo_from_every_side():
    for samp in jc.SUBSAMPLED:
        total = dict(left=0, right=0, above=0, below=0)
        for H, W in jc.TILE_SIZES:
            got = _halo_reads(H, W, samp)
            ntx, nty = -(-W // jc.TILE_W), -(-H // jc.TILE_H)
            # one pixel column / row per inner tile border: the even pixel behind it reads
            # back, the odd pixel before it reads ahead
            want_x = H * (ntx - 1)
            want_y = W * (nty - 1) if samp == S420 else 0
            assert got == dict(left=want_x, right=want_x, above=want_y, below=want_y), (H, W)
            for k in total:
                total[k] += got[k]
        assert total["left"] > 0 and total["right"] > 0
        if samp == S420:
            assert total["above"] > 0 and total["below"] > 0
        else:
            assert total["above"] == 0 and total["below"] == 0      # see jpeg_cases.UNREACHED
    # sizes on, one below and one above the tile grid; an interior tile in the largest
    for H, W in jc.TILE_SIZES:
        assert (H % jc.TILE_H, W % jc.TILE_W) in ((63, 127), (0, 0), (1, 1))
    H, W = jc.TILE_SIZES[-1]
    assert -(-W // jc.TILE_W) >= 3 and -(-H // jc.TILE_H) >= 3
    assert sum(1 for H, W in jc.TILE_SIZES if H > jc.TILE_H) >= 4   # every sampling crosses downwards


def test_narrow_reaches_the_replicated_and_the_first_filtered_chroma_planes():
    widths, heights = set(), set()
    for samp in jc.SUBSAMPLED:
        for H in jc.NARROW_H:
            for W in jc.NARROW_W:
                j = jc.narrow(samp, H, W)
                assert (j["W"], j["H"]) == (W, H)
                widths.add(-(-W // 2))
                if samp == S420:
                    heights.add(-(-H // 2))
    assert {1, 2, 3} <= widths and 1 in heights and 2 in heights


def test_stores_meet_both_store_paths():
    """The kernel stores three dwords where four pixels fit and the address is
    a multiple of four, bytes elsewhere."""
    dword = byte_tail = byte_misaligned = 0
    bases = set()
    for H, W in jc.STORE_SIZES:
        for f in range(jc.STORE_FRAMES):
            base = f * H * W * 3
            bases.add(base % 4)
            for y in range(H):
                for x in range(0, W, 4):
                    a = base + (y * W + x) * 3
                    if x + 4 > W:
                        byte_tail += 1
                    elif a % 4:
                        byte_misaligned += 1
                    else:
                        dword += 1
    assert dword > 0 and byte_tail > 0 and byte_misaligned > 0 and len(bases) >= 2
    assert jc.STORE_BUFFER == jc.STORE_FRAMES + 1


def test_saturate_reaches_every_clamp():
    for samp in jc.ALL:
        j = jc.saturate(samp)
        planes = jpeg_ref.full_planes(j)
        heavy = 0
        for c, g in enumerate(j["coef"]):
            h = j["hv"][c][0]
            blocks = g[:, j["flat_mcus"] * h:]
            s = jpeg_ref.idct_samples(blocks, j["qt"][c])
            assert (s < 0).sum() > 0 and (s > 255).sum() > 0
            assert (np.count_nonzero(blocks[..., 1:], axis=-1) > 32).all()
            heavy += blocks.shape[0] * blocks.shape[1]
        assert heavy >= jc.SAT_HEAVY
        if samp == SGRAY:
            assert set(jc.SAT_LEVELS) <= set(np.unique(planes[0]))
            continue
        seen = {tuple(t) for t in np.unique(np.stack(planes, -1).reshape(-1, 3), axis=0)}
        assert {(a, b, c) for a in jc.SAT_LEVELS for b in jc.SAT_LEVELS for c in jc.SAT_LEVELS} <= seen
        rgb = jpeg_ref.ycc_to_rgb_unclamped(*planes)
        for ch in range(3):
            assert (rgb[..., ch] < 0).sum() > 0 and (rgb[..., ch] > 255).sum() > 0


def test_mixed_batch_is_one_record_per_sampling():
    cases = jc.mixed_batch()
    assert [j["sampling"] for j in cases] == list(jc.ALL) and 0 <= jc.MIXED_BROKEN < 4
    assert all((j["H"], j["W"]) == jc.MIXED_SIZE for j in cases)
    assert len({jpeg_ref.record(j).size for j in cases}) == 4       # hence the zero padding


def test_the_restatement_decodes_the_cases_as_pillow_did(decoder_cases):
    want = json.load(open(os.path.join(GOLDEN, "jpeg_paths", "pillow_sha256.json")))
    ids = [k for k in decoder_cases if not k.startswith("beyond16")]
    assert sorted(want) == sorted(ids) and len(ids) > 100
    for k in ids:
        got = hashlib.sha256(np.ascontiguousarray(jpeg_ref.to_rgb(decoder_cases[k])).tobytes())
        assert got.hexdigest() == want[k], k


# ---- stream cases: the regimes -----------------------------------------------

def _dc_diffs_and_ac(j):
    """Per table class the set of DC differences and the list of AC blocks in
    zig-zag order, walking the scan."""
    diffs, blocks = (set(), set()), ([], [])
    for seg in jpeg_ref.scan_order(j):
        pred = [0] * 3
        for c, by, bx in seg:
            blk = j["coef"][c][by, bx].astype(int)
            t = 0 if c == 0 else 1
            diffs[t].add(int(blk[0]) - pred[c])
            pred[c] = int(blk[0])
            blocks[t].append(blk[ZIGZAG])
    return diffs, blocks


def test_sizes_hold_every_category_boundary():
    assert {1, -1, 511, -511, 512, -512, 1023, -1023} <= set(jc.AC_VALUES)
    assert {1, -1, 2047, -2047, 1024, -1024, 1023, -1023} <= set(jc.DC_DIFFS)
    assert {abs(v).bit_length() for v in jc.AC_VALUES} == set(range(1, 11))
    assert {abs(v).bit_length() for v in jc.DC_DIFFS} == set(range(1, 12))
    for samp in jc.COLOUR:
        diffs, blocks = _dc_diffs_and_ac(jc.sizes(samp))
        for t in (0, 1):
            assert set(jc.DC_DIFFS) <= diffs[t]
            assert set(jc.AC_VALUES) <= {int(v) for b in blocks[t] for v in b[1:] if v}


def _zero_runs(zz):
    out, run = [], 0
    for v in zz[1:]:
        if v == 0:
            run += 1
        else:
            out.append(run)
            run = 0
    return out


def test_runs_hold_every_run_and_both_block_ends():
    for samp in jc.COLOUR:
        _, blocks = _dc_diffs_and_ac(jc.runs(samp))
        for t in (0, 1):
            got = {r for b in blocks[t] for r in _zero_runs(b)}
            assert set(jc.RUNS) <= got
            assert sum(1 for b in blocks[t] if b[63] != 0) >= 3          # no EOB
            assert sum(1 for b in blocks[t] if not b[1:].any()) >= 1     # DC and EOB alone
            assert sum(1 for b in blocks[t] if b[63] != 0 and not b[1:63].any()) >= 1
            assert sum(1 for b in blocks[t] if b[1:].all()) >= 1         # no zero at all


def test_maxbits_fills_the_bit_buffer(coded):
    assert jc.BLOCK_BITS_MAX == (1658, 1408)        # chroma: see jpeg_cases.UNREACHED
    for samp in jc.COLOUR:
        j = jc.maxbits(samp)
        (seg,) = coded[f"maxbits-{jc.NAMES[samp]}"][1]
        order = jpeg_ref.scan_order(j)[0]
        assert len(order) >= 258 and len(order) > jc.CHUNK
        for (c, _, _), n in zip(order, seg["block_bits"]):
            assert n == jc.BLOCK_BITS_MAX[0 if c == 0 else 1]
        for g in j["coef"]:
            assert (np.abs(g[..., 1:].astype(int)) == 1023).all()
            assert set(np.unique(g[..., 0])) == {-1024, 1023}
        # the LDS bit buffer holds 256 blocks of 1660 bits: the fullest chunk fits
        assert 256 * 1408 < sum(seg["block_bits"][:jc.CHUNK]) <= 256 * 1660


def test_chunks_meet_every_boundary_and_padding_regime(coded):
    for samp in jc.COLOUR:
        sizes = set()
        got = dict(boundary_word=0, boundary_inside=0, total_word=0, total_byte=0)
        pads = {p: 0 for p in range(8)}
        for k, (_, info) in _of(coded, "chunks", samp).items():
            for seg in info:
                bits = seg["block_bits"]
                sizes.add(len(bits))
                for b in range(jc.CHUNK, len(bits), jc.CHUNK):     # blocks follow this boundary
                    off = sum(bits[:b]) % 32
                    got["boundary_word" if off == 0 else "boundary_inside"] += 1
                total = sum(bits)
                assert seg["raw_bytes"] == -(-total // 8)
                got["total_word"] += total % 32 == 0
                got["total_byte"] += total % 8 == 0 and total % 32 != 0
                pads[-total % 8] += 1
                assert sorted(bits)[len(bits) // 2] < 40 and max(bits) < 160    # sparse
        assert all(v > 0 for v in got.values()), got
        assert all(pads[p] > 0 for p in range(1, 8)), pads
        want = {S444: {255, 258, 513, 516}, S422: {252, 256, 260, 512, 516},
                S420: {252, 258, 510, 516}}[samp]
        assert sizes == want


def test_stuffing_meets_every_byte_regime(coded):
    for samp in jc.COLOUR:
        scan, info = coded[f"stuffing-{jc.NAMES[samp]}"]
        raws = [seg["raw"] for seg in info]
        assert len(raws[0]) > jc.PASS_BYTES and raws[0][jc.PASS_BYTES - 1] == 0xFF
        assert len(raws[1]) == jc.PASS_BYTES and len(raws[2]) == jc.PASS_BYTES + 1
        assert raws[1][-1] == 0xFF and raws[2][-1] == 0xFF
        assert sum(info[1]["block_bits"]) % 8 != 0 or sum(info[2]["block_bits"]) % 8 != 0
        # a block of 1023s: ten value bits of ones, then at least eight ones of the next
        # code; eighteen ones in a row always cover a whole byte, so one byte in four
        # (26 bits per coefficient at the most) is 0xFF
        for r in (raws[0], raws[3]):
            assert r.count(0xFF) * 4 >= len(r)
        for seg in info:
            assert seg["stuffed_bytes"] == seg["raw_bytes"] + seg["raw"].count(0xFF)
        assert len(scan) == sum(seg["stuffed_bytes"] + 2 for seg in info)


def test_rows_wrap_the_restart_index_and_need_two_passes_of_the_segment_sum(coded):
    assert 257 in jc.ROW_COUNTS and 10 in jc.ROW_COUNTS
    for samp in jc.COLOUR:
        fh, fv = jc.HV[samp][0]
        for n in jc.ROW_COUNTS:
            j = jc.rows(samp, n)
            assert (j["W"], j["H"]) == (8 * fh, 8 * fv * n)
            scan, info = coded[f"rows-{jc.NAMES[samp]}-{n}"]
            assert len(info) == n
            assert scan.count(b"\xff\xd0") == (n - 1 + 7) // 8 and scan.endswith(b"\xff\xd9")
    assert jc.rows(S444, 257)["H"] == 2056 and jc.rows(S420, 257)["H"] == 4112


def _capacity_points(scan):
    """Offsets into the scan: of a stuffed zero, and of the second byte of an RST."""
    zero = scan.find(b"\xff\x00") + 1
    rst = next((i + 1 for i in range(len(scan) - 1)
                if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7), 0)
    return zero, rst


def test_capacity_points_exist(coded):
    for samp in jc.COLOUR:
        zero, rst = _capacity_points(coded[f"maxbits-{jc.NAMES[samp]}"][0])
        assert zero > 0 and rst == 0        # one segment
        zero, rst = _capacity_points(coded[f"stuffing-{jc.NAMES[samp]}"][0])
        assert zero > 0 and rst > 0


def test_batch_records_differ_in_length_and_span_chunks(coded):
    for samp in jc.COLOUR:
        got = [coded[f"batch-{jc.NAMES[samp]}-f{f}"] for f in range(3)]
        assert len({len(scan) for scan, _ in got}) == 3
        for _, info in got:
            assert len(info) == 2 and all(len(seg["block_bits"]) > jc.CHUNK for seg in info)


# ---- stream cases: reference coder, parse() and the host coder agree ---------

def _host_encode(rec, ri):
    from rvs_amd import _lib
    cap = 700 + 2 * rec.size
    out = np.zeros(cap, np.uint8)
    n = ctypes.c_size_t(0)
    st = _lib.load().rv_jpeg_encode_coef(rec.ctypes.data, rec.size, ri, out.ctypes.data, cap,
                                         ctypes.addressof(n))
    assert st == 0, _lib.load().rv_last_error()
    return out[:n.value].tobytes()


@pytest.mark.parametrize("name", ["sizes", "runs", "maxbits", "chunks", "stuffing", "rows", "batch"])
@pytest.mark.parametrize("samp", jc.COLOUR, ids=[jc.NAMES[s] for s in jc.COLOUR])
def test_reference_coder_parse_and_host_coder_agree(stream_cases, coded, name, samp):
    from rvs_amd.io_video import jpeg_coefficients
    from rvs_amd.kernels import jpeg_file_header
    cases = _of(stream_cases, name, samp)
    assert cases
    for k, j in cases.items():
        scan = coded[k][0]
        mx = j["coef"][1].shape[1]
        header = jpeg_file_header(j["W"], j["H"], samp, jc.STREAM_QUALITY, mx)
        back = jpeg_ref.parse(header + scan)
        assert (back["W"], back["H"], back["sampling"]) == (j["W"], j["H"], samp)
        for a, b in zip(back["coef"], j["coef"]):
            np.testing.assert_array_equal(a, b, err_msg=k)
        rec = jpeg_ref.record(j)
        host = _host_encode(rec, mx)
        _, start = jpeg_ref.segments(host)
        assert host[start:] == scan, k
        np.testing.assert_array_equal(jpeg_coefficients(host), rec, err_msg=k)

"""Every path of the JPEG kernels on hand-built coefficient records
(tests/jpeg_cases.py; tests/test_jpeg_cases_cpu.py proves which path each case
runs).  The decoder (csrc/jpeg.hip) against jpeg_ref.to_rgb, the entropy and
compact kernels (csrc/jpeg_enc.hip) against jpeg_ref.entropy_encode: exact
equality everywhere, and nothing written beyond a frame, an image or a
capacity.  Pillow is not needed."""
import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_ref
from jpeg_ref import S420, S422

pytestmark = pytest.mark.gpu

PREFILL = jc.PREFILL
MAGIC, OVERFLOW, BAD_RECORD = 0x534A5652, 1, 2
SAMP_IDS = [jc.NAMES[s] for s in jc.ALL]
COLOUR_IDS = [jc.NAMES[s] for s in jc.COLOUR]


def _bgr(j):
    return np.ascontiguousarray(jpeg_ref.to_rgb(j)[..., ::-1])


def _decode(cuda, records, W, H, frames):
    """records (S, bytes) u8 -> the (frames, H, W, 3) host buffer whose first S
    frames the kernel was given; the rest is the guard."""
    from rvs_amd.kernels import jpeg_to_bgr
    S = records.shape[0]
    buf = torch.full((frames, H, W, 3), PREFILL, dtype=torch.uint8, device=cuda)
    jpeg_to_bgr(torch.from_numpy(records).to(cuda), W, H, out=buf[:S])
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _check_single(cuda, k, j):
    got = _decode(cuda, jpeg_ref.record(j)[None], j["W"], j["H"], 2)
    np.testing.assert_array_equal(got[0], _bgr(j), err_msg=k)
    assert (got[1] == PREFILL).all(), f"{k}: the frame behind the batch was written"


# narrow is about chroma planes one to three samples wide: the subsampled samplings only
DECODER_GROUPS = [(name, samp) for name in ("basis", "tiles", "narrow", "stores", "saturate",
                                            "beyond16")
                  for samp in jc.ALL if name != "narrow" or samp in jc.SUBSAMPLED]


@pytest.mark.parametrize("name,samp", DECODER_GROUPS,
                         ids=[f"{n}-{jc.NAMES[s]}" for n, s in DECODER_GROUPS])
def test_decoder_case_equals_the_restatement(cuda, name, samp):
    pre = f"{name}-{jc.NAMES[samp]}"
    cases = {k: j for k, j in jc.decoder_cases().items() if k == pre or k.startswith(pre + "-")}
    assert cases
    for k, j in cases.items():
        _check_single(cuda, k, j)


@pytest.mark.parametrize("samp", jc.ALL, ids=SAMP_IDS)
def test_stores_as_a_batch_into_the_head_of_a_longer_buffer(cuda, samp):
    for H, W in jc.STORE_SIZES:
        frames = jc.stores(samp, H, W)
        recs = np.stack([jpeg_ref.record(j) for j in frames])
        got = _decode(cuda, recs, W, H, jc.STORE_BUFFER)
        for f, j in enumerate(frames):
            np.testing.assert_array_equal(got[f], _bgr(j), err_msg=f"{H}x{W} frame {f}")
        assert (got[jc.STORE_FRAMES:] == PREFILL).all()


def test_mixed_batch_of_every_sampling_with_a_broken_record(cuda):
    cases = jc.mixed_batch()
    H, W = jc.MIXED_SIZE
    recs = [jpeg_ref.record(j) for j in cases]
    stride = max(r.size for r in recs)
    batch = np.zeros((len(recs), stride), np.uint8)
    for r, row in zip(recs, batch):
        row[:r.size] = r
    batch[jc.MIXED_BROKEN, 0] ^= 0xFF
    got = _decode(cuda, batch, W, H, len(recs) + 1)
    for f, j in enumerate(cases):
        if f == jc.MIXED_BROKEN:
            assert (got[f] == PREFILL).all()
        else:
            np.testing.assert_array_equal(got[f], _bgr(j), err_msg=jc.NAMES[j["sampling"]])
    assert (got[len(recs)] == PREFILL).all()


# ---- streams -----------------------------------------------------------------

def _want(j):
    """(header + scan) of the image the device must write, segments."""
    from rvs_amd.kernels import jpeg_file_header
    mx = j["coef"][1].shape[1]
    header = jpeg_file_header(j["W"], j["H"], j["sampling"], jc.STREAM_QUALITY, mx)
    return header + jpeg_ref.entropy_encode(j)[0], j["coef"][1].shape[0]


def _streams(cuda, records, j, capacity=None, slack=64):
    """Run the entropy and compact kernels; the host copy of the (S, bound +
    slack) buffer, prefilled, and the capacity used."""
    from rvs_amd.kernels import jpeg_coef_to_stream, jpeg_stream_bound
    bound = jpeg_stream_bound(j["W"], j["H"], j["sampling"])
    cap = bound if capacity is None else capacity
    out = torch.full((records.shape[0], bound + slack), PREFILL, dtype=torch.uint8, device=cuda)
    jpeg_coef_to_stream(torch.from_numpy(records).to(cuda), j["W"], j["H"], j["sampling"],
                        jc.STREAM_QUALITY, capacity=cap, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cap


def _check_stream(host, cap, want, segments, what):
    assert list(host[:16].view(np.uint32)) == \
        [MAGIC, len(want), OVERFLOW if 16 + len(want) > cap else 0, segments], what
    end = min(cap, 16 + len(want))
    assert host[16:end].tobytes() == want[:end - 16], what
    assert (host[end:] == PREFILL).all(), f"{what}: bytes behind the image or the capacity"


@pytest.mark.parametrize("samp", jc.COLOUR, ids=COLOUR_IDS)
@pytest.mark.parametrize("name", ["sizes", "runs", "maxbits", "chunks", "stuffing", "rows"])
def test_stream_case_equals_the_reference_coder(cuda, name, samp):
    pre = f"{name}-{jc.NAMES[samp]}"
    cases = {k: j for k, j in jc.stream_cases().items() if k == pre or k.startswith(pre + "-")}
    assert cases
    for k, j in cases.items():
        want, segments = _want(j)
        host, cap = _streams(cuda, jpeg_ref.record(j)[None], j)
        assert 16 + len(want) <= cap, k
        _check_stream(host[0], cap, want, segments, k)


@pytest.mark.parametrize("samp", jc.COLOUR, ids=COLOUR_IDS)
def test_capacity_ends_inside_a_stuffed_pair_inside_a_marker_and_at_the_image(cuda, samp):
    for j, has_rst in ((jc.maxbits(samp), False), (jc.stuffing(samp), True)):
        want, segments = _want(j)
        scan_at = len(want) - len(jpeg_ref.entropy_encode(j)[0])
        scan = want[scan_at:]
        zero = scan.find(b"\xff\x00") + 1
        rst = next((i + 1 for i in range(len(scan) - 1)
                    if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7), 0)
        assert zero > 0 and (rst > 0) == has_rst
        caps = [16 + scan_at + zero, 16 + len(want), 16 + len(want) - 1]
        if has_rst:
            caps.append(16 + scan_at + rst)
        rec = jpeg_ref.record(j)[None]
        for cap in caps:
            host, _ = _streams(cuda, rec, j, capacity=cap)
            assert host[0, cap - 1] == 0xFF or cap >= 16 + len(want) - 1
            _check_stream(host[0], cap, want, segments, f"capacity {cap} of {16 + len(want)}")


@pytest.mark.parametrize("samp", jc.COLOUR, ids=COLOUR_IDS)
def test_batch_of_three_lengths_with_an_invalid_record(cuda, samp):
    cases = jc.batch(samp)
    recs = np.stack([jpeg_ref.record(j) for j in cases])
    recs[jc.BATCH_BROKEN, 4:8] = 0          # another width
    host, cap = _streams(cuda, recs, cases[0], slack=0)
    for f, j in enumerate(cases):
        if f == jc.BATCH_BROKEN:
            assert list(host[f, :16].view(np.uint32)) == [MAGIC, 0, BAD_RECORD, 0]
            assert (host[f, 16:] == PREFILL).all()
        else:
            want, segments = _want(j)
            _check_stream(host[f], cap, want, segments, f"record {f}")


# ---- both halves ---------------------------------------------------------------

def test_round_trip_of_multi_tile_records(cuda):
    """The decoder on a record equals the decoder on the image the device wrote
    from it, with the header's quant tables in the record."""
    from rvs_amd import _lib
    from rvs_amd.io_video import decode_jpeg
    from rvs_amd.kernels import jpeg_to_bgr
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    assert _lib.load().rv_jpeg_quant_tables(jc.STREAM_QUALITY, luma.ctypes.data,
                                            chroma.ctypes.data) == 0
    for samp, (H, W) in ((S420, (129, 257)), (S422, (192, 384))):
        j = dict(jc.tiles(samp, H, W), qt=np.stack([luma, chroma, chroma]))
        rec = jpeg_ref.record(j)
        want, segments = _want(j)
        host, cap = _streams(cuda, rec[None], j)
        _check_stream(host[0], cap, want, segments, f"{H}x{W}")
        direct = jpeg_to_bgr(torch.from_numpy(rec).to(cuda), W, H)
        back = decode_jpeg(host[0, 16:16 + len(want)].tobytes(), device=cuda)
        assert torch.equal(direct, back)
        np.testing.assert_array_equal(direct.cpu().numpy(), _bgr(j))

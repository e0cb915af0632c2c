"""The JPEG encoder on the GPU, the Motion-JPEG sink and preview.record:
byte for byte the files Pillow (libjpeg-turbo) wrote for the pixels of
tests/golden/jpeg_enc (quality=q, subsampling=s, restart_marker_rows=1)."""
import os

import numpy as np
import pytest
import torch

import jpeg_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EDIR = os.path.join(GOLDEN, "jpeg_enc")
NAMES = sorted(os.path.basename(p)[:-4] for p in os.listdir(EDIR) if p.endswith(".jpg"))
CLIP = "clip_40x56_420_q90"


def _params(name):
    _, s, q, _ = name.split("_")
    return s, int(q[1:])


def _file(name):
    return open(os.path.join(EDIR, name + ".jpg"), "rb").read()


@pytest.fixture(scope="module")
def pixels():
    """name -> BGR input pixels; read once, never written."""
    z = np.load(os.path.join(EDIR, "input.npz"))
    out = {k: np.ascontiguousarray(z[k][..., ::-1]) for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def decoded():
    z = np.load(os.path.join(EDIR, "decoded.npz"))
    return {k: np.ascontiguousarray(z[k][..., ::-1]) for k in z.files}


@pytest.fixture(scope="module")
def clip_images():
    return jpeg_ref.split_frames(open(os.path.join(EDIR, CLIP + ".mjpeg"), "rb").read())


def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)


@pytest.mark.parametrize("name", NAMES)
def test_coefficient_records_equal_the_files(cuda, pixels, name):
    from rvs_amd.io_video import jpeg_coefficients
    from rvs_amd.kernels import bgr_to_jpeg_coef
    s, q = _params(name)
    rec = bgr_to_jpeg_coef(_dev(pixels[name], cuda), q, s)
    want = jpeg_coefficients(_file(name))
    assert tuple(rec.shape) == (1, want.size)
    np.testing.assert_array_equal(rec[0].cpu().numpy(), want)


@pytest.mark.parametrize("name", NAMES)
def test_encode_jpeg_equals_the_file(cuda, pixels, name):
    from rvs_amd.io_video import encode_jpeg
    s, q = _params(name)
    got = encode_jpeg(_dev(pixels[name], cuda), quality=q, sampling=s)
    assert len(got) == 1
    assert got[0] == _file(name)


def test_a_batch_of_frames_with_different_lengths(cuda, pixels, clip_images):
    from rvs_amd.io_video import encode_jpeg
    from rvs_amd.kernels import bgr_to_jpeg_coef, jpeg_coef_to_stream, jpeg_to_bgr
    x = _dev(pixels[CLIP][[0, 1, 4]], cuda)
    got = encode_jpeg(x, quality=90, sampling="420")
    assert got == [clip_images[i] for i in (0, 1, 4)]
    assert len({len(g) for g in got}) == 3
    # the two halves on their own; the decoder reads the encoder's records
    from rvs_amd.io_video.sink import stream_payloads
    rec = bgr_to_jpeg_coef(x, 90, "420")
    assert stream_payloads(jpeg_coef_to_stream(rec, 56, 40, "420", 90)) == got
    back = jpeg_to_bgr(rec, 56, 40)
    from rvs_amd.io_video import decode_jpeg
    for i in range(3):
        assert torch.equal(back[i], decode_jpeg(got[i], device=cuda))
    # a record of another size is flagged, and nothing but its header is written
    bad = rec.clone()
    bad[1, 4:8] = 0
    out = torch.full((3, 8192), 0xA5, dtype=torch.uint8, device=cuda)
    jpeg_coef_to_stream(bad, 56, 40, "420", 90, out=out)
    hdr = out[:, :16].cpu().numpy().view(np.uint32)
    assert list(hdr[:, 2]) == [0, 2, 0] and hdr[1, 1] == 0
    assert bool((out[1, 16:] == 0xA5).all())
    assert out[2, 16:16 + len(got[2])].cpu().numpy().tobytes() == got[2]


@pytest.mark.parametrize("name", NAMES)
def test_round_trip_equals_pillows_decode(cuda, pixels, decoded, name):
    from rvs_amd.io_video import decode_jpeg, encode_jpeg
    s, q = _params(name)
    img = encode_jpeg(_dev(pixels[name], cuda), quality=q, sampling=s)[0]
    np.testing.assert_array_equal(decode_jpeg(img, device=cuda).cpu().numpy(), decoded[name])


def test_capacity_is_never_exceeded(cuda, pixels):
    from rvs_amd.kernels import jpeg_encode, jpeg_stream_bound
    name = "37x91_444_q100_noise"
    want = _file(name)
    x = _dev(pixels[name], cuda)
    bound = jpeg_stream_bound(91, 37, "444")
    assert bound >= 16 + len(want)
    for cap in (16 + len(want) - 1, 16 + len(want) // 2, 700, 16):
        out = torch.full((1, bound), 0xA5, dtype=torch.uint8, device=cuda)
        jpeg_encode(x, 100, "444", capacity=cap, out=out)
        host = out[0].cpu().numpy()
        magic, n, flags, segs = host[:16].view(np.uint32)
        assert (magic, n, flags, segs) == (0x534A5652, len(want), 1, 5)
        assert (host[cap:] == 0xA5).all(), f"capacity {cap}: bytes behind it were written"
        assert host[16:cap].tobytes() == want[:cap - 16]
    out = torch.full((1, bound + 64), 0xA5, dtype=torch.uint8, device=cuda)
    jpeg_encode(x, 100, "444", capacity=bound, out=out)     # with the bound it fits
    host = out[0].cpu().numpy()
    assert list(host[:16].view(np.uint32)) == [0x534A5652, len(want), 0, 5]
    assert host[16:16 + len(want)].tobytes() == want and (host[bound:] == 0xA5).all()
    out = torch.full((1, bound), 0xA5, dtype=torch.uint8, device=cuda)
    jpeg_encode(x, 100, "444", capacity=16 + len(want), out=out)    # exactly enough
    host = out[0].cpu().numpy()
    assert host[8:12].view(np.uint32)[0] == 0 and host[16:16 + len(want)].tobytes() == want
    assert (host[16 + len(want):] == 0xA5).all()


def test_multistream_sink_writes_what_video_source_reads(cuda, pixels, clip_images, tmp_path):
    """Five frames on each of three streams (stream s starts at frame s of the
    clip), nbuf = 2 < 5 so every ring wraps."""
    from rvs_amd.io_video import MultiStreamSink, VideoSource, decode_jpeg
    clip = _dev(pixels[CLIP], cuda)
    paths = [str(tmp_path / f"cam{s}.mjpeg") for s in range(3)]
    sink = MultiStreamSink(paths, (40, 56), quality=90, sampling="420", device=cuda, nbuf=2)
    order = [[(f + s) % 5 for f in range(5)] for s in range(3)]
    for f in range(5):
        sink.write(torch.stack([clip[order[s][f]] for s in range(3)]))
    sink.flush()
    stats = sink.stats()
    sink.close()
    for s in range(3):
        want = b"".join(clip_images[i] for i in order[s])
        assert open(paths[s], "rb").read() == want
        st = stats[s]
        assert (st["submitted"], st["written"], st["overflowed"], st["failed"]) == (5, 5, 0, 0)
        assert st["bytes_written"] == len(want)
        assert st["bytes_written"] <= st["bytes_copied"] <= st["bytes_written"] + 5 * (4096 + 16)
        src = VideoSource(paths[s], device=cuda)
        for i in order[s]:
            fr = src.read(device=True)
            assert fr.ok
            assert torch.equal(fr.image, decode_jpeg(clip_images[i], device=cuda))
        assert not src.read().ok
        src.release()


def test_sink_reports_a_frame_that_does_not_fit(cuda, pixels, tmp_path):
    from rvs_amd import _lib
    from rvs_amd.io_video import VideoSink
    clip = pixels[CLIP]
    sink = VideoSink(str(tmp_path / "small.mjpeg"), (40, 56), quality=90, sampling="420",
                     device=cuda, capacity=2048)       # the noise frame needs more
    sink.write(np.array(clip[0]))
    sink.write(_dev(clip[1], cuda))
    with pytest.raises(_lib.RVError, match=r"small\.mjpeg: frame 1: .*overflowed the capacity"):
        sink._m.flush()
    sink.write(np.array(clip[2]))                       # reported once; the sink goes on
    assert sink.stats()["overflowed"] == 1
    sink.release()
    st = open(tmp_path / "small.mjpeg", "rb").read()
    assert len(jpeg_ref.split_frames(st)) == 2          # the frames that fitted are in the file
    with pytest.raises(ValueError, match="no MP4 muxer"):
        VideoSink(str(tmp_path / "x.mp4"), (40, 56))


def _dets(res):
    return [[(d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id, d.track_id) for d in r] for r in res]


def test_engine_step_records_proc(cuda, pixels, tmp_path):
    """preview.record on: the files hold a JPEG of every step's proc frames,
    and the detections are those of the same steps without recording."""
    from rvs_amd.config import load_config
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.io_video import decode_jpeg, encode_jpeg
    frames = _dev(pixels[CLIP], cuda)
    runs = {}
    for rec in (False, True):
        cfg = load_config()
        cfg["detect"]["weights"] = "synthetic"
        cfg["preview"]["record"] = {"enable": rec, "path": str(tmp_path / "proc{stream}.mjpeg"),
                                    "fps": 30, "quality": 85, "sampling": "422"}
        eng = RoadVisionEngine(cfg, 2, (40, 56), device=cuda)
        assert (eng.recorder is not None) == rec
        procs, dets = [], []
        for f in range(3):
            ts = torch.full((2,), f / 30.0, dtype=torch.float64, device=cuda)
            out = eng.step(torch.stack([frames[f], frames[f + 1]]), ts)
            dets.append(_dets(eng.results(out)))
            procs.append(out["proc"].clone())
        eng.close()
        runs[rec] = (procs, dets)
    assert runs[True][1] == runs[False][1]
    for a, b in zip(runs[True][0], runs[False][0]):
        assert torch.equal(a, b)
    for s in range(2):
        images = jpeg_ref.split_frames(open(tmp_path / f"proc{s}.mjpeg", "rb").read())
        assert len(images) == 3
        for f, img in enumerate(images):
            proc = runs[True][0][f][s]
            assert img == encode_jpeg(proc, quality=85, sampling="422")[0]
            assert jpeg_ref.parse(img)["sampling"] == jpeg_ref.S422
            assert torch.equal(decode_jpeg(img, device=cuda),
                               decode_jpeg(encode_jpeg(proc, 85, "422")[0], device=cuda))
    assert not os.path.exists(tmp_path / "proc2.mjpeg")


def test_engine_step_unit_records_every_step_of_the_unit(cuda, pixels, tmp_path):
    """Pair mode: one step_unit of two steps writes two frames per stream, in
    step order."""
    from rvs_amd.config import load_config
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.handback import Record
    from rvs_amd.io_video import encode_jpeg
    frames = _dev(pixels[CLIP], cuda)
    cfg = load_config()
    cfg["detect"]["weights"] = "synthetic"
    cfg["preview"]["record"] = {"enable": True, "path": str(tmp_path / "u{stream}.mjpg")}
    eng = RoadVisionEngine(cfg, 2, (40, 56), device=cuda, pair=2)
    recs = [Record(2, eng.detector.max_det, cuda) for _ in range(2)]
    ts = [torch.full((2,), h / 30.0, dtype=torch.float64, device=cuda) for h in range(2)]
    outs = eng.step_unit([frames[0:2], frames[2:4]], ts, recs)
    procs = [o["proc"].clone() for o in outs]
    eng.close()
    for s in range(2):
        images = jpeg_ref.split_frames(open(tmp_path / f"u{s}.mjpg", "rb").read())
        assert images == [encode_jpeg(p[s], quality=95, sampling="420")[0] for p in procs]


def test_random_sweep_against_pillow(cuda):
    """Wider than the fixtures, where Pillow is installed: random sizes,
    samplings, qualities and contents, and one 1080 x 1920 frame."""
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    from rvs_amd.io_video import encode_jpeg
    rng = np.random.default_rng(2027)
    cases = [(int(rng.integers(1, 200)), int(rng.integers(1, 400))) for _ in range(18)]
    cases.append((1080, 1920))
    for k, (H, W) in enumerate(cases):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if k % 2:
            img = np.sort(img, axis=1)
        if k % 5 == 3:
            img = (img // 64) * 64
        q = int(rng.integers(5, 101))
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=k % 3, restart_marker_rows=1)
        got = encode_jpeg(img[..., ::-1].copy(), quality=q, sampling=("444", "422", "420")[k % 3],
                          device=cuda)[0]
        assert got == buf.getvalue(), f"case {k}: {H}x{W} q{q} sampling {k % 3}"

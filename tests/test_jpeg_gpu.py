"""Baseline JPEG on the GPU: decode_jpeg, rv_jpeg_coef_to_bgr_u8 and the
MJPEG capture path give, bit for bit, the pixels Pillow (libjpeg-turbo)
decodes from the fixtures of tests/golden/jpeg (expected.npz, RGB)."""
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_jpeg_cpu import JDIR, STILLS, STREAMS, _data, _images, _named

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected():
    """name -> BGR pixels ((F, H, W, 3) for the streams); read once, never written."""
    z = np.load(os.path.join(GOLDEN, "jpeg", "expected.npz"))
    out = {k: np.ascontiguousarray(z[k][..., ::-1]) for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("name", STILLS + STREAMS)
def test_decode_jpeg_is_bit_exact(cuda, expected, name):
    from rvs_amd.io_video import decode_jpeg
    want = expected[name] if name.endswith(".mjpeg") else expected[name][None]
    for img, w in zip(_images(name), want):
        got = decode_jpeg(img, device=cuda)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == w.shape
        np.testing.assert_array_equal(got.cpu().numpy(), w)


def test_batch_of_records_with_different_quant_tables(cuda, expected):
    """S = 3 records of one size whose quant tables differ, in one launch,
    equal the three single decodes (and Pillow); then a batch whose records
    differ in sampling, and a record of another size, which is left alone."""
    from rvs_amd.io_video import jpeg_coefficients
    from rvs_amd.kernels import jpeg_to_bgr
    name = "40x56_420_5frames.mjpeg"
    imgs = [_images(name)[i] for i in (0, 2, 4)]
    recs = np.stack([jpeg_coefficients(i) for i in imgs])
    lay_q = {recs[i, 32:32 + 384].tobytes() for i in range(3)}
    assert len(lay_q) == 3
    dev = torch.from_numpy(recs).to(cuda)
    got = jpeg_to_bgr(dev, 56, 40)
    singles = torch.stack([jpeg_to_bgr(dev[i], 56, 40) for i in range(3)])
    assert torch.equal(got, singles)
    np.testing.assert_array_equal(got.cpu().numpy(), expected[name][[0, 2, 4]])
    # records of one size but different sampling (and lengths) in one batch
    names = [_named("48x64_444_"), _named("48x64_420_q"), _named("48x64_gray_"), _named("48x64_422_")]
    rs = [jpeg_coefficients(_data(n)) for n in names]
    stride = max(r.size for r in rs)
    batch = np.zeros((4, stride), np.uint8)
    for i, r in enumerate(rs):
        batch[i, :r.size] = r
    got = jpeg_to_bgr(torch.from_numpy(batch).to(cuda), 64, 48)
    for i, n in enumerate(names):
        np.testing.assert_array_equal(got[i].cpu().numpy(), expected[n])
    # a record that is not W x H is not decoded
    out = torch.full((1, 48, 64, 3), 7, dtype=torch.uint8, device=cuda)
    other = np.zeros(stride, np.uint8)
    r = jpeg_coefficients(_data(_named("16x16_420_")))
    other[:r.size] = r
    jpeg_to_bgr(torch.from_numpy(other[None]).to(cuda), 64, 48, out=out)
    assert bool((out == 7).all())


@pytest.mark.parametrize("name", STREAMS + ["37x91_420_q75_rst2.jpg"])
def test_video_source_reads_mjpeg(cuda, expected, name):
    from rvs_amd.io_video import VideoSource
    want = expected[name] if name.endswith(".mjpeg") else expected[name][None]
    for device in (False, True):
        src = VideoSource(os.path.join(JDIR, name), device=cuda)
        assert (src.height, src.width) == want.shape[1:3]
        for w in want:
            fr = src.read(device=device)
            assert fr.ok and fr.ts > 0
            img = fr.image.cpu().numpy() if device else fr.image
            assert isinstance(fr.image, torch.Tensor if device else np.ndarray)
            np.testing.assert_array_equal(img, w)
        assert not src.read().ok
        src.release()


@pytest.mark.parametrize("prefetch", [True, False])
def test_multistream_capture_over_mjpeg(cuda, expected, tmp_path, prefetch):
    """The uncompressed path's contract (tests/test_capture_gpu.py): frames in
    order, per-stream indices, read times that do not go back, None at the end;
    nbuf = 2 < 5 frames, so every ring wraps."""
    from rvs_amd.io_video import MultiStreamCapture
    name = "40x56_420_5frames.mjpeg"
    paths = []
    for s in range(3):
        p = tmp_path / f"cam{s}.mjpeg"
        shutil.copyfile(os.path.join(JDIR, name), p)
        paths.append(str(p))
    cap = MultiStreamCapture(paths, device=cuda, nbuf=2, prefetch=prefetch)
    assert (cap.S, cap.H, cap.W) == (3, 40, 56)
    last = np.zeros(3)
    for f in range(5):
        got = cap.next_batch()
        assert got is not None
        frames, ts, idx = got
        assert list(idx) == [f] * 3 and tuple(frames.shape) == (3, 40, 56, 3)
        host = frames.cpu().numpy()
        for s in range(3):
            np.testing.assert_array_equal(host[s], expected[name][f])
        t = ts.cpu().numpy()
        assert (t >= last).all()
        last = t
    assert cap.next_batch() is None and cap.next_batch() is None
    cap.close()


def test_engine_step_from_mjpeg_equals_step_from_tensor(cuda, expected, tmp_path):
    from rvs_amd.config import load_config
    from rvs_amd.engine import RoadVisionEngine
    from rvs_amd.io_video import MultiStreamCapture
    name = "40x56_420_5frames.mjpeg"
    paths = []
    for s in range(2):
        p = tmp_path / f"cam{s}.mjpeg"
        shutil.copyfile(os.path.join(JDIR, name), p)
        paths.append(str(p))
    cfg = load_config()
    cfg["detect"]["weights"] = "synthetic"
    outs = []
    for fed in ("mjpeg", "tensor"):
        eng = RoadVisionEngine(cfg, 2, (40, 56), device=cuda)
        ts = torch.zeros(2, dtype=torch.float64, device=cuda)
        if fed == "mjpeg":
            cap = MultiStreamCapture(paths, device=cuda)
            frames = cap.next_batch()[0]
        else:
            frames = torch.from_numpy(np.stack([expected[name][0]] * 2)).to(cuda)
        out = eng.step(frames, ts)
        res = eng.results(out)
        outs.append((out["proc"].cpu().numpy(),
                     [[(d.x1, d.y1, d.x2, d.y2, d.conf, d.cls_id, d.track_id) for d in r]
                      for r in res]))
        if fed == "mjpeg":
            cap.close()
        eng.close()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]


def test_random_sweep_against_pillow(cuda):
    """Wider than the fixtures, where Pillow is installed: random sizes (one to
    several kernel tiles), samplings, qualities, restart intervals."""
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    from rvs_amd.io_video import decode_jpeg
    rng = np.random.default_rng(2026)
    for k in range(24):
        H, W = int(rng.integers(1, 200)), int(rng.integers(1, 300))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if k % 2:
            img = np.sort(img, axis=1)
        kw = {"quality": int(rng.integers(5, 101))}
        if k % 4 == 3:
            kw["restart_marker_blocks"] = int(rng.integers(1, 9))
        if k % 5 == 4:
            kw["optimize"] = True
        buf = io.BytesIO()
        if k % 6 == 5:
            Image.fromarray(img[..., 0]).save(buf, "JPEG", **kw)
        else:
            Image.fromarray(img).save(buf, "JPEG", subsampling=k % 3, **kw)
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[..., ::-1]
        got = decode_jpeg(buf.getvalue(), device=cuda).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"case {k}: {H}x{W} {kw}")

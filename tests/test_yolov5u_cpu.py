"""YOLOv5u (variants 5..9) without a GPU: the native conv list against
tests/yolov5u_ref.py and the published totals, model-name resolution, the
checkpoint loader and its refusals, the k6 stem's integer digit block
(yolo_def.hip pack_conv0q6, the analogue of tests/test_conv0q.py), the fp8 /
synthetic-weight refusals in Python and through the C ABI, and the packed
blobs of the YOLOv8 variants, which this family must not move.
"""
import ctypes
import hashlib

import numpy as np
import pytest

import yolo_nc
import yolov5u_ref as v5

VARIANTS = (5, 6, 7, 8, 9)
NU_NC3_FLOATS = 2503513  # YOLOv5nu with 3 classes


@pytest.mark.parametrize("variant", VARIANTS)
def test_conv_list_counts_and_flat_sizes(variant):
    from rvs_amd import _lib
    from rvs_amd.detect.weights import conv_list
    lib = _lib.load()
    specs, _ = v5.conv_specs(variant)
    got = conv_list(variant)
    assert [g[0] for g in got] == [s[0] for s in specs]
    assert got == specs
    convs, floats, unfused = v5.TOTALS[variant]
    assert len(got) == convs == lib.rv_yolo_num_convs_nc(variant, 80) == lib.rv_yolo_num_convs(variant)
    assert sum(co * ci * k * k + co for _, ci, co, k, _, _ in got) == floats
    assert lib.rv_yolo_flat_floats_nc(variant, 80) == floats == lib.rv_yolo_flat_floats(variant)
    assert v5.unfused_total(variant) == unfused  # the helper's graph is the published one
    for nc in (1, 3, 70, 128):
        s_nc, _ = v5.conv_specs(variant, nc)
        assert conv_list(variant, nc) == s_nc, nc
        assert lib.rv_yolo_flat_floats_nc(variant, nc) == sum(co * ci * k * k + co
                                                              for _, ci, co, k, _, _ in s_nc)
    assert lib.rv_yolo_packed_bytes3(variant, 0, 80) > 0


def test_yolov5nu_with_three_classes():
    from rvs_amd import _lib
    from rvs_amd.detect.weights import conv_list
    assert len(conv_list(5, 3)) == 75
    assert _lib.load().rv_yolo_flat_floats_nc(5, 3) == NU_NC3_FLOATS


def test_variant_of():
    from rvs_amd.detect import weights
    assert weights.VARIANTS == {"n": 0, "s": 1, "m": 2, "l": 3, "x": 4}
    for i, k in enumerate("nsmlx"):
        for name in (f"yolov5{k}.pt", f"yolov5{k}u.pt", f"yolov5{k}", f"yolov5{k}u",
                     f"/data/ckpt/yolov5{k}u.pt", f"weights/YOLOv5{k}.PT", f"yolov5{k}u.safetensors"):
            assert weights.variant_of(name) == 5 + i, name
        assert weights.variant_of(f"yolov8{k}.pt") == i
    for name in ("yolov5n6u.pt", "yolov5n6.pt", "yolov5s6u", "yolo11n.pt", "yolov3u.pt",
                 "yolov5nu-seg.pt", "yolov5.pt", "yolov5nuu.pt", "rtdetr-l.pt"):
        with pytest.raises(ValueError, match=r"unsupported model.*YOLOv8.*YOLOv5u"):
            weights.variant_of(name)


def test_loader_folds_like_the_helper_and_reads_nc(tmp_path):
    from rvs_amd.detect.weights import (detector_weights, flat_from_state_dict, load_weights,
                                        nc_of_state_dict)
    for nc in (80, 3):
        base = yolo_flat(5, nc, seed=nc)
        unf = v5.state_dict(5, base, nc, fused=False, seed=3)
        want = v5.fold_state_dict(5, unf, nc)
        got, got_nc = flat_from_state_dict(unf, 5, return_nc=True)
        assert got_nc == nc == nc_of_state_dict(unf, 5)
        np.testing.assert_array_equal(got, want)
        nested_unf = {"model." + k: v for k, v in unf.items()}
        np.testing.assert_array_equal(flat_from_state_dict(nested_unf, 5), want)
        assert nc_of_state_dict(nested_unf, 5) == nc
        # the fused forms of the folded values give the same array
        for nested in (False, True):
            sd = v5.state_dict(5, want, nc, fused=True, nested=nested)
            np.testing.assert_array_equal(flat_from_state_dict(sd, 5), want)
        path = str(tmp_path / f"v5nu_{nc}.npz")
        np.savez(path, **unf)
        w, n = load_weights(path, 5, return_nc=True)
        assert n == nc
        np.testing.assert_array_equal(w, want)
        w, n = detector_weights({"model": "yolov5n.pt", "weights": path}, 5)
        assert n == nc
        other = 80 if nc != 80 else 3
        with pytest.raises(ValueError, match=rf"nc = {other}\b.*\b{nc} classes.*model\.24\.cv3\.0\.2"):
            load_weights(path, 5, nc=other)
    # the default of nc_of_state_dict is unchanged: it reads the YOLOv8 key
    with pytest.raises(KeyError, match=r"model\.22\.cv3\.0\.2\.weight"):
        nc_of_state_dict(unf)
    with pytest.raises(KeyError, match=r"model\.24\.cv3\.0\.2\.weight"):
        flat_from_state_dict({k: v for k, v in unf.items() if k != "model.24.cv3.0.2.weight"}, 5)
    # the wrong scale names the first tensor that does not fit
    with pytest.raises(ValueError, match=r"model\.0\.conv\.weight.*YOLOv5u"):
        flat_from_state_dict(unf, 6)


def yolo_flat(variant, nc, seed):
    rng = np.random.default_rng(seed)
    parts = []
    for n, ci, co, k, s, act in v5.conv_specs(variant, nc)[0]:
        parts += [rng.normal(0, 1 / np.sqrt(ci * k * k), co * ci * k * k), rng.normal(0, 0.05, co)]
    return np.concatenate(parts).astype(np.float32)


def test_loader_refusals():
    from rvs_amd.detect.weights import detector_weights, flat_from_state_dict
    sd5 = v5.state_dict(5, yolo_flat(5, 80, 1), fused=True)
    # an anchor-based checkpoint of the original yolov5 repository
    old = {k: v for k, v in sd5.items() if not k.startswith("model.24.")}
    old["model.24.anchors"] = np.zeros((3, 3, 2), np.float32)
    for i in range(3):
        old[f"model.24.m.{i}.weight"] = np.zeros((255, 64 << i, 1, 1), np.float32)
        old[f"model.24.m.{i}.bias"] = np.zeros(255, np.float32)
    for sd in (old, {"model." + k: v for k, v in old.items()}):
        with pytest.raises(ValueError, match=r"anchor-based YOLOv5.*'u' checkpoint"):
            flat_from_state_dict(sd, 5)
    # the other family than detect.model names, both ways
    with pytest.raises(ValueError, match=r"is a YOLOv5u one.*names a YOLOv8 model"):
        flat_from_state_dict(sd5, 0)
    flat8 = yolo_nc.random_flat(0, 80, seed=2)
    specs8, params8 = yolo_nc.split(0, 80, flat8)
    sd8 = {}
    for n, ci, co, k, s, act in specs8:
        sd8[n + (".conv.weight" if act else ".weight")] = params8[n][0]
        sd8[n + (".conv.bias" if act else ".bias")] = params8[n][1]
    with pytest.raises(ValueError, match=r"is a YOLOv8 one.*names a YOLOv5u model"):
        flat_from_state_dict(sd8, 5)
    np.testing.assert_array_equal(flat_from_state_dict(sd8, 0), flat8)
    # no shipped calibration: synthetic weights, asked for or by default
    for cfg in ({"model": "yolov5n.pt", "weights": "synthetic"}, {"model": "yolov5nu.pt"},
                {"model": "yolov5x.pt", "weights": None}):
        with pytest.raises(ValueError, match=r"YOLOv5u.*no shipped.*detect\.weights"):
            detector_weights(cfg, 5)


def test_fp8_and_synthetic_are_refused_in_python_and_in_the_abi():
    from rvs_amd import _lib
    from rvs_amd.detect.weights import pack, synthetic_weights
    from rvs_amd.detect.yolo_hip import YoloEngine
    lib = _lib.load()
    flat = yolo_flat(5, 80, 4)
    with pytest.raises(ValueError, match=r"fp8.*YOLOv5u.*bf16"):
        pack(5, flat, "fp8")
    with pytest.raises(ValueError, match=r"fp8.*YOLOv5u.*bf16"):
        YoloEngine(5, flat, 1, (64, 64), dtype="fp8", device="cpu")
    with pytest.raises(ValueError, match=r"YOLOv5u.*detect\.weights"):
        synthetic_weights(5)
    for variant in VARIANTS:
        out = np.full(64, 0xCD, np.uint8)
        assert lib.rv_yolo_pack3(variant, 1, 80, flat.ctypes.data, flat.size, out.ctypes.data,
                                 out.size) == -1000
        msg = lib.rv_last_error().decode()
        assert "YOLOv5u" in msg and "bf16 only" in msg and "fp8" in msg
        assert (out == 0xCD).all()
        assert lib.rv_yolo_packed_bytes3(variant, 1, 80) == 0
        assert lib.rv_yolo_packed_bytes3(variant, 0, 80) > 0
        h = ctypes.c_void_p()
        assert lib.rv_yolo_create3(variant, 1, 80, out.ctypes.data, 1, 64, 64, ctypes.byref(h)) == -1000
        assert "bf16 only" in lib.rv_last_error().decode() and not h
    for variant in (-1, 10):
        assert lib.rv_yolo_num_convs_nc(variant, 80) == -1000
        assert lib.rv_yolo_flat_floats_nc(variant, 80) == 0


def _k6_block(variant, flat):
    """The k6 digit block of a packed blob (it closes the blob, 256-B aligned)."""
    from rvs_amd.detect import weights
    blob = weights.pack(variant, flat, "bf16")
    c0 = v5.conv_specs(variant)[0][0][2]
    n = 9 * c0 * 64
    qb = n + 20 * c0
    start = blob.size - ((qb + 255) & ~255)
    blk = blob[start:start + qb]
    d = blk[:n].view(np.int8).reshape(3, c0, 192).astype(np.int64)
    s = blk[n:n + 4 * c0].view(np.float32)
    b = blk[n + 4 * c0:n + 8 * c0].view(np.float32)
    c = blk[n + 8 * c0:n + 20 * c0].view(np.int32).reshape(3, c0)
    w = flat[:c0 * 108].reshape(c0, 3, 6, 6).astype(np.float64)
    return c0, d, s, b, c, w, flat[c0 * 108:c0 * 109], blob[:c0 * 108 * 4].view(np.float32)


@pytest.mark.parametrize("variant", (5, 9, 7))
def test_k6_digit_block(variant):
    """Digits reconstruct round(V / s) at 2^-23 of the channel maximum; every
    unused K slot is zero; accumulator starts are 128 sum D; on random and
    all-255 windows the per-digit sums are exact and below 2^24; the kernel's
    f32 combine equals the f64 conv to the bound of tests/test_conv0q.py
    (2^-21 of the output scale)."""
    rng = np.random.default_rng(variant)
    c0 = v5.conv_specs(variant)[0][0][2]
    n0 = c0 * 108
    flat = yolo_flat(variant, 80, seed=variant) if variant == 5 else np.concatenate(
        [rng.normal(0, 0.1, n0), rng.normal(0, 0.5, c0),
         np.zeros(v5.TOTALS[variant][1] - n0 - c0)]).astype(np.float32)
    c0, d, s, b, c, w, b_ref, w0 = _k6_block(variant, flat)
    np.testing.assert_array_equal(b, b_ref)
    np.testing.assert_array_equal(w0, flat[:n0])  # conv 0's f32 OIHW copy opens the blob
    assert (d >= -128).all() and (d <= 127).all()
    Q = d[0] * 65536 + d[1] * 256 + d[2]
    V = np.zeros((c0, 192))
    used = np.zeros(192, bool)
    for ky in range(6):
        for kx in range(6):
            for ch in range(3):
                k = 64 * (ky // 2) + 32 * (ky & 1) + 3 * kx + ch
                assert not used[k]
                used[k] = True
                V[:, k] = w[:, 2 - ch, ky, kx] / 255.0
    assert used.sum() == 108
    assert not d[:, :, ~used].any()
    np.testing.assert_array_equal(c, 128 * d.sum(2))
    M = np.abs(V).max(1)
    assert (M > 0).all()
    sd = s.astype(np.float64)
    np.testing.assert_array_equal(Q, np.rint(V / sd[:, None]).astype(np.int64))
    assert (np.abs(Q * sd[:, None] - V) <= (M * 2.0 ** -23)[:, None]).all()
    # windows: random (some all-zero: the padding), all 255; the unused slots
    # hold garbage (bytes of the neighbouring pixels, or zeros out of range)
    x = rng.integers(0, 256, size=(4096, 192)).astype(np.int64)
    x[:64][:, used] = 0
    x[64:128] = 255
    T = []
    for i in range(3):
        acc = c[i][None, :] + (x - 128) @ d[i].T  # the MFMA chain: start + sum D (x - 128)
        np.testing.assert_array_equal(acc, x @ d[i].T)
        assert np.abs(acc).max() < 2 ** 24
        T.append(acc)
    t12 = T[1] * 256 + T[2]
    assert np.abs(t12).max() < 2 ** 31
    u = (T[0].astype(np.float32).astype(np.float64) * 65536 +
         t12.astype(np.float32).astype(np.float64)).astype(np.float32)
    got = (s[None, :].astype(np.float64) * u.astype(np.float64)).astype(np.float64) + b[None, :]
    got = got.astype(np.float32).astype(np.float64)  # one fma: a single rounding
    ref = x @ V.T + b.astype(np.float64)
    scale = np.abs(V).sum(1) * 255 + np.abs(b)
    assert (np.abs(got - ref) <= scale * 2.0 ** -21).all()


# sha256 of weights.pack(v, flat, dtype) from a build of the parent commit of
# the YOLOv5u change (flat as in _v8_flat)
PARENT_PACKED_SHA256 = {
    (0, "bf16"): "15ed6ed03a61e5d76343cd577570f32cf512c2b5a605af3f4e3798d2d0ee5f43",
    (0, "fp8"): "e4b5d83fe7518829349a51ce6fa8e9f40cbda65ee31472f8e0d51dcc70bb1830",
    (1, "bf16"): "aefcff32beeebfa1f3c2ef09f32a02b8041f7a65e25771dac0d19094bab97493",
    (1, "fp8"): "e619f7ae13c11890aa6c841ca8badfa3c3e5db65d6003a596d3e23fc7879f440",
    (2, "bf16"): "a655182c4474feeac6da23e48542a57d7c24a892bbc4899b2c9d8765460c3470",
    (2, "fp8"): "fe654bf1fb6cfc304261835204a3c38b1c89c3f64b3408644d3a1b662e7cf597",
    (3, "bf16"): "964641d11451f31ad47177de363d8f4e0fe2d637596766320a55c3774cc9c4bb",
    (3, "fp8"): "a15efb8efe2c7b508d737601f271b180220bcb78c1e3d52f35077715a5dc916a",
    (4, "bf16"): "d42815ee8d6c6c5768eeef9148c4eec4da24bd3876c24e4cf202ba2403702fbb",
    (4, "fp8"): "843ae06d566b0de5e337284145a2cea4d984f3ec2371d8a8f4a40191f29a76b6",
}


def _v8_flat(variant):
    from rvs_amd.detect import weights
    if variant in (0, 2):  # the variants that ship calibration
        return weights.synthetic_weights(variant, seed=11)
    return yolo_nc.random_flat(variant, 80, seed=11)


@pytest.mark.parametrize("variant", (0, 1, 2, 3, 4))
def test_yolov8_packed_blobs_are_unchanged(variant):
    """The packed blobs of variants 0..4, bf16 and fp8, are byte for byte what
    the parent commit packed: PARENT_PACKED_SHA256 was recorded from a build
    of the parent commit with the same flat arrays (synthetic_weights(v,
    seed=11) for n and m, which ship calibration; yolo_nc.random_flat(v, 80,
    seed=11) for s, l and x)."""
    from rvs_amd.detect import weights
    flat = _v8_flat(variant)
    for dtype in ("bf16", "fp8"):
        blob = weights.pack(variant, flat, dtype)
        assert hashlib.sha256(blob.tobytes()).hexdigest() == PARENT_PACKED_SHA256[(variant, dtype)]

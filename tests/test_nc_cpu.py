"""YOLOv8 plans with a custom class count (nc 1..128): everything that needs
no GPU -- the native conv list against the Ultralytics width rule, the packer,
the range / fp8 refusals, checkpoint loading with the class count read from
the state_dict, and the class-name handling.
"""
import ctypes

import numpy as np
import pytest
import torch

import yolo_nc

VARIANTS = (0, 1, 4)  # n, s, x
NCS = (1, 4, 17, 64, 65, 70, 80, 100, 128)


@pytest.mark.parametrize("variant", VARIANTS)
def test_conv_list_follows_the_width_rule(variant):
    from rvs_amd import _lib
    from rvs_amd.detect.weights import conv_list
    lib = _lib.load()
    assert lib.rv_abi_version() >= 8
    for nc in NCS:
        specs, _ = yolo_nc.conv_specs(variant, nc)
        got = conv_list(variant, nc)
        assert got == specs, (variant, nc)
        c3d = yolo_nc.c3d_of(variant, nc)
        cls = {n: (ci, co) for n, ci, co, *_ in got if n.startswith("model.22.cv3.")}
        for i in range(3):
            assert cls[f"model.22.cv3.{i}.0"][1] == c3d
            assert cls[f"model.22.cv3.{i}.1"] == (c3d, c3d)
            assert cls[f"model.22.cv3.{i}.2"] == (c3d, nc)
        floats = sum(co * ci * k * k + co for _, ci, co, k, _, _ in specs)
        assert lib.rv_yolo_flat_floats_nc(variant, nc) == floats
        assert lib.rv_yolo_num_convs_nc(variant, nc) == len(specs)
    assert conv_list(variant, 80) == conv_list(variant)
    assert lib.rv_yolo_flat_floats_nc(variant, 80) == lib.rv_yolo_flat_floats(variant)


@pytest.mark.parametrize("variant", (0, 2))
def test_default_packing_unchanged(variant):
    """pack() without nc, with nc = 80, and the pre-nc entry rv_yolo_pack2:
    the same bytes."""
    from rvs_amd import _lib
    from rvs_amd.detect.weights import pack, synthetic_weights
    flat = synthetic_weights(variant, seed=3)
    a, b = pack(variant, flat), pack(variant, flat, nc=80)
    assert a.tobytes() == b.tobytes()
    lib = _lib.load()
    assert lib.rv_yolo_packed_bytes3(variant, 0, 80) == lib.rv_yolo_packed_bytes2(variant, 0) == a.size
    old = np.full(a.size, 0xAB, np.uint8)
    assert lib.rv_yolo_pack2(variant, 0, flat.ctypes.data, flat.size, old.ctypes.data, old.size) == 0
    assert old.tobytes() == a.tobytes()


def test_packed_padding_is_zero():
    """nc = 70 (YOLOv8n: c3d = 70, run 72 wide): the packed rows / columns the
    padded launches read beyond the state_dict shapes are zero, and the real
    ones hold the bf16 weights."""
    from rvs_amd.detect.weights import conv_list, pack
    nc = 70
    flat = yolo_nc.random_flat(0, nc, seed=5)
    packed = pack(0, flat, nc=nc)
    specs, params = yolo_nc.split(0, nc, flat)
    assert conv_list(0, nc) == specs
    # walk the packed layout (include/rvhip.h: conv 0 f32 OIHW; then bf16
    # [Cout16][k][k][Cin32] + f32 bias [Cout16], every block 256-byte aligned)
    al = lambda x: (x + 255) & ~255  # noqa: E731
    off = 0
    for i, (n, ci, co, k, s, act) in enumerate(specs):
        cop, cip = (co + 15) & ~15, (ci + 31) & ~31
        wb = co * ci * k * k * 4 if i == 0 else cop * k * k * cip * 2
        if i and n.startswith("model.22.cv3."):
            w = packed[off:off + wb].view(np.uint16).reshape(cop, k, k, cip)
            assert not w[co:].any() and not w[:, :, :, ci:].any(), n
            want = torch.from_numpy(params[n][0]).to(torch.bfloat16).view(torch.int16).numpy()
            np.testing.assert_array_equal(w[:co, :, :, :ci].view(np.int16), want.transpose(0, 2, 3, 1))
        off = al(off + wb)
        bias = packed[off:off + cop * 4].view(np.float32)
        if i:
            np.testing.assert_array_equal(bias[:co], params[n][1])
            assert not bias[co:].any(), n
        off = al(off + cop * 4)
    assert off <= packed.size


@pytest.mark.parametrize("nc", (0, 129, -3))
def test_class_count_range(nc):
    from rvs_amd import _lib
    from rvs_amd._lib import RVError
    from rvs_amd.detect.weights import conv_list, pack
    from rvs_amd.detect.yolo_hip import YoloEngine
    lib = _lib.load()
    with pytest.raises(RVError, match=r"outside the supported range 1\.\.128"):
        conv_list(0, nc)
    flat = np.zeros(16, np.float32)
    with pytest.raises(RVError, match=r"outside the supported range 1\.\.128"):
        pack(0, flat, nc=nc)
    assert lib.rv_yolo_num_convs_nc(0, nc) == -1000
    assert lib.rv_yolo_flat_floats_nc(0, nc) == 0 and lib.rv_yolo_packed_bytes3(0, 0, nc) == 0
    info = (ctypes.c_int * 5)(*([-7] * 5))
    name = ctypes.create_string_buffer(b"untouched", 32)
    assert lib.rv_yolo_conv_info_nc(0, nc, 0, info, name, 32) == -1000
    assert b"1..128" in lib.rv_last_error()
    assert list(info) == [-7] * 5 and name.value == b"untouched"
    out = np.full(64, 0xCD, np.uint8)
    assert lib.rv_yolo_pack3(0, 0, nc, flat.ctypes.data, flat.size, out.ctypes.data, out.size) == -1000
    assert (out == 0xCD).all()
    # rv_yolo_create3 checks the class count before any device call
    h = ctypes.c_void_p()
    assert lib.rv_yolo_create3(0, 0, nc, out.ctypes.data, 1, 64, 64, ctypes.byref(h)) == -1000
    assert b"1..128" in lib.rv_last_error() and not h
    with pytest.raises(ValueError, match=r"1\.\.128"):
        YoloEngine(0, flat, 1, (64, 64), nc=nc, device="cpu")


def test_fp8_and_synthetic_refusals():
    from rvs_amd import _lib
    from rvs_amd.detect.weights import pack, synthetic_weights
    from rvs_amd.detect.yolo_hip import YoloEngine
    lib = _lib.load()
    flat = yolo_nc.random_flat(0, 4)
    with pytest.raises(ValueError, match="fp8.*nc = 80 only.*nc = 4"):
        pack(0, flat, "fp8", nc=4)
    out = np.full(64, 0xCD, np.uint8)
    assert lib.rv_yolo_pack3(0, 1, 4, flat.ctypes.data, flat.size, out.ctypes.data, out.size) == -1000
    assert b"fp8" in lib.rv_last_error() and b"nc = 80 only" in lib.rv_last_error()
    assert (out == 0xCD).all() and lib.rv_yolo_packed_bytes3(0, 1, 4) == 0
    assert lib.rv_yolo_packed_bytes3(0, 1, 80) == lib.rv_yolo_packed_bytes2(0, 1) > 0
    # Python refuses before any native call: no device is needed to get here
    with pytest.raises(ValueError, match="fp8.*nc = 80 only"):
        YoloEngine(0, flat, 1, (64, 64), dtype="fp8", nc=4, device="cpu")
    with pytest.raises(ValueError, match=r"nc = 4.*80-class.*detect\.weights"):
        synthetic_weights(0, nc=4)
    assert synthetic_weights(0, 1, nc=80).tobytes() == synthetic_weights(0, 1).tobytes()


def _state_dicts(nc, seed):
    """(flat of the fused values, {kind: state_dict}) for YOLOv8n with nc
    classes: fused keys (conv.weight + conv.bias) and unfused ones (conv.weight
    + bn.*, un-folded from the same values), each also under the "model."
    nesting of YOLO(...).state_dict()."""
    flat = yolo_nc.random_flat(0, nc, seed)
    specs, params = yolo_nc.split(0, nc, flat)
    rng = np.random.default_rng(seed + 1)
    fused, unfused = {}, {}
    for n, ci, co, k, s, act in specs:
        w, b = params[n]
        if not act:  # Detect's plain nn.Conv2d
            for sd in (fused, unfused):
                sd[n + ".weight"], sd[n + ".bias"] = w.copy(), b.copy()
            continue
        fused[n + ".conv.weight"], fused[n + ".conv.bias"] = w.copy(), b.copy()
        gamma = rng.uniform(0.5, 1.5, co).astype(np.float32)
        var = rng.uniform(0.5, 2.0, co).astype(np.float32)
        mean = rng.normal(0, 0.1, co).astype(np.float32)
        sd_ = np.sqrt(var + np.float32(1e-3))
        scale = gamma / sd_
        unfused[n + ".conv.weight"] = (w / scale[:, None, None, None]).astype(np.float32)
        unfused[n + ".bn.weight"] = gamma
        unfused[n + ".bn.bias"] = (b + gamma * mean / sd_).astype(np.float32)
        unfused[n + ".bn.running_mean"] = mean
        unfused[n + ".bn.running_var"] = var
        unfused[n + ".bn.num_batches_tracked"] = np.array(7, np.int64)
    for sd in (fused, unfused):
        sd["model.22.dfl.conv.weight"] = np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)
    nest = lambda sd: {"model." + k: v for k, v in sd.items()}  # noqa: E731
    return flat, {"fused": fused, "unfused": unfused, "fused-nested": nest(fused),
                  "unfused-nested": nest(unfused)}


@pytest.mark.parametrize("nc", (4, 70))
def test_checkpoint_loading_infers_the_class_count(tmp_path, nc):
    from rvs_amd.detect.weights import (detector_weights, flat_from_state_dict, load_weights,
                                        nc_of_state_dict, pack)
    flat, sds = _state_dicts(nc, seed=nc)
    for kind, sd in sds.items():
        path = str(tmp_path / f"{kind}.npz")
        np.savez(path, **sd)
        assert nc_of_state_dict(sd) == nc
        got, got_nc = load_weights(path, 0, return_nc=True)
        assert got_nc == nc and got.dtype == np.float32 and got.shape == flat.shape, kind
        if kind.startswith("fused"):
            np.testing.assert_array_equal(got, flat, err_msg=kind)
        else:  # folded back in f32: the un-fold / fold round trip costs a few ulp
            np.testing.assert_allclose(got, flat, rtol=2e-6, atol=1e-7, err_msg=kind)
        # without return_nc: the flat array alone, as before
        np.testing.assert_array_equal(load_weights(path, 0), got)
        # the config path: nc comes from the checkpoint; a matching detect.nc passes
        for cfg in ({"weights": path}, {"weights": path, "nc": nc}):
            w, n = detector_weights(cfg, 0)
            assert n == nc
            np.testing.assert_array_equal(w, got)
        assert pack(0, got, nc=nc).size > 0
        other = 80 if nc != 80 else 4
        with pytest.raises(ValueError, match=rf"nc = {other}\b.*\b{nc} classes"):
            load_weights(path, 0, nc=other)
        with pytest.raises(ValueError, match=rf"nc = {other}\b.*\b{nc} classes"):
            detector_weights({"weights": path, "nc": other}, 0)
    # a class-branch tensor that does not fit the variant / nc: named, no numpy reshape error
    for kind in ("fused", "unfused-nested"):
        bad = dict(sds[kind])
        pre = "model." if kind.endswith("nested") else ""
        key = pre + "model.22.cv3.1.1.conv.weight"
        bad[key] = bad[key][:, :-1]
        with pytest.raises((KeyError, ValueError), match=r"model\.22\.cv3\.1\.1") as ei:
            flat_from_state_dict(bad, 0)
        assert "reshape" not in str(ei.value)
    # the wrong variant for the checkpoint names the first tensor that does not fit
    with pytest.raises(ValueError, match=r"model\.0\.conv\.weight"):
        flat_from_state_dict(sds["fused"], 1)
    missing = {k: v for k, v in sds["fused"].items() if k != "model.22.cv3.0.2.weight"}
    with pytest.raises(KeyError, match=r"model\.22\.cv3\.0\.2\.weight"):
        flat_from_state_dict(missing, 0)


def test_names():
    from rvs_amd.detect.weights import COCO80, names_from_config
    from rvs_amd.detect.yolo_hip import YoloEngine
    assert names_from_config({}, 80) == list(COCO80)
    assert names_from_config({}, 4) == []
    assert names_from_config({"names": ["car", "truck", "bus", "person"]}, 4) == \
        ["car", "truck", "bus", "person"]
    assert names_from_config({"names": ["car", "truck"]}, 4) == ["car", "truck"]
    assert names_from_config({"names": {0: "car", "2": "bus"}}, 4) == ["car", "1", "bus"]
    with pytest.raises(ValueError, match="5 names.*4 classes"):
        names_from_config({"names": ["a", "b", "c", "d", "e"]}, 4)
    with pytest.raises(ValueError, match="class id 4.*4 classes"):
        names_from_config({"names": {4: "e"}}, 4)
    # Detection.cls_name: the name when there is one, else str(id)
    dets = torch.tensor([[[1, 2, 3, 4, 0.9, 0], [1, 2, 3, 4, 0.8, 3], [0, 0, 0, 0, 0, 1]]],
                        dtype=torch.float32)
    n = torch.tensor([2], dtype=torch.int32)
    for names, want in ((names_from_config({"names": {0: "car", 3: "person"}}, 4), ["car", "person"]),
                        (names_from_config({"names": ["car"]}, 4), ["car", "3"]),
                        (names_from_config({}, 4), ["0", "3"]),
                        (names_from_config({}, 80), ["person", "motorcycle"])):
        out = YoloEngine.to_detections(dets, n, names)
        assert [d.cls_name for d in out[0]] == want and [d.cls_id for d in out[0]] == [0, 3]

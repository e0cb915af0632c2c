"""YOLOv8, YOLOv5u and YOLO11 weights for the HIP detector.

The conv list (names, shapes, order) comes from the native plan in
csrc/yolo_def.hip (rv_yolo_conv_info) -- Ultralytics state_dict order with BN
fused.  Real checkpoints are not available in this environment
(.MISSING_LARGE_BLOBS:1 lists yolov8n.pt; there is no network), so weights are
either loaded from a local Ultralytics state_dict (load_weights: .safetensors,
.npz, or a tensors-only torch file read with weights_only=True -- never a
pickle), or generated synthetically from a seed.

load_weights accepts the Ultralytics DetectionModel state_dict keys as they
are before and after ``model.fuse()`` (the reference calls it,
src/detect/yolo_ultralytics.py:16-17):
  * unfused Conv blocks: ``model.N[...].conv.weight`` + ``.bn.weight / .bn.bias
    / .bn.running_mean / .bn.running_var`` -- folded here exactly as
    ultralytics.utils.torch_utils.fuse_conv_and_bn does (BatchNorm2d eps =
    1e-3, set by initialize_weights), in float32;
  * fused Conv blocks: ``model.N[...].conv.weight`` + ``.conv.bias``;
  * the Detect head's plain 1x1 convs: ``model.22.cv2.i.2.weight / .bias``;
  * the plan's own names (``model.2.m.0.cv1.weight / .bias``, round-1 files).
The DFL conv (``model.22.dfl.conv.weight``, a fixed arange) and
``num_batches_tracked`` are ignored.

The class count is the checkpoint's own (the first dimension of
``model.22.cv3.0.2.weight``, 1..128), as the reference's YOLO(cfg["model"])
takes it from the checkpoint; ``detect.nc`` may state it and must then agree,
``detect.names`` names the classes (names_from_config).  Synthetic weights
exist for 80 classes only.

YOLOv5u (``yolov5n.pt`` ... ``yolov5xu.pt``: Ultralytics resolves the plain
YOLOv5 names to the anchor-free "u" re-release, yolov5.yaml under the YOLOv8
Detect head) is variants 5..9.  Its Detect module is ``model.24``, so the
class count is read from ``model.24.cv3.0.2.weight``.  There is no shipped
calibration and no fp8 plan for it: it needs a ``detect.weights`` file and
runs in bf16.  An anchor-based checkpoint of the original yolov5 repository
(``model.24.m.*`` / ``model.24.anchors``) is a different network and refused.

YOLO11 (``yolo11n.pt`` ... ``yolo11x.pt``, yolo11.yaml: C3k2 / C2PSA, Detect
at ``model.23``) is variants 20..24 (resolve_model; variant_of keeps to the two
conv-only families).  Its depthwise convs (``DWConv``: the Detect class
branch's ``cv3.i.j.0`` and the attention's ``attn.pe``) are Conv blocks with a
``[C, 1, 3, 3]`` weight, fused or unfused like the others (conv_groups).  As
for YOLOv5u there is no shipped calibration and no fp8 plan.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, Tuple

import numpy as np

from .. import _lib

VARIANTS = {"n": 0, "s": 1, "m": 2, "l": 3, "x": 4}
COCO80 = [
    "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat",
    "traffic light", "fire hydrant", "stop sign", "parking meter", "bench", "bird", "cat", "dog",
    "horse", "sheep", "cow", "elephant", "bear", "zebra", "giraffe", "backpack", "umbrella",
    "handbag", "tie", "suitcase", "frisbee", "skis", "snowboard", "sports ball", "kite",
    "baseball bat", "baseball glove", "skateboard", "surfboard", "tennis racket", "bottle",
    "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple", "sandwich", "orange",
    "broccoli", "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch", "potted plant",
    "bed", "dining table", "toilet", "tv", "laptop", "mouse", "remote", "keyboard", "cell phone",
    "microwave", "oven", "toaster", "sink", "refrigerator", "book", "clock", "vase", "scissors",
    "teddy bear", "hair drier", "toothbrush"]


V5U_VARIANTS = {"n": 5, "s": 6, "m": 7, "l": 8, "x": 9}  # YOLOv5u (include/rvhip.h)
_V5U_NAME = re.compile(r"yolov5([nsmlx])u?(\.[a-z0-9]+)?$")


def variant_of(model_name: str) -> int:
    """'yolov8n.pt' -> 0 ..., 'yolov5n.pt' / 'yolov5nu.pt' -> 5 ... (the
    reference's cfg['model'], default.yaml:39; Ultralytics resolves the plain
    YOLOv5 names to the "u" checkpoints).  The P6 models (yolov5n6u.pt) and
    every other family raise."""
    base = os.path.basename(str(model_name)).lower()
    for k, v in VARIANTS.items():
        if base.startswith(f"yolov8{k}"):
            return v
    m = _V5U_NAME.match(base)
    if m:
        return V5U_VARIANTS[m.group(1)]
    raise ValueError(f"unsupported model '{model_name}' (YOLOv8 n/s/m/l/x and YOLOv5u "
                     "n/s/m/l/x -- yolov5n.pt / yolov5nu.pt ... -- only)")


V11_VARIANTS = {"n": 20, "s": 21, "m": 22, "l": 23, "x": 24}  # YOLO11 (include/rvhip.h)
_V11_NAME = re.compile(r"yolo11([nsmlx])(\.[a-z0-9]+)?$")


def resolve_model(model_name: str) -> int:
    """The plan variant of the reference's cfg['model']: 'yolo11n.pt' /
    'yolo11n' / 'weights/YOLO11N.pt' -> 20 ... 'yolo11x.pt' -> 24; every other
    name as variant_of (YOLOv8 0..4, YOLOv5u 5..9).  The YOLO11 task models
    (yolo11n-seg.pt, -cls, -pose, -obb) and other families raise."""
    m = _V11_NAME.match(os.path.basename(str(model_name)).lower())
    if m:
        return V11_VARIANTS[m.group(1)]
    try:
        return variant_of(model_name)
    except ValueError as e:
        raise ValueError(f"{e}; YOLO11 detection models are yolo11n.pt ... yolo11x.pt") from None


def is_v5u(variant: int) -> bool:
    return 5 <= int(variant) < 10


def is_v11(variant: int) -> bool:
    return int(variant) >= 20


def family_name(variant: int) -> str:
    return "YOLO11" if is_v11(variant) else ("YOLOv5u" if is_v5u(variant) else "YOLOv8")


def head_prefix(variant: int) -> str:
    """State_dict prefix of the Detect module: layer 22 of yolov8.yaml, 24 of
    yolov5.yaml, 23 of yolo11.yaml."""
    return "model.23." if is_v11(variant) else ("model.24." if is_v5u(variant) else "model.22.")


NC_MIN, NC_MAX = 1, 128  # class counts the native plan supports (include/rvhip.h)
CLS_KEY = "model.22.cv3.0.2.weight"  # its first dimension is the checkpoint's class count


def cls_key(variant: int = None) -> str:
    """CLS_KEY of the variant's family (YOLOv8 without a variant)."""
    return CLS_KEY if variant is None else head_prefix(variant) + "cv3.0.2.weight"


def conv_list(variant: int, nc: int = 80) -> List[Tuple[str, int, int, int, int, int]]:
    """[(name, cin, cout, k, stride, silu)] in packing order: the Ultralytics
    state_dict shapes of a YOLOv8 / YOLOv5u with `nc` classes."""
    lib = _lib.load()
    out = []
    info = (ctypes.c_int * 5)()
    name = ctypes.create_string_buffer(96)
    n = lib.rv_yolo_num_convs_nc(variant, int(nc))
    if n < 0:
        _lib.check(n, "rv_yolo_num_convs_nc")
    for i in range(n):
        _lib.check(lib.rv_yolo_conv_info_nc(variant, int(nc), i, info, name, 96),
                   "rv_yolo_conv_info_nc")
        out.append((name.value.decode(), info[0], info[1], info[2], info[3], info[4]))
    return out


def conv_groups(variant: int, nc: int = 80) -> List[int]:
    """Per conv of conv_list(variant, nc): 1 for a dense conv, the channel
    count for a depthwise one (its state_dict weight is [C, 1, k, k])."""
    lib = _lib.load()
    n = lib.rv_yolo_num_convs_nc(variant, int(nc))
    if n < 0:
        _lib.check(n, "rv_yolo_num_convs_nc")
    out = []
    for i in range(n):
        g = lib.rv_yolo_conv_groups(variant, int(nc), i)
        if g < 0:
            _lib.check(g, "rv_yolo_conv_groups")
        out.append(g)
    return out


_CALIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "synthetic_calib.npz")


SMOOTH_KERNEL = "delta"  # spatial profile of the coherent part: "delta" (centre tap) or "blur"


def base_weights(rng, seed: int, idx: int, cin: int, cout: int, k: int, smooth: float):
    """Base (pre-calibration) weights and bias of conv `idx`: unit-fan-in
    He-normal weights (drawn from `rng`, the same stream for every `smooth`),
    mixed with weight `smooth` in [0, 1) of a channel-coherent part -- per
    output channel a signed gain times one positive per-input-channel profile
    on the centre tap (SMOOTH_KERNEL), rows scaled to the same norm as the
    random part.  Trained conv filters are spatially smooth and
    their inputs redundant, so noise added to an activation (quantisation,
    accumulation order) is averaged down layer by layer; pure random weights
    pass it on at full strength (the chaotic regime)."""
    w = rng.normal(0, 1 / np.sqrt(cin * k * k), size=(cout, cin, k, k)).astype(np.float32)
    b = rng.normal(0, 0.05, size=(cout,)).astype(np.float32)
    if smooth > 0:
        srng = np.random.default_rng([seed, 7919, idx])
        g = np.zeros((k, k))
        if SMOOTH_KERNEL == "blur" and k == 3:
            g1 = np.array([1.0, 2.0, 1.0])
            g = np.outer(g1, g1)
        else:
            g[k // 2, k // 2] = 1.0
        u = srng.uniform(0.5, 1.5, cin)
        a = srng.choice([-1.0, 1.0], cout) * srng.uniform(0.5, 1.5, cout)
        st = a[:, None, None, None] * u[None, :, None, None] * g[None, None]
        st /= np.sqrt((st ** 2).sum(axis=(1, 2, 3), keepdims=True))
        w = (np.sqrt(1 - smooth) * w + np.sqrt(smooth) * st).astype(np.float32)
    return w, b


def synthetic_weights(variant: int, seed: int = 0, nc: int = 80) -> np.ndarray:
    """Seeded BN-fused-like weights as one flat f32 array (80 classes only:
    the shipped calibration is the 80-class one).

    Base weights (base_weights: He-normal, for some variants mixed with a
    smooth part, data/synthetic_calib.npz "<variant>/smooth"), then the
    per-channel scale/shift stored in data/synthetic_calib.npz (w' =
    w*scale, b' = b*scale + shift; produced offline by
    tests/golden/make_yolo_scales.py), so every conv's pre-activation is O(1)
    like a trained model's fused BN output and a road frame yields a few
    hundred NMS candidates."""
    if is_v5u(variant):
        raise ValueError(f"no synthetic calibration for YOLOv5u (variant {variant}) in "
                         f"{os.path.basename(_CALIB)}: a YOLOv5u model needs a detect.weights "
                         "file (a local state_dict of the 'u' checkpoint)")
    if is_v11(variant):
        raise ValueError(f"no synthetic calibration for YOLO11 (variant {variant}) in "
                         f"{os.path.basename(_CALIB)}: a YOLO11 model needs a detect.weights "
                         "file (a local state_dict of the checkpoint)")
    if int(nc) != 80:
        raise ValueError(f"no synthetic calibration for nc = {nc} in {os.path.basename(_CALIB)} "
                         "(the shipped calibration is 80-class); a model with a custom class "
                         "count needs a detect.weights file (a local state_dict)")
    rng = np.random.default_rng(seed)
    parts = []
    with np.load(_CALIB, allow_pickle=False) as cal:
        have = sorted({k.split("/")[0] for k in cal.files})
        if str(variant) not in have:
            raise ValueError(f"no synthetic calibration for YOLOv8 variant {variant} in "
                             f"{os.path.basename(_CALIB)} (it has variants {', '.join(have)}); "
                             f"tests/golden/make_yolo_scales.py {variant} produces the arrays")
        smooth = float(cal[f"{variant}/smooth"]) if f"{variant}/smooth" in cal.files else 0.0
        for i, (name, cin, cout, k, s, act) in enumerate(conv_list(variant)):
            w, b = base_weights(rng, seed, i, cin, cout, k, smooth)
            sc = cal[f"{variant}/{name}/scale"].astype(np.float32)
            sh = cal[f"{variant}/{name}/shift"].astype(np.float32)
            parts += [(w * sc[:, None, None, None]).ravel(), b * sc + sh]
    return np.concatenate(parts).astype(np.float32)


BN_EPS = 1e-3  # ultralytics.nn.tasks.initialize_weights: BatchNorm2d.eps = 1e-3


def fold_bn(w: np.ndarray, gamma: np.ndarray, beta: np.ndarray, mean: np.ndarray,
            var: np.ndarray, bias=None, eps: float = BN_EPS):
    """ultralytics.utils.torch_utils.fuse_conv_and_bn in float32 torch ops:
    w_bn = diag(gamma / sqrt(eps + var)); W = w_bn @ w; b = w_bn @ b_conv +
    (beta - gamma * mean / sqrt(var + eps)).  torch's own sqrt / div / mul
    are used (torch's CPU sqrt is not always the correctly rounded one, and
    the reference folds with it); the diagonal matmuls are evaluated as the
    exact per-row products they denote (a BLAS sgemm of a diagonal matrix
    returns some of them 1 ulp off, platform-dependently)."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
    w, gamma, beta, mean, var = t(w), t(gamma), t(beta), t(mean), t(var)
    scale = gamma.div(torch.sqrt(eps + var))
    wf = scale.view(-1, *([1] * (w.dim() - 1))) * w
    b_conv = torch.zeros_like(beta) if bias is None else t(bias)
    b_bn = beta - gamma.mul(mean).div(torch.sqrt(var + eps))
    return wf.numpy(), (scale * b_conv + b_bn).numpy()


def read_state_dict(path: str) -> Dict[str, np.ndarray]:
    """Tensors of a local checkpoint, with loaders that execute nothing
    from the file: .safetensors, .npz (allow_pickle=False), or a torch file
    of plain tensors (torch.load(weights_only=True))."""
    if path.endswith(".safetensors"):
        from safetensors.numpy import load_file
        return dict(load_file(path))
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    import torch
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state_dict of tensors (save model.state_dict())")
    return {k: v.detach().float().numpy() if hasattr(v, "detach") else np.asarray(v)
            for k, v in sd.items()}


def _strip_prefix(t: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    # YOLO(...).state_dict() nests the DetectionModel under "model."
    if any(k.startswith("model.model.") for k in t):
        t = {k[len("model."):]: v for k, v in t.items() if k.startswith("model.")}
    return t


def nc_of_state_dict(tensors: Dict[str, np.ndarray], variant: int = None) -> int:
    """The class count of an Ultralytics DetectionModel state_dict: the first
    dimension of model.22.cv3.0.2.weight (a plain nn.Conv2d, so the key is the
    same before and after model.fuse(), with or without the "model." nesting);
    with a YOLOv5u `variant`, of model.24.cv3.0.2.weight, with a YOLO11 one of
    model.23.cv3.0.2.weight."""
    t = _strip_prefix(tensors)
    key = cls_key(variant)
    if key not in t:
        raise KeyError(f"{key}: not in the state_dict (the class count is read from it)")
    nc = int(np.asarray(t[key]).shape[0])
    if not NC_MIN <= nc <= NC_MAX:
        raise ValueError(f"{key} has {nc} classes: outside the supported range "
                         f"{NC_MIN}..{NC_MAX}")
    return nc


def check_family(t: Dict[str, np.ndarray], variant: int) -> None:
    """Refuse a state_dict that is not of `variant`'s family: an anchor-based
    YOLOv5 checkpoint (the original yolov5 repository's Detect: model.24.m.* /
    model.24.anchors), or the other supported family (recognised by its
    Detect module's layer number)."""
    if any(k.startswith("model.24.m.") or k.startswith("model.24.anchor") for k in t):
        raise ValueError("the state_dict is an anchor-based YOLOv5 checkpoint of the original "
                         "yolov5 repository (it has model.24.m.* / model.24.anchors): a different "
                         "network; the anchor-free 'u' checkpoint (yolov5nu.pt ...) is needed")
    if cls_key(variant) in t:
        return
    for other in (0, 5, 20):  # any variant of each other family
        if family_name(other) != family_name(variant) and cls_key(other) in t:
            raise ValueError(f"the state_dict is a {family_name(other)} one (Detect at "
                             f"{head_prefix(other)[:-1]}) but detect.model names a "
                             f"{family_name(variant)} model (Detect at "
                             f"{head_prefix(variant)[:-1]})")


def _shaped(t: Dict[str, np.ndarray], key: str, shape, variant: int, nc: int) -> np.ndarray:
    a = np.asarray(t[key], np.float32)
    if a.size != int(np.prod(shape)):
        raise ValueError(f"{key}: shape {tuple(a.shape)} does not fit {family_name(variant)} "
                         f"variant {variant} with nc = {nc} (expected {tuple(shape)})")
    return a.reshape(shape)


def flat_from_state_dict(tensors: Dict[str, np.ndarray], variant: int, nc: int = None,
                         return_nc: bool = False):
    """Flat f32 weights (the plan's conv order) from an Ultralytics
    DetectionModel state_dict, fused or not (see the module docstring).  The
    class count is the checkpoint's own (nc_of_state_dict); an `nc` that
    disagrees with it is an error.  return_nc: (flat, nc) instead of flat."""
    t = _strip_prefix(tensors)
    check_family(t, variant)
    have = nc_of_state_dict(t, variant if is_v5u(variant) or is_v11(variant) else None)
    if nc is not None and int(nc) != have:
        raise ValueError(f"detect.nc = {int(nc)} but the checkpoint has {have} classes "
                         f"({cls_key(variant)} has {have} rows)")
    nc = have
    parts = []
    groups = conv_groups(variant, nc)
    for (name, cin, cout, k, s, act), g in zip(conv_list(variant, nc), groups):
        shape = (cout, cin // g, k, k)
        if name + ".conv.weight" in t:  # Conv block (conv + bn + SiLU)
            w = _shaped(t, name + ".conv.weight", shape, variant, nc)
            if name + ".bn.running_var" in t:
                w, b = fold_bn(w, t[name + ".bn.weight"], t[name + ".bn.bias"],
                               t[name + ".bn.running_mean"], t[name + ".bn.running_var"],
                               t.get(name + ".conv.bias"))
            elif name + ".conv.bias" in t:
                b = _shaped(t, name + ".conv.bias", (cout,), variant, nc)
            else:
                raise KeyError(f"{name}: neither .bn.* nor .conv.bias in the state_dict")
        elif name + ".weight" in t:  # Detect's plain nn.Conv2d / the plan's own names
            w = _shaped(t, name + ".weight", shape, variant, nc)
            b = _shaped(t, name + ".bias", (cout,), variant, nc)
        else:
            raise KeyError(f"{name}: no weights in the state_dict "
                           f"(expected {name}.conv.weight or {name}.weight)")
        parts += [w.ravel(), b.reshape(cout)]
    flat = np.concatenate(parts).astype(np.float32)
    return (flat, nc) if return_nc else flat


def load_weights(path: str, variant: int, nc: int = None, return_nc: bool = False):
    """Flat f32 array from a local Ultralytics checkpoint (state_dict keys,
    fused or unfused; see read_state_dict for the accepted formats), with the
    checkpoint's own class count (flat_from_state_dict: `nc`, `return_nc`)."""
    return flat_from_state_dict(read_state_dict(path), variant, nc, return_nc)


DTYPES = {"bf16": 0, "fp8": 1}  # RV_YOLO_DTYPE_BF16 / RV_YOLO_DTYPE_FP8


def check_fp8_nc(dtype: str, nc: int) -> None:
    if dtype == "fp8" and int(nc) != 80:
        raise ValueError(f"dtype 'fp8' supports nc = 80 only (got nc = {int(nc)}): the fp8 parity "
                         "rests on the 80-class calibration; run a custom class count in bf16")


def check_fp8_variant(dtype: str, variant: int) -> None:
    if dtype == "fp8" and (is_v5u(variant) or is_v11(variant)):
        raise ValueError(f"dtype 'fp8' is not available for {family_name(variant)} (variant "
                         f"{int(variant)}): its plans are bf16 only; set detect.dtype to bf16")


def pack(variant: int, flat: np.ndarray, dtype: str = "bf16", nc: int = 80) -> np.ndarray:
    """Device layout as a u8 host array: bf16 [Cout16][ky][kx][Cin32] + f32
    bias, or (dtype 'fp8', nc = 80 only) OCP e4m3 [Cout16][ky][kx][Cin64] +
    f32 bias + f32 per-cout power-of-two scales for every conv the fp8 plan
    runs in fp8.  `flat` holds the state_dict shapes of conv_list(variant, nc)."""
    lib = _lib.load()
    dt = DTYPES[dtype]
    check_fp8_nc(dtype, nc)
    check_fp8_variant(dtype, variant)
    flat = np.ascontiguousarray(flat, np.float32)
    nbytes = lib.rv_yolo_packed_bytes3(variant, dt, int(nc))
    out = np.zeros(nbytes, np.uint8)
    _lib.check(lib.rv_yolo_pack3(variant, dt, int(nc), flat.ctypes.data, flat.size, out.ctypes.data,
                                 nbytes), "rv_yolo_pack3")
    return out


def detector_weights(det_cfg: dict, variant: int) -> Tuple[np.ndarray, int]:
    """(flat weights, class count) for a detect config (default.yaml:38-45
    keys plus ``nc``): ``weights: <path>`` loads a local Ultralytics
    state_dict and takes the class count from it (load_weights; a ``nc`` key
    that disagrees is an error); ``weights: synthetic`` opts in to the seeded
    synthetic weights (``seed``; 80 classes only).  With no ``weights`` key
    the synthetic weights are used too, with a warning: the reference's
    YOLO(model) loads the real checkpoint, and a production run must not
    silently detect with random weights."""
    import warnings
    w = det_cfg.get("weights")
    seed = int(det_cfg.get("seed", 0))
    nc = det_cfg.get("nc")
    if w and str(w).lower() != "synthetic":
        return load_weights(str(w), variant, nc, return_nc=True)
    if is_v5u(variant):
        raise ValueError(f"detect.model={det_cfg.get('model')!r} is a YOLOv5u model and there is "
                         "no shipped synthetic calibration for it: set detect.weights to a local "
                         "state_dict of the 'u' checkpoint")
    if is_v11(variant):
        raise ValueError(f"detect.model={det_cfg.get('model')!r} is a YOLO11 model and there is "
                         "no shipped synthetic calibration for it: set detect.weights to a local "
                         "state_dict of the checkpoint")
    if not w:
        warnings.warn(f"detect.model={det_cfg.get('model', 'yolov8n.pt')!r} but no detect.weights "
                      "file is configured: using seeded SYNTHETIC weights (set detect.weights to "
                      "a local state_dict, or to 'synthetic' to silence this)", RuntimeWarning,
                      stacklevel=3)
    nc = 80 if nc is None else int(nc)
    return synthetic_weights(variant, seed=seed, nc=nc), nc


def weights_from_config(det_cfg: dict, variant: int) -> np.ndarray:
    """The flat weights of detector_weights(det_cfg, variant)."""
    return detector_weights(det_cfg, variant)[0]


def names_from_config(det_cfg: dict, nc: int) -> List[str]:
    """Class names of a detect config as a list indexed by class id:
    ``names`` may be a list or an {id: name} mapping (Ultralytics' `names`;
    ids the mapping leaves out read str(id)).  Without the key: COCO80 for an
    80-class model, else no names -- Detection.cls_name is then str(id), the
    reference's own fallback (yolo_ultralytics.py:51).  More names than
    classes is an error."""
    names = det_cfg.get("names")
    if names is None:
        return list(COCO80) if nc == 80 else []
    if isinstance(names, dict):
        ids = {int(k): str(v) for k, v in names.items()}
        if ids and (min(ids) < 0 or max(ids) >= nc):
            raise ValueError(f"detect.names has class id {max(ids) if max(ids) >= nc else min(ids)}"
                             f" but the model has {nc} classes (ids 0..{nc - 1})")
        return [ids.get(k, str(k)) for k in range(max(ids) + 1)] if ids else []
    names = [str(x) for x in names]
    if len(names) > nc:
        raise ValueError(f"detect.names lists {len(names)} names but the model has {nc} classes")
    return names

"""Test-local statement of YOLOv5u (Ultralytics yolov5.yaml, the anchor-free
"u" models: Conv k6 / C3 / SPPF under the YOLOv8 Detect head), independent of
the native plan in csrc/yolo_def.hip and csrc/yolo.hip.

    scale  depth  width   c1..c5                 rep(3) rep(6) rep(9)
    n      0.33   0.25    16  32  64  128  256     1      2      3
    s      0.33   0.50    32  64 128  256  512     1      2      3
    m      0.67   0.75    48  96 192  384  768     2      4      6
    l      1.00   1.00    64 128 256  512 1024     3      6      9
    x      1.33   1.25    80 160 320  640 1280     4      8     12

     0 Conv(3,  c1, k6 s2 p2)      13 C3(2*c4, c4, rep(3), no shortcut)
     1 Conv(c1, c2, k3 s2)         14 Conv(c4, c3, k1)
     2 C3(c2, c2, rep(3))          15 Upsample x2 nearest
     3 Conv(c2, c3, k3 s2)         16 Concat[15, 4]
     4 C3(c3, c3, rep(6))          17 C3(2*c3, c3, rep(3), no shortcut) -> Detect P3
     5 Conv(c3, c4, k3 s2)         18 Conv(c3, c3, k3 s2)
     6 C3(c4, c4, rep(9))          19 Concat[18, 14]
     7 Conv(c4, c5, k3 s2)         20 C3(2*c3, c4, rep(3), no shortcut) -> Detect P4
     8 C3(c5, c5, rep(3))          21 Conv(c4, c4, k3 s2)
     9 SPPF(c5, c5, 5)             22 Concat[21, 10]
    10 Conv(c5, c4, k1)            23 C3(2*c4, c5, rep(3), no shortcut) -> Detect P5
    11 Upsample x2 nearest         24 Detect(nc) on [17, 20, 23]
    12 Concat[11, 6]

C3(a, b, n, shortcut), c = b / 2: cv1, cv2 = Conv(a, c, 1) on the block's
input; m.i: t -> t + m.i.cv2(m.i.cv1(t)) (the sum only with shortcut),
m.i.cv1 = Conv(c, c, 1), m.i.cv2 = Conv(c, c, 3); output cv3(cat[m(cv1(x)),
cv2(x)]), cv3 = Conv(2c, b, 1).  state_dict order: cv1, cv2, cv3, m.0.cv1,
m.0.cv2, m.1.cv1, ...

The graph is written once (_graph) over four operations -- conv, cat, up,
pool -- and run twice: on torch tensors (V5uRef.forward, the f32 / bf16-storage
reference) and on symbols (expected_producers), which gives for every conv the
ordered list of (producer conv, upsampled?) behind its input channels and the
producer of its residual.  synth_weights_on() is tests/yolo_synth.py's
one-pass weight normaliser for this graph (head prefix model.24., padding 2
on model.0).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import yolo_synth
from oracle import yolo_ref

V5U = {5: "n", 6: "s", 7: "m", 8: "l", 9: "x"}
SCALES = {5: (0.33, 0.25), 6: (0.33, 0.50), 7: (0.67, 0.75), 8: (1.00, 1.00), 9: (1.33, 1.25)}
HEAD = "model.24."
REG = 16
# the issue's table: (convs, fused flat floats at nc = 80, unfused parameter total)
TOTALS = {5: (75, 2649184, 2654816), 6: (75, 9142480, 9153152), 7: (97, 25091520, 25111456),
          8: (119, 53193072, 53225024), 9: (141, 97229632, 97276448)}
POOL = "maxpool"  # the producer of SPPF's pooled channels (no conv)


def widths(variant):
    d, w = SCALES[variant]
    ch = lambda c: int(math.ceil(min(c, 1024) * w / 8) * 8)  # noqa: E731
    rep = lambda n: max(round(n * d), 1)  # noqa: E731
    return [ch(c) for c in (64, 128, 256, 512, 1024)], [rep(n) for n in (3, 6, 9)]


def conv_specs(variant, nc=80):
    """([(name, cin, cout, k, s, silu)] in state_dict order, meta)."""
    (c1, c2, c3, c4, c5), (r3, r6, r9) = widths(variant)
    out = []

    def conv(n, ci, co, k, s, act=1):
        out.append(("model." + n, ci, co, k, s, act))

    def c3blk(p, a, b, n):
        c = b // 2
        conv(p + ".cv1", a, c, 1, 1)
        conv(p + ".cv2", a, c, 1, 1)
        conv(p + ".cv3", 2 * c, b, 1, 1)
        for i in range(n):
            conv(f"{p}.m.{i}.cv1", c, c, 1, 1)
            conv(f"{p}.m.{i}.cv2", c, c, 3, 1)

    conv("0", 3, c1, 6, 2)
    conv("1", c1, c2, 3, 2)
    c3blk("2", c2, c2, r3)
    conv("3", c2, c3, 3, 2)
    c3blk("4", c3, c3, r6)
    conv("5", c3, c4, 3, 2)
    c3blk("6", c4, c4, r9)
    conv("7", c4, c5, 3, 2)
    c3blk("8", c5, c5, r3)
    conv("9.cv1", c5, c5 // 2, 1, 1)
    conv("9.cv2", 2 * c5, c5, 1, 1)
    conv("10", c5, c4, 1, 1)
    c3blk("13", 2 * c4, c4, r3)
    conv("14", c4, c3, 1, 1)
    c3blk("17", 2 * c3, c3, r3)
    conv("18", c3, c3, 3, 2)
    c3blk("20", 2 * c3, c4, r3)
    conv("21", c4, c4, 3, 2)
    c3blk("23", 2 * c4, c5, r3)
    c2d, c3d = max(16, c3 // 4, 4 * REG), max(c3, min(nc, 100))
    for br, wd, last in (("cv2", c2d, 4 * REG), ("cv3", c3d, nc)):
        for i, c in enumerate((c3, c4, c5)):
            conv(f"24.{br}.{i}.0", c, wd, 3, 1)
            conv(f"24.{br}.{i}.1", wd, wd, 3, 1)
            conv(f"24.{br}.{i}.2", wd, last, 1, 1, 0)
    return out, dict(r3=r3, r6=r6, r9=r9, c2d=c2d, c3d=c3d)


def unfused_total(variant, nc=80):
    """Every tensor of the unfused checkpoint: conv weights, BN weight + bias
    per Conv block, the bias of the head's plain convs, DFL's 16."""
    return sum(co * ci * k * k + (2 * co if act else co)
               for n, ci, co, k, s, act in conv_specs(variant, nc)[0]) + REG


def _graph(ops, x, meta):
    """yolov5.yaml on the operations ops = (conv(name, x, res=None), cat(list),
    up(x), pool(x)); returns the three levels' (box, cls) logits."""
    conv, cat, up, pool = ops

    def c3blk(p, x, n, shortcut):
        t = conv(f"model.{p}.cv1", x)
        for i in range(n):
            t = conv(f"model.{p}.m.{i}.cv2", conv(f"model.{p}.m.{i}.cv1", t),
                     res=t if shortcut else None)
        return conv(f"model.{p}.cv3", cat([t, conv(f"model.{p}.cv2", x)]))

    r3, r6, r9 = meta["r3"], meta["r6"], meta["r9"]
    x = conv("model.0", x)
    x = conv("model.1", x)
    x = c3blk(2, x, r3, True)
    x = conv("model.3", x)
    l4 = c3blk(4, x, r6, True)
    x = conv("model.5", l4)
    l6 = c3blk(6, x, r9, True)
    x = conv("model.7", l6)
    x = c3blk(8, x, r3, True)
    s = conv("model.9.cv1", x)
    y1 = pool(s)
    y2 = pool(y1)
    y3 = pool(y2)
    x = conv("model.9.cv2", cat([s, y1, y2, y3]))
    l10 = conv("model.10", x)
    x = c3blk(13, cat([up(l10), l6]), r3, False)
    l14 = conv("model.14", x)
    l17 = c3blk(17, cat([up(l14), l4]), r3, False)
    l20 = c3blk(20, cat([conv("model.18", l17), l14]), r3, False)
    l23 = c3blk(23, cat([conv("model.21", l20), l10]), r3, False)
    outs = []
    for i, f in enumerate((l17, l20, l23)):
        box = conv(f"{HEAD}cv2.{i}.2", conv(f"{HEAD}cv2.{i}.1", conv(f"{HEAD}cv2.{i}.0", f)))
        cls = conv(f"{HEAD}cv3.{i}.2", conv(f"{HEAD}cv3.{i}.1", conv(f"{HEAD}cv3.{i}.0", f)))
        outs.append((box, cls))
    return outs


def expected_producers(variant, nc=80):
    """{conv name: ([(producer conv, upsampled?)] in channel order, residual
    producer or None)}; model.0 reads ("input", False), SPPF's pooled channels
    are one (POOL, False) entry."""
    prod = {}

    def conv(n, x, res=None):
        prod[n] = (list(x), res[0][0] if res is not None else None)
        return [(n, False)]

    def cat(xs):
        out = []
        for t in xs:
            for seg in t:
                if not (out and out[-1] == seg == (POOL, False)):
                    out.append(seg)
        return out

    up = lambda t: [(n, True) for n, _ in t]  # noqa: E731
    pool = lambda t: [(POOL, False)]  # noqa: E731
    _graph((conv, cat, up, pool), [("input", False)], conv_specs(variant, nc)[1])
    return prod


def split_params(variant, flat, nc=80):
    """(specs, {conv name: (weight (cout, cin, k, k), bias (cout,))}) views of flat."""
    specs, _ = conv_specs(variant, nc)
    params, off = {}, 0
    for n, ci, co, k, s, act in specs:
        nw = co * ci * k * k
        params[n] = (flat[off:off + nw].reshape(co, ci, k, k), flat[off + nw:off + nw + co])
        off += nw + co
    assert off == flat.size
    return specs, params


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


class V5uRef:
    """CPU forward of YOLOv5u from flat fused weights, f32 (dtype=torch.float64
    for f64).  quant=True: the HIP path's storage precision as
    yolo_ref.YoloRef(quant=True) -- bf16 weights except model.0, every
    activation rounded to bf16 once after bias / SiLU / residual, f32 head
    logits."""

    def __init__(self, variant, flat, quant=False, nc=80, dtype=torch.float32):
        self.quant, self.dtype = quant, dtype
        self.specs, self.meta = conv_specs(variant, nc)
        _, params = split_params(variant, np.asarray(flat, np.float32), nc)
        self.p = {}
        for n, ci, co, k, s, act in self.specs:
            w, b = (torch.from_numpy(a.copy()) for a in params[n])
            if quant and n != "model.0":
                w = _bf16(w)
            self.p[n] = (w.to(dtype), b.to(dtype), s, k, act)

    @staticmethod
    def pad(n, k):
        return 2 if n == "model.0" else k // 2

    def conv(self, n, x, res=None):
        w, b, s, k, act = self.p[n]
        y = F.conv2d(x, w, b, stride=s, padding=self.pad(n, k))
        y = F.silu(y) if act else y
        if res is not None:
            y = res + y
        if self.quant and not (n.startswith(HEAD) and n.endswith(".2")):
            y = _bf16(y.float()).to(self.dtype)
        return y

    @torch.no_grad()
    def forward(self, x):
        """x: (B, 3, H, W) RGB in [0, 1] -> raw (B, 4 + nc, A)."""
        ops = (self.conv, lambda xs: torch.cat(xs, 1),
               lambda t: F.interpolate(t, scale_factor=2, mode="nearest"),
               lambda t: F.max_pool2d(t, 5, 1, 2))
        outs = _graph(ops, x.to(self.dtype), self.meta)
        return yolo_ref.YoloRef._decode([torch.cat(o, 1).float() for o in outs])


def _is_head(n, branch):
    return n.startswith(f"{HEAD}{branch}.") and n.endswith(".2")


class _Normalising(V5uRef):
    """V5uRef whose conv() rescales its own weights on first use (the rule of
    yolo_synth._Normalising)."""

    def __init__(self, variant, flat, seed, nc, road):
        super().__init__(variant, flat, nc=nc)
        self.seed, self.road = seed, road
        self.order = {n: i for i, (n, *_r) in enumerate(self.specs)}
        self.done = set()
        self.cls_logits = []

    def conv(self, n, x, res=None):
        if n in self.done:
            return super().conv(n, x, res)
        w, b, s, k, act = self.p[n]
        y = F.conv2d(x, w, b, stride=s, padding=self.pad(n, k))
        co = w.shape[0]
        target = (yolo_synth.BOX_STD if _is_head(n, "cv2") else
                  yolo_synth.CLS_STD if _is_head(n, "cv3") else 1.0)
        sc = (target / y.std((0, 2, 3)).clamp_min(1e-6)).float()
        mu = torch.zeros(co)
        if act:
            mu = torch.from_numpy(np.random.default_rng([self.seed, self.order[n]])
                                  .uniform(yolo_synth.MU[0], yolo_synth.MU[1], co).astype(np.float32))
        shift = mu - y.mean((0, 2, 3)) * sc
        if _is_head(n, "cv3") and self.road:
            shift[list(self.road)] += yolo_synth.ROAD_PRIOR
        self.p[n] = (w * sc.view(-1, 1, 1, 1), b * sc + shift, s, k, act)
        self.done.add(n)
        y = y * sc.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if _is_head(n, "cv3"):
            self.cls_logits.append(y.flatten(2))
        y = F.silu(y) if act else y
        return y if res is None else res + y


def synth_weights_on(variant, lb, seed=1, target_cand=0.04, nc=80):
    """Flat f32 weights of YOLOv5u `variant` with `nc` classes, normalised on
    the letterboxed BGR u8 batch `lb` (yolo_synth.synth_weights_on's rule)."""
    from rvs_amd.detect.weights import base_weights
    specs, _ = conv_specs(variant, nc)
    rng = np.random.default_rng(seed)
    flat = []
    for i, (n, ci, co, k, s, act) in enumerate(specs):
        w, b = base_weights(rng, seed, i, ci, co, k, 0.0)
        flat += [w.ravel(), b]
    m = _Normalising(variant, np.concatenate(flat), seed, nc,
                     tuple(c for c in yolo_synth.ROAD if c < nc))
    del flat
    m.forward(yolo_ref.preprocess(lb))
    assert len(m.done) == len(specs) and len(m.cls_logits) == 3
    best = torch.cat(m.cls_logits, 2).max(1).values.numpy().ravel()
    conf = yolo_synth.CONF
    delta = np.float32(np.log(conf / (1 - conf)) - np.quantile(best, 1 - target_cand))
    out = []
    for n, ci, co, k, s, act in specs:
        w, b = m.p[n][0], m.p[n][1]
        if _is_head(n, "cv3"):
            b = b + delta
        out += [w.numpy().ravel(), b.numpy().ravel()]
    return np.concatenate(out).astype(np.float32)


_CASES = {}


def synth_case(variant, H, W, B, nc=80):
    """(flat weights, frames (B, H, W, 3) u8, letterbox (B, H, W, 3) u8) of a
    test geometry at imgsz max(H, W); computed once, read-only."""
    key = (variant, H, W, B, nc)
    if key not in _CASES:
        lb = yolo_synth.letterboxed(H, W, B, max(H, W))
        flat = synth_weights_on(variant, lb, nc=nc)
        fr = yolo_synth.frames(H, W, B)
        for a in (flat, fr, lb):
            a.setflags(write=False)
        if len(_CASES) >= 4:
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = (flat, fr, lb)
    return _CASES[key]


def state_dict(variant, flat, nc=80, fused=True, nested=False, seed=0):
    """An Ultralytics-style state_dict of the flat weights.  fused: conv.weight
    + conv.bias per Conv block.  Unfused: conv.weight + random BatchNorm
    statistics (and the DFL conv and num_batches_tracked, which loaders
    ignore); flat's biases of the Conv blocks are then not represented -- use
    fold_state_dict for the flat array such a dict folds to."""
    specs, params = split_params(variant, flat, nc)
    rng = np.random.default_rng(seed)
    sd = {}
    for n, ci, co, k, s, act in specs:
        w, b = params[n]
        if not act:
            sd[n + ".weight"], sd[n + ".bias"] = w, b
        elif fused:
            sd[n + ".conv.weight"], sd[n + ".conv.bias"] = w, b
        else:
            sd[n + ".conv.weight"] = w
            sd[n + ".bn.weight"] = rng.uniform(0.5, 1.5, co).astype(np.float32)
            sd[n + ".bn.bias"] = rng.normal(0, 0.2, co).astype(np.float32)
            sd[n + ".bn.running_mean"] = rng.normal(0, 0.2, co).astype(np.float32)
            sd[n + ".bn.running_var"] = rng.uniform(0.5, 2.0, co).astype(np.float32)
            sd[n + ".bn.num_batches_tracked"] = np.array(7, np.int64)
    if not fused:
        sd[HEAD + "dfl.conv.weight"] = np.arange(REG, dtype=np.float32).reshape(1, REG, 1, 1)
    return {"model." + k: v for k, v in sd.items()} if nested else sd


def fold_state_dict(variant, sd, nc=80):
    """The flat array an unfused state_dict folds to, through
    rvs_amd.detect.weights.fold_bn conv by conv in this file's conv order."""
    from rvs_amd.detect.weights import fold_bn
    parts = []
    for n, ci, co, k, s, act in conv_specs(variant, nc)[0]:
        if act:
            w, b = fold_bn(sd[n + ".conv.weight"], sd[n + ".bn.weight"], sd[n + ".bn.bias"],
                           sd[n + ".bn.running_mean"], sd[n + ".bn.running_var"])
        else:
            w, b = sd[n + ".weight"], sd[n + ".bias"]
        parts += [np.asarray(w, np.float32).ravel(), np.asarray(b, np.float32).ravel()]
    return np.concatenate(parts)

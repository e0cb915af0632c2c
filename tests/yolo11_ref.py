"""Test-local statement of YOLO11 (Ultralytics yolo11.yaml: Conv / C3k2 /
SPPF / C2PSA under a Detect head whose class branch is depthwise-separable),
independent of the native plan in csrc/yolo_def.hip and csrc/yolo.hip.

    scale  depth width max_ch   a64 a128 a256 a512 a1024   rep   PSA c / heads
    n      0.50  0.25  1024      16   32   64  128   256    1     128 / 2
    s      0.50  0.50  1024      32   64  128  256   512    1     256 / 4
    m      0.50  1.00   512      64  128  256  512   512    1     256 / 4
    l      1.00  1.00   512      64  128  256  512   512    2     256 / 4
    x      1.00  1.50   512      96  192  384  768   768    2     384 / 6
    aX = ceil(min(X, max_ch) * width / 8) * 8;  rep = max(round(2 * depth), 1)

     0 Conv(3, a64, k3 s2)             12 Concat[up2(10), 6]
     1 Conv(a64, a128, k3 s2)          13 C3k2(a1024+a512, a512, c3k=F)
     2 C3k2(a128, a256, c3k=F, e=.25)  15 Concat[up2(13), 4]
     3 Conv(a256, a256, k3 s2)         16 C3k2(a512+a512, a256, c3k=F)  -> Detect P3
     4 C3k2(a256, a512, c3k=F, e=.25)  17 Conv(a256, a256, k3 s2)
     5 Conv(a512, a512, k3 s2)         18 Concat[17, 13]
     6 C3k2(a512, a512, c3k=T)         19 C3k2(a256+a512, a512, c3k=F)  -> Detect P4
     7 Conv(a512, a1024, k3 s2)        20 Conv(a512, a512, k3 s2)
     8 C3k2(a1024, a1024, c3k=T)       21 Concat[20, 10]
     9 SPPF(a1024, a1024, 5)           22 C3k2(a512+a1024, a1024, c3k=T) -> Detect P5
    10 C2PSA(a1024, a1024)             23 Detect(nc) on [16, 19, 22]

Scales m, l, x force c3k = T in every C3k2.  C3k2(a, b, c3k, e = 0.5), c =
int(b e): cv1 = Conv(a, 2c, 1); rep blocks m.i, each on the previous output,
always with the shortcut; cv2 = Conv((2 + rep) c, b, 1) on [y0 | y1 | m.0 ...].
m.i without c3k: t + cv2(cv1(t)), cv1 = Conv(c, c/2, 3), cv2 = Conv(c/2, c, 3).
With c3k (h = c/2): cv3([chain(cv1(t)) | cv2(t)]), cv1, cv2 = Conv(c, h, 1),
two bottlenecks t + cv2(cv1(t)) of 3x3 convs at width h, cv3 = Conv(2h, c, 1).
C2PSA(C, C), c = C/2: cv1 = Conv(C, 2c, 1) -> a | b; rep PSA blocks on b;
cv2 = Conv(2c, C, 1) on [a | b].  PSA: b = b + proj(attn(qkv(b)) + pe(v)),
b = b + ffn.1(ffn.0(b)); heads = c/64, per head 128 qkv channels = q 32 | k 32
| v 64, softmax(q^T k 32^-1/2) over the keys, o channel 64 h + d; pe =
DWConv(c, c, 3) on v in that order; qkv, proj, pe and ffn.1 have no activation.
Detect: the box branch is YOLOv8's; the class branch is DWConv(x, x, 3),
Conv(x, c3d, 1), DWConv(c3d, c3d, 3), Conv(c3d, c3d, 1), Conv2d(c3d, nc, 1).

The graph is written once (_graph) over six operations -- conv, dwconv, attn,
cat, up, pool -- and run twice: on torch tensors (Y11Ref.forward) and on
symbols (expected_producers).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import yolo_synth
from oracle import yolo_ref

V11 = {20: "n", 21: "s", 22: "m", 23: "l", 24: "x"}
SCALES = {20: (0.50, 0.25, 1024), 21: (0.50, 0.50, 1024), 22: (0.50, 1.00, 512),
          23: (1.00, 1.00, 512), 24: (1.00, 1.50, 512)}
HEAD = "model.23."
REG = 16
# the issue's table: (convs, depthwise convs, fused flat floats at nc = 80,
# published unfused parameter total)
TOTALS = {20: (87, 7, 2616232, 2624080), 21: (87, 7, 9443744, 9458752),
          22: (112, 7, 20091696, 20114688), 23: (173, 8, 25340976, 25372160),
          24: (173, 8, 56919408, 56966176)}
# YOLO11n at other class counts: nc -> (flat floats, c3d)
N_TOTALS = {1: (2582331, 64), 70: (2602362, 70), 128: (2656056, 100)}
POOL = "maxpool"  # the producer of SPPF's pooled channels (no conv)


def widths(variant):
    d, w, mc = SCALES[variant]
    ch = lambda c: int(math.ceil(min(c, mc) * w / 8) * 8)  # noqa: E731
    return [ch(c) for c in (64, 128, 256, 512, 1024)], max(round(2 * d), 1)


def conv_specs(variant, nc=80):
    """([(name, cin, cout, k, s, silu)] in state_dict order, meta); meta["dw"]
    is the set of depthwise convs (weight [cout][1][k][k])."""
    (a64, a128, a256, a512, a1024), rep = widths(variant)
    big = variant >= 22
    out, dw = [], set()

    def conv(n, ci, co, k, s, act=1):
        out.append(("model." + n, ci, co, k, s, act))

    def dwconv(n, c, act):
        conv(n, c, c, 3, 1, act)
        dw.add("model." + n)

    def c3k2(p, a, b, c3k, e=0.5):
        c = int(b * e)
        conv(p + ".cv1", a, 2 * c, 1, 1)
        conv(p + ".cv2", (2 + rep) * c, b, 1, 1)
        for i in range(rep):
            q = f"{p}.m.{i}"
            if not (c3k or big):
                conv(q + ".cv1", c, c // 2, 3, 1)
                conv(q + ".cv2", c // 2, c, 3, 1)
                continue
            h = c // 2
            conv(q + ".cv1", c, h, 1, 1)
            conv(q + ".cv2", c, h, 1, 1)
            conv(q + ".cv3", 2 * h, c, 1, 1)
            for j in range(2):
                conv(f"{q}.m.{j}.cv1", h, h, 3, 1)
                conv(f"{q}.m.{j}.cv2", h, h, 3, 1)

    conv("0", 3, a64, 3, 2)
    conv("1", a64, a128, 3, 2)
    c3k2("2", a128, a256, False, 0.25)
    conv("3", a256, a256, 3, 2)
    c3k2("4", a256, a512, False, 0.25)
    conv("5", a512, a512, 3, 2)
    c3k2("6", a512, a512, True)
    conv("7", a512, a1024, 3, 2)
    c3k2("8", a1024, a1024, True)
    conv("9.cv1", a1024, a1024 // 2, 1, 1)
    conv("9.cv2", 2 * a1024, a1024, 1, 1)
    c = a1024 // 2
    conv("10.cv1", a1024, 2 * c, 1, 1)
    conv("10.cv2", 2 * c, a1024, 1, 1)
    for i in range(rep):
        q = f"10.m.{i}"
        conv(q + ".attn.qkv", c, 2 * c, 1, 1, 0)
        conv(q + ".attn.proj", c, c, 1, 1, 0)
        dwconv(q + ".attn.pe", c, 0)
        conv(q + ".ffn.0", c, 2 * c, 1, 1)
        conv(q + ".ffn.1", 2 * c, c, 1, 1, 0)
    c3k2("13", a1024 + a512, a512, False)
    c3k2("16", a512 + a512, a256, False)
    conv("17", a256, a256, 3, 2)
    c3k2("19", a256 + a512, a512, False)
    conv("20", a512, a512, 3, 2)
    c3k2("22", a512 + a1024, a1024, True)
    c2d, c3d = max(16, a256 // 4, 4 * REG), max(a256, min(nc, 100))
    for i, x in enumerate((a256, a512, a1024)):
        conv(f"23.cv2.{i}.0", x, c2d, 3, 1)
        conv(f"23.cv2.{i}.1", c2d, c2d, 3, 1)
        conv(f"23.cv2.{i}.2", c2d, 4 * REG, 1, 1, 0)
    for i, x in enumerate((a256, a512, a1024)):
        dwconv(f"23.cv3.{i}.0.0", x, 1)
        conv(f"23.cv3.{i}.0.1", x, c3d, 1, 1)
        dwconv(f"23.cv3.{i}.1.0", c3d, 1)
        conv(f"23.cv3.{i}.1.1", c3d, c3d, 1, 1)
        conv(f"23.cv3.{i}.2", c3d, nc, 1, 1, 0)
    return out, dict(rep=rep, big=big, c2d=c2d, c3d=c3d, dw=dw, psa_c=c, heads=c // 64)


def weight_shape(spec, dw):
    n, ci, co, k, s, act = spec
    return (co, 1 if n in dw else ci, k, k)


def flat_total(variant, nc=80):
    specs, meta = conv_specs(variant, nc)
    return sum(int(np.prod(weight_shape(sp, meta["dw"]))) + sp[2] for sp in specs)


def unfused_total(variant, nc=80):
    """Every tensor of the unfused checkpoint: conv weights, BN weight + bias
    per Conv block (every conv but the head's plain ones -- qkv, proj, pe and
    ffn.1 are Conv blocks with act=False), the plain convs' biases, DFL's 16."""
    specs, meta = conv_specs(variant, nc)
    return sum(int(np.prod(weight_shape(sp, meta["dw"]))) + (sp[2] if _is_plain(sp[0]) else 2 * sp[2])
               for sp in specs) + REG


def _is_plain(n):
    """The Detect head's nn.Conv2d layers (state_dict keys n.weight / n.bias)."""
    return n.startswith(HEAD) and n.endswith(".2")


def _graph(ops, x, meta):
    """yolo11.yaml on the operations ops = (conv(name, x, res=None),
    dwconv(name, x, res=None), attn(prefix, qkv) -> (o, v), cat(list), up(x),
    pool(x)); returns the three levels' (box, cls) logits."""
    conv, dwconv, attn, cat, up, pool = ops
    rep, big = meta["rep"], meta["big"]

    def bneck(p, t):
        return conv(p + ".cv2", conv(p + ".cv1", t), res=t)

    def c3k(p, t):
        u = conv(p + ".cv1", t)
        for j in range(2):
            u = bneck(f"{p}.m.{j}", u)
        return conv(p + ".cv3", cat([u, conv(p + ".cv2", t)]))

    def c3k2(i, x, nested):
        p = f"model.{i}"
        y = conv(p + ".cv1", x)          # [y0 | y1]; m.0 reads y1
        ys, t = [y], ("half", y)
        for j in range(rep):
            t_in = t
            t = (c3k if (nested or big) else bneck)(f"{p}.m.{j}", t_in)
            ys.append(t)
        return conv(p + ".cv2", cat(ys))

    # `("half", y)`: the second half of y's channels -- resolved by the ops
    x = conv("model.0", x)
    x = conv("model.1", x)
    x = c3k2(2, x, False)
    x = conv("model.3", x)
    l4 = c3k2(4, x, False)
    x = conv("model.5", l4)
    l6 = c3k2(6, x, True)
    x = conv("model.7", l6)
    x = c3k2(8, x, True)
    s = conv("model.9.cv1", x)
    y1 = pool(s)
    y2 = pool(y1)
    y3 = pool(y2)
    x = conv("model.9.cv2", cat([s, y1, y2, y3]))
    ab = conv("model.10.cv1", x)
    a, b = ("first", ab), ("half", ab)
    for i in range(rep):
        q = f"model.10.m.{i}"
        o, v = attn(q + ".attn", conv(q + ".attn.qkv", b))
        b = conv(q + ".attn.proj", dwconv(q + ".attn.pe", v, res=o), res=b)
        b = conv(q + ".ffn.1", conv(q + ".ffn.0", b), res=b)
    l10 = conv("model.10.cv2", cat([a, b]))
    l13 = c3k2(13, cat([up(l10), l6]), False)
    l16 = c3k2(16, cat([up(l13), l4]), False)
    l19 = c3k2(19, cat([conv("model.17", l16), l13]), False)
    l22 = c3k2(22, cat([conv("model.20", l19), l10]), True)
    outs = []
    for i, f in enumerate((l16, l19, l22)):
        box = conv(f"{HEAD}cv2.{i}.2", conv(f"{HEAD}cv2.{i}.1", conv(f"{HEAD}cv2.{i}.0", f)))
        t = conv(f"{HEAD}cv3.{i}.0.1", dwconv(f"{HEAD}cv3.{i}.0.0", f))
        t = conv(f"{HEAD}cv3.{i}.1.1", dwconv(f"{HEAD}cv3.{i}.1.0", t))
        outs.append((box, conv(f"{HEAD}cv3.{i}.2", t)))
    return outs


HALF, FIRST, V = "[1/2:]", "[:1/2]", "[v]"  # producer-name tags: the part of its output read


def expected_producers(variant, nc=80):
    """{op name: ([(producer, upsampled?)] in channel order, residual producer
    or None)} for every conv (depthwise ones included) and every attention
    ("model.10.m.i.attn", reading its qkv conv).  A producer name carries a
    tag when only part of its output is read: HALF (the second half of its
    channels: a C3k2's first block on y1, the PSA blocks on b), FIRST (the
    first half: C2PSA.cv2 on a) or V (the v channels of a qkv conv, read by
    attn.pe, whose residual is the attention).  model.0 reads ("input",
    False); SPPF's pooled channels are one (POOL, False) entry."""
    prod = {}

    def sym(t):
        if not isinstance(t, tuple):
            return t
        return [(n + (HALF if t[0] == "half" else FIRST), u) for n, u in t[1]]

    def conv(n, x, res=None):
        prod[n] = (list(sym(x)), sym(res)[0][0] if res is not None else None)
        return [(n, False)]

    def attn(n, qkv):
        prod[n] = (list(qkv), None)
        return [(n, False)], [(m + V, u) for m, u in qkv]

    def cat(xs):
        out = []
        for t in xs:
            for seg in sym(t):
                if not (out and out[-1] == seg == (POOL, False)):
                    out.append(seg)
        return out

    up = lambda t: [(n, True) for n, _ in t]  # noqa: E731
    pool = lambda t: [(POOL, False)]  # noqa: E731
    _graph((conv, conv, attn, cat, up, pool), [("input", False)], conv_specs(variant, nc)[1])
    return prod


def split_params(variant, flat, nc=80):
    """(specs, {conv name: (weight (cout, cin / groups, k, k), bias (cout,))}) views of flat."""
    specs, meta = conv_specs(variant, nc)
    params, off = {}, 0
    for sp in specs:
        shp = weight_shape(sp, meta["dw"])
        nw, co = int(np.prod(shp)), sp[2]
        params[sp[0]] = (flat[off:off + nw].reshape(shp), flat[off + nw:off + nw + co])
        off += nw + co
    assert off == flat.size
    return specs, params


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def attention(qkv, heads):
    """Ultralytics Attention.forward between qkv and pe / proj: (B, 2c, H, W)
    -> (o, v), both (B, c, H, W), channel 64 h + d."""
    B, C2, H, W = qkv.shape
    N = H * W
    q, k, v = qkv.view(B, heads, 128, N).split([32, 32, 64], dim=2)
    att = (q.transpose(-2, -1) @ k) * 32 ** -0.5
    att = att.softmax(dim=-1)
    o = (v @ att.transpose(-2, -1)).view(B, C2 // 2, H, W)
    return o, v.reshape(B, C2 // 2, H, W)


class Y11Ref:
    """CPU forward of YOLO11 from flat fused weights, f32 (dtype=torch.float64
    for f64).  quant=True: the HIP path's storage precision -- bf16 weights
    except model.0, every activation (the attention output included) rounded
    to bf16 once after bias / SiLU / residual, f32 head logits."""

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
    def pick(x):
        """("half" / "first", t) -> that half of t's channels."""
        if not isinstance(x, tuple):
            return x
        c = x[1].shape[1] // 2
        return x[1][:, c:] if x[0] == "half" else x[1][:, :c]

    def _round(self, n, y):
        if self.quant and not _is_plain(n):
            y = _bf16(y.float()).to(self.dtype)
        return y

    def conv(self, n, x, res=None):
        x = self.pick(x)
        w, b, s, k, act = self.p[n]
        y = F.conv2d(x, w, b, stride=s, padding=k // 2, groups=x.shape[1] // w.shape[1])
        y = F.silu(y) if act else y
        if res is not None:
            y = self.pick(res) + y
        return self._round(n, y)

    def attn(self, n, qkv):
        o, v = attention(qkv, self.meta["heads"])
        return self._round(n, o), v

    def ops(self):
        return (self.conv, self.conv, self.attn, lambda xs: torch.cat([self.pick(t) for t in xs], 1),
                lambda t: F.interpolate(t, scale_factor=2, mode="nearest"),
                lambda t: F.max_pool2d(t, 5, 1, 2))

    @torch.no_grad()
    def forward(self, x):
        """x: (B, 3, H, W) RGB in [0, 1] -> raw (B, 4 + nc, A)."""
        outs = _graph(self.ops(), x.to(self.dtype), self.meta)
        return yolo_ref.YoloRef._decode([torch.cat(o, 1).float() for o in outs])


def _is_head(n, branch):
    return n.startswith(f"{HEAD}{branch}.") and n.endswith(".2")


class _Normalising(Y11Ref):
    """Y11Ref whose conv() rescales its own weights on first use (the rule of
    yolo_synth._Normalising; convs without activation get mean 0)."""

    def __init__(self, variant, flat, seed, nc, road):
        super().__init__(variant, flat, nc=nc)
        self.seed, self.road = seed, road
        self.order = {n: i for i, (n, *_r) in enumerate(self.specs)}
        self.done = set()
        self.cls_logits = []

    def conv(self, n, x, res=None):
        if n in self.done:
            return super().conv(n, x, res)
        x = self.pick(x)
        w, b, s, k, act = self.p[n]
        y = F.conv2d(x, w, b, stride=s, padding=k // 2, groups=x.shape[1] // w.shape[1])
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
        return y if res is None else self.pick(res) + y


def base_flat(variant, seed=1, nc=80):
    """He-normal base weights in conv order (depthwise: fan-in k * k)."""
    from rvs_amd.detect.weights import base_weights
    specs, meta = conv_specs(variant, nc)
    rng = np.random.default_rng(seed)
    flat = []
    for i, sp in enumerate(specs):
        co, ci, k, _ = weight_shape(sp, meta["dw"])
        w, b = base_weights(rng, seed, i, ci, co, k, 0.0)
        flat += [w.ravel(), b]
    return np.concatenate(flat)


def synth_weights_on(variant, lb, seed=1, target_cand=0.04, nc=80):
    """Flat f32 weights of YOLO11 `variant` with `nc` classes, normalised on
    the letterboxed BGR u8 batch `lb` (yolo_synth.synth_weights_on's rule)."""
    specs, _ = conv_specs(variant, nc)
    m = _Normalising(variant, base_flat(variant, seed, nc), seed, nc,
                     tuple(c for c in yolo_synth.ROAD if c < nc))
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
    + conv.bias per Conv block (DWConv and the activation-free blocks are Conv
    blocks too).  Unfused: conv.weight + random BatchNorm statistics (and the
    DFL conv and num_batches_tracked, which loaders ignore); flat's biases of
    the Conv blocks are then not represented -- use fold_state_dict for the
    flat array such a dict folds to."""
    specs, params = split_params(variant, flat, nc)
    rng = np.random.default_rng(seed)
    sd = {}
    for n, ci, co, k, s, act in specs:
        w, b = params[n]
        if _is_plain(n):
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
        if _is_plain(n):
            w, b = sd[n + ".weight"], sd[n + ".bias"]
        else:
            w, b = fold_bn(sd[n + ".conv.weight"], sd[n + ".bn.weight"], sd[n + ".bn.bias"],
                           sd[n + ".bn.running_mean"], sd[n + ".bn.running_var"])
        parts += [np.asarray(w, np.float32).ravel(), np.asarray(b, np.float32).ravel()]
    return np.concatenate(parts)

"""rv_conv_bf16, the single-layer entry of the conv launcher, off the shapes
the YOLOv8 plans use: its three kernels (conv_patch_kernel in its 4- and
8-wave forms, conv1x1_direct_kernel, and the generic conv_mfma_kernel no plan
reaches) against float64 at tiny and odd maps, YOLOv8x's channel counts,
channel strides on both sides of the fast epilogue's 2048 limit, and every
explicit tile configuration; and its argument contract (include/rvhip.h) on
both sides.

Reference: F.conv2d in float64 on the bf16 input and weights, then SiLU,
then the residual.  Bars (test_yolo_layers_gpu.py's): every element finite
and within 2 bf16 ulp + 1e-3 RMS, and fewer than 1e-4 of the elements beyond
1.01 ulp + 1e-3 RMS; every case has at least 2e4 output elements (B is chosen
for that), so the fraction bar allows at least two elements.

Buffers: input, output and residual are channel slices of wider tensors
(pointer at a nonzero channel offset, *_cs the wide width).  The input
tensor's other channels hold large finite values (a read at a wrong channel
offset meets nonzero weights and changes the result), or NaN in the cases
whose Cin is exactly the contract's granularity (the padding lanes' zero
weights must never meet them).  The output tensor's other channels and one
guard image before and after hold a fixed bit pattern that must survive.

Explicit configurations {MR, NR, G = 1, resw, persist, kind}: every one that
rv_conv_bf16 accepts must reproduce the default configuration's bits.  Which
kinds must have run at least once per shape (`kinds_that_apply`): kind 0, the
4-wave patch kernel, for every k / stride it is built for (all but 1x1
stride 2, where every configuration is rejected, so the default call's
success means the generic kernel ran); kind 1, the direct kernel, for 1x1
stride 1; kind 2, the 8-wave patch kernel, for 3x3 convs of at least two
16-channel output fragments (its tiles are at least two fragments tall and
conv_cfg_ok rejects a tile taller than the layer) -- except at stride 2 on a
map one pixel wide: an 8-wave tile has at least 128 pixel slots and is no
wider than the map, so it is 128 rows tall, its stride-2 input patch 257 x 3
pixels of 64 bytes = 49 KB per pipeline stage, and two such stages plus two
stages (or one resident slab) of two fragments' 3x3 weights exceed the
160 KB of LDS.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_yolo_layers_gpu import ulp_bf16

pytestmark = pytest.mark.gpu

RV_EINVAL = -1000  # include/rvhip.h
PATTERN = 0x5AA5  # bf16 bits of every output element the call must not write
MIN_ELEMS = 20000
TILES = [(8, 2), (8, 1), (5, 2), (5, 1), (4, 4), (4, 2), (4, 1), (2, 4), (2, 2), (2, 1), (1, 4),
         (1, 2), (1, 1)]  # RV_TILES of csrc/conv_kernels.h
CONFIGS = [(mr, nr, 1, resw, persist, kind) for (mr, nr) in TILES for kind in (0, 1, 2)
           for resw in (0, 1) for persist in (0, 1)]


def kinds_that_apply(k, stride, Cout, Wo):
    if k == 1 and stride == 2:
        return set()
    kinds = {0}
    if k == 1:
        kinds.add(1)
    if k == 3 and Cout >= 32 and not (stride == 2 and Wo == 1):
        kinds.add(2)
    return kinds


class Case:
    """One conv call: tensors on the device, the float64 reference on the host."""

    def __init__(self, cuda, k, stride, Hin, Win, Cin, Cout, act, res, in_cs=None, in_co=8,
                 out_cs=None, out_co=8, res_cs=None, res_co=4, junk=1.0e6, seed=0):
        from rvs_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.k, self.stride, self.Hin, self.Win, self.Cin, self.Cout = k, stride, Hin, Win, Cin, Cout
        self.act, self.has_res = act, res
        Ho, Wo = (Hin - 1) // stride + 1, (Win - 1) // stride + 1  # pad k / 2
        self.Ho, self.Wo = Ho, Wo
        B = self.B = max(2, -(-MIN_ELEMS // (Ho * Wo * Cout)))
        assert B * Ho * Wo * Cout >= MIN_ELEMS
        self.in_cs = in_cs or Cin + 24
        self.out_cs = out_cs or Cout + 24
        self.res_cs = res_cs or Cout + 12
        self.in_co, self.out_co, self.res_co = in_co, out_co, res_co
        assert in_co + Cin <= self.in_cs and out_co + Cout <= self.out_cs
        assert res_co + Cout <= self.res_cs
        g = torch.Generator().manual_seed(1000 + seed)
        x = (torch.randn((B, Hin, Win, Cin), generator=g) * 0.5).to(torch.bfloat16)
        wt = (torch.randn((Cout, Cin, k, k), generator=g) / (Cin * k * k) ** 0.5).to(torch.bfloat16)
        bias = torch.randn(Cout, generator=g) * 0.1
        r = (torch.randn((B, Ho, Wo, Cout), generator=g) * 0.5).to(torch.bfloat16)
        # the wide tensors
        xin = torch.full((B, Hin, Win, self.in_cs), junk, dtype=torch.bfloat16)
        xin[..., 0::2] = -xin[..., 0::2]
        xin[..., in_co:in_co + Cin] = x
        rin = torch.full((B, Ho, Wo, self.res_cs), junk, dtype=torch.bfloat16)
        rin[..., res_co:res_co + Cout] = r
        cp, kp = 16 * ((Cout + 15) // 16), 32 * ((Cin + 31) // 32)
        wp = torch.zeros((cp, k * k, kp), dtype=torch.bfloat16)
        wp[:Cout, :, :Cin] = wt.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin)
        bp = torch.zeros(cp)
        bp[:Cout] = bias
        self.x, self.w, self.b, self.r = xin.to(cuda), wp.to(cuda), bp.to(cuda), rin.to(cuda)
        # output: guard image, B images, guard image
        self.fill = torch.full((B + 2, Ho, Wo, self.out_cs), PATTERN, dtype=torch.int16, device=cuda)
        self.out = self.fill.clone()
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), bias.double(), stride=stride,
                       padding=k // 2)
        assert ref.shape[2:] == (Ho, Wo)
        if act:
            ref = ref * torch.sigmoid(ref)
        ref = ref.permute(0, 2, 3, 1)
        self.ref = (ref + r.double() if res else ref).numpy()

    def run(self, cfg=None, in_shift=0, out_shift=0, res_shift=0, **over):
        """One call into a freshly pattern-filled output; returns the status.
        *_shift: extra elements on a pointer (contract tests), `over`:
        overridden integer arguments."""
        self.out.copy_(self.fill)
        a = dict(Cin=self.Cin, in_cs=self.in_cs, Cout=self.Cout, out_cs=self.out_cs,
                 res_cs=self.res_cs)
        a.update(over)
        esz = 2
        px = self.Ho * self.Wo * self.out_cs  # skip the leading guard image
        st = self.lib.rv_conv_bf16(
            self._lib.ptr(self.x) + (self.in_co + in_shift) * esz, self.B, self.Hin, self.Win,
            a["Cin"], a["in_cs"], self._lib.ptr(self.w), self._lib.ptr(self.b), a["Cout"], self.k,
            self.stride, self._lib.ptr(self.out) + (px + self.out_co + out_shift) * esz,
            a["out_cs"], (self._lib.ptr(self.r) + (self.res_co + res_shift) * esz)
            if self.has_res else None, a["res_cs"], self.act,
            self._lib.int_array(cfg) if cfg is not None else None, self._lib.stream_ptr())
        torch.cuda.synchronize()
        return st

    def untouched(self):
        return torch.equal(self.out, self.fill)

    def check_against_reference(self, what):
        out = self.out.cpu().numpy()
        sl = slice(self.out_co, self.out_co + self.Cout)
        guard = out.copy()
        guard[1:-1, ..., sl] = PATTERN
        assert (guard == PATTERN).all(), f"{what}: wrote outside its channel slice / images"
        bits = out[1:-1, ..., sl].astype(np.uint16)
        got = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        assert np.isfinite(got).all(), f"{what}: non-finite output"
        ref = self.ref
        rms = float(np.sqrt(np.mean(ref ** 2)))
        d = np.abs(got - ref)
        frac = float((d > 1.01 * ulp_bf16(ref) + 1e-3 * rms).mean())
        worst = float((d / (2 * ulp_bf16(ref) + 1e-3 * rms)).max())
        print(f"{what}: B={self.B} {got.size} elements, {frac:.2e} beyond 1 ulp, "
              f"worst element at {worst:.2f} of the 2 ulp + 1e-3 rms bar")
        assert (d <= 2 * ulp_bf16(ref) + 1e-3 * rms).all(), f"{what}: max dev {d.max()}"
        assert frac < 1e-4, f"{what}: {frac:.2e} of the elements beyond 1 ulp"

    def sweep(self, what):
        """Default configuration against the reference, then every explicit
        configuration that is valid for the layer against the default's bits."""
        assert self.run() == 0, self._lib.load().rv_last_error()
        self.check_against_reference(what)
        base = self.out.clone()
        ran = {0: [], 1: [], 2: []}
        for cfg in CONFIGS:
            st = self.run(cfg)
            if st == RV_EINVAL:
                assert self.untouched(), f"{what}: rejected configuration {cfg} wrote output"
                continue
            assert st == 0, f"{what}: configuration {cfg} failed with status {st}"
            assert torch.equal(self.out, base), f"{what}: configuration {cfg} differs from the default"
            ran[cfg[5]].append(cfg)
        print(f"{what}: ran " + ", ".join(
            f"kind {kd}: {len(v)} [" + " ".join("%dx%d/r%dp%d" % (c[0], c[1], c[3], c[4]) for c in v)
            + "]" for kd, v in ran.items()))
        need = kinds_that_apply(self.k, self.stride, self.Cout, self.Wo)
        for kd in (0, 1, 2):
            if kd in need:
                assert ran[kd], f"{what}: no explicit configuration of kind {kd} ran"
        if not need:  # 1x1 stride 2: the default ran the generic kernel
            assert not any(ran.values()), f"{what}: a patch configuration accepted a 1x1 stride-2 conv"
        return ran


KS = [(1, 1), (3, 1), (3, 2), (1, 2)]
MAPS = [(1, 1), (3, 5), (13, 19), (6, 17)]  # (13, 19) -> 7x10 at stride 2; Wo = 17 below
CHANNELS = [(16, 16), (80, 80), (48, 80), (96, 640), (1280, 64)]
ACT_RES = [(1, 1), (0, 0), (1, 0), (0, 1)]


def _grid():
    """k / stride x map x channels; (act, residual) rotates so that each k /
    stride, each map and each channel pair meets all four combinations."""
    out = []
    for i, ((k, s), (ci, co)) in enumerate(itertools.product(KS, CHANNELS)):
        if ci == 1280 and k != 1:
            continue
        for j, (h, w) in enumerate(MAPS):
            if (h, w) == (6, 17) and s == 2:
                w = 33  # Wo = 17: one column past a 16-column tile
            act, res = ACT_RES[(i + j) % 4]
            out.append((k, s, h, w, ci, co, act, res))
    return out


@pytest.mark.parametrize("k,s,H,W,Cin,Cout,act,res", _grid())
def test_shapes_against_float64_and_every_configuration(cuda, k, s, H, W, Cin, Cout, act, res):
    c = Case(cuda, k, s, H, W, Cin, Cout, act, res)
    c.sweep(f"k{k}s{s} {H}x{W} {Cin}->{Cout} act{act} res{res}")


@pytest.mark.parametrize("res", [1, 0])
@pytest.mark.parametrize("cs", [2040, 2048, 2560])
@pytest.mark.parametrize("k", [3, 1])
def test_channel_strides_around_the_fast_epilogue_limit(cuda, k, cs, res):
    """Output and residual views of 2040, 2048 and 2560 channels per pixel
    (YOLOv8l's and x's model.6 concat buffers are 2048 and 2560 wide): below
    2048 the patch and direct kernels run epilogue_fast, from 2048 on the
    generic epilogue with its 64-bit addresses."""
    c = Case(cuda, k, 1, 9, 11, 32, 32, 1, res, out_cs=cs, out_co=cs - 40, res_cs=cs, res_co=cs - 72)
    c.sweep(f"k{k}s1 9x11 32->32 out_cs=res_cs={cs} res{res}")


@pytest.mark.parametrize("k,s", KS)
def test_unused_input_channels_may_hold_nan(cuda, k, s):
    """Cin = 8, one 16-byte load: the other channels of the wide input tensor
    are NaN.  The kernels pad Cin to 32 with zero weights; a padding lane that
    loaded a neighbouring channel would turn the output NaN (NaN * 0)."""
    c = Case(cuda, k, s, 13, 19, 8, 16, 1, 1, junk=float("nan"))
    c.sweep(f"k{k}s{s} 13x19 8->16 NaN around the input slice")


@pytest.mark.parametrize("k,s", KS)
@pytest.mark.parametrize("Cout,out_cs,out_co", [(20, 28, 4), (16, 20, 4), (36, 44, 4)])
def test_output_side_in_whole_fours(cuda, k, s, Cout, out_cs, out_co):
    """The contract's output granularity: Cout, out_cs, res_cs and the slice
    offsets in whole 4 channels (8-byte aligned views), Cin and in_cs in whole
    8s.  Cout % 16 != 0 takes the generic epilogue; Cout = 16 in a 20-wide
    tensor the fast one, its 16-byte stores at 8-byte alignment."""
    c = Case(cuda, k, s, 13, 19, 8, Cout, 1, 1, in_cs=16, in_co=8, out_cs=out_cs, out_co=out_co,
             res_cs=Cout + 4, res_co=4)
    c.sweep(f"k{k}s{s} 13x19 8->{Cout} out_cs={out_cs}")


REJECTED = [
    ("Cin not a multiple of 8", dict(Cin=12)),
    ("in_cs not a multiple of 8", dict(in_cs=44)),
    ("Cout not a multiple of 4", dict(Cout=14)),
    ("out_cs not a multiple of 4", dict(out_cs=42)),
    ("res_cs not a multiple of 4", dict(res_cs=30)),
    ("in_cs below Cin", dict(in_cs=8)),
    ("out_cs below Cout", dict(out_cs=12)),
    ("input view 8-byte aligned only", dict(in_shift=4)),
    ("output view 4-byte aligned only", dict(out_shift=2)),
    ("residual view 4-byte aligned only", dict(res_shift=2)),
]


@pytest.mark.parametrize("k,s", KS)
def test_contract_violations_are_rejected_before_any_launch(cuda, k, s):
    """Every violation of the documented contract returns RV_EINVAL with the
    output bit-untouched, with the default and with an explicit
    configuration; the same call without the violation succeeds."""
    c = Case(cuda, k, s, 13, 19, 16, 16, 1, 1)
    assert c.run() == 0 and not c.untouched()
    for why, args in REJECTED:
        for cfg in (None, (1, 1, 1, 1, 1, 0)):
            assert c.run(cfg, **args) == RV_EINVAL, why
            assert c.untouched(), why

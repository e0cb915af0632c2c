"""Every path of the preprocess kernels (csrc/preprocess.hip) against the
oracle on the named cases of tests/preprocess_cases.py: the three histogram
forms of the LUT kernel (u16 pairs summed as words, u16 pairs summed by
halves, u32) on flat tiles that fill one bin past 65 535 and on spread ones,
its vector loader at one group and at more than 256 groups a row and its
scalar loader on reflected tiles, grids of 1, 2 and 64 tiles on frames
smaller than the grid, every class of the clip redistribution; the colour
arithmetic of the three CLAHE appliers and the Lab tables on a lattice of
every saturated colour; the median kernels (3 x 3 byte-permute form, radix
select at k = 5, 7, 9) on windows that split at the rank, on two-level and
full-range noise, on frames smaller than a halo and one pixel either side of
a block edge; every entry on views that start one pixel into a wider buffer;
the gray span with its extremes on the last pixel a block reaches; the gated
chain by ops (16-byte copies) and fused; the fused letterbox in its blend,
copy, identity and pad forms.  test_preprocess_cases_cpu.py proves from the
host predicates and the oracle alone that every case runs the path and the
regime it is named for.

No tolerances: uint8 work, compared byte for byte.  Every case is one call
of its entry; the input must come back unchanged and, on a view, the
buffers' padding columns untouched.  Where a second route to the same bytes
exists (the fused pass and the eager calls, the chain and the fused entry)
the two device results are compared as well."""
import ctypes

import numpy as np
import pytest

import preprocess_cases as pc

pytestmark = pytest.mark.gpu


def _eager(case, x):
    """The same bytes by the unfused eager calls (CLAHE apply + median)."""
    from rvs_amd import kernels
    return kernels.median(kernels.clahe_ycrcb(x, case.tiles, case.clip), case.k).cpu().numpy()


def _run(cuda, name):
    case = pc.cases()[name]
    dv = pc.device_run(case, cuda)
    pc.compare(case, dv)
    return case, dv


@pytest.mark.parametrize("name", pc.group("clahe"))
def test_clahe_histogram_and_lut(cuda, name):
    case, dv = _run(cuda, name)
    if case.entry == "clahe_median":
        np.testing.assert_array_equal(dv.proc, _eager(case, dv.x))


@pytest.mark.parametrize("name", pc.group("colour"))
def test_colour(cuda, name):
    case, dv = _run(cuda, name)
    if case.entry == "clahe_median":
        np.testing.assert_array_equal(dv.proc, _eager(case, dv.x))


@pytest.mark.parametrize("name", pc.group("median"))
def test_median(cuda, name):
    case, dv = _run(cuda, name)
    if case.entry == "clahe_median":
        np.testing.assert_array_equal(dv.proc, _eager(case, dv.x))


@pytest.mark.parametrize("name", pc.group("layout"))
def test_layouts(cuda, name):
    _run(cuda, name)


@pytest.mark.parametrize("name", pc.group("span"))
def test_gray_span(cuda, name):
    _run(cuda, name)


@pytest.mark.parametrize("name", pc.group("chain", "letterbox"))
def test_chain_and_letterbox(cuda, name):
    from rvs_amd import _lib, kernels
    case, dv = _run(cuda, name)
    geo = pc.case_geo(case)
    if case.entry == "chain":
        route = kernels.preprocess_chain_route(pc.chain_desc(case), case.H, case.W, geo)
        assert pc.ROUTES[route] == case.expect_path.route
    if case.gate:
        return
    # the other routes to the same bytes: the eager calls, and for a chain the fused entry
    np.testing.assert_array_equal(dv.proc, _eager(case, dv.x))
    two_pass = kernels.letterbox(kernels.clahe_median(dv.x, case.tiles, case.clip, case.k), geo)
    np.testing.assert_array_equal(two_pass.cpu().numpy(), dv.lb)
    fits = kernels.clahe_median_letterbox_fits(case.H, case.W, case.tiles, case.k, geo)
    assert fits == pc.LETTERBOX[(case.H, case.W)][0]
    if case.entry == "chain" and fits:
        proc, lb = kernels.clahe_median_letterbox(dv.x, case.tiles, case.clip, case.k, geo)
        np.testing.assert_array_equal(proc.cpu().numpy(), dv.proc)
        np.testing.assert_array_equal(lb.cpu().numpy(), dv.lb)
    elif case.entry == "chain":
        with pytest.raises(_lib.RVError, match="-1000"):
            kernels.clahe_median_letterbox(dv.x, case.tiles, case.clip, case.k, geo)


def test_gated_fused_batch_and_its_frames_alone(cuda):
    """The gated fused batch, and every frame of it alone."""
    from rvs_amd import kernels
    gated = [c for c in pc.cases().values() if c.group == "chain" and c.imgsz == pc.LB_IMGSZ]
    assert len(gated) == 1
    case = gated[0]
    dv = pc.device_run(case, cuda)
    pc.compare(case, dv)
    ans = pc.oracle(case.name)
    for b in range(case.B):   # a frame alone: its blocks are then slots 0, 1, .. of the grid
        proc, lb = kernels.preprocess_chain(dv.x[b:b + 1].contiguous(), pc.chain_desc(case),
                                            pc.case_geo(case))
        np.testing.assert_array_equal(proc.cpu().numpy()[0], ans.proc[b])
        np.testing.assert_array_equal(lb.cpu().numpy()[0], ans.lb[b])


def test_refused_geometries(cuda):
    """rv_clahe_median_u8 answers RV_EINVAL where neither fused pass holds
    the grid (the CLAHE cases without a clahe_median row), and writes nothing."""
    import torch
    from rvs_amd import _lib, kernels
    for H, W, tiles in [(32, 32, 8), (64, 128, 64), (3, 5, 8), (1, 1, 8)]:
        x = torch.from_numpy(pc.make_frame(("noise", 11), H, W).copy()).to(cuda)[None]
        out = torch.full_like(x, 9)
        assert not kernels.clahe_median_fits(x, tiles, 3)
        with pytest.raises(_lib.RVError, match="-1000"):
            kernels.clahe_median(x, tiles, 2.0, 3, out=out)
        assert bool((out == 9).all())


def test_argument_contract(cuda):
    """RV_EINVAL (-1000) for what the entries refuse, success for B = 0;
    nothing is launched either way: the output keeps its fill."""
    import torch
    from rvs_amd import _lib
    from rvs_amd._lib import ptr
    lib = _lib.load()
    H, W, B, EINVAL = 8, 12, 2, -1000
    x = torch.from_numpy(np.stack([pc.make_frame(("noise", s), H, W) for s in (1, 2)])).to(cuda)
    out = torch.full_like(x, 9)
    need = int(lib.rv_clahe_ws_bytes(B, 2))
    assert need == B * 4 * 256
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    lb = torch.full((B, 32, 32, 3), 9, dtype=torch.uint8, device=cuda)
    geo = (ctypes.c_int * 6)(32, 32, H, W, 12, 10)
    assert lib.rv_clahe_median_letterbox_fits(H, W, 2, 3, geo) == 1
    P, O, WS, p = ptr(x), ptr(out), ptr(ws), 3 * W

    def clahe(fn):
        return lambda i=P, o=O, b=B, pitch=p, tiles=2, w=WS, wb=need: \
            fn(i, o, b, H, W, pitch, tiles, 2.0, w, wb, None)

    def clahe_k(i=P, o=O, b=B, pitch=p, tiles=2, w=WS, wb=need, k=3):
        return lib.rv_clahe_median_u8(i, o, b, H, W, pitch, tiles, 2.0, k, w, wb, None)

    def clahe_lb(i=P, o=O, b=B, pitch=p, tiles=2, w=WS, wb=need, k=3, lbo=None, g=geo):
        return lib.rv_clahe_median_letterbox_u8(i, o, b, H, W, pitch, tiles, 2.0, k, w, wb,
                                                ptr(lb) if lbo is None else lbo, g, None)

    for f in (clahe(lib.rv_clahe_ycrcb_u8), clahe(lib.rv_clahe_lab_u8), clahe_k, clahe_lb):
        assert f(tiles=0) == EINVAL and f(tiles=65) == EINVAL
        assert f(o=P) == EINVAL                    # in == out
        assert f(pitch=p - 1) == EINVAL            # pitch < 3 W
        assert f(wb=need - 1) == EINVAL            # a workspace one byte short
        assert f(w=None) == EINVAL
        assert f(i=None) == EINVAL and f(o=None) == EINVAL
        assert f(b=-1) == EINVAL
        assert f(b=0) == 0
    assert clahe_k(k=4) == EINVAL and clahe_lb(k=4) == EINVAL and clahe_lb(k=5) == EINVAL
    assert clahe_lb(lbo=0) == EINVAL and clahe_lb(g=None) == EINVAL

    def median(i=P, o=O, b=B, pitch=p, k=3):
        return lib.rv_median_u8c3(i, o, b, H, W, pitch, k, None)
    for k in (4, 1, 11, 0):
        assert median(k=k) == EINVAL
    assert median(o=P) == EINVAL and median(pitch=p - 1) == EINVAL and median(i=None) == EINVAL
    assert median(b=0) == 0

    span = torch.full((B,), -5, dtype=torch.int32, device=cuda)
    sws = torch.zeros(2 * B, dtype=torch.int32, device=cuda)

    def gspan(i=P, b=B, pitch=p, w=None, s=None):
        return lib.rv_gray_span_u8(i, b, H, W, pitch, ptr(sws) if w is None else w,
                                   ptr(span) if s is None else s, None)
    assert gspan(i=None) == EINVAL and gspan(w=0) == EINVAL and gspan(s=0) == EINVAL
    assert gspan(pitch=p - 1) == EINVAL and gspan(b=-1) == EINVAL and gspan(b=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((lb == 9).all()) and bool((span == -5).all())
    # ... and the same calls with nothing wrong run
    assert clahe_lb() == 0 and median() == 0 and gspan() == 0
    torch.cuda.synchronize()

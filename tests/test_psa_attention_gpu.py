"""rv_psa_attention_bf16 (csrc/attn.hip: the multi-head self-attention of
YOLO11's PSA block) against a float64 softmax attention on the device's own
bf16 qkv.  Every element of every head of every image is checked.

Bar: |got - ref| <= 2^-7 A with A = sum_j P_ij |v_jd| in float64.  The bf16
rounding of P in the numerator contributes at most 2^-9 A, the normalisation
2^-9 A, the output's rounding to bf16 2^-9 A, and the f32 score and exp error
less than half of one of those: 2^-7 is 4/3 of that worst case.  In the two
extreme-score cases (|score| up to 200) the f32 error of a score grows with
|score| and is amplified by exp, so their bar is 2^-6 A.

The crafted cases force the branches bounded random data never takes: a key
whose score towers over the running maximum in the second key tile and again
in the last, partial tile (the online rescale), the maximum in the first tile
(later tiles scaled by ~0), scores near +-200 (overflow or 0/0 without the max
subtraction), all-equal scores (the mean of v) and v = 0 (exactly 0).  Every
qkv channel outside the view and every row past B * N holds NaN; the output
view is framed by canaries.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RV_EINVAL = -1000
QKV_CO, OUT_CO, PAD_C, PAD_ROWS = 8, 16, 8, 3
TILE = 32  # keys per tile of the kernel (csrc/attn.hip)


@pytest.fixture(scope="module")
def lib(cuda):
    from rvs_amd import _lib
    return _lib.load()


def cases(rng, B, N, heads):
    """name -> (q, k, v) of shape (B, N, heads, 32 / 32 / 64), and the bar's exponent."""
    def g(d, s=1.0):
        return rng.normal(0, s, (B, N, heads, d))

    out = {"gaussian": (g(32), g(32), g(64), -7)}
    # every query has q[0] = 3, so a key with k[0] = t scores 0.53 t above the rest
    q, k = g(32), g(32)
    q[..., 0] = 3.0
    j2 = min(TILE + 3, N - 1)  # in the second tile when there is one
    k[:, j2, :, 0] = 48.0      # + 25.5
    k[:, N - 1, :, 0] = 96.0   # the last (partial) tile: + 50.9
    out["max jumps in tile 2 and in the last tile"] = (q, k, g(64), -7)
    q, k = g(32), g(32)
    q[..., 0] = 3.0
    k[:, 0, :, 0] = 56.0  # + 29.7 in the first tile: every later tile is far below
    k[:, min(1, N - 1), :, 0] = 55.0
    out["max in the first tile"] = (q, k, g(64), -7)
    # |score| ~ 6 * 5.875 * 32 * 32^-1/2 = 199.4
    sgn = rng.choice([-1.0, 1.0], (B, N, heads, 1))
    q = np.full((B, N, heads, 32), 6.0)
    out["scores near +200 and -200"] = (q, sgn * 5.875 + g(32, 0.0625), g(64), -6)
    out["scores near -200"] = (q, -5.875 + g(32, 0.0625), g(64), -6)
    out["all scores equal"] = (np.zeros((B, N, heads, 32)), g(32), g(64), -7)
    out["v = 0"] = (g(32), g(32), np.zeros((B, N, heads, 64)), -7)
    return out


def run(lib, cuda, q, k, v):
    """The kernel on a wide qkv tensor (NaN outside the view) -> the wide
    output (canaries outside the view) and the bf16 qkv as float64."""
    from rvs_amd import _lib
    B, N, heads = q.shape[:3]
    cs = QKV_CO + 128 * heads + PAD_C
    wide = np.full((B * N + PAD_ROWS, cs), np.nan, np.float32)
    wide[:B * N, QKV_CO:QKV_CO + 128 * heads] = np.concatenate([q, k, v], -1).reshape(B * N, -1)
    qkv = torch.from_numpy(wide).to(cuda).to(torch.bfloat16)
    ocs = OUT_CO + 64 * heads + PAD_C
    out = torch.full((B * N + PAD_ROWS, ocs), 7.0, dtype=torch.bfloat16, device=cuda)
    st = lib.rv_psa_attention_bf16(qkv.data_ptr(), B, N, heads, cs, QKV_CO, out.data_ptr(), ocs,
                                   OUT_CO, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    dev = qkv.float().cpu().numpy().astype(np.float64)[:B * N, QKV_CO:QKV_CO + 128 * heads]
    return out.float().cpu().numpy().astype(np.float64), dev.reshape(B, N, heads, 128)


def check(lib, cuda, name, q, k, v, exp):
    B, N, heads = q.shape[:3]
    o, dev = run(lib, cuda, q, k, v)
    np.testing.assert_array_equal(o[B * N:], 7.0, err_msg=f"{name}: rows past B * N written")
    np.testing.assert_array_equal(o[:, :OUT_CO], 7.0, err_msg=f"{name}: channels below the view")
    np.testing.assert_array_equal(o[:, OUT_CO + 64 * heads:], 7.0,
                                  err_msg=f"{name}: channels above the view")
    got = o[:B * N, OUT_CO:OUT_CO + 64 * heads].reshape(B, N, heads, 64)
    assert np.isfinite(got).all(), f"{name}: non-finite output (NaN read from outside the view?)"
    qd, kd, vd = dev[..., :32], dev[..., 32:64], dev[..., 64:]
    S = np.einsum("bihc,bjhc->bhij", qd, kd) * 32.0 ** -0.5
    P = np.exp(S - S.max(-1, keepdims=True))
    P /= P.sum(-1, keepdims=True)
    ref = np.einsum("bhij,bjhd->bihd", P, vd)
    A = np.einsum("bhij,bjhd->bihd", P, np.abs(vd))
    d = np.abs(got - ref)
    tol = 2.0 ** exp * A
    ratio = float((d / np.maximum(tol, 1e-300)).max()) if (tol > 0).any() else 0.0
    print(f"N={N} heads={heads} {name}: worst |d| / (2^{exp} A) = {ratio:.3f}")
    bad = d > tol
    assert not bad.any(), (f"{name}, N={N}: {int(bad.sum())} of {bad.size} beyond 2^{exp} A, worst "
                           f"{ratio:.2f} x the bar at (b, i, h, d) = {np.argwhere(bad)[0].tolist()}")
    return got, ref, vd


@pytest.mark.parametrize("N,heads", [(1, 2), (6, 2), (35, 2), (63, 2), (64, 2), (65, 2), (130, 2),
                                     (400, 2), (80, 6)])
def test_attention_matches_float64(lib, cuda, N, heads):
    rng = np.random.default_rng(100 * N + heads)
    for name, (q, k, v, exp) in cases(rng, 2, N, heads).items():
        got, ref, vd = check(lib, cuda, name, q, k, v, exp)
        if name == "v = 0":
            assert (got == 0).all()
        if name == "all scores equal":  # the mean of v, to the output's rounding
            mean = np.broadcast_to(vd.mean(1, keepdims=True), got.shape)
            assert (np.abs(got - mean) <= 2.0 ** -8 * np.abs(mean) + 1e-6).all()


def test_rescale_cases_force_the_branch():
    """The crafted spikes do what their names say, on the reference side:
    the running maximum of some query row rises by more than 8 in the second
    key tile and again in the last one (N = 130: tiles of 32)."""
    rng = np.random.default_rng(0)
    q, k, v, _ = cases(rng, 1, 130, 2)["max jumps in tile 2 and in the last tile"]
    S = np.einsum("bihc,bjhc->bhij", q, k) * 32.0 ** -0.5
    run_max = np.maximum.accumulate(S, -1)
    t1, t2, tl = run_max[..., TILE - 1], run_max[..., 2 * TILE - 1], run_max[..., -1]
    before_last = run_max[..., (130 - 1) // TILE * TILE - 1]
    assert ((t2 - t1) > 8).all() and ((tl - before_last) > 8).all()
    q, k, v, _ = cases(rng, 1, 130, 2)["max in the first tile"]
    S = np.einsum("bihc,bjhc->bhij", q, k) * 32.0 ** -0.5
    assert (S[..., :TILE].max(-1) - S[..., TILE:].max(-1) > 15).all()


def test_argument_contract(lib, cuda):
    from rvs_amd import _lib
    B, N, heads = 1, 8, 2
    qkv = torch.zeros((B * N, 256), dtype=torch.bfloat16, device=cuda)
    out = torch.full((B * N, 128), 7.0, dtype=torch.bfloat16, device=cuda)
    Q, O, s = qkv.data_ptr(), out.data_ptr(), _lib.stream_ptr()
    good = [Q, B, N, heads, 256, 0, O, 128, 0, s]
    assert lib.rv_psa_attention_bf16(*good) == 0
    torch.cuda.synchronize()
    assert (out.float() == 0).all()
    out.fill_(7.0)
    bad = {"null qkv": {0: 0}, "null out": {6: 0}, "B 0": {1: 0}, "N 0": {2: 0}, "heads 0": {3: 0},
           "heads past qkv_cs": {3: 3}, "qkv_co past": {5: 8}, "qkv_cs 12": {4: 252},
           "qkv_co 4": {4: 264, 5: 4}, "qkv_co < 0": {5: -8}, "qkv misaligned": {0: Q + 8},
           "out_cs short": {7: 120}, "out_co past": {8: 4}, "out_cs 2": {7: 130},
           "out_co 2": {7: 132, 8: 2}, "out misaligned": {6: O + 4}, "out_co < 0": {8: -4}}
    for what, ch in bad.items():
        a = list(good)
        for i, v in ch.items():
            a[i] = v
        assert lib.rv_psa_attention_bf16(*a) == RV_EINVAL, what
    torch.cuda.synchronize()
    assert (out.float() == 7.0).all(), "a refused call wrote"

"""CPU proof of the first layer's arithmetic on the bf16 matrix pipe (csrc/conv1_bf16x3.hip): every fp32 operand is split into three
bf16 pieces (round to nearest even, subtract in fp32, repeat) and a product a*b is recovered by the six piece-products of order at most
2^-16 -- a1b1, a1b2, a2b1, a1b3, a2b2, a3b1 -- accumulated in fp32.  The emulation below follows the kernel's order: K runs filter row
by filter row, 192 per row (1 lead dummy + 7*27 + 2 padding lanes, zero weights), in groups of 16; per group the six products go
smallest first into the fp32 accumulator.  The yardstick is the fp64 product; the bound is twice the worst error of a plain fp32
accumulation of the same data in the fp32 MFMA's order (two k per step).

Ranges.  bf16 has fp32's exponent range, so the pieces of any finite fp32 value are finite EXCEPT within half a bf16 ulp of the top
(|x| > 3.3961775e38 rounds to infinity); such inputs give NaN, like an infinity.  The kernel's inputs are image data in [0, 1].  At the
bottom, bf16 denormals are multiples of 2^-133 where fp32's are multiples of 2^-149: below 2^-110 or so the three pieces no longer
sum to x exactly and the split loses up to 2^-134 per element, absolutely -- nothing next to max|y|."""
import numpy as np
import torch

EPS = 1.1920929e-07
KH, KW, CIN, COUT, SEGP, LEAD = 7, 7, 27, 64, 192, 1


def split3(x):
    """fp32 tensor -> its three bf16 pieces, as fp32 tensors"""
    x = x.float()
    h = x.bfloat16().float()
    r1 = x - h
    m = r1.bfloat16().float()
    r2 = r1 - m
    l = r2.bfloat16().float()
    return h, m, l


def rows_k_layout(a, w):
    """a [M][7][189], w [7][189][N] -> the kernel's K order [M][7*192], [7*192][N] with the lead dummy and the padding lanes (zeros)"""
    M, N = a.shape[0], w.shape[2]
    ap = torch.zeros(M, KH, SEGP, dtype=a.dtype)
    wp = torch.zeros(KH, SEGP, N, dtype=w.dtype)
    ap[:, :, LEAD:LEAD + KW * CIN] = a
    wp[:, LEAD:LEAD + KW * CIN, :] = w
    return ap.reshape(M, KH * SEGP), wp.reshape(KH * SEGP, N)


def dot_bf16x3(a, w, products=6):
    """the emulation: a [M][K], w [K][N] fp32, K a multiple of 16.  Per K-group every piece-product is a 16-term fp32 sum of exact
    products (bf16 x bf16 fits fp32), added to the fp32 accumulator; smallest products first."""
    A, W = split3(a), split3(w)
    order = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]
    if products == 9:
        order = [(2, 2), (2, 1), (1, 2)] + order
    acc = torch.zeros(a.shape[0], w.shape[1], dtype=torch.float32)
    for g in range(0, a.shape[1], 16):
        for pa, pb in order:
            acc = acc + A[pa][:, g:g + 16] @ W[pb][g:g + 16, :]
    return acc


def dot_fp32(a, w):
    """plain fp32 accumulation in the fp32 MFMA's order: two k per step into the fp32 accumulator"""
    acc = torch.zeros(a.shape[0], w.shape[1], dtype=torch.float32)
    for k in range(0, a.shape[1], 2):
        acc = acc + (a[:, k:k + 1] * w[k:k + 1, :] + a[:, k + 1:k + 2] * w[k + 1:k + 2, :])
    return acc


def err_eps(y, ref):
    return float((y.double() - ref).abs().max() / (EPS * ref.abs().max()))


def conv1_like(seed, M=512, scale_spread=False):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(M, KH, KW * CIN, generator=g)                                   # image data
    w = torch.randn(KH, KW * CIN, COUT, generator=g) * (2.0 / (KH * KW * CIN)) ** 0.5   # variance scaling, fan-in
    if scale_spread:                                                               # folded BatchNorm scales of several magnitudes
        w = w * torch.exp(torch.randn(COUT, generator=g) * 1.5)
    return rows_k_layout(a, w)


def test_split_is_exact_and_pieces_are_bf16():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g), torch.rand(4096, generator=g), torch.randn(4096, generator=g) * 1e30,
                   torch.randn(4096, generator=g) * 1e-30, torch.tensor([0.0, -0.0, 1.0, 3.3895314e38, -3.3895314e38, 1.17549435e-38])])
    h, m, l = split3(x)
    for p in (h, m, l):
        assert torch.isfinite(p).all() and torch.equal(p.bfloat16().float(), p)
    assert torch.equal((h.double() + m.double() + l.double()), x.double())         # 8 + 8 + 8 significand bits cover fp32's 24
    assert float((m.abs() / h.abs().clamp_min(1e-45)).max()) <= 2.0 ** -8 and float((l.abs() / h.abs().clamp_min(1e-45)).max()) <= 2.0 ** -16


def test_denormal_inputs_lose_at_most_a_bf16_denormal_step():
    x = torch.tensor([1e-40, -3e-41, 7e-39, 1.4e-45, 2e-38])
    h, m, l = split3(x)
    assert torch.isfinite(h + m + l).all()
    assert float(((h.double() + m.double() + l.double()) - x.double()).abs().max()) <= 2.0 ** -134


def test_top_of_the_range_rounds_to_infinity_and_gives_nan():
    x = torch.tensor([3.4e38])                   # above bf16's largest finite value by more than half an ulp
    h, m, l = split3(x)                          # inf, x - inf = -inf, -inf + inf = NaN: the output is NaN
    assert torch.isinf(h).all() and torch.isinf(m).all() and torch.isnan(l).all()


def test_six_products_within_twice_the_fp32_form():
    for seed, spread in [(1, False), (2, True), (3, True)]:
        a, w = conv1_like(seed, scale_spread=spread)
        ref = a.double() @ w.double()
        e6, e32 = err_eps(dot_bf16x3(a, w), ref), err_eps(dot_fp32(a, w), ref)
        print(f"seed {seed}: six bf16 piece-products {e6:.2f} eps of max|y|, fp32 form {e32:.2f}, nine {err_eps(dot_bf16x3(a, w, 9), ref):.2f}")
        assert e6 <= 2.0 * e32, (seed, e6, e32)


def test_scaled_inputs_keep_the_bound():
    # huge and tiny operands: the pieces stay in range (bf16 shares fp32's exponent range), the relative error does not move
    for sa, sw in [(1e30, 1e-6), (1e-30, 1.0), (1e18, 1e18)]:
        a, w = conv1_like(4)
        a, w = a * sa, w * sw
        ref = a.double() @ w.double()
        y = dot_bf16x3(a, w)
        assert torch.isfinite(y).all()
        assert err_eps(y, ref) <= 2.0 * err_eps(dot_fp32(a, w), ref)


def test_nan_and_inf_propagate_like_the_fp32_form():
    a, w = conv1_like(5, M=64)
    a[3, 200] = float("nan")
    a[7, 5 * SEGP + 17] = float("inf")
    a[9, 3 * SEGP + 40] = float("-inf")
    y, y32 = dot_bf16x3(a, w), dot_fp32(a, w)
    assert torch.isnan(y[3]).all() and torch.isnan(y32[3]).all()                   # a NaN anywhere in the receptive field: NaN out
    # an infinity: its middle piece is inf - inf = NaN, so the row is NaN; the fp32 form gives +-inf (or NaN against a zero weight).
    # Non-finite either way, never finite garbage
    assert torch.isnan(y[7]).all() and torch.isnan(y[9]).all()
    assert not torch.isfinite(y32[7]).any() and not torch.isfinite(y32[9]).any()
    rest = [i for i in range(64) if i not in (3, 7, 9)]
    assert torch.isfinite(y[rest]).all()

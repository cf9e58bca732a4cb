"""What tests/test_gpu_pow2_scaling.py and tests/test_gpu_thin_operand_range.py assume about the operands of tests/_operands.py, proved on
the CPU with a torch.bfloat16 emulation of the three-piece split (csrc/fdn_common.h: fdn_split3) and of the six-term product sum of the
fp32-storage head forward (csrc/heads_mfma.hip: mfma_step).  No GPU and nothing from the package.

Bounds, all relative to |x w| of one product of two pieces3 values x = h + m + l, w = h' + m' + l' (2^e <= |h| < 2^(e+1), 2^(e-9) < |m| < 2^(e-8),
2^(e-18) <= |l| < 2^(e-17), and |x| > 2^e because h is no power of two):
  * the three dropped terms m l', l m', l l' are below 2^-8 2^-17 each way and 2^-34: 2 * 2^-25 + 2^-34; the last fp32 addition rounds by at most
    2^-24, the five before it act on partial sums below 2^-8 |x w|: 2^-32 each.  Total < 2^-22, asserted.
  * a kept term is at least m m' > (129/128)^2 2^-20 (|m| >= (129/128) 2^(e-9), |x| < 2^(e+1)); h l' and l h' are at least about 2^-19, m h' and
    h m' 2^-10.  So leaving any ONE of the six out moves the sum by more than 2^-20 -- asserted per element -- which a probe bound of 2^-21 on top
    of an error below 2^-22 cannot absorb.  (2^-19 holds for five of the six terms on all but a few values and for m m' only where b b' is large:
    the test prints the smallest movement of each term.)
Range of the scaling tests: a bounded operand has 2^-6 <= |v| < 2^7; scaled by 2^a, |a| <= 40, its smallest non-zero piece is one unit in the last
place, 2^(-6 - 23 + a).  The smallest of the six kept products, mid x mid of two values whose residuals are a single last-place bit, is
2^(-29 + a) 2^(-29 + b) >= 2^-118 for a + b >= -60: a normal fp32 number (>= 2^-126), asserted on the drawn operands, so no
product is rounded or flushed; 1728 products below 2^14 2^60 stay below 2^100."""
import math

import pytest
import torch

import _operands as P

F64 = torch.float64
N = 20000


def _log2(v):
    return math.log2(float(v)) if float(v) > 0 else -math.inf


@pytest.fixture(scope="module")
def xw():
    g = P.gen(11)
    return P.pieces3(g, (N,)), P.pieces3(g, (N,))


@pytest.mark.parametrize("recipe", ["pieces3", "pieces2", "pieces1"])
def test_split3_returns_the_pieces_the_values_were_built_from(recipe):
    v, (h, m, l) = getattr(P, recipe)(P.gen(3), (N,))
    hi, mid, lo = P.split3(v)
    assert torch.equal(hi, h) and torch.equal(mid, m) and torch.equal(lo, l)
    assert bool((h != 0).all())
    if recipe != "pieces1":
        assert bool((m.abs() > torch.exp2(torch.floor(torch.log2(h.abs())) - 9)).all())         # more than half of its largest size 2^(e-8)
    if recipe == "pieces3":
        assert bool((l.abs() >= torch.exp2(torch.floor(torch.log2(h.abs())) - 18)).all())
    if recipe == "pieces1":
        assert torch.equal(v.to(torch.bfloat16).to(torch.float32), v)                         # bf16-exact


def _all_recipes():
    g = P.gen(5)
    out = {"bounded": P.bounded(g, (N,)), "skewed": P.skewed(g, (N // 50, 50), 1)}
    for kind in P.WIDE_KINDS:
        out["wide:" + kind] = P.wide(g, kind, (N,))
    for r in ("pieces3", "pieces2", "pieces1"):
        out[r] = getattr(P, r)(g, (N,))[0]
    for a, b in P.SCALE_PAIRS:
        out["bounded * 2^%d" % a] = P.pow2(out["bounded"], a)
        out["bounded * 2^%d" % b] = P.pow2(out["bounded"], b)
    return out


def test_split3_is_exact_on_every_recipe():
    for name, v in _all_recipes().items():
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all()), name
        hi, mid, lo = P.split3(v)
        assert torch.equal(hi.to(F64) + mid.to(F64) + lo.to(F64), v.to(F64)), name


def test_recipes_have_the_stated_ranges():
    g = P.gen(6)
    b = P.bounded(g, (N,)).abs()
    assert float(b.min()) >= 2.0 ** -6 and float(b.max()) < 2.0 ** 7
    assert len(torch.unique(torch.floor(torch.log2(b)))) == 13                                 # every exponent -6 .. 6 drawn
    lu = P.wide(g, "loguniform", (N,)).abs()
    assert 1e-6 * (1 - 1e-6) <= float(lu.min()) and float(lu.max()) <= 1.0 and float(lu.min()) < 1e-5
    for m in (0, 10, 100):
        o = P.wide(g, "offset%d" % m, (N,))
        assert float(o.min()) >= 0.7 * m * (1 - 1e-6) and abs(float(o.mean()) - 0.7 * (m + math.sqrt(2 / math.pi))) < 0.02
    k = P.wide(g, "kernel", (N,))
    assert abs(float(k.mean()) - 0.015) < 1e-3 and abs(float(k.std()) - 0.03) < 1e-3
    s = P.skewed(g, (400, 64), 1)
    ratio = s.abs().amax(dim=0)
    assert float(ratio.max() / ratio.min()) >= 2.0 ** 16                                       # quiet and loud channels side by side
    # same generator state -> same operands (the GPU tests regenerate instead of keeping tensors)
    assert torch.equal(P.bounded(P.gen(9), (64,)), P.bounded(P.gen(9), (64,)))


def test_six_terms_reproduce_the_product_to_2_to_the_minus_22(xw):
    (x, _), (w, _) = xw
    ref = x.to(F64) * w.to(F64)
    err = ((P.six_term_products(x, w).to(F64) - ref).abs() / ref.abs()).max()
    print("\n  [recipes] six-term product sum: worst error 2^%.2f of |x w|" % _log2(err))
    assert float(err) <= 2.0 ** -22


@pytest.mark.parametrize("drop", range(6))
def test_leaving_out_any_one_term_moves_the_sum(xw, drop):
    (x, _), (w, _) = xw
    ref = (x.to(F64) * w.to(F64)).abs()
    full = P.six_term_products(x, w).to(F64)
    moved = (P.six_term_products(x, w, drop=drop).to(F64) - full).abs() / ref
    print("\n  [recipes] without term %s (piece of x, piece of w): moves by 2^%.2f .. 2^%.2f of |x w|, %.1f %% of the products by 2^-19 or more"
          % (P.SIX_TERMS[drop], _log2(moved.min()), _log2(moved.max()), 100.0 * float((moved >= 2.0 ** -19).double().mean())))
    assert float(moved.min()) > 2.0 ** -20
    err = ((P.six_term_products(x, w, drop=drop).to(F64) - x.to(F64) * w.to(F64)).abs() / ref).min()
    assert float(err) > 2.0 ** -21, "a five-term sum would pass the probe's 2^-21"


@pytest.fixture(scope="module")
def gemm():
    g = P.gen(21)
    x, w = P.bounded(g, (48, 64)), P.bounded(g, (27, 64))
    return x, w, P.six_term_gemm(x, w)


@pytest.mark.parametrize("a,b", P.SCALE_PAIRS)
def test_six_term_gemm_commutes_with_power_of_two_scaling_bit_for_bit(gemm, a, b):
    """K = 64 channels, 27 taps, fp32 accumulation in the kernel's term order."""
    x, w, base = gemm
    got = P.six_term_gemm(P.pow2(x, a), P.pow2(w, b))
    assert torch.equal(got, P.pow2(base, a + b))
    assert bool(torch.isfinite(got).all()) and bool((got != 0).all())


@pytest.mark.parametrize("a,b", P.SCALE_PAIRS)
def test_scaled_bounded_products_stay_normal_fp32_numbers(gemm, a, b):
    x, w, base = gemm
    xs, ws = P.split3(P.pow2(x, a)), P.split3(P.pow2(w, b))
    smallest = math.inf
    for p, q in P.SIX_TERMS:
        prod = (xs[p].to(F64)[:, None, :] * ws[q].to(F64)[None, :, :]).abs()
        smallest = min(smallest, float(prod[prod > 0].min()))
    total = 27.0 * float(P.pow2(base.abs().max(), a + b))                                      # 27 taps of the largest |z|
    print("\n  [recipes] scales 2^%d, 2^%d: smallest non-zero kept product 2^%.1f, largest sum below 2^%.1f" % (a, b, _log2(smallest), _log2(total)))
    assert smallest >= 2.0 ** -118 and total <= 2.0 ** 100
    assert abs(a + b) <= 60 and max(abs(a), abs(b)) <= 40

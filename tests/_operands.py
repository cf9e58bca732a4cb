"""Operand recipes of the operand-range tests, in plain torch (nothing from the package) on whatever device the generator lives on.

Four kinds, each a pure function of a torch.Generator:

    bounded(g, shape)        random sign, magnitude 2^e (1 + m / 2^23) with integer e uniform in -6 .. 6 and a full 23-bit mantissa m: every
                             value has 2^-6 <= |v| < 2^7, none is zero or near zero.  The operands of tests/test_gpu_pow2_scaling.py.
    wide(g, kind, shape)     the recipes of DESIGN.md section 5.6 (a): "offset0" / "offset10" / "offset100" = |N(0,1)| s + m with s = 0.7 and
                             m / s = 0, 10, 100; "loguniform" = random sign times 10^(-6 U(0,1)); "kernel" = N(0, 0.03) + 0.015.
    skewed(g, shape, dim)    N(0,1) times 2^k per index of `dim`, integer k uniform in -12 .. 12 (a trained layer's quiet and loud channels).
    pieces3 / pieces2 / pieces1(g, shape)
                             fp32 values built as h + m + l: h = (128 + a) 2^(e-7) (8 significant bits at exponent e, e uniform in -3 .. 3),
                             |m| = (1 + b / 128) 2^(e-9), |l| = (1 + c / 32) 2^(e-18), independent signs.  l ends at bit 2^(e-23), the last place
                             of an fp32 number in [2^e, 2^(e+1)): 24 significant bits, every piece non-zero and at least half of its largest
                             size.  a and b are drawn from 1 .. 127: were h (or m) a power of two, a piece of the other sign would pull the sum
                             into the binade below, where round-to-nearest picks another h.  pieces2 has l = 0, pieces1 (bf16-exact) h alone.
                             Returned as (value, (h, m, l)).

split3 / six_term_products / six_term_gemm emulate the three-piece bf16 arithmetic of csrc/fdn_common.h (fdn_split3) and of the fp32-storage
head forward (csrc/heads_mfma.hip, mfma_step) with torch.bfloat16 roundings and fp32 accumulation: tests/test_operand_recipes.py uses them to
prove on the CPU what the GPU tests assume about these operands."""
import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
WIDE_KINDS = ("offset0", "offset10", "offset100", "loguniform", "kernel")
# scale pairs (a, b) of tests/test_gpu_pow2_scaling.py: the first operand times 2^a, the second times 2^b, |a + b| <= 60
SCALE_PAIRS = ((-40, -20), (40, 20), (-30, 30))
# the six kept cross terms (piece of x, piece of w) in the order mfma_step issues them: small terms first
SIX_TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


def gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


def _randint(g, lo, hi, shape):
    """Integers uniform in lo .. hi - 1, as float64."""
    return torch.randint(lo, hi, tuple(shape), generator=g, device=g.device).to(F64)


def _sign(g, shape):
    return _randint(g, 0, 2, shape) * 2.0 - 1.0


def pow2(t, k):
    """t * 2^k, exact while nothing leaves the normal range (the caller's contract); keeps dtype.  (A multiplication by the scalar 2.0^k, which
    fp32 and bf16 hold exactly for |k| <= 126; not ldexp, whose 2^k some backends form with pow.)"""
    return t * (2.0 ** k)


def bounded(g, shape):
    e = _randint(g, -6, 7, shape)
    m = _randint(g, 0, 1 << 23, shape)
    v = _sign(g, shape) * torch.exp2(e) * (1.0 + m / float(1 << 23))
    out = v.to(F32)
    assert torch.equal(out.to(F64), v)
    return out


def wide(g, kind, shape):
    dev = g.device
    if kind.startswith("offset"):
        s = 0.7
        return torch.randn(tuple(shape), generator=g, device=dev).abs() * s + float(kind[6:]) * s
    if kind == "loguniform":
        mag = 10.0 ** (-6.0 * torch.rand(tuple(shape), generator=g, device=dev))
        return mag * _sign(g, shape).to(F32)
    if kind == "kernel":
        return torch.randn(tuple(shape), generator=g, device=dev) * 0.03 + 0.015
    raise ValueError(kind)


def skew_exponents(g, n):
    return _randint(g, -12, 13, (n,))


def skewed(g, shape, dim):
    shape = tuple(shape)
    k = skew_exponents(g, shape[dim])
    view = [1] * len(shape)
    view[dim] = shape[dim]
    return torch.randn(shape, generator=g, device=g.device) * torch.exp2(k).to(F32).reshape(view)


def _pieces(g, shape, n):
    e = _randint(g, -3, 4, shape)
    h = _sign(g, shape) * (128.0 + _randint(g, 1, 128, shape)) * torch.exp2(e - 7)
    m = _sign(g, shape) * (1.0 + _randint(g, 1, 128, shape) / 128.0) * torch.exp2(e - 9)
    l = _sign(g, shape) * (1.0 + _randint(g, 0, 32, shape) / 32.0) * torch.exp2(e - 18)
    if n < 3:
        l = torch.zeros_like(l)
    if n < 2:
        m = torch.zeros_like(m)
    v = h + m + l
    out = v.to(F32)
    assert torch.equal(out.to(F64), v)              # 24 significant bits: the sum is an fp32 number
    return out, (h.to(F32), m.to(F32), l.to(F32))


def pieces3(g, shape):
    return _pieces(g, shape, 3)


def pieces2(g, shape):
    return _pieces(g, shape, 2)


def pieces1(g, shape):
    return _pieces(g, shape, 1)


def split3(v):
    """fdn_split3: (hi, mid, lo), each the round-to-nearest-even bf16 of what the pieces before it leave, as fp32 tensors."""
    assert v.dtype == F32
    hi = v.to(BF16).to(F32)
    r = v - hi
    mid = r.to(BF16).to(F32)
    lo = (r - mid).to(BF16).to(F32)
    return hi, mid, lo


def six_term_products(x, w, drop=None):
    """The six kept cross terms of x * w, each an exact bf16 x bf16 product, added in fp32 in the kernel's order; drop: index into SIX_TERMS
    of a term to leave out."""
    xs, ws = split3(x), split3(w)
    acc = torch.zeros(torch.broadcast_shapes(x.shape, w.shape), dtype=F32, device=x.device)
    for i, (p, q) in enumerate(SIX_TERMS):
        if i != drop:
            acc = acc + xs[p] * ws[q]               # (the product of two 8-bit significands is exact in fp32)
    return acc


def six_term_gemm(x, w, block=16):
    """z[v][t] = sum_c x[v][c] w[t][c] as the fp32-storage head forward forms it: channel blocks of `block` in order, inside a block the six
    terms in order, inside a term the channels in order, one fp32 addition per product.  x (V, K), w (T, K) -> (V, T) fp32."""
    xs, ws = split3(x), split3(w)
    V, K = x.shape
    acc = torch.zeros((V, w.shape[0]), dtype=F32, device=x.device)
    for c0 in range(0, K, block):
        for p, q in SIX_TERMS:
            for c in range(c0, min(c0 + block, K)):
                acc = acc + xs[p][:, c:c + 1] * ws[q][:, c].unsqueeze(0)
    return acc

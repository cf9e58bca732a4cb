"""Power-of-two scaling, bit for bit: a kernel's result may depend on nothing but its operands.

Every conv, fold and upsample kernel of the library is linear in its data (bilinear in data and weights), apart from a sign test.  For a
kernel f that is linear in each of two operands

    f(2^a u, 2^b v)  must  torch.equal  2^(a+b) f(u, v)                     -- every output, bias gradients and bf16-stored outputs included

because every step of the arithmetic commutes exactly with a power-of-two scaling while nothing under- or overflows:
  * an fp32 multiply, add or FMA rounds the significand; the exponent only shifts -- also inside the matrix instructions, and also for the
    Winograd transforms, whose constants multiply a scaled value;
  * round-to-nearest-even to bf16 (operand splits hi / mid / lo, packs, stored outputs) looks at the significand alone, so every piece of a
    scaled value is the scaled piece;
  * max(z, 0.2 z), ReLU and the sign masks test z > 0, which a positive scale keeps;
  * the reductions over voxels, workgroup partials and taps run in a fixed order, so the same roundings happen to the same partial sums.
A result that does NOT scale is mixing in something that did not scale with the operands: a stale workspace partial or padded-scratch cell
from the previous launch, a lane that was not predicated off, a small piece flushed to zero, a hidden absolute constant.  The tests that
normalise by max |ref| only see such junk when it is large.

Operands: tests/_operands.py `bounded` (2^-6 <= |v| < 2^7, full mantissas, no zeros); scale pairs (a, b) = (-40, -20), (+40, +20), (-30, +30),
|a + b| <= 60.  tests/test_operand_recipes.py proves on the CPU that under these pairs every product of two operand pieces stays a normal fp32
number and every sum stays below 2^100, and that an emulation of the six-term bf16 GEMM is bit-identical under them.  A bias is scaled by
2^(a+b); skip / residual operands scale like the output; y_prev / sign-mask operands are not scaled (only their signs are read).

Order: the unscaled case runs first and the scaled cases after it into the SAME output, scratch, pack and workspace tensors, each filled with
a finite sentinel before every launch: whatever a launch leaves unwritten, or picks up from the launch before, breaks the equality.

Grids: (2,6,6,6) one ragged tile; (1,5,7,9) W off the multiple-of-4 raster (direct strips); (1,10,12,16) and (2,12,10,24) several tiles with
shell regions on the F(4,3) x F(4,3) raster; (1,16,16,16) full 8 x 8 x 8 bf16 tiles."""
import contextlib
import importlib

import pytest
import torch

import _operands as P
from test_gpu_plan_coverage import sign_mask_words

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("4dflownet_amd._lib")
ops = importlib.import_module("4dflownet_amd.ops")
bops = importlib.import_module("4dflownet_amd.ops_bf16")

GRIDS = [(2, 6, 6, 6), (1, 5, 7, 9), (1, 10, 12, 16), (2, 12, 10, 24)]
BF_GRIDS = GRIDS + [(1, 16, 16, 16)]
DT_GRIDS = [("f32", d) for d in GRIDS] + [("bf16", d) for d in BF_GRIDS]
ALGOS = {"auto": ops.ALGO_AUTO, "direct": ops.ALGO_DIRECT, "wino_w": ops.ALGO_WINO_W, "bf16x3": ops.ALGO_WINO_BF16X3}
BF_VARIANTS = [0, 8, 20, 52]                        # tests/test_gpu_bf16.py: planner, forced MT 8, full-depth tiles, never the two-slice kernel
SENTINEL, SENTINEL_WORD = 1234.5, 0x5A5A
BF16 = torch.bfloat16
HOOK_DEFAULTS = {"heads_mfma": 1, "cin3_mfma": 1, "conv1x1_mfma": 1, "wgrad64_direct": 0, "wgrad64_bf16_variant": 0, "conv64_bf16_mt": 0,
                 "conv64_bf16_mode2": 1}


@contextlib.contextmanager
def hooks(**values):
    """Run on the product library (no values), or on the test build with fdn_debug_set_<name>(value), restored afterwards."""
    if not values:
        yield
        return
    with _lib.test_build() as lib:
        try:
            for name, v in values.items():
                getattr(lib, "fdn_debug_set_" + name)(v)
            yield
        finally:
            for name in values:
                getattr(lib, "fdn_debug_set_" + name)(HOOK_DEFAULTS[name])


def bf_variant(mt):
    return {} if mt == 0 else {"conv64_bf16_mt": mt & 31, "conv64_bf16_mode2": 0 if mt & 32 else 1}


def _o(dt):
    return bops if dt == "bf16" else ops


def _st(t, dt):
    """An activation operand in the storage type (the bf16 rounding of a bounded value is a bounded value up to |v| = 2^7)."""
    return t.to(BF16) if dt == "bf16" else t


def _b(g, *shape):
    return P.bounded(g, shape)


def _randn(g, *shape):
    return torch.randn(shape, generator=g, device="cuda")


def _empty(*shape, dtype=torch.float32):
    return torch.empty(shape, device="cuda", dtype=dtype)


def _scale(t, k):
    if t is None:
        return None
    if isinstance(t, (list, tuple)):
        return [_scale(e, k) for e in t]
    return P.pow2(t, k)


def _prefill(t):
    t.fill_(SENTINEL if t.is_floating_point() else SENTINEL_WORD)


def check_pow2(name, launch, u, v=None, like_out=(), bufs=()):
    """launch(u, v, *like_out) -> [(tensor, kind)], kind = which power the output carries: "ab", "a", "b" or "same".  u is scaled by 2^a,
    v by 2^b, every like_out operand by 2^(a+b); bufs are sentinel-filled before every launch."""
    def once(a, b):
        for t in bufs:
            _prefill(t)
        outs = launch(_scale(u, a), _scale(v, b), *[_scale(t, a + b) for t in like_out])
        torch.cuda.synchronize()
        return [(t.clone(), kind) for t, kind in outs]

    base = once(0, 0)
    for i, (t, kind) in enumerate(base):
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), "%s: output %d is not finite" % (name, i)
            assert bool((t != 0).any()), "%s: output %d is all zero" % (name, i)
    for a, b in P.SCALE_PAIRS:
        for i, ((t, kind), (t0, _)) in enumerate(zip(once(a, b), base)):
            k = {"ab": a + b, "a": a, "b": b, "same": 0}[kind]
            want = P.pow2(t0, k) if t0.is_floating_point() and k else t0
            if not torch.equal(t, want):
                bad = (t != want).reshape(-1)
                j = int(bad.nonzero()[0])
                raise AssertionError("%s: output %d under the scales (2^%d, 2^%d): %d of %d elements are not 2^%d times the unscaled result; "
                                     "flat index %d holds %r, expected %r" % (name, i, a, b, int(bad.sum()), bad.numel(), k, j,
                                                                             float(t.reshape(-1)[j]), float(want.reshape(-1)[j])))


def _seed(*parts):
    s = 17
    for p in parts:
        for q in (p if isinstance(p, (tuple, list)) else (p,)):
            s = (s * 1000003 + (sum(map(ord, q)) if isinstance(q, str) else int(q))) % (2 ** 31 - 1)
    return s


# ---------------------------------------------------------------------------------------------------------------- forward, 64 -> 64
@pytest.mark.parametrize("algo", sorted(ALGOS))
@pytest.mark.parametrize("dims", GRIDS)
def test_conv64_fwd_f32(fdn, dims, algo):
    N, D, H, W = dims
    g = P.gen(_seed(dims, algo, 1), "cuda")
    x, w, bias, res = _b(g, N, D, H, W, 64), _b(g, 3, 3, 3, 64, 64), _b(g, 64), _b(g, N, D, H, W, 64)
    out, pack = _empty(N, D, H, W, 64), _empty(ops.CONV64_PACK_FLOATS)
    A = ALGOS[algo]
    mask = ops.new_sign_mask(out) if ops.conv64_mask_ok(N, D, H, W, A) else None

    def launch(m):
        def f(x, w, bias, res):
            ops.pack_conv64_weights(w, wp_fwd=pack, want_dgrad=False)
            ops.conv3d_fwd(x, w, bias, ops.ACT_LEAKY, 0.2, res, wpack=pack, out=out, algo=A, mask=m)
            return [(out, "ab")] + ([(m, "same")] if m is not None else [])
        return f
    check_pow2("conv64 fwd f32 %s %s" % (dims, algo), launch(None), x, w, (bias, res), (out, pack))
    if mask is not None:
        check_pow2("conv64 fwd f32 %s %s + sign mask" % (dims, algo), launch(mask), x, w, (bias, res), (out, pack, mask))


@pytest.mark.parametrize("mt", BF_VARIANTS)
@pytest.mark.parametrize("dims", BF_GRIDS)
def test_conv64_fwd_bf16(fdn, dims, mt):
    N, D, H, W = dims
    g = P.gen(_seed(dims, mt, 2), "cuda")
    x, w, bias, res = _b(g, N, D, H, W, 64).to(BF16), _b(g, 3, 3, 3, 64, 64), _b(g, 64), _b(g, N, D, H, W, 64).to(BF16)
    out, pack = _empty(N, D, H, W, 64, dtype=BF16), _empty(bops.PACK_ELEMS, dtype=BF16)
    mask = bops.new_sign_mask(out)

    def launch(m):
        def f(x, w, bias, res):
            bops.pack_conv64_weights(w, wp_fwd=pack, want_dgrad=False)
            bops.conv3d_fwd(x, w, bias, ops.ACT_LEAKY, 0.2, res, wpack=pack, out=out, mask=m)
            return [(out, "ab")] + ([(m, "same")] if m is not None else [])
        return f
    with hooks(**bf_variant(mt)):
        check_pow2("conv64 fwd bf16 %s variant %d" % (dims, mt), launch(None), x, w, (bias, res), (out, pack))
        check_pow2("conv64 fwd bf16 %s variant %d + sign mask" % (dims, mt), launch(mask), x, w, (bias, res), (out, pack, mask))


# ---------------------------------------------------------------------------------------------------------------- forward, thin layers
@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_cin3_fwd(fdn, dt, dims, mfma):
    N, D, H, W = dims
    o = _o(dt)
    g = P.gen(_seed(dims, dt, 3), "cuda")
    x, w, bias = _st(_b(g, N, D, H, W, 3), dt), _b(g, 3, 3, 3, 3, 64), _b(g, 64)
    out = _empty(N, D, H, W, 64, dtype=o.ACT_DTYPE)

    def launch(x, w, bias):
        o.conv3d_fwd(x, w, bias, ops.ACT_RELU, out=out)
        return [(out, "ab")]
    with hooks(**({} if mfma else {"cin3_mfma": 0})):
        check_pow2("3->64 fwd %s %s mfma=%d" % (dt, dims, mfma), launch, x, w, (bias,), (out,))


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_head_fwd_into_channel_1(fdn, dt, dims, mfma):
    """64 -> 1 into channel 1 of an (N,V,3) fp32 prediction; channels 0 and 2 keep the sentinel."""
    N, D, H, W = dims
    o = _o(dt)
    g = P.gen(_seed(dims, dt, 4), "cuda")
    x, w, bias = _st(_b(g, N, D, H, W, 64), dt), _b(g, 3, 3, 3, 64, 1), _b(g, 1)
    pred = _empty(N, D, H, W, 3)

    def launch(x, w, bias):
        o.conv3d_fwd(x, w, bias, ops.ACT_NONE, out=pred, ldy=3, y_coff=1)
        return [(pred[..., 1], "ab"), (pred[..., 0], "same"), (pred[..., 2], "same")]
    with hooks(**({} if mfma else {"heads_mfma": 0})):
        check_pow2("64->1 fwd %s %s mfma=%d" % (dt, dims, mfma), launch, x, w, (bias,), (pred,))
    assert bool((pred[..., 0] == SENTINEL).all()) and bool((pred[..., 2] == SENTINEL).all())


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_conv1x1_fwd_with_x2(fdn, dt, dims, mfma):
    N, D, H, W = dims
    o = _o(dt)
    g = P.gen(_seed(dims, dt, 5), "cuda")
    xa, xb, w, bias = _st(_b(g, N, D, H, W, 64), dt), _st(_b(g, N, D, H, W, 64), dt), _b(g, 1, 1, 1, 128, 64), _b(g, 64)
    out = _empty(N, D, H, W, 64, dtype=o.ACT_DTYPE)

    def launch(xs, w, bias):
        o.conv3d_fwd(xs[0], w, bias, ops.ACT_RELU, x2=xs[1], out=out)
        return [(out, "ab")]
    with hooks(**({} if mfma else {"conv1x1_mfma": 0})):
        check_pow2("1x1 fwd %s %s mfma=%d" % (dt, dims, mfma), launch, [xa, xb], w, (bias,), (out,))


# ---------------------------------------------------------------------------------------------------------------- input gradients, 64 -> 64
def _fused_dgrad_case(o, dt, dims, g, nsrc):
    N, D, H, W = dims
    dzs = [_st(_b(g, N, D, H, W, 64), dt) for _ in range(nsrc)]
    ws = [_b(g, 3, 3, 3, 64, 64) for _ in range(nsrc)]
    skip, y = _st(_b(g, N, D, H, W, 64), dt), _st(_randn(g, N, D, H, W, 64), dt)
    pad, out = _empty(N, D + 2, H + 2, W + 2, 64), _empty(N, D, H, W, 64, dtype=o.ACT_DTYPE)
    packs = _empty(nsrc, 2, o.PACK_ELEMS, dtype=o.ACT_DTYPE)
    return dzs, ws, skip, y, pad, out, packs


@pytest.mark.parametrize("algo", sorted(ALGOS))
@pytest.mark.parametrize("dims", GRIDS)
def test_conv64_dgrad_fused_f32(fdn, dims, algo):
    """skip + y_prev, then the border fold; with mask= where the grid has sign masks."""
    N, D, H, W = dims
    A = ALGOS[algo]
    (dz,), (w,), skip, y, pad, out, packs = _fused_dgrad_case(ops, "f32", dims, P.gen(_seed(dims, algo, 6), "cuda"), 1)

    def launch(m):
        def f(dz, w, skip):
            ops.pack_conv64_weights(w, packs[0, 0], packs[0, 1])
            ops.conv3d_dgrad_fused(dz, packs[0, 1], pad, out, skip=skip, y_prev=None if m is not None else y, act=ops.ACT_LEAKY, algo=A, mask=m)
            ops.fold_halo_border([pad], out, skip, y, ops.ACT_LEAKY)
            return [(out, "ab")]
        return f
    check_pow2("fused dgrad f32 %s %s" % (dims, algo), launch(None), dz, w, (skip,), (pad, out, packs))
    if ops.conv64_mask_ok(N, D, H, W, A):
        check_pow2("fused dgrad f32 %s %s, sign mask" % (dims, algo), launch(sign_mask_words(y, planar=True)), dz, w, (skip,), (pad, out, packs))


@pytest.mark.parametrize("mt", BF_VARIANTS)
@pytest.mark.parametrize("dims", BF_GRIDS)
def test_conv64_dgrad_fused_bf16(fdn, dims, mt):
    (dz,), (w,), skip, y, pad, out, packs = _fused_dgrad_case(bops, "bf16", dims, P.gen(_seed(dims, mt, 7), "cuda"), 1)

    def launch(m):
        def f(dz, w, skip):
            bops.pack_conv64_weights(w, packs[0, 0], packs[0, 1])
            bops.conv3d_dgrad_fused(dz, packs[0, 1], pad, out, skip=skip, y_prev=None if m is not None else y, act=ops.ACT_LEAKY, mask=m)
            bops.fold_halo_border([pad], out, skip, y, ops.ACT_LEAKY)
            return [(out, "ab")]
        return f
    with hooks(**bf_variant(mt)):
        check_pow2("fused dgrad bf16 %s variant %d" % (dims, mt), launch(None), dz, w, (skip,), (pad, out, packs))
        check_pow2("fused dgrad bf16 %s variant %d, sign mask" % (dims, mt), launch(sign_mask_words(y, planar=False)), dz, w, (skip,), (pad, out, packs))


@pytest.mark.parametrize("dt,dims,variant", [("f32", d, a) for d in GRIDS for a in ("auto", "bf16x3")] + [("bf16", d, m) for d in BF_GRIDS for m in BF_VARIANTS])
def test_conv64_dgrad_fused_multi_three_sources(fdn, dt, dims, variant):
    """One launch for three layers that share their input (fp32: only where the grid has sign masks; elsewhere the call must refuse)."""
    N, D, H, W = dims
    o = _o(dt)
    A = ALGOS[variant] if dt == "f32" else ops.ALGO_AUTO
    dzs, ws, skip, y, pad, out, packs = _fused_dgrad_case(o, dt, dims, P.gen(_seed(dims, dt, variant, 8), "cuda"), 3)
    wds = [packs[s, 1] for s in range(3)]
    if not o.conv64_mask_ok(N, D, H, W, A):
        for s in range(3):
            o.pack_conv64_weights(ws[s], packs[s, 0], packs[s, 1])
        with pytest.raises(_lib.FdnError):
            o.conv3d_dgrad_fused_multi(dzs, wds, pad, out, skip=skip, y_prev=y, act=ops.ACT_LEAKY, algo=A)
        return

    def launch(m):
        def f(dzs, ws, skip):
            for s in range(3):
                o.pack_conv64_weights(ws[s], packs[s, 0], packs[s, 1])
            o.conv3d_dgrad_fused_multi(dzs, wds, pad, out, skip=skip, y_prev=None if m is not None else y, act=ops.ACT_LEAKY, algo=A, mask=m)
            o.fold_halo_border([pad], out, skip, y, ops.ACT_LEAKY)
            return [(out, "ab")]
        return f
    with hooks(**(bf_variant(variant) if dt == "bf16" else {})):
        check_pow2("multi-source fused dgrad %s %s %s" % (dt, dims, variant), launch(None), dzs, ws, (skip,), (pad, out, packs))
        check_pow2("multi-source fused dgrad %s %s %s, sign mask" % (dt, dims, variant), launch(sign_mask_words(y, planar=dt == "f32")), dzs, ws,
                   (skip,), (pad, out, packs))


@pytest.mark.parametrize("algo", ["auto", "direct"])
@pytest.mark.parametrize("dims", GRIDS)
def test_conv3d_dgrad_then_fold_halo(fdn, dims, algo):
    """The padded-grid dgrad and the whole-grid fold (fp32 only): 64 -> 64, and the 64 -> 1 head reading channel 1 of an (N,V,3) gradient."""
    N, D, H, W = dims
    g = P.gen(_seed(dims, algo, 9), "cuda")
    skip, y = _b(g, N, D, H, W, 64), _randn(g, N, D, H, W, 64)
    pad, out, packs = _empty(N, D + 2, H + 2, W + 2, 64), _empty(N, D, H, W, 64), _empty(2, ops.PACK_ELEMS)
    for cout in (64, 1):
        dz, w = _b(g, N, D, H, W, 64 if cout == 64 else 3), _b(g, 3, 3, 3, 64, cout)

        def launch(dz, w, skip):
            if cout == 64:
                ops.pack_conv64_weights(w, packs[0], packs[1])
                ops.conv3d_dgrad(dz, w, wpack_dgrad=packs[1], out=pad, algo=ALGOS[algo])
            else:
                ops.conv3d_dgrad(dz, w, out=pad, lddz=3, dz_coff=1, spatial=dims)
            ops.fold_halo([pad], skip, y, ops.ACT_LEAKY, 0.2, out=out)
            return [(out, "ab"), (pad, "ab")]
        check_pow2("dgrad + fold_halo %s %s cout=%d" % (dims, algo, cout), launch, dz, w, (skip,), (pad, out, packs))


# ---------------------------------------------------------------------------------------------------------------- input gradients, thin layers
@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_head_dgrad_folded_with_bias_gradient(fdn, dt, dims, mfma):
    """conv_cout1_dgrad_folded with dbias_prev (its workspace sentinel-filled); the mask form where it exists (fp32: W % 4 == 0, MFMA kernel)."""
    N, D, H, W = dims
    o = _o(dt)
    g = P.gen(_seed(dims, dt, 10), "cuda")
    dpred, w, y = _b(g, N, D, H, W, 3), _b(g, 3, 3, 3, 64, 1), _st(_randn(g, N, D, H, W, 64), dt)
    out, db, wsp = _empty(N, D, H, W, 64, dtype=o.ACT_DTYPE), _empty(64), _empty(2048 * 64)

    def launch(m):
        def f(dpred, w):
            o.conv_cout1_dgrad_folded(dpred, w, dims, None if m is not None else y, ops.ACT_LEAKY, 0.2, lddz=3, dz_coff=1, out=out, dbias_prev=db,
                                      workspace=wsp, mask=m)
            return [(out, "ab"), (db, "ab")]
        return f
    with hooks(**({} if mfma else {"heads_mfma": 0})):
        check_pow2("64->1 dgrad folded %s %s mfma=%d" % (dt, dims, mfma), launch(None), dpred, w, (), (out, db, wsp))
        if mfma and (dt == "bf16" or W % 4 == 0):
            check_pow2("64->1 dgrad folded %s %s, sign mask" % (dt, dims), launch(sign_mask_words(y, planar=dt == "f32")), dpred, w, (), (out, db, wsp))


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_conv1x1_dgrad(fdn, dt, dims, mfma):
    N, D, H, W = dims
    o = _o(dt)
    g = P.gen(_seed(dims, dt, 11), "cuda")
    dz, w = _st(_b(g, N, D, H, W, 64), dt), _b(g, 1, 1, 1, 128, 64)
    ya, yb = _st(_randn(g, N, D, H, W, 64), dt), _st(_randn(g, N, D, H, W, 64), dt)
    dxa, dxb = torch.empty_like(ya), torch.empty_like(yb)

    def launch(dz, w):
        o.conv1x1_dgrad(dz, w, ya, yb, dxa, dxb)
        return [(dxa, "ab"), (dxb, "ab")]
    with hooks(**({} if mfma else {"conv1x1_mfma": 0})):
        check_pow2("1x1 dgrad %s %s mfma=%d" % (dt, dims, mfma), launch, dz, w, (), (dxa, dxb))


# ---------------------------------------------------------------------------------------------------------------- weight gradients
def _wgrad_bufs(o, dims, Cin, Cout, K):
    return (_empty(K, K, K, Cin, Cout), _empty(Cout), _empty((o.wgrad_workspace_bytes(*dims, Cin, Cout, K) + 3) // 4))


@pytest.mark.parametrize("direct", [0, 1, 2])                # tests/test_gpu_kernels.py test_conv64_wgrad: product / the direct kernel / FDN_ALGO_WINO_W
@pytest.mark.parametrize("dims", GRIDS)
def test_conv64_wgrad_f32(fdn, dims, direct):
    N, D, H, W = dims
    g = P.gen(_seed(dims, direct, 12), "cuda")
    x, dz = _b(g, N, D, H, W, 64), _b(g, N, D, H, W, 64)
    dw, db, wsp = _wgrad_bufs(ops, dims, 64, 64, 3)

    def launch(x, dz):
        ops.conv3d_wgrad(x, dz, 3, 64, 64, want_bias=True, dw=dw, dbias=db, workspace=wsp, algo=ops.ALGO_WINO_W if direct == 2 else ops.ALGO_AUTO)
        return [(dw, "ab"), (db, "b")]
    with hooks(**({"wgrad64_direct": 1} if direct == 1 else {})):
        check_pow2("wgrad64 f32 %s direct=%d" % (dims, direct), launch, x, dz, (), (dw, db, wsp))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dims", BF_GRIDS)
def test_conv64_wgrad_bf16(fdn, dims, variant):
    N, D, H, W = dims
    g = P.gen(_seed(dims, variant, 13), "cuda")
    x, dz = _b(g, N, D, H, W, 64).to(BF16), _b(g, N, D, H, W, 64).to(BF16)
    dw, db, wsp = _wgrad_bufs(bops, dims, 64, 64, 3)

    def launch(x, dz):
        bops.conv3d_wgrad(x, dz, 3, 64, 64, want_bias=True, dw=dw, dbias=db, workspace=wsp)
        return [(dw, "ab"), (db, "b")]
    with hooks(**({"wgrad64_bf16_variant": 1} if variant else {})):
        check_pow2("wgrad64 bf16 %s variant=%d" % (dims, variant), launch, x, dz, (), (dw, db, wsp))


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_thin_wgrads(fdn, dt, dims, mfma):
    """3 -> 64, 64 -> 1 reading channel 1 of an (N,V,3) gradient (lddz = 3) and 1x1, each with its bias gradient."""
    N, D, H, W = dims
    o = _o(dt)
    g = P.gen(_seed(dims, dt, 14), "cuda")
    x3, x, xb = _st(_b(g, N, D, H, W, 3), dt), _st(_b(g, N, D, H, W, 64), dt), _st(_b(g, N, D, H, W, 64), dt)
    dz, dpred = _st(_b(g, N, D, H, W, 64), dt), _b(g, N, D, H, W, 3)
    with hooks(**({} if mfma else {"cin3_mfma": 0, "heads_mfma": 0, "conv1x1_mfma": 0})):
        dw, db, wsp = _wgrad_bufs(o, dims, 3, 64, 3)

        def launch3(x3, dz):
            o.conv3d_wgrad(x3, dz, 3, 3, 64, want_bias=True, dw=dw, dbias=db, workspace=wsp)
            return [(dw, "ab"), (db, "b")]
        check_pow2("3->64 wgrad %s %s mfma=%d" % (dt, dims, mfma), launch3, x3, dz, (), (dw, db, wsp))
        dw1, db1, wsp1 = _wgrad_bufs(o, dims, 64, 1, 3)

        def launch1(x, dpred):
            o.conv3d_wgrad(x, dpred, 3, 64, 1, want_bias=True, dw=dw1, dbias=db1, workspace=wsp1, lddz=3, dz_coff=1)
            return [(dw1, "ab"), (db1, "b")]
        check_pow2("64->1 wgrad %s %s mfma=%d" % (dt, dims, mfma), launch1, x, dpred, (), (dw1, db1, wsp1))
        dwk, dbk, wspk = _wgrad_bufs(o, dims, 128, 64, 1)

        def launchk(xs, dz):
            o.conv3d_wgrad(xs[0], dz, 1, 128, 64, x2=xs[1], want_bias=True, dw=dwk, dbias=dbk, workspace=wspk)
            return [(dwk, "ab"), (dbk, "b")]
        check_pow2("1x1 wgrad %s %s mfma=%d" % (dt, dims, mfma), launchk, [x, xb], dz, (), (dwk, dbk, wspk))


@pytest.mark.parametrize("dt,dims,algo", [("f32", d, a) for d in GRIDS for a in ("auto", "bf16x3")] + [("bf16", d, "auto") for d in BF_GRIDS])
def test_conv64_wgrad_batch_three_layers(fdn, dt, dims, algo):
    N, D, H, W = dims
    o = _o(dt)
    g = P.gen(_seed(dims, dt, algo, 15), "cuda")
    xs = [_st(_b(g, N, D, H, W, 64), dt) for _ in range(3)]
    dzs = [_st(_b(g, N, D, H, W, 64), dt) for _ in range(3)]
    dws, dbs = [_empty(3, 3, 3, 64, 64) for _ in range(3)], [_empty(64), None, _empty(64)]
    wsp = _empty((o.wgrad_batch_workspace_bytes(3, N, D, H, W) + 3) // 4 + 1)

    def launch(xs, dzs):
        o.conv3d_wgrad_batch(xs, dzs, dws, dbs, workspace=wsp, algo=ALGOS[algo])
        return [(t, "ab") for t in dws] + [(t, "b") for t in dbs if t is not None]
    check_pow2("batched wgrad64 %s %s %s" % (dt, dims, algo), launch, xs, dzs, (), dws + [dbs[0], dbs[2], wsp])


# ---------------------------------------------------------------------------------------------------------------- trilinear upsampling
@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_upsample_fwd_and_bwd(fdn, dt, dims, R):
    """One operand each: the forward scales with x, the backward (with y_prev, leaky) with dy."""
    N, D, H, W = dims
    o = _o(dt)
    g = P.gen(_seed(dims, dt, R, 16), "cuda")
    x, y = _st(_b(g, N, D, H, W, 64), dt), _st(_randn(g, N, D, H, W, 64), dt)
    dy = _st(_b(g, N, D * R, H * R, W * R, 64), dt)
    up, dx = torch.empty_like(dy), torch.empty_like(x)

    def fwd(x, _):
        o.upsample_trilinear_fwd(x, R, out=up)
        return [(up, "a")]
    check_pow2("upsample fwd %s %s R=%d" % (dt, dims, R), fwd, x, None, (), (up,))

    def bwd(dy, _):
        o.upsample_trilinear_bwd(dy, R, y, ops.ACT_LEAKY, 0.2, out=dx)
        return [(dx, "a")]
    check_pow2("upsample bwd %s %s R=%d" % (dt, dims, R), bwd, dy, None, (), (dx,))

"""The kernels outside the 64 -> 64 layers -- the three 64 -> 1 head operations, the 3 -> 64 layer and the 1x1 layer, both storage types --
against float64 PER ELEMENT on wide-range and channel-skewed operands, and single-product probes of the head kernels' "exact" claims.

(1) Per-element parity.  The other kernel tests draw N(0,1) operands and divide the error by max |ref| of the whole tensor: a quiet output
channel next to a loud one, or an output that is a small difference of large terms, can be wrong there without notice.  Here every output
element is held to a multiple of ITS OWN sum of term magnitudes, the same float64 reference evaluated on absolute values (head_wgrad_bound of
tests/_head_ref.py):
    fp32 outputs          |got - ref| <= SUM_TOL * sum|term|                     SUM_TOL = 1e-5, the constant of tests/test_gpu_head_walks.py
    bf16-stored outputs   |got - ref| <= 2^-8 |ref| + SUM_TOL * sum|term|         the one-ulp rule with its absolute slack made per-element
There is no max |ref| term.  Plain fp32 summation of these sums sits at 3e-7 .. 5e-7 of sum|term| (CPU emulation of the head GEMM), the
six-term bf16 form at 2e-7 .. 5e-7; the bf16-storage head forward drops the third piece of w, 2^-17 = 7.6e-6 of a term at worst.
Operands (tests/_operands.py): `wide` = x offset by m/s in {0, 10, 100}, dz log-uniform over 1e-6 .. 1, kernels N(0, 0.03) + 0.015; `skewed` =
N(0,1) times 2^k per channel, k in -12 .. 12, along the input channels of x and, independently, along the channels of the second operand
that become the OUTPUT's channels (w's output channels in a forward, dz's channels in a weight gradient, w's input channels in an input
gradient).  With an activation the linear part (ACT_NONE) is compared, and a ReLU launch separately: elements whose float64 pre-activation
lies within the bound of zero may take either side and are exempt, at most 1 % of the elements (asserted).
The test-build reference variants (the VALU kernels: fdn_debug_set_heads_mfma / _cin3_mfma / _conv1x1_mfma (0)) run beside the product
kernels on the same operands; both worst fractions of the bound are printed ([thin_range] lines, pytest -s; DESIGN.md section 5.6a holds them).

(2) Single-product probes.  x is one-hot in a random channel per voxel and w is non-zero at ONE tap (dense over channels), bias zero: every
output element is one product plus exact zeros, so the float64 reference is the exact product and the bound is relative to it.
    fp32 head forward    pieces3 x pieces3      <= 2^-21 |x w|   dropped terms 2 * 2^-25 + 2^-34, last accumulation 2^-24, earlier ones 2^-32 each:
                                                                 under 2^-22, a 2x margin; a missing kept term moves the result by more than 2^-20
                                                                 (tests/test_operand_recipes.py) on top of that error: it cannot pass
    bf16 head forward    bf16-exact x pieces3   <= 2^-16 |x w|   w = hi + lo drops the third piece (below 2^-17 |w|) by design; a missing lo
                                                                 term costs the second piece, more than 2^-10
    head weight gradient pieces3 dz, one non-zero dz voxel per launch (interior, corner); x bf16-exact (bf16 storage) or pieces2 (fp32 storage)
                                                <= 2^-22 |dz x|  three-piece scalars times bf16 x are exact products, the second and third
                                                                 piece each round the running sum once: 2 * 2^-24; fp32 storage: one fp32 multiply
    the VALU head kernels on the same probes    <= 2^-23         a single fp32 multiply"""
import importlib

import numpy as np
import pytest
import torch

import _head_ref as R
import _operands as P
from test_gpu_head_walks import SUM_TOL, _cin3_wgrad_ref
from test_gpu_pow2_scaling import BF_GRIDS, GRIDS, hooks

pytestmark = pytest.mark.gpu

ops = importlib.import_module("4dflownet_amd.ops")
bops = importlib.import_module("4dflownet_amd.ops_bf16")

F64, BF16 = torch.float64, torch.bfloat16
DT_GRIDS = [("f32", d) for d in GRIDS] + [("bf16", d) for d in BF_GRIDS]
FWD_RECIPES = ["offset0", "offset10", "offset100", "skewed"]          # x offset / skewed; the second operand: kernel / log-uniform / skewed
DGRAD_RECIPES = ["loguniform", "skewed"]                              # (an input gradient has no x: dz log-uniform, kernels shifted)
RELU_EXEMPT_CAP = 0.01


def _o(dt):
    return bops if dt == "bf16" else ops


def _st(t, dt):
    return t.to(BF16) if dt == "bf16" else t


def _gen(*parts):
    s = 29
    for p in parts:
        for q in (p if isinstance(p, (tuple, list)) else (p,)):
            s = (s * 1000003 + (sum(map(ord, q)) if isinstance(q, str) else int(q))) % (2 ** 31 - 1)
    return P.gen(s, "cuda")


def _x(g, recipe, shape):
    return P.skewed(g, shape, len(shape) - 1) if recipe == "skewed" else P.wide(g, recipe, shape)


def _second(g, recipe, kind, shape, dim):
    """The second operand: `kind` ("kernel" / "loguniform") under a wide recipe, skewed along `dim` under "skewed"."""
    return P.skewed(g, shape, dim) if recipe == "skewed" else P.wide(g, kind, shape)


def _excess(got, ref, bound, bf16_out, exempt=None):
    """(worst error as a fraction of the per-element bound, all within).  ref, bound float64."""
    err = (got.to(F64) - ref).abs()
    tol = SUM_TOL * bound + (2.0 ** -8 * ref.abs() if bf16_out else 0.0)
    if exempt is not None:
        err = torch.where(exempt, torch.zeros_like(err), err)
    return float((err / tol.clamp_min(1e-300)).max()), bool((err <= tol).all()) and bool(torch.isfinite(got).all())


def _relu_exempt(ref, bound, bf16_out, name):
    tol = SUM_TOL * bound + (2.0 ** -8 * ref.abs() if bf16_out else 0.0)
    exempt = ref.abs() <= tol
    share = float(exempt.to(F64).mean())
    assert share <= RELU_EXEMPT_CAP, "%s: %.2f %% of the pre-activations lie within the bound of zero" % (name, 100 * share)
    return exempt


def _both(hook, fn):
    """fn() on the product library and on the test build's reference variant."""
    with hooks():
        a = fn()
    with hooks(**{hook: 0}):
        b = fn()
    torch.cuda.synchronize()
    return a, b


def _judge(kernel, dt, recipe, dims, rows):
    """rows: [(label, (frac, ok) of the product kernel, (frac, ok) of the reference variant)]; print every row, then assert."""
    for label, (fp, _), (fv, _) in rows:
        print("\n  [thin_range] %-34s | %-4s | %-10s | %-14s | product %.4f | reference variant %.4f" % (kernel + " " + label, dt, recipe,
                                                                                                       "x".join(map(str, dims)), fp, fv))
    for label, (fp, okp), (fv, okv) in rows:
        assert okp, "%s %s %s %s %s: product kernel at %.3f of the per-element bound" % (kernel, label, dt, recipe, dims, fp)
        assert okv, "%s %s %s %s %s: reference variant at %.3f of the per-element bound" % (kernel, label, dt, recipe, dims, fv)


# ---------------------------------------------------------------------------------------------------------------- float64 references
def _cols3(x):
    """im2col of the edge-clamped 3x3x3 neighbourhood: (N,D,H,W,C) -> (V, 27 C) float64, column 3 tap + c for C = 3."""
    N, D, H, W = x.shape[:4]
    xp = R.edge_pad(R.edge_pad(R.edge_pad(x.to(F64), 1), 2), 3)
    cols = torch.stack([xp[:, a:a + D, b:b + H, c:c + W] for a in range(3) for b in range(3) for c in range(3)], dim=4)
    return cols.reshape(N * D * H * W, -1)


def _cin3_fwd_ref(x, w, b):
    return (torch.matmul(_cols3(x), w.to(F64).reshape(81, 64)) + b.to(F64)).reshape(tuple(x.shape[:4]) + (64,))


def _c1_fwd_ref(xa, xb, w, b):
    cat = torch.cat([xa, xb], dim=-1).to(F64).reshape(-1, 128)
    return (torch.matmul(cat, w.to(F64).reshape(128, 64)) + b.to(F64)).reshape(xa.shape)


def _c1_dgrad_ref(dz, w):
    d = torch.matmul(dz.to(F64).reshape(-1, 64), w.to(F64).reshape(128, 64).t())
    return d[:, :64].reshape(dz.shape), d[:, 64:].reshape(dz.shape)


def test_matmul_references_equal_the_numpy_oracle(oracle):
    """The float64 matmul formulations above against oracle/flownet_oracle.py on one ragged grid (1e-12 of scale)."""
    O = oracle
    g = _gen("refs")
    N, D, H, W = 1, 5, 7, 9
    rn = lambda *shape: torch.randn(shape, generator=g, device="cuda")
    x3, w3, b = rn(N, D, H, W, 3), rn(3, 3, 3, 3, 64), rn(64)
    xa, xb, wk, dz = rn(N, D, H, W, 64), rn(N, D, H, W, 64), rn(1, 1, 1, 128, 64), rn(N, D, H, W, 64)
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    close = lambda a, r: np.abs(a.cpu().numpy() - r).max() <= 1e-12 * np.abs(r).max()
    assert close(_cin3_fwd_ref(x3, w3, b), O.conv3d_fwd(n64(x3), n64(w3), n64(b), O.ACT_NONE))
    assert close(_cin3_wgrad_ref(x3, dz), O.conv3d_wgrad(n64(x3), n64(dz), 3))
    cat = np.concatenate([n64(xa), n64(xb)], -1)
    assert close(_c1_fwd_ref(xa, xb, wk, b), O.conv3d_fwd(cat, n64(wk), n64(b), O.ACT_NONE))
    dcat = O.conv3d_dgrad(n64(dz), n64(wk), cat.shape)
    da, db = _c1_dgrad_ref(dz, wk)
    assert close(da, dcat[..., :64]) and close(db, dcat[..., 64:])


# ---------------------------------------------------------------------------------------------------------------- the 64 -> 1 heads
@pytest.mark.parametrize("recipe", FWD_RECIPES)
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_head_fwd_per_element(fdn, dt, dims, recipe):
    o = _o(dt)
    g = _gen("head fwd", dt, dims, recipe)
    x = _st(_x(g, recipe, dims + (64,)), dt)
    w, b = _second(g, recipe, "kernel", (3, 3, 3, 64, 1), 4), P.wide(g, "kernel", (1,))
    ref, bound = R.head_fwd_ref(x, w, b), R.head_fwd_ref(x.abs(), w.abs(), b.abs())
    name = "head fwd %s %s %s" % (dt, dims, recipe)
    exempt = _relu_exempt(ref, bound, False, name)

    def run():
        pred = torch.zeros(dims + (3,), device="cuda")
        o.conv3d_fwd(x, w, b, ops.ACT_NONE, out=pred, ldy=3, y_coff=1)
        return pred[..., 1].clone(), o.conv3d_fwd(x, w, b, ops.ACT_RELU).reshape(dims)
    (lin_p, relu_p), (lin_v, relu_v) = _both("heads_mfma", run)
    _judge("head fwd", dt, recipe, dims, [("linear", _excess(lin_p, ref, bound, False), _excess(lin_v, ref, bound, False)),
                                          ("relu", _excess(relu_p, ref.clamp_min(0), bound, False, exempt), _excess(relu_v, ref.clamp_min(0), bound, False, exempt))])


@pytest.mark.parametrize("recipe", DGRAD_RECIPES)
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_head_dgrad_per_element(fdn, dt, dims, recipe):
    """dz_prev per element (channels of very different size under `skewed`: w along its input channels) and the producer's bias gradient."""
    o = _o(dt)
    g = _gen("head dgrad", dt, dims, recipe)
    dpred, w = _second(g, recipe, "loguniform", dims + (3,), 4), _second(g, recipe, "kernel", (3, 3, 3, 64, 1), 3)
    ref, bound = R.head_dgrad_ref(dpred[..., 1], w, dims), R.head_dgrad_ref(dpred[..., 1].abs(), w.abs(), dims)

    def run():
        db = torch.full((64,), float("nan"), device="cuda")
        return o.conv_cout1_dgrad_folded(dpred, w, dims, None, ops.ACT_NONE, 0.2, lddz=3, dz_coff=1, dbias_prev=db), db
    (out_p, db_p), (out_v, db_v) = _both("heads_mfma", run)
    bf = dt == "bf16"
    rs, bs = ref.reshape(-1, 64).sum(dim=0), bound.reshape(-1, 64).sum(dim=0)
    _judge("head dgrad", dt, recipe, dims, [("dz_prev", _excess(out_p, ref, bound, bf), _excess(out_v, ref, bound, bf)),
                                            ("producer bias grad", _excess(db_p, rs, bs, False), _excess(db_v, rs, bs, False))])


@pytest.mark.parametrize("recipe", FWD_RECIPES)
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_head_wgrad_per_element(fdn, dt, dims, recipe):
    o = _o(dt)
    g = _gen("head wgrad", dt, dims, recipe)
    x, dpred = _st(_x(g, recipe, dims + (64,)), dt), _second(g, recipe, "loguniform", dims + (3,), 4)
    dz = dpred[..., 1]
    ref, bound = R.head_wgrad_ref(x, dz), R.head_wgrad_bound(x, dz)
    rb, bb = dz.to(F64).sum().reshape(1), dz.to(F64).abs().sum().reshape(1)
    (dw_p, db_p), (dw_v, db_v) = _both("heads_mfma", lambda: o.conv3d_wgrad(x, dpred, 3, 64, 1, want_bias=True, lddz=3, dz_coff=1))
    _judge("head wgrad", dt, recipe, dims, [("dW", _excess(dw_p, ref, bound, False), _excess(dw_v, ref, bound, False)),
                                            ("bias grad", _excess(db_p, rb, bb, False), _excess(db_v, rb, bb, False))])


# ---------------------------------------------------------------------------------------------------------------- the 3 -> 64 layer
@pytest.mark.parametrize("recipe", FWD_RECIPES)
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_cin3_fwd_per_element(fdn, dt, dims, recipe):
    o = _o(dt)
    g = _gen("cin3 fwd", dt, dims, recipe)
    x = _st(_x(g, recipe, dims + (3,)), dt)
    w, b = _second(g, recipe, "kernel", (3, 3, 3, 3, 64), 4), P.wide(g, "kernel", (64,))
    ref, bound = _cin3_fwd_ref(x, w, b), _cin3_fwd_ref(x.abs(), w.abs(), b.abs())
    bf = dt == "bf16"
    exempt = _relu_exempt(ref, bound, bf, "3->64 fwd %s %s %s" % (dt, dims, recipe))
    (lin_p, relu_p), (lin_v, relu_v) = _both("cin3_mfma", lambda: (o.conv3d_fwd(x, w, b, ops.ACT_NONE), o.conv3d_fwd(x, w, b, ops.ACT_RELU)))
    rr = ref.clamp_min(0)
    _judge("3->64 fwd", dt, recipe, dims, [("linear", _excess(lin_p, ref, bound, bf), _excess(lin_v, ref, bound, bf)),
                                           ("relu", _excess(relu_p, rr, bound, bf, exempt), _excess(relu_v, rr, bound, bf, exempt))])


@pytest.mark.parametrize("recipe", FWD_RECIPES)
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_cin3_wgrad_and_bias_grad_per_element(fdn, dt, dims, recipe):
    o = _o(dt)
    g = _gen("cin3 wgrad", dt, dims, recipe)
    x, dz = _st(_x(g, recipe, dims + (3,)), dt), _st(_second(g, recipe, "loguniform", dims + (64,), 4), dt)
    ref, bound = _cin3_wgrad_ref(x, dz), _cin3_wgrad_ref(x.abs(), dz.abs())
    d2 = dz.to(F64).reshape(-1, 64)
    (dw_p, db_p), (dw_v, db_v) = _both("cin3_mfma", lambda: o.conv3d_wgrad(x, dz, 3, 3, 64, want_bias=True))
    _judge("3->64 wgrad", dt, recipe, dims, [("dW", _excess(dw_p, ref, bound, False), _excess(dw_v, ref, bound, False)),
                                             ("bias grad", _excess(db_p, d2.sum(dim=0), d2.abs().sum(dim=0), False),
                                              _excess(db_v, d2.sum(dim=0), d2.abs().sum(dim=0), False))])


# ---------------------------------------------------------------------------------------------------------------- the 1x1 layer
@pytest.mark.parametrize("recipe", FWD_RECIPES)
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_conv1x1_fwd_per_element(fdn, dt, dims, recipe):
    o = _o(dt)
    g = _gen("1x1 fwd", dt, dims, recipe)
    xa, xb = _st(_x(g, recipe, dims + (64,)), dt), _st(_x(g, recipe, dims + (64,)), dt)
    w, b = _second(g, recipe, "kernel", (1, 1, 1, 128, 64), 4), P.wide(g, "kernel", (64,))
    ref, bound = _c1_fwd_ref(xa, xb, w, b), _c1_fwd_ref(xa.abs(), xb.abs(), w.abs(), b.abs())
    bf = dt == "bf16"
    exempt = _relu_exempt(ref, bound, bf, "1x1 fwd %s %s %s" % (dt, dims, recipe))
    (lin_p, relu_p), (lin_v, relu_v) = _both("conv1x1_mfma", lambda: (o.conv3d_fwd(xa, w, b, ops.ACT_NONE, x2=xb), o.conv3d_fwd(xa, w, b, ops.ACT_RELU, x2=xb)))
    rr = ref.clamp_min(0)
    _judge("1x1 fwd", dt, recipe, dims, [("linear", _excess(lin_p, ref, bound, bf), _excess(lin_v, ref, bound, bf)),
                                         ("relu", _excess(relu_p, rr, bound, bf, exempt), _excess(relu_v, rr, bound, bf, exempt))])


@pytest.mark.parametrize("recipe", DGRAD_RECIPES)
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_conv1x1_dgrad_per_element(fdn, dt, dims, recipe):
    """Both halves, each times the ReLU mask of its producer (signs of ya / yb: exact in either storage type)."""
    o = _o(dt)
    g = _gen("1x1 dgrad", dt, dims, recipe)
    dz, w = _st(_second(g, recipe, "loguniform", dims + (64,), 4), dt), _second(g, recipe, "kernel", (1, 1, 1, 128, 64), 3)
    ya, yb = (_st(torch.randn(dims + (64,), generator=g, device="cuda"), dt) for _ in range(2))
    (ra, rb), (ba, bb) = _c1_dgrad_ref(dz, w), _c1_dgrad_ref(dz.abs(), w.abs())
    ra, rb, ba, bb = ra * (ya > 0), rb * (yb > 0), ba * (ya > 0), bb * (yb > 0)
    (da_p, db_p), (da_v, db_v) = _both("conv1x1_mfma", lambda: o.conv1x1_dgrad(dz, w, ya, yb))
    bf = dt == "bf16"
    _judge("1x1 dgrad", dt, recipe, dims, [("a", _excess(da_p, ra, ba, bf), _excess(da_v, ra, ba, bf)), ("b", _excess(db_p, rb, bb, bf), _excess(db_v, rb, bb, bf))])


@pytest.mark.parametrize("recipe", FWD_RECIPES)
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_conv1x1_wgrad_per_element(fdn, dt, dims, recipe):
    o = _o(dt)
    g = _gen("1x1 wgrad", dt, dims, recipe)
    xa, xb = _st(_x(g, recipe, dims + (64,)), dt), _st(_x(g, recipe, dims + (64,)), dt)
    dz = _st(_second(g, recipe, "loguniform", dims + (64,), 4), dt)
    cat, d2 = torch.cat([xa, xb], dim=-1).to(F64).reshape(-1, 128), dz.to(F64).reshape(-1, 64)
    ref, bound = torch.matmul(cat.t(), d2).reshape(1, 1, 1, 128, 64), torch.matmul(cat.abs().t(), d2.abs()).reshape(1, 1, 1, 128, 64)
    (dw_p, db_p), (dw_v, db_v) = _both("conv1x1_mfma", lambda: o.conv3d_wgrad(xa, dz, 1, 128, 64, x2=xb, want_bias=True))
    _judge("1x1 wgrad", dt, recipe, dims, [("dW", _excess(dw_p, ref, bound, False), _excess(dw_v, ref, bound, False)),
                                           ("bias grad", _excess(db_p, d2.sum(dim=0), d2.abs().sum(dim=0), False),
                                            _excess(db_v, d2.sum(dim=0), d2.abs().sum(dim=0), False))])


# ---------------------------------------------------------------------------------------------------------------- single-product probes
PROBE_GRIDS = [(1, 5, 7, 9), (2, 12, 10, 24)]
PROBE_TAPS = {"corner": (0, 0, 0), "centre": (1, 1, 1), "edge": (2, 1, 0)}
FWD_PROBE_TOL = {"f32": 2.0 ** -21, "bf16": 2.0 ** -16}
WGRAD_PROBE_TOL, VALU_PROBE_TOL = 2.0 ** -22, 2.0 ** -23


def _rel(got, ref):
    """Worst |got - ref| / |ref| (ref non-zero everywhere: one product of non-zero pieces per element), as a power of two."""
    assert bool((ref != 0).all()) and bool(torch.isfinite(got).all())
    return float(((got.to(F64) - ref).abs() / ref.abs()).max())


def _probe_report(name, rel_p, tol_p, rel_v):
    print("\n  [thin_range probe] %-52s product 2^%.2f (bound 2^%d) | VALU 2^%.2f (bound 2^-23)"
          % (name, np.log2(max(rel_p, 1e-300)), round(np.log2(tol_p)), np.log2(max(rel_v, 1e-300))))
    assert rel_p <= tol_p, "%s: product kernel off the exact product by 2^%.2f" % (name, np.log2(rel_p))
    assert rel_v <= VALU_PROBE_TOL, "%s: VALU kernel off the exact product by 2^%.2f" % (name, np.log2(rel_v))


@pytest.mark.parametrize("tap", sorted(PROBE_TAPS))
@pytest.mark.parametrize("dims", PROBE_GRIDS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_fwd_single_product_probe(fdn, dt, dims, tap):
    o = _o(dt)
    g = _gen("probe fwd", dt, dims, tap)
    N, D, H, W = dims
    vals = (P.pieces3 if dt == "f32" else P.pieces1)(g, dims)[0]
    ch = torch.randint(0, 64, dims, generator=g, device="cuda")
    x = _st(torch.zeros(dims + (64,), device="cuda").scatter_(4, ch.unsqueeze(-1), vals.unsqueeze(-1)), dt)
    w = torch.zeros((3, 3, 3, 64, 1), device="cuda")
    a, b, c = PROBE_TAPS[tap]
    w[a, b, c, :, 0] = P.pieces3(g, (64,))[0]
    ref = R.head_fwd_ref(x, w)                                     # one non-zero float64 term per output: the exact product
    zero_bias = torch.zeros(1, device="cuda")

    def run():
        pred = torch.full(dims + (3,), 7.5, device="cuda")
        o.conv3d_fwd(x, w, zero_bias, ops.ACT_NONE, out=pred, ldy=3, y_coff=1)
        return pred[..., 1].clone()
    got_p, got_v = _both("heads_mfma", run)
    _probe_report("head fwd %s %s tap %s" % (dt, dims, tap), _rel(got_p, ref), FWD_PROBE_TOL[dt], _rel(got_v, ref))


@pytest.mark.parametrize("where", ["interior", "corner"])
@pytest.mark.parametrize("dims", [(1, 5, 7, 9), (1, 10, 12, 16)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_wgrad_single_product_probe(fdn, dt, dims, where):
    """One non-zero dz voxel in the (single) sample: dW[t][c] = dz[o] x[clamp(o + t - 1)][c], one product for each of the 27 x 64 elements."""
    o = _o(dt)
    g = _gen("probe wgrad", dt, dims, where)
    N, D, H, W = dims
    x = _st((P.pieces2 if dt == "f32" else P.pieces1)(g, dims + (64,))[0], dt)
    dz = torch.zeros(dims + (1,), device="cuda")
    pos = (0, D - 1, 0, W - 1) if where == "corner" else (0, D // 2, H // 2, W // 2)
    dz[pos] = P.pieces3(g, (1,))[0]
    ref = R.head_wgrad_ref(x, dz)
    (dw_p, _), (dw_v, _) = _both("heads_mfma", lambda: o.conv3d_wgrad(x, dz, 3, 64, 1, want_bias=True))
    _probe_report("head wgrad %s %s dz voxel %s" % (dt, dims, where), _rel(dw_p, ref), WGRAD_PROBE_TOL, _rel(dw_v, ref))

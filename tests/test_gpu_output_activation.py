"""The heads' tanh output activation (FDN_ACT_TANH in head_fwd_kernel's epilogue) and non_fluid_weight (fdn_loss_metrics_act) on the GPU,
from the kernels up to TrainerController and prepare_network, against the float64 reference in tests/_output_activation.py."""
import functools
import hashlib
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import flownet_oracle as O
from _kink import kink_sides
from _output_activation import ACT_NONE, ACT_TANH, loss_reference, ulp_distance, weighted_loss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The formula of head_tanh (heads_mfma.hip): odd polynomial below |z| = 0.625, 1 - 2 / (exp(2|z|) + 1) above.  Largest error against
# float32(numpy.tanh(float64(z))) measured on the MI355X over the cases of test_head_forward below (profiles/output_activation.txt),
# in ulps of the reference; the assertion allows one ulp more for inputs the sweep does not hold.
TANH_ULP_MEASURED = 2.0
TANH_ULP_BOUND = TANH_ULP_MEASURED + 1.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rel_err(got, ref):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


# ------------------------------------------------------------------------------------------------------------- head forward
HEAD_CASES = [((1, 5, 7, 9), 0), ((2, 12, 12, 12), 0), ((8, 24, 24, 24), 0), ((2, 12, 12, 12), -10), ((2, 12, 12, 12), 20)]


@functools.lru_cache(maxsize=None)
def head_operands(shape, log2_scale):
    """x (N,D,H,W,64), w (3,3,3,64,1), bias (1,): pre-activations of about +-12 (standard deviation 4 at the largest rows, rows scaled
    down to 2 % of that), times 2^log2_scale through the weights and the bias."""
    rng = np.random.default_rng(1000 + sum(shape) + log2_scale)
    x = rng.normal(size=shape + (64,)) * rng.uniform(0.02, 1.0, size=shape + (1,))
    s = 2.0 ** log2_scale
    w = rng.normal(0, 0.17, size=(3, 3, 3, 64, 1)) * s
    b = np.array([0.3 * s])
    return x.astype(np.float32), w.astype(np.float32), b.astype(np.float32)


def run_head(fdn, dtype, x, w, b, act):
    ops = fdn.ops if dtype == "float32" else importlib.import_module("4dflownet_amd.ops_bf16")
    xt = dev(x).to(ops.ACT_DTYPE)
    y = ops.conv3d_fwd(xt, dev(w), dev(b), act)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and tuple(y.shape) == x.shape[:4] + (1,)
    return y.cpu().numpy()


def golden_none():
    with open(os.path.join(ROOT, "tests", "golden", "output_activation_none.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("shape,log2_scale", HEAD_CASES)
def test_head_forward(fdn, dtype, shape, log2_scale):
    x, w, b = head_operands(shape, log2_scale)
    z = run_head(fdn, dtype, x, w, b, fdn.ops.ACT_NONE)
    y = run_head(fdn, dtype, x, w, b, fdn.ops.ACT_TANH)
    ref = np.tanh(z.astype(np.float64)).astype(np.float32)
    ulps = ulp_distance(y, ref)
    az = np.abs(z)
    print("head %s %s 2^%d: |z| max %.3g median %.3g, %d of %d below 0.625, %d at or above 9.02; worst %.3f ulp at z = %r"
          % (dtype, shape, log2_scale, az.max(), np.median(az), (az < 0.625).sum(), az.size, (az >= 9.02).sum(), ulps.max(),
             float(z.reshape(-1)[ulps.argmax()])))
    assert not np.isnan(y).any() and not np.isnan(z).any()
    assert ulps.max() <= TANH_ULP_BOUND, ulps.max()
    assert (np.abs(y) <= 1).all()
    sat = az >= 9.02
    assert (y[sat] == np.sign(z[sat])).all()
    if log2_scale == 0:
        assert az.max() >= 11 and (az < 0.625).sum() >= az.size // 20 and sat.sum() >= 1       # the span the bound was measured on
    elif log2_scale > 0:
        assert sat.mean() > 0.99
    else:
        assert az.max() < 0.625                                                                   # the polynomial side alone
    # odd, bit for bit, by negating the weights and the bias: wherever that negates the pre-activation exactly (the matrix pipe's
    # accumulation does not everywhere; test_tanh_on_exact_probes has pre-activations that are exact on both sides)
    zn = run_head(fdn, dtype, x, -w, -b, fdn.ops.ACT_NONE)
    yn = run_head(fdn, dtype, x, -w, -b, fdn.ops.ACT_TANH)
    exact = zn.view(np.uint32) == (-z).view(np.uint32)
    print("  pre-activation negated exactly at %d of %d outputs" % (exact.sum(), exact.size))
    assert exact.sum() >= 32
    assert np.array_equal(yn.view(np.uint32)[exact], (-y).view(np.uint32)[exact])
    assert ulp_distance(yn, np.tanh(zn.astype(np.float64)).astype(np.float32)).max() <= TANH_ULP_BOUND
    # ACT_NONE: the bits of the library before the activation existed (recorded from it on these operands)
    key = "%s %s 2^%d" % (dtype, "x".join(map(str, shape)), log2_scale)
    assert hashlib.sha256(z.tobytes()).hexdigest() == golden_none()[key], key


@functools.lru_cache(maxsize=None)
def probe_values():
    """8 x 24^3 pre-activations chosen one by one: magnitudes from 2^-40 to 2^6 (log-uniform), every float around the seam of the two
    formulas (0.625), the interval where 1 - tanh crosses half an ulp of 1 (9.0 .. 9.03), and large finite values."""
    rng = np.random.default_rng(77)
    n = 8 * 24 ** 3
    v = np.exp2(rng.uniform(-40, 6, size=n)).astype(np.float32)
    seam = np.float32(0.625)
    k = 4096
    v[:k] = seam - (np.arange(k) + 1).astype(np.float32) * np.spacing(np.float32(0.5))
    v[k:2 * k] = seam + np.arange(k).astype(np.float32) * np.spacing(seam)
    v[2 * k:6 * k] = np.linspace(9.0, 9.03, 4 * k).astype(np.float32)
    v[6 * k:7 * k] = np.linspace(2.0 ** -20, 12.0, k).astype(np.float32)
    v[7 * k:7 * k + 4] = [3e38, 1e30, 16.0, 9.02]
    return v.reshape(8, 24, 24, 24)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_tanh_on_exact_probes(fdn, dtype):
    """One input channel and the centre tap of weight +-1, bias 0: the pre-activation of every output IS its voxel's input value (the
    three bf16 pieces of an fp32 value add back to it exactly; every other product is a zero), so z and -z are exact and chosen."""
    v = probe_values()
    if dtype == "bfloat16":
        v = torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()
    x = np.zeros(v.shape + (64,), np.float32)
    x[..., 0] = v
    w = np.zeros((3, 3, 3, 64, 1), np.float32)
    w[1, 1, 1, 0, 0] = 1.0
    b = np.zeros(1, np.float32)
    z = run_head(fdn, dtype, x, w, b, fdn.ops.ACT_NONE)[..., 0]
    assert np.array_equal(z.view(np.uint32), v.view(np.uint32))
    zn = run_head(fdn, dtype, x, -w, b, fdn.ops.ACT_NONE)[..., 0]
    assert np.array_equal(zn.view(np.uint32), (-v).view(np.uint32)), (zn.view(np.uint32) != (-v).view(np.uint32)).sum()
    y = run_head(fdn, dtype, x, w, b, fdn.ops.ACT_TANH)[..., 0]
    yn = run_head(fdn, dtype, x, -w, b, fdn.ops.ACT_TANH)[..., 0]
    assert np.array_equal(yn.view(np.uint32), (-y).view(np.uint32))                        # odd, bit for bit
    ulps = ulp_distance(y, np.tanh(v.astype(np.float64)).astype(np.float32))
    print("probes %s: worst %.3f ulp at z = %r; below the seam %.3f, above %.3f" % (dtype, ulps.max(), float(v.reshape(-1)[ulps.argmax()]),
                                                                                  ulps[v < 0.625].max(), ulps[v >= 0.625].max()))
    assert ulps.max() <= TANH_ULP_BOUND
    assert not np.isnan(y).any() and (np.abs(y) <= 1).all()
    assert (y[v >= 9.02] == 1).all() and (v >= 9.02).sum() > 1000 and (y[(v > 0) & (v < 9.0)] < 1).any()


def test_tanh_through_the_prediction_layout(fdn):
    """The heads write into the (N,V,3) prediction (ldy = 3, y_coff = head): the activation follows the route, not the layout."""
    x, w, b = head_operands((1, 5, 7, 9), 0)
    pred = torch.full((1, 5, 7, 9, 3), 7.0, device="cuda")
    fdn.ops.conv3d_fwd(dev(x), dev(w), dev(b), fdn.ops.ACT_TANH, out=pred, ldy=3, y_coff=1)
    y = run_head(fdn, "float32", x, w, b, fdn.ops.ACT_TANH)
    p = pred.cpu().numpy()
    assert np.array_equal(p[..., 1:2], y) and (p[..., 0] == 7).all() and (p[..., 2] == 7).all()


# ------------------------------------------------------------------------------------------------------------- loss kernel
LOSS_SHAPES = [(2, 6, 6, 6), (1, 1, 4, 5), (3, 5, 7, 9), (8, 24, 24, 24)]


@functools.lru_cache(maxsize=None)
def loss_case(shape, mask_kind):
    """pred in (-1, 1) with values within 2^-20 of +-1 and exactly +-1, truth, mask -- numpy and device copies."""
    rng = np.random.default_rng(sum(shape) * 3 + len(mask_kind))
    pred = rng.uniform(-0.999, 0.999, size=shape + (3,)).astype(np.float32)
    flat = pred.reshape(-1)
    n = flat[3::11].size
    flat[3::11] = (np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 - rng.integers(1, 17, size=n) * 2.0 ** -24)).astype(np.float32)
    flat[5::13] = np.where(np.arange(flat[5::13].size) % 2 == 0, 1.0, -1.0)
    assert ((np.abs(flat) < 1) & (np.abs(flat) >= 1 - 2.0 ** -20)).sum() >= 3 and (np.abs(flat) == 1).sum() >= 3
    truth = [rng.uniform(-0.9, 0.9, size=shape).astype(np.float32) for _ in range(3)]
    if mask_kind == "binary":
        mask = (rng.uniform(size=shape) < 0.3).astype(np.float32)
    else:
        mask = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), size=shape)
        mask.reshape(-1)[::7] = 0.5                        # exactly on the non-fluid threshold
    return (pred, truth, mask), (dev(pred), [dev(t) for t in truth], dev(mask))


@functools.lru_cache(maxsize=None)
def loss_ref(shape, mask_kind, div_weight, non_fluid_weight, out_act):
    (pred, truth, mask), _ = loss_case(shape, mask_kind)
    hires = np.stack(truth, -1).astype(np.float64)
    mse_b, div_b, dz = loss_reference(pred, hires, mask, div_weight, non_fluid_weight, out_act)
    return mse_b, div_b, dz, O.relative_error(pred, hires.astype(np.float32), mask)


@pytest.mark.parametrize("out_act", [ACT_NONE, ACT_TANH])
@pytest.mark.parametrize("non_fluid_weight", [0.0, 0.25, 1.0, 3.0])
@pytest.mark.parametrize("div_weight", [0.0, 0.8])
@pytest.mark.parametrize("mask_kind", ["binary", "fractional"])
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_loss_kernel_matches_float64(fdn, shape, mask_kind, div_weight, non_fluid_weight, out_act):
    (pred, truth, mask), (p, t, m) = loss_case(shape, mask_kind)
    out, dp = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, div_weight=div_weight, non_fluid_weight=non_fluid_weight, out_act=out_act)
    default = non_fluid_weight == 1.0 and out_act == ACT_NONE
    assert tuple(out.shape) == (shape[0], 4 if default and div_weight == 0 else 5)           # at the defaults: today's calls
    out = out.cpu().numpy().astype(np.float64)
    dp = dp.cpu().numpy()
    mse_b, div_b, dz, rel = loss_ref(shape, mask_kind, div_weight, non_fluid_weight, out_act)
    figures = (rel_err(out[:, 0], mse_b), rel_err(out[:, 1], rel), rel_err(dp, dz))
    print("loss %s %s div %g nf %g act %d: mse %.2e metric %.2e dpred %.2e" % ((shape, mask_kind, div_weight, non_fluid_weight, out_act) + figures))
    assert figures[0] <= 1e-5
    assert figures[1] <= 2e-3                              # (the metric rounds to 1e-4 steps)
    assert rel_err(out[:, 2], mask.astype(np.float64).sum((1, 2, 3))) <= 1e-5
    assert rel_err(out[:, 3], (mask < 0.5).sum((1, 2, 3))) <= 1e-5
    if out.shape[1] == 5:
        assert rel_err(out[:, 4], div_b) <= 1e-5, (out[:, 4], div_b)
    assert figures[2] <= 1e-5
    if out_act == ACT_TANH:
        assert (dp[np.abs(pred) == 1] == 0).all()          # 1 - y^2 from the output: exactly 0 at y = +-1
        near = (np.abs(pred) < 1) & (np.abs(pred) >= 1 - 2.0 ** -20)
        assert ((dp[near] != 0) == (dz[near] != 0)).all() and (non_fluid_weight == 0 or (dp[near] != 0).any())
    # want_grad=False: the same values, no gradient
    out2, none = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, want_grad=False, div_weight=div_weight, non_fluid_weight=non_fluid_weight,
                                      out_act=out_act)
    assert none is None and np.array_equal(out2.cpu().numpy().astype(np.float64), out)


def call_act(fdn, p, t, m, div_weight, non_fluid_weight, out_act):
    N, D, H, W = p.shape[:4]
    out = torch.empty((N, 5), device="cuda")
    dp = torch.empty_like(p)
    scratch = torch.empty((N * (8 + 5 * 256),), device="cuda")
    lib = fdn._lib.load()
    rc = lib.fdn_loss_metrics_act(p.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), m.data_ptr(), div_weight, non_fluid_weight,
                                  out_act, out.data_ptr(), dp.data_ptr(), scratch.data_ptr(), N, D, H, W, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.fdn_last_error()
    return out, dp


def call_div(fdn, p, t, m, div_weight):
    N, D, H, W = p.shape[:4]
    out = torch.empty((N, 5), device="cuda")
    dp = torch.empty_like(p)
    scratch = torch.empty((N * (8 + 5 * 256),), device="cuda")
    lib = fdn._lib.load()
    rc = lib.fdn_loss_metrics_div(p.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), m.data_ptr(), div_weight, out.data_ptr(),
                                  dp.data_ptr(), scratch.data_ptr(), N, D, H, W, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.fdn_last_error()
    return out, dp


@pytest.mark.parametrize("shape", [(2, 6, 6, 6), (3, 5, 7, 9), (8, 24, 24, 24)])
def test_defaults_are_the_existing_entry_points_bit_for_bit(fdn, shape):
    _, (p, t, m) = loss_case(shape, "fractional")
    for wgt in (0.8, 0.0):
        ref, dref = call_div(fdn, p, t, m, wgt)
        out, dp = call_act(fdn, p, t, m, wgt, 1.0, ACT_NONE)
        torch.cuda.synchronize()
        assert torch.equal(out, ref) and torch.equal(dp, dref), wgt
    plain, dp_plain = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m)
    assert tuple(plain.shape) == (shape[0], 4)
    assert torch.equal(out[:, :4], plain) and torch.equal(dp, dp_plain) and (out[:, 4] == 0).all()


def test_deterministic_and_linear_in_the_non_fluid_weight(fdn):
    """Two calls give the same bits.  Linearity as test_deterministic_and_linear_in_the_weight checks it, on a product: the prediction
    equals the truth on the fluid voxels of a binary mask, so the fluid part of column 0 is exactly 0 and the column IS
    non_fluid_weight times the non-fluid part n -- rn(3 n) - n against 2 n, one rounding."""
    (pred, truth, mask), _ = loss_case((8, 24, 24, 24), "binary")
    pred = pred.copy()
    for c in range(3):
        pred[..., c][mask == 1] = truth[c][mask == 1]
    p, t, m = dev(pred), [dev(x) for x in truth], dev(mask)
    o1, d1 = call_act(fdn, p, t, m, 0.8, 0.25, ACT_TANH)
    o1b, d1b = call_act(fdn, p, t, m, 0.8, 0.25, ACT_TANH)
    assert torch.equal(o1, o1b) and torch.equal(d1, d1b)
    outs = dict((w, call_act(fdn, p, t, m, 0.0, w, ACT_NONE)[0].cpu().numpy()) for w in (0.0, 1.0, 3.0))
    assert (outs[0.0][:, 0] == 0).all() and (outs[1.0][:, 0] > 0).all()
    a = outs[3.0][:, 0].astype(np.float64) - outs[1.0][:, 0]
    b = 2.0 * outs[1.0][:, 0].astype(np.float64)
    assert (np.abs(a - b) <= np.spacing(outs[3.0][:, 0])).all(), (a, b)
    for w in (0.0, 3.0):
        assert np.array_equal(outs[w][:, 1:4], outs[1.0][:, 1:4])


# ------------------------------------------------------------------------------------------------------------- train step
def make_trainer(P, R, LB, HB, seed=0, head_scale=1.0, **kw):
    """test_gpu_divergence_loss.make_trainer at Glorot scale, the three 64 -> 1 kernels times head_scale."""
    trainer_mod = importlib.import_module("4dflownet_amd.trainer")
    tc = trainer_mod.TrainerController(P, R, initial_learning_rate=1e-3, quicksave_enable=False, low_resblock=LB, hi_resblock=HB,
                                       seed=seed, **kw)
    params = O.init_params(seed, LB, HB, np.float64)
    rng = np.random.default_rng(seed + 1)
    arrays = []
    for p in params:
        p["w"] = (p["w"] * (head_scale if p["w"].shape[-1] == 1 else 1.0)).astype(np.float32).astype(np.float64)
        arrays.append(p["w"].astype(np.float32))
        if p["b"] is not None:
            p["b"] = rng.normal(0, 0.05, p["b"].shape).astype(np.float32).astype(np.float64)
            arrays.append(p["b"].astype(np.float32))
    tc.model.set_weights(arrays)
    return tc, params


def hot_corner_batch(B, P, R, seed, gain):
    """O.synthetic_batch with the velocities of one 2^3 low-res corner times `gain`: a few output voxels far out, most where they were."""
    batch = [a.copy() for a in O.synthetic_batch(B, P, R, seed=seed)]
    for k in range(3):
        batch[k][:, :2, :2, :2] *= gain
    return tuple(batch)


@pytest.mark.parametrize("div_weight", [0.0, 0.5])
@pytest.mark.parametrize("P,R,LB,HB,B,head_scale", [(6, 2, 1, 1, 2, 6.0), (4, 3, 0, 1, 1, 12.0)])
def test_train_step_matches_float64(fdn, P, R, LB, HB, B, head_scale, div_weight):
    nfw = 0.25
    tc, params = make_trainer(P, R, LB, HB, seed=2, head_scale=head_scale, output_activation="tanh", non_fluid_weight=nfw, div_weight=div_weight)
    assert tc.model.output_activation == "tanh" and tc.model.out_act == fdn.ops.ACT_TANH
    batch = hot_corner_batch(B, P, R, 41, 20.0)
    b64 = tuple(a.astype(np.float64) for a in batch)
    inputs, hires, venc, mask = tc._unpack(batch)
    pred = tc.model.forward(inputs, training=True)
    ref_z, rc = O.network_forward(params, b64[:6], R, LB, HB, f32_coeffs=True)
    ref_pred = np.tanh(ref_z)
    sides, flips, worst = kink_sides(tc.model._cache, rc)
    pred_np = pred.cpu().numpy()
    nsat = int((np.abs(pred_np) == 1).sum())
    print("train step %s div %g: flips %d worst %.2e, prediction %.2e, %d of %d outputs saturated, |z| median %.2f"
          % ((P, R, LB, HB, B), div_weight, flips, worst, rel_err(pred_np, ref_pred), nsat, pred_np.size, np.median(np.abs(ref_z))))
    assert flips <= 2 and worst <= 2e-5, (flips, worst)
    assert rel_err(pred_np, ref_pred) < 1e-4
    assert 1 <= nsat < pred_np.size // 2 and (np.abs(ref_z) >= 9.02).sum() >= 1              # some saturate, most do not
    hires64 = np.concatenate(b64[6:9], -1)
    mse, div_b, dz = loss_reference(ref_pred, hires64, b64[10], div_weight, nfw, ACT_TANH)
    grads = O.network_backward(params, rc, dz, R, LB, HB, f32_coeffs=True, sides=sides)
    for g, p in zip(grads, params):
        g["w"] = g["w"] + (B * 2 * O.L2_LAMBDA) * p["w"]
    gref = O.flatten(grads)
    l2 = O.l2_regularizer(params)
    w_before = tc.model.flat_w.cpu().numpy().astype(np.float64)
    tc.reset_metrics()
    loss = tc.train_step(batch)
    g = tc.model.flat_g.cpu().numpy().astype(np.float64)                # backward's gradient (Adam reads it, L2 added inside)
    isk = tc.model.is_kernel.cpu().numpy().astype(np.float64)
    g_total = g + B * 2 * O.L2_LAMBDA * w_before * isk
    worst_g = 0.0
    for L in tc.model.layers:
        sl = slice(L.w_off, L.w_off + L.w.numel())
        worst_g = max(worst_g, rel_err(g_total[sl], gref[sl]))
        assert rel_err(g_total[sl], gref[sl]) < 1e-4, (L.name, "kernel grad", rel_err(g_total[sl], gref[sl]))
        if L.b is not None:
            sb = slice(L.b_off, L.b_off + L.cout)
            assert rel_err(g_total[sb], gref[sb]) < 1e-4, (L.name, "bias grad")
    print("  worst kernel-gradient error %.2e" % worst_g)
    assert rel_err(loss.cpu().numpy(), mse + div_b + l2) < 1e-4
    # the weights after one Adam step: lr * g / (|g| + eps) per element; compared where the gradient is well-conditioned (smoke())
    # (an element whose gradient is rounding noise may go either way, by at most 2 lr)
    w_ref = O.flatten(params).copy()
    O.adam_step_tf(w_ref, gref, np.zeros_like(gref), np.zeros_like(gref), 1, 1e-3)
    w_after = tc.model.flat_w.cpu().numpy().astype(np.float64)
    good = np.abs(gref) >= 1e-3 * np.abs(gref).max()
    assert np.abs(w_after - w_before).max() <= 2.1e-3
    assert np.abs(w_after - w_ref)[good].max() <= 1e-5, np.abs(w_after - w_ref)[good].max()
    res = dict((k, v.result()) for k, v in tc.loss_metrics.items())
    assert abs(res["train_mse"] - mse.mean()) <= 1e-4 * abs(mse.mean())
    assert abs(res["train_div"] - div_b.mean()) <= 1e-4 * abs(div_b.mean())


def test_bf16_mode(fdn):
    """One step in bf16 mode at the bounds of test_bf16_mode_with_divergence: the loss pass sees the fp32 prediction the tanh heads wrote."""
    P, R, LB, HB, B = 8, 2, 1, 1, 2
    tc, _ = make_trainer(P, R, LB, HB, seed=3, head_scale=6.0, dtype="bfloat16", div_weight=0.5, output_activation="tanh", non_fluid_weight=0.25)
    assert tc.model.act_dtype == torch.bfloat16
    batch = hot_corner_batch(B, P, R, 31, 20.0)
    inputs, hires, venc, mask = tc._unpack(batch)
    pred = tc.model.forward(inputs, training=True)
    assert pred.dtype == torch.float32 and float(pred.abs().max()) <= 1.0
    out, dp = fdn.ops.loss_metrics(pred, hires[0], hires[1], hires[2], mask, div_weight=0.5, non_fluid_weight=0.25, out_act=fdn.ops.ACT_TANH)
    hires64 = np.concatenate([a.astype(np.float64) for a in batch[6:9]], -1)
    mse, div_b, dz = loss_reference(pred.cpu().numpy(), hires64, batch[10], 0.5, 0.25, ACT_TANH)
    assert rel_err(out[:, 4].cpu().numpy(), div_b) <= 1e-5 and rel_err(out[:, 0].cpu().numpy(), mse) <= 1e-5
    assert rel_err(dp.cpu().numpy(), dz) <= 1e-5
    tc.reset_metrics()
    loss = tc.train_step(batch)
    assert np.isfinite(loss.cpu().numpy()).all()
    assert abs(tc.loss_metrics["train_div"].result() - div_b.mean()) <= 1e-5 * div_b.mean()
    assert abs(tc.loss_metrics["train_mse"].result() - mse.mean()) <= 1e-5 * mse.mean()
    assert math.isfinite(tc.loss_metrics["train_loss"].result())


def test_test_step_and_quicksave_report_the_weighted_loss(fdn, tmp_path):
    P, R, LB, HB, B = 6, 2, 1, 1, 2
    tc, params = make_trainer(P, R, LB, HB, seed=4, head_scale=6.0, output_activation="tanh")
    batch = hot_corner_batch(B, P, R, 43, 20.0)
    hires64 = np.concatenate([a.astype(np.float64) for a in batch[6:9]], -1)
    mask64 = batch[10].astype(np.float64)
    pred = tc.test_step(batch).cpu().numpy().astype(np.float64)
    mse1, _, _ = weighted_loss(pred, hires64, mask64, 0.0, 1.0)
    assert abs(tc.loss_metrics["val_mse"].result() - mse1.mean()) <= 1e-5 * mse1.mean()
    tc.non_fluid_weight = 0.25                                             # set after construction: read on every call
    tc.div_weight = 0.5
    tc.reset_metrics()
    pred = tc.test_step(batch).cpu().numpy().astype(np.float64)
    mse, div_b, _ = weighted_loss(pred, hires64, mask64, 0.5, 0.25)
    assert mse.mean() < 0.9 * mse1.mean()                                  # the weight has teeth
    res = dict((k, v.result()) for k, v in tc.loss_metrics.items())
    assert abs(res["val_mse"] - mse.mean()) <= 1e-5 * mse.mean()
    assert abs(res["val_div"] - div_b.mean()) <= 1e-5 * div_b.mean()
    assert abs(res["val_loss"] - (mse + div_b).mean()) <= 1e-5 * (mse + div_b).mean()
    tc.init_model_dir(base_dir=str(tmp_path))
    ql, qa, qm, qd = tc.quicksave([batch], 1)
    assert rel_err(qm, mse) <= 1e-5 and rel_err(qd, div_b) <= 1e-5 and rel_err(ql, mse + div_b) <= 1e-5
    log = open(tc.logfile).read()
    assert "Non fluid weight: 0.25\n" in log and "Output activation: tanh\n" in log
    tc.non_fluid_weight = float("nan")
    with pytest.raises(ValueError):
        tc.test_step(batch)
    with pytest.raises(ValueError):
        tc.train_step(batch)


def test_predictor_network_with_tanh_heads(fdn):
    predictor = importlib.import_module("4dflownet_amd.predictor")
    P, R, LB, HB, B = 6, 2, 1, 1, 2
    net = predictor.prepare_network(P, R, LB, HB, output_activation="tanh")
    twin = predictor.prepare_network(P, R, LB, HB)
    assert net.output_activation == "tanh" and twin.output_activation == "linear"
    weights = [w * (8.0 if w.ndim == 5 and w.shape[-1] == 1 else 1.0) for w in twin.get_weights()]
    twin.set_weights(weights)
    net.set_weights(weights)
    batch = hot_corner_batch(B, P, R, 47, 20.0)
    inputs = [dev(a) for a in batch[:6]]
    z = twin.forward(inputs).cpu().numpy()
    y = net.forward(inputs).cpu().numpy()
    ref = np.tanh(z.astype(np.float64)).astype(np.float32)
    assert np.abs(z).max() >= 9.02 and np.median(np.abs(z)) < 2
    assert ulp_distance(y, ref).max() <= TANH_ULP_BOUND
    assert (np.abs(y) <= 1).all() and (y[np.abs(z) >= 9.02] == np.sign(z[np.abs(z) >= 9.02])).all()

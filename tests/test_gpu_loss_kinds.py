"""The data term's penalties (mae, huber, charbonnier) on the GPU: fdn_loss_metrics_kind, ops.loss_metrics(kind=) and
TrainerController(loss=) against the float64 restatement in tests/_loss_kinds.py, and the default ('mse') against the calls it always made,
bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import flownet_oracle as O
from _guarded import NAN, SENTINEL, guarded, guarded_like, intact, unchanged
from _kink import kink_sides
from _loss_kinds import ACT_NONE, ACT_TANH, KINDS, loss_reference, rho_psi, voxel_weight
from test_gpu_output_activation import call_act, dev, loss_case, make_trainer, rel_err

pytestmark = pytest.mark.gpu

# several blocks per sample, a ragged last block, a one-voxel axis for the clamped stencil, non-cubic extents
SHAPES = [(2, 6, 6, 6), (1, 1, 4, 5), (3, 5, 7, 9), (2, 3, 130, 2)]
REAL_GRID = (8, 24, 24, 24)
KIND_CASES = [("mae", None), ("huber", 0.25), ("huber", 1.0), ("charbonnier", 1e-3), ("charbonnier", 2.0 ** -10)]
# Every element of dpred (div_weight = 0) within this many fp32 roundings (2^-24 relative each) of its float64 value: one for d, up to four
# for psi (square, add, sqrt, divide), seven for the voxel weight m inv_f + nf inv_nf, one for the product, one for 1 - y^2, one for its
# product.  numpy's fp32 emulation of that path stays below 4 (tests/test_loss_kinds_host.py); the GPU's worst ratio is printed per case
# and recorded in profiles/loss_kinds.txt.
DPRED_ROUNDINGS = 16


def f32(x):
    """The parameter as the entry point receives it: a C float."""
    return None if x is None else float(np.float32(x))


def planted_residuals(kind, param):
    """d = 0, |d| = 2^-20, and |d| exactly the parameter (0.25 for mae, which has none) and one fp32 step to either side of it, both signs."""
    p = np.float32(0.25 if param is None else param)
    mags = [np.float32(2.0 ** -20), p, np.nextafter(p, np.float32(4)), np.nextafter(p, np.float32(0))]
    return [np.float32(0)] + [s * m for m in mags for s in (np.float32(1), np.float32(-1))]


@functools.lru_cache(maxsize=None)
def planted_case(shape, mask_kind, kind, param):
    """loss_case's operands with the residuals above planted so that pred - truth IS the wanted value in fp32 (and in float64): the
    truth's component becomes 0, or -+0.5 where the prediction would leave [-1, 1].  Returns numpy operands, device copies and the flat
    indices (into pred) of the planted components with their residuals."""
    (pred, truth, mask), _ = loss_case(shape, mask_kind)
    pred = pred.copy()
    truth = [t.copy() for t in truth]
    nvox = mask.size
    where = []
    for k, d in enumerate(planted_residuals(kind, param)):
        vox, c = (3 * k + 1) % nvox, k % 3
        for T in (np.float32(0), np.float32(-0.5) * np.sign(d)):
            y = np.float32(T + d)
            if abs(y) <= 1 and float(y) - float(T) == float(d):
                break
        else:
            raise AssertionError((d, "no exact placement"))
        truth[c].reshape(-1)[vox] = T
        pred.reshape(-1, 3)[vox, c] = y
        where.append((vox * 3 + c, float(d)))
    assert len(set(i for i, _ in where)) == len(where)
    got = (pred.astype(np.float64) - np.stack(truth, -1).astype(np.float64)).reshape(-1)
    assert all(got[i] == d for i, d in where)
    assert np.array_equal((pred - np.stack(truth, -1)).reshape(-1)[[i for i, _ in where]], np.array([d for _, d in where], np.float32))
    return (pred, truth, mask), (dev(pred), [dev(t) for t in truth], dev(mask)), where


@functools.lru_cache(maxsize=None)
def planted_ref(shape, mask_kind, kind, param, div_weight, non_fluid_weight, out_act):
    (pred, truth, mask), _, _ = planted_case(shape, mask_kind, kind, param)
    hires = np.stack(truth, -1).astype(np.float64)
    data_b, div_b, dz = loss_reference(pred, hires, mask, kind, f32(param), div_weight, non_fluid_weight, out_act)
    return data_b, div_b, dz, O.relative_error(pred, hires.astype(np.float32), mask)


def check_against_float64(fdn, shape, mask_kind, kind, param, div_weight, non_fluid_weight, out_act):
    (pred, truth, mask), (p, t, m), where = planted_case(shape, mask_kind, kind, param)
    kw = dict(div_weight=div_weight, non_fluid_weight=non_fluid_weight, out_act=out_act, kind=kind, kind_param=param)
    out, dp = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, **kw)
    assert tuple(out.shape) == (shape[0], 5)
    out = out.cpu().numpy().astype(np.float64)
    dp = dp.cpu().numpy()
    data_b, div_b, dz, rel = planted_ref(shape, mask_kind, kind, param, div_weight, non_fluid_weight, out_act)
    figures = [rel_err(out[:, 0], data_b), rel_err(out[:, 1], rel), rel_err(dp, dz)]
    assert figures[0] <= 1e-5
    assert figures[1] <= 2e-3                              # (the metric rounds to 1e-4 steps)
    assert rel_err(out[:, 2], mask.astype(np.float64).sum((1, 2, 3))) <= 1e-5
    assert rel_err(out[:, 3], (mask < 0.5).sum((1, 2, 3))) <= 1e-5
    if div_weight:
        assert rel_err(out[:, 4], div_b) <= 1e-5, (out[:, 4], div_b)
        assert figures[2] <= 1e-5                          # the two parts cancel: the max-norm bound of the divergence tests
        worst = float("nan")
    else:
        assert (out[:, 4] == 0).all()
        zero = dz == 0
        assert (dp[zero] == 0).all(), "dpred must be exactly 0 where the reference is"
        ratio = np.abs(dp.astype(np.float64) - dz)[~zero] / np.abs(dz)[~zero]
        worst = ratio.max() / 2.0 ** -24 if ratio.size else 0.0
        flat = dp.reshape(-1)
        for i, d in where:                                 # the planted d = 0 has gradient exactly 0 whatever its weight
            if d == 0:
                assert flat[i] == 0
        assert worst <= DPRED_ROUNDINGS, worst
    print("loss %s %s %s %s div %g nf %g act %d: data %.2e metric %.2e dpred %.2e, worst element %.2f roundings"
          % (kind, param, shape, mask_kind, div_weight, non_fluid_weight, out_act, figures[0], figures[1], figures[2], worst))
    if out_act == ACT_TANH:
        assert (dp[np.abs(pred) == 1] == 0).all()          # 1 - y^2 from the output: exactly 0 at y = +-1
    # want_grad=False: the same bits, no gradient
    out2, none = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, want_grad=False, **kw)
    assert none is None and np.array_equal(out2.cpu().numpy().astype(np.float64), out)
    return worst


@pytest.mark.parametrize("out_act", [ACT_NONE, ACT_TANH])
@pytest.mark.parametrize("div_weight", [0.0, 0.8])
@pytest.mark.parametrize("non_fluid_weight", [0.0, 0.25, 1.0, 3.0])
@pytest.mark.parametrize("mask_kind", ["binary", "fractional"])
@pytest.mark.parametrize("kind,param", KIND_CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_float64(fdn, shape, kind, param, mask_kind, non_fluid_weight, div_weight, out_act):
    check_against_float64(fdn, shape, mask_kind, kind, param, div_weight, non_fluid_weight, out_act)


@pytest.mark.parametrize("div_weight", [0.0, 0.8])
@pytest.mark.parametrize("kind,param", KIND_CASES)
def test_kernel_matches_float64_on_the_real_grid(fdn, kind, param, div_weight):
    check_against_float64(fdn, REAL_GRID, "fractional", kind, param, div_weight, 0.25, ACT_TANH)


# ------------------------------------------------------------------------------------------------------------- the default, bit for bit
def call_kind(fdn, p, t, m, kind, param, div_weight, non_fluid_weight, out_act, want_grad=True, bufs=None):
    N, D, H, W = p.shape[:4]
    out, dp, scratch = bufs or (torch.empty((N, 5), device="cuda"), torch.empty_like(p), torch.empty((N * (8 + 5 * 256),), device="cuda"))
    lib = fdn._lib.load()
    rc = lib.fdn_loss_metrics_kind(p.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), m.data_ptr(), KINDS[kind],
                                   0.0 if param is None else param, div_weight, non_fluid_weight, out_act, out.data_ptr(),
                                   dp.data_ptr() if want_grad else None, scratch.data_ptr(), N, D, H, W, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.fdn_last_error()
    return out, dp


@pytest.mark.parametrize("shape", [(2, 6, 6, 6), (3, 5, 7, 9), REAL_GRID])
def test_mse_kind_is_the_existing_entry_point_bit_for_bit(fdn, shape):
    _, (p, t, m) = loss_case(shape, "fractional")
    for div_weight in (0.0, 0.8):
        for nfw in (1.0, 0.25):
            for act in (ACT_NONE, ACT_TANH):
                ref, dref = call_act(fdn, p, t, m, div_weight, nfw, act)
                out, dp = call_kind(fdn, p, t, m, "mse", None, div_weight, nfw, act)
                torch.cuda.synchronize()
                assert torch.equal(out, ref) and torch.equal(dp, dref), (div_weight, nfw, act)
    # through ops.loss_metrics: kind='mse' is the plain call, (N,4) shape included
    plain, dp_plain = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m)
    named, dp_named = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, kind="mse")
    zero, dp_zero = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, kind="mse", kind_param=0)
    assert tuple(plain.shape) == tuple(named.shape) == tuple(zero.shape) == (shape[0], 4)
    assert torch.equal(plain, named) and torch.equal(dp_plain, dp_named) and torch.equal(plain, zero) and torch.equal(dp_plain, dp_zero)
    out, dp = call_kind(fdn, p, t, m, "mse", None, 0.0, 1.0, ACT_NONE)
    assert torch.equal(out[:, :4], plain) and torch.equal(dp, dp_plain) and (out[:, 4] == 0).all()
    for div_weight, nfw, act in ((0.8, 1.0, ACT_NONE), (0.8, 0.25, ACT_TANH)):
        a = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, div_weight=div_weight, non_fluid_weight=nfw, out_act=act)
        b = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, div_weight=div_weight, non_fluid_weight=nfw, out_act=act, kind="mse")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and tuple(a[0].shape) == (shape[0], 5)


# ------------------------------------------------------------------------------------------------------------- determinism and limits
@pytest.mark.parametrize("kind,param", KIND_CASES)
def test_two_calls_give_the_same_bits(fdn, kind, param):
    _, (p, t, m) = loss_case(REAL_GRID, "fractional")
    a = call_kind(fdn, p, t, m, kind, param, 0.8, 0.25, ACT_TANH)
    b = call_kind(fdn, p, t, m, kind, param, 0.8, 0.25, ACT_TANH)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), REAL_GRID])
def test_huber_above_every_residual_is_half_the_mse(fdn, shape):
    """|d| < 2 on these operands: with delta = 4 every residual is in the quadratic branch, rho = d^2 / 2 and psi = d.  Halving is exact
    in fp32, so the column and every element of dpred equal half the MSE call's within one rounding."""
    (pred, truth, mask), (p, t, m) = loss_case(shape, "fractional")
    assert np.abs(pred - np.stack(truth, -1)).max() < 2
    for div_weight, nfw, act in ((0.0, 1.0, ACT_NONE), (0.0, 0.25, ACT_TANH)):
        mse, dmse = call_kind(fdn, p, t, m, "mse", None, div_weight, nfw, act)
        hub, dhub = call_kind(fdn, p, t, m, "huber", 4.0, div_weight, nfw, act)
        half = 0.5 * mse[:, 0].cpu().numpy().astype(np.float64)
        got = hub[:, 0].cpu().numpy().astype(np.float64)
        print("huber delta 4 %s: column 0 differs from MSE / 2 by at most %.2f ulp" % (shape, (np.abs(got - half) / np.spacing(np.float32(half))).max()))
        assert (np.abs(got - half) <= np.spacing(np.float32(half))).all(), (got, half)
        dhalf = 0.5 * dmse.cpu().numpy().astype(np.float64)
        dgot = dhub.cpu().numpy().astype(np.float64)
        assert (np.abs(dgot - dhalf) <= np.spacing(np.abs(dhalf).astype(np.float32))).all()
        assert torch.equal(hub[:, 1:4], mse[:, 1:4])       # the metric and the counts do not depend on the kind


def test_charbonnier_tends_to_mae_as_epsilon_vanishes(fdn):
    """0 <= sqrt(d^2 + eps^2) - |d| <= eps, with equality on the right at d = 0: column 0 exceeds MAE's by at most eps * 3 * (sum of the voxel
    weights), and where the prediction IS the truth it is exactly that and MAE's is 0.  At eps = 2^-20, against float64 (not against
    the MAE kernel)."""
    eps = 2.0 ** -20
    (pred, truth, mask), (p, t, m) = loss_case((3, 5, 7, 9), "fractional")
    hires = np.stack(truth, -1).astype(np.float64)
    for nfw in (1.0, 0.25):
        cap = eps * 3 * voxel_weight(mask, nfw).sum(axis=(1, 2, 3))
        out, _ = call_kind(fdn, p, t, m, "charbonnier", eps, 0.0, nfw, ACT_NONE)
        got = out[:, 0].cpu().numpy().astype(np.float64)
        ref, _, _ = loss_reference(pred, hires, mask, "charbonnier", eps, 0.0, nfw)
        mae, _, _ = loss_reference(pred, hires, mask, "mae", None, 0.0, nfw)
        assert rel_err(got, ref) <= 1e-5
        assert (ref >= mae).all() and (ref - mae <= cap).all()
        assert (got >= mae * (1 - 1e-5)).all() and (got <= (mae + cap) * (1 + 1e-5)).all()
        # pred == truth: the column is eps * 3 * (sum of the weights), every gradient exactly 0
        same = dev(np.stack(truth, -1))
        out, dp = call_kind(fdn, same, t, m, "charbonnier", eps, 0.0, nfw, ACT_NONE)
        assert rel_err(out[:, 0].cpu().numpy(), cap) <= 1e-5 and not bool(dp.any())
        out, dp = call_kind(fdn, same, t, m, "mae", None, 0.0, nfw, ACT_NONE)
        assert not bool(out[:, 0].any()) and not bool(dp.any())


# ------------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("kind,param", [("mse", None)] + KIND_CASES[:2] + KIND_CASES[3:4])
@pytest.mark.parametrize("shape", [(1, 1, 4, 5), (3, 5, 7, 9), (2, 3, 130, 2)])
def test_guard_bands(fdn, shape, kind, param, want_grad):
    """out, dpred and a scratch of exactly FDN_LOSS_DIV_SCRATCH_FLOATS(N) between intact bands, the operands unchanged -- with NaN and
    with a finite sentinel around them, the same bits both times."""
    N = shape[0]
    _, (p, t, m) = loss_case(shape, "binary")
    results = []
    for fill in (NAN, SENTINEL):
        ins = [guarded_like(x, fill) for x in (p, t[0], t[1], t[2], m)]
        snaps = [h.t.clone() for h in ins]
        out, dp, scratch = guarded((N, 5), torch.float32, fill, "cuda"), guarded(p.shape, torch.float32, fill, "cuda"), \
            guarded((N * (8 + 5 * 256),), torch.float32, fill, "cuda")
        dp_before = dp.t.clone()
        call_kind(fdn, ins[0].t, [ins[1].t, ins[2].t, ins[3].t], ins[4].t, kind, param, 0.8, 0.25, ACT_TANH, want_grad=want_grad,
                  bufs=(out.t, dp.t, scratch.t))
        torch.cuda.synchronize()
        for name, h in (("out", out), ("dpred", dp), ("scratch", scratch)):
            assert intact(h), (name, h.damaged())
        for h, snap in zip(ins, snaps):
            assert intact(h) and unchanged(h, snap)
        if not want_grad:                                  # dpred = NULL: a buffer that was not passed is not written
            assert unchanged(dp, dp_before)
        results.append((out.t.clone(), dp.t.clone()))
    assert torch.equal(results[0][0], results[1][0]) and not bool(torch.isnan(results[0][0]).any())
    if want_grad:
        assert torch.equal(results[0][1], results[1][1]) and not bool(torch.isnan(results[0][1]).any())


# ------------------------------------------------------------------------------------------------------------- train step
TRAIN_CASES = [(6, 2, 1, 1, 2, "mae", None, {}), (6, 2, 1, 1, 2, "huber", 0.25, {}), (6, 2, 1, 1, 2, "charbonnier", 1e-3, {}),
               (4, 3, 0, 1, 1, "mae", None, {}), (4, 3, 0, 1, 1, "huber", 0.25, {}), (4, 3, 0, 1, 1, "charbonnier", 1e-3, {}),
               (6, 2, 1, 1, 2, "huber", 0.25, dict(output_activation="tanh", non_fluid_weight=0.25, div_weight=0.5))]


@pytest.mark.parametrize("P,R,LB,HB,B,kind,param,more", TRAIN_CASES)
def test_train_step_matches_float64(fdn, P, R, LB, HB, B, kind, param, more):
    """Layer by layer against the float64 oracle, as test_gpu_output_activation.test_train_step_matches_float64.  mae has a kink at d = 0:
    like the activations' kinks, the reference gradient takes each residual's sign from the side the GPU's prediction landed on, and the
    residuals whose sign differs from the float64 forward's are counted and bounded (the inputs have none within 1e-5 of 0; the
    forward's error is bounded at 1e-4 of max |z| below)."""
    tanh = more.get("output_activation") == "tanh"
    nfw, div_weight = more.get("non_fluid_weight", 1.0), more.get("div_weight", 0.0)
    tc, params = make_trainer(P, R, LB, HB, seed=2, loss=kind, loss_param=param, **more)
    assert tc.loss == kind and tc.loss_param == param
    batch = O.synthetic_batch(B, P, R, seed=41)
    b64 = tuple(a.astype(np.float64) for a in batch)
    inputs, hires, venc, mask = tc._unpack(batch)
    pred = tc.model.forward(inputs, training=True)
    ref_z, rc = O.network_forward(params, b64[:6], R, LB, HB, f32_coeffs=True)
    ref_pred = np.tanh(ref_z) if tanh else ref_z
    sides, flips, worst = kink_sides(tc.model._cache, rc)
    assert flips <= 2 and worst <= 2e-5, (flips, worst)
    pred_np = pred.cpu().numpy()
    assert rel_err(pred_np, ref_pred) < 1e-4
    hires64 = np.concatenate(b64[6:9], -1)
    d_ref = ref_pred - hires64
    sign = None
    if kind == "mae":
        sign = np.sign(pred_np.astype(np.float64) - hires64)                # exact: the kernel's fp32 difference has this sign
        differ = int((sign != np.sign(d_ref)).sum())
        print("train step mae %s: %d of %d residuals on the other side of 0 than in float64, smallest |d| %.2e"
              % ((P, R, LB, HB, B), differ, d_ref.size, np.abs(d_ref).min()))
        assert differ <= 2, differ
    if kind == "huber":
        inner = (np.abs(d_ref) <= param).mean()
        assert 0.05 < inner < 0.95, inner                                     # both branches populated
    data_b, div_b, dz = loss_reference(ref_pred, hires64, b64[10], kind, f32(param), div_weight, nfw, ACT_TANH if tanh else ACT_NONE, sign=sign)
    grads = O.network_backward(params, rc, dz, R, LB, HB, f32_coeffs=True, sides=sides)
    for g, p in zip(grads, params):
        g["w"] = g["w"] + (B * 2 * O.L2_LAMBDA) * p["w"]
    gref = O.flatten(grads)
    l2 = O.l2_regularizer(params)
    w_before = tc.model.flat_w.cpu().numpy().astype(np.float64)
    tc.reset_metrics()
    loss = tc.train_step(batch)
    g = tc.model.flat_g.cpu().numpy().astype(np.float64)                    # backward's gradient (Adam reads it, L2 added inside)
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
    print("train step %s %s %s: flips %d, worst kernel-gradient error %.2e" % (kind, param, (P, R, LB, HB, B), flips, worst_g))
    assert rel_err(loss.cpu().numpy(), data_b + div_b + l2) < 1e-4
    w_ref = O.flatten(params).copy()
    O.adam_step_tf(w_ref, gref, np.zeros_like(gref), np.zeros_like(gref), 1, 1e-3)
    w_after = tc.model.flat_w.cpu().numpy().astype(np.float64)
    good = np.abs(gref) >= 1e-3 * np.abs(gref).max()
    assert np.abs(w_after - w_before).max() <= 2.1e-3
    assert np.abs(w_after - w_ref)[good].max() <= 1e-5, np.abs(w_after - w_ref)[good].max()
    res = dict((k, v.result()) for k, v in tc.loss_metrics.items())
    assert abs(res["train_mse"] - data_b.mean()) <= 1e-4 * abs(data_b.mean())         # the column keeps its name, it holds the data term
    if div_weight:
        assert abs(res["train_div"] - div_b.mean()) <= 1e-4 * abs(div_b.mean())
    else:
        assert res["train_div"] == 0.0


def test_test_step_and_quicksave_report_the_chosen_loss(fdn, tmp_path):
    P, R, LB, HB, B = 6, 2, 1, 1, 2
    tc, _ = make_trainer(P, R, LB, HB, seed=4, loss="huber", loss_param=0.25)
    plain, _ = make_trainer(P, R, LB, HB, seed=4)
    named, _ = make_trainer(P, R, LB, HB, seed=4, loss="mse", loss_param=None)
    batch = O.synthetic_batch(B, P, R, seed=43)
    hires64 = np.concatenate([a.astype(np.float64) for a in batch[6:9]], -1)
    mask64 = batch[10].astype(np.float64)
    pred = tc.test_step(batch).cpu().numpy().astype(np.float64)
    hub, _, _ = loss_reference(pred, hires64, mask64, "huber", 0.25)
    mse, _, _ = loss_reference(pred, hires64, mask64, "mse")
    assert hub.mean() < 0.5 * mse.mean()                                   # another loss, not the MSE under another name
    res = dict((k, v.result()) for k, v in tc.loss_metrics.items())
    assert abs(res["val_mse"] - hub.mean()) <= 1e-5 * hub.mean() and abs(res["val_loss"] - hub.mean()) <= 1e-5 * hub.mean()
    tc.init_model_dir(base_dir=str(tmp_path / "huber"))
    ql, qa, qm, qd = tc.quicksave([batch], 1)
    assert rel_err(qm, hub) <= 1e-5 and rel_err(ql, hub) <= 1e-5
    log = open(tc.logfile).read()
    assert "Loss: huber (delta=0.25)\n" in log
    # the attributes are read on every call: charbonnier with the divergence term from now on
    tc.loss, tc.loss_param, tc.div_weight = "charbonnier", None, 0.5
    tc.reset_metrics()
    pred = tc.test_step(batch).cpu().numpy().astype(np.float64)
    cha, div_b, _ = loss_reference(pred, hires64, mask64, "charbonnier", f32(1e-3), 0.5)
    res = dict((k, v.result()) for k, v in tc.loss_metrics.items())
    assert abs(res["val_mse"] - cha.mean()) <= 1e-5 * cha.mean() and abs(res["val_div"] - div_b.mean()) <= 1e-5 * div_b.mean()
    assert abs(res["val_loss"] - (cha + div_b).mean()) <= 1e-5 * (cha + div_b).mean()
    ql, qa, qm, qd = tc.quicksave([batch], 2)
    assert rel_err(qm, cha) <= 1e-5 and rel_err(qd, div_b) <= 1e-5 and rel_err(ql, cha + div_b) <= 1e-5
    tc.loss = "l1"
    with pytest.raises(ValueError):
        tc.test_step(batch)
    with pytest.raises(ValueError):
        tc.train_step(batch)
    # the default's log file: the header of a trainer built without the arguments, byte for byte, and no line about the loss
    plain.init_model_dir(base_dir=str(tmp_path / "plain"))
    named.init_model_dir(base_dir=str(tmp_path / "named"))
    a, b = open(plain.logfile, "rb").read(), open(named.logfile, "rb").read()
    assert a == b and b"Loss:" not in a
    head = log[:log.index("epoch, ")]
    assert head.replace("Loss: huber (delta=0.25)\n", "") == a.decode()[:a.decode().index("epoch, ")]      # one line more, nothing else
    mae, _ = make_trainer(P, R, LB, HB, seed=4, loss="mae")
    mae.init_model_dir(base_dir=str(tmp_path / "mae"))
    assert "Loss: mae\n" in open(mae.logfile).read()


def test_bf16_mode(fdn):
    """One step in bf16 mode at the bounds of test_gpu_output_activation.test_bf16_mode: the loss pass sees the fp32 prediction."""
    P, R, LB, HB, B = 8, 2, 1, 1, 2
    tc, _ = make_trainer(P, R, LB, HB, seed=3, dtype="bfloat16", div_weight=0.5, non_fluid_weight=0.25, loss="charbonnier")
    assert tc.model.act_dtype == torch.bfloat16
    batch = O.synthetic_batch(B, P, R, seed=31)
    inputs, hires, venc, mask = tc._unpack(batch)
    pred = tc.model.forward(inputs, training=True)
    assert pred.dtype == torch.float32
    out, dp = fdn.ops.loss_metrics(pred, hires[0], hires[1], hires[2], mask, div_weight=0.5, non_fluid_weight=0.25, kind="charbonnier")
    hires64 = np.concatenate([a.astype(np.float64) for a in batch[6:9]], -1)
    data_b, div_b, dz = loss_reference(pred.cpu().numpy(), hires64, batch[10], "charbonnier", f32(1e-3), 0.5, 0.25)
    assert rel_err(out[:, 4].cpu().numpy(), div_b) <= 1e-5 and rel_err(out[:, 0].cpu().numpy(), data_b) <= 1e-5
    assert rel_err(dp.cpu().numpy(), dz) <= 1e-5
    tc.reset_metrics()
    loss = tc.train_step(batch)
    assert np.isfinite(loss.cpu().numpy()).all()
    assert abs(tc.loss_metrics["train_div"].result() - div_b.mean()) <= 1e-5 * div_b.mean()
    assert abs(tc.loss_metrics["train_mse"].result() - data_b.mean()) <= 1e-5 * data_b.mean()
    assert math.isfinite(tc.loss_metrics["train_loss"].result())


def test_changing_the_loss_between_two_steps(fdn):
    """The attribute is read on every step: a trainer switched to huber after its first (mse) step then takes the step of a trainer that was
    built with huber and took the same first step under mse -- equal state before, equal bits after -- and not the mse step."""
    P, R, LB, HB, B = 6, 2, 1, 1, 2
    batch = O.synthetic_batch(B, P, R, seed=41)
    a, _ = make_trainer(P, R, LB, HB, seed=2)
    b, _ = make_trainer(P, R, LB, HB, seed=2, loss="huber", loss_param=0.25)
    c, _ = make_trainer(P, R, LB, HB, seed=2)
    assert torch.equal(a.model.flat_w, b.model.flat_w)
    # first step: b built with huber; a switched to it before its first step
    a.loss, a.loss_param = "huber", 0.25
    la, lb, lc = a.train_step(batch), b.train_step(batch), c.train_step(batch)
    assert torch.equal(la, lb) and torch.equal(a.model.flat_w, b.model.flat_w)
    assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v)
    assert not torch.equal(la, lc) and not torch.equal(a.model.flat_w, c.model.flat_w)
    # second step: back to mse on a, while b is set to mse too -- the same state, the same bits; c (mse all along) is somewhere else
    a.loss, a.loss_param = "mse", None
    b.loss, b.loss_param = "mse", None
    la, lb = a.train_step(batch), b.train_step(batch)
    assert torch.equal(la, lb) and torch.equal(a.model.flat_w, b.model.flat_w)
    # and from equal state a step under mse and one under huber differ only through the loss call: restore, switch, compare
    d, _ = make_trainer(P, R, LB, HB, seed=2)
    e, _ = make_trainer(P, R, LB, HB, seed=2, loss="huber", loss_param=0.25)
    e.loss, e.loss_param = "mse", None
    d.train_step(batch); e.train_step(batch)                                # equal first steps under mse
    assert torch.equal(d.model.flat_w, e.model.flat_w) and torch.equal(d.model.flat_w, c.model.flat_w)
    d.loss, d.loss_param = "huber", 0.25                                    # d switches after the step, e goes back to what it was built with
    e.loss, e.loss_param = "huber", 0.25
    ld, le = d.train_step(batch), e.train_step(batch)
    lc2 = c.train_step(batch)
    assert torch.equal(ld, le) and torch.equal(d.model.flat_w, e.model.flat_w) and torch.equal(d.optimizer.v, e.optimizer.v)
    assert not torch.equal(ld, lc2) and d.optimizer.iterations == c.optimizer.iterations == 2

"""The divergence loss on the GPU (fdn_loss_metrics_div, ops.loss_metrics(div_weight=), TrainerController(div_weight=)) against the
float64 restatement of src/Network/loss_utils.py:4-62 + src/Network/TrainerController.py:84-127 in tests/_divergence.py."""
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import flownet_oracle as O
from _divergence import divergence_loss
from _kink import kink_sides

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rel_err(got, ref):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def make_case(shape, mask_kind, seed):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(-0.5, 0.5, size=shape + (3,)).astype(np.float32)
    truth = [rng.uniform(-0.45, 0.45, size=shape).astype(np.float32) for _ in range(3)]
    if mask_kind == "binary":
        mask = (rng.uniform(size=shape) < 0.3).astype(np.float32)
    else:
        mask = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), size=shape)
        mask.reshape(-1)[::7] = 0.5                        # exactly on the non-fluid threshold
    return pred, truth, mask


SHAPES = [(2, 6, 6, 6), (1, 1, 4, 5), (2, 3, 2, 7), (3, 5, 7, 9), (8, 48, 48, 48), (1, 128, 128, 128)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mask_kind", ["binary", "fractional"])
def test_kernel_matches_float64(fdn, shape, mask_kind):
    pred, truth, mask = make_case(shape, mask_kind, seed=sum(shape) + len(mask_kind))
    wgt = 0.8
    out, dp = fdn.ops.loss_metrics(dev(pred), dev(truth[0]), dev(truth[1]), dev(truth[2]), dev(mask), div_weight=wgt)
    assert tuple(out.shape) == (shape[0], 5)
    out = out.cpu().numpy().astype(np.float64)
    hires = np.stack(truth, -1).astype(np.float64)
    mse, dp_mse = O.masked_mse_loss_fwd_bwd(pred.astype(np.float64), hires, mask.astype(np.float64))
    rel = O.relative_error(pred, hires.astype(np.float32), mask)
    div_b, dp_div = divergence_loss(pred, hires, mask, wgt)
    assert rel_err(out[:, 0], mse) <= 1e-5
    assert rel_err(out[:, 1], rel) <= 2e-3                 # (the metric rounds to 1e-4 steps)
    assert rel_err(out[:, 2], mask.astype(np.float64).sum((1, 2, 3))) <= 1e-5
    assert rel_err(out[:, 3], (mask < 0.5).sum((1, 2, 3))) <= 1e-5
    assert rel_err(out[:, 4], div_b) <= 1e-5, (out[:, 4], div_b)
    ref = dp_mse + dp_div
    assert rel_err(dp.cpu().numpy(), ref) <= 1e-5
    # want_grad=False: the same values, no gradient
    out2, none = fdn.ops.loss_metrics(dev(pred), dev(truth[0]), dev(truth[1]), dev(truth[2]), dev(mask), want_grad=False, div_weight=wgt)
    assert none is None and rel_err(out2.cpu().numpy()[:, 4], div_b) <= 1e-5


def _call_div(fdn, pred, truth, mask, wgt):
    N, D, H, W = pred.shape[:4]
    out = torch.empty((N, 5), device="cuda")
    dp = torch.empty_like(pred)
    scratch = torch.empty((N * (8 + 5 * 256),), device="cuda")
    rc = fdn._lib.load().fdn_loss_metrics_div(pred.data_ptr(), truth[0].data_ptr(), truth[1].data_ptr(), truth[2].data_ptr(),
                                             mask.data_ptr(), wgt, out.data_ptr(), dp.data_ptr(), scratch.data_ptr(), N, D, H, W,
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, fdn._lib.load().fdn_last_error()
    return out, dp


@pytest.mark.parametrize("shape", [(2, 6, 6, 6), (8, 24, 24, 24), (3, 5, 7, 9)])
def test_weight_zero_is_the_plain_loss_bit_for_bit(fdn, shape):
    pred, truth, mask = make_case(shape, "fractional", seed=5)
    p, t, m = dev(pred), [dev(x) for x in truth], dev(mask)
    plain, dp_plain = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m)
    out, dp = _call_div(fdn, p, t, m, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :4], plain) and torch.equal(dp, dp_plain)
    assert (out[:, 4] == 0).all()
    # and the python surface routes weight 0 to the plain call: (N,4)
    out0, _ = fdn.ops.loss_metrics(p, t[0], t[1], t[2], m, div_weight=0.0)
    assert tuple(out0.shape) == (shape[0], 4) and torch.equal(out0, plain)


def test_deterministic_and_linear_in_the_weight(fdn):
    pred, truth, mask = make_case((8, 24, 24, 24), "binary", seed=9)
    p, t, m = dev(pred), [dev(x) for x in truth], dev(mask)
    o1, d1 = _call_div(fdn, p, t, m, 1.0)
    o1b, d1b = _call_div(fdn, p, t, m, 1.0)
    assert torch.equal(o1, o1b) and torch.equal(d1, d1b)
    o2, _ = _call_div(fdn, p, t, m, 2.0)
    a = o2[:, 4].cpu().numpy()
    b = 2 * o1[:, 4].cpu().numpy()
    assert (np.abs(a - b) <= np.spacing(np.abs(b))).all(), (a, b)
    assert torch.equal(o2[:, :4], o1[:, :4])


def make_trainer(P, R, LB, HB, seed=0, wscale=3.0, **kw):
    """test_gpu_train_step.make with extra TrainerController keywords."""
    trainer_mod = importlib.import_module("4dflownet_amd.trainer")
    tc = trainer_mod.TrainerController(P, R, initial_learning_rate=1e-3, quicksave_enable=False, low_resblock=LB, hi_resblock=HB,
                                       seed=seed, **kw)
    params = O.init_params(seed, LB, HB, np.float64)
    rng = np.random.default_rng(seed + 1)
    arrays = []
    for p in params:
        p["w"] = (p["w"] * wscale).astype(np.float32).astype(np.float64)
        arrays.append(p["w"].astype(np.float32))
        if p["b"] is not None:
            p["b"] = rng.normal(0, 0.05, p["b"].shape).astype(np.float32).astype(np.float64)
            arrays.append(p["b"].astype(np.float32))
    tc.model.set_weights(arrays)
    return tc, params


@pytest.mark.parametrize("P,R,LB,HB,B", [(6, 2, 1, 1, 2), (4, 3, 0, 1, 1)])
def test_train_step_with_divergence_matches_float64(fdn, P, R, LB, HB, B):
    wgt = 0.5
    # weights at Glorot scale: a prediction of the truth's size, whose error is as rough as the truth (x3, as test_gpu_train_step scales
    # them, the smooth large prediction dominates the error and the MSE gradient outweighs the divergence gradient 6:1)
    tc, params = make_trainer(P, R, LB, HB, seed=2, wscale=1.0, div_weight=wgt)
    batch = O.synthetic_batch(B, P, R, seed=41)
    b64 = tuple(a.astype(np.float64) for a in batch)
    inputs, hires, venc, mask = tc._unpack(batch)
    pred = tc.model.forward(inputs, training=True)
    ref_pred, rc = O.network_forward(params, b64[:6], R, LB, HB, f32_coeffs=True)
    sides, flips, worst = kink_sides(tc.model._cache, rc)
    assert flips <= 2 and worst <= 2e-5, (flips, worst)
    assert rel_err(pred.cpu().numpy(), ref_pred) < 1e-4
    hires64 = np.concatenate(b64[6:9], -1)
    mse, dp_mse = O.masked_mse_loss_fwd_bwd(ref_pred, hires64, b64[10])
    div_b, dp_div = divergence_loss(ref_pred, hires64, b64[10], wgt)
    assert np.linalg.norm(dp_div) >= 0.3 * np.linalg.norm(dp_mse)        # the term has teeth
    grads = O.network_backward(params, rc, dp_mse + dp_div, R, LB, HB, f32_coeffs=True, sides=sides)
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
    for L in tc.model.layers:
        sl = slice(L.w_off, L.w_off + L.w.numel())
        assert rel_err(g_total[sl], gref[sl]) < 1e-4, (L.name, "kernel grad", rel_err(g_total[sl], gref[sl]))
        if L.b is not None:
            sb = slice(L.b_off, L.b_off + L.cout)
            assert rel_err(g_total[sb], gref[sb]) < 1e-4, (L.name, "bias grad")
    assert rel_err(loss.cpu().numpy(), mse + div_b + l2) < 1e-4
    res = dict((k, v.result()) for k, v in tc.loss_metrics.items())
    assert abs(res["train_div"] - div_b.mean()) <= 1e-4 * abs(div_b.mean())
    assert abs(res["train_mse"] - mse.mean()) <= 1e-4 * abs(mse.mean())
    assert abs(res["train_loss"] - (mse + div_b + l2).mean()) <= 1e-4 * abs((mse + div_b + l2).mean())
    assert tc.loss_metrics["train_div"]._count == B                        # the (B,) vector, as Keras' Mean takes the reference's tensor


def test_test_step_quicksave_and_log(fdn, tmp_path):
    P, R, LB, HB, B = 6, 2, 1, 1, 2
    tc, params = make_trainer(P, R, LB, HB, seed=4)
    assert tc.div_weight == 0
    batch = O.synthetic_batch(B, P, R, seed=43)
    tc.test_step(batch)
    assert tc.loss_metrics["val_div"].result() == 0.0 and tc.loss_metrics["val_div"]._count == 1     # weight 0: as before
    tc.div_weight = 0.5                                                    # set after construction: read on every call
    tc.reset_metrics()
    pred = tc.test_step(batch).cpu().numpy().astype(np.float64)
    hires64 = np.concatenate([a.astype(np.float64) for a in batch[6:9]], -1)
    mask64 = batch[10].astype(np.float64)
    div_b, _ = divergence_loss(pred, hires64, mask64, 0.5)
    mse, _ = O.masked_mse_loss_fwd_bwd(pred, hires64, mask64)
    res = dict((k, v.result()) for k, v in tc.loss_metrics.items())
    assert abs(res["val_div"] - div_b.mean()) <= 1e-5 * div_b.mean()
    assert abs(res["val_loss"] - (mse + div_b).mean()) <= 1e-5 * (mse + div_b).mean()
    assert abs(res["val_mse"] - mse.mean()) <= 1e-5 * mse.mean()
    tc.init_model_dir(base_dir=str(tmp_path))
    ql, qa, qm, qd = tc.quicksave([batch], 1)
    assert rel_err(qd, div_b) <= 1e-5 and rel_err(qm, mse) <= 1e-5 and rel_err(ql, mse + div_b) <= 1e-5
    log = open(tc.logfile).read()
    assert "Divergence weight: 0.5\n" in log
    tc2, _ = make_trainer(P, R, LB, HB, seed=4, div_weight=0.25)
    tc2.init_model_dir(base_dir=str(tmp_path / "b"))
    assert "Divergence weight: 0.25\n" in open(tc2.logfile).read()
    # a negative or non-finite weight is refused, at construction and when set later
    trainer_mod = importlib.import_module("4dflownet_amd.trainer")
    for bad in (-0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            trainer_mod.TrainerController(P, R, quicksave_enable=False, low_resblock=0, hi_resblock=1, div_weight=bad)
    tc.div_weight = -1.0
    with pytest.raises(ValueError):
        tc.test_step(batch)
    with pytest.raises(ValueError):
        tc.train_step(batch)


def test_bf16_mode_with_divergence(fdn):
    P, R, LB, HB, B = 8, 2, 1, 1, 2
    tc, _ = make_trainer(P, R, LB, HB, seed=3, dtype="bfloat16", div_weight=0.5)
    assert tc.model.act_dtype == torch.bfloat16
    batch = O.synthetic_batch(B, P, R, seed=31)
    inputs, hires, venc, mask = tc._unpack(batch)
    pred = tc.model.forward(inputs, training=True)
    assert pred.dtype == torch.float32                                     # the prediction stays fp32 in bf16 mode
    out, dp = fdn.ops.loss_metrics(pred, hires[0], hires[1], hires[2], mask, div_weight=0.5)
    hires64 = np.concatenate([a.astype(np.float64) for a in batch[6:9]], -1)
    div_b, dp_div = divergence_loss(pred.cpu().numpy(), hires64, batch[10], 0.5)
    assert rel_err(out[:, 4].cpu().numpy(), div_b) <= 1e-5
    tc.reset_metrics()
    loss = tc.train_step(batch)
    assert np.isfinite(loss.cpu().numpy()).all()
    assert abs(tc.loss_metrics["train_div"].result() - div_b.mean()) <= 1e-5 * div_b.mean()
    assert math.isfinite(tc.loss_metrics["train_loss"].result())

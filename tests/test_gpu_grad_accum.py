"""Gradient accumulation on the GPU: fdn_grad_accumulate bit for bit against numpy, and TrainerController(accum_steps=K) against the
sum of its micro-batch gradients (exact), the big batch (the data-parallel test's tolerances: the same regrouping of partial sums) and
the float64 oracle.

Semantics under test (src/Network/TrainerController.py:223,245-249): tape.gradient of the (B,) loss vector = gradient of sum_b loss_b
with the scalar L2 term counted once per sample -> K micro-batches of B/K are one batch of B: SUM of the gradient buffers, batch-size
slot included."""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import flownet_oracle as O
from _kink import kink_sides

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")

P, R, LB, HB = 8, 2, 1, 1          # the data-parallel test's configuration (tests/test_gpu_parallel.py)
LR = 1e-4


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _nbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _tc(trainer, **kw):
    return trainer.TrainerController(P, R, initial_learning_rate=LR, quicksave_enable=False, low_resblock=LB, hi_resblock=HB, seed=0, **kw)


def _rows(batch, rows):
    return tuple(a[rows] for a in batch)


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _operands(n, seed):
    """standard normal scaled over 2^+-20 (no subnormal input, and a sum of two such values is 0 or >= 2^-24 of the larger: no subnormal
    result), with exact zeros of both signs and +-inf sprinkled in -- inf - inf gives the NaN positions."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        a = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n))).astype(np.float32)
        special = np.array([0.0, -0.0, np.inf, -np.inf], np.float32)
        hit = rng.random(n) < 0.15
        a[hit] = special[rng.integers(0, 4, int(hit.sum()))]
        out.append(a)
    if n >= 4:                                                       # one of each by construction: -0 + -0, +0 + -0, inf - inf, inf + inf
        out[0][:4] = (-0.0, 0.0, np.inf, np.inf)
        out[1][:4] = (-0.0, -0.0, -np.inf, np.inf)
    assert all(np.all((a == 0) | ~np.isfinite(a) | (np.abs(a) >= np.finfo(np.float32).tiny)) for a in out)
    return out


def _check_sum(got_bits, a, g):
    with np.errstate(invalid="ignore"):
        want = a.astype(np.float32) + g
    nan = np.isnan(want)
    got = got_bits.view(np.float32)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got_bits[~nan], _nbits(want)[~nan])
    assert np.all((want[~nan] == 0) | ~np.isfinite(want[~nan]) | (np.abs(want[~nan]) >= np.finfo(np.float32).tiny))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 * 256 + 3])      # a block edge on either side; one element past what 4096 blocks cover in one trip
def test_grad_accumulate_is_a_bit_copy_then_numpy_float32_addition(fdn, n):
    a, g = _operands(n, seed=n)
    dg = torch.from_numpy(g).cuda()
    acc = torch.full((n,), float("nan"), device="cuda")
    fdn.ops.grad_accumulate(acc, dg, True)
    assert np.array_equal(_bits(acc), _nbits(g))                      # first = 1: whatever acc held
    acc.copy_(torch.from_numpy(a))
    fdn.ops.grad_accumulate(acc, dg, False)
    once = _bits(acc)
    _check_sum(once, a, g)
    acc.copy_(torch.from_numpy(a))                                   # two identical calls on identical inputs
    fdn.ops.grad_accumulate(acc, dg, False)
    assert np.array_equal(_bits(acc), once)
    assert np.array_equal(_bits(dg), _nbits(g))                      # g is only read


@pytest.mark.parametrize("oa,og", [(0, 0), (1, 0), (0, 3), (2, 1), (3, 3)])
def test_grad_accumulate_at_any_float_offset_leaves_its_neighbours_alone(fdn, oa, og):
    n, pad = 257, 8
    a, g = _operands(n, seed=7)
    canary = np.float32(-12345.678)
    for first in (True, False):
        big_a = torch.full((n + 2 * pad,), float(canary), device="cuda")
        big_g = torch.full((n + 2 * pad,), 777.0, device="cuda")
        acc, dg = big_a[pad + oa:pad + oa + n], big_g[pad + og:pad + og + n]
        assert (acc.data_ptr() // 4) % 4 == oa and (dg.data_ptr() // 4) % 4 == og          # float offsets from a 16-byte boundary
        acc.copy_(torch.from_numpy(a))
        dg.copy_(torch.from_numpy(g))
        fdn.ops.grad_accumulate(acc, dg, first)
        if first:
            assert np.array_equal(_bits(acc), _nbits(g))
        else:
            _check_sum(_bits(acc), a, g)
        whole = _bits(big_a)
        lo = pad + oa
        assert np.all(whole[:lo] == _nbits(canary)) and np.all(whole[lo + n:] == _nbits(canary))


def test_grad_accumulate_accepts_adjacent_ranges_and_refuses_overlapping_ones(fdn):
    n = 257
    a, g = _operands(n, seed=11)
    buf = torch.empty(2 * n, device="cuda")
    buf[:n].copy_(torch.from_numpy(a))
    buf[n:].copy_(torch.from_numpy(g))
    fdn.ops.grad_accumulate(buf[:n], buf[n:], False)                  # g = acc + 4 n bytes: the first distance that is no overlap
    _check_sum(_bits(buf[:n]), a, g)
    fdn.ops.grad_accumulate(buf[n:], buf[:n], True)                   # and g = acc - 4 n bytes
    assert np.array_equal(_bits(buf[n:]), _bits(buf[:n]))
    before = _bits(buf)
    for acc, src in ((buf[:n], buf[:n]), (buf[:n], buf[1:n + 1]), (buf[n - 1:2 * n - 1], buf[:n])):
        with pytest.raises(fdn.FdnError, match="overlap"):
            fdn.ops.grad_accumulate(acc, src, False)
    assert np.array_equal(_bits(buf), before)


# ------------------------------------------------------------------------------------------------ 2.-4. one group of two micro-batches
def _run_group(trainer, overlap=True, keep_caches=False, **kw):
    """accum_steps = 2 on the global batch of 4 (seed 31) fed as rows [0,1] then [2,3]; everything the cases below look at."""
    tc = _tc(trainer, accum_steps=2, **kw)
    if not overlap:
        tc.model.overlap_wgrad = False
    gb = O.synthetic_batch(4, P, R, seed=31)
    state = lambda: [_bits(tc.model.flat_w), _bits(tc.optimizer.m), _bits(tc.optimizer.v), tc.optimizer.iterations, tc.model.weights_version]
    caches = []
    if keep_caches:                                                  # the activations of each micro-batch's forward, for kink_sides
        backward = tc.model.backward

        def keeping(dpred, grad_ready=None):
            c = tc.model._cache
            cpu = lambda t: t.float().cpu()
            caches.append(dict([(k, cpu(c[k])) for k in ("a0", "a1", "p0", "p1", "c0", "c1")] +
                               [("blocks", [(None, cpu(h), cpu(out)) for _, h, out in c["blocks"]]), ("heads", [cpu(g) for g in c["heads"]])]))
            return backward(dpred, grad_ready=grad_ready)
        tc.model.backward = keeping
    r = {"tc": tc, "gb": gb, "before": state(), "w0": _np(tc.model.flat_w)}
    tc.train_step(_rows(gb, [0, 1]))
    r["snap1"] = _np(tc.model.flat_g_ext)
    r["after1"] = state()
    r["acc1"] = _np(tc.accum_g_ext)
    tc.train_step(_rows(gb, [2, 3]))
    r["snap2"] = _np(tc.model.flat_g_ext)
    r["after2"] = state()
    r["acc"] = _np(tc.accum_g_ext)
    r["w"] = _np(tc.model.flat_w)
    r["metrics"] = dict((k, v.result()) for k, v in tc.loss_metrics.items())
    r["caches"] = caches
    return r


@pytest.fixture(scope="module")
def group():
    return _run_group(importlib.import_module("4dflownet_amd.trainer"), keep_caches=True)


@pytest.fixture(scope="module")
def big():
    """A fresh controller that takes the same 4 rows in one train_step."""
    tc = _tc(importlib.import_module("4dflownet_amd.trainer"))
    tc.train_step(O.synthetic_batch(4, P, R, seed=31))
    return {"g": _np(tc.model.flat_g_ext), "w": _np(tc.model.flat_w), "metrics": dict((k, v.result()) for k, v in tc.loss_metrics.items())}


def _check_group_is_the_sum_of_its_micro_batches(r):
    assert r["snap1"][-1] == 2.0 and r["snap2"][-1] == 2.0            # flat_g_ext keeps the micro-batch's own gradient and batch size
    assert not np.array_equal(r["snap1"], r["snap2"])
    assert np.array_equal(_nbits(r["acc1"]), _nbits(r["snap1"]))      # first = 1: a copy
    assert np.array_equal(_nbits(r["acc"]), _nbits(r["snap1"] + r["snap2"]))
    assert r["acc"][-1] == 4.0
    # call 1 moved nothing: weights, Adam slots, iterations, the weights' version (and with it the packs)
    for k in range(3):
        assert np.array_equal(r["after1"][k], r["before"][k])
    assert r["after1"][3] == r["before"][3] == 0 and r["after1"][4] == r["before"][4]
    # call 2: exactly one optimiser step
    assert r["after2"][3] == 1 and r["after2"][4] == r["before"][4] + 1
    assert not np.array_equal(r["after2"][0], r["before"][0])
    assert np.abs(r["w"].astype(np.float64) - r["w0"]).max() <= 1.05 * LR    # |Adam's first update| <= lr


def test_group_equals_the_sum_of_its_micro_batches(group):
    _check_group_is_the_sum_of_its_micro_batches(group)


def test_group_equals_the_sum_of_its_micro_batches_on_one_stream(group):
    r = _run_group(importlib.import_module("4dflownet_amd.trainer"), overlap=False)
    _check_group_is_the_sum_of_its_micro_batches(r)
    assert np.array_equal(_nbits(r["acc"]), _nbits(group["acc"]))     # the weight-gradient stream changes no bit
    assert np.array_equal(_nbits(r["w"]), _nbits(group["w"]))


def _check_against(acc_g, w, ref_g, ref_w, steps=1):
    """tests/test_gpu_parallel.py's tolerances: gradient 1e-3 relative in L2 and max norm; weights within 2.1 lr per step (Adam moves a
    weight by ~lr sign(g) in its first steps, so an element whose gradient is summation-order noise may go either way), every
    well-conditioned element to 1e-6."""
    ref = ref_g[:-1].astype(np.float64)
    d = acc_g[:-1].astype(np.float64) - ref
    print("gradient: rel L2 %.3e, rel max %.3e" % (np.linalg.norm(d) / np.linalg.norm(ref), np.abs(d).max() / np.abs(ref).max()))
    assert np.linalg.norm(d) <= 1e-3 * np.linalg.norm(ref)
    assert np.abs(d).max() <= 1e-3 * np.abs(ref).max()
    _check_weights(w, ref_g, ref_w, steps)


def _check_weights(w, ref_g, ref_w, steps):
    dw = np.abs(w.astype(np.float64) - ref_w)
    g = np.abs(ref_g[:-1])
    good = g >= 1e-3 * g.max()
    print("weights: max |dw| %.3e (%.2f lr), well-conditioned %.1f %%, max |dw| there %.3e" % (dw.max(), dw.max() / LR, 100.0 * good.mean(), dw[good].max()))
    assert dw.max() <= 2.1 * steps * LR
    assert good.sum() > 0.2 * good.size
    assert dw[good].max() <= 1e-6


def test_group_equals_the_big_batch(group, big):
    assert big["g"][-1] == 4.0
    _check_against(group["acc"], group["w"], big["g"], big["w"])
    for k in ("train_loss", "train_mse", "train_accuracy"):
        a, b = group["metrics"][k], big["metrics"][k]
        print(k, a, b)
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-6), (k, a, b)


def test_accumulated_gradient_matches_the_float64_oracle(group):
    """The bound of tests/test_gpu_train_step.py::test_train_step_matches_oracle (tol_g = 1e-4: per layer, kernel and bias gradient
    apart, max-norm relative error of gradient + B 2 lambda w against the oracle's gradient of the loss with its L2 term, the oracle
    differentiating in the linear region the GPU forward landed in; flips <= max(2, 1e-5 units), none further than 2e-5 from its kink)."""
    tc, gb = group["tc"], group["gb"]
    params = O.init_params(0, LB, HB, np.float64)
    w0 = group["w0"]
    for p, L in zip(params, tc.model.layers):                        # the oracle starts from the fp32 values the GPU held during the group
        p["w"] = w0[L.w_off:L.w_off + L.w.numel()].reshape(p["w"].shape).astype(np.float64)
        if p["b"] is not None:
            p["b"] = w0[L.b_off:L.b_off + L.cout].astype(np.float64)
    c1, c2 = group["caches"]
    cat = lambda a, b: torch.cat([a, b], 0)
    cache4 = dict((k, cat(c1[k], c2[k])) for k in ("a0", "a1", "p0", "p1", "c0", "c1"))
    cache4["blocks"] = [(None, cat(h1, h2), cat(o1, o2)) for (_, h1, o1), (_, h2, o2) in zip(c1["blocks"], c2["blocks"])]
    cache4["heads"] = [cat(a, b) for a, b in zip(c1["heads"], c2["heads"])]
    seen = {}

    def sides_of(rc):
        sides, seen["flips"], seen["worst"] = kink_sides(cache4, rc)
        seen["units"] = sum(int(np.size(v)) for v in sides.values() if isinstance(v, np.ndarray)) + \
            sum(h.size + o.size for h, o in sides["blocks"]) + sum(g.size for g in sides["heads"])
        return sides
    ref = O.loss_and_grads(params, tuple(a.astype(np.float64) for a in gb), R, LB, HB, f32_coeffs=True, sides=sides_of)
    print("flips %d of %d units, worst %.3e" % (seen["flips"], seen["units"], seen["worst"]))
    assert seen["flips"] <= max(2, 1e-5 * seen["units"]) and seen["worst"] <= 2e-5, seen
    tol_g = 1e-4
    rel_err = lambda got, want: np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    isk = _np(tc.model.is_kernel).astype(np.float64)
    g_total = group["acc"][:-1].astype(np.float64) + 4 * 2 * O.L2_LAMBDA * w0.astype(np.float64) * isk
    gref = O.flatten(ref["grads"])
    worst = 0.0
    for L in tc.model.layers:
        sl = slice(L.w_off, L.w_off + L.w.numel())
        e = rel_err(g_total[sl], gref[sl])
        worst = max(worst, e)
        assert e < tol_g, (L.name, "kernel grad", e)
        if L.b is not None:
            sb = slice(L.b_off, L.b_off + L.cout)
            e = rel_err(g_total[sb], gref[sb])
            worst = max(worst, e)
            assert e < tol_g, (L.name, "bias grad", e)
    print("worst per-layer relative error %.3e" % worst)


# ------------------------------------------------------------------------------------------------ 5. ragged group and flush
def test_ragged_group_is_applied_by_apply_accumulated_and_a_second_call_is_a_no_op(fdn):
    trainer = importlib.import_module("4dflownet_amd.trainer")
    micro = [O.synthetic_batch(2, P, R, seed=s) for s in (31, 32, 34)]
    tc = _tc(trainer, accum_steps=2)
    for b in micro:
        tc.train_step(b)
    assert tc.optimizer.iterations == 1
    assert tc.apply_accumulated() is True
    assert tc.optimizer.iterations == 2
    assert np.array_equal(_nbits(_np(tc.accum_g_ext)), _nbits(_np(tc.model.flat_g_ext))) and _np(tc.accum_g_ext)[-1] == 2.0   # a group of one
    state = [_bits(tc.model.flat_w), _bits(tc.optimizer.m), _bits(tc.optimizer.v)]
    version = tc.model.weights_version
    assert tc.apply_accumulated() is False
    torch.cuda.synchronize()
    for a, t in zip(state, (tc.model.flat_w, tc.optimizer.m, tc.optimizer.v)):
        assert np.array_equal(a, _bits(t))
    assert tc.optimizer.iterations == 2 and tc.model.weights_version == version
    # a controller that stepped on the 4 rows of the first two micro-batches, then on the third alone
    ref = _tc(trainer)
    ref.train_step(tuple(np.concatenate([a, b], 0) for a, b in zip(micro[0], micro[1])))
    g1 = _np(ref.model.flat_g_ext)
    ref.train_step(micro[2])
    assert ref.optimizer.iterations == 2
    _check_weights(_np(tc.model.flat_w), g1, _np(ref.model.flat_w), steps=2)


# ------------------------------------------------------------------------------------------------ 6. accum_steps = 1 is the plain path
def test_accum_steps_1_never_accumulates(fdn, monkeypatch):
    trainer = importlib.import_module("4dflownet_amd.trainer")

    def boom(*a, **k):
        raise AssertionError("grad_accumulate launched with accum_steps = 1")
    monkeypatch.setattr(fdn.ops, "grad_accumulate", boom)
    tc = _tc(trainer, accum_steps=np.int64(1))                       # (a numpy integer is an integer)
    ref = _tc(trainer)
    for seed in (31, 32):
        b = O.synthetic_batch(2, P, R, seed=seed)
        tc.train_step(b)
        ref.train_step(b)
    assert tc.apply_accumulated() is False
    assert tc.optimizer.iterations == 2
    assert np.array_equal(_bits(tc.model.flat_w), _bits(ref.model.flat_w))
    n_ext = tc.model.flat_g_ext.numel()
    for owner in (tc, tc.model, tc.optimizer):
        for name, val in vars(owner).items():
            if isinstance(val, torch.Tensor) and val.numel() == n_ext:
                assert name == "flat_g_ext", (type(owner).__name__, name)
    assert tc.accum_g_ext is None


@pytest.mark.parametrize("bad", [0, -1, 1.5, "2", float("nan")])
def test_accum_steps_is_validated_at_construction_and_when_a_group_starts(bad):
    trainer = importlib.import_module("4dflownet_amd.trainer")
    with pytest.raises(ValueError, match="accum_steps"):
        _tc(trainer, accum_steps=bad)


def test_accum_steps_is_read_when_a_group_starts(fdn):
    trainer = importlib.import_module("4dflownet_amd.trainer")
    tc = _tc(trainer, accum_steps=np.int32(2))
    b = O.synthetic_batch(2, P, R, seed=31)
    tc.train_step(b)
    tc.accum_steps = 3                                               # mid-group: this group still closes after two
    tc.train_step(b)
    assert tc.optimizer.iterations == 1
    tc.train_step(b); tc.train_step(b)
    assert tc.optimizer.iterations == 1                              # the next group takes three
    tc.train_step(b)
    assert tc.optimizer.iterations == 2
    tc.accum_steps = 0
    with pytest.raises(ValueError, match="accum_steps"):
        tc.train_step(b)


# ------------------------------------------------------------------------------------------------ 7. train_network
def test_train_network_applies_the_ragged_group_before_validation(tmp_path):
    """cfg1 as in tests/test_gpu_pipeline.py (patch 16, res 1, batch 2, 2 + 1 blocks): 6 training rows = 3 batches, accum_steps = 2 -> per
    epoch one full group and one flushed group of one."""
    data = importlib.import_module("4dflownet_amd.data")
    trainer = importlib.import_module("4dflownet_amd.trainer")
    P1, R1, B, LB1, HB1 = 16, 1, 2, 2, 1
    idx = data.load_indexes(os.path.join(DATA, "train.csv"))[:6]
    val = data.load_indexes(os.path.join(DATA, "validate.csv"))[:4]
    mk = lambda rows, sh: data.PatchHandler3D(DATA, P1, R1, B, 0.6).initialize_dataset(rows, shuffle=sh, shard=(0, 1))
    tc = trainer.TrainerController(P1, R1, initial_learning_rate=2e-4, quicksave_enable=False, network_name="t4d", low_resblock=LB1,
                                   hi_resblock=HB1, accum_steps=2)
    tc.init_model_dir(base_dir=str(tmp_path / "models"))
    tc.train_network(mk(idx, True), mk(val, True), n_epoch=2, verbose=False)
    lines = open(os.path.join(tc.model_dir, "loss.csv")).read().splitlines()
    assert len([l for l in lines if l[:2] in ("1,", "2,")]) == 2
    assert tc.optimizer.iterations == 4
    assert tc.apply_accumulated() is False                           # nothing crossed the epoch's end
    assert os.path.exists(os.path.join(tc.model_dir, "t4d-best.h5")) and os.path.exists(os.path.join(tc.model_dir, "optimizer.pkl"))


# ------------------------------------------------------------------------------------------------ 8. bf16 activations
def test_bf16_group_equals_the_float32_sum_of_its_micro_batches(fdn):
    """Parameter gradients are fp32 in bf16 mode: the same accumulator, the same exact sum."""
    r = _run_group(importlib.import_module("4dflownet_amd.trainer"), dtype="bfloat16")
    _check_group_is_the_sum_of_its_micro_batches(r)

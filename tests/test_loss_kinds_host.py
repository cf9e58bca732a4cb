"""CPU checks of the data term's penalties (mse, mae, huber, charbonnier): the float64 restatement (tests/_loss_kinds.py) against torch
float64 autograd of the loss written literally, the header and the C-ABI's refusals (fake pointers: nothing is dereferenced before the
checks), the argument validation of ops.loss_metrics and TrainerController, and the training script.  No GPU needed."""
import ctypes
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

import _output_activation
from _loss_kinds import ACT_NONE, ACT_TANH, KINDS, data_gradient_fp32, loss_reference, rho_psi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, BAD_ARG = -2, -1
KIND_CASES = [("mse", None), ("mae", None), ("huber", 0.25), ("huber", 1.0), ("charbonnier", 1e-3), ("charbonnier", 2.0 ** -10)]


def _case(seed=3):
    """z, truth (2,3,4,5,3), mask (2,3,4,5) with values exactly on the non-fluid threshold; every residual of the linear AND of the tanh
    prediction at least 1e-3 from 0 (mae's kink) and from 0.25 and 1 (huber's seams), so autograd's subgradient choice never matters."""
    rng = np.random.default_rng(seed)
    shape = (2, 3, 4, 5)
    z = rng.normal(0, 1.2, size=shape + (3,))
    truth = rng.uniform(-0.8, 0.8, size=shape + (3,))
    for pred in (z, np.tanh(z)):
        for _ in range(4):
            a = np.abs(pred - truth)
            close = (a < 1e-3) | (np.abs(a - 0.25) < 1e-3) | (np.abs(a - 1.0) < 1e-3)
            truth[close] += 0.01
    for pred in (z, np.tanh(z)):
        a = np.abs(pred - truth)
        assert a.min() >= 1e-3 and np.abs(a - 0.25).min() >= 1e-3 and np.abs(a - 1.0).min() >= 1e-3
    mask = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], size=shape) * rng.uniform(0.5, 1.0, size=shape)
    mask.reshape(-1)[::3] = 0.5
    assert (mask == 0.5).sum() >= 40 and (mask < 0.5).sum() >= 10
    return z, truth, mask


def _literal_loss(z, truth, mask, kind, param, div_weight, non_fluid_weight, out_act):
    """The loss written out in torch float64, as one would in the reference: (data_b, div_b) with a graph back to z."""
    pred = torch.tanh(z) if out_act == ACT_TANH else z
    d = pred - truth
    if kind == "mse":
        rho = d * d
    elif kind == "mae":
        rho = torch.abs(d)
    elif kind == "huber":
        rho = torch.where(torch.abs(d) <= param, 0.5 * d * d, param * (torch.abs(d) - 0.5 * param))
    else:
        rho = torch.sqrt(d * d + param * param)
    nf = (mask < 0.5).to(torch.float64)
    ax = (1, 2, 3)
    fluid = lambda x: (x * mask).sum(ax) / (mask.sum(ax) + 1)
    nonfluid = lambda x: (x * nf).sum(ax) / (nf.sum(ax) + 1)
    e = rho.sum(-1)
    data_b = fluid(e) + non_fluid_weight * nonfluid(e)
    # the divergence term (TrainerController.py:111-120): SYMMETRIC pad 1, then x[k-1] - x[k+1] along the axis paired with the channel
    dd = 0
    for c in range(3):
        x = d[..., c]
        ax_c = c + 1
        n = x.shape[ax_c]
        idx = torch.arange(n)
        lo, hi = torch.clamp(idx - 1, 0, n - 1), torch.clamp(idx + 1, 0, n - 1)
        dd = dd + (x.index_select(ax_c, lo) - x.index_select(ax_c, hi)) ** 2
    div_b = div_weight * (fluid(dd) + non_fluid_weight * nonfluid(dd))
    return data_b, div_b


@pytest.mark.parametrize("out_act", [ACT_NONE, ACT_TANH])
@pytest.mark.parametrize("div_weight", [0.0, 0.8])
@pytest.mark.parametrize("non_fluid_weight", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("kind,param", KIND_CASES)
def test_restatement_matches_autograd_of_the_literal_loss(kind, param, non_fluid_weight, div_weight, out_act):
    z, truth, mask = _case()
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    data_t, div_t = _literal_loss(zt, torch.tensor(truth), torch.tensor(mask), kind, param, div_weight, non_fluid_weight, out_act)
    (data_t + div_t).sum().backward()
    pred = np.tanh(z) if out_act == ACT_TANH else z
    data_b, div_b, dz = loss_reference(pred, truth, mask, kind, param, div_weight, non_fluid_weight, out_act)
    assert np.abs(data_b - data_t.detach().numpy()).max() <= 1e-12
    assert np.abs(div_b - div_t.detach().numpy()).max() <= 1e-12
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12
    assert np.abs(dz).max() > 1e-4 or non_fluid_weight == 0


def test_mse_restatement_is_the_existing_reference():
    z, truth, mask = _case(5)
    for div_weight, nfw, act in ((0.0, 1.0, ACT_NONE), (0.6, 0.25, ACT_TANH), (0.6, 3.0, ACT_NONE), (0.0, 0.0, ACT_TANH)):
        pred = np.tanh(z) if act == ACT_TANH else z
        new = loss_reference(pred, truth, mask, "mse", None, div_weight, nfw, act)
        old = _output_activation.loss_reference(pred, truth, mask, div_weight, nfw, act)
        for a, b in zip(new, old):
            assert np.abs(a - b).max() <= 1e-15


def test_rho_psi_definitions():
    d = np.array([-2.0, -0.25, -2.0 ** -20, 0.0, 2.0 ** -20, 0.25, 0.3, 2.0])
    rho, psi = rho_psi(d, "mae")
    assert np.array_equal(rho, np.abs(d)) and np.array_equal(psi, [-1, -1, -1, 0, 1, 1, 1, 1])
    rho, psi = rho_psi(d, "huber", 0.25)
    assert np.array_equal(psi, [-0.25, -0.25, -2.0 ** -20, 0, 2.0 ** -20, 0.25, 0.25, 0.25])
    assert rho[5] == 0.5 * 0.25 ** 2 and rho[6] == 0.25 * (0.3 - 0.125) and rho[3] == 0
    rho, psi = rho_psi(d, "charbonnier", 1e-3)
    assert rho[3] == 1e-3 and psi[3] == 0 and np.array_equal(psi, -rho_psi(-d, "charbonnier", 1e-3)[1]) and abs(psi[-1] - 1) < 1e-6
    assert rho_psi(d, "huber")[0][-1] == 1.0 * (2.0 - 0.5) and rho_psi(d, "charbonnier")[0][3] == 1e-3            # the defaults
    # Huber with delta above every |d| is half the MSE
    assert np.array_equal(rho_psi(d, "huber", 4.0)[0], 0.5 * rho_psi(d, "mse")[0])
    assert np.array_equal(rho_psi(d, "huber", 4.0)[1], 0.5 * rho_psi(d, "mse")[1])
    with pytest.raises(ValueError):
        rho_psi(d, "l1")


@pytest.mark.parametrize("out_act", [ACT_NONE, ACT_TANH])
@pytest.mark.parametrize("kind,param", KIND_CASES[1:])
def test_fp32_emulation_of_the_gradient_stays_inside_the_rounding_count(kind, param, out_act):
    """The bound tests/test_gpu_loss_kinds.py holds every element of dpred to, 16 * 2^-24 of its own magnitude, counts the roundings of
    the straightforward fp32 path; numpy's fp32 emulation of that path stays well below it on the CPU."""
    rng = np.random.default_rng(11)
    shape = (3, 5, 7, 9)
    pred = rng.uniform(-0.999, 0.999, size=shape + (3,)).astype(np.float32)
    truth = rng.uniform(-0.9, 0.9, size=shape + (3,)).astype(np.float32)
    mask = (rng.uniform(size=shape) < 0.3).astype(np.float32)
    worst = 0.0
    for nfw in (0.0, 0.25, 1.0, 3.0):
        got = data_gradient_fp32(pred, truth, mask, kind, param, nfw, out_act).astype(np.float64)
        _, _, ref = loss_reference(pred, truth, mask, kind, param, 0.0, nfw, out_act)
        nz = ref != 0
        assert (got[~nz] == 0).all()
        worst = max(worst, (np.abs(got - ref)[nz] / np.abs(ref)[nz]).max() / 2.0 ** -24)
    print("fp32 emulation %s %s act %d: worst %.2f roundings" % (kind, param, out_act, worst))
    assert worst <= 16


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_version_and_symbol(fdn):
    lib = fdn._lib.load()
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    for name, code in (("MSE", 0), ("MAE", 1), ("HUBER", 2), ("CHARBONNIER", 3)):
        assert re.search(r"^#define FDN_LOSS_%s %d\b" % (name, code), header, re.M), name
        assert KINDS[name.lower()] == code and fdn.ops.LOSS_KINDS[name.lower()] == code
    assert re.search(r"int fdn_loss_metrics_kind\(const float\* pred, const float\* uh, const float\* vh, const float\* wh, const float\* mask,"
                     r" int kind,\s+float kind_param, float div_weight, float non_fluid_weight, int out_act, float\* out, float\* dpred,\s+"
                     r"float\* scratch, int N, int D, int H, int W, void\* stream\);", header)
    assert "#define FDN_VERSION 161" in header and lib.fdn_version() == 161 and fdn._lib.FDN_VERSION == 161
    res, args = fdn._lib.SIGNATURES["fdn_loss_metrics_kind"]
    assert res is ctypes.c_int and len(args) == 18
    assert args[5] is ctypes.c_int and args[6:9] == [ctypes.c_float] * 3 and args[9] is ctypes.c_int
    assert args[:5] == [ctypes.c_void_p] * 5 and args[10:13] == [ctypes.c_void_p] * 3 and args[13:17] == [ctypes.c_int] * 4
    assert hasattr(lib, "fdn_loss_metrics_kind")
    assert fdn.ops.LOSS_PARAM_DEFAULTS == {"huber": 1.0, "charbonnier": 1e-3}


def test_loss_metrics_kind_refusals_need_no_gpu(fdn):
    lib = fdn._lib.load()
    f = lib.fdn_loss_metrics_kind
    err = lambda: lib.fdn_last_error().decode()
    p = [0x1000 * (k + 1) for k in range(8)]              # pred uh vh wh mask | out dpred scratch
    ok = lambda **kw: dict(dict(ptrs=list(p), kind=2, kp=0.25, w=0.5, nfw=0.25, act=ACT_TANH, N=2, D=4, H=4, W=4), **kw)

    def call(a):
        q = a["ptrs"]
        return f(q[0], q[1], q[2], q[3], q[4], a["kind"], a["kp"], a["w"], a["nfw"], a["act"], q[5], q[6], q[7], a["N"], a["D"], a["H"],
                 a["W"], None)

    named = lambda: err().startswith("fdn_loss_metrics_kind:")
    for k in (0, 1, 2, 3, 4, 5, 7):                        # every operand but dpred (which may be NULL)
        q = list(p); q[k] = None
        assert call(ok(ptrs=q)) == BAD_ARG and named() and "NULL" in err(), k
    for bad in (-1, 4, 7, 1 << 20):
        assert call(ok(kind=bad)) == BAD_ARG and named() and "kind %d" % bad in err(), bad
    for kind, word in ((2, "delta"), (3, "epsilon")):
        for bad in (0.0, -0.0, -0.25, -1e-30, float("nan"), float("inf"), float("-inf")):
            assert call(ok(kind=kind, kp=bad)) == BAD_ARG and named() and word in err(), (kind, bad)
    for kind, word in ((0, "FDN_LOSS_MSE"), (1, "FDN_LOSS_MAE")):
        for bad in (0.25, -1.0, 1e-30, float("nan"), float("inf")):
            assert call(ok(kind=kind, kp=bad)) == BAD_ARG and named() and word in err() and "no parameter" in err(), (kind, bad)
    # everything fdn_loss_metrics_act refuses, for every kind
    for kind, kp in ((0, 0.0), (1, 0.0), (2, 0.25), (3, 1e-3)):
        for ext in ("N", "D", "H", "W"):
            for bad in (0, -3):
                assert call(ok(kind=kind, kp=kp, **{ext: bad})) == BAD_ARG and named() and "extents" in err(), (ext, bad)
        for bad in (-0.5, -1e-30, float("nan"), float("inf"), float("-inf")):
            assert call(ok(kind=kind, kp=kp, w=bad)) == BAD_ARG and named() and "div_weight" in err(), bad
            assert call(ok(kind=kind, kp=kp, nfw=bad)) == BAD_ARG and named() and "non_fluid_weight" in err(), bad
        for bad in (1, 2, 4, -1, 7):
            assert call(ok(kind=kind, kp=kp, act=bad)) == UNSUPPORTED and named() and "out_act" in err(), bad
        assert call(ok(kind=kind, kp=kp, D=1 << 11, H=1 << 10, W=1 << 10)) == BAD_ARG and "2^31" in err()


# ---------------------------------------------------------------------------------------------------------------- the Python surface
BAD_KINDS = ("l1", "MSE", "Huber", "", None, 2, b"mae")
BAD_PARAMS = (0, 0.0, -0.25, float("nan"), float("inf"), float("-inf"), 1e-60, 1e60, "x", True, [0.25])


def test_ops_loss_metrics_validates_before_it_needs_a_tensor(fdn):
    E = fdn._lib.FdnError
    none5 = (None,) * 5
    for bad in BAD_KINDS:
        with pytest.raises(E, match="loss must be one of"):
            fdn.ops.loss_metrics(*none5, kind=bad)
    for kind in ("huber", "charbonnier"):
        for bad in BAD_PARAMS:
            with pytest.raises(E, match="delta" if kind == "huber" else "epsilon"):
                fdn.ops.loss_metrics(*none5, kind=kind, kind_param=bad)
    for kind in ("mse", "mae"):
        for bad in (0.25, -1, float("nan"), "x", True):
            with pytest.raises(E, match="takes no parameter"):
                fdn.ops.loss_metrics(*none5, kind=kind, kind_param=bad)
    # the other options are still checked, whatever the kind
    with pytest.raises(E, match="non_fluid_weight"):
        fdn.ops.loss_metrics(*none5, kind="mae", non_fluid_weight=-1.0)
    with pytest.raises(E, match="out_act"):
        fdn.ops.loss_metrics(*none5, kind="huber", kind_param=0.25, out_act=1)
    assert fdn.ops.checked_loss_kind("huber", None) == ("huber", 2, 1.0)
    assert fdn.ops.checked_loss_kind("charbonnier", None) == ("charbonnier", 3, 1e-3)
    assert fdn.ops.checked_loss_kind("mae", None) == ("mae", 1, 0.0) and fdn.ops.checked_loss_kind("mse", 0) == ("mse", 0, 0.0)
    assert fdn.ops.checked_loss_kind("huber", np.float32(0.25)) == ("huber", 2, 0.25)


def test_trainer_validates_its_arguments(fdn):
    trainer = importlib.import_module("4dflownet_amd.trainer")
    make = lambda **kw: trainer.TrainerController(8, 2, quicksave_enable=False, low_resblock=0, hi_resblock=1, **kw)
    for bad in BAD_KINDS:
        with pytest.raises(ValueError, match="loss"):
            make(loss=bad)
    for kind in ("huber", "charbonnier"):
        for bad in BAD_PARAMS:
            with pytest.raises(ValueError, match="delta" if kind == "huber" else "epsilon"):
                make(loss=kind, loss_param=bad)
    for kind in ("mse", "mae"):
        with pytest.raises(ValueError, match="takes no parameter"):
            make(loss=kind, loss_param=0.25)
    with pytest.raises(ValueError, match="takes no parameter"):
        make(loss_param=0.25)                              # the default loss is 'mse'


def test_loss_is_read_on_every_step(fdn, monkeypatch):
    trainer = importlib.import_module("4dflownet_amd.trainer")
    seen = []

    def fake_loss_metrics(pred, uh, vh, wh, mask, **kw):
        seen.append(kw)
        return "out", "dpred"

    monkeypatch.setattr(trainer.ops, "loss_metrics", fake_loss_metrics)
    tc = object.__new__(trainer.TrainerController)
    tc.div_weight, tc.non_fluid_weight = 0, 1
    tc.model = types.SimpleNamespace(out_act=fdn.ops.ACT_NONE, output_activation="linear")
    base = dict(div_weight=0.0, non_fluid_weight=1.0, out_act=fdn.ops.ACT_NONE)
    assert tc._loss_call(("u", "v", "w"), "p", "m", True) == ("out", "dpred", 0.0)
    tc.loss, tc.loss_param = "huber", 0.25
    tc._loss_call(("u", "v", "w"), "p", "m", False)
    tc.loss_param = None
    tc._loss_call(("u", "v", "w"), "p", "m", True)
    tc.loss = "mae"
    tc.div_weight = 0.5
    tc._loss_call(("u", "v", "w"), "p", "m", True)
    tc.loss, tc.loss_param = "charbonnier", 2.0 ** -10
    tc._loss_call(("u", "v", "w"), "p", "m", True)
    tc.loss, tc.loss_param = "mse", None
    tc._loss_call(("u", "v", "w"), "p", "m", True)
    assert seen[0] == dict(base, want_grad=True)                                   # the default: the call as it always was
    assert seen[1] == dict(base, want_grad=False, kind="huber", kind_param=0.25)
    assert seen[2] == dict(base, want_grad=True, kind="huber", kind_param=1.0)
    assert seen[3] == dict(base, want_grad=True, div_weight=0.5, kind="mae", kind_param=None)
    assert seen[4] == dict(base, want_grad=True, div_weight=0.5, kind="charbonnier", kind_param=2.0 ** -10)
    assert seen[5] == dict(base, want_grad=True, div_weight=0.5)
    for loss, param, word in (("l1", None, "loss"), ("huber", -1, "delta"), ("mae", 0.5, "takes no parameter"), ("charbonnier", 0, "epsilon")):
        tc.loss, tc.loss_param = loss, param
        with pytest.raises(ValueError, match=word):
            tc._loss_call(("u", "v", "w"), "p", "m", False)
    assert len(seen) == 6
    # train_step, test_step and quicksave reach the loss pass through that one call
    src = open(os.path.join(ROOT, "4dflownet_amd", "trainer.py")).read()
    assert src.count("ops.loss_metrics(") == 1 and src.count("self._loss_call(") == 2


def test_training_script_names_both_options():
    src = open(os.path.join(ROOT, "scripts", "trainer.py")).read()
    assert re.search(r"^    loss = 'mse'$", src, re.M) and re.search(r"^    loss_param = None$", src, re.M)
    assert re.search(r"loss=loss,\s+loss_param=loss_param\)", src)

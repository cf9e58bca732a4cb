"""CPU checks of the heads' tanh output activation and of non_fluid_weight: the float64 reference (tests/_output_activation.py) against
central finite differences of its own loss, the refusals of the C-ABI (fake pointers: nothing is dereferenced before the checks), the
argument validation of the Python surface, and the script flags.  No GPU needed."""
import ctypes
import importlib
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from _output_activation import ACT_NONE, ACT_TANH, loss_reference, total_loss_of_preactivations, activation, weighted_loss
from _divergence import divergence_loss
from oracle import flownet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, BAD_ARG = -2, -1


def _case(seed=3):
    rng = np.random.default_rng(seed)
    shape = (2, 3, 4, 5)
    z = rng.normal(0, 1.2, size=shape + (3,))
    truth = rng.uniform(-0.8, 0.8, size=shape + (3,))
    mask = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], size=shape) * rng.uniform(0.5, 1.0, size=shape)
    mask.reshape(-1)[::3] = 0.5                           # exactly on the threshold: fluid weight 0.5, not non-fluid
    assert (mask == 0.5).sum() >= 40 and (mask < 0.5).sum() >= 10
    return z, truth, mask


@pytest.mark.parametrize("div_weight,non_fluid_weight,out_act", [(0.7, 0.25, ACT_TANH), (0.7, 1.0, ACT_TANH), (0.0, 1.0, ACT_TANH),
                                                                 (0.7, 0.25, ACT_NONE), (0.0, 3.0, ACT_NONE), (0.7, 0.0, ACT_NONE)])
def test_reference_gradient_matches_finite_differences(div_weight, non_fluid_weight, out_act):
    z, truth, mask = _case()
    _, _, dz = loss_reference(activation(z, out_act), truth, mask, div_weight, non_fluid_weight, out_act)
    eps = 1e-5
    fd = np.zeros_like(z)
    for i in range(z.size):
        zp = z.copy(); zp.reshape(-1)[i] += eps
        zm = z.copy(); zm.reshape(-1)[i] -= eps
        fd.reshape(-1)[i] = (total_loss_of_preactivations(zp, truth, mask, div_weight, non_fluid_weight, out_act) -
                             total_loss_of_preactivations(zm, truth, mask, div_weight, non_fluid_weight, out_act)) / (2 * eps)
    # the loss is quadratic in pred (central differences exact up to rounding); through tanh the truncation is eps^2 |L'''| / 6 ~ 1e-10
    assert np.abs(dz - fd).max() <= 1e-7 * np.abs(fd).max(), np.abs(dz - fd).max() / np.abs(fd).max()
    assert np.abs(fd).max() > 1e-3


def test_reference_reduces_to_the_existing_helpers_at_the_defaults():
    z, truth, mask = _case(5)
    mse_b, div_b, dp = weighted_loss(z, truth, mask, 0.6, 1.0)
    mse0, dp_mse = O.masked_mse_loss_fwd_bwd(z, truth, mask)
    div0, dp_div = divergence_loss(z, truth, mask, 0.6)
    assert np.abs(mse_b - mse0).max() <= 1e-13 and np.abs(div_b - div0).max() <= 1e-13
    assert np.abs(dp - (dp_mse + dp_div)).max() <= 1e-13 * np.abs(dp).max()
    # weight 0: the fluid part alone; the weight is linear
    m0, d0, _ = weighted_loss(z, truth, mask, 0.6, 0.0)
    m3, d3, _ = weighted_loss(z, truth, mask, 0.6, 3.0)
    assert np.allclose(m3 - m0, 3 * (mse_b - m0), rtol=1e-12) and np.allclose(d3 - d0, 3 * (div_b - d0), rtol=1e-12)
    assert (m0 < mse_b).all() and (d0 < div_b).all()


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_version_and_symbol(fdn):
    lib = fdn._lib.load()
    assert lib.fdn_version() == 161
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    assert re.search(r"^#define FDN_ACT_TANH 3\b", header, re.M) and "#define FDN_VERSION 161" in header
    assert re.search(r"int fdn_loss_metrics_act\(const float\* pred, const float\* uh, const float\* vh, const float\* wh, const float\* mask,"
                     r" float div_weight,\s+float non_fluid_weight, int out_act, float\* out, float\* dpred, float\* scratch,", header)
    sig = fdn._lib.SIGNATURES["fdn_loss_metrics_act"]
    assert sig[1][5] is ctypes.c_float and sig[1][6] is ctypes.c_float and sig[1][7] is ctypes.c_int and len(sig[1]) == 16
    assert hasattr(lib, "fdn_loss_metrics_act")
    assert fdn.ops.ACT_TANH == 3 and importlib.import_module("4dflownet_amd.ops_bf16").ACT_TANH == 3


def test_loss_metrics_act_refusals_need_no_gpu(fdn):
    lib = fdn._lib.load()
    f = lib.fdn_loss_metrics_act
    err = lambda: lib.fdn_last_error().decode()
    p = [0x1000 * (k + 1) for k in range(8)]              # pred uh vh wh mask | out dpred scratch
    ok = lambda **kw: dict(dict(ptrs=list(p), w=0.5, nfw=0.25, act=ACT_TANH, N=2, D=4, H=4, W=4), **kw)

    def call(a):
        q = a["ptrs"]
        return f(q[0], q[1], q[2], q[3], q[4], a["w"], a["nfw"], a["act"], q[5], q[6], q[7], a["N"], a["D"], a["H"], a["W"], None)

    for k in (0, 1, 2, 3, 4, 5, 7):                        # every operand but dpred (which may be NULL)
        q = list(p); q[k] = None
        assert call(ok(ptrs=q)) == BAD_ARG and "fdn_loss_metrics_act" in err() and "NULL" in err(), k
    for ext in ("N", "D", "H", "W"):
        for bad in (0, -3):
            assert call(ok(**{ext: bad})) == BAD_ARG and "fdn_loss_metrics_act" in err() and "extents" in err(), (ext, bad)
    for bad in (-0.5, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert call(ok(w=bad)) == BAD_ARG and "fdn_loss_metrics_act" in err() and "div_weight" in err(), bad
        assert call(ok(nfw=bad)) == BAD_ARG and "fdn_loss_metrics_act" in err() and "non_fluid_weight" in err(), bad
    for bad in (1, 2, 4, -1, 7):                           # RELU and LEAKY are no activations of the heads either
        assert call(ok(act=bad)) == UNSUPPORTED and "fdn_loss_metrics_act" in err() and "out_act" in err(), bad
    assert call(ok(D=1 << 11, H=1 << 10, W=1 << 10)) == BAD_ARG and "2^31" in err()


def _fake(n):
    return [0x10000 * (k + 1) for k in range(n)]


def test_tanh_is_refused_everywhere_but_on_the_heads_forward(fdn):
    """FDN_ACT_TANH on the 64->64, 3->64 and 1x1 routes of both forwards and on every dgrad, fold and upsample entry point that takes an
    act: refused under the function's name before anything touches the device (the pointers are fake).  FDN_ERR_UNSUPPORTED where an
    unknown act used to pass as "none"; the entry points that always range-checked their act keep the FDN_ERR_BAD_ARG that
    tests/test_api_twins_host.py pins for act = 3."""
    lib = fdn._lib.load()
    err = lambda: lib.fdn_last_error().decode()
    T = ACT_TANH
    a = _fake(8)
    N, D, H, W = 1, 4, 4, 4
    for (cin, cout, k) in ((64, 64, 3), (3, 64, 3), (128, 64, 1), (5, 7, 3)):
        rc = lib.fdn_conv3d_fwd(a[0], a[1], a[2], a[3], a[4], None, a[5], N, D, H, W, cin, cout, k, cout, 0, T, 0.2, 0, None)
        assert rc == BAD_ARG and "fdn_conv3d_fwd:" in err() and "TANH" in err(), (cin, cout, k, rc, err())
        rc = lib.fdn_conv3d_fwd_bf16(a[0], a[1], a[2], a[3], a[4], None, a[5], N, D, H, W, cin, cout, k, cout, 0, T, 0.2, None)
        assert rc == BAD_ARG and "fdn_conv3d_fwd_bf16:" in err() and "TANH" in err(), (cin, cout, k, rc, err())
    # an act beyond the last one stays a bad argument
    assert lib.fdn_conv3d_fwd(a[0], a[1], a[2], a[3], a[4], None, a[5], N, D, H, W, 64, 1, 3, 1, 0, 4, 0.2, 0, None) == BAD_ARG
    assert "bad act" in err()
    calls = {
        "fdn_conv3d_dgrad_fused": lambda f: f(a[0], a[1], a[2], None, a[3], T, 0.2, a[4], N, D, H, W, 0, None),
        "fdn_conv3d_dgrad_fused_part": lambda f: f(a[0], a[1], a[2], None, a[3], T, 0.2, a[4], N, D, H, W, 3, 0, None),
        "fdn_conv64_fwd_mask": lambda f: f(a[0], a[1], a[2], None, a[3], a[4], N, D, H, W, T, 0.2, 0, None),
        "fdn_conv64_dgrad_fused_mask": lambda f: f(a[0], a[1], a[2], None, a[3], T, 0.2, a[4], N, D, H, W, 0, None),
        "fdn_conv64_fwd_bf16": lambda f: f(a[0], a[1], a[2], None, a[3], N, D, H, W, T, 0.2, None),
        "fdn_conv64_dgrad_fused_bf16": lambda f: f(a[0], a[1], a[2], None, a[3], T, 0.2, a[4], N, D, H, W, None),
        "fdn_fold_halo": lambda f: f(a[0], None, None, 1, None, a[1], T, 0.2, a[2], N, D, H, W, 64, None),
        "fdn_fold_halo_border": lambda f: f(a[0], None, None, 1, None, a[1], T, 0.2, a[2], N, D, H, W, None),
        "fdn_fold_halo_border_bf16": lambda f: f(a[0], None, None, 1, None, a[1], T, 0.2, a[2], N, D, H, W, None),
        "fdn_upsample_trilinear_bwd": lambda f: f(a[0], a[1], T, 0.2, a[2], N, D, H, W, 64, 2, None),
        "fdn_upsample_trilinear_bwd_bf16": lambda f: f(a[0], a[1], T, 0.2, a[2], N, D, H, W, 64, 2, None),
        "fdn_conv_cout1_dgrad_folded": lambda f: f(a[0], a[1], a[2], T, 0.2, a[3], None, None, 0, N, D, H, W, 3, 0, None),
        "fdn_conv_cout1_dgrad_folded_bf16": lambda f: f(a[0], a[1], a[2], T, 0.2, a[3], None, None, 0, N, D, H, W, 3, 0, None),
    }
    range_checked = ("fdn_conv3d_dgrad_fused", "fdn_conv3d_dgrad_fused_part", "fdn_conv64_fwd_mask", "fdn_conv64_dgrad_fused_mask",
                     "fdn_conv64_fwd_bf16", "fdn_conv64_dgrad_fused_bf16")
    for name, call in calls.items():
        rc = call(getattr(lib, name))
        if name in range_checked:
            assert rc == BAD_ARG and err().startswith(name + ":") and "act" in err(), (name, rc, err())
        else:
            assert rc == UNSUPPORTED and err().startswith(name + ":") and "TANH" in err(), (name, rc, err())


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_build_network_and_trainer_validate_their_arguments(fdn):
    network = importlib.import_module("4dflownet_amd.network")
    trainer = importlib.import_module("4dflownet_amd.trainer")
    assert network.output_activation_code(None) == ("linear", fdn.ops.ACT_NONE)
    assert network.output_activation_code("linear") == ("linear", fdn.ops.ACT_NONE)
    assert network.output_activation_code("tanh") == ("tanh", fdn.ops.ACT_TANH)
    ins = [network.Input((8, 8, 8, 1), n) for n in "abcdef"]
    for bad in ("relu", "Tanh", 3, ""):
        with pytest.raises(ValueError, match="output_activation"):
            network.SR4DFlowNet(2).build_network(*ins, 1, 1, output_activation=bad)
        with pytest.raises(ValueError, match="output_activation"):
            trainer.TrainerController(8, 2, quicksave_enable=False, low_resblock=0, hi_resblock=1, output_activation=bad)
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="non_fluid_weight"):
            trainer.TrainerController(8, 2, quicksave_enable=False, low_resblock=0, hi_resblock=1, non_fluid_weight=bad)


def test_ops_loss_metrics_validates_before_it_needs_a_tensor(fdn):
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(fdn._lib.FdnError, match="non_fluid_weight"):
            fdn.ops.loss_metrics(None, None, None, None, None, non_fluid_weight=bad)
    for bad in (1, 2, 4, "tanh"):
        with pytest.raises(fdn._lib.FdnError, match="out_act"):
            fdn.ops.loss_metrics(None, None, None, None, None, out_act=bad)


def test_non_fluid_weight_is_read_on_every_step(fdn, monkeypatch):
    trainer = importlib.import_module("4dflownet_amd.trainer")
    seen = []

    def fake_loss_metrics(pred, uh, vh, wh, mask, **kw):
        seen.append(kw)
        return "out", "dpred"

    monkeypatch.setattr(trainer.ops, "loss_metrics", fake_loss_metrics)
    tc = object.__new__(trainer.TrainerController)
    tc.div_weight, tc.non_fluid_weight = 0, 1
    tc.model = types.SimpleNamespace(out_act=fdn.ops.ACT_TANH, output_activation="tanh")
    assert tc._loss_call(("u", "v", "w"), "p", "m", True) == ("out", "dpred", 0.0)
    tc.non_fluid_weight = 0.25
    tc.div_weight = 0.5
    tc._loss_call(("u", "v", "w"), "p", "m", False)
    assert seen[0] == dict(want_grad=True, div_weight=0.0, non_fluid_weight=1.0, out_act=fdn.ops.ACT_TANH)
    assert seen[1] == dict(want_grad=False, div_weight=0.5, non_fluid_weight=0.25, out_act=fdn.ops.ACT_TANH)
    tc.non_fluid_weight = -2
    with pytest.raises(ValueError, match="non_fluid_weight"):
        tc._loss_call(("u", "v", "w"), "p", "m", False)
    # train_step, test_step and quicksave reach the loss pass through that one call
    src = open(os.path.join(ROOT, "4dflownet_amd", "trainer.py")).read()
    assert src.count("ops.loss_metrics(") == 1 and src.count("self._loss_call(") == 2


@pytest.mark.parametrize("script", ["predictor", "evaluate"])
def test_script_flags_parse(script):
    spec = importlib.util.spec_from_file_location("_script_" + script, os.path.join(ROOT, "scripts", script + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                             # (the run itself sits under __main__)
    assert mod._output_activation([]) is None
    assert mod._output_activation(["--blend", "2", "--output-activation", "tanh"]) == "tanh"
    assert mod._output_activation(["--output-activation", "linear", "--self-ensemble"]) == "linear"
    for bad in (["--output-activation"], ["--output-activation", "relu"], ["--output-activation", "--blend"]):
        with pytest.raises(SystemExit):
            mod._output_activation(bad)
    assert "output_activation=_output_activation(sys.argv[1:])" in open(os.path.join(ROOT, "scripts", script + ".py")).read()


def test_trainer_script_names_the_options():
    src = open(os.path.join(ROOT, "scripts", "trainer.py")).read()
    assert "non_fluid_weight = 1\n" in src and "output_activation = None\n" in src
    assert "non_fluid_weight=non_fluid_weight, output_activation=output_activation" in src

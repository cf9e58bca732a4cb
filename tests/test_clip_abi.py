"""CPU-side checks of gradient clipping's boundary: the three entry points in the header, the ctypes table and both libraries, the version they
leave alone, every refusal reported before the device is touched (the pointers here are fake and never dereferenced), the checks of the ops
wrappers and of TrainerController's two arguments, and the float64 restatement the GPU tests compare against."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

import _clip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdn_grad_sumsq_partials", "fdn_clip_scale", "fdn_adam_step_clipped")


def _comment(header, name):
    proto = header[:header.index("int " + name + "(")]
    return proto[proto.rindex("\n/*"):]


def test_header_ctypes_table_and_both_libraries_hold_the_entry_points(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    sig = fdn._lib.SIGNATURES
    for name in NAMES:
        assert name in declared and name in sig, name
        assert "TrainerController.py:73,223-225" in _comment(header, name), name
    c = _comment(header, "fdn_grad_sumsq_partials")
    assert "g_i + l2s * w_i" in c and "l2_grad_scale * l2_scale_dev[0]" in c and "frozen[i] == 0" in c and "not read" in c
    c = _comment(header, "fdn_clip_scale")
    assert "clip_norm / max(N, clip_norm)" in c and "exactly 1.0f" in c and "clip_norm * min(1 / N, 1 / clip_norm)" in c
    assert "not finite" in c and "s = NaN" in c
    c = _comment(header, "fdn_adam_step_clipped")
    assert "g'_i * g_scale_dev[0]" in c and "g'_i > clip_value ? clip_value : (g'_i < -clip_value ? -clip_value : g'_i)" in c
    assert "bit-identical" in c and "NaN" in c and "frozen elements keep their bits" in c
    p, f, i64, i = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64, ctypes.c_int
    assert sig["fdn_grad_sumsq_partials"] == (i, [p, p, p, p, i64, f, p, p, p])
    assert sig["fdn_clip_scale"] == (i, [p, i, f, p, p])
    # fdn_adam_step_masked's list with g_scale_dev and clip_value in front of sumsq_partials
    masked = list(sig["fdn_adam_step_masked"][1])
    assert sig["fdn_adam_step_clipped"] == (i, masked[:-2] + [p, f] + masked[-2:])
    build = import_module("4dflownet_amd.build")
    for path in (build.build_library(), build.build_library(test_hooks=True)):
        lib = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(lib, name), (path, name)
    assert fdn._lib.load().fdn_version() == 161 == fdn._lib.FDN_VERSION          # paths of existing kernels, additive: the version stays


def test_entry_points_refuse_bad_arguments_before_they_touch_the_device(fdn):
    lib = fdn._lib.load()
    err = lambda: lib.fdn_last_error().decode()
    nan, inf = float("nan"), float("inf")

    # fdn_grad_sumsq_partials(g, w, is_kernel, frozen, n, l2_grad_scale, l2_scale_dev, partials, stream)
    f, name = lib.fdn_grad_sumsq_partials, "fdn_grad_sumsq_partials"
    ptrs = dict(g=0x100000, w=0x200000, is_kernel=0x300000, partials=0x400000)
    call = lambda a, n: f(a["g"], a["w"], a["is_kernel"], None, n, 1e-6, None, a["partials"], None)
    for bad in ptrs:
        a = dict(ptrs)
        a[bad] = None
        assert call(a, 1024) != 0 and name in err() and "%s is NULL" % bad in err(), (bad, err())
    for n in (0, -1, -(1 << 40)):
        assert call(ptrs, n) != 0 and name in err() and "n=%d" % n in err(), n

    # fdn_clip_scale(partials, n_partials, clip_norm, out, stream)
    f, name = lib.fdn_clip_scale, "fdn_clip_scale"
    assert f(None, 2048, 1.0, 0x200000, None) != 0 and name in err() and "partials is NULL" in err()
    assert f(0x100000, 2048, 1.0, None, None) != 0 and name in err() and "out is NULL" in err()
    for n in (0, -5):
        assert f(0x100000, n, 1.0, 0x200000, None) != 0 and name in err() and "n_partials=%d" % n in err()
    for c in (0.0, -1.0, nan, inf, -inf):
        assert f(0x100000, 2048, c, 0x200000, None) != 0 and name in err() and "clip_norm" in err(), (c, err())

    # fdn_adam_step_clipped(w, g, m, v, is_kernel, frozen, n, lr_t, lr_t_dev, b1, b2, eps, l2_grad_scale, l2_scale_dev, g_scale_dev, clip_value, sumsq, stream)
    f, name = lib.fdn_adam_step_clipped, "fdn_adam_step_clipped"
    ptrs = dict(w=0x100000, g=0x200000, m=0x300000, v=0x400000, is_kernel=0x500000)
    call = lambda a, n, cv: f(a["w"], a["g"], a["m"], a["v"], a["is_kernel"], None, n, 1e-3, None, 0.9, 0.999, 1e-7, 1e-6, None, None, cv, None, None)
    for bad in ptrs:
        a = dict(ptrs)
        a[bad] = None
        assert call(a, 1024, 0.5) != 0 and name in err() and "%s is NULL" % bad in err(), (bad, err())
    for n in (0, -1, -(1 << 40)):
        assert call(ptrs, n, 0.5) != 0 and name in err() and "n=%d" % n in err(), n
    for cv in (-1.0, -1e-30, nan, -inf):
        assert call(ptrs, 1024, cv) != 0 and name in err() and "clip_value" in err(), (cv, err())


def test_ops_wrappers_check_their_operands_before_the_library_is_called(fdn):
    import torch
    ops = fdn.ops
    z, k = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    one = torch.ones(1)
    adam = lambda **kw: ops.adam_step(z, z, z, z, k, 1e-3, 0.9, 0.999, 1e-7, 0.0, **kw)
    with pytest.raises(fdn.FdnError, match="both set"):
        adam(g_scale_dev=one, clip_value=0.5)
    with pytest.raises(fdn.FdnError, match="g_scale_dev must hold one float32 on the GPU"):
        adam(g_scale_dev=one)                                         # on the host
    with pytest.raises(fdn.FdnError, match="g_scale_dev must hold one float32 on the GPU"):
        adam(g_scale_dev=torch.ones(1, dtype=torch.float64))
    with pytest.raises(fdn.FdnError, match="g_scale_dev must hold one float32 on the GPU"):
        adam(g_scale_dev=torch.ones(2))
    for bad in (-0.5, float("nan")):
        with pytest.raises(fdn.FdnError, match="clip_value must be >= 0"):
            adam(clip_value=bad)
    with pytest.raises(fdn.FdnError, match="frozen holds 4 bytes for 8 parameters"):
        adam(clip_value=0.5, frozen=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(fdn.FdnError, match="GPU"):                    # a host tensor reaches the clipped entry point's pointer check, no CPU path
        adam(clip_value=0.5)
    part = torch.zeros(ops.ADAM_PARTIALS)
    with pytest.raises(fdn.FdnError, match="partials needs %d floats" % ops.ADAM_PARTIALS):
        ops.grad_sumsq_partials(z, z, k, 1e-6, partials=torch.zeros(16))
    with pytest.raises(fdn.FdnError, match="w holds 4 elements for 8 gradients"):
        ops.grad_sumsq_partials(z, torch.zeros(4), k, 1e-6, partials=part)
    with pytest.raises(fdn.FdnError, match="is_kernel holds 4 elements for 8 gradients"):
        ops.grad_sumsq_partials(z, z, k[:4], 1e-6, partials=part)
    with pytest.raises(fdn.FdnError, match="frozen holds 4 elements for 8 gradients"):
        ops.grad_sumsq_partials(z, z, k, 1e-6, partials=part, frozen=k[:4])
    with pytest.raises(fdn.FdnError, match="l2_scale_dev must hold one float32 on the GPU"):
        ops.grad_sumsq_partials(z, z, k, 1e-6, l2_scale_dev=one, partials=part)
    with pytest.raises(fdn.FdnError, match="GPU"):
        ops.grad_sumsq_partials(z, z, k, 1e-6, partials=part)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e300, 1e-60):   # the last two are inf and 0 as float32
        with pytest.raises(fdn.FdnError, match="clip_norm must be finite and > 0"):
            ops.clip_scale(part, bad, torch.zeros(2))
    with pytest.raises(fdn.FdnError, match="out needs 2 floats"):
        ops.clip_scale(part, 1.0, torch.zeros(1))
    with pytest.raises(fdn.FdnError, match="GPU"):
        ops.clip_scale(part, 1.0, torch.zeros(2))
    # ops_bf16 offers the same adam_step
    assert import_module("4dflownet_amd.ops_bf16").adam_step is ops.adam_step


def test_trainer_validates_the_two_arguments():
    """TrainerController(global_clipnorm=, clipvalue=) and every later optimiser step go through trainer._clip_arguments (construction needs
    a device; the helper does not)."""
    import inspect
    trainer = import_module("4dflownet_amd.trainer")
    check = trainer._clip_arguments
    assert check(None, None) == (None, None)
    assert check(2, None) == (2.0, None) and check(None, np.float32(0.5)) == (None, 0.5) and check(1e30, None)[0] == float(np.float32(1e30))
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e300, 1e-60, "1.0", True, [1.0], object()):
        with pytest.raises(ValueError, match="global_clipnorm"):
            check(bad, None)
        with pytest.raises(ValueError, match="clipvalue"):
            check(None, bad)
    with pytest.raises(ValueError, match="both set"):
        check(1.0, 1.0)
    params = inspect.signature(trainer.TrainerController.__init__).parameters
    assert params["global_clipnorm"].default is None and params["clipvalue"].default is None
    assert "clipnorm" not in params                                   # Keras' per-variable clipnorm is out of scope
    src = inspect.getsource(trainer.TrainerController)
    assert src.count("self._checked_clip()") >= 3                     # construction, every optimiser step (_adam), logging
    assert "return _clip_arguments(self.global_clipnorm, self.clipvalue)" in src


def test_float64_restatement_is_tf_clip_by_global_norm():
    """c / max(N, c) against the literal TF formula c * min(1 / N, 1 / c) at 1e-12 in float64, clip active and inactive; the clipped
    gradient's norm is min(N, c); clip_by_value is numpy's clip and keeps NaN; the Adam step behind is adam_step_tf."""
    oracle = import_module("oracle.flownet_oracle")
    rng = np.random.default_rng(3)
    n = 1001
    g, w = rng.standard_normal(n), rng.standard_normal(n)
    isk = rng.random(n) < 0.8
    live = rng.random(n) < 0.7
    l2s = 0.4
    for lv in (None, live):
        gp = _clip_ref.step_gradient(g, w, isk, l2s, lv)
        sel = slice(None) if lv is None else lv
        assert np.array_equal(gp[sel], (g + l2s * w * isk)[sel]) and (lv is None or not gp[~lv].any())
        N = _clip_ref.global_norm(gp)
        assert abs(N - np.linalg.norm(gp)) <= 1e-12 * N
        for c in (0.25 * N, N, 4 * N, 1e-3, 1e30):
            s, s_tf = _clip_ref.clip_scale(N, c), _clip_ref.clip_scale_tf(N, c)
            assert abs(s - s_tf) <= 1e-12 * s_tf, (c, s, s_tf)
            assert (s == 1.0) == (N <= c)
            clipped, n2 = _clip_ref.clip_by_global_norm(gp, c)
            assert n2 == N and abs(np.linalg.norm(clipped) - min(N, c)) <= 1e-12 * N
    for bad in (float("inf"), float("nan")):
        assert np.isnan(_clip_ref.clip_scale(bad, 1.0)) and np.isnan(_clip_ref.clip_scale_tf(bad, 1.0))
    x = np.array([-2.0, -0.5, 0.0, 0.5, 2.0, np.nan])
    got = _clip_ref.clip_by_value(x, 0.75)
    assert np.array_equal(got[:5], np.clip(x[:5], -0.75, 0.75)) and np.isnan(got[5])
    # the step: clip, then Keras Adam, on the live elements only
    for kw in (dict(global_clipnorm=0.25 * _clip_ref.global_norm(_clip_ref.step_gradient(g, w, isk, l2s, live))), dict(clipvalue=0.3), {}):
        w1, m1, v1 = w.copy(), np.zeros(n), np.zeros(n)
        norm = _clip_ref.clipped_adam_step(w1, g, m1, v1, isk, 1, 1e-3, l2s, live=live, **kw)
        gp = _clip_ref.step_gradient(g, w, isk, l2s, live)
        assert norm == _clip_ref.global_norm(gp)
        if "global_clipnorm" in kw:
            gp = gp * 0.25
        elif "clipvalue" in kw:
            gp = np.clip(gp, -0.3, 0.3)
        w2, m2, v2 = w.copy(), np.zeros(n), np.zeros(n)
        oracle.adam_step_tf(w2, gp, m2, v2, 1, 1e-3)
        assert np.allclose(w1[live], w2[live], rtol=1e-13, atol=0) and np.allclose(m1[live], m2[live], rtol=1e-13, atol=0)
        assert np.array_equal(w1[~live], w[~live]) and not m1[~live].any() and not v1[~live].any()

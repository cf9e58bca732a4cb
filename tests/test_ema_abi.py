"""CPU-side checks of the weight EMA's boundary: the entry point in the header, the ctypes table and both libraries, the version it leaves
alone, every refusal reported before the device is touched (the pointers here are fake and never dereferenced), the checks of the ops
wrapper and of TrainerController's arguments, and the float64 restatement the GPU tests compare against."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

import _ema_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fdn_adam_step_ema"


def test_header_ctypes_table_and_both_libraries_hold_the_entry_point(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    sig = fdn._lib.SIGNATURES
    assert NAME in declared and NAME in sig
    proto = header[:header.index("int " + NAME + "(")]
    c = proto[proto.rindex("\n/*"):]
    assert "ema[i] = ema_momentum * ema[i] + (1.f - ema_momentum) * wn" in c           # the recurrence
    assert "ema_init != 0" in c and "a_0 = w_0" in c and "not read" in c               # the init rule
    assert "frozen[i] != 0" in c and "ema[i] = wi" in c                                # the frozen rule
    assert "bit-identical w, m, v, partials" in c
    assert "[TF]" in c
    p, f, i = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    clipped = list(sig["fdn_adam_step_clipped"][1])
    assert sig[NAME] == (i, clipped[:-2] + [p, f, i] + clipped[-2:])                   # ema, ema_momentum, ema_init ahead of sumsq_partials, stream
    args = header[header.index("int " + NAME + "("):]
    args = re.sub(r"/\*.*?\*/", "", args[:args.index(";")])
    names = [a.split()[-1].lstrip("*") for a in args[args.index("(") + 1:args.rindex(")")].split(",")]
    assert names[-5:] == ["ema", "ema_momentum", "ema_init", "sumsq_partials", "stream"] and len(names) == len(sig[NAME][1])
    build = import_module("4dflownet_amd.build")
    for path in (build.build_library(), build.build_library(test_hooks=True)):
        assert hasattr(ctypes.CDLL(path), NAME), path
    assert fdn._lib.load().fdn_version() == 161 == fdn._lib.FDN_VERSION               # an option of an existing kernel, additive: the version stays


def test_entry_point_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    err = lambda: lib.fdn_last_error().decode()
    nan, inf = float("nan"), float("inf")
    f = lib.fdn_adam_step_ema
    ptrs = dict(w=0x100000, g=0x200000, m=0x300000, v=0x400000, is_kernel=0x500000, ema=0x600000)
    # (w, g, m, v, is_kernel, frozen, n, lr_t, lr_t_dev, b1, b2, eps, l2_grad_scale, l2_scale_dev, g_scale_dev, clip_value, ema, ema_momentum, ema_init, sumsq, stream)
    call = lambda a, n=1024, cv=0.0, mom=0.99: f(a["w"], a["g"], a["m"], a["v"], a["is_kernel"], None, n, 1e-3, None, 0.9, 0.999, 1e-7, 1e-6,
                                                 None, None, cv, a["ema"], mom, 0, None, None)
    for bad in ptrs:
        a = dict(ptrs)
        a[bad] = None
        assert call(a) != 0 and NAME in err() and "%s is NULL" % bad in err(), (bad, err())
    for n in (0, -1, -(1 << 40)):
        assert call(ptrs, n=n) != 0 and NAME in err() and "n=%d" % n in err(), n
    for mom in (1.0, 1.5, -0.25, -1e-30, nan, inf, -inf, 0.999999999):               # the last is 1.0f as float32
        assert call(ptrs, mom=mom) != 0 and NAME in err() and "ema_momentum" in err(), (mom, err())
    for cv in (-1.0, -1e-30, nan, -inf):
        assert call(ptrs, cv=cv) != 0 and NAME in err() and "clip_value" in err(), (cv, err())


def test_ops_wrapper_checks_its_operands_before_the_library_is_called(fdn):
    import torch
    ops = fdn.ops
    z, k = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    adam = lambda **kw: ops.adam_step(z, z, z, z, k, 1e-3, 0.9, 0.999, 1e-7, 0.0, **kw)
    for bad in (torch.zeros(8), torch.zeros(8, dtype=torch.float64), torch.zeros(4)):       # on the host; (the device ones need a device)
        with pytest.raises(fdn.FdnError, match="ema must hold 8 float32 on the GPU"):
            adam(ema=bad, ema_momentum=0.5)

    class OnDevice:                                                   # passes the placement check, never reaches a pointer
        is_cuda, dtype = True, torch.float32

        def __init__(self, n):
            self.n = n

        def numel(self):
            return self.n
    with pytest.raises(fdn.FdnError, match="ema must hold 8 float32 on the GPU"):
        adam(ema=OnDevice(7), ema_momentum=0.5)
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf"), 0.999999999):
        with pytest.raises(fdn.FdnError, match=r"ema_momentum must lie in \[0, 1\) as float32"):
            adam(ema=OnDevice(8), ema_momentum=bad)
    with pytest.raises(fdn.FdnError, match="GPU"):                    # a good average: the host tensors are refused next, no CPU path
        adam(ema=OnDevice(8), ema_momentum=0.99, ema_init=True)
    import inspect
    params = inspect.signature(ops.adam_step).parameters
    assert params["ema"].default is None and params["ema_momentum"].default == 0.0 and params["ema_init"].default is False
    assert import_module("4dflownet_amd.ops_bf16").adam_step is ops.adam_step


def test_trainer_validates_the_ema_arguments():
    """TrainerController(use_ema=, ema_momentum=, ema_overwrite_frequency=, ema_validation=) and every later optimiser step go through
    trainer._ema_arguments (construction needs a device; the helper does not)."""
    import inspect
    trainer = import_module("4dflownet_amd.trainer")
    check = trainer._ema_arguments
    assert check(False, 0.99, None) == (False, float(np.float32(0.99)), None, False)
    assert check(True, 0, 3, True) == (True, 0.0, 3, True)
    assert check(True, np.float32(0.5), np.int64(1)) == (True, 0.5, 1, False)
    assert check(True, 0.999, None)[1] == E.mom32(0.999)
    for bad in (1.0, 1, 1.5, -0.1, -1e-30, float("nan"), float("inf"), -float("inf"), 0.999999999, 1e300, "0.9", True, False, [0.9], None, object()):
        with pytest.raises(ValueError, match="ema_momentum"):
            check(True, bad, None)
    for bad in (0, -1, 1.0, 2.5, "2", True, False, [2], float("nan")):
        with pytest.raises(ValueError, match="ema_overwrite_frequency"):
            check(True, 0.99, bad)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="use_ema"):
            check(bad, 0.99, None)
        with pytest.raises(ValueError, match="ema_validation"):
            check(True, 0.99, None, bad)
    with pytest.raises(ValueError, match="ema_validation=True .* needs use_ema=True"):
        check(False, 0.99, None, True)
    params = inspect.signature(trainer.TrainerController.__init__).parameters
    assert params["use_ema"].default is False and params["ema_momentum"].default == 0.99
    assert params["ema_overwrite_frequency"].default is None and params["ema_validation"].default is False
    src = inspect.getsource(trainer.TrainerController)
    assert src.count("self._checked_ema()") >= 4                      # construction, train_step, every optimiser step (_adam), logging
    assert "return _ema_arguments(self.use_ema, self.ema_momentum, self.ema_overwrite_frequency, self.ema_validation)" in src
    for name in ("finalize_ema", "ema_weights"):
        assert callable(getattr(trainer.TrainerController, name))


def test_float64_restatement_is_the_recurrence():
    """tests/_ema_ref.py against a literal loop over elements and steps, with the init and the frozen rule."""
    rng = np.random.default_rng(11)
    n, T = 37, 5
    frozen = (rng.random(n) < 0.3).astype(np.uint8)
    for fz in (None, frozen):
        weights = [rng.standard_normal(n).astype(np.float32)]
        for _ in range(T):
            step = (1e-2 * rng.standard_normal(n)).astype(np.float32)
            if fz is not None:
                step[fz != 0] = 0                                        # a frozen weight does not move
            weights.append(weights[-1] + step)
        for momentum in (0.0, 0.5, 0.99, 0.999):
            mom = float(np.float32(momentum))
            assert E.mom32(momentum) == mom
            got = E.ema_chain(weights, momentum, frozen=fz)
            assert len(got) == T
            a = [float(x) for x in weights[0]]                           # a_0 = w_0
            for t in range(1, T + 1):
                for i in range(n):
                    if fz is not None and fz[i]:
                        a[i] = float(weights[t - 1][i])
                    else:
                        a[i] = mom * a[i] + (1.0 - mom) * float(weights[t][i])
                assert np.array_equal(got[t - 1], np.array(a)), (momentum, t)
            if momentum == 0.0:
                assert all(np.array_equal(got[t - 1], weights[t].astype(np.float64)) for t in range(1, T + 1))
            bound = E.ema_bound(weights, got)
            big = np.max(np.abs(np.stack([w.astype(np.float64) for w in weights] + got)), axis=0)
            assert np.array_equal(bound, 4 * T * 2.0 ** -24 * big)
    # init ignores the old average, NaN included; without init it is read
    w0, w1 = np.array([1.0, 2.0]), np.array([3.0, 6.0])
    junk = np.array([np.nan, np.nan])
    assert np.array_equal(E.ema_step(junk, w0, w1, 0.5, init=True), np.array([2.0, 4.0]))
    assert np.isnan(E.ema_step(junk, w0, w1, 0.5)).all()
    assert np.array_equal(E.ema_step(junk, w0, w0, 0.5, frozen=np.array([1, 1])), w0)

"""CPU-side checks of gradient accumulation's boundary: fdn_grad_accumulate in the header, the ctypes table and both libraries, the
version it leaves alone, and every argument error of its reported before the device is touched (the pointers here are never
dereferenced).  TrainerController validates accum_steps before it builds the model, so the refusals need no GPU either."""
import ctypes
import os
import re
from importlib import import_module

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fdn_grad_accumulate"


def test_header_ctypes_table_and_both_libraries_hold_the_entry_point(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    assert NAME in declared and NAME in fdn._lib.SIGNATURES
    proto = header[:header.index("int " + NAME + "(")]
    comment = proto[proto.rindex("/*"):]
    assert "TrainerController.py:223" in comment and ":245-249" in comment
    res, args = fdn._lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    build = import_module("4dflownet_amd.build")
    for path in (build.build_library(), build.build_library(test_hooks=True)):
        assert hasattr(ctypes.CDLL(path), NAME), path
    assert fdn._lib.load().fdn_version() == 161 == fdn._lib.FDN_VERSION          # purely additive: the version stays


def test_grad_accumulate_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    f = lib.fdn_grad_accumulate
    err = lambda: lib.fdn_last_error().decode()
    acc, n = 0x100000, 1000
    far = acc + 4 * n + 4096
    assert f(None, far, n, 0, None) == -1 and NAME in err() and "NULL" in err()
    assert f(acc, None, n, 1, None) == -1 and NAME in err() and "NULL" in err()
    for bad in (0, -1, -(1 << 40)):
        assert f(acc, far, bad, 1, None) == -1 and NAME in err() and "n=%d" % bad in err(), bad
    for first in (2, -1, 256):
        assert f(acc, far, n, first, None) == -1 and NAME in err() and "first" in err(), first
    # overlap: |acc - g| < n floats.  (g = acc + 4 n bytes is the first distance that passes; that accepting call is made on the GPU only)
    for g in (acc, acc + 4 * (n - 1), acc - 4 * (n - 1), acc + 4, acc - 4):
        for first in (0, 1):
            assert f(acc, g, n, first, None) == -1 and NAME in err() and "overlap" in err(), (g - acc, first)


@pytest.mark.parametrize("bad", [0, -1, 1.5, "2", float("nan"), None, True])
def test_trainer_refuses_accum_steps_that_are_no_positive_integer(bad):
    trainer = import_module("4dflownet_amd.trainer")
    with pytest.raises(ValueError, match="accum_steps") as e:
        trainer.TrainerController(8, 2, accum_steps=bad)           # refused before the model (and with it the device) is touched
    assert repr(bad) in str(e.value)


def test_ops_wrapper_refuses_host_tensors_and_unequal_sizes(fdn):
    import torch
    with pytest.raises(fdn.FdnError, match="elements"):
        fdn.ops.grad_accumulate(torch.zeros(4), torch.zeros(5), True)
    with pytest.raises(fdn.FdnError, match="float32"):
        fdn.ops.grad_accumulate(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), True)
    with pytest.raises(fdn.FdnError, match="GPU"):
        fdn.ops.grad_accumulate(torch.zeros(4), torch.zeros(4), False)

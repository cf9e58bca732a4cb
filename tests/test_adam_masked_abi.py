"""CPU-side checks of the masked Adam step's boundary: fdn_adam_step_masked in the header, the ctypes table and both libraries, the version
it leaves alone, and every refusal reported before the device is touched (the pointers here are fake and never dereferenced)."""
import ctypes
import os
import re
from importlib import import_module

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fdn_adam_step_masked"


def test_header_ctypes_table_and_both_libraries_hold_the_entry_point(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    assert NAME in declared and NAME in fdn._lib.SIGNATURES
    proto = header[:header.index("int " + NAME + "(")]
    comment = proto[proto.rindex("/*"):]
    assert "neither read nor written" in comment and "TrainerController.py:129-141" in comment and "bit-identical" in comment
    res, args = fdn._lib.SIGNATURES[NAME]
    p, f = ctypes.c_void_p, ctypes.c_float
    assert res is ctypes.c_int and args == [p, p, p, p, p, p, ctypes.c_int64, f, p, f, f, f, f, p, p, p]
    # fdn_adam_step's list with `frozen` behind is_kernel and `lr_t_dev` behind lr_t
    base = list(fdn._lib.SIGNATURES["fdn_adam_step"][1])
    assert args == base[:5] + [p] + base[5:7] + [p] + base[7:]
    build = import_module("4dflownet_amd.build")
    for path in (build.build_library(), build.build_library(test_hooks=True)):
        assert hasattr(ctypes.CDLL(path), NAME), path
    assert fdn._lib.load().fdn_version() == 161 == fdn._lib.FDN_VERSION          # an option of adam_kernel: the version stays


def test_masked_step_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    f = lib.fdn_adam_step_masked
    err = lambda: lib.fdn_last_error().decode()
    ptrs = dict(w=0x100000, g=0x200000, m=0x300000, v=0x400000, is_kernel=0x500000, frozen=0x600000)
    tail = (1e-3, None, 0.9, 0.999, 1e-7, 1e-6, None, None, None)
    for bad in ptrs:
        a = dict(ptrs)
        a[bad] = None
        rc = f(a["w"], a["g"], a["m"], a["v"], a["is_kernel"], a["frozen"], 1024, *tail)
        assert rc != 0 and NAME in err() and "%s is NULL" % bad in err(), (bad, err())
    for n in (0, -1, -(1 << 40)):
        rc = f(*ptrs.values(), n, *tail)
        assert rc != 0 and NAME in err() and "n=%d" % n in err(), n


def test_ops_wrapper_checks_the_map_before_the_library_is_called(fdn):
    import torch
    z = torch.zeros(8)
    with pytest.raises(fdn.FdnError, match="frozen holds 4 bytes for 8 parameters"):
        fdn.ops.adam_step(z, z, z, z, z.to(torch.uint8), 1e-3, 0.9, 0.999, 1e-7, 0.0, frozen=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(fdn.FdnError, match="GPU"):
        fdn.ops.adam_step(z, z, z, z, z.to(torch.uint8), 1e-3, 0.9, 0.999, 1e-7, 0.0, frozen=torch.zeros(8, dtype=torch.uint8))

"""CPU-side checks of the pieces a train step recorded into a HIP graph needs: fdn_adam_step_dev, the device-scalar form of fdn_adam_step
(a by-value step size would be frozen into the graph), and a Mean whose total stays the same tensor over resets."""
import ctypes
from importlib import import_module

import pytest


def test_adam_step_dev_refuses_bad_arguments_before_it_touches_the_device(fdn):
    """A NULL lr_t_dev and n <= 0 come back as FDN_ERR_BAD_ARG (-1) with the function's name in fdn_last_error(); the pointers are never
    dereferenced and no device call is made (this runs without a GPU)."""
    lib = fdn._lib.load()
    assert "fdn_adam_step_dev" in fdn._lib.SIGNATURES
    f = lib.fdn_adam_step_dev
    err = lambda: lib.fdn_last_error().decode()
    w, g, m, v, isk, lr, slot, part = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000
    tail = (0.9, 0.999, 1e-7, 1e-6, slot, part, None)
    assert f(w, g, m, v, isk, 1024, None, *tail) == -1
    assert "fdn_adam_step_dev" in err() and "lr_t_dev" in err()
    for n in (0, -5):
        assert f(w, g, m, v, isk, n, lr, *tail) == -1
        assert "fdn_adam_step_dev" in err() and "n=%d" % n in err()
    assert f(None, g, m, v, isk, 1024, lr, *tail) == -1 and "fdn_adam_step_dev" in err()
    # same argument list as fdn_adam_step except for the step size: a pointer in place of the float
    a, b = fdn._lib.SIGNATURES["fdn_adam_step"][1], fdn._lib.SIGNATURES["fdn_adam_step_dev"][1]
    assert len(a) == len(b) and [i for i in range(len(a)) if a[i] is not b[i]] == [6]
    assert a[6] is ctypes.c_float and b[6] is ctypes.c_void_p


def test_ops_adam_step_refuses_a_host_lr_t_dev(fdn, monkeypatch):
    """lr_t_dev on the host, or of another dtype, is refused by adam_step's own check: the other operands are made to pass theirs (the
    pointer conversion is replaced, the library is never reached)."""
    import torch
    monkeypatch.setattr(fdn.ops, "_p", lambda t, name="tensor", allow_none=False: None if t is None else t.data_ptr())
    z = torch.zeros(4)
    for bad in (torch.zeros(1), torch.zeros(1, dtype=torch.float64), torch.zeros(0)):
        with pytest.raises(fdn.FdnError, match="lr_t_dev"):
            fdn.ops.adam_step(z, z, z, z, z.to(torch.uint8), 1e-3, 0.9, 0.999, 1e-7, 0.0, lr_t_dev=bad)


def test_mean_is_zeroed_in_place():
    """A captured step accumulates into the tensor result() reads: reset_states must keep that tensor."""
    import torch
    trainer = import_module("4dflownet_amd.trainer")
    m = trainer.Mean("x", "cpu")
    total = m._total
    m.update_state(torch.tensor([1.0, 3.0]))
    m.update_state(2.0)
    assert m.result() == 2.0 and m._count == 3
    m.reset_states()
    assert m._total is total and m.result() == 0.0 and m._count == 0
    m.update_state(torch.tensor([5.0]))
    assert m.result() == 5.0

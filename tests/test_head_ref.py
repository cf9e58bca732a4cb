"""tests/_head_ref.py (the float64 reference the GPU tests run on the device at 10^5..10^6 voxels) against the numpy oracle, on the CPU.

Shapes: a ragged one, and two with extents of 1 (there the low and the high face of an axis are the same voxel: all eight corner cases of the
fold).  1e-12 of scale: both sides are float64 sums of the same <= 1728 (forward, dgrad) or N*D*H*W (wgrad) products in another order."""
import numpy as np
import pytest
import torch

from oracle import flownet_oracle as O

import _head_ref as R

SHAPES = [(2, 5, 7, 9), (1, 1, 2, 3), (1, 4, 1, 8)]
TOL = 1e-12


def _operands(shape):
    rng = np.random.default_rng(sum(shape))
    N, D, H, W = shape
    x = rng.normal(size=(N, D, H, W, 64))
    w = rng.normal(size=(3, 3, 3, 64, 1)) * 0.1
    b = rng.normal(size=1)
    dpred = rng.normal(size=(N, D, H, W, 3))
    return x, w, b, dpred


def _close(got, ref, name):
    got = got.numpy()
    assert got.shape == ref.shape and got.dtype == np.float64, (name, got.shape, ref.shape, got.dtype)
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    assert err <= TOL * scale, "%s: %.3e of scale %.3e" % (name, err, scale)


@pytest.mark.parametrize("shape", SHAPES)
def test_head_ref_matches_the_oracle(shape):
    x, w, b, dpred = _operands(shape)
    N, D, H, W = shape
    tx, tw, tb, tz = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), torch.from_numpy(dpred)[..., 1]   # (a strided channel of dpred)
    dz = dpred[..., 1:2]
    _close(R.head_fwd_ref(tx, tw, tb), O.conv3d_fwd(x, w, b)[..., 0], "forward")
    _close(R.head_fwd_ref(tx, tw), O.conv3d_fwd(x, w)[..., 0], "forward without bias")
    dx = O.conv3d_dgrad(dz, w, x.shape)
    got = R.head_dgrad_ref(tz, tw, shape)
    _close(got, dx, "dgrad")
    _close(got.reshape(-1, 64).sum(dim=0), O.bias_grad(dx), "producer bias gradient")
    _close(R.head_wgrad_ref(tx, tz), O.conv3d_wgrad(x, dz, 3), "wgrad")
    _close(R.head_wgrad_bound(tx, tz), O.conv3d_wgrad(np.abs(x), np.abs(dz), 3), "wgrad bound")
    _close(R.head_fold(tz, shape).sum(dim=(0, 1, 2, 3)), np.full(27, O.bias_grad(dz)[0]), "every tap column sums to the bias gradient")


def test_head_ref_takes_float32_and_bfloat16_operands():
    """The GPU tests hand over fp32 / bf16 tensors: they are widened exactly, not computed in."""
    x, w, b, dpred = _operands((1, 3, 4, 5))
    x32, w32, z32 = torch.from_numpy(x).float(), torch.from_numpy(w).float(), torch.from_numpy(dpred).float()[..., 2]
    xb = x32.to(torch.bfloat16)
    for xx in (x32, xb):
        _close(R.head_fwd_ref(xx, w32), O.conv3d_fwd(xx.double().numpy(), w32.double().numpy())[..., 0], "forward %s" % xx.dtype)
        _close(R.head_wgrad_ref(xx, z32), O.conv3d_wgrad(xx.double().numpy(), z32.double().numpy()[..., None], 3), "wgrad %s" % xx.dtype)
    _close(R.head_dgrad_ref(z32, w32, (1, 3, 4, 5)), O.conv3d_dgrad(z32.double().numpy()[..., None], w32.double().numpy(), x.shape), "dgrad float32")

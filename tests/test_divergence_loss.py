"""CPU checks of the divergence loss: the float64 helper (tests/_divergence.py) against torch-CPU autograd of the reference written
literally (src/Network/loss_utils.py:4-62, src/Network/TrainerController.py:84-127 with lines 111-120 live), and the argument checks of
fdn_loss_metrics_div, which need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _divergence import divergence_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_kernels():
    """create_divergence_kernels (loss_utils.py:4-28) as (1,1,3,3,3) conv3d weights; tf's [depth, height, width] = torch's [D, H, W]."""
    ks = []
    for taps in (((0, 1, 1), (2, 1, 1)), ((1, 0, 1), (1, 2, 1)), ((1, 1, 0), (1, 1, 2))):
        k = torch.zeros((3, 3, 3), dtype=torch.float64)
        k[taps[0]] = 1
        k[taps[1]] = -1
        ks.append(k.reshape(1, 1, 3, 3, 3))
    return ks


def _reference_loss(pred, truth, mask, div_weight):
    """TrainerController.loss_function's divergence part, literally: calculate_gradient = SYMMETRIC pad 1 (replicate, for a pad of 1) +
    VALID conv3d (:30-45), calculate_divergence_loss2 (:58-62), then the weight and the +1 masked means (TrainerController.py:111-120)."""
    kx, ky, kz = _reference_kernels()

    def gradient(image, kernel):
        x = F.pad(image.unsqueeze(1), (1, 1, 1, 1, 1, 1), mode="replicate")
        return F.conv3d(x, kernel).squeeze(1)

    u, v, w = truth[..., 0], truth[..., 1], truth[..., 2]
    up, vp, wp = pred[..., 0], pred[..., 1], pred[..., 2]
    divpx, divpy, divpz = gradient(up, kx), gradient(vp, ky), gradient(wp, kz)
    divx, divy, divz = gradient(u, kx), gradient(v, ky), gradient(w, kz)
    divergence_loss = (divpx - divx) ** 2 + (divpy - divy) ** 2 + (divpz - divz) ** 2
    divergence_loss = div_weight * divergence_loss
    non_fluid_mask = (mask < 0.5).to(torch.float64)
    fluid = (divergence_loss * mask).sum(dim=(1, 2, 3)) / (mask.sum(dim=(1, 2, 3)) + 1)
    non_fluid = (divergence_loss * non_fluid_mask).sum(dim=(1, 2, 3)) / (non_fluid_mask.sum(dim=(1, 2, 3)) + 1)
    return fluid + non_fluid


SHAPES = [(2, 1, 4, 5), (2, 4, 1, 5), (2, 4, 5, 1), (1, 2, 3, 4), (1, 3, 2, 4), (1, 3, 4, 2), (2, 2, 2, 2), (1, 1, 1, 1),
          (3, 5, 6, 7), (1, 1, 1, 6)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mask_kind", ["binary", "fractional"])
def test_helper_matches_autograd_of_the_reference(shape, mask_kind):
    rng = np.random.default_rng(sum(shape) * 7 + len(mask_kind))
    pred = rng.normal(size=shape + (3,))
    truth = rng.normal(size=shape + (3,))
    if mask_kind == "binary":
        mask = (rng.uniform(size=shape) < 0.4).astype(np.float64)
    else:
        mask = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], size=shape) * rng.uniform(0.5, 1.0, size=shape)
        mask.reshape(-1)[::3] = 0.5                       # exactly on the threshold: fluid weight 0.5, not non-fluid
    wgt = 0.7
    div_b, dpred = divergence_loss(pred, truth, mask, wgt)
    tp = torch.tensor(pred, requires_grad=True)
    ref = _reference_loss(tp, torch.tensor(truth), torch.tensor(mask), wgt)
    ref.sum().backward()                                  # tape.gradient of the (B,) loss = gradient of its sum
    ref_v = ref.detach().numpy()
    ref_g = tp.grad.numpy()
    assert np.abs(div_b - ref_v).max() <= 1e-12 * max(np.abs(ref_v).max(), 1.0)
    assert np.abs(dpred - ref_g).max() <= 1e-12 * max(np.abs(ref_g).max(), 1.0)
    # the term is live: non-zero wherever an axis has two voxels or more
    if max(shape[1:]) > 1:
        assert np.abs(ref_g).max() > 0.1


def test_header_scratch_size_matches_the_python_binding():
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    m = re.search(r"#define FDN_LOSS_DIV_SCRATCH_FLOATS\(N\) \(\(N\) \* \(8 \+ 5 \* FDN_LOSS_BLOCKS\)\)", header)
    assert m and "#define FDN_LOSS_BLOCKS 256" in header
    src = open(os.path.join(ROOT, "4dflownet_amd", "ops.py")).read()
    assert "N * (8 + 5 * 256)" in src


def test_loss_metrics_div_argument_checks_need_no_gpu(fdn):
    """fdn_loss_metrics_div refuses NULL operands, non-positive extents and a non-finite or negative weight before it touches the
    device (the pointers here are never dereferenced), naming itself in fdn_last_error()."""
    lib = fdn._lib.load()
    f = lib.fdn_loss_metrics_div
    err = lambda: lib.fdn_last_error().decode()
    p = [0x1000 * (k + 1) for k in range(8)]              # pred uh vh wh mask | out dpred scratch
    ok = lambda **kw: dict(dict(ptrs=list(p), w=0.5, N=2, D=4, H=4, W=4), **kw)

    def call(a):
        q = a["ptrs"]
        return f(q[0], q[1], q[2], q[3], q[4], a["w"], q[5], q[6], q[7], a["N"], a["D"], a["H"], a["W"], None)

    for k in (0, 1, 2, 3, 4, 5, 7):                        # every operand but dpred (which may be NULL)
        q = list(p); q[k] = None
        assert call(ok(ptrs=q)) != 0 and "fdn_loss_metrics_div" in err() and "NULL" in err(), k
    for ext in ("N", "D", "H", "W"):
        for bad in (0, -3):
            assert call(ok(**{ext: bad})) != 0 and "fdn_loss_metrics_div" in err() and "extents" in err(), (ext, bad)
    for bad in (-0.5, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert call(ok(w=bad)) != 0 and "fdn_loss_metrics_div" in err() and "div_weight" in err(), bad
    assert call(ok(D=1 << 11, H=1 << 10, W=1 << 10)) != 0 and "2^31" in err()
    assert fdn._lib.SIGNATURES["fdn_loss_metrics_div"][1][5] is ctypes.c_float

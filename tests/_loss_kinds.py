"""Float64 restatement of the data term's penalties (fdn_loss_metrics_kind, ops.loss_metrics(kind=), TrainerController(loss=)).

Per component of the residual d = pred_c - truth_c:
    mse          rho = d^2                                                      psi = 2 d
    mae          rho = |d|                                                      psi = sign(d), psi(0) = 0 (tf.abs' gradient)
    huber        rho = d^2 / 2 if |d| <= delta, else delta (|d| - delta / 2)    psi = d, else delta sign(d)
    charbonnier  rho = sqrt(d^2 + eps^2)                                        psi = d / sqrt(d^2 + eps^2)
Per voxel e = sum_c rho(d_c); with nf = mask < 0.5 and the divergence term d of tests/_divergence.py (squared for every kind)
    data_b = sum(mask e) / (sum(mask) + 1) + non_fluid_weight * sum(nf e) / (sum(nf) + 1)
    div_b  = div_weight * (sum(mask d) / (sum(mask) + 1) + non_fluid_weight * sum(nf d) / (sum(nf) + 1))
and the gradient handed to the network is that of sum_b (data_b + div_b) w.r.t. the heads' pre-activations (times 1 - y^2 under tanh).
Imports nothing from the package under test."""
import numpy as np

from _divergence import AXES, central_diff, central_diff_adjoint

ACT_NONE, ACT_TANH = 0, 3
KINDS = {"mse": 0, "mae": 1, "huber": 2, "charbonnier": 3}          # FDN_LOSS_*
DEFAULT_PARAM = {"huber": 1.0, "charbonnier": 1e-3}


def rho_psi(d, kind, param=None, sign=None):
    """(rho(d), rho'(d)) elementwise in float64.  sign (mae only): the sign every residual is taken to have, instead of its own -- the
    side of the kink at d = 0 another forward pass landed on."""
    d = np.asarray(d, np.float64)
    if kind == "mse":
        return d * d, 2.0 * d
    if kind == "mae":
        return np.abs(d), (np.sign(d) if sign is None else np.asarray(sign, np.float64))
    if kind == "huber":
        delta = float(DEFAULT_PARAM["huber"] if param is None else param)
        a = np.abs(d)
        inner = a <= delta
        return np.where(inner, 0.5 * d * d, delta * (a - 0.5 * delta)), np.where(inner, d, delta * np.sign(d))
    if kind == "charbonnier":
        eps = float(DEFAULT_PARAM["charbonnier"] if param is None else param)
        s = np.sqrt(d * d + eps * eps)
        return s, d / s
    raise ValueError(kind)


def voxel_weight(mask, non_fluid_weight):
    """c = mask / (sum mask + 1) + nf * non_fluid_weight / (sum nf + 1): the weight of a voxel's term in its sample's loss."""
    mask = np.asarray(mask, np.float64)
    ax = (1, 2, 3)
    nf = (mask < 0.5).astype(np.float64)
    inv_f = 1.0 / (mask.sum(axis=ax) + 1)
    inv_nf = non_fluid_weight / (nf.sum(axis=ax) + 1)
    return mask * inv_f[:, None, None, None] + nf * inv_nf[:, None, None, None]


def loss_reference(pred, truth, mask, kind="mse", param=None, div_weight=0.0, non_fluid_weight=1.0, out_act=ACT_NONE, sign=None):
    """pred (the heads' OUTPUT), truth (N,D,H,W,3), mask (N,D,H,W) -> data_b (N,), div_b (N,), d(sum_b (data_b + div_b)) / d(heads'
    pre-activations), in float64."""
    pred = np.asarray(pred, np.float64); truth = np.asarray(truth, np.float64)
    ax = (1, 2, 3)
    cw = voxel_weight(mask, non_fluid_weight)
    e = pred - truth
    rho, psi = rho_psi(e, kind, param, sign)
    data_b = (rho.sum(axis=-1) * cw).sum(axis=ax)
    g = [central_diff(e[..., c], AXES[c]) for c in range(3)]
    d = g[0] ** 2 + g[1] ** 2 + g[2] ** 2
    div_b = div_weight * (d * cw).sum(axis=ax)
    dz = psi * cw[..., None]
    dz = dz + np.stack([central_diff_adjoint(2.0 * div_weight * cw * g[c], AXES[c]) for c in range(3)], axis=-1)
    if out_act == ACT_TANH:
        dz = dz * (1.0 - pred * pred)
    return data_b, div_b, dz


def data_gradient_fp32(pred, truth, mask, kind, param, non_fluid_weight, out_act):
    """numpy float32 emulation of the straightforward path of the data term's gradient (div_weight = 0), rounding where fp32 code rounds:
    d, psi (square, add, sqrt, divide), the voxel weight m * inv_f + nf * inv_nf, the product, 1 - y^2 and its product.  The CPU figure
    the 16-rounding bound of tests/test_gpu_loss_kinds.py is compared with."""
    f = np.float32
    pred = np.asarray(pred, f); truth = np.asarray(truth, f); mask = np.asarray(mask, f)
    nf = (mask < f(0.5)).astype(f)
    sm = mask.astype(np.float64).sum(axis=(1, 2, 3)).astype(f)          # (the kernel's counts: exact for binary masks)
    sn = nf.astype(np.float64).sum(axis=(1, 2, 3)).astype(f)
    inv_f = (f(1) / (sm + f(1))).astype(f)
    inv_nf = (f(non_fluid_weight) * (f(1) / (sn + f(1))).astype(f)).astype(f)
    c0 = ((mask * inv_f[:, None, None, None]).astype(f) + (nf * inv_nf[:, None, None, None]).astype(f)).astype(f)
    d = (pred - truth).astype(f)
    if kind == "mae":
        psi = np.sign(d).astype(f)
    elif kind == "huber":
        psi = np.where(np.abs(d) <= f(param), d, np.copysign(f(param), d)).astype(f)
    elif kind == "charbonnier":
        s = np.sqrt(((d * d).astype(f) + (f(param) * f(param)).astype(f)).astype(f)).astype(f)
        psi = (d / s).astype(f)
    else:
        psi = (f(2) * d).astype(f)
    g = (psi * c0[..., None]).astype(f)
    if out_act == ACT_TANH:
        y = pred.astype(np.float64)
        g = (g * (1.0 - y * y).astype(f)).astype(f)          # fmaf(-y, y, 1): y * y is exact in float64, so this rounds once
    return g

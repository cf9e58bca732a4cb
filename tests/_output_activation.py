"""Float64 reference of the two options fdn_loss_metrics_act adds to the loss pass: the reference's non_fluid_weight ("Weighting for non
fluid region", src/Network/TrainerController.py:24) and the bounded output of the heads, Keras' Conv3D(activation='tanh').

Per sample, with e = pred - truth, d the divergence term of tests/_divergence.py, nf = mask < 0.5:
    mse_b = sum(mask e^2) / (sum(mask) + 1) + non_fluid_weight * sum(nf e^2) / (sum(nf) + 1)
    div_b = div_weight * (sum(mask d) / (sum(mask) + 1) + non_fluid_weight * sum(nf d) / (sum(nf) + 1))
and the gradient handed to the network is that of sum_b (mse_b + div_b) w.r.t. the heads' PRE-activations z: pred = tanh(z) multiplies
every component of the gradient w.r.t. pred by 1 - pred^2 (TensorFlow's TanhGrad works from the output as well)."""
import numpy as np

from oracle import flownet_oracle as O          # noqa: F401  (the network the train-step tests differentiate)
from _divergence import AXES, central_diff, central_diff_adjoint

ACT_NONE, ACT_TANH = 0, 3


def activation(z, out_act):
    z = np.asarray(z, np.float64)
    return np.tanh(z) if out_act == ACT_TANH else z


def weighted_loss(pred, truth, mask, div_weight=0.0, non_fluid_weight=1.0):
    """pred, truth (N,D,H,W,3), mask (N,D,H,W) -> mse_b (N,), div_b (N,), d(sum_b (mse_b + div_b)) / dpred, in float64."""
    pred = np.asarray(pred, np.float64); truth = np.asarray(truth, np.float64); mask = np.asarray(mask, np.float64)
    ax = (1, 2, 3)
    nf = (mask < 0.5).astype(np.float64)
    inv_f = 1.0 / (mask.sum(axis=ax) + 1)
    inv_nf = non_fluid_weight / (nf.sum(axis=ax) + 1)
    cw = mask * inv_f[:, None, None, None] + nf * inv_nf[:, None, None, None]        # the weight of a voxel's term in its sample's loss
    e = pred - truth
    mse_b = ((e ** 2).sum(axis=-1) * cw).sum(axis=ax)
    g = [central_diff(e[..., c], AXES[c]) for c in range(3)]
    d = g[0] ** 2 + g[1] ** 2 + g[2] ** 2
    div_b = div_weight * (d * cw).sum(axis=ax)
    dpred = 2.0 * e * cw[..., None]
    dpred = dpred + np.stack([central_diff_adjoint(2.0 * div_weight * cw * g[c], AXES[c]) for c in range(3)], axis=-1)
    return mse_b, div_b, dpred


def loss_reference(pred, truth, mask, div_weight=0.0, non_fluid_weight=1.0, out_act=ACT_NONE):
    """What fdn_loss_metrics_act returns for a prediction `pred` (the heads' OUTPUT): mse_b, div_b and the gradient w.r.t. the
    pre-activations."""
    mse_b, div_b, dpred = weighted_loss(pred, truth, mask, div_weight, non_fluid_weight)
    if out_act == ACT_TANH:
        y = np.asarray(pred, np.float64)
        dpred = dpred * (1.0 - y * y)
    return mse_b, div_b, dpred


def total_loss_of_preactivations(z, truth, mask, div_weight, non_fluid_weight, out_act):
    """sum_b (mse_b + div_b) as a function of the pre-activations: what the finite differences differentiate."""
    mse_b, div_b, _ = weighted_loss(activation(z, out_act), truth, mask, div_weight, non_fluid_weight)
    return float((mse_b + div_b).sum())


def ulp_distance(got, ref):
    """|got - ref| in units of ref's float32 spacing, elementwise (got, ref float32 arrays; ref the correctly rounded value)."""
    got = np.asarray(got, np.float32); ref = np.asarray(ref, np.float32)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)

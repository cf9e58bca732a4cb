"""Float64 restatement of the divergence loss of the reference and of its gradient: the yardstick of fdn_loss_metrics_div.

src/Network/loss_utils.py:4-62: per velocity component a central difference along ONE axis, a 3x3x3 `tf.nn.conv3d` (a
cross-correlation) over a SYMMETRIC pad of 1 (an edge clamp): kernel_x (:10-14, taps [0,1,1] = +1, [2,1,1] = -1) differentiates u
along the first spatial axis D, kernel_y (:16-20) v along H, kernel_z (:22-26) w along W; calculate_divergence_loss2 (:58-62) squares
the differences of prediction and truth.  src/Network/TrainerController.py:84-127 weights the voxel term by div_weight (:112) and takes
the fluid / non-fluid masked means with the same +1 as the MSE (:114-120); the sample's loss is mse_b + div_b (:124)."""
import numpy as np

AXES = (1, 2, 3)          # channel c of pred (N,D,H,W,3) differentiates along array axis AXES[c]


def central_diff(x, axis):
    """(Da x)[i] = x[clamp(i-1)] - x[clamp(i+1)] along `axis` (loss_utils.py:30-45)."""
    n = x.shape[axis]
    i = np.arange(n)
    return np.take(x, np.clip(i - 1, 0, n - 1), axis=axis) - np.take(x, np.clip(i + 1, 0, n - 1), axis=axis)


def central_diff_adjoint(r, axis):
    """Da^T r: r[j+1] - r[j-1] inside, r[0] + r[1] at the first voxel, -(r[n-2] + r[n-1]) at the last, 0 on an axis of extent 1."""
    r = np.moveaxis(r, axis, -1)
    n = r.shape[-1]
    out = np.zeros_like(r)
    if n > 1:
        out[..., 1:n - 1] = r[..., 2:] - r[..., :n - 2]
        out[..., 0] = r[..., 0] + r[..., 1]
        out[..., n - 1] = -(r[..., n - 2] + r[..., n - 1])
    return np.moveaxis(out, -1, axis)


def divergence_loss(pred, truth, mask, div_weight):
    """pred, truth (N,D,H,W,3), mask (N,D,H,W) -> div_b (N,) and dpred (N,D,H,W,3) = d(sum_b div_b)/dpred, in float64."""
    pred = np.asarray(pred, np.float64); truth = np.asarray(truth, np.float64); mask = np.asarray(mask, np.float64)
    g = [central_diff(pred[..., c], AXES[c]) - central_diff(truth[..., c], AXES[c]) for c in range(3)]
    d = g[0] ** 2 + g[1] ** 2 + g[2] ** 2
    nf = (mask < 0.5).astype(np.float64)
    sm = mask.sum(axis=(1, 2, 3))
    snf = nf.sum(axis=(1, 2, 3))
    div_b = div_weight * ((d * mask).sum(axis=(1, 2, 3)) / (sm + 1) + (d * nf).sum(axis=(1, 2, 3)) / (snf + 1))
    cw = mask / (sm + 1)[:, None, None, None] + nf / (snf + 1)[:, None, None, None]
    dpred = np.stack([central_diff_adjoint(2.0 * div_weight * cw * g[c], AXES[c]) for c in range(3)], axis=-1)
    return div_b, dpred

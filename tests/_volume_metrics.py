"""Float64 restatement of fdn_volume_metrics: the yardstick of the whole-volume evaluation (include/fdn.h states the definitions).

pred, truth (F,3,X,Y,Z) planar, mask (1 or F,X,Y,Z).  Per voxel e_c = p_c - t_c, q = sum_c e_c^2, nf = [m < 0.5]
(src/Network/TrainerController.py:96), fl = [m == 1.0] (src/Network/loss_utils.py:91), corr the relative error of loss_utils.py:64-92
rounded to four decimals, g_c the clamped central difference of e_c along the axis paired with the component (tests/_divergence.py),
d = sum_c g_c^2.  The 26 columns are sums of those terms over a frame."""
import numpy as np

from _divergence import central_diff

COLUMNS = 26
BAND = 1e-9               # |corr * 1e4 - (k + 1/2)| below this: the rounding to four decimals could go either way on another machine


def relative_error_terms(pred, truth):
    """(corr before the rounding, corr after it), each (F,X,Y,Z) (loss_utils.py:64-92 in float64)."""
    pred = np.asarray(pred, np.float64); truth = np.asarray(truth, np.float64)
    diff = np.sqrt(((pred - truth) ** 2).sum(axis=1))
    actual = np.sqrt((truth ** 2).sum(axis=1))
    rel = np.clip(diff / (actual + 1e-5), 0.0, 1.0)
    raw = np.where(actual != 0, rel, diff)
    return raw, np.rint(raw * 1e4) / 1e4


def volume_terms(pred, truth, mask):
    """The 26 per-voxel terms, (26,F,X,Y,Z) float64."""
    pred = np.asarray(pred, np.float64); truth = np.asarray(truth, np.float64); mask = np.asarray(mask, np.float64)
    F = pred.shape[0]
    assert pred.ndim == 5 and pred.shape[1] == 3 and truth.shape == pred.shape
    assert mask.shape[1:] == pred.shape[2:] and mask.shape[0] in (1, F)
    m = np.broadcast_to(mask, (F,) + mask.shape[1:])
    nf = (m < 0.5).astype(np.float64)
    fl = (m == 1.0).astype(np.float64)
    e = pred - truth
    q = (e ** 2).sum(axis=1)
    _, corr = relative_error_terms(pred, truth)
    d = sum(central_diff(e[:, c], 1 + c) ** 2 for c in range(3))          # u along X, v along Y, w along Z
    terms = [m, nf, fl, q * m, q * nf, corr * fl] + [e[:, c] ** 2 * fl for c in range(3)] + [d * m, d * nf]
    for c in range(3):
        t, p = truth[:, c], pred[:, c]
        terms += [t * fl, p * fl, t * t * fl, p * p * fl, t * p * fl]
    return np.stack(terms)


def volume_sums(pred, truth, mask):
    """-> (sums (F,26), sums of |term| (F,26), per frame the number of fl voxels whose corr * 1e4 lies within BAND of a half-integer)."""
    terms = volume_terms(pred, truth, mask)
    assert terms.shape[0] == COLUMNS
    sums = terms.sum(axis=(2, 3, 4)).T
    mags = np.abs(terms).sum(axis=(2, 3, 4)).T
    raw, _ = relative_error_terms(pred, truth)
    x = raw * 1e4
    near = np.abs(x - np.floor(x) - 0.5) < BAND
    band = (near & (terms[2] == 1.0)).sum(axis=(1, 2, 3))
    return np.ascontiguousarray(sums), np.ascontiguousarray(mags), band


def bound(mags, voxels_per_frame):
    """|device - yardstick| per column: any order of summing n terms in double differs from any other by at most n 2^-52 sum|term|
    to first order ((n - 1) u each, u = 2^-53), plus a few ulp per term for the device's contracted products and its sqrt / divide:
    (n + 64) 2^-52 sum|term|.  Derived, not measured."""
    return (voxels_per_frame + 64) * 2.0 ** -52 * mags

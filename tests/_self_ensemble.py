"""The geometric self-ensemble restated in numpy: the forward orientation of a patch, the inverse orientation of a prediction and the
fp32 accumulate / divide of the mean -- what fdn_input_features_volume_oriented and fdn_unrotate_accumulate are held to, bit for bit.

An orientation is (plane, k): (0, 0) the identity, else a rotation by k quarter turns (np.rot90) in plane 1:(0,1), 2:(0,2), 3:(1,2), with
the component swap and sign rule of the training loader.  The table below is written out here on its own; test_self_ensemble_host.py
holds it against data.rotate_vector_field."""
import numpy as np

AXES = {1: (0, 1), 2: (0, 2), 3: (1, 2)}
# (plane, k): (perm, sign) -- component i of the rotated field is sign[i] * rot90(component perm[i])
TABLE = {
    (0, 0): ((0, 1, 2), (1, 1, 1)),
    (1, 1): ((0, 2, 1), (1, 1, -1)), (1, 2): ((0, 1, 2), (1, -1, -1)), (1, 3): ((0, 2, 1), (1, -1, 1)),
    (2, 1): ((2, 1, 0), (-1, 1, 1)), (2, 2): ((0, 1, 2), (-1, 1, -1)), (2, 3): ((2, 1, 0), (1, 1, -1)),
    (3, 1): ((1, 0, 2), (-1, 1, 1)), (3, 2): ((0, 1, 2), (-1, -1, 1)), (3, 3): ((1, 0, 2), (1, -1, 1)),
}
ROT90 = ((0, 0), (1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3))


def _rot(a, plane, k, lead):
    """np.rot90 of the three spatial axes that follow `lead` leading axes; the identity for plane 0."""
    if plane == 0:
        return a
    ax = AXES[plane]
    return np.rot90(a, k, axes=(ax[0] + lead, ax[1] + lead))


def forward(comps, orientation, signed=True, lead=0):
    """Three component arrays (velocities with signed=True, magnitudes with False) -> the three of the rotated patch.  The sign is applied by
    an fp32 multiplication (a zero under a negative sign becomes -0.0); lead: number of batch axes in front of the three spatial ones."""
    plane, k = orientation
    perm, sign = TABLE[orientation]
    out = []
    for i in range(3):
        c = np.asarray(comps[perm[i]], dtype=np.float32)
        if signed and sign[i] < 0:
            c = c * np.float32(-1)
        out.append(np.ascontiguousarray(_rot(c, plane, k, lead)))
    return tuple(out)


def inverse(pred, orientation, lead=0):
    """A prediction (..., S, S, S, 3) made in the rotated frame -> the same in the frame of the window: q[perm[i]] = sign[i] * rot90(p[i], 4 - k)."""
    plane, k = orientation
    perm, sign = TABLE[orientation]
    pred = np.asarray(pred, dtype=np.float32)
    out = np.empty_like(pred)
    for i in range(3):
        out[..., perm[i]] = np.float32(sign[i]) * _rot(pred[..., i], plane, (4 - k) % 4, lead)
    return out


def accumulate(pred, acc, orientation, first, divisor=1, lead=1):
    """fdn_unrotate_accumulate in numpy float32: t = inverse(pred); v = t or acc + t; v / divisor where divisor > 1.  Returns the new acc."""
    t = inverse(pred, orientation, lead=lead)
    with np.errstate(invalid="ignore", over="ignore"):          # inf - inf is a NaN here as on the device, not a warning
        v = t if first else (np.asarray(acc, dtype=np.float32) + t).astype(np.float32)
        if divisor > 1:
            v = (v / np.float32(divisor)).astype(np.float32)
    return v


def mean(preds, orientations, lead=1):
    """The ensemble mean of predictions made under `orientations`, summed in list order in fp32, divided once by their number."""
    acc = None
    for j, (p, o) in enumerate(zip(preds, orientations)):
        acc = accumulate(p, acc, o, first=j == 0, divisor=len(orientations) if j == len(orientations) - 1 else 1, lead=lead)
    return acc


def same_bits(a, b):
    """Equal as bit patterns (the sign of zero counts).  Only NaNs are compared as NaNs: IEEE 754 leaves the sign and payload of the NaN an
    invalid operation (inf - inf) produces to the implementation."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    ia, ib = a.view(view), b.view(view)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.array_equal(ia[~na], ib[~nb]))
    return bool(np.array_equal(ia, ib))

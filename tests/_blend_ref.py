"""Reference for overlap-add stitching, in numpy and nothing from the package: the geometry of the overlapping window, the separable
linear-ramp weights, the float32 accumulate in ascending patch order -- what fdn_blend_patches and the host tiler are held to, bit for
bit -- and the same sum in float64 with exact weights, with the bound the float32 result has to keep to it.

Geometry.  P the patch edge, E = P - 4, b the overlap in low-res voxels (0 <= b, 2b <= E), stride s = E - b.  An axis of extent n holds
nr = max(1, ceil((n - E) / s) + 1) patches and a far pad of (nr - 1) s + E - n voxels; voxel (a,b,c) of patch (i,j,k) reads source
(i s + a - 2, j s + b - 2, k s + c - 2), zero outside the volume.  Global patch g: frame g // (nx ny nz), then (i,j,k) with k fastest.

Weights.  R the upsampling factor, C = E R the HR core edge, r = b R the ramp width, t in [0,C) the HR core coordinate.  A patch with a
lower neighbour (i > 0) has w = (float)(2t+1) / (float)(2r) for t < r, one with an upper neighbour (i < nr-1) has
w = (float)(2(C-t)-1) / (float)(2r) for t >= C - r, w = 1 elsewhere.  The voxel weight is fl(fl(wx wy) wz).

Accumulate.  acc = acc + fl(w_g p_g) over the covering patches in ascending g, from a zeroed volume.

Bound.  |float32 - float64| <= 16 * 2^-24 * sum_g w_g |p_g| per voxel: per term three weight roundings, two weight products and the
product with p, on top up to seven adds -- 13 roundings of 2^-24 to first order, rounded up to 16."""
import math

import numpy as np

BOUND_ROUNDINGS = 16
EPS = 2.0 ** -24


def axis_plan(n, P, b):
    """(patches, stride, far pad) of an axis of extent n."""
    E = P - 4
    s = E - b
    nr = max(1, math.ceil((n - E) / s) + 1)
    return nr, s, (nr - 1) * s + E - n


def counts(shape, P, b):
    return tuple(axis_plan(int(n), P, b)[0] for n in shape)


def patches(vol, P, b):
    """The overlapping window patches of one low-res volume (X,Y,Z): (nx*ny*nz,P,P,P), k fastest, zero outside the volume."""
    nr = counts(vol.shape, P, b)
    s = P - 4 - b
    out = np.zeros((nr[0] * nr[1] * nr[2], P, P, P), vol.dtype)
    g = 0
    for i in range(nr[0]):
        for j in range(nr[1]):
            for k in range(nr[2]):
                for a in range(P):
                    x = i * s + a - 2
                    if not 0 <= x < vol.shape[0]:
                        continue
                    for bb in range(P):
                        y = j * s + bb - 2
                        if not 0 <= y < vol.shape[1]:
                            continue
                        z0 = k * s - 2
                        lo, hi = max(z0, 0), min(z0 + P, vol.shape[2])
                        if hi > lo:
                            out[g, a, bb, lo - z0:hi - z0] = vol[x, y, lo:hi]
                g += 1
    return out


def axis_weights32(i, nr, C, r):
    """float32 weights along one axis of patch i of nr: one correctly rounded fp32 divide per ramp voxel."""
    w = np.ones(C, np.float32)
    for t in range(C):
        if i > 0 and t < r:
            w[t] = np.float32(2 * t + 1) / np.float32(2 * r)
        elif i < nr - 1 and t >= C - r:
            w[t] = np.float32(2 * (C - t) - 1) / np.float32(2 * r)
    return w


def axis_weights64(i, nr, C, r):
    """The same weights in float64 (exact: odd numerators over 2r, far inside the 53 bits)."""
    w = np.ones(C, np.float64)
    for t in range(C):
        if i > 0 and t < r:
            w[t] = (2 * t + 1) / (2 * r)
        elif i < nr - 1 and t >= C - r:
            w[t] = (2 * (C - t) - 1) / (2 * r)
    return w


def _walk(pred, F, nr, side, stride_hr, g0):
    """(frame, destination slices, core of the patch, (i,j,k)) of every patch of pred (count,S,S,S,3), global patches g0 .. in order."""
    S = pred.shape[1]
    C = S - 2 * side
    per = nr[0] * nr[1] * nr[2]
    for n in range(pred.shape[0]):
        g = g0 + n
        f, rem = divmod(g, per)
        assert f < F
        i, rem = divmod(rem, nr[1] * nr[2])
        j, k = divmod(rem, nr[2])
        core = pred[n, side:S - side, side:S - side, side:S - side]
        yield f, tuple(slice(q * stride_hr, q * stride_hr + C) for q in (i, j, k)), core, (i, j, k)


def _full_extents(nr, C, stride_hr):
    return tuple((q - 1) * stride_hr + C for q in nr)


def blend32(pred, F, nr, side, stride_hr, extents, g0=0, acc=None):
    """The float32 emulation: pred (count,S,S,S,3) float32, the predictions of global patches g0 .. g0 + count - 1 of F frames of
    nr = (nx,ny,nz) patches -> acc (F,3) + extents float32 (zeroed when not given; given: added to, as a later call of the kernel does).
    acc = acc + fl(fl(fl(wx wy) wz) p), patch after patch in ascending g; voxels beyond the extents (the far pad) are dropped."""
    pred = np.asarray(pred)
    assert pred.dtype == np.float32
    C = pred.shape[1] - 2 * side
    r = C - stride_hr
    full = np.zeros((F, 3) + _full_extents(nr, C, stride_hr), np.float32)
    X, Y, Z = extents
    if acc is not None:
        assert acc.dtype == np.float32
        full[:, :, :X, :Y, :Z] = acc
    for f, (sx, sy, sz), core, (i, j, k) in _walk(pred, F, nr, side, stride_hr, g0):
        wx, wy, wz = (axis_weights32(q, n, C, r) for q, n in zip((i, j, k), nr))
        w = (wx[:, None, None] * wy[None, :, None]) * wz[None, None, :]
        assert w.dtype == np.float32
        for c in range(3):
            term = w * core[..., c]
            full[f, c, sx, sy, sz] = full[f, c, sx, sy, sz] + term
    return np.ascontiguousarray(full[:, :, :X, :Y, :Z])


def blend64(pred, F, nr, side, stride_hr, extents, g0=0):
    """The same sum in float64 with exact weights, and sum_g w_g |p_g| per voxel: (value, magnitude), each (F,3) + extents float64."""
    pred = np.asarray(pred, np.float64)
    C = pred.shape[1] - 2 * side
    r = C - stride_hr
    val = np.zeros((F, 3) + _full_extents(nr, C, stride_hr), np.float64)
    mag = np.zeros_like(val)
    for f, (sx, sy, sz), core, (i, j, k) in _walk(pred, F, nr, side, stride_hr, g0):
        wx, wy, wz = (axis_weights64(q, n, C, r) for q, n in zip((i, j, k), nr))
        w = wx[:, None, None] * wy[None, :, None] * wz[None, None, :]
        for c in range(3):
            val[f, c, sx, sy, sz] += w * core[..., c]
            mag[f, c, sx, sy, sz] += w * np.abs(core[..., c])
    X, Y, Z = extents
    return np.ascontiguousarray(val[:, :, :X, :Y, :Z]), np.ascontiguousarray(mag[:, :, :X, :Y, :Z])


def within_bound(got32, val64, mag64):
    """|got32 - val64| <= 16 * 2^-24 * mag64 everywhere; returns (ok, the largest error in units of 2^-24 * magnitude)."""
    err = np.abs(np.asarray(got32, np.float64) - val64)
    ok = bool((err <= BOUND_ROUNDINGS * EPS * mag64).all())
    worst = float((err[mag64 > 0] / (EPS * mag64[mag64 > 0])).max()) if (mag64 > 0).any() else 0.0
    return ok, worst


def finish(vol, scale):
    """The predictor's post-processing on an fp32 volume (F,3,...): d = (double)v * venc_f, +0.0 where fabs(d) < threshold_f (strict)."""
    out = np.empty(vol.shape, np.float64)
    for f, (venc, thr) in enumerate(scale):
        d = vol[f].astype(np.float64) * np.float64(venc)
        d[np.abs(d) < np.float64(thr)] = 0.0
        out[f] = d
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()

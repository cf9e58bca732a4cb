"""Operator layer: torch tensors (containers only) -> raw pointers -> lib4dflow_hip.so.

Every function launches asynchronously on torch's current HIP stream and returns its output tensor(s).
Tensors must be fp32, contiguous and on a ROCm device; anything else raises (no CPU path)."""
import ctypes
import functools
import math
import numbers
import operator
import struct

import numpy as np
import torch

from . import _lib
from ._lib import FdnError, check

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
ACT_TANH = 3            # FDN_ACT_TANH: the bounded output of the 64->1 heads (conv3d_fwd on that route, loss_metrics(out_act=))
# FDN_ALGO_*: per-call algorithm of the 64->64 3x3x3 entry points (AUTO = Winograd along W when W % 4 == 0, DIRECT = never)
# ALGO_WINO_BF16X3: like AUTO, the F(4,3)xF(4,3) products on the bf16 matrix pipe (operands split exactly into 3 bf16 pieces, 6 terms, fp32 accumulation)
ALGO_AUTO, ALGO_DIRECT, ALGO_WINO_W, ALGO_WINO_H2, ALGO_WINO_BF16X3 = 0, 1, 2, 3, 4
LEAKY_ALPHA = 0.2
# FDN_CONV64_PACK_FLOATS (mirrored; _lib.load() checks fdn_version() against FDN_VERSION below): direct stream (27 taps) + Winograd F(4,3)
# stream (54) + 2-D F(2,3)xF(4,3) stream (72) + 2-D F(4,3)xF(4,3) stream (108) + the same as three bf16 pieces per value (162 float-sized slots)
CONV64_PACK_FLOATS = 423 * 64 * 64
# what network.py reads from either operator module: storage type of the activations, elements of one 64->64 pack of that type
ACT_DTYPE = torch.float32
PACK_ELEMS = CONV64_PACK_FLOATS


def _ptr(dtype, t, name="tensor", allow_none=False):
    """The device address of a contiguous GPU tensor of exactly `dtype` (None -> NULL where allowed): the one pointer check of both operator
    modules."""
    if t is None:
        if allow_none:
            return None
        raise FdnError("%s is None" % name)
    if not t.is_cuda:
        raise FdnError("%s must live on the GPU; the HIP path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise FdnError("%s must be %s (got %s)" % (name, str(dtype).replace("torch.", ""), t.dtype))
    if not t.is_contiguous():
        raise FdnError("%s must be contiguous" % name)
    return t.data_ptr()


_p = functools.partial(_ptr, torch.float32)
_p64 = functools.partial(_ptr, torch.float64)
_pu8 = functools.partial(_ptr, torch.uint8)              # the is_kernel flags of the flat parameter buffer
_pm = functools.partial(_ptr, torch.int16, name="mask")


def _mask_ptr(mask, nvox, who):
    """A sign mask of nvox voxels (four int16 words each, in the shape the storage type's new_sign_mask gives it), or None -> NULL."""
    if mask is not None and mask.numel() != 4 * nvox:
        raise FdnError("%s: a sign mask of 4 x %d int16 words expected" % (who, nvox))
    return _pm(mask, allow_none=True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# An operator whose two storage types differ only in the type of the activation tensors and the suffix of the library's entry point has
# ONE body here, a private helper both modules' public functions forward to: `entry` names the entry point, act_dtype is the type of the
# activation tensors (parameters, their gradients, the padded dgrad scratch and workspaces are fp32 in both modes).
def _input_features(entry, act_dtype, u, v, w, mu, mv, mw, phase, pc):
    shp = u.shape[:-1] if u.shape[-1] == 1 else u.shape
    if phase is None:
        phase = torch.empty(tuple(shp) + (3,), device=u.device, dtype=act_dtype)
    if pc is None:
        pc = torch.empty(tuple(shp) + (3,), device=u.device, dtype=act_dtype)
    check(getattr(_lib.load(), entry)(_p(u, "u"), _p(v, "v"), _p(w, "w"), _p(mu, "mu"), _p(mv, "mv"), _p(mw, "mw"),
                                      _ptr(act_dtype, phase, "phase"), _ptr(act_dtype, pc, "pc"), u.numel(), _stream()), entry)
    return phase, pc


def input_features(u, v, w, mu, mv, mw, phase=None, pc=None):
    return _input_features("fdn_input_features", ACT_DTYPE, u, v, w, mu, mv, mw, phase, pc)


def _volume_geometry(frames, patch_size, counts, g0, count, who):
    if frames.dim() != 5 or frames.shape[1] != 6:
        raise FdnError("%s: frames must be (F,6,X,Y,Z), got %s" % (who, tuple(frames.shape)))
    F, _, X, Y, Z = frames.shape
    nx, ny, nz = (int(n) for n in counts)
    count = F * nx * ny * nz - int(g0) if count is None else int(count)
    return (F, X, Y, Z, int(patch_size), nx, ny, nz, int(g0), count)


# the geometric self-ensemble's orientations (plane, k): the identity and the nine rotations the loader trains with, in its order
# (data._ROT; plane 1:(0,1), 2:(0,2), 3:(1,2) np.rot90 axes, k quarter turns)
ROT90_ORIENTATIONS = ((0, 0),) + tuple((p, k) for p in (1, 2, 3) for k in (1, 2, 3))


def _orientation(orientation, who):
    """(plane, k) of an `orientation=` argument: None is the identity (0, 0); anything outside ROT90_ORIENTATIONS raises ValueError."""
    if orientation is None:
        return 0, 0
    try:
        plane, k = (operator.index(v) for v in orientation)
    except (TypeError, ValueError):
        plane = k = -1
    if (plane, k) not in ROT90_ORIENTATIONS or any(isinstance(v, bool) for v in orientation):
        raise ValueError("%s: orientation must be (0, 0) or (plane, k) with plane in 1..3 and k in 1..3, got %r" % (who, orientation))
    return plane, k


def self_ensemble_orientations(self_ensemble):
    """The `self_ensemble=` option of the predictor as a tuple of (plane, k) orientations, or None for off (None / False).  "rot90":
    ROT90_ORIENTATIONS, the ten views the network was trained with; a non-empty sequence of unique valid (plane, k) pairs is used as
    given, in its order.  Anything else raises ValueError."""
    if self_ensemble is None or self_ensemble is False:
        return None
    if isinstance(self_ensemble, str):
        if self_ensemble == "rot90":
            return ROT90_ORIENTATIONS
        raise ValueError('self_ensemble: %r is not a known ensemble ("rot90")' % (self_ensemble,))
    try:
        items = list(self_ensemble)
    except TypeError:
        raise ValueError('self_ensemble must be None, False, "rot90" or a sequence of (plane, k) pairs, got %r' % (self_ensemble,)) from None
    if not items:
        raise ValueError("self_ensemble: an empty list of orientations")
    res = tuple(_orientation(() if o is None else o, "self_ensemble") for o in items)
    if len(set(res)) != len(res):
        raise ValueError("self_ensemble: the orientations must be unique, got %r" % (self_ensemble,))
    return res


def _input_features_volume(entry, act_dtype, frames, patch_size, counts, g0, count, phase, pc, orientation=None, stride=None):
    """input_features_volume of either storage type: `entry` names the library's entry point, act_dtype is the type of phase / pc."""
    plane, k = _orientation(orientation, "input_features_volume")
    if stride is not None:
        if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= int(patch_size) - 4:
            raise ValueError("input_features_volume: stride must be an integer in 1..patch_size-4 = %d, got %r" % (int(patch_size) - 4, stride))
    geo = _volume_geometry(frames, patch_size, counts, g0, count, "input_features_volume")
    P, count = geo[4], geo[9]
    if phase is None:
        phase = torch.empty((max(count, 0), P, P, P, 3), device=frames.device, dtype=act_dtype)
    if pc is None:
        pc = torch.empty((max(count, 0), P, P, P, 3), device=frames.device, dtype=act_dtype)
    if min(phase.numel(), pc.numel()) < max(count, 0) * P ** 3 * 3:
        raise FdnError("input_features_volume: phase / pc hold fewer than (%d,%d,%d,%d,3) elements" % (count, P, P, P))
    if stride is not None:                                    # the window of overlapping cores (tiler.PatchGenerator(blend=))
        entry = entry.replace("_volume", "_volume_strided")
        geo = geo + (int(stride), plane, k)
    elif plane:                                               # (0, 0) is the plain entry point
        entry = entry.replace("_volume", "_volume_oriented")
        geo = geo + (plane, k)
    check(getattr(_lib.load(), entry)(_p(frames, "frames"), *geo, _ptr(act_dtype, phase, "phase"), _ptr(act_dtype, pc, "pc"), _stream()), entry)
    return phase, pc


def input_features_volume(frames, patch_size, counts, g0=0, count=None, phase=None, pc=None, stride=None, orientation=None):
    """input_features of patches [g0, g0 + count) of the sliding window over resident frames (F,6,X,Y,Z) (u,v,w,mag_u,mag_v,mag_w,
    normalised): the patches are never materialised.  counts = (nx,ny,nz) of tiler.PatchGenerator.plan; patch g = frame g // (nx*ny*nz),
    then (i,j,k) with k fastest.  Returns (phase, pc), each (count,P,P,P,3).
    orientation=(plane, k): the features of the patches as data.rotate_vector_field turns them (fdn_input_features_volume_oriented).
    stride (None: patch_size - 4): the voxels the window advances by, with counts of PatchGenerator(blend=).plan
    (fdn_input_features_volume_strided); ValueError outside 1..patch_size-4."""
    return _input_features_volume("fdn_input_features_volume", ACT_DTYPE, frames, patch_size, counts, g0, count, phase, pc, orientation,
                                  stride)


def unrotate_accumulate(pred, acc, orientation, first, divisor=1):
    """The self-ensemble's fan-in (fdn_unrotate_accumulate): pred (count,S,S,S,3) fp32, predicted from features of `orientation`, is turned
    back and added to acc of the same shape -- stored, not added, with `first` -- and the sum divided by `divisor` where it exceeds 1
    (the count of orientations, on the last one).  Returns acc."""
    S = _pred_edge(pred, "unrotate_accumulate")
    if tuple(acc.shape) != tuple(pred.shape):
        raise FdnError("unrotate_accumulate: acc must be %s like pred, got %s" % (tuple(pred.shape), tuple(acc.shape)))
    plane, k = _orientation(orientation, "unrotate_accumulate")
    check(_lib.load().fdn_unrotate_accumulate(_p(pred, "pred"), _p(acc, "acc"), pred.shape[0], S, plane, k, int(bool(first)), int(divisor),
                                              _stream()), "fdn_unrotate_accumulate")
    return acc


def kspace_crops(shape, crop_ratio):
    """The crop half-widths of fft_downsampling.rectangular_crop3d, int((N // 2) * crop_ratio) per axis: the output extents are twice these."""
    return tuple(int((int(n) // 2) * crop_ratio) for n in shape)


def kspace_workspace_bytes(nvol, shape, crops):
    X, Y, Z = (int(n) for n in shape)
    cx, cy, cz = (int(c) for c in crops)
    return _lib.load().fdn_kspace_downsample_workspace_bytes(int(nvol), X, Y, Z, cx, cy, cz)


def kspace_downsample(vel, mag, venc, snr_db, crops, noise=None, seed=0, stream_id=0, mag_scale=None, out=None, workspace=None):
    """Low-res synthesis on the device (fdn_kspace_downsample; fft_downsampling.downsample_phase_img): vel (nvol,X,Y,Z) velocity volumes that
    share the magnitude volume mag (X,Y,Z) -> (lr_vel, lr_mag, sigma), the first two (nvol,2cx,2cy,2cz) with crops = (cx,cy,cz) =
    kspace_crops(shape, crop_ratio), sigma (nvol,) the noise level of each volume.  venc, snr_db and mag_scale (default 1: mag is used as
    it is) are scalars or one value per volume; 10**(snr_db/10) is formed in float64 and rounded once.  noise: a device tensor
    (nvol,2cx,2cy,2cz) of standard normals, or None: Philox4x32-10 in the kernel, keyed by (seed, stream_id).  out = (lr_vel, lr_mag)
    and workspace (kspace_workspace_bytes, any fp32 tensor) may be supplied by a caller that repeats the call; nothing here waits for the
    device."""
    if vel.dim() != 4 or mag.dim() != 3 or tuple(vel.shape[1:]) != tuple(mag.shape):
        raise FdnError("kspace_downsample: vel must be (nvol,X,Y,Z) and mag (X,Y,Z), got %s and %s" % (tuple(vel.shape), tuple(mag.shape)))
    nvol, X, Y, Z = (int(n) for n in vel.shape)
    cx, cy, cz = (int(c) for c in crops)
    lr_shape = (nvol, 2 * cx, 2 * cy, 2 * cz)
    per_vol = lambda a, name: _per_volume(a, nvol, "kspace_downsample: " + name)
    table = np.zeros((nvol, 4), np.float64)
    table[:, 0] = per_vol(venc, "venc")
    table[:, 1] = per_vol(1.0 if mag_scale is None else mag_scale, "mag_scale")
    table[:, 2] = 10.0 ** (per_vol(snr_db, "snr_db") / 10.0)
    pv, pm = _p(vel, "vel"), _p(mag, "mag")
    lib = _lib.load()
    need = lib.fdn_kspace_downsample_workspace_bytes(nvol, X, Y, Z, cx, cy, cz)
    if need == 0:
        raise FdnError("kspace_downsample: extents %s (1..1024 each), crops %s (1..N//2 each) or nvol=%d are out of range" % ((X, Y, Z), (cx, cy, cz), nvol))
    if noise is not None and tuple(noise.shape) != lr_shape:
        raise FdnError("kspace_downsample: noise must be %s, got %s" % (lr_shape, tuple(noise.shape)))
    if out is None:
        out = (torch.empty(lr_shape, device=vel.device, dtype=torch.float32), torch.empty(lr_shape, device=vel.device, dtype=torch.float32))
    elif tuple(out[0].shape) != lr_shape or tuple(out[1].shape) != lr_shape:
        raise FdnError("kspace_downsample: out must be two tensors of %s" % (lr_shape,))
    sigma = torch.empty(nvol, device=vel.device, dtype=torch.float32)
    if workspace is None:
        workspace = torch.empty((need + 3) // 4, device=vel.device, dtype=torch.float32)
    elif workspace.numel() * 4 < need:
        raise FdnError("kspace_downsample: workspace of %d bytes expected, got %d" % (need, workspace.numel() * 4))
    params = torch.from_numpy(table.astype(np.float32)).to(vel.device)
    check(lib.fdn_kspace_downsample(pv, pm, _p(params, "params"), nvol, X, Y, Z, cx, cy, cz, _p(noise, "noise", allow_none=True),
                                    int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1), _p(out[0], "out[0]"), _p(out[1], "out[1]"),
                                    _p(sigma, "sigma"), _p(workspace, "workspace"), _stream()), "fdn_kspace_downsample")
    return out[0], out[1], sigma


def _per_volume(a, nvol, name):
    a = np.asarray(a, np.float64).reshape(-1)
    if a.size not in (1, nvol):
        raise FdnError("%s must be a scalar or one value per volume (%d), got %d" % (name, nvol, a.size))
    return np.broadcast_to(a, (nvol,))


def _pred_edge(pred, who):
    if pred.dim() != 5 or pred.shape[4] != 3 or not (pred.shape[1] == pred.shape[2] == pred.shape[3]):
        raise FdnError("%s: pred must be (count,S,S,S,3), got %s" % (who, tuple(pred.shape)))
    return pred.shape[1]


def stitch_patches(pred, vol, side, counts, g0=0, frame_scale=None):
    """Cores of the predicted patches [g0, g0 + len(pred)) into the stitched volumes: pred (count,S,S,S,3), vol (F,3,Xo,Yo,Zo), side =
    2 * res_increase HR voxels stripped per patch side; core voxels that fall into the cropped far pad are dropped (tiler.PatchGenerator.
    _patchup_with_overlap per frame and component).  Writes of different patches are disjoint: any batching gives the same volume.
    frame_scale (a float64 device tensor (F,2) of {venc, threshold} per frame): vol is float64 and every value is finished on the way,
    p * venc with +0.0 where the magnitude is below the threshold (predictor.py:103-107; fdn_stitch_patches_finish)."""
    S = _pred_edge(pred, "stitch_patches")
    if vol.dim() != 5 or vol.shape[1] != 3:
        raise FdnError("stitch_patches: vol must be (F,3,Xo,Yo,Zo), got %s" % (tuple(vol.shape),))
    F, _, Xo, Yo, Zo = vol.shape
    nx, ny, nz = (int(n) for n in counts)
    if frame_scale is None:
        check(_lib.load().fdn_stitch_patches(_p(pred, "pred"), _p(vol, "vol"), F, Xo, Yo, Zo, S, int(side), nx, ny, nz,
                                             int(g0), pred.shape[0], _stream()), "fdn_stitch_patches")
        return vol
    if vol.dtype != torch.float64:
        raise FdnError("stitch_patches: vol must be float64 with frame_scale (got %s)" % vol.dtype)
    if tuple(frame_scale.shape) != (F, 2):
        raise FdnError("stitch_patches: frame_scale must be (F,2) = (%d,2), got %s" % (F, tuple(frame_scale.shape)))
    check(_lib.load().fdn_stitch_patches_finish(_p(pred, "pred"), _p64(vol, "vol (with frame_scale)"), _p64(frame_scale, "frame_scale"),
                                                F, Xo, Yo, Zo, S, int(side), nx, ny, nz, int(g0), pred.shape[0], _stream()),
          "fdn_stitch_patches_finish")
    return vol


def blend_patches(pred, acc, side, stride_hr, counts, g0=0):
    """Overlap-add stitching (fdn_blend_patches): the cores of the predicted patches [g0, g0 + len(pred)) -- pred (count,S,S,S,3), core =
    S - 2*side, advancing by stride_hr HR voxels -- are added with their linear-ramp weights into acc (F,3,Xo,Yo,Zo) fp32, which the
    caller zeroes once per volume.  acc = acc + fl(w * p) per covering patch in ascending g: calls in ascending g0 give the same bits
    however the patch list is cut.  side = 0: cores packed by pack_patch_cores.  Returns acc."""
    S = _pred_edge(pred, "blend_patches")
    if acc.dim() != 5 or acc.shape[1] != 3:
        raise FdnError("blend_patches: acc must be (F,3,Xo,Yo,Zo), got %s" % (tuple(acc.shape),))
    F, _, Xo, Yo, Zo = acc.shape
    nx, ny, nz = (int(n) for n in counts)
    check(_lib.load().fdn_blend_patches(_p(pred, "pred"), _p(acc, "acc"), F, Xo, Yo, Zo, S, int(side), int(stride_hr), nx, ny, nz, int(g0),
                                        pred.shape[0], _stream()), "fdn_blend_patches")
    return acc


def finish_volume(acc, frame_scale, out=None):
    """The predictor's post-processing on an accumulated volume (fdn_finish_volume): acc (F,3,Xo,Yo,Zo) fp32 -> float64 of the same shape,
    acc * venc with +0.0 where the magnitude is below the threshold; frame_scale a float64 device tensor (F,2) of {venc, threshold} per
    frame (the rule of stitch_patches(frame_scale=))."""
    if acc.dim() != 5 or acc.shape[1] != 3:
        raise FdnError("finish_volume: acc must be (F,3,Xo,Yo,Zo), got %s" % (tuple(acc.shape),))
    F, _, Xo, Yo, Zo = acc.shape
    if tuple(frame_scale.shape) != (F, 2):
        raise FdnError("finish_volume: frame_scale must be (F,2) = (%d,2), got %s" % (F, tuple(frame_scale.shape)))
    if out is None:
        out = torch.empty(tuple(acc.shape), device=acc.device, dtype=torch.float64)
    elif tuple(out.shape) != tuple(acc.shape):
        raise FdnError("finish_volume: out must be %s, got %s" % (tuple(acc.shape), tuple(out.shape)))
    check(_lib.load().fdn_finish_volume(_p(acc, "acc"), _p64(out, "out"), _p64(frame_scale, "frame_scale"), F, Xo, Yo, Zo, _stream()),
          "fdn_finish_volume")
    return out


def pack_patch_cores(pred, side, out=None):
    """The cores of predicted patches, contiguous: pred (count,S,S,S,3) -> (count,c,c,c,3), c = S - 2*side (fdn_pack_patch_cores).
    stitch_patches(pack_patch_cores(pred, side), vol, 0, ...) equals stitch_patches(pred, vol, side, ...)."""
    S = _pred_edge(pred, "pack_patch_cores")
    side = int(side)
    c = S - 2 * side
    if side < 0 or c <= 0:
        raise FdnError("pack_patch_cores: S=%d must exceed 2*side (side=%d)" % (S, side))
    shape = (pred.shape[0], c, c, c, 3)
    if out is None:
        out = torch.empty(shape, device=pred.device, dtype=torch.float32)
    elif tuple(out.shape) != shape:
        raise FdnError("pack_patch_cores: out must be %s, got %s" % (shape, tuple(out.shape)))
    check(_lib.load().fdn_pack_patch_cores(_p(pred, "pred"), _p(out, "out"), S, side, pred.shape[0], _stream()), "fdn_pack_patch_cores")
    return out


def _pack_conv64_weights(entry, act_dtype, elems, w, wp_fwd, wp_dgrad, want_dgrad):
    """pack_conv64_weights of either storage type: a pack holds `elems` elements of act_dtype."""
    if tuple(w.shape) != (3, 3, 3, 64, 64):
        raise FdnError("pack_conv64_weights: expected (3,3,3,64,64), got %s" % (tuple(w.shape),))
    if wp_fwd is None:
        wp_fwd = torch.empty(elems, device=w.device, dtype=act_dtype)
    if wp_dgrad is None and want_dgrad:
        wp_dgrad = torch.empty(elems, device=w.device, dtype=act_dtype)
    check(getattr(_lib.load(), entry)(_p(w, "w"), _ptr(act_dtype, wp_fwd, "wp_fwd"), _ptr(act_dtype, wp_dgrad, "wp_dgrad", allow_none=True),
                                      _stream()), entry)
    return wp_fwd, wp_dgrad


def pack_conv64_weights(w, wp_fwd=None, wp_dgrad=None, want_dgrad=True):
    return _pack_conv64_weights("fdn_pack_conv64_weights", ACT_DTYPE, PACK_ELEMS, w, wp_fwd, wp_dgrad, want_dgrad)


def conv64_mask_ok(N, D, H, W, algo=ALGO_AUTO):
    """True when the 64->64 forward and fused dgrad of an (N,D,H,W) grid can write / read sign masks (fdn_conv64_mask_ok)."""
    r = _lib.load().fdn_conv64_mask_ok(int(N), int(D), int(H), int(W), int(algo))
    check(min(r, 0), "fdn_conv64_mask_ok")
    return r == 1


def new_sign_mask(y):
    """Sign-mask buffer of an fp32 (N,D,H,W,64) tensor: four planes [cout / 16][voxel] of int16 words (include/fdn.h)."""
    return torch.empty((4, y.shape[0] * y.shape[1] * y.shape[2] * y.shape[3]), device=y.device, dtype=torch.int16)


def conv3d_fwd(x, w, bias=None, act=ACT_NONE, alpha=LEAKY_ALPHA, residual=None, x2=None, wpack=None, out=None,
               ldy=None, y_coff=0, algo=ALGO_AUTO, mask=None):
    """x (N,D,H,W,Cin[/2 if x2]); w Keras layout (K,K,K,Cin,Cout).
    mask (64->64 only, new_sign_mask(out), where conv64_mask_ok): also receives the sign mask of the output."""
    N, D, H, W = x.shape[:4]
    K, Cin, Cout = w.shape[0], w.shape[3], w.shape[4]
    if mask is not None:
        if (K, Cin, Cout) != (3, 64, 64) or x2 is not None or (ldy not in (None, 64)) or y_coff != 0:
            raise FdnError("conv3d_fwd: a sign mask belongs to a dense 64->64 3x3x3 layer")
        if out is None:
            out = torch.empty((N, D, H, W, 64), device=x.device, dtype=torch.float32)
        if wpack is None:
            wpack, _ = pack_conv64_weights(w, want_dgrad=False)
        check(_lib.load().fdn_conv64_fwd_mask(_p(x, "x"), _p(wpack, "wpack"), _p(bias, allow_none=True), _p(residual, allow_none=True),
                                              _p(out, "out"), _mask_ptr(mask, N * D * H * W, "conv3d_fwd"), N, D, H, W, act, float(alpha), int(algo),
                                              _stream()), "fdn_conv64_fwd_mask")
        return out
    if out is None:
        out = torch.empty((N, D, H, W, Cout), device=x.device, dtype=torch.float32)
        ldy = Cout
    elif ldy is None:
        ldy = out.shape[-1]
    if Cin == 64 and Cout == 64 and K == 3 and wpack is None:
        wpack, _ = pack_conv64_weights(w, want_dgrad=False)
    check(_lib.load().fdn_conv3d_fwd(_p(x, "x"), _p(x2, allow_none=True), _p(w, "w"), _p(wpack, allow_none=True),
                                     _p(bias, allow_none=True), _p(residual, allow_none=True), _p(out, "out"),
                                     N, D, H, W, Cin, Cout, K, ldy, y_coff, act, float(alpha), int(algo), _stream()),
          "fdn_conv3d_fwd")
    return out


def conv3d_dgrad(dz, w, wpack_dgrad=None, out=None, lddz=None, dz_coff=0, spatial=None, algo=ALGO_AUTO):
    """Returns the gradient on the PADDED input grid (N,D+2,H+2,W+2,Cin) for K=3."""
    K, Cin, Cout = w.shape[0], w.shape[3], w.shape[4]
    N, D, H, W = dz.shape[:4] if spatial is None else spatial
    if lddz is None:
        lddz = dz.shape[-1]
    if out is None:
        out = torch.empty((N, D + 2, H + 2, W + 2, Cin), device=dz.device, dtype=torch.float32)
    if Cin == 64 and Cout == 64 and K == 3 and wpack_dgrad is None:
        _, wpack_dgrad = pack_conv64_weights(w)
    check(_lib.load().fdn_conv3d_dgrad(_p(dz, "dz"), _p(w, "w"), _p(wpack_dgrad, allow_none=True), _p(out, "dxpad"),
                                       N, D, H, W, Cin, Cout, K, lddz, dz_coff, int(algo), _stream()), "fdn_conv3d_dgrad")
    return out


def _conv_cout1_dgrad_folded(entry, act_dtype, src, dz, w, spatial, act, alpha, lddz, dz_coff, out, dbias_prev, workspace):
    """conv_cout1_dgrad_folded of either storage type (dz is the fp32 prediction gradient in both).  src: the checked pointers the entry
    point reads act' from -- y_prev, or its sign mask, or both."""
    N, D, H, W = spatial
    if out is None:
        out = torch.empty((N, D, H, W, 64), device=dz.device, dtype=act_dtype)
    if dbias_prev is not None and workspace is None:
        workspace = torch.empty(2048 * 64, device=dz.device, dtype=torch.float32)
    wsb = 0 if workspace is None else workspace.numel() * workspace.element_size()
    check(getattr(_lib.load(), entry)(_p(dz, "dz"), _p(w, "w"), *src, act, float(alpha), _ptr(act_dtype, out, "out"),
                                      _p(dbias_prev, "dbias_prev", allow_none=True), _p(workspace, "workspace", allow_none=True), wsb,
                                      N, D, H, W, lddz, dz_coff, _stream()), entry)
    return out


def conv_cout1_dgrad_folded(dz, w, spatial, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, lddz=1, dz_coff=0, out=None,
                            dbias_prev=None, workspace=None, mask=None):
    """64->1 head dgrad + halo fold + act'(y_prev) in one kernel.  Returns (N,D,H,W,64).  With dbias_prev (64 floats) it
    also emits the producing layer's bias gradient (sum of the result over voxels); needs a >= 512 KB workspace.
    mask: the sign mask conv3d_fwd(mask=...) wrote beside y_prev (W % 4 == 0), read instead of y_prev's rows."""
    if mask is not None:
        entry, src = "fdn_conv_cout1_dgrad_folded_mask", (_mask_ptr(mask, math.prod(spatial), "conv_cout1_dgrad_folded"),)
    else:
        entry, src = "fdn_conv_cout1_dgrad_folded", (_p(y_prev, "y_prev", allow_none=True),)
    return _conv_cout1_dgrad_folded(entry, ACT_DTYPE, src, dz, w, spatial, act, alpha, lddz, dz_coff, out, dbias_prev, workspace)


def fold_halo(dxpads, skip=None, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, out=None):
    """dxpads: 1..3 tensors (N,D+2,H+2,W+2,C).  Returns (N,D,H,W,C)."""
    p0 = dxpads[0]
    N, D, H, W, C = p0.shape[0], p0.shape[1] - 2, p0.shape[2] - 2, p0.shape[3] - 2, p0.shape[4]
    if out is None:
        out = torch.empty((N, D, H, W, C), device=p0.device, dtype=torch.float32)
    ptrs = [_p(t) for t in dxpads] + [None] * (3 - len(dxpads))
    check(_lib.load().fdn_fold_halo(ptrs[0], ptrs[1], ptrs[2], len(dxpads), _p(skip, allow_none=True),
                                    _p(y_prev, allow_none=True), act, float(alpha), _p(out), N, D, H, W, C, _stream()),
          "fdn_fold_halo")
    return out


DGRAD_INNER, DGRAD_SHELL = 1, 2


def conv3d_dgrad_fused(dz, wpack_dgrad, dxpad, out, skip=None, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, parts=3,
                       algo=ALGO_AUTO, mask=None):
    """64->64 dgrad; interior voxels of `out` are finished in the conv epilogue (skip may alias out), the rest lands
    in the padded scratch `dxpad` for fold_halo_border.  parts: DGRAD_INNER | DGRAD_SHELL -- the two pieces write disjoint
    positions and may run on different streams.  mask: the sign mask the forward wrote beside y_prev (conv3d_fwd(mask=...)), read
    instead of y_prev for act' (the one-launch form only)."""
    N, D, H, W = dz.shape[:4]
    if mask is not None:
        if parts != 3:
            raise FdnError("conv3d_dgrad_fused: a sign mask needs the one-launch form")
        check(_lib.load().fdn_conv64_dgrad_fused_mask(_p(dz, "dz"), _p(wpack_dgrad, "wpack"), _p(dxpad, "dxpad"), _p(skip, allow_none=True),
                                                      _mask_ptr(mask, N * D * H * W, "conv3d_dgrad_fused"), act, float(alpha), _p(out, "out"),
                                                      N, D, H, W, int(algo), _stream()), "fdn_conv64_dgrad_fused_mask")
        return out
    if parts == 3:
        check(_lib.load().fdn_conv3d_dgrad_fused(_p(dz, "dz"), _p(wpack_dgrad, "wpack"), _p(dxpad, "dxpad"),
                                                 _p(skip, allow_none=True), _p(y_prev, allow_none=True), act, float(alpha),
                                                 _p(out, "out"), N, D, H, W, int(algo), _stream()), "fdn_conv3d_dgrad_fused")
    else:
        check(_lib.load().fdn_conv3d_dgrad_fused_part(_p(dz, "dz"), _p(wpack_dgrad, "wpack"), _p(dxpad, "dxpad"),
                                                      _p(skip, allow_none=True), _p(y_prev, allow_none=True), act, float(alpha),
                                                      _p(out, "out"), N, D, H, W, int(parts), int(algo), _stream()),
              "fdn_conv3d_dgrad_fused_part")
    return out


def _dgrad_fused_multi(entry, pa, dzs, wpacks_dgrad, dxpad, out, skip, y_prev, act, alpha, mask, *algo):
    """conv3d_dgrad_fused_multi of either storage type: `entry` names the library's entry point, pa checks an activation pointer, algo is
    (algo,) where the entry point takes one."""
    n = len(dzs)
    N, D, H, W = dzs[0].shape[:4]
    if not 1 <= n <= 3 or len(wpacks_dgrad) != n or any(tuple(t.shape) != tuple(dzs[0].shape) for t in dzs):
        raise FdnError("conv3d_dgrad_fused_multi: 1..3 sources of one shape, one pack each")
    tz = (ctypes.c_void_p * n)(*[pa(t, "dz") for t in dzs])
    tw = (ctypes.c_void_p * n)(*[pa(t, "wpack") for t in wpacks_dgrad])
    check(getattr(_lib.load(), entry)(tz, tw, n, _p(dxpad, "dxpad"), pa(skip, allow_none=True), pa(y_prev, allow_none=True),
                                      _mask_ptr(mask, N * D * H * W, "conv3d_dgrad_fused_multi"), act, float(alpha), pa(out, "out"),
                                      N, D, H, W, *algo, _stream()), entry)
    return out


def conv3d_dgrad_fused_multi(dzs, wpacks_dgrad, dxpad, out, skip=None, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, algo=ALGO_AUTO, mask=None):
    """The fused dgrad of 1..3 64->64 layers that share their input, as ONE launch: out / dxpad receive what chained conv3d_dgrad_fused
    calls (skip = the running sum) would leave, to fp32 rounding -- the sum over the sources is formed in the kernel's registers.  Only
    where conv64_mask_ok(N, D, H, W, algo); the packs must be views of one pack buffer.  y_prev or mask (its sign mask) or neither."""
    if mask is not None and y_prev is not None:
        raise FdnError("conv3d_dgrad_fused_multi: y_prev OR its sign mask")
    return _dgrad_fused_multi("fdn_conv64_dgrad_fused_multi", _p, dzs, wpacks_dgrad, dxpad, out, skip, y_prev, act, alpha, mask, int(algo))


def conv64_dgrad_multi_ok(algos):
    """May 64->64 layers with these algorithms go out as one conv3d_dgrad_fused_multi launch (on a grid where conv64_mask_ok)?  fp32: the
    launch has one algorithm."""
    return len(set(algos)) == 1


def _fold_halo_border(entry, pa, dxpads, out, skip, y_prev, act, alpha):
    """fold_halo_border of either storage type: pa checks an activation pointer (the padded scratches are fp32 in both)."""
    N, D, H, W = out.shape[:4]
    ptrs = [_p(t, "dxpad") for t in dxpads] + [None] * (3 - len(dxpads))
    check(getattr(_lib.load(), entry)(ptrs[0], ptrs[1], ptrs[2], len(dxpads), pa(skip, "skip", allow_none=True),
                                      pa(y_prev, "y_prev", allow_none=True), act, float(alpha), pa(out, "out"), N, D, H, W, _stream()), entry)
    return out


def fold_halo_border(dxpads, out, skip=None, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA):
    return _fold_halo_border("fdn_fold_halo_border", _p, dxpads, out, skip, y_prev, act, alpha)


def _conv1x1_dgrad(entry, pa, dz, w, ya, yb, dxa, dxb):
    nvox = dz.numel() // 64
    if dxa is None:
        dxa = torch.empty_like(ya)
    if dxb is None:
        dxb = torch.empty_like(yb)
    check(getattr(_lib.load(), entry)(pa(dz, "dz"), _p(w, "w"), pa(ya, "ya"), pa(yb, "yb"), pa(dxa, "dxa"), pa(dxb, "dxb"), nvox, _stream()),
          entry)
    return dxa, dxb


def conv1x1_dgrad(dz, w, ya, yb, dxa=None, dxb=None):
    return _conv1x1_dgrad("fdn_conv1x1_dgrad", _p, dz, w, ya, yb, dxa, dxb)


def wgrad_workspace_bytes(N, D, H, W, Cin, Cout, K):
    return int(_lib.load().fdn_conv3d_wgrad_workspace_bytes(N, D, H, W, Cin, Cout, K))


def _conv3d_wgrad(entry, act_dtype, need, x, dz, K, Cin, Cout, x2, want_bias, dw, dbias, workspace, lddz, dz_coff, *algo):
    """conv3d_wgrad of either storage type: need is wgrad_workspace_bytes of the module, algo is (algo,) where the entry point takes one.
    x (and x2) are act_dtype; so is dz, except for Cout == 1, where it is the fp32 prediction gradient; dw / dbias are fp32."""
    N, D, H, W = x.shape[:4]
    if lddz is None:
        lddz = dz.shape[-1]
    if dw is None:
        dw = torch.empty((K, K, K, Cin, Cout), device=x.device, dtype=torch.float32)
    if want_bias and dbias is None:
        dbias = torch.empty((Cout,), device=x.device, dtype=torch.float32)
    nbytes = need(N, D, H, W, Cin, Cout, K)
    if workspace is None:
        workspace = torch.empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32)
    check(getattr(_lib.load(), entry)(_ptr(act_dtype, x, "x"), _ptr(act_dtype, x2, "x2", allow_none=True),
                                      _ptr(torch.float32 if Cout == 1 else act_dtype, dz, "dz"), _p(dw, "dw"),
                                      _p(dbias, "dbias", allow_none=True), _p(workspace, "workspace"),
                                      workspace.numel() * workspace.element_size(), N, D, H, W, Cin, Cout, K, lddz, dz_coff, *algo,
                                      _stream()), entry)
    return dw, dbias


def conv3d_wgrad(x, dz, K, Cin, Cout, x2=None, want_bias=False, dw=None, dbias=None, workspace=None, lddz=None,
                 dz_coff=0, algo=ALGO_AUTO):
    return _conv3d_wgrad("fdn_conv3d_wgrad", ACT_DTYPE, wgrad_workspace_bytes, x, dz, K, Cin, Cout, x2, want_bias, dw, dbias, workspace,
                         lddz, dz_coff, int(algo))


def wgrad_batch_workspace_bytes(n_layers, N, D, H, W):
    return int(_lib.load().fdn_conv3d_wgrad_batch_workspace_bytes(n_layers, N, D, H, W))


def _wgrad_batch(entry, pa, need, xs, dzs, dws, dbiases, workspace, *algo):
    """conv3d_wgrad_batch of either storage type: `entry` names the library's entry point, pa checks an activation pointer, need is
    wgrad_batch_workspace_bytes of the module, algo is (algo,) where the entry point takes one."""
    n = len(xs)
    if not (n and len(dzs) == n and len(dws) == n and (dbiases is None or len(dbiases) == n)):
        raise ValueError("conv3d_wgrad_batch: xs, dzs, dws (and dbiases) must be lists of one length")
    N, D, H, W = xs[0].shape[:4]
    for x, dz in zip(xs, dzs):
        if tuple(x.shape) != (N, D, H, W, 64) or tuple(dz.shape) != (N, D, H, W, 64):
            raise ValueError("conv3d_wgrad_batch: every layer must have the grid %s with 64 channels" % ((N, D, H, W),))
    nbytes = need(n, N, D, H, W)
    if workspace is None:
        workspace = torch.empty((nbytes + 3) // 4, device=xs[0].device, dtype=torch.float32)
    table = lambda ptr, ts, name, **kw: (ctypes.c_void_p * n)(*[ptr(t, name, **kw) for t in ts])
    tx, tz, tw = table(pa, xs, "x"), table(pa, dzs, "dz"), table(_p, dws, "dw")
    tb = table(_p, dbiases, "dbias", allow_none=True) if dbiases is not None and any(b is not None for b in dbiases) else None
    check(getattr(_lib.load(), entry)(tx, tz, tw, tb, n, _p(workspace, "workspace"), workspace.numel() * workspace.element_size(),
                                      N, D, H, W, *algo, _stream()), entry)
    return dws


def conv3d_wgrad_batch(xs, dzs, dws, dbiases=None, workspace=None, algo=ALGO_AUTO):
    """Weight gradients of several 64->64 3x3x3 layers that share one grid in ONE launch (fdn_conv3d_wgrad_batch): xs / dzs / dws are
    lists of tensors (N,D,H,W,64) / (N,D,H,W,64) / (3,3,3,64,64); dbiases: None or a list with None / (64,) entries."""
    return _wgrad_batch("fdn_conv3d_wgrad_batch", _p, wgrad_batch_workspace_bytes, xs, dzs, dws, dbiases, workspace, int(algo))


def conv64_wgrad_batch_ok(algo=ALGO_AUTO):
    """May the weight gradient of a 64->64 layer with this algorithm join a conv3d_wgrad_batch launch?  fp32: the Winograd kernels' batch."""
    return algo in (ALGO_AUTO, ALGO_WINO_H2, ALGO_WINO_BF16X3)


def _upsample_trilinear_fwd(entry, act_dtype, x, R, out):
    N, D, H, W, C = x.shape
    if out is None:
        out = torch.empty((N, D * R, H * R, W * R, C), device=x.device, dtype=act_dtype)
    check(getattr(_lib.load(), entry)(_ptr(act_dtype, x, "x"), _ptr(act_dtype, out, "out"), N, D, H, W, C, R, _stream()), entry)
    return out


def upsample_trilinear_fwd(x, R, out=None):
    return _upsample_trilinear_fwd("fdn_upsample_trilinear_fwd", ACT_DTYPE, x, R, out)


def _upsample_trilinear_bwd(entry, act_dtype, dy, R, y_prev, act, alpha, out):
    N, OD, OH, OW, C = dy.shape
    D, H, W = OD // R, OH // R, OW // R
    if out is None:
        out = torch.empty((N, D, H, W, C), device=dy.device, dtype=act_dtype)
    check(getattr(_lib.load(), entry)(_ptr(act_dtype, dy, "dy"), _ptr(act_dtype, y_prev, "y_prev", allow_none=True), act, float(alpha),
                                      _ptr(act_dtype, out, "out"), N, D, H, W, C, R, _stream()), entry)
    return out


def upsample_trilinear_bwd(dy, R, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, out=None):
    return _upsample_trilinear_bwd("fdn_upsample_trilinear_bwd", ACT_DTYPE, dy, R, y_prev, act, alpha, out)


LOSS_KINDS = {'mse': 0, 'mae': 1, 'huber': 2, 'charbonnier': 3}       # FDN_LOSS_MSE .. FDN_LOSS_CHARBONNIER
LOSS_PARAM_DEFAULTS = {'huber': 1.0, 'charbonnier': 1e-3}             # delta (tf.keras.losses.Huber's default), epsilon


def checked_loss_kind(kind, kind_param, who="loss_metrics", error=None):
    """(name, FDN_LOSS_* code, parameter as the float the entry point takes) of a penalty of the data term, validated without a tensor.
    'mse' and 'mae' take no parameter (None or 0); 'huber' takes delta and 'charbonnier' epsilon, finite and > 0 also once rounded to
    fp32, None = the default (1.0 / 1e-3)."""
    error = error or FdnError
    if not isinstance(kind, str) or kind not in LOSS_KINDS:
        raise error("%s: the loss must be one of %s, got %r" % (who, ", ".join(repr(k) for k in LOSS_KINDS), kind))
    if kind not in LOSS_PARAM_DEFAULTS:
        if kind_param is not None and not (isinstance(kind_param, numbers.Real) and not isinstance(kind_param, bool) and kind_param == 0):
            raise error("%s: the %r loss takes no parameter, got %r" % (who, kind, kind_param))
        return kind, LOSS_KINDS[kind], 0.0
    what = "delta" if kind == 'huber' else "epsilon"
    if kind_param is None:
        kind_param = LOSS_PARAM_DEFAULTS[kind]
    try:
        pf = float(kind_param)
        if isinstance(kind_param, bool):
            raise TypeError
        p32 = struct.unpack("f", struct.pack("f", pf))[0] if math.isfinite(pf) else pf
    except (TypeError, ValueError, OverflowError):
        raise error("%s: %s of the %r loss must be a finite number > 0, got %r" % (who, what, kind, kind_param)) from None
    if not (math.isfinite(p32) and p32 > 0):
        raise error("%s: %s of the %r loss must be a finite number > 0 (in fp32), got %r" % (who, what, kind, kind_param))
    return kind, LOSS_KINDS[kind], pf


def loss_metrics(pred, uh, vh, wh, mask, want_grad=True, out=None, dpred=None, scratch=None, div_weight=0.0, non_fluid_weight=1.0,
                 out_act=ACT_NONE, kind='mse', kind_param=None):
    """Returns out (N,4) = [mse-loss, rel-err %, sum mask, sum nonfluid] and dpred (N,...,3) or None.
    div_weight != 0 (pred (N,D,H,W,3)): fdn_loss_metrics_div, out (N,5) with the weighted divergence loss div_b in column 4 and its
    gradient in dpred (the sample's loss is out[:, 0] + out[:, 4]).  div_weight == 0 is exactly the plain call.
    non_fluid_weight != 1 or out_act == ACT_TANH (pred (N,D,H,W,3)): fdn_loss_metrics_act, out (N,5): the non-fluid part of the MSE and of
    the divergence term weighted, and dpred the gradient w.r.t. the heads' PRE-activations (times 1 - pred^2 under ACT_TANH) -- what
    FlowNetModel.backward takes.  At the defaults the calls are exactly the ones above.
    kind: the penalty rho of the data term, summed over the three components of the residual d = pred - truth: 'mse' d^2 (the reference's
    calculate_mse; the calls above, untouched), 'mae' |d|, 'huber' d^2 / 2 up to |d| = kind_param = delta and delta (|d| - delta / 2)
    beyond (default 1.0; on velocities normalised to [-1, 1] that is MSE / 2 almost everywhere, so choose a smaller delta),
    'charbonnier' sqrt(d^2 + eps^2), kind_param = eps (default 1e-3).  Other than 'mse' (pred (N,D,H,W,3)): fdn_loss_metrics_kind, out
    (N,5) with the data term in column 0; the divergence term stays squared, the metric and the counts do not depend on the kind."""
    kind, kind_code, kind_param = checked_loss_kind(kind, kind_param)
    non_fluid_weight = float(non_fluid_weight)
    if not (math.isfinite(non_fluid_weight) and non_fluid_weight >= 0):
        raise FdnError("loss_metrics: non_fluid_weight must be a finite number >= 0, got %r" % (non_fluid_weight,))
    if out_act not in (ACT_NONE, ACT_TANH):
        raise FdnError("loss_metrics: out_act must be ACT_NONE or ACT_TANH, got %r" % (out_act,))
    if kind != 'mse':
        return _loss_metrics_div(pred, uh, vh, wh, mask, float(div_weight), want_grad, out, dpred, scratch, non_fluid_weight, out_act,
                                 (kind_code, kind_param))
    if non_fluid_weight != 1.0 or out_act != ACT_NONE:
        return _loss_metrics_div(pred, uh, vh, wh, mask, float(div_weight), want_grad, out, dpred, scratch, non_fluid_weight, out_act)
    N = pred.shape[0]
    if div_weight != 0:
        return _loss_metrics_div(pred, uh, vh, wh, mask, float(div_weight), want_grad, out, dpred, scratch)
    V = pred.numel() // (3 * N)
    if out is None:
        out = torch.empty((N, 4), device=pred.device, dtype=torch.float32)
    if scratch is None:
        scratch = torch.empty((N * (8 + 3 * 256),), device=pred.device, dtype=torch.float32)     # FDN_LOSS_SCRATCH_FLOATS(N)
    if want_grad and dpred is None:
        dpred = torch.empty_like(pred)
    check(_lib.load().fdn_loss_metrics(_p(pred), _p(uh), _p(vh), _p(wh), _p(mask), _p(out),
                                       _p(dpred, allow_none=True) if want_grad else None, _p(scratch), N, V, _stream()),
          "fdn_loss_metrics")
    return out, (dpred if want_grad else None)


def _loss_metrics_div(pred, uh, vh, wh, mask, div_weight, want_grad, out, dpred, scratch, non_fluid_weight=None, out_act=ACT_NONE, kind=None):
    """fdn_loss_metrics_div, (non_fluid_weight given) fdn_loss_metrics_act or (kind = (code, parameter) given too) fdn_loss_metrics_kind:
    same operands, same buffers."""
    if pred.dim() != 5 or pred.shape[-1] != 3:
        raise FdnError("loss_metrics: the divergence term needs pred of shape (N,D,H,W,3), got %s" % (tuple(pred.shape),))
    N, D, H, W = pred.shape[:4]
    V = D * H * W
    for name, t in (("uh", uh), ("vh", vh), ("wh", wh), ("mask", mask)):
        if t.numel() != N * V:
            raise FdnError("loss_metrics: %s holds %d values, pred's grid %d" % (name, t.numel(), N * V))
    if out is None:
        out = torch.empty((N, 5), device=pred.device, dtype=torch.float32)
    if scratch is None:
        scratch = torch.empty((N * (8 + 5 * 256),), device=pred.device, dtype=torch.float32)     # FDN_LOSS_DIV_SCRATCH_FLOATS(N)
    if want_grad and dpred is None:
        dpred = torch.empty_like(pred)
    if out.numel() < N * 5 or scratch.numel() < N * (8 + 5 * 256) or (want_grad and dpred.numel() != pred.numel()):
        raise FdnError("loss_metrics: out needs (N,5), scratch N*(8 + 5*256) floats and dpred pred's shape")
    if kind is not None:
        check(_lib.load().fdn_loss_metrics_kind(_p(pred), _p(uh), _p(vh), _p(wh), _p(mask), kind[0], kind[1], div_weight, non_fluid_weight,
                                                int(out_act), _p(out), _p(dpred, allow_none=True) if want_grad else None, _p(scratch),
                                                N, D, H, W, _stream()),
              "fdn_loss_metrics_kind")
        return out, (dpred if want_grad else None)
    if non_fluid_weight is not None:
        check(_lib.load().fdn_loss_metrics_act(_p(pred), _p(uh), _p(vh), _p(wh), _p(mask), div_weight, non_fluid_weight, int(out_act), _p(out),
                                               _p(dpred, allow_none=True) if want_grad else None, _p(scratch), N, D, H, W, _stream()),
              "fdn_loss_metrics_act")
        return out, (dpred if want_grad else None)
    check(_lib.load().fdn_loss_metrics_div(_p(pred), _p(uh), _p(vh), _p(wh), _p(mask), div_weight, _p(out),
                                           _p(dpred, allow_none=True) if want_grad else None, _p(scratch), N, D, H, W, _stream()),
          "fdn_loss_metrics_div")
    return out, (dpred if want_grad else None)


VOLUME_METRICS_COLUMNS = 26           # FDN_VOLUME_METRICS_COLUMNS
_volume_metrics_scratch = {}          # device -> float64 buffer of per-block partials, grown on demand


def volume_metrics_scratch_doubles(F):
    """FDN_VOLUME_METRICS_SCRATCH_DOUBLES(F)."""
    return F * VOLUME_METRICS_COLUMNS * 256


def volume_metrics(pred, truth, mask, out=None, scratch=None):
    """The 26 sums per frame of a stitched prediction against the high-resolution truth (fdn_volume_metrics; the columns are
    predictor.VOLUME_SUM_NAMES, predictor.metrics_from_sums turns them into metrics).  pred (F,3,X,Y,Z) fp32 or float64 -- what
    predict_volume returns --, truth (F,3,X,Y,Z) fp32 in the same units, mask (1,X,Y,Z) or (F,X,Y,Z) fp32.  Returns out, the (F,26)
    float64 device tensor.  The per-block partials live in one buffer per device kept on this module (calls on one device are ordered
    by its stream); scratch= (float64, volume_metrics_scratch_doubles(F) elements) replaces it."""
    if pred.dim() != 5 or pred.shape[1] != 3:
        raise FdnError("volume_metrics: pred must be (F,3,X,Y,Z), got %s" % (tuple(pred.shape),))
    if pred.dtype not in (torch.float32, torch.float64):
        raise FdnError("volume_metrics: pred must be float32 or float64 (got %s)" % pred.dtype)
    F, _, X, Y, Z = pred.shape
    if tuple(truth.shape) != tuple(pred.shape):
        raise FdnError("volume_metrics: truth must be %s like pred, got %s" % (tuple(pred.shape), tuple(truth.shape)))
    if mask.dim() != 4 or tuple(mask.shape[1:]) != (X, Y, Z) or mask.shape[0] not in (1, F):
        raise FdnError("volume_metrics: mask must be (1,%d,%d,%d) or (%d,%d,%d,%d), got %s" % (X, Y, Z, F, X, Y, Z, tuple(mask.shape)))
    p_pred = _p64(pred, "pred") if pred.dtype == torch.float64 else _p(pred, "pred")
    p_truth, p_mask = _p(truth, "truth"), _p(mask, "mask")
    if truth.device != pred.device or mask.device != pred.device:
        raise FdnError("volume_metrics: pred, truth and mask must live on one device")
    if out is None:
        out = torch.empty((F, VOLUME_METRICS_COLUMNS), device=pred.device, dtype=torch.float64)
    elif tuple(out.shape) != (F, VOLUME_METRICS_COLUMNS) or out.device != pred.device:
        raise FdnError("volume_metrics: out must be (%d,%d) on %s, got %s on %s" % (F, VOLUME_METRICS_COLUMNS, pred.device,
                                                                                  tuple(out.shape), out.device))
    need = volume_metrics_scratch_doubles(F)
    if scratch is None:
        scratch = _volume_metrics_scratch.get(pred.device)
        if scratch is None or scratch.numel() < need:
            scratch = _volume_metrics_scratch[pred.device] = torch.empty((need,), device=pred.device, dtype=torch.float64)
    elif scratch.numel() < need or scratch.device != pred.device:
        raise FdnError("volume_metrics: scratch needs %d float64 elements on %s" % (need, pred.device))
    check(_lib.load().fdn_volume_metrics(p_pred, int(pred.dtype == torch.float64), p_truth, p_mask, mask.shape[0], _p64(out, "out"),
                                         _p64(scratch, "scratch"), F, X, Y, Z, _stream()), "fdn_volume_metrics")
    return out


def l2_sumsq(w_flat, is_kernel, out=None):
    if out is None:
        out = torch.empty((1,), device=w_flat.device, dtype=torch.float32)
    check(_lib.load().fdn_l2_sumsq(_p(w_flat), _pu8(is_kernel, "is_kernel"), w_flat.numel(), _p(out), _stream()), "fdn_l2_sumsq")
    return out


ADAM_PARTIALS = 2048                  # FDN_ADAM_PARTIALS


def adam_step(w, g, m, v, is_kernel, lr_t, b1, b2, eps, l2_grad_scale, l2_scale_dev=None, sumsq_partials=None, lr_t_dev=None, frozen=None,
              g_scale_dev=None, clip_value=0.0, ema=None, ema_momentum=0.0, ema_init=False):
    """sumsq_partials (ADAM_PARTIALS floats): also receive per-block sums of the updated kernel parameters' squares.
    lr_t_dev (one fp32 device element): the step size is read from it on the device and `lr_t` is ignored (fdn_adam_step_dev) -- the
    form a captured launch needs, since a by-value lr_t would be frozen into the graph.
    frozen (one uint8 per parameter, fine-tuning): elements with a non-zero byte keep w, m and v, and their g, m and v are not touched
    (fdn_adam_step_masked); the others are updated exactly as without it.  None: the two entry points above, as always.
    Gradient clipping (fdn_adam_step_clipped; at most one of the two): g_scale_dev (one fp32 device element, the second float clip_scale
    leaves behind) multiplies the gradient, L2 term included, on the device; clip_value > 0 clamps every element of it to
    [-clip_value, clip_value].  Neither: the entry points above, as always.
    Weight EMA (fdn_adam_step_ema, the widest entry point): ema (one fp32 per parameter on the GPU) becomes
    ema_momentum * ema + (1 - ema_momentum) * w_new in fp32, formed in the same launch; ema_init: the old contents of ema are not read and
    the weights before the step take their place; frozen elements store their weight.  w, m, v and sumsq_partials get the bits of the
    call without ema.  None: the four routes above, as always."""
    clip_value = float(clip_value)
    clipped = g_scale_dev is not None or clip_value != 0.0
    if clipped:
        if g_scale_dev is not None and clip_value != 0.0:
            raise FdnError("adam_step: g_scale_dev and clip_value are both set (global_clipnorm and clipvalue exclude each other)")
        if g_scale_dev is not None and (not g_scale_dev.is_cuda or g_scale_dev.dtype != torch.float32 or g_scale_dev.numel() != 1):
            raise FdnError("adam_step: g_scale_dev must hold one float32 on the GPU")
        if not clip_value >= 0.0:
            raise FdnError("adam_step: clip_value must be >= 0 (0 = off), got %r" % clip_value)
    if sumsq_partials is not None and sumsq_partials.numel() < ADAM_PARTIALS:
        raise FdnError("adam_step: sumsq_partials needs %d floats" % ADAM_PARTIALS)
    if lr_t_dev is not None and (not lr_t_dev.is_cuda or lr_t_dev.dtype != torch.float32 or lr_t_dev.numel() < 1):
        raise FdnError("adam_step: lr_t_dev must hold one float32 on the GPU")
    if frozen is not None and frozen.numel() != w.numel():
        raise FdnError("adam_step: frozen holds %d bytes for %d parameters" % (frozen.numel(), w.numel()))
    if ema is not None:
        if not ema.is_cuda or ema.dtype != torch.float32 or ema.numel() != w.numel():
            raise FdnError("adam_step: ema must hold %d float32 on the GPU (one per parameter)" % w.numel())
        mom32 = ctypes.c_float(float(ema_momentum)).value              # what the device receives
        if not 0.0 <= mom32 < 1.0:
            raise FdnError("adam_step: ema_momentum must lie in [0, 1) as float32, got %r" % (ema_momentum,))
    lib = _lib.load()
    # every operand once, in the order the widest entry point takes them; the four argument lists below differ in what they leave out
    bufs = [_p(w), _p(g), _p(m), _p(v), _pu8(is_kernel, "is_kernel")]
    frozen_p, n = _pu8(frozen, "frozen", allow_none=True), w.numel()
    lr = [0.0 if lr_t_dev is not None else float(lr_t), _p(lr_t_dev, allow_none=True)]
    hyper = [float(b1), float(b2), float(eps), float(l2_grad_scale), _p(l2_scale_dev, allow_none=True)]
    clip = [_p(g_scale_dev, "g_scale_dev", allow_none=True), clip_value]
    tail = [_p(sumsq_partials, allow_none=True), _stream()]
    if ema is not None:
        entry = "fdn_adam_step_ema"
        args = bufs + [frozen_p, n] + lr + hyper + clip + [_p(ema, "ema"), mom32, 1 if ema_init else 0] + tail
    elif clipped:
        entry, args = "fdn_adam_step_clipped", bufs + [frozen_p, n] + lr + hyper + clip + tail
    elif frozen is not None:
        entry, args = "fdn_adam_step_masked", bufs + [frozen_p, n] + lr + hyper + tail
    elif lr_t_dev is not None:
        entry, args = "fdn_adam_step_dev", bufs + [n] + lr[1:] + hyper + tail
    else:
        entry, args = "fdn_adam_step", bufs + [n] + lr[:1] + hyper + tail
    check(getattr(lib, entry)(*args), entry)


def grad_accumulate(acc, g, first):
    """acc = g (first: a bit copy, whatever acc held) or acc += g (one fp32 add per element), on the current stream: the sum of the
    micro-batch gradient buffers of one optimiser step (fdn_grad_accumulate).  fp32 contiguous device tensors of equal numel that do
    not overlap; slices at any float offset are fine."""
    if acc.numel() != g.numel():
        raise FdnError("grad_accumulate: acc holds %d elements, g %d" % (acc.numel(), g.numel()))
    for name, t in (("acc", acc), ("g", g)):
        if t.dtype != torch.float32:
            raise FdnError("grad_accumulate: %s must be float32 (got %s)" % (name, t.dtype))
    check(_lib.load().fdn_grad_accumulate(_p(acc, "acc"), _p(g, "g"), acc.numel(), 1 if first else 0, _stream()), "fdn_grad_accumulate")
    return acc


def l2_sumsq_partials(w_flat, is_kernel, partials):
    """ADAM_PARTIALS per-block sums of the kernel parameters' squares (what adam_step leaves behind), for parameters no Adam step has touched."""
    if partials.numel() < ADAM_PARTIALS:
        raise FdnError("l2_sumsq_partials: partials needs %d floats" % ADAM_PARTIALS)
    check(_lib.load().fdn_l2_sumsq_partials(_p(w_flat), _pu8(is_kernel, "is_kernel"), w_flat.numel(), _p(partials), _stream()), "fdn_l2_sumsq_partials")
    return partials


def grad_sumsq_partials(g, w, is_kernel, l2_grad_scale, l2_scale_dev=None, partials=None, frozen=None):
    """ADAM_PARTIALS per-block sums of the squares of the gradient the next adam_step is about to consume: g + l2s * w on kernel
    elements (l2s = l2_grad_scale * l2_scale_dev[0], as in adam_step), g on biases, elements with a non-zero byte in `frozen` left out
    (their g is not read).  fdn_grad_sumsq_partials; follow with clip_scale."""
    if partials is None:
        partials = torch.empty((ADAM_PARTIALS,), device=g.device, dtype=torch.float32)
    elif partials.numel() < ADAM_PARTIALS:
        raise FdnError("grad_sumsq_partials: partials needs %d floats" % ADAM_PARTIALS)
    n = g.numel()
    for name, t in (("w", w), ("is_kernel", is_kernel), ("frozen", frozen)):
        if t is not None and t.numel() != n:
            raise FdnError("grad_sumsq_partials: %s holds %d elements for %d gradients" % (name, t.numel(), n))
    if l2_scale_dev is not None and (not l2_scale_dev.is_cuda or l2_scale_dev.dtype != torch.float32 or l2_scale_dev.numel() < 1):
        raise FdnError("grad_sumsq_partials: l2_scale_dev must hold one float32 on the GPU")
    check(_lib.load().fdn_grad_sumsq_partials(_p(g, "g"), _p(w, "w"), _pu8(is_kernel, "is_kernel"), _pu8(frozen, "frozen", allow_none=True), n,
                                              float(l2_grad_scale), _p(l2_scale_dev, "l2_scale_dev", allow_none=True), _p(partials, "partials"),
                                              _stream()), "fdn_grad_sumsq_partials")
    return partials


def clip_scale(partials, clip_norm, out=None):
    """out[0] = the global norm sqrt(sum of partials), out[1] = clip_norm / max(norm, clip_norm) (1.0 exactly when the clip is inactive, NaN
    when the norm is not finite), both left on the device (fdn_clip_scale).  out[1:2] is adam_step's g_scale_dev."""
    c32 = ctypes.c_float(float(clip_norm)).value              # the fp32 value the library receives
    if not (c32 > 0.0 and c32 != float("inf")):
        raise FdnError("clip_scale: clip_norm must be finite and > 0 in float32, got %r" % (clip_norm,))
    clip_norm = c32
    if out is None:
        out = torch.empty((2,), device=partials.device, dtype=torch.float32)
    elif out.numel() < 2:
        raise FdnError("clip_scale: out needs 2 floats")
    check(_lib.load().fdn_clip_scale(_p(partials, "partials"), partials.numel(), clip_norm, _p(out, "out"), _stream()), "fdn_clip_scale")
    return out


def sum_partials(partials, out=None):
    if out is None:
        out = torch.empty((1,), device=partials.device, dtype=torch.float32)
    check(_lib.load().fdn_sum_partials(_p(partials), partials.numel(), _p(out), _stream()), "fdn_sum_partials")
    return out


def pack_conv64_weights_batch(w_flat, w_offsets, packs, streams=None):
    """Every 64->64 kernel of the flat parameter buffer in one launch.  w_offsets: int64 DEVICE tensor of float offsets;
    packs: (n_layers, 2, CONV64_PACK_FLOATS).  streams = (forward mask, dgrad mask) of PACK_STREAM_* bits restricts the launch to
    those streams of the packs (conv64_pack_streams names the ones a grid reads); None = all."""
    n = w_offsets.numel()
    if w_offsets.dtype != torch.int64 or not w_offsets.is_cuda or packs.numel() != n * 2 * CONV64_PACK_FLOATS:
        raise FdnError("pack_conv64_weights_batch: bad offsets / packs")
    sf, sd = (PACK_STREAM_ALL, PACK_STREAM_ALL) if streams is None else streams
    check(_lib.load().fdn_pack_conv64_weights_batch_streams(_p(w_flat), w_offsets.data_ptr(), n, _p(packs), int(sf), int(sd), _stream()),
          "fdn_pack_conv64_weights_batch_streams")
    return packs


PACK_STREAM_DIRECT, PACK_STREAM_WINO_W, PACK_STREAM_WINO_H2, PACK_STREAM_WINO_H4, PACK_STREAM_WINO_H4S = 1, 2, 4, 8, 16
PACK_STREAM_ALL = 31
ROLE_FWD, ROLE_DGRAD, ROLE_DGRAD_FUSED = 0, 1, 2


def conv64_pack_streams(N, D, H, W, algo=ALGO_AUTO, role=ROLE_FWD):
    """PACK_STREAM_* bits of the pack streams the 64->64 entry point of `role` reads on an (N,D,H,W) grid (fdn_conv64_pack_streams)."""
    m = _lib.load().fdn_conv64_pack_streams(int(N), int(D), int(H), int(W), int(algo), int(role))
    check(min(m, 0), "fdn_conv64_pack_streams")
    return m

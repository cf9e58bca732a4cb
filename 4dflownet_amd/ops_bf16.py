"""Operator layer of the bf16 activation path (BASELINE.json configs[3]): torch.bfloat16 activation tensors,
fp32 parameters / parameter gradients / prediction -> raw pointers -> lib4dflow_hip.so.

Same function names, parameters and defaults as ops.py for everything network.py reaches through `self.ops`, so it selects one of the
two modules by dtype and asks nothing more (tests/test_abi.py holds the two to that).  Same rules: GPU only, no fallback.  An operator
that differs from its ops.py namesake only in the storage type is a call of the one body in ops.py."""
import functools
import math

import torch

from . import _lib
from ._lib import FdnError, check
from .ops import (ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, LEAKY_ALPHA, ALGO_AUTO, ROLE_FWD, _stream, loss_metrics, l2_sumsq, adam_step,  # noqa: F401
                  stitch_patches, pack_patch_cores, blend_patches, finish_volume, unrotate_accumulate, self_ensemble_orientations, volume_metrics, _ptr, _p as _pf, _mask_ptr,
                  _input_features, _input_features_volume, _pack_conv64_weights, _conv_cout1_dgrad_folded, _dgrad_fused_multi, _fold_halo_border,
                  _conv1x1_dgrad, _conv3d_wgrad, _wgrad_batch, _upsample_trilinear_fwd, _upsample_trilinear_bwd)

BF16 = torch.bfloat16
ACT_DTYPE = BF16
PACK_ELEMS = 27 * 64 * 64             # one bf16 operand stream per pack
_pb = functools.partial(_ptr, BF16)


def input_features(u, v, w, mu, mv, mw, phase=None, pc=None):
    return _input_features("fdn_input_features_bf16", BF16, u, v, w, mu, mv, mw, phase, pc)


def input_features_volume(frames, patch_size, counts, g0=0, count=None, phase=None, pc=None, stride=None, orientation=None):
    """ops.input_features_volume with bf16 phase / pc (the frames stay fp32)."""
    return _input_features_volume("fdn_input_features_volume_bf16", BF16, frames, patch_size, counts, g0, count, phase, pc, orientation,
                                  stride)


def pack_conv64_weights(w, wp_fwd=None, wp_dgrad=None, want_dgrad=True):
    """fp32 (3,3,3,64,64) -> bf16 operand streams (27*64*64 each)."""
    return _pack_conv64_weights("fdn_pack_conv64_weights_bf16", BF16, PACK_ELEMS, w, wp_fwd, wp_dgrad, want_dgrad)


def pack_conv64_weights_batch(w_flat, w_offsets, packs, streams=None):
    """Every 64->64 kernel of the flat fp32 parameter buffer in one launch.  w_offsets: int64 DEVICE tensor of float offsets;
    packs: bf16 (n_layers, 2, PACK_ELEMS).  streams: accepted and ignored, a bf16 pack is one stream (conv64_pack_streams)."""
    n = w_offsets.numel()
    if w_offsets.dtype != torch.int64 or not w_offsets.is_cuda or packs.dtype != BF16 or packs.numel() != n * 2 * PACK_ELEMS:
        raise FdnError("pack_conv64_weights_batch (bf16): bad offsets / packs")
    check(_lib.load().fdn_pack_conv64_weights_bf16_batch(_pf(w_flat, "w"), w_offsets.data_ptr(), n, _pb(packs), _stream()),
          "fdn_pack_conv64_weights_bf16_batch")
    return packs


def conv64_pack_streams(N, D, H, W, algo=ALGO_AUTO, role=ROLE_FWD):
    """ops.conv64_pack_streams: 0, no stream of a bf16 pack is selected by grid or algorithm (pack_conv64_weights_batch writes all of it)."""
    return 0


def conv64_mask_ok(N, D, H, W, algo=ALGO_AUTO):
    """ops.conv64_mask_ok: True, the bf16 64->64 kernels write / read sign masks on every grid."""
    return True


def conv64_dgrad_multi_ok(algos):
    """ops.conv64_dgrad_multi_ok: True, the bf16 kernels ignore the algorithm."""
    return True


def conv64_wgrad_batch_ok(algo=ALGO_AUTO):
    """ops.conv64_wgrad_batch_ok: True, the bf16 kernels ignore the algorithm."""
    return True


def conv3d_fwd(x, w, bias=None, act=ACT_NONE, alpha=LEAKY_ALPHA, residual=None, x2=None, wpack=None, out=None,
               ldy=None, y_coff=0, algo=ALGO_AUTO, mask=None):
    """x bf16 (N,D,H,W,Cin[/2 if x2]); w fp32 Keras layout; output bf16, except Cout == 1 (prediction) -> fp32.
    algo is accepted for signature parity with ops.conv3d_fwd and ignored: the bf16 kernels are direct convolutions.
    mask (64->64 only; new_sign_mask(out)): also receives the sign mask of the output, see conv64_fwd."""
    N, D, H, W = x.shape[:4]
    K, Cin, Cout = w.shape[0], w.shape[3], w.shape[4]
    if mask is not None:
        if (K, Cin, Cout) != (3, 64, 64) or x2 is not None or ldy not in (None, 64) or y_coff:
            raise FdnError("conv3d_fwd (bf16): a sign mask belongs to a dense 64->64 3x3x3 layer")
        if wpack is None:
            wpack, _ = pack_conv64_weights(w, want_dgrad=False)
        return conv64_fwd(x, wpack, bias, act, alpha, residual, out, mask=mask)
    odt = torch.float32 if Cout == 1 else BF16
    if out is None:
        out = torch.empty((N, D, H, W, Cout), device=x.device, dtype=odt)
        ldy = Cout
    elif ldy is None:
        ldy = out.shape[-1]
    if Cin == 64 and Cout == 64 and K == 3 and wpack is None:
        wpack, _ = pack_conv64_weights(w, want_dgrad=False)
    check(_lib.load().fdn_conv3d_fwd_bf16(_pb(x, "x"), _pb(x2, allow_none=True), _pf(w, "w"), _pb(wpack, allow_none=True),
                                          _pf(bias, allow_none=True), _pb(residual, allow_none=True), _ptr(odt, out, "out"),
                                          N, D, H, W, Cin, Cout, K, ldy, y_coff, act, float(alpha), _stream()),
          "fdn_conv3d_fwd_bf16")
    return out


def new_sign_mask(y):
    """Sign-mask buffer for a bf16 (N,D,H,W,64) tensor: 64 bits per voxel as four int16 words (include/fdn.h)."""
    return torch.empty(tuple(y.shape[:4]) + (4,), device=y.device, dtype=torch.int16)


def conv64_fwd(x, wpack, bias=None, act=ACT_NONE, alpha=LEAKY_ALPHA, residual=None, out=None, mask=None):
    """mask (new_sign_mask(out)), if given, receives bit c of voxel v = (out[v][c] > 0): what the fused dgrad needs of `out` for act'."""
    N, D, H, W, C = x.shape
    if C != 64:
        raise FdnError("conv64_fwd: 64 input channels expected, got %d" % C)
    if out is None:
        out = torch.empty_like(x)
    check(_lib.load().fdn_conv64_fwd_bf16_mask(_pb(x, "x"), _pb(wpack, "wpack"), _pf(bias, allow_none=True),
                                               _pb(residual, allow_none=True), _pb(out, "out"), _mask_ptr(mask, N * D * H * W, "conv64_fwd"),
                                               N, D, H, W, act, float(alpha), _stream()), "fdn_conv64_fwd_bf16_mask")
    return out


def conv3d_dgrad_fused(dz, wpack_dgrad, dxpad, out, skip=None, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, parts=3,
                       algo=ALGO_AUTO, mask=None):
    """mask: the sign mask the forward wrote beside y_prev (conv64_fwd(mask=...)); read instead of y_prev for act'.
    parts: 3 only, the bf16 kernel covers the inner box and the shell in one launch; algo is ignored."""
    N, D, H, W = dz.shape[:4]
    if parts != 3:
        raise FdnError("conv3d_dgrad_fused (bf16): one launch covers the inner box and the shell (parts=%r)" % (parts,))
    check(_lib.load().fdn_conv64_dgrad_fused_bf16_mask(_pb(dz, "dz"), _pb(wpack_dgrad, "wpack"), _pf(dxpad, "dxpad"),
                                                       _pb(skip, allow_none=True), _pb(y_prev, allow_none=True),
                                                       _mask_ptr(mask, N * D * H * W, "conv3d_dgrad_fused"), act, float(alpha),
                                                       _pb(out, "out"), N, D, H, W, _stream()), "fdn_conv64_dgrad_fused_bf16_mask")
    return out


conv64_dgrad_fused = conv3d_dgrad_fused


def conv3d_dgrad_fused_multi(dzs, wpacks_dgrad, dxpad, out, skip=None, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, algo=ALGO_AUTO, mask=None):
    """The fused dgrad of 1..3 64->64 layers that share their input, as ONE launch (ops.conv3d_dgrad_fused_multi for bf16 activations): the
    sum over the sources stays in the fp32 accumulators (the chained launches round the running sum to bf16 after every source)."""
    return _dgrad_fused_multi("fdn_conv64_dgrad_fused_bf16_multi", _pb, dzs, wpacks_dgrad, dxpad, out, skip, y_prev, act, alpha, mask)


def fold_halo_border(dxpads, out, skip=None, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA):
    return _fold_halo_border("fdn_fold_halo_border_bf16", _pb, dxpads, out, skip, y_prev, act, alpha)


def conv_cout1_dgrad_folded(dz, w, spatial, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, lddz=1, dz_coff=0, out=None,
                            dbias_prev=None, workspace=None, mask=None):
    """64->1 head dgrad (dz = fp32 prediction gradient) + halo fold + act'(y_prev): bf16 (N,D,H,W,64).
    mask: the sign mask conv64_fwd(mask=...) wrote beside y_prev; read instead of y_prev for act'."""
    src = (_pb(y_prev, "y_prev", allow_none=True), _mask_ptr(mask, math.prod(spatial), "conv_cout1_dgrad_folded"))
    return _conv_cout1_dgrad_folded("fdn_conv_cout1_dgrad_folded_bf16_mask", BF16, src, dz, w, spatial, act, alpha, lddz, dz_coff, out,
                                    dbias_prev, workspace)


def conv1x1_dgrad(dz, w, ya, yb, dxa=None, dxb=None):
    return _conv1x1_dgrad("fdn_conv1x1_dgrad_bf16", _pb, dz, w, ya, yb, dxa, dxb)


def wgrad_workspace_bytes(N, D, H, W, Cin, Cout, K):
    return int(_lib.load().fdn_conv3d_wgrad_bf16_workspace_bytes(N, D, H, W, Cin, Cout, K))


def conv3d_wgrad(x, dz, K, Cin, Cout, x2=None, want_bias=False, dw=None, dbias=None, workspace=None, lddz=None,
                 dz_coff=0, algo=ALGO_AUTO):
    """x bf16; dz bf16, except Cout == 1 where dz is the fp32 prediction gradient; dw / dbias fp32."""
    return _conv3d_wgrad("fdn_conv3d_wgrad_bf16", BF16, wgrad_workspace_bytes, x, dz, K, Cin, Cout, x2, want_bias, dw, dbias, workspace,
                         lddz, dz_coff)


def wgrad_batch_workspace_bytes(n_layers, N, D, H, W):
    return int(_lib.load().fdn_conv3d_wgrad_bf16_batch_workspace_bytes(n_layers, N, D, H, W))


def conv3d_wgrad_batch(xs, dzs, dws, dbiases=None, workspace=None, algo=ALGO_AUTO):
    """Weight gradients of several 64->64 3x3x3 layers that share one grid, up to seven per launch (fdn_conv3d_wgrad_bf16_batch): xs / dzs
    bf16 (N,D,H,W,64), dws fp32 (3,3,3,64,64); dbiases: None or a list with None / fp32 (64,) entries.  algo: signature parity, ignored."""
    return _wgrad_batch("fdn_conv3d_wgrad_bf16_batch", _pb, wgrad_batch_workspace_bytes, xs, dzs, dws, dbiases, workspace)


def upsample_trilinear_fwd(x, R, out=None):
    return _upsample_trilinear_fwd("fdn_upsample_trilinear_fwd_bf16", BF16, x, R, out)


def upsample_trilinear_bwd(dy, R, y_prev=None, act=ACT_NONE, alpha=LEAKY_ALPHA, out=None):
    return _upsample_trilinear_bwd("fdn_upsample_trilinear_bwd_bf16", BF16, dy, R, y_prev, act, alpha, out)

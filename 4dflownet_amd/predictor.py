"""Full-volume sliding-window inference, mirroring src/predictor.py: patchify -> batched forward -> stitch ->
de-normalise -> zero sub-pixel velocities -> append u,v,w (+dx/res_increase) to the output HDF5.

With torch.distributed initialised (BASELINE cfg5) the patch list is split contiguously across ranks; every rank
runs its share through the same pipelined HIP forward loop and sends exactly its rows to rank 0, which stitches and writes.
With the device tiler (predict_file(device_tiler=True)) the ranks send only the cores of their predictions, and rank 0
stitches, de-normalises and zeroes them on the device (_predict_file_device)."""
import functools
import os
import time
import types

import numpy as np
import torch

from . import h5io, parallel
from .data import ImageDataset
from .network import Input, SR4DFlowNet
from .ops import self_ensemble_orientations
from .tiler import PatchGenerator, check_blend


def prepare_network(patch_size, res_increase, low_resblock, hi_resblock, device=None, dtype="float32", output_activation=None):
    """predictor.py:11-29.  dtype="bfloat16" runs the forward with bf16 activation storage (fp32 weights / prediction).
    output_activation: None / 'linear', or 'tanh' for weights trained with bounded heads (the reference's first published set); a
    weights file does not say which, so the caller does."""
    shape = (patch_size, patch_size, patch_size, 1)
    ins = [Input(shape, n) for n in ('u', 'v', 'w', 'u_mag', 'v_mag', 'w_mag')]
    return SR4DFlowNet(res_increase).build_network(*ins, low_resblock, hi_resblock, device=device, dtype=dtype,
                                                    output_activation=output_activation)


def save_to_h5(output_filepath, col_name, dataset, compression=None):
    """src/utils/prediction_utils.py:15-28."""
    h5io.append_dataset(output_filepath, col_name, dataset, compression=compression)


class _PredictorState:
    """What the predictor keeps on a network between calls: ONE copy stream, created on first use, and buffers by name -- pinned host ones
    and device ones.  A name holds `count` equal tensors; they are re-allocated when a request no longer fits: another shape, or with
    grow=True (flat storage, handed out as views) more elements than are held."""

    def __init__(self, device):
        self.device, self.stream, self.pinned_buffers, self.device_buffers = device, None, {}, {}

    def copy_stream(self):
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        return self.stream

    def _buffers(self, held, name, shape, count, grow, alloc):
        shape, n = tuple(shape), int(np.prod(shape))
        bufs = held.get(name)
        if bufs is None or (bufs[0].numel() < n if grow else tuple(bufs[0].shape) != shape):
            bufs = held[name] = [alloc((n,) if grow else shape) for _ in range(count)]
        return [b[:n].view(shape) for b in bufs] if grow else bufs

    def pinned(self, name, shape, dtype, count=1, grow=False):
        return self._buffers(self.pinned_buffers, name, shape, count, grow, lambda s: torch.empty(s, dtype=dtype).pin_memory())

    def on_device(self, name, shape, dtype):
        return self._buffers(self.device_buffers, name, shape, 1, False, lambda s: torch.empty(s, device=self.device, dtype=dtype))[0]


def _state(network):
    st = getattr(network, "_predictor_state", None)
    if st is None:
        st = network._predictor_state = _PredictorState(network.device)
    return st


class _CopyOut:
    """Device results to the host behind the producer of the next one.  push() queues the copy of chunk k into pinned slot k & 1 on the
    copy stream and then runs the host work of chunk k - 1 -- its copy has long finished, and its slot is not written again before the
    next push --, so the loop costs the producer's time only; flush() runs the host work that is still owed."""

    def __init__(self, network, stage):
        self.stage, self.copy_stream = stage, _state(network).copy_stream()
        self.main = torch.cuda.current_stream(network.device)
        self.k, self.owed = 0, None                  # owed: (event, host view, on_host, device tensor kept alive)

    def push(self, t, count, on_host):
        """t: a device tensor whose first dimension is `count` <= the slots'; on_host(view) gets that many rows of the slot, as numpy."""
        view = self.stage[self.k & 1][:count]
        self.k += 1
        self.copy_stream.wait_stream(self.main)
        with torch.cuda.stream(self.copy_stream):
            view.copy_(t, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        t.record_stream(self.copy_stream)
        self.flush()                                 # the previous chunk, while this one is copied and the next one produced
        self.owed = (ev, view, on_host, t)

    def flush(self):
        if self.owed is not None:
            ev, view, on_host, _keep = self.owed
            self.owed = None
            ev.synchronize()
            on_host(view.numpy())


def _drain_to_host(network, chunks, res, batch_size):
    """chunks: iterable of (first row, device tensor (cnt,S,S,S,3) fp32 or fp64) in production order.  Converts to float64 on the
    device (main stream) and moves every chunk into its rows of `res` through _CopyOut."""
    S = res.shape[1]
    pipe = _CopyOut(network, _state(network).pinned("rows", (batch_size, S, S, S, 3), torch.float64, count=2))

    def into(r0):
        def on_host(rows):
            res[r0:r0 + len(rows)] = rows
        return on_host

    for r0, out in chunks:
        out64 = out.double()
        pipe.push(out64, out64.shape[0], into(r0))
    pipe.flush()
    return res


def _forward_chunks(network, velocities, magnitudes, batch_size, lo, hi, base=0, keep=None):
    """The batched forward loop of predictor.py:79-94 over patches [lo, hi): yields (row - base, prediction) per batch; with `keep`
    (a device buffer) every prediction is also stored at rows [row - lo, ...) of it."""
    for s in range(lo, hi, batch_size):
        e = min(s + batch_size, hi)
        ins = [velocities[i][s:e] for i in range(3)] + [magnitudes[i][s:e] for i in range(3)]
        out = network.forward(ins)
        if keep is not None:
            keep[s - lo:e - lo].copy_(out)
        yield s - base, out


def _predict_pipelined(network, velocities, magnitudes, batch_size, lo, hi):
    """Single-process path: forward + float64 conversion on the device, results to the host behind the next batch's compute."""
    S = velocities[0].shape[1] * network.res_increase
    res = np.empty((hi - lo, S, S, S, 3), dtype=np.float64)
    return _drain_to_host(network, _forward_chunks(network, velocities, magnitudes, batch_size, lo, hi, base=lo), res, batch_size)


def shard_bounds(n, world):
    """Contiguous shards of the patch list: rank r owns rows [bounds[r], bounds[r+1]) (the last ranks may own none)."""
    per = (n + world - 1) // world
    return [min(r * per, n) for r in range(world + 1)]


def _send_rows(network, t):
    """A rank's shard -- one fp32 device buffer of predictions or packed cores -- to rank 0: one grouped RCCL send of the device buffer,
    or through pinned host memory under gloo."""
    import torch.distributed as dist
    if parallel._host_staged():
        host, = _state(network).pinned("transport", tuple(t.shape), torch.float32, grow=True)
        host.copy_(t, non_blocking=True)
        torch.cuda.current_stream(network.device).synchronize()
        dist.send(host, dst=0)
        return
    for q in dist.batch_isend_irecv([dist.P2POp(dist.isend, t, 0)]):
        q.wait()


def _recv_rows(network, shapes):
    """Rank 0: the shards of the peers {rank: shape} -- shapes that differ in the number of rows alone -- as ONE fp32 device tensor, rank after
    rank, ordered on the current stream.  One grouped RCCL launch for all peers; under gloo each shard arrives in pinned host memory and
    is uploaded."""
    import torch.distributed as dist
    dev = torch.device(network.device)
    ranks = sorted(shapes)
    rows = torch.empty((sum(shapes[r][0] for r in ranks),) + tuple(shapes[ranks[0]][1:]), device=dev, dtype=torch.float32)
    parts = dict(zip(ranks, rows.split([shapes[r][0] for r in ranks])))
    if parallel._host_staged():
        for r, part in parts.items():
            host, = _state(network).pinned("transport", shapes[r], torch.float32, grow=True)
            dist.recv(host, src=r)
            part.copy_(host, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()          # the one staging buffer is reused for the next peer
        return rows
    for q in dist.batch_isend_irecv([dist.P2POp(dist.irecv, part, r) for r, part in parts.items()]):     # one grouped RCCL launch
        q.wait()                                                  # makes the current stream wait for the transfers; no host sync
    return rows


def predict_patches(network, velocities, magnitudes, batch_size):
    """The batched predict loop of predictor.py:79-94 (results accumulate in float64 like np.zeros + np.append there).

    Data-parallel (BASELINE cfg5): the patch list is sharded contiguously over the ranks, every rank runs the same pipelined loop
    on its shard, and rank 0 -- the only rank that stitches and writes -- receives exactly the rows each rank owns (no padding, no
    copy to ranks that do not need it).  Returns the (n,S,S,S,3) float64 array on rank 0 and None on the other ranks.
      On the device the fp32 predictions of every peer travel as one buffer (_send_rows / _recv_rows: device-to-device under nccl = RCCL,
      through pinned host memory under gloo, two ranks on one device); rank 0 then converts them to float64 on the device and drains
      them through the pinned staging buffers like its own.
      CPU stand-in network (tests, gloo): every rank fills float64 host rows and sends those."""
    n = len(velocities[0])
    world, rank = parallel.world_size(), parallel.rank()
    if world == 1:
        return _predict_pipelined(network, velocities, magnitudes, batch_size, 0, n)
    import torch.distributed as dist
    S = velocities[0].shape[1] * network.res_increase
    bounds = shard_bounds(n, world)
    lo, hi = bounds[rank], bounds[rank + 1]
    dev = torch.device(network.device)
    if dev.type == "cuda":
        if rank == 0:
            res = np.empty((n, S, S, S, 3), dtype=np.float64)
            _drain_to_host(network, _forward_chunks(network, velocities, magnitudes, batch_size, lo, hi), res, batch_size)
            # receives are posted AFTER the own shard (a pending RCCL receive is a kernel spinning on a few CUs); the peers finish
            # their equal shards at about the same time, so only the transfer itself (1.3 MB per patch over xGMI) is exposed
            peers = {r: (bounds[r + 1] - bounds[r], S, S, S, 3) for r in range(1, world) if bounds[r + 1] > bounds[r]}
            rest = _recv_rows(network, peers) if peers else None         # rows [hi, n): an empty shard is not waited for
            step = max(batch_size, 1)
            _drain_to_host(network, ((s, rest[s - hi:min(s + step, n) - hi]) for s in range(hi, n, step)), res, batch_size)
            return res
        if hi > lo:
            mine = torch.empty((hi - lo, S, S, S, 3), device=dev, dtype=torch.float32)
            for _ in _forward_chunks(network, velocities, magnitudes, batch_size, lo, hi, keep=mine):
                pass
            _send_rows(network, mine)
        return None
    # CPU stand-in network (tests): the same loop and host rows, without streams or pinned memory
    mine = np.empty((hi - lo, S, S, S, 3), dtype=np.float64)
    for r0, out in _forward_chunks(network, velocities, magnitudes, batch_size, lo, hi, base=lo):
        mine[r0:r0 + out.shape[0]] = out.detach().cpu().numpy().astype(np.float64)
    if rank == 0:
        res = np.empty((n, S, S, S, 3), dtype=np.float64)
        res[lo:hi] = mine
        for r in range(1, world):
            if bounds[r + 1] > bounds[r]:
                dist.recv(torch.from_numpy(res[bounds[r]:bounds[r + 1]]), src=r)     # straight into the result rows
        return res
    if hi > lo:
        dist.send(torch.from_numpy(mine), dst=0)
    return None


def _frame_scale_tensor(frame_scale, F, device):
    """frame_scale of predict_volume as the (F,2) float64 device table fdn_stitch_patches_finish reads."""
    if isinstance(frame_scale, torch.Tensor):
        t = frame_scale.to(device=device, dtype=torch.float64).contiguous()
    else:
        t = torch.tensor([[float(v), float(thr)] for v, thr in frame_scale], dtype=torch.float64).reshape(-1, 2).to(device)
    if tuple(t.shape) != (F, 2):
        raise ValueError("frame_scale must hold (venc, threshold) for each of the %d frames, got %s" % (F, tuple(t.shape)))
    return t


def _orientations(self_ensemble):
    """self_ensemble= of the predictor as the tuple of orientations to average over, or None for the plain path: off, and a list that is
    exactly the identity (ops.self_ensemble_orientations)."""
    orientations = self_ensemble_orientations(self_ensemble)
    return None if orientations is None or tuple(orientations) == ((0, 0),) else orientations


def _predict_batch(network, frames, patch_size, counts, g0, count, batch_size, orientations, stride=None):
    """The predictions (count,S,S,S,3) fp32 of global patches [g0, g0 + count) of resident frames.  orientations (a tuple of (plane, k),
    or None): for each one in order the features are formed in the rotated frame (ops.input_features_volume(orientation=)), the network
    runs on them and the prediction is turned back into the accumulator (ops.unrotate_accumulate); the last one divides by their
    number.  The mean lives in the accumulator until the next batch: the caller stitches or packs it before asking for another.
    stride (None: patch_size - 4): the window's advance for overlapping cores (PatchGenerator(blend=).stride)."""
    window = {} if stride is None else {"stride": stride}
    if orientations is None:
        phase, pc = network.ops.input_features_volume(frames, patch_size, counts, g0, count, **window)
        return network.forward_features(phase, pc)
    S = patch_size * network.res_increase
    acc = _state(network).on_device("ensemble", (batch_size, S, S, S, 3), torch.float32)[:count]     # kept on the network between calls
    last = len(orientations) - 1
    for j, o in enumerate(orientations):
        phase, pc = network.ops.input_features_volume(frames, patch_size, counts, g0, count, orientation=o, **window)
        network.ops.unrotate_accumulate(network.forward_features(phase, pc), acc, o, first=j == 0,
                                        divisor=len(orientations) if j == last else 1)
    return acc


def _volume_plan(who, network, frames, patch_size, self_ensemble, blend):
    """What predict_volume and predict_cores (`who`, for the messages) open with: the options checked -- blend first, before the network or
    the frames are touched --, the frames on the device and the window plan.  Returns (blend, orientations, frames, pgen, counts, extents)."""
    blend = check_blend(blend, patch_size, who)
    orientations = _orientations(self_ensemble)
    frames = network._to_dev(frames)
    if frames.dim() != 5 or frames.shape[1] != 6:
        raise ValueError("%s: frames must be (F,6,X,Y,Z), got %s" % (who, tuple(frames.shape)))
    pgen = PatchGenerator(patch_size, network.res_increase, blend)
    counts, _, extents = pgen.plan(tuple(frames.shape[2:]))
    return blend, orientations, frames, pgen, counts, extents


def predict_volume(network, frames, patch_size, batch_size, out=None, frame_scale=None, patch_range=None, self_ensemble=None, blend=0):
    """Sliding-window inference with the tiler on the device (predictor.py:67-115 without its host work).  frames: (F,6,X,Y,Z)
    normalised fp32 (u,v,w,mag_u,mag_v,mag_w as ImageDataset.load_vectorfield leaves them), numpy or a device tensor; they are
    uploaded once.  Runs batches of `batch_size` consecutive global patches -- a batch may span two frames, so only the last one is
    ragged --: features straight from the frames (ops.input_features_volume), network.forward_features, the cores into the output
    (ops.stitch_patches).  Returns the stitched NORMALISED predictions, a (F,3,X*R,Y*R,Z*R) fp32 device tensor (`out` if given);
    de-normalisation and the zeroing of sub-pixel velocities stay with the caller.
    frame_scale (a host sequence of (venc, threshold) per frame, or that as an (F,2) float64 device tensor): the output is float64 and
    FINISHED instead -- prediction * venc, +0.0 where its magnitude is below the threshold (predictor.py:103-107; a threshold of 0
    zeroes nothing) -- inside the stitch launch.
    patch_range=(lo, hi): only global patches [lo, hi) are computed and stitched (a data-parallel shard); the voxels of the other
    patches are left as they are.  Everything is queued on the current stream.
    self_ensemble ("rot90", or a sequence of (plane, k) orientations; ops.self_ensemble_orientations): every batch is predicted under each
    orientation -- the rotations the loader trains with, data.rotate_vector_field -- turned back and averaged in fp32 on the device before
    it is stitched (_predict_batch): len(orientations) forwards per patch.  None, False or [(0, 0)]: the plain path.
    blend=b > 0 (tiler.PatchGenerator(blend=b); 2*b <= patch_size - 4, else ValueError): overlap-add stitching.  Neighbouring cores overlap
    by b low-res voxels -- (E/(E-b))^3 times the patches, E = patch_size - 4 -- and every batch (the averaged one under self_ensemble) is
    added with its linear-ramp weights into an fp32 accumulator (ops.blend_patches), in ascending patch order: the bits do not depend on
    batch_size.  Without frame_scale the accumulator is the result: a fresh zeroed tensor, or `out`, which the caller zeroed and which
    is ADDED to -- this is how patch_range parts, run in ascending order, compose to the whole.  With frame_scale the accumulator is
    internal and the float64 output is finished from it at the end (ops.finish_volume): it holds the patches of patch_range alone."""
    blend, orientations, frames, pgen, counts, extents = _volume_plan("predict_volume", network, frames, patch_size, self_ensemble, blend)
    R = network.res_increase
    F = frames.shape[0]
    scale = None if frame_scale is None else _frame_scale_tensor(frame_scale, F, frames.device)
    dtype = torch.float32 if scale is None else torch.float64
    if out is None:
        # without blend every voxel belongs to one patch core; with it the fp32 result is accumulated into
        out = (torch.zeros if blend and scale is None else torch.empty)((F, 3) + extents, device=frames.device, dtype=dtype)
    elif tuple(out.shape) != (F, 3) + extents or out.dtype != dtype:
        raise ValueError("predict_volume: out must be %s %s, got %s %s" % (dtype, (F, 3) + extents, out.dtype, tuple(out.shape)))
    total = F * counts[0] * counts[1] * counts[2]
    lo, hi = (0, total) if patch_range is None else (int(patch_range[0]), int(patch_range[1]))
    if not 0 <= lo <= hi <= total:
        raise ValueError("predict_volume: patch_range (%d, %d) outside [0, %d]" % (lo, hi, total))
    if blend:
        acc = out if scale is None else torch.zeros((F, 3) + extents, device=frames.device, dtype=torch.float32)
        place = lambda pred, g0: network.ops.blend_patches(pred, acc, 2 * R, pgen.stride * R, counts, g0)
    else:
        place = lambda pred, g0: network.ops.stitch_patches(pred, out, 2 * R, counts, g0, frame_scale=scale)
    for g0 in range(lo, hi, batch_size):
        place(_predict_batch(network, frames, patch_size, counts, g0, min(batch_size, hi - g0), batch_size, orientations,
                             pgen.stride if blend else None), g0)
    return network.ops.finish_volume(acc, scale, out=out) if blend and scale is not None else out


def shard_frame_span(lo, hi, per_frame):
    """Frames [f0, f1) that the global patches [lo, hi) of frames of `per_frame` patches touch ((0, 0) for an empty range): what a
    rank loads for its shard.  Patch g is patch g - f0 * per_frame of those frames."""
    if hi <= lo:
        return 0, 0
    return lo // per_frame, (hi - 1) // per_frame + 1


def predict_cores(network, frames, patch_size, batch_size, lo, hi, first_frame=0, self_ensemble=None, blend=0):
    """The shard of a data-parallel rank: global patches [lo, hi) in batches of `batch_size` consecutive patches, the core of every
    prediction packed (ops.pack_patch_cores) into ONE (hi - lo, c, c, c, 3) fp32 device buffer, c = (patch_size - 4) * R -- what the
    rank sends; the receiver stitches it with side 0 at g0 = lo.  frames as in predict_volume; they may hold only the frames the range
    touches (shard_frame_span), first_frame being the global index of frames[0].  self_ensemble: as in predict_volume; the mean over the
    orientations is formed before the cores are packed, so what travels and what the receiver does are the same.
    blend: as in predict_volume -- the patches are those of the overlapping window; the receiver blends the cores (ops.blend_patches with
    side 0 at g0 = lo) instead of stitching them."""
    blend, orientations, frames, pgen, counts, _ = _volume_plan("predict_cores", network, frames, patch_size, self_ensemble, blend)
    R = network.res_increase
    per_frame = counts[0] * counts[1] * counts[2]
    lo, hi, base = int(lo), int(hi), int(first_frame) * per_frame
    if not base <= lo <= hi <= base + frames.shape[0] * per_frame:
        raise ValueError("predict_cores: patches [%d, %d) are not in frames %d..%d (%d patches each)"
                         % (lo, hi, first_frame, first_frame + frames.shape[0] - 1, per_frame))
    c = (patch_size - 4) * R
    cores = torch.empty((hi - lo, c, c, c, 3), device=frames.device, dtype=torch.float32)
    for s in range(lo, hi, batch_size):
        e = min(s + batch_size, hi)
        pred = _predict_batch(network, frames, patch_size, counts, s - base, e - s, batch_size, orientations,
                              pgen.stride if blend else None)
        network.ops.pack_patch_cores(pred, 2 * R, out=cores[s - lo:e - lo])
    return cores


def _write_row(output_filepath, dataset, volume, meta, res_increase, round_small_values, finished=False):
    """One row of the output file from its stitched prediction.  volume: the three (X,Y,Z) components, normalised (fp32 or float64) -- or,
    finished=True, float64 in a staging buffer, de-normalised and zeroed on the device already: they are copied out and no arithmetic is
    done.  meta: the row's (venc, velocity_per_px, dx).  Appends u, v, w (+ dx / res_increase) and returns the three (1,X,Y,Z) float64
    volumes written."""
    venc, velocity_per_px, dx = meta
    vols, cols = [], []
    for i in range(3):
        if finished:
            v = volume[i].copy()                                       # the staging buffer is reused
        else:
            v = np.asarray(volume[i], dtype=np.float64) * venc         # de-normalise (:103)
            if round_small_values:
                v[np.abs(v) < velocity_per_px] = 0                     # (:104-107)
        v = np.expand_dims(v, axis=0)
        vols.append(v)
        cols.append((dataset.velocity_colnames[i], v))
    if dx is not None:
        cols.append((dataset.dx_colname, np.expand_dims(dx / res_increase, axis=0)))
    h5io.append_datasets(output_filepath, cols, compression='gzip')   # u, v, w (+ dx/R): one pass over the file
    return tuple(vols)


DEVICE_TILER_GROUP_BYTES = 1 << 30        # frames + stitched output of one group of rows (predict_file(device_tiler=True))


def _plan_groups(job, frames_per_group):
    """The groups of _predict_file_device, added to its `job`: fpg rows per group (frames_per_group, or what fits
    DEVICE_TILER_GROUP_BYTES), the window plan of one frame and the side of a packed core."""
    job.lr_shape = job.dataset.get_volume_shape(job.input_filepath)
    R, blend, device_finish = job.R, job.blend, job.device_finish
    if frames_per_group is None:                                       # depends on the file alone: all ranks walk the same groups
        # the six fp32 inputs, the stitched output (float64 when finished here) and, under blend, the fp32 accumulator beside it
        per_frame = int(np.prod(job.lr_shape)) * (24 + ((36 if blend else 24) if device_finish else 12) * R ** 3)
        frames_per_group = max(1, DEVICE_TILER_GROUP_BYTES // per_frame)
    job.fpg = max(1, min(int(frames_per_group), job.nr_rows))
    job.pgen = PatchGenerator(job.patch_size, R, blend)
    job.counts, _, _ = job.pgen.plan(job.lr_shape)
    job.per_frame_patches = job.counts[0] * job.counts[1] * job.counts[2]
    job.core = (job.patch_size - 4) * R


def _load_rows(job, rows):
    """Rows `rows` of the input file: the (len(rows),6,X,Y,Z) fp32 frames predict_volume takes and each row's (venc, velocity_per_px, dx)."""
    dataset = job.dataset
    frames = np.empty((len(rows), 6) + job.lr_shape, dtype=np.float32)
    meta = []
    for f, nrow in enumerate(rows):
        dataset.load_vectorfield(job.input_filepath, nrow)
        for c, a in enumerate((dataset.u, dataset.v, dataset.w, dataset.mag_u, dataset.mag_v, dataset.mag_w)):
            frames[f, c] = a
        meta.append((dataset.venc, dataset.velocity_per_px, dataset.dx))
    return frames, meta


def _device_peer_loop(network, job):
    """Rank r > 0 of _predict_file_device: per group the rows its shard touches, predict_cores, one buffer of cores to rank 0."""
    world, rank = parallel.world_size(), parallel.rank()
    for r0 in range(0, job.nr_rows, job.fpg):
        nrows = min(job.fpg, job.nr_rows - r0)
        bounds = shard_bounds(nrows * job.per_frame_patches, world)
        lo, hi = bounds[rank], bounds[rank + 1]
        if hi > lo:                                                    # an empty shard neither sends nor is waited for
            f0, f1 = shard_frame_span(lo, hi, job.per_frame_patches)
            frames, _ = _load_rows(job, list(range(r0 + f0, r0 + f1)))
            _send_rows(network, predict_cores(network, frames, job.patch_size, job.batch_size, lo, hi, first_frame=f0,
                                              self_ensemble=job.orientations, blend=job.blend))


def _write_group(job, rows, meta, t0, written, host):
    """The host work of one group that has arrived in pinned memory (host: (len(rows),3,X*R,Y*R,Z*R)): its rows to the file and to `written`."""
    if job.verbose:
        print("Processed rows %d-%d/%d: %d patches%s in %.2f secs." % (
            rows[0] + 1, rows[-1] + 1, job.nr_rows, len(rows) * job.per_frame_patches,
            "" if job.orientations is None else " x %d orientations" % len(job.orientations), time.time() - t0))
    for f, m in enumerate(meta):
        written.append(_write_row(job.output_filepath, job.dataset, host[f], m, job.R, job.round_small_values, finished=job.device_finish))


def _device_root_loop(network, job):
    """Rank 0 of _predict_file_device: per group its own shard through predict_volume, the peers' cores placed behind it, on_group, and the
    copy-out whose host work (_write_group) runs behind the next group's compute.  Returns the volumes written."""
    world, R, blend, counts = parallel.world_size(), job.R, job.blend, job.counts
    written, pipe = [], None
    if job.output_filepath is not None:
        # one pair of pinned buffers per dtype -- float64 for finished groups, fp32 with FDN_DEVICE_FINISH=0 --: switching does not re-pin
        dtype = torch.float64 if job.device_finish else torch.float32
        out_shape = (job.fpg, 3) + tuple(n * R for n in job.lr_shape)
        pipe = _CopyOut(network, _state(network).pinned(("groups", dtype), out_shape, dtype, count=2))
    for r0 in range(0, job.nr_rows, job.fpg):
        rows = list(range(r0, min(r0 + job.fpg, job.nr_rows)))
        frames, meta = _load_rows(job, rows)
        t0 = time.time()
        scale = None
        if job.device_finish:                                          # the doubles the host finish multiplies and compares with
            scale = _frame_scale_tensor([(venc, vpp if job.round_small_values else 0.0) for venc, vpp, _ in meta], len(rows), network.device)
        bounds = shard_bounds(len(rows) * job.per_frame_patches, world)
        vol = predict_volume(network, frames, job.patch_size, job.batch_size, frame_scale=None if blend else scale,
                             patch_range=(bounds[0], bounds[1]), self_ensemble=job.orientations, blend=blend)
        peers = {r: (bounds[r + 1] - bounds[r], job.core, job.core, job.core, 3) for r in range(1, world) if bounds[r + 1] > bounds[r]}
        if peers:                                                      # posted after the own shard (see predict_patches)
            got = _recv_rows(network, peers)                           # patches [bounds[1], ...), rank after rank
            for r in sorted(peers):
                cores = got[bounds[r] - bounds[1]:bounds[r + 1] - bounds[1]]
                if blend:
                    network.ops.blend_patches(cores, vol, 0, job.pgen.stride * R, counts, bounds[r])
                else:
                    network.ops.stitch_patches(cores, vol, 0, counts, bounds[r], frame_scale=scale)
        if blend and scale is not None:                                # the accumulator is complete: de-normalise and zero (:103-107)
            vol = network.ops.finish_volume(vol, scale)
        if job.on_group is not None:
            job.on_group(rows, vol)
        if pipe is not None:
            pipe.push(vol, len(rows), functools.partial(_write_group, job, rows, meta, t0, written))
    if pipe is not None:
        pipe.flush()
    return written



def _predict_file_device(network, input_filepath, output_filepath, patch_size, res_increase, batch_size, round_small_values, verbose,
                         frames_per_group, on_group=None, device_finish=None, self_ensemble=None, blend=0):
    """predict_file with the tiler on the device: rows in groups whose frames and stitched output fit DEVICE_TILER_GROUP_BYTES (or
    frames_per_group rows), one predict_volume per group, de-normalised and zeroed inside its stitch launches (frame_scale); the
    finished float64 group travels to pinned host memory on the copy stream while the next group computes and is then appended exactly
    as on the host path.  FDN_DEVICE_FINISH=0: the stitched group travels as fp32 and is finished on the host (A/B timing).
    Data-parallel: every group's patch list is split with shard_bounds; rank r > 0 loads the rows its shard touches, runs
    predict_cores and sends its one buffer of cores to rank 0, which stitches (and finishes) its own batches directly, posts the
    receives after its own shard (see predict_patches), and stitches every peer's buffer with side 0 at that peer's first patch.
    on_group(rows, vol): called on rank 0 for every group once it is stitched (the peers' cores included), before the copy-out, with the
    row numbers and the group's (len(rows),3,X*R,Y*R,Z*R) device tensor; what it queues on the current stream runs before the next group
    (evaluate_file).  output_filepath=None: no staging buffers, no copy to the host and no file; nothing is returned per row.
    device_finish: overrides FDN_DEVICE_FINISH.  self_ensemble: handed to predict_volume and, on the peers, predict_cores.
    blend > 0: overlap-add stitching (predict_volume(blend=)).  Rank 0 blends its own batches into the group's fp32 accumulator, then every
    peer's cores with side 0 at that peer's first patch, in rank order -- ascending patch order, so the bits are those of a single rank --
    and finishes the accumulator into the float64 group (ops.finish_volume); the byte budget counts the accumulator."""
    blend = check_blend(blend, patch_size, "predict_file")
    orientations = _orientations(self_ensemble)
    if device_finish is None:
        device_finish = os.environ.get("FDN_DEVICE_FINISH", "1") not in ("", "0")
    dataset = ImageDataset()
    nr_rows = dataset.get_dataset_len(input_filepath)
    if nr_rows == 0:
        return []
    job = types.SimpleNamespace(dataset=dataset, nr_rows=nr_rows, input_filepath=input_filepath, output_filepath=output_filepath,
                                patch_size=patch_size, R=res_increase, batch_size=batch_size, round_small_values=round_small_values,
                                verbose=verbose, on_group=on_group, device_finish=device_finish, orientations=orientations, blend=blend)
    _plan_groups(job, frames_per_group)
    if parallel.rank() > 0:
        _device_peer_loop(network, job)
        return []
    return _device_root_loop(network, job)


def predict_file(network, input_filepath, output_filepath, patch_size, res_increase, batch_size=8,
                 round_small_values=True, verbose=True, device_tiler=False, frames_per_group=None, self_ensemble=None, blend=0):
    """predictor.py:67-115 for every row of the input file.  Returns the list of (u,v,w) volumes written (rank 0; the other ranks
    of a data-parallel run compute their shard of every row's patches and return an empty list).
    device_tiler=True (or FDN_DEVICE_TILER=1): patchify and stitch run on the device (predict_volume) over groups of rows --
    frames_per_group rows, default what fits DEVICE_TILER_GROUP_BYTES; same file, same returned volumes (dtype and shape).  The
    de-normalisation and the zeroing of sub-pixel velocities run inside the stitch launch (FDN_DEVICE_FINISH=0: on the host, as before).
    Data-parallel runs shard every group's patches over the ranks; the peers send the cores of their patches, rank 0 stitches, finishes
    and writes (_predict_file_device).
    self_ensemble ("rot90" or a sequence of (plane, k) orientations, see predict_volume): every patch is predicted under each orientation
    and the predictions are averaged.  It exists on the device tiler only: when set, the file goes through _predict_file_device whatever
    device_tiler says (FDN_DEVICE_FINISH=0 keeps working); the host tiler path below does not have it.
    blend=b > 0: overlap-add stitching, neighbouring cores overlap by b low-res voxels and are cross-faded (predict_volume(blend=));
    like self_ensemble it goes through _predict_file_device whatever device_tiler says.  ValueError for a blend that is not an integer
    with 0 <= blend and 2*blend <= patch_size - 4.  (PatchGenerator(blend=b) + predict_patches is the same computation on the host.)"""
    blend = check_blend(blend, patch_size, "predict_file")
    orientations = _orientations(self_ensemble)
    if blend or orientations is not None or device_tiler or os.environ.get("FDN_DEVICE_TILER", "0") not in ("", "0"):
        return _predict_file_device(network, input_filepath, output_filepath, patch_size, res_increase, batch_size,
                                    round_small_values, verbose, frames_per_group, self_ensemble=orientations, blend=blend)
    pgen = PatchGenerator(patch_size, res_increase)
    dataset = ImageDataset()
    nr_rows = dataset.get_dataset_len(input_filepath)
    is0 = parallel.rank() == 0
    written = []
    for nrow in range(nr_rows):
        dataset.load_vectorfield(input_filepath, nrow)
        velocities, magnitudes = pgen.patchify(dataset)
        t0 = time.time()
        results = predict_patches(network, velocities, magnitudes, batch_size)
        if not is0:
            continue                              # rank 0 holds the gathered patches: it alone stitches and writes
        if verbose:
            print("Processed row %d/%d: %d patches in %.2f secs." % (nrow + 1, nr_rows, len(results), time.time() - t0))
        stitched = [pgen._patchup_with_overlap(results[:, :, :, :, i], pgen.nr_x, pgen.nr_y, pgen.nr_z) for i in range(3)]
        written.append(_write_row(output_filepath, dataset, stitched, (dataset.venc, dataset.velocity_per_px, dataset.dx), res_increase,
                                  round_small_values))
    return written


# the columns of ops.volume_metrics (fdn_volume_metrics): sums over one frame; m the mask, nf = [m < 0.5], fl = [m == 1], e = prediction -
# truth, q = |e|^2, corr the relative error of loss_utils.py:64-92, d the squared clamped central differences of e (the divergence term)
VOLUME_SUM_NAMES = (("sum_m", "sum_nf", "sum_fl", "sum_q_m", "sum_q_nf", "sum_corr_fl", "sum_eu2_fl", "sum_ev2_fl", "sum_ew2_fl",
                     "sum_d_m", "sum_d_nf") +
                    tuple(n.replace("c", c) for c in "uvw" for n in ("sum_tc_fl", "sum_pc_fl", "sum_tc2_fl", "sum_pc2_fl", "sum_tcpc_fl")))
METRIC_NAMES = (("mse", "rel_error", "div", "rmse_u", "rmse_v", "rmse_w", "rmse") + tuple("k_" + c for c in "uvw") +
                tuple("b_" + c for c in "uvw") + tuple("r2_" + c for c in "uvw") + ("n_fluid",))


def metrics_from_sums(sums):
    """Per frame a dict of METRIC_NAMES from the (F,26) sums of ops.volume_metrics (VOLUME_SUM_NAMES), on the host in float64:
    mse = S3/(S0+1) + S4/(S1+1) (TrainerController.py:101-107); rel_error = 100 S5/(S0+1) in % (loss_utils.py:97-101); div the divergence
    term with the same two means; rmse_c = sqrt(S_{6+c}/S2) and rmse = sqrt((S6+S7+S8)/S2) over the fluid voxels (m == 1); k_c, b_c, r2_c
    slope, intercept and R^2 of the least-squares line of prediction on truth over the fluid voxels; n_fluid = S2.  Without fluid voxels
    the RMSEs are 0 and the regression values NaN; they are NaN as well when the truth has no variance the moments can resolve."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, len(VOLUME_SUM_NAMES))
    nan = float("nan")
    res = []
    for S in sums:
        n = S[2]
        d = {"mse": S[3] / (S[0] + 1) + S[4] / (S[1] + 1), "rel_error": 100.0 * S[5] / (S[0] + 1),
             "div": S[9] / (S[0] + 1) + S[10] / (S[1] + 1)}
        for c, name in enumerate("uvw"):
            d["rmse_" + name] = float(np.sqrt(S[6 + c] / n)) if n > 0 else 0.0
        d["rmse"] = float(np.sqrt((S[6] + S[7] + S[8]) / n)) if n > 0 else 0.0
        for c, name in enumerate("uvw"):
            st, sp, stt, spp, stp = S[11 + 5 * c:16 + 5 * c]
            k = b = r2 = nan
            if n > 0:
                sxx, syy, sxy = stt - st * st / n, spp - sp * sp / n, stp - st * sp / n
                if sxx > 1e-12 * stt:          # below that the variance is the rounding of the moments' cancellation
                    k = sxy / sxx
                    b = sp / n - k * st / n
                    r2 = sxy * sxy / (sxx * syy) if syy > 0 else nan
            d["k_" + name], d["b_" + name], d["r2_" + name] = float(k), float(b), float(r2)
        d["n_fluid"] = float(n)
        res.append({key: float(d[key]) for key in METRIC_NAMES})
    return res


def write_metrics_csv(csv_path, metrics, first_row=0):
    """One header line `row,` + METRIC_NAMES and one line per row; %.17g, so the numbers read back exactly."""
    with open(csv_path, "w") as f:
        f.write("row," + ",".join(METRIC_NAMES) + "\n")
        for i, m in enumerate(metrics):
            f.write("%d," % (first_row + i) + ",".join("%.17g" % m[key] for key in METRIC_NAMES) + "\n")


def evaluate_file(network, input_filepath, hr_filepath, patch_size, res_increase, batch_size=8, round_small_values=True,
                  output_filepath=None, csv_path=None, frames_per_group=None, verbose=True, return_sums=False, self_ensemble=None,
                  blend=0):
    """Predict every row of the low-resolution file with the tiler on the device (_predict_file_device) and score the finished float64
    prediction, in m/s, against u, v, w of the same row of the high-resolution file (m/s as well: nothing is rescaled), where the
    prediction already is: ops.volume_metrics on every stitched group, 26 doubles per row to the host, metrics_from_sums there.  The
    HR file's mask holds one row (used for every frame) or one per row.  Returns the list of per-row dicts (METRIC_NAMES); with
    return_sums=True (metrics, sums) with sums the (rows,26) float64 array (VOLUME_SUM_NAMES).
    output_filepath=None: the prediction never leaves the device (no staging copy, no HDF5 write).  Given: the file
    predict_file(device_tiler=True) writes.  csv_path: write_metrics_csv.  Data-parallel: the peers send their cores as in
    _predict_file_device; rank 0 evaluates (and writes) and returns the list, the other ranks return [].
    self_ensemble: as in predict_file -- the scores are those of the averaged prediction, what the option buys on this checkpoint.
    blend: as in predict_file -- the scores are those of the blended volume.
    ValueError, before any GPU work: an invalid self_ensemble or blend, the two files hold different numbers of rows, the HR volume is not
    res_increase x the LR volume, or the mask has neither one row nor one per row."""
    blend = check_blend(blend, patch_size, "evaluate_file")
    orientations = _orientations(self_ensemble)
    dataset = ImageDataset()
    nr_rows = dataset.get_dataset_len(input_filepath)
    hr_rows = dataset.get_dataset_len(hr_filepath)
    if hr_rows != nr_rows:
        raise ValueError("evaluate_file: %s holds %d rows, %s holds %d" % (input_filepath, nr_rows, hr_filepath, hr_rows))
    lr_shape, hr_shape = dataset.get_volume_shape(input_filepath), dataset.get_volume_shape(hr_filepath)
    if hr_shape != tuple(n * res_increase for n in lr_shape):
        raise ValueError("evaluate_file: the high-resolution volume %s is not %d x the low-resolution volume %s"
                         % (hr_shape, res_increase, lr_shape))
    with h5io.open_read(hr_filepath) as hl:
        mask_shape = tuple(int(n) for n in hl["mask"].shape)
    if mask_shape[1:] != hr_shape or mask_shape[0] not in (1, nr_rows):
        raise ValueError("evaluate_file: the mask of %s is %s, expected (1 or %d,) + %s" % (hr_filepath, mask_shape, nr_rows, hr_shape))
    rd = lambda name: dataset._cache.get(hr_filepath, name)
    dev = torch.device(network.device)
    shared_mask = []                                                    # a one-row mask is uploaded once
    collected = []                                                      # (first row, (n,26) device tensor): read back at the end

    def score(rows, vol):
        truth = np.empty((len(rows), 3) + hr_shape, dtype=np.float32)
        for c, name in enumerate(dataset.velocity_colnames):
            truth[:, c] = rd(name)[rows[0]:rows[-1] + 1]
        if mask_shape[0] == 1:
            if not shared_mask:
                shared_mask.append(torch.from_numpy(np.ascontiguousarray(rd("mask"), dtype=np.float32)).to(dev))
            mask = shared_mask[0]
        else:
            mask = torch.from_numpy(np.ascontiguousarray(rd("mask")[rows[0]:rows[-1] + 1], dtype=np.float32)).to(dev)
        collected.append((rows[0], network.ops.volume_metrics(vol, torch.from_numpy(truth).to(dev), mask)))

    t0 = time.time()
    _predict_file_device(network, input_filepath, output_filepath, patch_size, res_increase, batch_size, round_small_values,
                         verbose and output_filepath is not None, frames_per_group, on_group=score, device_finish=True,
                         self_ensemble=orientations, blend=blend)
    if parallel.rank() != 0:
        return ([], np.empty((0, len(VOLUME_SUM_NAMES)))) if return_sums else []
    sums = np.empty((nr_rows, len(VOLUME_SUM_NAMES)), dtype=np.float64)
    for r0, t in collected:
        sums[r0:r0 + t.shape[0]] = t.cpu().numpy()
    metrics = metrics_from_sums(sums)
    if verbose:
        for i, m in enumerate(metrics):
            print("Row %d/%d: rel. error %.3f %%, RMSE %.5f m/s, slope u/v/w %.4f/%.4f/%.4f, R2 %.4f/%.4f/%.4f" % (
                i + 1, nr_rows, m["rel_error"], m["rmse"], m["k_u"], m["k_v"], m["k_w"], m["r2_u"], m["r2_v"], m["r2_w"]))
        print("Evaluated %d rows%s in %.2f secs." % (nr_rows, "" if orientations is None else " x %d orientations" % len(orientations),
                                                     time.time() - t0))
    if csv_path is not None:
        write_metrics_csv(csv_path, metrics)
    return (metrics, sums) if return_sums else metrics


def _start(who, blend, patch_size, res_increase, low_resblock, hi_resblock, dtype, output_activation, model_path, output_dir):
    """What main and evaluate_main (`who`) open with: blend checked before anything else, the process group from the environment, the
    network with its weights, and the output directory (made by rank 0).  Returns the network."""
    check_blend(blend, patch_size, who)
    parallel.init_from_env()
    network = prepare_network(patch_size, res_increase, low_resblock, hi_resblock, dtype=dtype, output_activation=output_activation)
    network.load_weights(model_path)
    if not os.path.isdir(output_dir) and parallel.rank() == 0:
        os.makedirs(output_dir)
    return network


def main(data_dir='../data', filename='example_data.h5', output_dir="../result", output_filename='example_result.h5',
         model_path="../models/4DFlowNet/4DFlowNet.h5", patch_size=24, res_increase=2, batch_size=8,
         round_small_values=True, low_resblock=8, hi_resblock=4, dtype="float32", device_tiler=False, frames_per_group=None,
         self_ensemble=None, blend=0, output_activation=None):
    """Same hard-coded surface as predictor.py:31-47 (+ dtype, + the device tiler switch, self_ensemble and blend of predict_file,
    + output_activation of prepare_network)."""
    network = _start("main", blend, patch_size, res_increase, low_resblock, hi_resblock, dtype, output_activation, model_path, output_dir)
    predict_file(network, '{}/{}'.format(data_dir, filename), '{}/{}'.format(output_dir, output_filename), patch_size,
                 res_increase, batch_size, round_small_values, device_tiler=device_tiler, frames_per_group=frames_per_group,
                 self_ensemble=self_ensemble, blend=blend)
    if parallel.rank() == 0:
        print("Done!")


def evaluate_main(data_dir='../data', filename='example_data.h5', hr_filename='example_data_HR.h5', output_dir="../result",
                  csv_filename='example_metrics.csv', output_filename=None, model_path="../models/4DFlowNet/4DFlowNet.h5", patch_size=24,
                  res_increase=2, batch_size=8, round_small_values=True, low_resblock=8, hi_resblock=4, dtype="float32",
                  frames_per_group=None, self_ensemble=None, blend=0, output_activation=None):
    """The surface of main() for scoring a checkpoint: + hr_filename, the ground truth beside `filename`, and csv_filename; the
    prediction itself is written only with output_filename."""
    network = _start("evaluate_main", blend, patch_size, res_increase, low_resblock, hi_resblock, dtype, output_activation, model_path,
                     output_dir)
    evaluate_file(network, '{}/{}'.format(data_dir, filename), '{}/{}'.format(data_dir, hr_filename), patch_size, res_increase, batch_size,
                  round_small_values, output_filepath=None if output_filename is None else '{}/{}'.format(output_dir, output_filename),
                  csv_path='{}/{}'.format(output_dir, csv_filename) if parallel.rank() == 0 else None, frames_per_group=frames_per_group,
                  self_ensemble=self_ensemble, blend=blend)
    if parallel.rank() == 0:
        print("Done!")


if __name__ == '__main__':
    main()

"""On-device input pipeline: PatchHandler3D whose volumes live in HBM.

Every HDF5 volume is decoded once and uploaded once; a batch is then produced by ten launches of
fdn_gather_patches (slice + np.rot90 + component swap/sign + /venc, /4095 or mask threshold), driven by a
descriptor table built from the CSV rows.  Outputs are device tensors, bit-identical to the host loader
(data.PatchHandler3D), which in turn is bit-identical to the reference's loader.

resynthesize=dict(seed=s): the low-res side is not read from a file but synthesised from the resident high-res volumes at the start of
every pass (fdn_kspace_downsample: k-space crop + noise, prepare_lowres.py's draws from private generators) -- a fresh noise
realisation, SNR, VENC set and magnitude level per frame and epoch."""
import os

import numpy as np
import torch

from . import _lib, h5io, ops, parallel, prepare_lowres
from ._lib import check
from .data import _ROT, PatchHandler3D

DESC_DTYPE = np.dtype([('src', '<u8'), ('X', '<i4'), ('Y', '<i4'), ('Z', '<i4'), ('t', '<i4'), ('x0', '<i4'), ('y0', '<i4'),
                       ('z0', '<i4'), ('plane', '<i4'), ('k', '<i4'), ('mode', '<i4'), ('sign', '<f4'), ('div', '<f4')])
assert DESC_DTYPE.itemsize == 56


class _DeviceBatches:
    def __init__(self, handler, indexes, shuffle, seed, shard):
        self.h = handler
        self.indexes = np.atleast_2d(indexes)
        self.sampler = parallel.ShardedIndexSampler(len(self.indexes), handler.batch_size, shuffle, seed,
                                                    rank_=shard[0], world=shard[1])
        self.passes = 0                                      # the epoch a resynthesising handler degrades for

    def __len__(self):
        return len(self.sampler)

    def __iter__(self):
        if self.h.resynthesize is not None:
            self.h.resynthesize_lowres(self.passes, self.indexes)
            self.passes += 1
        for rows in self.sampler:
            yield self.h.load_batch_device([self.indexes[r] for r in rows])


class DevicePatchHandler3D(PatchHandler3D):
    def __init__(self, data_dir, patch_size, res_increase, batch_size, mask_threshold=0.6, device=None, resynthesize=None):
        """resynthesize: None, or dict(seed=s[, downsample=res_increase]): every pass over a dataset of
        initialize_dataset begins with resynthesize_lowres(pass number); the low-res files the index rows name need not exist."""
        super().__init__(data_dir, patch_size, res_increase, batch_size, mask_threshold)
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self._dev = {}
        self._venc_override = {}                             # lr_path -> (T,3) float32, installed by resynthesize_lowres
        self.resynthesize = None if resynthesize is None else dict(resynthesize)
        if self.resynthesize is not None:
            unknown = set(self.resynthesize) - {"seed", "downsample"}
            if unknown or "seed" not in self.resynthesize:
                raise ValueError("resynthesize must be dict(seed=..[, downsample=..]), got %r" % (resynthesize,))
            if self.resynthesize.setdefault("downsample", res_increase) != res_increase:
                raise ValueError("resynthesize: downsample=%r must equal res_increase=%r" % (self.resynthesize["downsample"], res_increase))

    def _vencs(self, lr_path, idx):
        """venc_u, venc_v, venc_w of a frame: what resynthesize_lowres installed, else the file's."""
        if lr_path in self._venc_override:
            return self._venc_override[lr_path][idx]
        return [self._cache.get(lr_path, n)[idx] for n in self.venc_colnames]

    def resynthesize_lowres(self, epoch, indexes):
        """Degrade u, v, w of every frame of every high-res file the index rows name, on the device, and install the results as the
        resident low-res volumes (u, v, w, mag_u, mag_v, mag_w) and VENCs of the low-res name in those rows.  Per file and frame
        prepare_lowres.draw_degradations(seed, epoch, ordinal of the file) gives the SNR, the VENCs and the magnitude level
        (mag = mask * level); the noise is Philox in the kernel with stream_id = epoch << 32 | ordinal << 20 | frame.  High-res
        volumes and the mask are untouched."""
        rs = self.resynthesize
        if rs is None:
            raise ValueError("this handler was built without resynthesize=dict(seed=..)")
        R = self.res_increase
        pairs = sorted({(str(self._cell(r[0])), str(self._cell(r[1]))) for r in np.atleast_2d(indexes)})
        for ordinal, (lr_name, hr_name) in enumerate(pairs):
            lr_path = '{}/{}'.format(self.data_directory, lr_name)
            hr_path = '{}/{}'.format(self.data_directory, hr_name)
            hr = [self._dvol(hr_path, n) for n in self.hr_colnames]
            mask = self._dvol(hr_path, self.mask_colname)[0]
            T, shape = hr[0].shape[0], tuple(hr[0].shape[1:])
            if T >= 1 << 20 or ordinal >= 1 << 12:
                raise ValueError("resynthesize: %d frames / %d files exceed the stream_id layout" % (T, len(pairs)))
            crops = ops.kspace_crops(shape, 1 / R)
            lr_shape = tuple(2 * c for c in crops)                     # 2 * int((N // 2) / R) per axis
            if os.path.exists(lr_path):                                # a prepared file beside it: the index rows were made for ITS extents
                with h5io.open_read(lr_path) as f:
                    have = tuple(int(n) for n in f[self.lr_colnames[0]].shape[1:])
                if have != lr_shape:
                    raise ValueError("resynthesize: %s holds low-res volumes of %s, the synthesis of %s at 1/%d gives %s"
                                     % (lr_name, have, hr_name, R, lr_shape))
            snr, vencs, mags = prepare_lowres.draw_degradations(
                *[self._cache.get(hr_path, n + "_max") for n in self.hr_colnames], seed=rs["seed"], epoch=epoch, ordinal=ordinal)
            names = self.lr_colnames + self.mag_colnames
            if (lr_path, names[0]) not in self._dev or tuple(self._dev[(lr_path, names[0])].shape) != (T,) + lr_shape:
                for n in names:
                    self._dev[(lr_path, n)] = torch.empty((T,) + lr_shape, device=self.device, dtype=torch.float32)
            stage = torch.empty((3,) + shape, device=self.device, dtype=torch.float32)
            out = (torch.empty((3,) + lr_shape, device=self.device, dtype=torch.float32),
                   torch.empty((3,) + lr_shape, device=self.device, dtype=torch.float32))
            ws = torch.empty((ops.kspace_workspace_bytes(3, shape, crops) + 3) // 4, device=self.device, dtype=torch.float32)
            for t in range(T):
                for c in range(3):
                    stage[c].copy_(hr[c][t])
                ops.kspace_downsample(stage, mask, vencs[t], snr[t], crops, noise=None, seed=rs["seed"],
                                      stream_id=(int(epoch) << 32) | (ordinal << 20) | t, mag_scale=mags[t], out=out, workspace=ws)
                for c in range(3):
                    self._dev[(lr_path, self.lr_colnames[c])][t].copy_(out[0][c])
                    self._dev[(lr_path, self.mag_colnames[c])][t].copy_(out[1][c])
            self._venc_override[lr_path] = vencs.astype(np.float32)

    def _dvol(self, path, name):
        key = (path, name)
        if key not in self._dev:
            a = self._cache.get(path, name)
            if a is None:
                raise KeyError("%s has no dataset %r" % (path, name))
            self._dev[key] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        return self._dev[key]

    def initialize_dataset(self, indexes, shuffle, n_parallel=None, seed=0, shard=None, prefetch=None, pinned=None):
        print("Total dataset:", len(np.atleast_2d(indexes)), 'shuffle', shuffle)
        if shard is None:
            shard = (parallel.rank(), parallel.world_size())
        return _DeviceBatches(self, indexes, shuffle, seed, shard)

    def load_batch_device(self, rows):
        """rows: CSV rows -> the 11-tuple of PatchHandler3D batches as device tensors."""
        P, R = self.patch_size, self.res_increase
        H = P * R
        B = len(rows)
        z = lambda *s: torch.zeros(s, device=self.device)
        if B == 0:
            return tuple([z(0, P, P, P, 1)] * 6 + [z(0, H, H, H, 1)] * 3 + [z(0), z(0, H, H, H)])
        descs = [np.zeros(B, DESC_DTYPE) for _ in range(10)]        # lr u,v,w | mag u,v,w | hr u,v,w | mask
        vencs = np.zeros(B, np.float32)
        for b, row in enumerate(rows):
            row = [self._cell(c) for c in row]
            lr_path = '{}/{}'.format(self.data_directory, row[0])
            hr_path = '{}/{}'.format(self.data_directory, row[1])
            idx = int(row[2])
            x0, y0, z0 = int(row[3]), int(row[4]), int(row[5])
            is_rotate, plane, k = int(row[6]), int(row[7]), int(row[8])
            venc = np.max(self._vencs(lr_path, idx))
            vencs[b] = venc
            rot = _ROT.get((plane, k)) if is_rotate > 0 else None
            perm, sign = rot if rot else ((0, 1, 2), (1, 1, 1))
            pl, kk = (plane, k) if rot else (0, 0)

            def fill(d, vol, t, start, mode, sgn, div, pl_, kk_):
                S = P if d is descs[0] or d is descs[1] or d is descs[2] or d is descs[3] or d is descs[4] or d is descs[5] else H
                if t >= vol.shape[0] or any(s0 < 0 or s0 + S > n for s0, n in zip(start, vol.shape[1:])):
                    raise ValueError("patch %s + %d exceeds volume %s (row %s): the host loader would return a ragged patch"
                                     % (start, S, tuple(vol.shape), row))
                d[b] =(vol.data_ptr(), vol.shape[1], vol.shape[2], vol.shape[3], t, start[0], start[1], start[2], pl_, kk_,
                        mode, sgn, div)
            for c in range(3):
                src = perm[c]
                fill(descs[c], self._dvol(lr_path, self.lr_colnames[src]), idx, (x0, y0, z0), 0, float(sign[c]), float(venc), pl, kk)
                fill(descs[3 + c], self._dvol(lr_path, self.mag_colnames[src]), idx, (x0, y0, z0), 0, 1.0, 4095.0, pl, kk)
                fill(descs[6 + c], self._dvol(hr_path, self.hr_colnames[src]), idx, (x0 * R, y0 * R, z0 * R), 0, float(sign[c]),
                     float(venc), pl, kk)
            # the mask is rotated for any rotation_plane in 1..3 when rotate > 0 (rotate_object), one mask per file (row 0)
            mpl, mk = (plane, k) if (is_rotate > 0 and plane in (1, 2, 3)) else (0, 0)
            fill(descs[9], self._dvol(hr_path, self.mask_colname), 0, (x0 * R, y0 * R, z0 * R), 1, 1.0, float(self.mask_threshold),
                 mpl, mk % 4)
        table = torch.from_numpy(np.concatenate(descs).view(np.uint8)).to(self.device)      # one small H2D copy per batch
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        outs = []
        for i in range(10):
            S = P if i < 6 else H
            o = torch.empty((B, S, S, S, 1) if i < 9 else (B, S, S, S), device=self.device, dtype=torch.float32)
            check(lib.fdn_gather_patches(table.data_ptr() + i * B * DESC_DTYPE.itemsize, o.data_ptr(), B, S, stream),
                  "fdn_gather_patches")
            outs.append(o)
        self._keep = table                                   # keep the table alive until the next batch is built
        venc_t = torch.from_numpy(vencs).to(self.device)
        return tuple(outs[:9]) + (venc_t, outs[9])

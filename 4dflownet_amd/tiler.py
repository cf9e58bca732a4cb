"""Sliding-window tiler / stitcher, API-compatible with src/Network/PatchGenerator.py.

LR volume -> zero-pad 2 voxels per side (+ far-side pad so the stride P-4 tiles it exactly) -> overlapping P^3
patches at stride P-4 -> (network) -> crop 2*R HR voxels per side of every patch -> stitch -> crop the far-side pad.
Same outputs as the reference (pinned by tests/golden/reference_golden.json); the implementation is vectorised
(strided window view for patchify, one reshape/transpose for the stitch) instead of Python loops.

blend=b > 0 (no counterpart in the reference): neighbouring cores overlap by b LR voxels -- the window advances by stride = P-4-b -- and
are cross-faded with a linear ramp when they are stitched (overlap-add), in float32 and in the order of the device kernel
(fdn_blend_patches), so the host and the device tiler give the same bits."""
import operator

import numpy as np


def check_blend(blend, patch_size, who="PatchGenerator"):
    """blend as an int: the overlap of neighbouring cores in LR voxels, 0 <= blend and 2*blend <= patch_size - 4 (at most two cores
    overlap per axis).  Anything else raises ValueError."""
    try:
        b = None if isinstance(blend, bool) else operator.index(blend)
    except TypeError:
        b = None
    if b is None or b < 0 or 2 * b > int(patch_size) - 4:
        raise ValueError("%s: blend must be an integer with 0 <= blend and 2*blend <= patch_size-4 = %d, got %r"
                         % (who, int(patch_size) - 4, blend))
    return b


def ramp_weights(i, nr, core, ramp):
    """fp32 weights of the `core` HR voxels of patch i of nr along one axis: (2t+1)/(2*ramp) over the first `ramp` voxels where a lower
    neighbour overlaps, (2(core-t)-1)/(2*ramp) over the last `ramp` where an upper one does, 1 elsewhere (one fp32 divide each)."""
    w = np.ones(core, dtype=np.float32)
    if ramp > 0:
        t = np.arange(core)
        den = np.float32(2 * ramp)
        if i > 0:
            w[:ramp] = (2 * t[:ramp] + 1).astype(np.float32) / den
        if i < nr - 1:
            w[core - ramp:] = (2 * (core - t[core - ramp:]) - 1).astype(np.float32) / den
    return w


class PatchGenerator:
    def __init__(self, patch_size, res_increase, blend=0):
        self.patch_size = patch_size
        self.effective_patch_size = patch_size - 4      # 2 voxels stripped per side on LR (PatchGenerator.py:8)
        self.res_increase = res_increase
        self.blend = check_blend(blend, patch_size)
        self.stride = self.effective_patch_size - self.blend      # LR voxels the window advances by
        self.padding = (0, 0, 0)
        self.nr_x = self.nr_y = self.nr_z = 0

    # ---- padding rule of _pad_to_patch_size_with_overlap (PatchGenerator.py:53-86) ----
    def _far_pad(self, padded_len):
        side_pad = (self.patch_size - self.effective_patch_size) // 2
        res = padded_len % self.effective_patch_size
        if res > 2 * side_pad:
            return self.patch_size - res
        return 2 * side_pad - res

    def plan(self, shape):
        """Geometry of an LR volume of `shape` without touching its data: ((nr_x, nr_y, nr_z), HR crop padding, stitched output
        extents) -- what patchify leaves in nr_* / padding, and the shape _patchup_with_overlap returns.  With blend > 0: plan_blend."""
        if self.blend:
            return self.plan_blend(shape)
        side_pad = (self.patch_size - self.effective_patch_size) // 2
        padded = [int(n) + 2 * side_pad for n in shape]
        far = [self._far_pad(n) for n in padded]
        nr = tuple((n + f - 2 * side_pad) // self.effective_patch_size for n, f in zip(padded, far))
        return nr, tuple(f * self.res_increase for f in far), tuple(int(n) * self.res_increase for n in shape)

    def plan_blend(self, shape):
        """plan() for overlapping cores: per axis of extent n, nr = max(1, ceil((n - E) / stride) + 1) patches at self.stride and a far pad
        of (nr - 1) * stride + E - n voxels, so that the cores cover [0, n) and the last one is needed."""
        E, s = self.effective_patch_size, self.stride
        nr = tuple(max(1, -((E - int(n)) // s) + 1) for n in shape)
        far = tuple((c - 1) * s + E - int(n) for c, n in zip(nr, shape))
        return nr, tuple(f * self.res_increase for f in far), tuple(int(n) * self.res_increase for n in shape)

    def _generate_blend_patches(self, img):
        P, s = self.patch_size, self.stride
        nr, pad_hr, _ = self.plan_blend(img.shape)
        self.padding = pad_hr
        img = np.pad(img, tuple((2, 2 + p // self.res_increase) for p in pad_hr), 'constant')
        win = np.lib.stride_tricks.sliding_window_view(img, (P, P, P))[::s, ::s, ::s]
        assert win.shape[:3] == nr
        return np.ascontiguousarray(win).reshape((-1, P, P, P)), nr[0], nr[1], nr[2]

    def _blend_cores(self, patches, x, y, z):
        """Overlap-add of the cores in float32, patch after patch in (i,j,k) order with k fastest: acc = acc + fl(w * p) with
        w = fl(fl(wx*wy)*wz) -- the arithmetic and the order of fdn_blend_patches -- then the crop of the far pad."""
        R = self.res_increase
        side, C, sh = 2 * R, self.effective_patch_size * R, self.stride * R
        ramp = C - sh
        S = patches.shape[1]
        core = np.asarray(patches[:, side:S - side, side:S - side, side:S - side]).astype(np.float32)   # exact: they hold fp32 values
        acc = np.zeros(((x - 1) * sh + C, (y - 1) * sh + C, (z - 1) * sh + C), dtype=np.float32)
        wx = [ramp_weights(i, x, C, ramp) for i in range(x)]
        wy = [ramp_weights(j, y, C, ramp) for j in range(y)]
        wz = [ramp_weights(k, z, C, ramp) for k in range(z)]
        g = 0
        for i in range(x):
            for j in range(y):
                wxy = wx[i][:, None, None] * wy[j][None, :, None]
                for k in range(z):
                    w = wxy * wz[k][None, None, :]
                    dst = acc[i * sh:i * sh + C, j * sh:j * sh + C, k * sh:k * sh + C]
                    dst += w * core[g]
                    g += 1
        px, py, pz = self.padding
        acc = acc[:acc.shape[0] - px, :acc.shape[1] - py, :acc.shape[2] - pz]
        return acc.astype(patches.dtype) if np.issubdtype(patches.dtype, np.floating) else acc

    def _pad_to_patch_size_with_overlap(self, img):
        side_pad = (self.patch_size - self.effective_patch_size) // 2
        img = np.pad(img, ((side_pad, side_pad),) * 3, 'constant')
        pads = tuple(self._far_pad(n) for n in img.shape)
        img = np.pad(img, tuple((0, p) for p in pads), 'constant')
        self.padding = tuple(p * self.res_increase for p in pads)       # HR voxels to crop after stitching
        return img

    def _generate_overlapping_patches(self, img):
        if self.blend:
            return self._generate_blend_patches(img)
        P, E = self.patch_size, self.effective_patch_size
        img = self._pad_to_patch_size_with_overlap(img)
        all_pads = P - E
        nr = tuple((n - all_pads) // E for n in img.shape)
        win = np.lib.stride_tricks.sliding_window_view(img, (P, P, P))[::E, ::E, ::E]
        win = win[:nr[0], :nr[1], :nr[2]]
        stack = np.ascontiguousarray(win).reshape((-1, P, P, P))
        return stack, nr[0], nr[1], nr[2]

    def patchify(self, dataset):
        """-> ((u,v,w stacks), (mag stacks)), each (n_patches,P,P,P,1).  PatchGenerator.py:13-40."""
        stacks = []
        for a in (dataset.u, dataset.v, dataset.w, dataset.mag_u, dataset.mag_v, dataset.mag_w):
            s, i, j, k = self._generate_overlapping_patches(a)
            stacks.append(np.expand_dims(s, -1))
        self.nr_x, self.nr_y, self.nr_z = i, j, k
        return tuple(stacks[:3]), tuple(stacks[3:])

    def unpatchify(self, results):
        return tuple(self._patchup_with_overlap(results[:, :, :, :, c], self.nr_x, self.nr_y, self.nr_z) for c in range(3))

    def _patchup_with_overlap(self, patches, x, y, z):
        """patches (n,S,S,S) in (i,j,k) order with k fastest -> stitched volume.  PatchGenerator.py:116-154.  With blend > 0 the cores
        overlap and are cross-faded (_blend_cores)."""
        if self.blend:
            return self._blend_cores(patches, x, y, z)
        side_pad_hr = ((self.patch_size - self.effective_patch_size) // 2) * self.res_increase
        S = patches.shape[1]
        core = patches[:, side_pad_hr:S - side_pad_hr, side_pad_hr:S - side_pad_hr, side_pad_hr:S - side_pad_hr]
        c = core.shape[1]
        nx = len(patches) // (y * z)
        vol = core[:nx * y * z].reshape(nx, y, z, c, c, c).transpose(0, 3, 1, 4, 2, 5).reshape(nx * c, y * c, z * c)
        px, py, pz = self.padding
        if px > 0:
            vol = vol[:-px]
        if py > 0:
            vol = vol[:, :-py]
        if pz > 0:
            vol = vol[:, :, :-pz]
        return vol

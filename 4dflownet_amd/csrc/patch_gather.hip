// On-device input pipeline: the per-sample work of PatchHandler3D.load_patches_from_index_file
// (src/Network/PatchHandler3D.py:49-160) -- slice a P^3 (or (PR)^3) patch out of a resident 4-D volume, np.rot90 it
// in one of three planes, flip the sign of a velocity component, divide by venc / 4095, or threshold the mask --
// as ONE gather kernel per output tensor, driven by a small descriptor table built from the CSV rows.
// HBM-bound and tiny (2.1 MB per sample); its purpose is to take h5py + numpy slicing + H2D copies off the step's
// critical path when training from real data.
#include "fdn_common.h"
#include "kspace_dft.h"

struct PatchDesc {          // one per (sample, output tensor); mirrored by data_device.py (8 x int64)
    const float* src;       // volume base, layout (T, X, Y, Z)
    int32_t X, Y;
    int32_t Z, t;
    int32_t x0, y0;
    int32_t z0, plane;      // plane 0 = no rotation, 1:(0,1) 2:(0,2) 3:(1,2)  (np.rot90 axes)
    int32_t k, mode;        // k = rot90 count (1..3); mode 0 = sign * (v / div), 1 = (v >= thr) ? 1 : 0
    float sign, div;        // div = venc or 4095; thr is passed in `div` for mode 1
};

// mode 1 of the kernel, fdn_stitch_patches (src/Network/PatchGenerator.py:116-154, src/predictor.py:67-115): the inverse direction for
// inference.  B predicted patches (B,S,S,S,3) at `pred`, global patches g0 .. g0 + B of F frames of nx*ny*nz patches each (k fastest);
// the core of every patch (S - 2*side per axis) goes to out = (F,3,Xo,Yo,Zo) at patch coordinate * core, voxels beyond the extents (the
// cropped far pad) are dropped.  One element (voxel, component) per thread and step: reads are contiguous, writes of different patches
// disjoint.
// mode 2, fdn_stitch_patches_finish: the same walk, `out` is a float64 volume and every value is finished on the way
// (src/predictor.py:103-107, src/utils/ImageDataset.py:31): d = (double)p * venc_f, +0.0 where |d| < threshold_f, with {venc_f, threshold_f}
// read from the device table `scale` (F,2).
// mode 3, fdn_pack_patch_cores: the cores alone, contiguous, out = (B,cs,cs,cs,3) -- what a data-parallel rank sends to the rank that
// stitches (the same element walk: out[i] is the element mode 1 would place).
// mode 4, fdn_unrotate_accumulate: the self-ensemble's fan-in.  `pred` holds B predictions (B,S,S,S,3) of patches that were fed in a
// rotated frame (PatchHandler3D.apply_rotation, src/Network/PatchHandler3D.py:97-108,166-274); every element of out = (B,S,S,S,3) takes
// t = sign * pred[n][rho(a,b,c)][comp'] -- sg.orient is the INVERSE fdn_orient_word -- then v = first ? t : out + t, and on the last
// orientation v / (float)divisor.  One IEEE add and one correctly rounded divide; it walks the destination, so writes are contiguous
// (reads are strided for planes 2 and 3) and no two threads meet.
// modes 5 and 6, fdn_kspace_downsample: one forward / inverse truncated-DFT stage of the low-res synthesis (kspace_dft.h), driven by the
// by-value KspaceGeom; the only modes that are launched with dynamic LDS (the twiddle table).
// mode 7, fdn_blend_patches: overlap-add stitching.  The cores advance by sg.stride < core HR voxels, so up to two cores per axis -- eight
// per voxel -- cover an output voxel, each with the separable linear ramp of blend_weight.  The DESTINATION is walked: frames sg.f0 ..
// sg.f0 + sg.nf - 1, rows sg.x0 .. sg.x0 + sg.xs - 1 (the slab the patches of the call can touch), one (voxel, component) per thread and
// step.  The thread finds the covering patches from its coordinates, keeps those inside [g0, g0 + B) and adds them in ascending g:
// acc = acc + fl(w * p), the multiply and the add rounded separately (blend_add).  No atomics, no two threads on one voxel, and the bits
// do not depend on how the patch list is cut into calls that come in ascending g0.
// mode 8, fdn_finish_volume: mode 2's finish on an accumulated fp32 volume, `pred` (F,3,Xo,Yo,Zo) -> `out` float64 of the same shape.
struct StitchGeom {
    const float* pred;
    int64_t g0;
    int32_t Xo, Yo, Zo, side;
    int32_t nx, ny, nz, orient;
    const double* scale;    // mode 2 only
    int32_t first, divisor; // mode 4 only
    int32_t stride, f0;     // mode 7 only: HR stride of the cores, first frame of the slab
    int32_t nf, x0, xs;     // mode 7 only: frames of the slab, its first row and its rows
};

// Weight of HR core coordinate t in [0, cs) along one axis for patch i of n: the ramp (2t+1)/(2r) over the first r = cs - stride voxels
// where a lower neighbour overlaps, (2(cs-t)-1)/(2r) over the last r where an upper one does, 1 elsewhere.  One correctly rounded divide;
// the two ramps of an overlap sum to 1.  r <= cs - r (at most two cores overlap), so the two conditions exclude each other.
__device__ __forceinline__ float blend_weight(int i, int n, int t, int cs, int r) {
    if (i > 0 && t < r) return (float)(2 * t + 1) / (float)(2 * r);
    if (i < n - 1 && t >= cs - r) return (float)(2 * (cs - t) - 1) / (float)(2 * r);
    return 1.f;
}

// acc + fl(w * p): never contracted into a fused multiply-add, whatever the surrounding code invites the compiler to do
__device__ __forceinline__ float blend_add(float acc, float w, float p) {
#pragma clang fp contract(off)
    const float t = w * p;
    return acc + t;
}

__global__ __launch_bounds__(256) void gather_patches_kernel(const PatchDesc* __restrict__ desc, float* __restrict__ out, int B,
                                                              int S, int mode, StitchGeom sg, KspaceGeom kg) {
    if (mode == 5 || mode == 6) {                                       // fdn_kspace_downsample: 5 a forward stage, 6 an inverse one
        extern __shared__ __attribute__((aligned(16))) float ks_lds[];
        if (mode == 5) fdn_ks_stage<false>(kg, ks_lds);
        else fdn_ks_stage<true>(kg, ks_lds);
        return;
    }
    if (mode == 8) {
        const int64_t per = (int64_t)3 * sg.Xo * sg.Yo * sg.Zo;
        const int64_t total = per * B;                                  // B frames
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t f = i / per;
            double d = (double)sg.pred[i] * sg.scale[2 * f];            // de-normalise (:103)
            if (fabs(d) < sg.scale[2 * f + 1]) d = 0.0;                 // strict: a product equal to the threshold stays (:104-107)
            ((double*)out)[i] = d;
        }
        return;
    }
    if (mode == 7) {
        const int cs = S - 2 * sg.side, sh = sg.stride, r = cs - sh;
        const int64_t yz = (int64_t)sg.Yo * sg.Zo;
        const int64_t per = 3 * sg.xs * yz;                              // one frame of the slab
        const int64_t total = per * sg.nf;
        const int64_t g1 = sg.g0 + B;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t fl = i / per;
            int64_t q = i - fl * per;
            const int comp = (int)(q / (sg.xs * yz)); q -= comp * (sg.xs * yz);
            const int xl = (int)(q / yz); q -= xl * yz;
            const int y = (int)(q / sg.Zo), z = (int)(q - (int64_t)y * sg.Zo);
            const int x = sg.x0 + xl;
            const int64_t f = sg.f0 + fl;
            // per axis: the last patch that starts at or before the voxel, and the one before it where its core still reaches the voxel
            const int i1 = min(x / sh, sg.nx - 1), j1 = min(y / sh, sg.ny - 1), k1 = min(z / sh, sg.nz - 1);
            const int i0 = (i1 > 0 && x - (i1 - 1) * sh < cs) ? i1 - 1 : i1;
            const int j0 = (j1 > 0 && y - (j1 - 1) * sh < cs) ? j1 - 1 : j1;
            const int k0 = (k1 > 0 && z - (k1 - 1) * sh < cs) ? k1 - 1 : k1;
            const int64_t dst = (((f * 3 + comp) * sg.Xo + x) * sg.Yo + y) * sg.Zo + z;
            float v = 0.f;
            bool touched = false;
            for (int pi = i0; pi <= i1; ++pi)
                for (int pj = j0; pj <= j1; ++pj)
                    for (int pk = k0; pk <= k1; ++pk) {                  // ascending g
                        const int64_t g = ((f * sg.nx + pi) * sg.ny + pj) * sg.nz + pk;
                        if (g < sg.g0 || g >= g1) continue;
                        const int a = x - pi * sh, b = y - pj * sh, c = z - pk * sh;
                        const float w = blend_weight(pi, sg.nx, a, cs, r) * blend_weight(pj, sg.ny, b, cs, r) *
                                        blend_weight(pk, sg.nz, c, cs, r);           // fl(fl(wx * wy) * wz)
                        const int64_t n = g - sg.g0;
                        const float p = sg.pred[(((n * S + sg.side + a) * S + sg.side + b) * S + sg.side + c) * 3 + comp];
                        if (!touched) { v = out[dst]; touched = true; }
                        v = blend_add(v, w, p);
                    }
            if (touched) out[dst] = v;
        }
        return;
    }
    if (mode == 4) {
        const int64_t per = (int64_t)S * S * S * 3;
        const int64_t total = per * B;
        const float div = (float)sg.divisor;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t n = i / per;
            int r = (int)(i - n * per);
            int a = r / (S * S * 3); r -= a * S * S * 3;
            int b = r / (S * 3); r -= b * S * 3;
            int c = r / 3;
            const int comp = r - c * 3;
            fdn_rot_source(sg.orient, S, a, b, c);
            const int sc = comp == 0 ? fdn_orient_src(sg.orient, 0) : comp == 1 ? fdn_orient_src(sg.orient, 1) : fdn_orient_src(sg.orient, 2);
            const float sgn = comp == 0 ? fdn_orient_sign(sg.orient, 0) : comp == 1 ? fdn_orient_sign(sg.orient, 1) : fdn_orient_sign(sg.orient, 2);
            const float t = sgn * sg.pred[(((n * S + a) * S + b) * S + c) * 3 + sc];
            const float v = sg.first ? t : out[i] + t;
            out[i] = sg.divisor > 1 ? v / div : v;
        }
        return;
    }
    if (mode != 0) {
        const int cs = S - 2 * sg.side;                                  // core edge
        const int64_t per = (int64_t)cs * cs * cs * 3;
        const int64_t total = per * B;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t n = i / per;
            int r = (int)(i - n * per);
            const int a = r / (cs * cs * 3); r -= a * cs * cs * 3;
            const int b = r / (cs * 3); r -= b * cs * 3;
            const int c = r / 3, comp = r - c * 3;
            const int64_t src = (((n * S + sg.side + a) * S + sg.side + b) * S + sg.side + c) * 3 + comp;
            if (mode == 3) { out[i] = sg.pred[src]; continue; }
            int64_t g = sg.g0 + n;
            const int pk = (int)(g % sg.nz); g /= sg.nz;
            const int pj = (int)(g % sg.ny); g /= sg.ny;
            const int pi = (int)(g % sg.nx);
            const int64_t f = g / sg.nx;
            const int64_t x = (int64_t)pi * cs + a, y = (int64_t)pj * cs + b, z = (int64_t)pk * cs + c;
            if (x >= sg.Xo || y >= sg.Yo || z >= sg.Zo) continue;
            const float v = sg.pred[src];
            const int64_t dst = (((f * 3 + comp) * sg.Xo + x) * sg.Yo + y) * sg.Zo + z;
            if (mode == 2) {
                double d = (double)v * sg.scale[2 * f];                  // de-normalise (:103)
                if (fabs(d) < sg.scale[2 * f + 1]) d = 0.0;              // strict: a product equal to the threshold stays (:104-107)
                ((double*)out)[dst] = d;
            } else {
                out[dst] = v;
            }
        }
        return;
    }
    const int64_t per = (int64_t)S * S * S;
    const int64_t total = per * B;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / per);
        int r = (int)(i - (int64_t)b * per);
        int c[3];
        c[0] = r / (S * S); r -= c[0] * S * S;
        c[1] = r / S;
        c[2] = r - c[1] * S;
        const PatchDesc d = desc[b];
        if (d.plane) {
            // out = np.rot90(m, k, axes=(a,b)):  k=1: out[ia,ib] = m[ib, S-1-ia];  k=2: m[S-1-ia, S-1-ib];  k=3: m[S-1-ib, ia]
            const int a = d.plane == 3 ? 1 : 0, bb = d.plane == 1 ? 1 : 2;
            const int ia = c[a], ib = c[bb];
            if (d.k == 1) { c[a] = ib; c[bb] = S - 1 - ia; }
            else if (d.k == 2) { c[a] = S - 1 - ia; c[bb] = S - 1 - ib; }
            else if (d.k == 3) { c[a] = S - 1 - ib; c[bb] = ia; }
        }
        const float v = d.src[(((int64_t)d.t * d.X + d.x0 + c[0]) * d.Y + d.y0 + c[1]) * d.Z + d.z0 + c[2]];
        out[i] = d.mode ? (v >= d.div ? 1.f : 0.f) : d.sign * (v / d.div);
    }
}

extern "C" int fdn_gather_patches(const void* desc, float* out, int B, int S, void* stream) {
    FDN_REQUIRE(desc && out && B > 0 && S > 0, "fdn_gather_patches: bad argument");
    const int64_t total = (int64_t)B * S * S * S;
    int64_t nb = (total + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(gather_patches_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const PatchDesc*)desc,
                       out, B, S, 0, StitchGeom{}, KspaceGeom{});
    FDN_CHECK_LAUNCH("gather_patches_kernel");
    return FDN_OK;
}

// argument checks and launch shared by fdn_stitch_patches (scale == nullptr, mode 1) and fdn_stitch_patches_finish (mode 2)
static int stitch_launch(const char* who, const float* pred, void* vol, const double* scale, int mode, int F, int Xo, int Yo, int Zo, int S,
                         int side, int nx, int ny, int nz, int64_t g0, int count, void* stream) {
    FDN_REQUIRE(pred && vol && (mode == 1 || scale), "%s: NULL argument", who);
    FDN_REQUIRE(side >= 0 && S > 2 * side && S <= 512, "%s: S=%d must exceed 2*side (side=%d) and not 512", who, S, side);
    FDN_REQUIRE(F > 0 && nx > 0 && ny > 0 && nz > 0, "%s: bad frame / patch counts (F=%d, %d,%d,%d)", who, F, nx, ny, nz);
    FDN_REQUIRE(count > 0, "%s: count=%d", who, count);
    FDN_REQUIRE(g0 >= 0, "%s: g0=%lld", who, (long long)g0);
    FDN_REQUIRE(g0 + count <= (int64_t)F * nx * ny * nz, "%s: patches [%lld, %lld) exceed F*nx*ny*nz = %lld", who,
                (long long)g0, (long long)(g0 + count), (long long)((int64_t)F * nx * ny * nz));
    const int64_t cs = S - 2 * side;
    FDN_REQUIRE(Xo > 0 && Yo > 0 && Zo > 0 && Xo <= nx * cs && Yo <= ny * cs && Zo <= nz * cs,
                "%s: output extents (%d,%d,%d) must be in 1..n*(S-2*side) = (%lld,%lld,%lld)", who, Xo, Yo, Zo,
                (long long)(nx * cs), (long long)(ny * cs), (long long)(nz * cs));
    const int64_t total = (int64_t)count * cs * cs * cs * 3;
    int64_t nb = (total + 255) / 256;
    if (nb > 4096) nb = 4096;
    StitchGeom sg{};
    sg.pred = pred; sg.g0 = g0; sg.Xo = Xo; sg.Yo = Yo; sg.Zo = Zo; sg.side = side; sg.nx = nx; sg.ny = ny; sg.nz = nz; sg.scale = scale;
    hipLaunchKernelGGL(gather_patches_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const PatchDesc*)nullptr,
                       (float*)vol, count, S, mode, sg, KspaceGeom{});
    FDN_CHECK_LAUNCH("gather_patches_kernel");
    return FDN_OK;
}

extern "C" int fdn_stitch_patches(const float* pred, float* vol, int F, int Xo, int Yo, int Zo, int S, int side, int nx, int ny, int nz,
                                  int64_t g0, int count, void* stream) {
    return stitch_launch("fdn_stitch_patches", pred, vol, nullptr, 1, F, Xo, Yo, Zo, S, side, nx, ny, nz, g0, count, stream);
}

extern "C" int fdn_stitch_patches_finish(const float* pred, double* vol, const double* frame_scale, int F, int Xo, int Yo, int Zo, int S,
                                         int side, int nx, int ny, int nz, int64_t g0, int count, void* stream) {
    return stitch_launch("fdn_stitch_patches_finish", pred, vol, frame_scale, 2, F, Xo, Yo, Zo, S, side, nx, ny, nz, g0, count, stream);
}

extern "C" int fdn_blend_patches(const float* pred, float* acc, int F, int Xo, int Yo, int Zo, int S, int side, int stride_hr, int nx,
                                 int ny, int nz, int64_t g0, int count, void* stream) {
    const char* who = "fdn_blend_patches";
    FDN_REQUIRE(pred && acc, "%s: NULL argument", who);
    FDN_REQUIRE(side >= 0 && S > 2 * side && S <= 512, "%s: S=%d must exceed 2*side (side=%d) and not 512", who, S, side);
    FDN_REQUIRE(F > 0 && nx > 0 && ny > 0 && nz > 0, "%s: bad frame / patch counts (F=%d, %d,%d,%d)", who, F, nx, ny, nz);
    FDN_REQUIRE(count > 0, "%s: count=%d", who, count);
    FDN_REQUIRE(g0 >= 0, "%s: g0=%lld", who, (long long)g0);
    FDN_REQUIRE(g0 + count <= (int64_t)F * nx * ny * nz, "%s: patches [%lld, %lld) exceed F*nx*ny*nz = %lld", who,
                (long long)g0, (long long)(g0 + count), (long long)((int64_t)F * nx * ny * nz));
    const int64_t cs = S - 2 * side;
    FDN_REQUIRE(stride_hr >= 1 && stride_hr <= cs, "%s: stride_hr=%d must be in 1..S-2*side = %lld", who, stride_hr, (long long)cs);
    FDN_REQUIRE(2 * (cs - stride_hr) <= cs, "%s: stride_hr=%d lets more than two cores of edge %lld overlap per axis", who, stride_hr,
                (long long)cs);
    const int64_t sh = stride_hr;
    FDN_REQUIRE(Xo > 0 && Yo > 0 && Zo > 0 && Xo <= (nx - 1) * sh + cs && Yo <= (ny - 1) * sh + cs && Zo <= (nz - 1) * sh + cs,
                "%s: output extents (%d,%d,%d) must be in 1..(n-1)*stride_hr+(S-2*side) = (%lld,%lld,%lld)", who, Xo, Yo, Zo,
                (long long)((nx - 1) * sh + cs), (long long)((ny - 1) * sh + cs), (long long)((nz - 1) * sh + cs));
    // the slab of the destination the patches of this call can touch: their frames, and within a single frame the rows of their
    // patch planes (a call that spans frames walks them whole)
    const int64_t per_frame = (int64_t)nx * ny * nz, yzp = (int64_t)ny * nz;
    const int64_t f0 = g0 / per_frame, f1 = (g0 + count - 1) / per_frame;
    int64_t x0 = 0, x1 = Xo;
    if (f0 == f1) {
        const int64_t i0 = (g0 - f0 * per_frame) / yzp, i1 = (g0 + count - 1 - f0 * per_frame) / yzp;
        x0 = i0 * sh;
        x1 = i1 * sh + cs < Xo ? i1 * sh + cs : Xo;
        if (x0 >= x1) return FDN_OK;                                     // every patch of the call lies in the cropped far pad
    }
    StitchGeom sg{};
    sg.pred = pred; sg.g0 = g0; sg.Xo = Xo; sg.Yo = Yo; sg.Zo = Zo; sg.side = side; sg.nx = nx; sg.ny = ny; sg.nz = nz;
    sg.stride = stride_hr; sg.f0 = (int32_t)f0; sg.nf = (int32_t)(f1 - f0 + 1); sg.x0 = (int32_t)x0; sg.xs = (int32_t)(x1 - x0);
    const int64_t total = (int64_t)sg.nf * 3 * sg.xs * Yo * Zo;
    int64_t nb = (total + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(gather_patches_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const PatchDesc*)nullptr, acc,
                       count, S, 7, sg, KspaceGeom{});
    FDN_CHECK_LAUNCH("gather_patches_kernel");
    return FDN_OK;
}

extern "C" int fdn_finish_volume(const float* acc, double* vol, const double* frame_scale, int F, int Xo, int Yo, int Zo, void* stream) {
    const char* who = "fdn_finish_volume";
    FDN_REQUIRE(acc && vol && frame_scale, "%s: NULL argument", who);
    FDN_REQUIRE(F > 0 && Xo > 0 && Yo > 0 && Zo > 0, "%s: bad volume (F=%d, %d,%d,%d)", who, F, Xo, Yo, Zo);
    const int64_t total = (int64_t)F * 3 * Xo * Yo * Zo;
    int64_t nb = (total + 255) / 256;
    if (nb > 4096) nb = 4096;
    StitchGeom sg{};
    sg.pred = acc; sg.Xo = Xo; sg.Yo = Yo; sg.Zo = Zo; sg.scale = frame_scale;
    hipLaunchKernelGGL(gather_patches_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const PatchDesc*)nullptr,
                       (float*)vol, F, 0, 8, sg, KspaceGeom{});
    FDN_CHECK_LAUNCH("gather_patches_kernel");
    return FDN_OK;
}

extern "C" int fdn_pack_patch_cores(const float* pred, float* cores, int S, int side, int count, void* stream) {
    FDN_REQUIRE(pred && cores, "fdn_pack_patch_cores: NULL argument");
    FDN_REQUIRE(side >= 0 && S > 2 * side && S <= 512, "fdn_pack_patch_cores: S=%d must exceed 2*side (side=%d) and not 512", S, side);
    FDN_REQUIRE(count > 0, "fdn_pack_patch_cores: count=%d", count);
    const int64_t cs = S - 2 * side;
    const int64_t total = (int64_t)count * cs * cs * cs * 3;
    int64_t nb = (total + 255) / 256;
    if (nb > 4096) nb = 4096;
    StitchGeom sg{};
    sg.pred = pred; sg.side = side;
    hipLaunchKernelGGL(gather_patches_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const PatchDesc*)nullptr, cores,
                       count, S, 3, sg, KspaceGeom{});
    FDN_CHECK_LAUNCH("gather_patches_kernel");
    return FDN_OK;
}

extern "C" int fdn_unrotate_accumulate(const float* pred, float* acc, int count, int S, int plane, int k, int first, int divisor,
                                       void* stream) {
    FDN_REQUIRE(pred && acc, "fdn_unrotate_accumulate: NULL argument");
    FDN_REQUIRE(count > 0, "fdn_unrotate_accumulate: count=%d", count);
    FDN_REQUIRE(S > 0 && S <= 512, "fdn_unrotate_accumulate: S=%d must be in 1..512", S);
    const int word = fdn_orient_word(plane, k, 1);
    FDN_REQUIRE(word >= 0, "fdn_unrotate_accumulate: orientation (plane=%d, k=%d) is neither (0,0) nor plane in 1..3 with k in 1..3", plane, k);
    FDN_REQUIRE(first == 0 || first == 1, "fdn_unrotate_accumulate: first=%d must be 0 or 1", first);
    FDN_REQUIRE(divisor >= 1, "fdn_unrotate_accumulate: divisor=%d must be at least 1", divisor);
    const int64_t total = (int64_t)count * S * S * S * 3;
    const uintptr_t p0 = (uintptr_t)pred, a0 = (uintptr_t)acc, bytes = (uintptr_t)total * sizeof(float);
    FDN_REQUIRE(p0 + bytes <= a0 || a0 + bytes <= p0, "fdn_unrotate_accumulate: pred and acc overlap (%lld bytes each)", (long long)bytes);
    int64_t nb = (total + 255) / 256;
    if (nb > 4096) nb = 4096;
    StitchGeom sg{};
    sg.pred = pred; sg.orient = word; sg.first = first; sg.divisor = divisor;
    hipLaunchKernelGGL(gather_patches_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const PatchDesc*)nullptr, acc,
                       count, S, 4, sg, KspaceGeom{});
    FDN_CHECK_LAUNCH("gather_patches_kernel");
    return FDN_OK;
}

// Workspace of fdn_kspace_downsample: two complex fp32 volumes the stages ping-pong between -- A (nvol, 2cx, Y, Z) and B (nvol, 2cx, 2cy, Z),
// each large enough for every later stage that lands in it -- then the last forward stage's partial sums (nvol, FDN_KS_MAX_BLOCKS) and
// their totals (nvol).  Every part starts on a 16-byte boundary.
struct KsLayout { size_t a, b, partials, sums, total; };
static KsLayout ks_layout(int nvol, int Y, int Z, int cx, int cy) {
    auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
    KsLayout l;
    l.a = 0;
    l.b = l.a + up((size_t)nvol * 2 * cx * Y * Z * sizeof(float2));
    l.partials = l.b + up((size_t)nvol * 2 * cx * 2 * cy * Z * sizeof(float2));
    l.sums = l.partials + up((size_t)nvol * FDN_KS_MAX_BLOCKS * sizeof(float));
    l.total = l.sums + up((size_t)nvol * sizeof(float));
    return l;
}
static bool ks_extents_ok(int nvol, int X, int Y, int Z, int cx, int cy, int cz) {
    return nvol > 0 && nvol <= 65535 && X >= 1 && X <= FDN_KS_MAX_EXTENT && Y >= 1 && Y <= FDN_KS_MAX_EXTENT && Z >= 1 &&
           Z <= FDN_KS_MAX_EXTENT && cx >= 1 && cx <= X / 2 && cy >= 1 && cy <= Y / 2 && cz >= 1 && cz <= Z / 2;
}

extern "C" size_t fdn_kspace_downsample_workspace_bytes(int nvol, int X, int Y, int Z, int cx, int cy, int cz) {
    return ks_extents_ok(nvol, X, Y, Z, cx, cy, cz) ? ks_layout(nvol, Y, Z, cx, cy).total : 0;
}

static unsigned ks_blocks(int64_t per) {
    const int64_t nb = (per + 255) / 256;
    return (unsigned)(nb > FDN_KS_MAX_BLOCKS ? FDN_KS_MAX_BLOCKS : nb);
}

extern "C" int fdn_kspace_downsample(const float* vel, const float* mag, const float* params, int nvol, int X, int Y, int Z, int cx, int cy,
                                     int cz, const float* noise, uint64_t seed, uint64_t stream_id, float* out_vel, float* out_mag,
                                     float* sigma_out, void* workspace, void* stream) {
    const char* who = "fdn_kspace_downsample";
    FDN_REQUIRE(vel, "%s: vel is NULL", who);
    FDN_REQUIRE(mag, "%s: mag is NULL", who);
    FDN_REQUIRE(params, "%s: params is NULL", who);
    FDN_REQUIRE(out_vel, "%s: out_vel is NULL", who);
    FDN_REQUIRE(out_mag, "%s: out_mag is NULL", who);
    FDN_REQUIRE(workspace, "%s: workspace is NULL", who);
    FDN_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    FDN_REQUIRE(nvol > 0 && nvol <= 65535, "%s: nvol=%d must be in 1..65535", who, nvol);
    FDN_REQUIRE(X >= 1 && X <= FDN_KS_MAX_EXTENT, "%s: X=%d must be in 1..%d", who, X, FDN_KS_MAX_EXTENT);
    FDN_REQUIRE(Y >= 1 && Y <= FDN_KS_MAX_EXTENT, "%s: Y=%d must be in 1..%d", who, Y, FDN_KS_MAX_EXTENT);
    FDN_REQUIRE(Z >= 1 && Z <= FDN_KS_MAX_EXTENT, "%s: Z=%d must be in 1..%d", who, Z, FDN_KS_MAX_EXTENT);
    FDN_REQUIRE(cx >= 1 && cx <= X / 2, "%s: cx=%d must be in 1..X/2 = %d", who, cx, X / 2);
    FDN_REQUIRE(cy >= 1 && cy <= Y / 2, "%s: cy=%d must be in 1..Y/2 = %d", who, cy, Y / 2);
    FDN_REQUIRE(cz >= 1 && cz <= Z / 2, "%s: cz=%d must be in 1..Z/2 = %d", who, cz, Z / 2);
    const int Mx = 2 * cx, My = 2 * cy, Mz = 2 * cz;
    const size_t hr = (size_t)X * Y * Z * sizeof(float), lr = (size_t)nvol * Mx * My * Mz * sizeof(float);
    struct Range { const char* name; const void* p; size_t bytes; };
    const Range ins[4] = {{"vel", vel, nvol * hr}, {"mag", mag, hr}, {"params", params, (size_t)nvol * 4 * sizeof(float)}, {"noise", noise, lr}};
    const Range outs[3] = {{"out_vel", out_vel, lr}, {"out_mag", out_mag, lr}, {"sigma_out", sigma_out, (size_t)nvol * sizeof(float)}};
    for (const Range& o : outs)
        for (const Range& i : ins) {
            const uintptr_t o0 = (uintptr_t)o.p, i0 = (uintptr_t)i.p;
            FDN_REQUIRE(!o.p || !i.p || o0 + o.bytes <= i0 || i0 + i.bytes <= o0, "%s: %s overlaps %s", who, o.name, i.name);
        }
    FDN_REQUIRE((uintptr_t)out_vel + lr <= (uintptr_t)out_mag || (uintptr_t)out_mag + lr <= (uintptr_t)out_vel,
                "%s: out_vel overlaps out_mag", who);

    const KsLayout l = ks_layout(nvol, Y, Z, cx, cy);
    float2* A = (float2*)((char*)workspace + l.a);
    float2* B = (float2*)((char*)workspace + l.b);
    float* partials = (float*)((char*)workspace + l.partials);
    float* sums = (float*)((char*)workspace + l.sums);
    KspaceGeom g{};
    g.params = params; g.sums = sums; g.seed = seed; g.stream_id = stream_id;
    g.count = (float)((int64_t)Mx * My * Mz);
    g.ratio = (float)((double)Mx * My * Mz / ((double)X * Y * Z));
    // stage: axis extents N -> M, crop c, outer x inner lines, operands (KspaceGeom)
    struct Stage { int mode, N, M, c, outer, inner; const void* in0; const float* in1; void* out0; float* out1; int first, last; };
    const Stage st[6] = {{5, X, Mx, cx, 1, Y * Z, vel, mag, A, nullptr, 1, 0},
                         {5, Y, My, cy, Mx, Z, A, nullptr, B, nullptr, 0, 0},
                         {5, Z, Mz, cz, Mx * My, 1, B, nullptr, A, partials, 0, 1},
                         {6, Mx, Mx, 0, 1, My * Mz, A, noise, B, sigma_out, 1, 0},
                         {6, My, My, 0, Mx, Mz, B, nullptr, A, nullptr, 0, 0},
                         {6, Mz, Mz, 0, Mx * My, 1, A, nullptr, out_vel, out_mag, 0, 1}};
    for (const Stage& s : st) {
        g.N = s.N; g.M = s.M; g.c = s.c; g.outer = s.outer; g.inner = s.inner; g.in0 = s.in0; g.in1 = s.in1; g.out0 = s.out0; g.out1 = s.out1;
        g.first = s.first; g.last = s.last;
        const unsigned nb = ks_blocks((int64_t)s.outer * s.M * s.inner);
        const unsigned lds = (unsigned)(2 * s.N + 4) * sizeof(float);
        hipLaunchKernelGGL(gather_patches_kernel, dim3(nb, (unsigned)nvol), dim3(256), lds, (hipStream_t)stream, (const PatchDesc*)nullptr,
                           (float*)nullptr, nvol, 0, s.mode, StitchGeom{}, g);
        FDN_CHECK_LAUNCH("gather_patches_kernel (k-space stage)");
        if (s.mode == 5 && s.last)                          // sum |F|^2 per volume: the partials in a fixed order (sum_partials_kernel)
            for (int v = 0; v < nvol; ++v) {
                const int rc = fdn_sum_partials(partials + (size_t)v * nb, (int)nb, sums + v, stream);
                if (rc != FDN_OK) return rc;
            }
    }
    return FDN_OK;
}

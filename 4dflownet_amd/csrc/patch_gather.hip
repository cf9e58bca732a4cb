// Patches on the device, in both directions, one kernel per job.
// Into the network: the per-sample work of PatchHandler3D.load_patches_from_index_file (src/Network/PatchHandler3D.py:49-160) -- slice a
// P^3 (or (PR)^3) patch out of a resident 4-D volume, np.rot90 it in one of three planes, flip the sign of a velocity component, divide
// by venc / 4095, or threshold the mask -- as ONE gather launch per output tensor, driven by a small descriptor table built from the CSV
// rows (gather_patches_kernel).  HBM-bound and tiny (2.1 MB per sample); its purpose is to take h5py + numpy slicing + H2D copies off the
// step's critical path when training from real data.
// Out of it, for inference (src/Network/PatchGenerator.py:116-154, src/predictor.py:67-115): the cores of predicted patches stitched into
// a volume (stitch_patches_kernel), packed for another rank (pack_patch_cores_kernel), blended where they overlap (blend_patches_kernel),
// the accumulated volume finished (finish_volume_kernel), and the self-ensemble's fan-in (unrotate_accumulate_kernel).
// Every kernel: 256 threads, one element per thread and step, the grid of stream_blocks().
#include "fdn_common.h"

struct PatchDesc {          // one per (sample, output tensor); mirrored by data_device.py (8 x int64)
    const float* src;       // volume base, layout (T, X, Y, Z)
    int32_t X, Y;
    int32_t Z, t;
    int32_t x0, y0;
    int32_t z0, plane;      // plane 0 = no rotation, 1:(0,1) 2:(0,2) 3:(1,2)  (np.rot90 axes)
    int32_t k, mode;        // k = rot90 count (1..3); mode 0 = sign * (v / div), 1 = (v >= thr) ? 1 : 0
    float sign, div;        // div = venc or 4095; thr is passed in `div` for mode 1
};

// Where the patches of a stitching or blending call land: global patches g0 .. g0 + B of frames of nx*ny*nz patches each (k fastest),
// in a volume (F,3,Xo,Yo,Zo).
struct PatchGrid {
    int64_t g0;
    int32_t Xo, Yo, Zo;
    int32_t nx, ny, nz;
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

// d = (double)p * venc_f, +0.0 where |d| < threshold_f, {venc_f, threshold_f} = scale[2f], scale[2f + 1] (src/predictor.py:103-107,
// src/utils/ImageDataset.py:31)
__device__ __forceinline__ double finish_value(float p, const double* __restrict__ scale, int64_t f) {
    double d = (double)p * scale[2 * f];                                // de-normalise (:103)
    if (fabs(d) < scale[2 * f + 1]) d = 0.0;                            // strict: a product equal to the threshold stays (:104-107)
    return d;
}

// fdn_gather_patches: B patches of S^3 voxels, out = (B,S,S,S)
__global__ __launch_bounds__(256) void gather_patches_kernel(const PatchDesc* __restrict__ desc, float* __restrict__ out, int B, int S) {
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

// Element i of the cores of B patches (B,cs,cs,cs,3), cs = S - 2*side: its patch n, its place (a,b,c) in the core and its component;
// returns its offset in pred = (B,S,S,S,3).  The walk stitch_patches_kernel and pack_patch_cores_kernel share.
__device__ __forceinline__ int64_t core_element(int64_t i, int S, int side, int64_t& n, int& a, int& b, int& c, int& comp) {
    const int cs = S - 2 * side;                                        // core edge
    const int64_t per = (int64_t)cs * cs * cs * 3;
    n = i / per;
    int r = (int)(i - n * per);
    a = r / (cs * cs * 3); r -= a * cs * cs * 3;
    b = r / (cs * 3); r -= b * cs * 3;
    c = r / 3; comp = r - c * 3;
    return (((n * S + side + a) * S + side + b) * S + side + c) * 3 + comp;
}

// fdn_stitch_patches (FINISH = false, out fp32) and fdn_stitch_patches_finish (FINISH = true, out float64, every value through
// finish_value on the way): the core of every predicted patch (B,S,S,S,3) goes to out = (F,3,Xo,Yo,Zo) at patch coordinate * core, voxels
// beyond the extents (the cropped far pad) are dropped.  Reads are contiguous, writes of different patches disjoint.
template <bool FINISH>
__global__ __launch_bounds__(256) void stitch_patches_kernel(const float* __restrict__ pred, void* __restrict__ out,
                                                              const double* __restrict__ scale, int B, int S, int side, PatchGrid pg) {
    const int cs = S - 2 * side;
    const int64_t total = (int64_t)cs * cs * cs * 3 * B;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t n;
        int a, b, c, comp;
        const int64_t src = core_element(i, S, side, n, a, b, c, comp);
        int64_t g = pg.g0 + n;
        const int pk = (int)(g % pg.nz); g /= pg.nz;
        const int pj = (int)(g % pg.ny); g /= pg.ny;
        const int pi = (int)(g % pg.nx);
        const int64_t f = g / pg.nx;
        const int64_t x = (int64_t)pi * cs + a, y = (int64_t)pj * cs + b, z = (int64_t)pk * cs + c;
        if (x >= pg.Xo || y >= pg.Yo || z >= pg.Zo) continue;
        const float v = pred[src];
        const int64_t dst = (((f * 3 + comp) * pg.Xo + x) * pg.Yo + y) * pg.Zo + z;
        if constexpr (FINISH) ((double*)out)[dst] = finish_value(v, scale, f);
        else ((float*)out)[dst] = v;
    }
}

// fdn_pack_patch_cores: the cores alone, contiguous, out = (B,cs,cs,cs,3) -- what a data-parallel rank sends to the rank that stitches
// (out[i] is the element stitch_patches_kernel would place).
__global__ __launch_bounds__(256) void pack_patch_cores_kernel(const float* __restrict__ pred, float* __restrict__ out, int B, int S,
                                                                int side) {
    const int cs = S - 2 * side;
    const int64_t total = (int64_t)cs * cs * cs * 3 * B;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t n;
        int a, b, c, comp;
        out[i] = pred[core_element(i, S, side, n, a, b, c, comp)];
    }
}

// fdn_unrotate_accumulate: the self-ensemble's fan-in.  `pred` holds B predictions (B,S,S,S,3) of patches that were fed in a rotated
// frame (PatchHandler3D.apply_rotation, src/Network/PatchHandler3D.py:97-108,166-274); every element of out = (B,S,S,S,3) takes
// t = sign * pred[n][rho(a,b,c)][comp'] -- orient is the INVERSE fdn_orient_word -- then v = first ? t : out + t, and on the last
// orientation v / (float)divisor.  One IEEE add and one correctly rounded divide; it walks the destination, so writes are contiguous
// (reads are strided for planes 2 and 3) and no two threads meet.
__global__ __launch_bounds__(256) void unrotate_accumulate_kernel(const float* __restrict__ pred, float* __restrict__ out, int B, int S,
                                                                   int orient, int first, int divisor) {
    const int64_t per = (int64_t)S * S * S * 3;
    const int64_t total = per * B;
    const float div = (float)divisor;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / per;
        int r = (int)(i - n * per);
        int a = r / (S * S * 3); r -= a * S * S * 3;
        int b = r / (S * 3); r -= b * S * 3;
        int c = r / 3;
        const int comp = r - c * 3;
        fdn_rot_source(orient, S, a, b, c);
        const int sc = comp == 0 ? fdn_orient_src(orient, 0) : comp == 1 ? fdn_orient_src(orient, 1) : fdn_orient_src(orient, 2);
        const float sgn = comp == 0 ? fdn_orient_sign(orient, 0) : comp == 1 ? fdn_orient_sign(orient, 1) : fdn_orient_sign(orient, 2);
        const float t = sgn * pred[(((n * S + a) * S + b) * S + c) * 3 + sc];
        const float v = first ? t : out[i] + t;
        out[i] = divisor > 1 ? v / div : v;
    }
}

// The slab of the destination one fdn_blend_patches call can touch: frames f0 .. f0 + nf - 1, rows x0 .. x0 + xs - 1.
struct BlendSlab {
    int32_t f0, nf, x0, xs;
};

// fdn_blend_patches: overlap-add stitching.  The cores advance by stride < core HR voxels, so up to two cores per axis -- eight per
// voxel -- cover an output voxel, each with the separable linear ramp of blend_weight.  The DESTINATION is walked: the slab, one (voxel,
// component) per thread and step.  The thread finds the covering patches from its coordinates, keeps those inside [g0, g0 + B) and adds
// them in ascending g: acc = acc + fl(w * p), the multiply and the add rounded separately (blend_add).  No atomics, no two threads on
// one voxel, and the bits do not depend on how the patch list is cut into calls that come in ascending g0.
__global__ __launch_bounds__(256) void blend_patches_kernel(const float* __restrict__ pred, float* __restrict__ out, int B, int S, int side,
                                                             int stride, PatchGrid pg, BlendSlab sl) {
    const int cs = S - 2 * side, sh = stride, r = cs - sh;
    const int64_t yz = (int64_t)pg.Yo * pg.Zo;
    const int64_t per = 3 * sl.xs * yz;                                  // one frame of the slab
    const int64_t total = per * sl.nf;
    const int64_t g1 = pg.g0 + B;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t fl = i / per;
        int64_t q = i - fl * per;
        const int comp = (int)(q / (sl.xs * yz)); q -= comp * (sl.xs * yz);
        const int xl = (int)(q / yz); q -= xl * yz;
        const int y = (int)(q / pg.Zo), z = (int)(q - (int64_t)y * pg.Zo);
        const int x = sl.x0 + xl;
        const int64_t f = sl.f0 + fl;
        // per axis: the last patch that starts at or before the voxel, and the one before it where its core still reaches the voxel
        const int i1 = min(x / sh, pg.nx - 1), j1 = min(y / sh, pg.ny - 1), k1 = min(z / sh, pg.nz - 1);
        const int i0 = (i1 > 0 && x - (i1 - 1) * sh < cs) ? i1 - 1 : i1;
        const int j0 = (j1 > 0 && y - (j1 - 1) * sh < cs) ? j1 - 1 : j1;
        const int k0 = (k1 > 0 && z - (k1 - 1) * sh < cs) ? k1 - 1 : k1;
        const int64_t dst = (((f * 3 + comp) * pg.Xo + x) * pg.Yo + y) * pg.Zo + z;
        float v = 0.f;
        bool touched = false;
        for (int pi = i0; pi <= i1; ++pi)
            for (int pj = j0; pj <= j1; ++pj)
                for (int pk = k0; pk <= k1; ++pk) {                      // ascending g
                    const int64_t g = ((f * pg.nx + pi) * pg.ny + pj) * pg.nz + pk;
                    if (g < pg.g0 || g >= g1) continue;
                    const int a = x - pi * sh, b = y - pj * sh, c = z - pk * sh;
                    const float w = blend_weight(pi, pg.nx, a, cs, r) * blend_weight(pj, pg.ny, b, cs, r) *
                                    blend_weight(pk, pg.nz, c, cs, r);               // fl(fl(wx * wy) * wz)
                    const int64_t n = g - pg.g0;
                    const float p = pred[(((n * S + side + a) * S + side + b) * S + side + c) * 3 + comp];
                    if (!touched) { v = out[dst]; touched = true; }
                    v = blend_add(v, w, p);
                }
        if (touched) out[dst] = v;
    }
}

// fdn_finish_volume: finish_value on an accumulated fp32 volume, acc (F,3,Xo,Yo,Zo) -> out float64 of the same shape; per = 3*Xo*Yo*Zo.
__global__ __launch_bounds__(256) void finish_volume_kernel(const float* __restrict__ acc, double* __restrict__ out,
                                                             const double* __restrict__ scale, int F, int64_t per) {
    const int64_t total = per * F;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = finish_value(acc[i], scale, i / per);
}

// the grid of every kernel here: one element per thread, at most 4096 workgroups that stride over the rest
static dim3 stream_blocks(int64_t total) {
    const int64_t nb = (total + 255) / 256;
    return dim3((unsigned)(nb > 4096 ? 4096 : nb));
}

extern "C" int fdn_gather_patches(const void* desc, float* out, int B, int S, void* stream) {
    FDN_REQUIRE(desc && out && B > 0 && S > 0, "fdn_gather_patches: bad argument");
    hipLaunchKernelGGL(gather_patches_kernel, stream_blocks((int64_t)B * S * S * S), dim3(256), 0, (hipStream_t)stream,
                       (const PatchDesc*)desc, out, B, S);
    FDN_CHECK_LAUNCH("gather_patches_kernel");
    return FDN_OK;
}

// the argument checks fdn_stitch_patches, fdn_stitch_patches_finish and fdn_blend_patches share: operands, patch edge, grid and range
static int check_patch_call(const char* who, bool operands, int F, int S, int side, int nx, int ny, int nz, int64_t g0, int count) {
    FDN_REQUIRE(operands, "%s: NULL argument", who);
    FDN_REQUIRE(side >= 0 && S > 2 * side && S <= 512, "%s: S=%d must exceed 2*side (side=%d) and not 512", who, S, side);
    FDN_REQUIRE(F > 0 && nx > 0 && ny > 0 && nz > 0, "%s: bad frame / patch counts (F=%d, %d,%d,%d)", who, F, nx, ny, nz);
    FDN_REQUIRE(count > 0, "%s: count=%d", who, count);
    FDN_REQUIRE(g0 >= 0, "%s: g0=%lld", who, (long long)g0);
    FDN_REQUIRE(g0 + count <= (int64_t)F * nx * ny * nz, "%s: patches [%lld, %lld) exceed F*nx*ny*nz = %lld", who,
                (long long)g0, (long long)(g0 + count), (long long)((int64_t)F * nx * ny * nz));
    return FDN_OK;
}

// argument checks and launch shared by fdn_stitch_patches (scale == nullptr) and fdn_stitch_patches_finish
template <bool FINISH>
static int stitch_launch(const char* who, const float* pred, void* vol, const double* scale, int F, int Xo, int Yo, int Zo, int S,
                         int side, int nx, int ny, int nz, int64_t g0, int count, void* stream) {
    if (int rc = check_patch_call(who, pred && vol && (!FINISH || scale), F, S, side, nx, ny, nz, g0, count)) return rc;
    const int64_t cs = S - 2 * side;
    FDN_REQUIRE(Xo > 0 && Yo > 0 && Zo > 0 && Xo <= nx * cs && Yo <= ny * cs && Zo <= nz * cs,
                "%s: output extents (%d,%d,%d) must be in 1..n*(S-2*side) = (%lld,%lld,%lld)", who, Xo, Yo, Zo,
                (long long)(nx * cs), (long long)(ny * cs), (long long)(nz * cs));
    hipLaunchKernelGGL(stitch_patches_kernel<FINISH>, stream_blocks((int64_t)count * cs * cs * cs * 3), dim3(256), 0, (hipStream_t)stream,
                       pred, vol, scale, count, S, side, PatchGrid{g0, Xo, Yo, Zo, nx, ny, nz});
    FDN_CHECK_LAUNCH("stitch_patches_kernel");
    return FDN_OK;
}

extern "C" int fdn_stitch_patches(const float* pred, float* vol, int F, int Xo, int Yo, int Zo, int S, int side, int nx, int ny, int nz,
                                  int64_t g0, int count, void* stream) {
    return stitch_launch<false>("fdn_stitch_patches", pred, vol, nullptr, F, Xo, Yo, Zo, S, side, nx, ny, nz, g0, count, stream);
}

extern "C" int fdn_stitch_patches_finish(const float* pred, double* vol, const double* frame_scale, int F, int Xo, int Yo, int Zo, int S,
                                         int side, int nx, int ny, int nz, int64_t g0, int count, void* stream) {
    return stitch_launch<true>("fdn_stitch_patches_finish", pred, vol, frame_scale, F, Xo, Yo, Zo, S, side, nx, ny, nz, g0, count, stream);
}

extern "C" int fdn_blend_patches(const float* pred, float* acc, int F, int Xo, int Yo, int Zo, int S, int side, int stride_hr, int nx,
                                 int ny, int nz, int64_t g0, int count, void* stream) {
    const char* who = "fdn_blend_patches";
    if (int rc = check_patch_call(who, pred && acc, F, S, side, nx, ny, nz, g0, count)) return rc;
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
    const BlendSlab sl{(int32_t)f0, (int32_t)(f1 - f0 + 1), (int32_t)x0, (int32_t)(x1 - x0)};
    hipLaunchKernelGGL(blend_patches_kernel, stream_blocks((int64_t)sl.nf * 3 * sl.xs * Yo * Zo), dim3(256), 0, (hipStream_t)stream, pred,
                       acc, count, S, side, stride_hr, PatchGrid{g0, Xo, Yo, Zo, nx, ny, nz}, sl);
    FDN_CHECK_LAUNCH("blend_patches_kernel");
    return FDN_OK;
}

extern "C" int fdn_finish_volume(const float* acc, double* vol, const double* frame_scale, int F, int Xo, int Yo, int Zo, void* stream) {
    const char* who = "fdn_finish_volume";
    FDN_REQUIRE(acc && vol && frame_scale, "%s: NULL argument", who);
    FDN_REQUIRE(F > 0 && Xo > 0 && Yo > 0 && Zo > 0, "%s: bad volume (F=%d, %d,%d,%d)", who, F, Xo, Yo, Zo);
    const int64_t per = (int64_t)3 * Xo * Yo * Zo;
    hipLaunchKernelGGL(finish_volume_kernel, stream_blocks(per * F), dim3(256), 0, (hipStream_t)stream, acc, vol, frame_scale, F, per);
    FDN_CHECK_LAUNCH("finish_volume_kernel");
    return FDN_OK;
}

extern "C" int fdn_pack_patch_cores(const float* pred, float* cores, int S, int side, int count, void* stream) {
    FDN_REQUIRE(pred && cores, "fdn_pack_patch_cores: NULL argument");
    FDN_REQUIRE(side >= 0 && S > 2 * side && S <= 512, "fdn_pack_patch_cores: S=%d must exceed 2*side (side=%d) and not 512", S, side);
    FDN_REQUIRE(count > 0, "fdn_pack_patch_cores: count=%d", count);
    const int64_t cs = S - 2 * side;
    hipLaunchKernelGGL(pack_patch_cores_kernel, stream_blocks((int64_t)count * cs * cs * cs * 3), dim3(256), 0, (hipStream_t)stream, pred,
                       cores, count, S, side);
    FDN_CHECK_LAUNCH("pack_patch_cores_kernel");
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
    hipLaunchKernelGGL(unrotate_accumulate_kernel, stream_blocks(total), dim3(256), 0, (hipStream_t)stream, pred, acc, count, S, word, first,
                       divisor);
    FDN_CHECK_LAUNCH("unrotate_accumulate_kernel");
    return FDN_OK;
}

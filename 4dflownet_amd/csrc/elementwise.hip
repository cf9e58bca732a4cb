// HBM-bound pieces of the train step: input features, halo fold (MirrorPadGrad) fused with gradient fan-in and
// activation gradient, trilinear upsample fwd/bwd, masked-MSE loss + relative-error metric + dPred, L2 sum, Adam.
// All of them stream 16-B vectors with 16 lanes per 256-B channel row.
#include "fdn_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// src/Network/SR4DFlowNet.py:10-15
// ---------------------------------------------------------------------------------------------
// sqrt(a*a + b*b + c*c) with its roundings spelled out -- one product rounded, the other two fused, the way this kernel has always been
// compiled.  Left to the compiler the choice of which products are fused follows the surrounding code (it changed when the loads
// moved into two branches), and results must not depend on that.
__device__ __forceinline__ float norm3(float a, float b, float c) {
    return sqrtf(__builtin_fmaf(c, c, __builtin_fmaf(a, a, b * b)));
}

// fdn_input_features: the six inputs of voxel i are u[i] .. mw[i].
template <typename T>
__global__ void input_features_kernel(const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ w,
                                      const float* __restrict__ mu, const float* __restrict__ mv,
                                      const float* __restrict__ mw, T* __restrict__ phase, T* __restrict__ pc, int64_t nvox) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) {
        const float a = u[i], b = v[i], c = w[i];
        const float ma = mu[i], mb = mv[i], mc = mw[i];
        const float speed = norm3(a, b, c);
        const float mag = norm3(ma, mb, mc);
        fdn_st1(phase + i * 3 + 0, a); fdn_st1(phase + i * 3 + 1, b); fdn_st1(phase + i * 3 + 2, c);
        fdn_st1(pc + i * 3 + 0, mag * speed); fdn_st1(pc + i * 3 + 1, mag); fdn_st1(pc + i * 3 + 2, speed);
    }
}

// Sliding-window geometry of fdn_input_features_volume (src/Network/PatchGenerator.py:13-40,53-86): the six inputs of output voxel i
// are gathered from resident frames (F,6,X,Y,Z) -- patch g0 + i / P^3 of the window at `stride`, shifted by the 2-voxel side pad, zero
// outside the volume.
// orient != 0 (fdn_input_features_volume_oriented, an fdn_orient_word): the features of the patch as PatchHandler3D.apply_rotation
// (src/Network/PatchHandler3D.py:97-108,166-274) would turn it -- voxel (a,b,c) reads the window voxel np.rot90 puts there, the zero
// fill comes first, then the components are permuted and signed by multiplication (a padded zero under a negative sign is -0.0, as on
// the host), and norm3 takes the permuted components in their new order.  0: the plain window.
// stride: voxels the window advances by, P - 4 for the plain tiler and less for overlapping cores (fdn_input_features_volume_strided).
struct InputGeom {
    int32_t P, X, Y, Z;
    int32_t nx, ny, nz, orient;
    int64_t g0;
    int32_t stride;
};

template <typename T>
__global__ void input_features_volume_kernel(const float* __restrict__ frames, T* __restrict__ phase, T* __restrict__ pc, int64_t nvox,
                                             InputGeom geo) {
    const int P = geo.P, E = geo.stride;
    const int64_t per = (int64_t)P * P * P, plane = (int64_t)geo.X * geo.Y * geo.Z;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / per;                       // patch of this launch
        int r = (int)(i - n * per);                      // voxel of the patch, z fastest
        int pa = r / (P * P); r -= pa * P * P;
        int pb = r / P, pcz = r - pb * P;
        int64_t g = geo.g0 + n;                          // global patch: frame, then (i, j, k) with k fastest
        const int pk = (int)(g % geo.nz); g /= geo.nz;
        const int pj = (int)(g % geo.ny); g /= geo.ny;
        const int pi = (int)(g % geo.nx);
        const int64_t f = g / geo.nx;
        if (geo.orient) fdn_rot_source(geo.orient, P, pa, pb, pcz);
        const int x = pi * E + pa - 2, y = pj * E + pb - 2, z = pk * E + pcz - 2;
        float a = 0.f, b = 0.f, c = 0.f, ma = 0.f, mb = 0.f, mc = 0.f;
        if (x >= 0 && x < geo.X && y >= 0 && y < geo.Y && z >= 0 && z < geo.Z) {
            const float* s = frames + f * 6 * plane + ((int64_t)x * geo.Y + y) * geo.Z + z;
            a = s[0]; b = s[plane]; c = s[2 * plane];
            ma = s[3 * plane]; mb = s[4 * plane]; mc = s[5 * plane];
        }
        if (geo.orient) {
            const int s0 = fdn_orient_src(geo.orient, 0), s1 = fdn_orient_src(geo.orient, 1), s2 = fdn_orient_src(geo.orient, 2);
            const float a0 = a, b0 = b, c0 = c, ma0 = ma, mb0 = mb, mc0 = mc;
            a = (s0 == 0 ? a0 : s0 == 1 ? b0 : c0) * fdn_orient_sign(geo.orient, 0);
            b = (s1 == 0 ? a0 : s1 == 1 ? b0 : c0) * fdn_orient_sign(geo.orient, 1);
            c = (s2 == 0 ? a0 : s2 == 1 ? b0 : c0) * fdn_orient_sign(geo.orient, 2);
            ma = s0 == 0 ? ma0 : s0 == 1 ? mb0 : mc0;
            mb = s1 == 0 ? ma0 : s1 == 1 ? mb0 : mc0;
            mc = s2 == 0 ? ma0 : s2 == 1 ? mb0 : mc0;
        }
        const float speed = norm3(a, b, c);
        const float mag = norm3(ma, mb, mc);
        fdn_st1(phase + i * 3 + 0, a); fdn_st1(phase + i * 3 + 1, b); fdn_st1(phase + i * 3 + 2, c);
        fdn_st1(pc + i * 3 + 0, mag * speed); fdn_st1(pc + i * 3 + 1, mag); fdn_st1(pc + i * 3 + 2, speed);
    }
}

// ---------------------------------------------------------------------------------------------
// fold: adjoint of the SYMMETRIC p=1 pad (MirrorPadGrad) + fan-in of up to 3 padded gradients + skip + act'
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fold_halo_kernel(const float* __restrict__ s0, const float* __restrict__ s1,
                                                         const float* __restrict__ s2, int nsrc,
                                                         const float* __restrict__ skip, const float* __restrict__ yprev,
                                                         int act, float alpha, float* __restrict__ out, int N, int D, int H,
                                                         int W, int C4) {
    const int64_t total = (int64_t)N * D * H * W * C4;
    const int PH = H + 2, PW = W + 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        int64_t v = i / C4;
        const int w = (int)(v % W); v /= W;
        const int h = (int)(v % H); v /= H;
        const int d = (int)(v % D);
        const int n = (int)(v / D);
        // padded indices that clamp onto (d,h,w): p = i+1, plus 0 when i==0, plus dim+1 when i==dim-1
        int pd[3], ph[3], pw[3];
        int nd = 0, nh = 0, nw = 0;
        pd[nd++] = d + 1; if (d == 0) pd[nd++] = 0; if (d == D - 1) pd[nd++] = D + 1;
        ph[nh++] = h + 1; if (h == 0) ph[nh++] = 0; if (h == H - 1) ph[nh++] = H + 1;
        pw[nw++] = w + 1; if (w == 0) pw[nw++] = 0; if (w == W - 1) pw[nw++] = W + 1;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < nd; ++a)
            for (int b = 0; b < nh; ++b)
                for (int c = 0; c < nw; ++c) {
                    const int64_t off = (((((int64_t)n * (D + 2) + pd[a]) * PH + ph[b]) * PW + pw[c]) * C4 + c4);
                    acc += ((const f32x4*)s0)[off];
                    if (nsrc > 1) acc += ((const f32x4*)s1)[off];
                    if (nsrc > 2) acc += ((const f32x4*)s2)[off];
                }
        if (skip) acc += ((const f32x4*)skip)[i];
        if (yprev) {
            const f32x4 y = ((const f32x4*)yprev)[i];
            acc.x *= fdn_act_grad(y.x, act, alpha); acc.y *= fdn_act_grad(y.y, act, alpha);
            acc.z *= fdn_act_grad(y.z, act, alpha); acc.w *= fdn_act_grad(y.w, act, alpha);
        }
        ((f32x4*)out)[i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// upsample3d (src/Network/SR4DFlowNet.py:53-90): trilinear, align_corners=True.
// coefficient rule of tf resize_bilinear(align_corners): in = out * scale (fp32), scale = (n-1)/(nR-1).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void lerp_coeff(int o, float scale, int n, int& lo, int& hi, float& f) {
    const float src = (float)o * scale;
    const float fl = floorf(src);
    lo = (int)fl;
    hi = min(lo + 1, n - 1);
    f = src - fl;
}

// block = one output row (n, od, oh): the d / h interpolation coefficients are block-uniform; thread = one 16-B vector
// (4 fp32 / 8 bf16 channels) of one output voxel, consecutive threads write consecutive vectors (32-bit index math only).
// STAGED (round 6): the four input rows (d0|d1, h0|h1) of the output row go through LDS once, as coalesced 16-B loads, and the
// eight corner vectors of every output vector come from there -- the direct form asks the vector cache for eight 16-B loads per
// 16 B written (1.8 GB of L1 traffic for the 226 MB of the cfg2 upsample: L1-bound at 0.078 ms, 2.9 TB/s written); same
// arithmetic in the same order, bit-identical.  Rows too long for the LDS take the direct form.
template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void upsample_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int D,
                                                            int H, int W, int CV, int R, float sd, float sh, float sw) {
    constexpr int E = FdnVec<T>::E;
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];      // STAGED: [4][W * CV] 16-B vectors
    const int OD = D * R, OH = H * R, OW = W * R;
    for (int row = blockIdx.x; row < N * OD * OH; row += gridDim.x) {
        const int oh = row % OH;
        const int t = row / OH;
        const int od = t % OD, n = t / OD;
        int d0, d1, h0, h1;
        float fd, fh;
        lerp_coeff(od, sd, D, d0, d1, fd);
        lerp_coeff(oh, sh, H, h0, h1, fh);
        const T* r00 = x + (((int64_t)n * D + d0) * H + h0) * W * CV * E;
        const T* r01 = x + (((int64_t)n * D + d0) * H + h1) * W * CV * E;
        const T* r10 = x + (((int64_t)n * D + d1) * H + h0) * W * CV * E;
        const T* r11 = x + (((int64_t)n * D + d1) * H + h1) * W * CV * E;
        if constexpr (STAGED) {
            const int nv = W * CV;
            __syncthreads();                               // the previous row's corner reads are done
            f32x4* dst = (f32x4*)rowbuf;
            for (int i = threadIdx.x; i < nv; i += blockDim.x) {
                const f32x4 a = ((const f32x4*)r00)[i], b = ((const f32x4*)r01)[i], c = ((const f32x4*)r10)[i], d = ((const f32x4*)r11)[i];
                dst[i] = a; dst[nv + i] = b; dst[2 * nv + i] = c; dst[3 * nv + i] = d;
            }
            __syncthreads();
            r00 = (const T*)rowbuf; r01 = r00 + nv * E; r10 = r01 + nv * E; r11 = r10 + nv * E;
        }
        T* yr = y + (int64_t)row * OW * CV * E;
        for (int i = threadIdx.x; i < OW * CV; i += blockDim.x) {
            const int ow = i / CV, cv = i - ow * CV;
            int w0, w1;
            float fw;
            lerp_coeff(ow, sw, W, w0, w1, fw);
            const int o0 = (w0 * CV + cv) * E, o1 = (w1 * CV + cv) * E;
            float c000[E], c001[E], c010[E], c011[E], c100[E], c101[E], c110[E], c111[E];
            FdnVec<T>::ld(r00 + o0, c000); FdnVec<T>::ld(r00 + o1, c001);
            FdnVec<T>::ld(r01 + o0, c010); FdnVec<T>::ld(r01 + o1, c011);
            FdnVec<T>::ld(r10 + o0, c100); FdnVec<T>::ld(r10 + o1, c101);
            FdnVec<T>::ld(r11 + o0, c110); FdnVec<T>::ld(r11 + o1, c111);
            // innermost (z) first, then y, then x -- the order of the reference's two resize passes
            float o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float a0 = c000[e] + (c001[e] - c000[e]) * fw, a1 = c010[e] + (c011[e] - c010[e]) * fw;
                const float b0 = c100[e] + (c101[e] - c100[e]) * fw, b1 = c110[e] + (c111[e] - c110[e]) * fw;
                const float aa = a0 + (a1 - a0) * fh, bb = b0 + (b1 - b0) * fh;
                o[e] = aa + (bb - aa) * fd;
            }
            FdnVec<T>::st(yr + (int64_t)i * E, o);
        }
    }
}

// weight of output index o on input index i along one axis (0 if o does not touch i)
__device__ __forceinline__ float axis_weight(int o, int i, float scale, int n) {
    int lo, hi;
    float f;
    lerp_coeff(o, scale, n, lo, hi, f);
    float wgt = 0.f;
    if (lo == i) wgt += 1.f - f;
    if (hi == i) wgt += f;
    return wgt;
}

// candidate output range [o0,o1] that can touch input i: o*scale in (i-1, i+1)
__device__ __forceinline__ void axis_range(int i, float inv_scale, int m, int& o0, int& o1) {
    o0 = max(0, (int)floorf((float)(i - 1) * inv_scale) - 1);
    o1 = min(m - 1, (int)ceilf((float)(i + 1) * inv_scale) + 1);
}

// Adjoint of the trilinear upsample, block = HB consecutive LOW-res rows (n, d, h0 .. h0 + HB - 1).  Phase A folds the high-res rows
// that touch them (block-uniform weights wd * wh per low-res row) into HB high-res-wide rows in LDS: coalesced 16-B reads of dy, eight
// rows requested before the first use, every loaded vector accumulated into all HB rows (weight 0 where it does not touch: exact).  A
// high-res row touches two low-res rows per axis, so with HB = 1 (rounds 1-5) every dy row went through the vector cache four times
// (1 GB of L2 -> L1 traffic for the 226 MB of cfg2: 0.071 ms); with HB = 2 it is three times.  Phase B folds each row along w, applies
// act'(y_prev), stores.  Per low-res row the non-zero terms are added in the same order as before: bit-identical for every HB.
template <typename T, int HB>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ yprev,
                                                            int act, float alpha, T* __restrict__ dx, int N, int D,
                                                            int H, int W, int CV, int R, float sd, float sh, float sw) {
    constexpr int E = FdnVec<T>::E;
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];      // [HB][OW][CV * E]
    constexpr int kCandD = 32, kCandH = 64;                             // candidate rows per axis (host checks R and HB against them)
    constexpr int kUpPairs = HB == 1 ? 1024 : 512;
    __shared__ int s_row[kUpPairs];
    __shared__ float s_wgt[kUpPairs * HB];
    __shared__ int s_od[kCandD], s_oh[kCandH], s_nd, s_nh;
    __shared__ float s_wd[kCandD], s_wh[kCandH * HB];
    const int OD = D * R, OH = H * R, OW = W * R;
    const int C = CV * E;
    const float isd = sd > 0.f ? 1.f / sd : 0.f, ish = sh > 0.f ? 1.f / sh : 0.f, isw = sw > 0.f ? 1.f / sw : 0.f;
    // XCD-aware block order: block ids are dealt round-robin to the 8 XCDs; an XCD takes one contiguous run of low-res row blocks,
    // so the high-res rows shared by neighbouring blocks are fetched into ITS L2 once (plain order: 3.8x dy from HBM)
    const int nhblk = (H + HB - 1) / HB;
    const int nrows = N * D * nhblk;
    for (int it = blockIdx.x; it < nrows; it += gridDim.x) {
        const int blk0 = it - (int)blockIdx.x, span = min((int)gridDim.x, nrows - blk0);     // blocks of this sweep
        const int q = span >> 3, rem = span & 7, xc = blockIdx.x & 7;
        const int row = blk0 + xc * q + (xc < rem ? xc : rem) + ((int)blockIdx.x >> 3);
        const int h0 = (row % nhblk) * HB;
        const int nhb = min(HB, H - h0);
        const int t = row / nhblk;
        const int d = t % D, n = t / D;
        int od0, od1, oh0, oh1, tmp;
        axis_range(d, isd, OD, od0, od1);
        axis_range(h0, ish, OH, oh0, tmp);
        axis_range(h0 + nhb - 1, ish, OH, tmp, oh1);
        if (sd == 0.f) { od0 = 0; od1 = OD - 1; }
        if (sh == 0.f) { oh0 = 0; oh1 = OH - 1; }
        __syncthreads();                                   // rowbuf and the pair list of the previous block fully consumed
        // The high-res rows (od, oh) with a non-zero weight on one of these low-res rows, as a compact block-uniform list: the fold
        // below then has no data-dependent branch around its loads (a `continue` per candidate row made every load its own round
        // trip: 103 us for 280 MB at cfg2).  Wave 0: the depth candidates od0.. (lanes 0..31), wave 1: the height candidates oh0..;
        // ballot + prefix count compacts the ones with a non-zero weight in index order (deterministic).
        if (threadIdx.x < 128) {
            const int lane = threadIdx.x & 63;
            const bool dl = threadIdx.x < 64;
            const int c = dl ? od0 + lane : oh0 + lane;
            float wgt[HB];
            bool any = false;
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) {
                wgt[hb] = 0.f;
                if (dl) { if (hb == 0 && lane < kCandD && c <= od1) wgt[0] = axis_weight(c, d, sd, D); }
                else if (hb < nhb && c <= oh1) wgt[hb] = axis_weight(c, h0 + hb, sh, H);
                any = any || wgt[hb] != 0.f;
            }
            const unsigned long long m = __ballot(any);
            if (any) {
                const int pos = __popcll(m & ((1ull << lane) - 1ull));
                if (dl) { s_od[pos] = c; s_wd[pos] = wgt[0]; }
                else {
                    s_oh[pos] = c;
#pragma unroll
                    for (int hb = 0; hb < HB; ++hb) s_wh[pos * HB + hb] = wgt[hb];
                }
            }
            if (lane == 0) { if (dl) s_nd = __popcll(m); else s_nh = __popcll(m); }
        }
        __syncthreads();
        const int nd_ = s_nd, nh_ = s_nh, npairs = nd_ * nh_;
        for (int k = threadIdx.x; k < npairs; k += blockDim.x) {
            const int a = k / nh_, b = k - a * nh_;
            s_row[k] = (n * OD + s_od[a]) * OH + s_oh[b];
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) s_wgt[k * HB + hb] = s_wd[a] * s_wh[b * HB + hb];
        }
        __syncthreads();
        constexpr int U = 8;                               // high-res rows requested before the first use (16 measured slower: 0.070 vs 0.057 ms at cfg2)
        for (int i = threadIdx.x; i < OW * CV; i += blockDim.x) {
            float acc[HB][E];
#pragma unroll
            for (int hb = 0; hb < HB; ++hb)
#pragma unroll
                for (int e = 0; e < E; ++e) acc[hb][e] = 0.f;
            for (int k0 = 0; k0 < npairs; k0 += U) {
                float g[U][E];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = min(k0 + u, npairs - 1);         // tail: re-read the last row with weight 0 (cache hit)
                    FdnVec<T>::ld(dy + ((int64_t)s_row[k] * OW * CV + i) * E, g[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = min(k0 + u, npairs - 1);
#pragma unroll
                    for (int hb = 0; hb < HB; ++hb) {
                        const float wv = k0 + u < npairs ? s_wgt[k * HB + hb] : 0.f;
#pragma unroll
                        for (int e = 0; e < E; ++e) acc[hb][e] += g[u][e] * wv;
                    }
                }
            }
#pragma unroll
            for (int hb = 0; hb < HB; ++hb)
#pragma unroll
                for (int e = 0; e < E; ++e) rowbuf[(hb * OW * CV + i) * E + e] = acc[hb][e];
        }
        __syncthreads();
        for (int j = threadIdx.x; j < nhb * W * CV; j += blockDim.x) {
            const int hb = j / (W * CV), i = j - hb * (W * CV);
            const int w = i / CV, cv = i - w * CV;
            int ow0, ow1;
            axis_range(w, isw, OW, ow0, ow1);
            if (sw == 0.f) { ow0 = 0; ow1 = OW - 1; }
            const float* rb = rowbuf + hb * OW * C;
            float acc[E];
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] = 0.f;
            for (int ow = ow0; ow <= ow1; ++ow) {
                const float ww = axis_weight(ow, w, sw, W);
                if (ww == 0.f) continue;
#pragma unroll
                for (int e = 0; e < E; ++e) acc[e] += rb[ow * C + cv * E + e] * ww;
            }
            const int64_t o = ((((int64_t)n * D + d) * H + h0 + hb) * W * CV + i) * E;
            if (yprev) {
                float yv[E];
                FdnVec<T>::ld(yprev + o, yv);
#pragma unroll
                for (int e = 0; e < E; ++e) acc[e] *= fdn_act_grad(yv[e], act, alpha);
            }
            FdnVec<T>::st(dx + o, acc);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// loss / metric: TrainerController.py:84-127,152-156 ; loss_utils.py:64-103
// scratch layout per sample: [0]=sum mask [1]=sum nonfluid [2]=sum mse*mask [3]=sum mse*nf [4]=sum rel
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int wv = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wv] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += red[k];
    return s;   // valid in thread 0
}

// ---------------------------------------------------------------------------------------------
// Whole-volume evaluation (fdn_volume_metrics): three kernels of its own, each taking a VolumeMetrics by value.  pred (F,3,X,Y,Z) fp32
// or float64, truth (F,3,X,Y,Z), mask (mask_frames,X,Y,Z); everything is summed in double.  part: per-block partials
// (F, gridDim.x, 26), every column written by exactly one pass; volume_finalize_kernel adds them over the blocks in a fixed order.
//   volume_mask_sums_kernel       columns 0-2 (sum m, sum nf, sum fl)
//   volume_metrics_kernel pass 1: columns 3-8 (q, corr, e_c^2)      pass 2: columns 9-10 (d: the pass that gathers the stencil neighbours)
//                     pass 3 + c: columns 11 + 5c .. 15 + 5c (the regression moments of component c over the fl voxels)
// 26 double accumulators are 52 VGPRs; a pass holds at most six of them, and each column is accumulated by the same threads in the
// same order whatever the grouping.
// ---------------------------------------------------------------------------------------------
struct VolumeMetrics {
    const void* pred;
    const float* truth;
    const float* mask;
    double* part;
    double* out;
    int32_t pass, pred_is_f64, per_frame_mask, X, Y, Z;
};

__device__ __forceinline__ double block_sum_d(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int wv = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wv] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += red[k];
    return s;   // valid in thread 0
}

__device__ __forceinline__ double vm_pred(const VolumeMetrics& a, int64_t i) {
    return a.pred_is_f64 ? ((const double*)a.pred)[i] : (double)((const float*)a.pred)[i];
}

// (Da e)[k] = e[clamp(k-1)] - e[clamp(k+1)], e = pred - truth, for the voxel at offset i of a component plane starting at `base`,
// at position p of an axis of extent n and voxel stride s.  Both neighbours stay inside the plane; 0 on an axis of extent 1.
__device__ __forceinline__ double vm_axis_diff(const VolumeMetrics& a, int64_t base, int64_t i, int p, int n, int64_t s) {
    const int64_t lo = base + i - (p > 0 ? s : 0), hi = base + i + (p < n - 1 ? s : 0);
    return (vm_pred(a, lo) - (double)a.truth[lo]) - (vm_pred(a, hi) - (double)a.truth[hi]);
}

__global__ __launch_bounds__(256) void volume_mask_sums_kernel(VolumeMetrics a) {
    __shared__ double red[4];
    const int f = blockIdx.y;
    const int64_t V = (int64_t)a.X * a.Y * a.Z;
    const float* mask = a.mask + (a.per_frame_mask ? (int64_t)f * V : 0);
    double sm = 0.0, snf = 0.0, sfl = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
        const float m = mask[i];
        sm += (double)m;
        snf += m < 0.5f ? 1.0 : 0.0;
        sfl += m == 1.0f ? 1.0 : 0.0;
    }
    const double s0 = block_sum_d(sm, red);
    const double s1 = block_sum_d(snf, red);
    const double s2 = block_sum_d(sfl, red);
    if (threadIdx.x == 0) {
        double* part = a.part + ((size_t)f * gridDim.x + blockIdx.x) * 26;
        part[0] = s0; part[1] = s1; part[2] = s2;
    }
}

__global__ __launch_bounds__(256) void volume_metrics_kernel(VolumeMetrics a) {
    __shared__ double red[4];
    const int f = blockIdx.y;
    const int64_t YZ = (int64_t)a.Y * a.Z, V = (int64_t)a.X * YZ;
    const float* mask = a.mask + (a.per_frame_mask ? (int64_t)f * V : 0);
    double* part = a.part + ((size_t)f * gridDim.x + blockIdx.x) * 26;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (a.pass == 1) {
        const int64_t bu = (int64_t)f * 3 * V, bv = bu + V, bw = bv + V;
        double sqm = 0.0, sqn = 0.0, srel = 0.0, seu = 0.0, sev = 0.0, sew = 0.0;
        for (int64_t i = first; i < V; i += step) {
            const float mf = mask[i];
            const double m = (double)mf;
            const bool nf = mf < 0.5f, fl = mf == 1.0f;
            const double tu = (double)a.truth[bu + i], tv = (double)a.truth[bv + i], tw = (double)a.truth[bw + i];
            const double eu = vm_pred(a, bu + i) - tu, ev = vm_pred(a, bv + i) - tv, ew = vm_pred(a, bw + i) - tw;
            const double qu = eu * eu, qv = ev * ev, qw = ew * ew;
            const double q = qu + qv + qw;
            sqm += q * m;
            sqn += nf ? q : 0.0;
            // relative error (loss_utils.py:64-92) in double; rint == round-half-to-even == tf.round
            const double diff = sqrt(q);
            const double actual = sqrt(tu * tu + tv * tv + tw * tw);
            double rel = diff / (actual + 1e-5);
            rel = fmin(fmax(rel, 0.0), 1.0);
            double corr = actual != 0.0 ? rel : diff;
            corr = rint(corr * 1e4) / 1e4;
            srel += fl ? corr : 0.0;
            seu += fl ? qu : 0.0;
            sev += fl ? qv : 0.0;
            sew += fl ? qw : 0.0;
        }
        const double r3 = block_sum_d(sqm, red), r4 = block_sum_d(sqn, red), r5 = block_sum_d(srel, red);
        const double r6 = block_sum_d(seu, red), r7 = block_sum_d(sev, red), r8 = block_sum_d(sew, red);
        if (threadIdx.x == 0) { part[3] = r3; part[4] = r4; part[5] = r5; part[6] = r6; part[7] = r7; part[8] = r8; }
        return;
    }
    if (a.pass == 2) {                                               // the pass that gathers the stencil neighbours
        const int64_t bu = (int64_t)f * 3 * V, bv = bu + V, bw = bv + V;
        double sdm = 0.0, sdn = 0.0;
        for (int64_t i = first; i < V; i += step) {
            const float mf = mask[i];
            const unsigned iv = (unsigned)i;                       // V < 2^31 (fdn_volume_metrics)
            const unsigned r = iv / (unsigned)a.Z;
            const int pz = (int)(iv - r * (unsigned)a.Z), py = (int)(r % (unsigned)a.Y), px = (int)(r / (unsigned)a.Y);
            const double gu = vm_axis_diff(a, bu, i, px, a.X, YZ);
            const double gv = vm_axis_diff(a, bv, i, py, a.Y, a.Z);
            const double gw = vm_axis_diff(a, bw, i, pz, a.Z, 1);
            const double d = gu * gu + gv * gv + gw * gw;
            sdm += d * (double)mf;
            sdn += mf < 0.5f ? d : 0.0;
        }
        const double r9 = block_sum_d(sdm, red), r10 = block_sum_d(sdn, red);
        if (threadIdx.x == 0) { part[9] = r9; part[10] = r10; }
        return;
    }
    const int c = a.pass - 3;                                       // the regression moments of one component over the fl voxels
    const int64_t base = ((int64_t)f * 3 + c) * V;
    double st = 0.0, sp = 0.0, stt = 0.0, spp = 0.0, stp = 0.0;
    for (int64_t i = first; i < V; i += step) {
        if (mask[i] == 1.0f) {
            const double t = (double)a.truth[base + i], p = vm_pred(a, base + i);
            st += t; sp += p; stt += t * t; spp += p * p; stp += t * p;
        }
    }
    const double r0 = block_sum_d(st, red), r1 = block_sum_d(sp, red), r2 = block_sum_d(stt, red);
    const double r3 = block_sum_d(spp, red), r4 = block_sum_d(stp, red);
    if (threadIdx.x == 0) {
        double* o = part + 11 + 5 * c;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4;
    }
}

// one wave per frame, column by column: lane t adds the partials of blocks t, t + 64, ... in block order, then the shuffle tree
__global__ __launch_bounds__(64) void volume_finalize_kernel(VolumeMetrics a, int nblk) {
    const int f = blockIdx.x;
    const double* part = a.part + (size_t)f * nblk * 26;
    for (int col = 0; col < 26; ++col) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblk; b += 64) s += part[(size_t)b * 26 + col];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (threadIdx.x == 0) a.out[(size_t)f * 26 + col] = s;
    }
}

__global__ __launch_bounds__(256) void mask_sums_kernel(const float* __restrict__ mask, float* __restrict__ scratch, int64_t V) {
    __shared__ float red[4];
    const int n = blockIdx.y;
    float sm = 0.f, snf = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
        const float m = mask[(int64_t)n * V + i];
        sm += m;
        snf += m < 0.5f ? 1.f : 0.f;
    }
    const float a = block_sum(sm, red);
    const float b = block_sum(snf, red);
    if (threadIdx.x == 0) { atomicAdd(&scratch[n * 8 + 0], a); atomicAdd(&scratch[n * 8 + 1], b); }
}

// divergence loss (loss_utils.py:4-62, TrainerController.py:84-127 with lines 111-120 live): along the axis a paired with channel c
// (u: D, v: H, w: W) (Da e)[k] = e[clamp(k-1)] - e[clamp(k+1)], e = pred - truth (the SYMMETRIC pad-1 cross-correlation; the
// difference of the two gradients is the gradient of the difference).  One voxel k at position p of an axis of extent n and
// voxel stride s: returns (Da e)[k] and adds Da^T r to *g, r[j] = two_w * c[j] * (Da e)[j], c[j] = m[j] inv_f + nf[j] inv_nf.
// Da^T r at k: r[k+1] - r[k-1] inside, r[0] + r[1] at k = 0, -(r[n-2] + r[n-1]) at k = n-1, 0 when n = 1.  Every neighbour index
// is clamped into the axis, so every load stays inside the sample.
__device__ __forceinline__ float div_axis(const float* __restrict__ pred, const float* __restrict__ t, const float* __restrict__ mask,
                                          int64_t g, int c, int p, int n, int64_t s, float e0, float c0, float inv_f, float inv_nf,
                                          float two_w, float* gout) {
    const int km2 = max(p - 2, 0), km1 = max(p - 1, 0), kp1 = min(p + 1, n - 1), kp2 = min(p + 2, n - 1);
    auto e = [&](int k) { const int64_t q = g + (int64_t)(k - p) * s; return pred[q * 3 + c] - t[q]; };
    auto cw = [&](int k) { const float m = mask[g + (int64_t)(k - p) * s]; return m * inv_f + (m < 0.5f ? inv_nf : 0.f); };
    const float em2 = e(km2), em1 = e(km1), ep1 = e(kp1), ep2 = e(kp2);
    const float cm1 = cw(km1), cp1 = cw(kp1);
    const float d0 = em1 - ep1;                                     // (Da e)[p]
    const float rm1 = p > 0 ? two_w * cm1 * (em2 - e0) : 0.f;       // r[p-1]: (Da e)[p-1] = e[clamp(p-2)] - e[p]
    const float rp1 = p < n - 1 ? two_w * cp1 * (e0 - ep2) : 0.f;   // r[p+1]: (Da e)[p+1] = e[p] - e[clamp(p+2)]
    const float r0 = two_w * c0 * d0;
    float acc = rp1 - rm1;
    if (p == 0) acc += r0;
    if (p == n - 1) acc -= r0;
    *gout += acc;
    return d0;
}

// fdn_loss_metrics_act, out_act == FDN_ACT_TANH: pred = tanh(z) of the heads' pre-activations z, and dpred is the gradient w.r.t. z -- each
// component times 1 - y^2 from the output y (TensorFlow's TanhGrad), one fma and one multiply; exactly 0 where y is exactly +-1.
__device__ __forceinline__ void tanh_grad_store(const float* yb, int64_t i, float* __restrict__ d, float gu, float gv, float gw) {
    asm volatile("" : "+s"(yb));                // fresh loads (L1 hits): the three outputs do not stay in registers across the stencil gathers
    const float* y = yb + i;
    const float yu = y[0];
    d[0] = gu * fmaf(-yu, yu, 1.f);
    const float yv = y[1];
    d[1] = gv * fmaf(-yv, yv, 1.f);
    const float yw = y[2];
    d[2] = gw * fmaf(-yw, yw, 1.f);
}

// The penalty rho of the data term and its derivative psi, per component of the residual d (fdn_loss_metrics_kind).  KIND is a
// compile-time parameter of loss_body: FDN_LOSS_MSE is the arithmetic the loss always had (rho = d^2 summed as one fma chain, psi's 2 in
// the voxel weight), the others sum theirs in pen_sum.  kp: delta (Huber) or epsilon (Charbonnier), kp2 = kp * kp.
// IEEE sqrtf and division (hipcc's default for fp32): correctly rounded, which the tests' rounding count relies on.  psi(0) is exactly 0
// for every kind (MAE: tf.abs' gradient; Huber: 0 lies in the inner branch; Charbonnier: 0 / eps, and 0 where eps^2 underflowed to 0).
template <int KIND>
__device__ __forceinline__ float pen_psi(float d, float kp, float kp2) {
    if (KIND == FDN_LOSS_MAE) return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    if (KIND == FDN_LOSS_HUBER) return fabsf(d) <= kp ? d : copysignf(kp, d);
    if (KIND == FDN_LOSS_CHARBONNIER) { const float s = sqrtf(fmaf(d, d, kp2)); return s > 0.f ? d / s : 0.f; }
    return d;                                                       // MSE: the factor 2 rides on the voxel weight
}
template <int KIND>
__device__ __forceinline__ float pen_sum(float du, float dv, float dw, float mse, float kp, float kp2) {
    if (KIND == FDN_LOSS_MAE) return fabsf(du) + fabsf(dv) + fabsf(dw);
    if (KIND == FDN_LOSS_HUBER) {
        // with t = clamp(d, -delta, delta): rho = t (d - t / 2), d^2 / 2 inside and delta (|d| - delta / 2) outside without a branch; summed
        // as the MSE's fma chain, so where every |d| <= delta the sum is the MSE's scaled by a power of two: half of it, bit for bit.
        // (psi is the same t; taking it from here instead of pen_psi's select costs the shared kernel a spill)
        const float tu = fminf(fmaxf(du, -kp), kp), tv = fminf(fmaxf(dv, -kp), kp), tw = fminf(fmaxf(dw, -kp), kp);
        return fmaf(tw, fmaf(-0.5f, tw, dw), fmaf(tv, fmaf(-0.5f, tv, dv), tu * fmaf(-0.5f, tu, du)));
    }
    if (KIND == FDN_LOSS_CHARBONNIER) return sqrtf(fmaf(du, du, kp2)) + sqrtf(fmaf(dv, dv, kp2)) + sqrtf(fmaf(dw, dw, kp2));
    return mse;
}

// div_w == 0: the masked data term alone, exactly the arithmetic and block -> voxel mapping of the plain loss.  div_w > 0 (fdn_loss_metrics_div):
// the same pass also gathers each channel's stencil neighbours (e at +-1, +-2 and m at +-1 along its axis; L1 / L2 hits), adds the
// divergence part of dpred and writes two more per-block partials (sum m d, sum nf d; the weight is applied in loss_finalize_kernel).
// nparts: partials per block, 3 (plain) or 5.  (The branch's gathers in flight take the kernel from 26 to 68 VGPRs: seven waves per
// SIMD instead of eight; capping it at 64 spills.)  nf_w (fdn_loss_metrics_act): the non-fluid region's weight, folded into inv_nf, so it
// reaches the region's part of dpred -- data term and divergence -- through the existing arithmetic; the sums stay unweighted and
// loss_finalize_kernel applies it.  The divergence term is squared for every KIND: it works on the raw residuals.
template <int KIND>
__device__ __forceinline__ void loss_body(const float* __restrict__ pred, const float* __restrict__ uh, const float* __restrict__ vh,
                                          const float* __restrict__ wh, const float* __restrict__ mask, float* __restrict__ scratch,
                                          float* __restrict__ dpred, int64_t V, int D, int H, int W, float div_w, int nparts, float nf_w,
                                          int out_act, float kp, float* red) {
    constexpr bool MSE = KIND == FDN_LOSS_MSE;
    const int n = blockIdx.y;
    const float inv_f = 1.f / (scratch[n * 8 + 0] + 1.f);
    const float inv_nf = nf_w * (1.f / (scratch[n * 8 + 1] + 1.f));     // non_fluid_weight rides on the region's scalar: exact at 1
    const float kp2 = kp * kp;
    if (div_w != 0.f) {
        const float two_w = 2.f * div_w;
        const int64_t HW = (int64_t)H * W;
        float sf = 0.f, snf = 0.f, srel = 0.f, sdf = 0.f, sdn = 0.f;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t g = (int64_t)n * V + i;
            const float tu = uh[g], tv = vh[g], tw = wh[g];
            const float du = pred[g * 3] - tu, dv = pred[g * 3 + 1] - tv, dw = pred[g * 3 + 2] - tw;
            const float m = mask[g];
            const float nf = m < 0.5f ? 1.f : 0.f;
            const float mse = du * du + dv * dv + dw * dw;
            const float e = pen_sum<KIND>(du, dv, dw, mse, kp, kp2);
            sf += e * m;
            snf += e * nf;
            const float diff = sqrtf(mse);
            const float actual = sqrtf(tu * tu + tv * tv + tw * tw);
            float rel = diff / (actual + 1e-5f);
            rel = fminf(fmaxf(rel, 0.f), 1.f);
            float corr = actual != 0.f ? rel : diff;
            corr = rintf(corr * 1e4f) / 1e4f;
            if (m == 1.0f) srel += corr;
            const unsigned iv = (unsigned)i;                       // V < 2^31 (fdn_loss_metrics_div)
            const unsigned q = iv / (unsigned)W;
            const int pw = (int)(iv - q * (unsigned)W), ph = (int)(q % (unsigned)H), pd = (int)(q / (unsigned)H);
            const float c0 = m * inv_f + nf * inv_nf;
            const float wgt = MSE ? 2.f * c0 : c0;
            float gu = pen_psi<KIND>(du, kp, kp2) * wgt, gv = pen_psi<KIND>(dv, kp, kp2) * wgt, gw = pen_psi<KIND>(dw, kp, kp2) * wgt;
            const float au = div_axis(pred, uh, mask, g, 0, pd, D, HW, du, c0, inv_f, inv_nf, two_w, &gu);
            const float av = div_axis(pred, vh, mask, g, 1, ph, H, W, dv, c0, inv_f, inv_nf, two_w, &gv);
            const float aw = div_axis(pred, wh, mask, g, 2, pw, W, 1, dw, c0, inv_f, inv_nf, two_w, &gw);
            const float dd = au * au + av * av + aw * aw;
            sdf += dd * m;
            sdn += dd * nf;
            if (dpred) {
                if (out_act == FDN_ACT_TANH) tanh_grad_store(pred, g * 3, dpred + g * 3, gu, gv, gw);
                else { dpred[g * 3] = gu; dpred[g * 3 + 1] = gv; dpred[g * 3 + 2] = gw; }
            }
        }
        const float a = block_sum(sf, red);
        const float b = block_sum(snf, red);
        const float c = block_sum(srel, red);
        const float d = block_sum(sdf, red);
        const float e = block_sum(sdn, red);
        if (threadIdx.x == 0) {
            float* part = scratch + (size_t)gridDim.y * 8 + ((size_t)n * gridDim.x + blockIdx.x) * 5;
            part[0] = a; part[1] = b; part[2] = c; part[3] = d; part[4] = e;
        }
        return;
    }
    float sf = 0.f, snf = 0.f, srel = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = (int64_t)n * V + i;
        const float tu = uh[g], tv = vh[g], tw = wh[g];
        const float du = pred[g * 3] - tu, dv = pred[g * 3 + 1] - tv, dw = pred[g * 3 + 2] - tw;
        const float m = mask[g];
        const float nf = m < 0.5f ? 1.f : 0.f;
        const float mse = du * du + dv * dv + dw * dw;
        const float e = pen_sum<KIND>(du, dv, dw, mse, kp, kp2);
        sf += e * m;
        snf += e * nf;
        // relative error (loss_utils.py:64-103); rintf == round-half-to-even == tf.round
        const float diff = sqrtf(mse);
        const float actual = sqrtf(tu * tu + tv * tv + tw * tw);
        float rel = diff / (actual + 1e-5f);
        rel = fminf(fmaxf(rel, 0.f), 1.f);
        float corr = actual != 0.f ? rel : diff;
        corr = rintf(corr * 1e4f) / 1e4f;
        if (m == 1.0f) srel += corr;
        if (dpred) {
            const float c0 = m * inv_f + nf * inv_nf;
            const float wgt = MSE ? 2.f * c0 : c0;
            const float gu = pen_psi<KIND>(du, kp, kp2) * wgt, gv = pen_psi<KIND>(dv, kp, kp2) * wgt, gw = pen_psi<KIND>(dw, kp, kp2) * wgt;
            if (out_act == FDN_ACT_TANH) tanh_grad_store(pred, g * 3, dpred + g * 3, gu, gv, gw);
            else { dpred[g * 3] = gu; dpred[g * 3 + 1] = gv; dpred[g * 3 + 2] = gw; }
        }
    }
    const float a = block_sum(sf, red);
    const float b = block_sum(snf, red);
    const float c = block_sum(srel, red);
    // per-block partials, summed by loss_finalize_kernel in block order: the reported loss / metric is run-to-run identical
    // (the mask counts above are integers < 2^24, so their atomic sums are exact in any order)
    if (threadIdx.x == 0) {
        float* part = scratch + (size_t)gridDim.y * 8 + ((size_t)n * gridDim.x + blockIdx.x) * nparts;
        part[0] = a; part[1] = b; part[2] = c;
        if (nparts == 5) { part[3] = 0.f; part[4] = 0.f; }
    }
}

// One kernel symbol for every kind (tests/test_isa.py pins the product library's kernel set): the block picks its instantiation of
// loss_body once, on a wave-uniform scalar, before the voxel loop; no loop holds a switch on the kind.  kind == FDN_LOSS_MSE (what
// fdn_loss_metrics / _div / _act pass) runs the instantiation that is the loss as it always was.  A kernel's register allocation is that
// of its hungriest path -- Charbonnier's divergence branch, 78 VGPRs left alone, which would cost every kind the seventh wave -- so the
// kernel asks for seven waves per SIMD: 72 VGPRs, no spills (DESIGN 5.4a'' has the table per instantiation).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7))) void loss_main_kernel(const float* __restrict__ pred, const float* __restrict__ uh,
                                                         const float* __restrict__ vh, const float* __restrict__ wh,
                                                         const float* __restrict__ mask, float* __restrict__ scratch,
                                                         float* __restrict__ dpred, int64_t V, int D, int H, int W, float div_w,
                                                         int nparts, float nf_w, int out_act, int kind, float kp) {
    __shared__ float red[4];
    if (kind == FDN_LOSS_MSE) {                   // the shipped loss first: its code follows the prologue, as it always did
        loss_body<FDN_LOSS_MSE>(pred, uh, vh, wh, mask, scratch, dpred, V, D, H, W, div_w, nparts, nf_w, out_act, 0.f, red);
        return;
    }
    int other = kind;
    asm volatile("" : "+s"(other));               // a second scalar: the compiler does not fold the test above into one four-way switch
    if (other == FDN_LOSS_MAE) loss_body<FDN_LOSS_MAE>(pred, uh, vh, wh, mask, scratch, dpred, V, D, H, W, div_w, nparts, nf_w, out_act, 0.f, red);
    else if (other == FDN_LOSS_HUBER) loss_body<FDN_LOSS_HUBER>(pred, uh, vh, wh, mask, scratch, dpred, V, D, H, W, div_w, nparts, nf_w, out_act, kp, red);
    else loss_body<FDN_LOSS_CHARBONNIER>(pred, uh, vh, wh, mask, scratch, dpred, V, D, H, W, div_w, nparts, nf_w, out_act, kp, red);
}

// one wave per sample: lane t sums the partials of blocks t, t + 64, ..., then a shuffle tree -- a fixed order, so the reported loss /
// metric stays run-to-run identical (one THREAD per sample walked the 256 partials as a chain of dependent loads: 24 us).
// nparts 3: out (N,4); nparts 5: out (N,5), column 4 = div_w * (sum m d / (sum m + 1) + nf_w * sum nf d / (sum nf + 1)); nf_w also weighs
// the non-fluid part of column 0 (a multiplication by 1.f, exact, everywhere but in fdn_loss_metrics_act).
__global__ __launch_bounds__(64) void loss_finalize_kernel(const float* __restrict__ scratch, float* __restrict__ out, int N, int nblk,
                                                           int nparts, float div_w, float nf_w) {
    const int n = blockIdx.x;
    const float* part = scratch + (size_t)N * 8 + (size_t)n * nblk * nparts;
    float sf = 0.f, sn = 0.f, sr = 0.f, sdf = 0.f, sdn = 0.f;
    if (nparts == 5) {
        for (int b = threadIdx.x; b < nblk; b += 64) {
            sf += part[b * 5]; sn += part[b * 5 + 1]; sr += part[b * 5 + 2]; sdf += part[b * 5 + 3]; sdn += part[b * 5 + 4];
        }
        for (int o = 32; o > 0; o >>= 1) { sdf += __shfl_down(sdf, o, 64); sdn += __shfl_down(sdn, o, 64); }
    } else {
        for (int b = threadIdx.x; b < nblk; b += 64) { sf += part[b * 3]; sn += part[b * 3 + 1]; sr += part[b * 3 + 2]; }
    }
    for (int o = 32; o > 0; o >>= 1) { sf += __shfl_down(sf, o, 64); sn += __shfl_down(sn, o, 64); sr += __shfl_down(sr, o, 64); }
    if (threadIdx.x) return;
    const float sm = scratch[n * 8 + 0], snf = scratch[n * 8 + 1];
    const int nc = nparts == 5 ? 5 : 4;
    out[n * nc + 0] = sf / (sm + 1.f) + nf_w * (sn / (snf + 1.f));
    out[n * nc + 1] = sr / (sm + 1.f) * 100.f;
    out[n * nc + 2] = sm;
    out[n * nc + 3] = snf;
    if (nparts == 5) out[n * 5 + 4] = div_w * (sdf / (sm + 1.f) + nf_w * (sdn / (snf + 1.f)));
}

// ONE block (fixed summation order, no atomics): this pass only runs when the parameters changed outside the optimizer
// (first step, load_weights); afterwards the Adam kernel supplies the sum
__global__ __launch_bounds__(1024) void l2_sumsq_kernel(const float* __restrict__ w, const uint8_t* __restrict__ isk,
                                                         int64_t n, float* __restrict__ out) {
    __shared__ float red[16];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;           // four independent chains: the loads of a trip overlap
    int64_t i = threadIdx.x;
    for (; i + 3 * 1024 < n; i += 4 * 1024) {
        const float a0 = isk[i] ? w[i] : 0.f, a1 = isk[i + 1024] ? w[i + 1024] : 0.f;
        const float a2 = isk[i + 2048] ? w[i + 2048] : 0.f, a3 = isk[i + 3072] ? w[i + 3072] : 0.f;
        s0 += a0 * a0; s1 += a1 * a1; s2 += a2 * a2; s3 += a3 * a3;
    }
    for (; i < n; i += 1024)
        if (isk[i]) s0 += w[i] * w[i];
    const float s = (s0 + s1) + (s2 + s3);
    const float a = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = a;
}

// The per-block sum every pass on the FDN_ADAM_PARTIALS blocking ends with: shuffle tree per wave, then the four waves in a fixed order.
__device__ __forceinline__ void block_partial(float ss, float* __restrict__ out) {
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// sumsq != null: block b also writes sum(w_new^2) over its kernel (non-bias) elements to sumsq[b] (fixed order: the
// regulariser value of the NEXT step's loss, so fdn_l2_sumsq does not have to stream the parameters again).
// lr_t_dev != null: the step size is lr_t_dev[0], read on the device (fdn_adam_step_dev: a captured launch must not bake it in).
// frozen != null (fdn_adam_step_masked: fine-tuning, one byte per parameter like isk): an element with frozen[i] != 0 keeps w, m and v --
// g[i], m[i] and v[i] are neither loaded nor stored -- and still adds w[i]^2 to its block's sum when it is a kernel: the regulariser
// value covers every kernel (TrainerController.py:129-141).  An element with frozen[i] == 0 takes the statements below unchanged.
// g_scale_dev != null / clip_value > 0 (fdn_adam_step_clipped): g' *= g_scale_dev[0] (one fp32 multiply behind the L2 term: the scale
// fdn_clip_scale left on the device) / g' clamped to [-clip_value, clip_value] by comparisons, so that a NaN stays a NaN.
// ema != null (fdn_adam_step_ema: tf.keras.optimizers.Adam(use_ema=, ema_momentum=)): the exponential moving average of the weights,
// ema[i] = mom * ema[i] + (1.f - mom) * wn in fp32, formed from the wn in the register right behind the store of w[i]; ema_init != 0
// (the first step with an average): ema[i] is not loaded, the average starts at wi, the weight before the step.  A frozen element
// stores the wi it loaded: the average of a frozen parameter is its weight.  w, m, v and sumsq get the bits of the call without ema.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, const uint8_t* __restrict__ isk, int64_t n, float lr_t_host,
                                                   const float* __restrict__ lr_t_dev, float b1, float b2, float eps, float l2s_host,
                                                   const float* __restrict__ l2s_dev, float* __restrict__ sumsq,
                                                   const uint8_t* __restrict__ frozen, const float* __restrict__ g_scale_dev,
                                                   float clip_value, float* __restrict__ ema, float ema_momentum, int ema_init) {
    const float lr_t = lr_t_dev ? lr_t_dev[0] : lr_t_host;
    const float l2s = l2s_dev ? l2s_host * l2s_dev[0] : l2s_host;
    const float g_scale = g_scale_dev ? g_scale_dev[0] : 1.f;
    float ss = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float wi = w[i];
        const bool k = isk[i] != 0;
        float wn = wi;
        if (!(frozen && frozen[i])) {
            float gi = g[i];
            if (k) gi += l2s * wi;
            if (g_scale_dev) gi *= g_scale;
            if (clip_value > 0.f) gi = gi > clip_value ? clip_value : (gi < -clip_value ? -clip_value : gi);
            const float mi = b1 * m[i] + (1.f - b1) * gi;
            const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            wn = wi - lr_t * mi / (sqrtf(vi) + eps);
            w[i] = wn;
            if (ema) ema[i] = ema_momentum * (ema_init ? wi : ema[i]) + (1.f - ema_momentum) * wn;
        } else if (ema) {
            ema[i] = wi;
        }
        if (k) ss += wn * wn;
    }
    if (sumsq) block_partial(ss, sumsq);
}

// fdn_grad_accumulate: the sum of micro-batch gradient buffers, acc[i] = g[i] (first) or acc[i] + g[i].  Scalar accesses: acc and g are
// bucket slices at any float offset, and the 13.4 MB of cfg2 are not where the step's time is.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, int64_t n, int first) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i];
        if (first) acc[i] = gi;                                      // a bit copy: the accumulator's old contents are never loaded
        else acc[i] = acc[i] + gi;                                   // one IEEE fp32 add
    }
}

// fdn_grad_sumsq_partials (gradient clipping, tf.clip_by_global_norm): sumsq[b] = block b's sum of g'^2, g' = g + l2s * w (kernels only)
// formed as adam_kernel forms it, over the elements with frozen[i] == 0 -- the square of the norm Keras clips,
// TrainerController.py:73,223-225.  The blocking of adam_kernel's own partials (FDN_ADAM_PARTIALS blocks, block_partial).
__global__ __launch_bounds__(256) void grad_sumsq_partials_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                                  const uint8_t* __restrict__ isk, const uint8_t* __restrict__ frozen,
                                                                  int64_t n, float l2s_host, const float* __restrict__ l2s_dev,
                                                                  float* __restrict__ sumsq) {
    const float l2s = l2s_dev ? l2s_host * l2s_dev[0] : l2s_host;
    float ss = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (frozen && frozen[i]) continue;                           // g[i] is not loaded; the element adds +0
        float gi = g[i];
        if (isk[i]) gi += l2s * w[i];
        ss += gi * gi;
    }
    block_partial(ss, sumsq);
}

// The same per-block sums the Adam kernel leaves behind (identical blocking: block b covers the elements b * 256 + t + k * grid * 256),
// for the steps that have no Adam step before them (first step, load_weights): FDN_ADAM_PARTIALS blocks stream the parameters at the
// rate of the chip instead of one block at 9 GB/s (l2_sumsq_kernel: 1.87 ms for the 13.4 MB of cfg2)
__global__ __launch_bounds__(256) void l2_sumsq_partials_kernel(const float* __restrict__ w, const uint8_t* __restrict__ isk, int64_t n,
                                                                 float* __restrict__ sumsq) {
    float ss = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (isk[i]) ss += w[i] * w[i];
    block_partial(ss, sumsq);
}

// The sum of n partials by one block of 256 threads in a fixed order (deterministic); valid in thread 0.
__device__ __forceinline__ float sum_partials(const float* __restrict__ part, int n) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return threadIdx.x == 0 ? (red[0] + red[1]) + (red[2] + red[3]) : 0.f;
}

// fdn_sum_partials: out[0] = that sum.
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    const float total = sum_partials(part, n);
    if (threadIdx.x == 0) out[0] = total;
}

// fdn_clip_scale: the partials are those of fdn_grad_sumsq_partials and their sum S becomes out[0] = N = sqrtf(S), the global norm, and
// out[1] = s = clip_norm / max(N, clip_norm), the factor of tf.clip_by_global_norm: exactly 1.0f whenever N <= clip_norm (x / x), so an
// inactive clip changes no bit downstream.  TF writes clip_norm * min(1 / N, 1 / clip_norm): two roundings instead of one, equal up to
// rounding.  N not finite (an inf or NaN gradient, or squares that overflow): s = NaN, which makes every parameter the step updates
// NaN, as in TF.
__global__ __launch_bounds__(256) void clip_scale_kernel(const float* __restrict__ part, int n, float* __restrict__ out, float clip_norm) {
    const float total = sum_partials(part, n);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(total);
        out[0] = norm;
        out[1] = __builtin_isfinite(norm) ? clip_norm / (norm > clip_norm ? norm : clip_norm) : __builtin_nanf("");
    }
}

int grid_for(int64_t items, int cap = 4096) {
    int64_t b = (items + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

float axis_scale(int n, int R) {
    const int m = n * R;
    return m > 1 ? (float)(n - 1) / (float)(m - 1) : 0.f;
}

}  // namespace

template <typename T>
static int input_features_t(const float* u, const float* v, const float* w, const float* mu, const float* mv, const float* mw,
                            T* phase, T* pc, int64_t nvox, void* stream) {
    FDN_REQUIRE(u && v && w && mu && mv && mw && phase && pc && nvox > 0, "fdn_input_features: NULL argument or nvox<=0");
    hipLaunchKernelGGL(input_features_kernel<T>, dim3(grid_for(nvox)), dim3(256), 0, (hipStream_t)stream, u, v, w, mu, mv, mw,
                       phase, pc, nvox);
    FDN_CHECK_LAUNCH("input_features_kernel");
    return FDN_OK;
}
template <typename T>
static int input_features_volume_t(const char* who, const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz,
                                   int64_t g0, int count, T* phase, T* pc, void* stream, int plane = 0, int k = 0, int stride = 0,
                                   bool strided = false) {
    FDN_REQUIRE(frames && phase && pc, "%s: NULL argument", who);
    FDN_REQUIRE(F > 0 && X > 0 && Y > 0 && Z > 0, "%s: bad frames (F=%d, X=%d, Y=%d, Z=%d)", who, F, X, Y, Z);
    FDN_REQUIRE(P > 4 && P <= 1024, "%s: patch size P=%d must be in 5..1024 (the window advances by P - 4)", who, P);
    FDN_REQUIRE(nx > 0 && ny > 0 && nz > 0, "%s: bad patch counts (%d,%d,%d)", who, nx, ny, nz);
    FDN_REQUIRE(count > 0, "%s: count=%d", who, count);
    FDN_REQUIRE(g0 >= 0, "%s: g0=%lld", who, (long long)g0);
    FDN_REQUIRE(g0 + count <= (int64_t)F * nx * ny * nz, "%s: patches [%lld, %lld) exceed F*nx*ny*nz = %lld", who, (long long)g0,
                (long long)(g0 + count), (long long)((int64_t)F * nx * ny * nz));
    const int word = fdn_orient_word(plane, k, 0);
    FDN_REQUIRE(word >= 0, "%s: orientation (plane=%d, k=%d) is neither (0,0) nor plane in 1..3 with k in 1..3", who, plane, k);
    FDN_REQUIRE(!strided || (stride >= 1 && stride <= P - 4), "%s: stride=%d must be in 1..P-4 = %d", who, stride, P - 4);
    const int64_t nvox = (int64_t)count * P * P * P;
    InputGeom geo{};
    geo.orient = plane ? word : 0;
    geo.stride = strided ? stride : P - 4;
    geo.P = P; geo.X = X; geo.Y = Y; geo.Z = Z; geo.nx = nx; geo.ny = ny; geo.nz = nz; geo.g0 = g0;
    hipLaunchKernelGGL(input_features_volume_kernel<T>, dim3(grid_for(nvox)), dim3(256), 0, (hipStream_t)stream, frames, phase, pc, nvox,
                       geo);
    FDN_CHECK_LAUNCH("input_features_volume_kernel");
    return FDN_OK;
}
extern "C" int fdn_input_features(const float* u, const float* v, const float* w, const float* mu, const float* mv,
                                  const float* mw, float* phase, float* pc, int64_t nvox, void* stream) {
    return input_features_t<float>(u, v, w, mu, mv, mw, phase, pc, nvox, stream);
}
extern "C" int fdn_input_features_bf16(const float* u, const float* v, const float* w, const float* mu, const float* mv,
                                       const float* mw, uint16_t* phase, uint16_t* pc, int64_t nvox, void* stream) {
    return input_features_t<uint16_t>(u, v, w, mu, mv, mw, phase, pc, nvox, stream);
}
extern "C" int fdn_input_features_volume(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz, int64_t g0,
                                         int count, float* phase, float* pc, void* stream) {
    return input_features_volume_t<float>("fdn_input_features_volume", frames, F, X, Y, Z, P, nx, ny, nz, g0, count, phase, pc, stream);
}
extern "C" int fdn_input_features_volume_bf16(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz,
                                              int64_t g0, int count, uint16_t* phase, uint16_t* pc, void* stream) {
    return input_features_volume_t<uint16_t>("fdn_input_features_volume_bf16", frames, F, X, Y, Z, P, nx, ny, nz, g0, count, phase, pc,
                                             stream);
}

extern "C" int fdn_input_features_volume_oriented(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz,
                                                  int64_t g0, int count, int plane, int k, float* phase, float* pc, void* stream) {
    return input_features_volume_t<float>("fdn_input_features_volume_oriented", frames, F, X, Y, Z, P, nx, ny, nz, g0, count, phase, pc,
                                          stream, plane, k);
}
extern "C" int fdn_input_features_volume_oriented_bf16(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz,
                                                       int64_t g0, int count, int plane, int k, uint16_t* phase, uint16_t* pc,
                                                       void* stream) {
    return input_features_volume_t<uint16_t>("fdn_input_features_volume_oriented_bf16", frames, F, X, Y, Z, P, nx, ny, nz, g0, count, phase,
                                             pc, stream, plane, k);
}

extern "C" int fdn_input_features_volume_strided(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz, int64_t g0,
                                                 int count, int stride, int plane, int k, float* phase, float* pc, void* stream) {
    return input_features_volume_t<float>("fdn_input_features_volume_strided", frames, F, X, Y, Z, P, nx, ny, nz, g0, count, phase, pc,
                                          stream, plane, k, stride, true);
}
extern "C" int fdn_input_features_volume_strided_bf16(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz,
                                                      int64_t g0, int count, int stride, int plane, int k, uint16_t* phase, uint16_t* pc,
                                                      void* stream) {
    return input_features_volume_t<uint16_t>("fdn_input_features_volume_strided_bf16", frames, F, X, Y, Z, P, nx, ny, nz, g0, count, phase,
                                             pc, stream, plane, k, stride, true);
}

extern "C" int fdn_fold_halo(const float* dxpad0, const float* dxpad1, const float* dxpad2, int nsrc, const float* skip,
                             const float* y_prev, int act, float alpha, float* dz_prev, int N, int D, int H, int W, int C,
                             void* stream) {
    FDN_REFUSE_TANH(act, "fdn_fold_halo");
    FDN_REQUIRE(dxpad0 && dz_prev, "fdn_fold_halo: NULL argument");
    FDN_REQUIRE(nsrc >= 1 && nsrc <= 3 && (nsrc < 2 || dxpad1) && (nsrc < 3 || dxpad2), "fdn_fold_halo: bad nsrc %d", nsrc);
    FDN_REQUIRE(C % 4 == 0 && N > 0 && D > 0 && H > 0 && W > 0, "fdn_fold_halo: bad dims (C must be a multiple of 4)");
    const int64_t total = (int64_t)N * D * H * W * (C / 4);
    hipLaunchKernelGGL(fold_halo_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, (hipStream_t)stream, dxpad0, dxpad1,
                       dxpad2, nsrc, skip, y_prev, act, alpha, dz_prev, N, D, H, W, C / 4);
    FDN_CHECK_LAUNCH("fold_halo_kernel");
    return FDN_OK;
}

template <typename T>
static int upsample_fwd_t(const T* x, T* y, int N, int D, int H, int W, int C, int R, void* stream) {
    constexpr int E = 16 / (int)sizeof(T);
    FDN_REQUIRE(x && y && C % E == 0 && R >= 1 && N > 0 && D > 0 && H > 0 && W > 0, "fdn_upsample_trilinear_fwd: bad argument");
    const int64_t rows = (int64_t)N * D * R * H * R;
    FDN_REQUIRE(rows < (1ll << 31), "fdn_upsample_trilinear_fwd: too many rows");
    const size_t lds = (size_t)4 * W * C * sizeof(T);
    FDN_PLAN("fam=upsample_fwd op=fwd dt=%s N=%d D=%d H=%d W=%d R=%d staged=%d grid=%lld tiles=%lld cus=%d", sizeof(T) == 2 ? "bf16" : "f32", N, D, H, W, R,
             lds <= 64 * 1024, (long long)(rows < 262144 ? rows : 262144), (long long)rows, fdn_plan_cus());
    if (lds <= 64 * 1024) {
        if (lds > 48 * 1024)
            if (int rc = fdn_func_max_lds((const void*)upsample_fwd_kernel<T, true>, 64 * 1024, "upsample_fwd")) return rc;
        hipLaunchKernelGGL((upsample_fwd_kernel<T, true>), dim3((unsigned)(rows < 262144 ? rows : 262144)), dim3(256), lds, (hipStream_t)stream,
                           x, y, N, D, H, W, C / E, R, axis_scale(D, R), axis_scale(H, R), axis_scale(W, R));
    } else {
        hipLaunchKernelGGL((upsample_fwd_kernel<T, false>), dim3((unsigned)(rows < 262144 ? rows : 262144)), dim3(256), 0, (hipStream_t)stream,
                           x, y, N, D, H, W, C / E, R, axis_scale(D, R), axis_scale(H, R), axis_scale(W, R));
    }
    FDN_CHECK_LAUNCH("upsample_fwd_kernel");
    return FDN_OK;
}
FDN_HOOK_VAR(int, fdn_upsample_bwd_hb, 0);        // test / bench hook: low-res rows per block of upsample_bwd_kernel (0 = planner)
#ifdef FDN_TEST_HOOKS
extern "C" int fdn_debug_set_upsample_bwd_hb(int hb) { fdn_upsample_bwd_hb = hb; return FDN_OK; }
#endif
template <typename T>
static int upsample_bwd_t(const T* dy, const T* y_prev, int act, float alpha, T* dx, int N, int D, int H, int W, int C, int R,
                          void* stream) {
    constexpr int E = 16 / (int)sizeof(T);
    FDN_REFUSE_TANH(act, sizeof(T) == 2 ? "fdn_upsample_trilinear_bwd_bf16" : "fdn_upsample_trilinear_bwd");
    FDN_REQUIRE(dy && dx && C % E == 0 && R >= 1 && N > 0 && D > 0 && H > 0 && W > 0, "fdn_upsample_trilinear_bwd: bad argument");
    const int64_t rows = (int64_t)N * D * H;
    const size_t row_lds = (size_t)W * R * C * sizeof(float);
    FDN_REQUIRE(rows * R * R < (1ll << 31) && row_lds <= 150 * 1024, "fdn_upsample_trilinear_bwd: row of %d x %d channels does not fit the LDS stage", W * R, C);
    // the adjoint compacts the high-res rows that can touch a low-res row with 32 lanes along d: a low-res row reaches
    // 2 (OD-1)/(D-1) high-res rows (align_corners scale) + the rounding margin, which exceeds 2R+1 on short axes; along h the HB rows of a
    // block share 64 lanes
    auto span = [](int n, int r, int hb) { return n > 1 ? ((hb + 1) * (n * r - 1) + (n - 2)) / (n - 1) + 3 : n * r; };
    FDN_REQUIRE(span(D, R, 1) <= 32 && span(H, R, 1) <= 32, "fdn_upsample_trilinear_bwd: R = %d on a %d x %d grid needs %d / %d candidate rows per axis "
                "(the adjoint keeps <= 32)", R, D, H, span(D, R, 1), span(H, R, 1));
    // HB = 2 low-res rows per block where the LDS rows leave room for two workgroups per CU and the candidates fit the tables, else 1
    // (measured, tools/bench_upsample.py --hb: fp32 (8,24^3) x2 0.062 / 0.057 / 0.087 ms with 1 / 2 / 4 rows -- four rows cost more
    // occupancy than their L1 traffic saves; bf16 (4,32^3) x4 0.370 / 0.302)
    auto fits = [&](int hb) { return hb * row_lds + 14 * 1024 <= 80 * 1024 && span(H, R, hb) <= 64 && span(D, R, 1) * span(H, R, hb) <= 512; };
    int hb = fits(2) ? 2 : 1;
    if (fdn_upsample_bwd_hb) {                                             // (test build: forced)
        FDN_REQUIRE(fdn_upsample_bwd_hb == 1 || fits(fdn_upsample_bwd_hb), "fdn_upsample_trilinear_bwd: %d rows per block do not fit", fdn_upsample_bwd_hb);
        hb = fdn_upsample_bwd_hb;
    }
    const size_t lds = (size_t)hb * row_lds;
    const int64_t blocks = (int64_t)N * D * ((H + hb - 1) / hb);
    const unsigned grid = (unsigned)(blocks < 65536 ? blocks : 65536);
    const float sd = axis_scale(D, R), sh = axis_scale(H, R), sw = axis_scale(W, R);
    FDN_PLAN("fam=upsample_bwd op=bwd dt=%s N=%d D=%d H=%d W=%d R=%d hb=%d grid=%u tiles=%lld cus=%d", sizeof(T) == 2 ? "bf16" : "f32", N, D, H, W, R, hb,
             grid, (long long)blocks, fdn_plan_cus());
    auto launch = [&](auto tag) -> int {
        constexpr int HB = decltype(tag)::value;
        if (lds > 48 * 1024) {
            if (int rc = fdn_func_max_lds((const void*)upsample_bwd_kernel<T, HB>, 150 * 1024, "upsample_bwd")) return rc;
        }
        hipLaunchKernelGGL((upsample_bwd_kernel<T, HB>), dim3(grid), dim3(256), lds, (hipStream_t)stream, dy, y_prev, act, alpha, dx, N, D, H, W,
                           C / E, R, sd, sh, sw);
        return FDN_OK;
    };
    FDN_REQUIRE(hb == 1 || hb == 2, "fdn_upsample_trilinear_bwd: %d rows per block", hb);
    if (int rc = hb == 2 ? launch(std::integral_constant<int, 2>{}) : launch(std::integral_constant<int, 1>{})) return rc;
    FDN_CHECK_LAUNCH("upsample_bwd_kernel");
    return FDN_OK;
}
extern "C" int fdn_upsample_trilinear_fwd(const float* x, float* y, int N, int D, int H, int W, int C, int R, void* stream) {
    return upsample_fwd_t<float>(x, y, N, D, H, W, C, R, stream);
}
extern "C" int fdn_upsample_trilinear_bwd(const float* dy, const float* y_prev, int act, float alpha, float* dx, int N, int D,
                                          int H, int W, int C, int R, void* stream) {
    return upsample_bwd_t<float>(dy, y_prev, act, alpha, dx, N, D, H, W, C, R, stream);
}
extern "C" int fdn_upsample_trilinear_fwd_bf16(const uint16_t* x, uint16_t* y, int N, int D, int H, int W, int C, int R,
                                               void* stream) {
    return upsample_fwd_t<uint16_t>(x, y, N, D, H, W, C, R, stream);
}
extern "C" int fdn_upsample_trilinear_bwd_bf16(const uint16_t* dy, const uint16_t* y_prev, int act, float alpha, uint16_t* dx,
                                               int N, int D, int H, int W, int C, int R, void* stream) {
    return upsample_bwd_t<uint16_t>(dy, y_prev, act, alpha, dx, N, D, H, W, C, R, stream);
}

// the three launches of both loss entry points; nparts 3: out (N,4) (fdn_loss_metrics), 5: out (N,5) (fdn_loss_metrics_div)
static int loss_launch(const char* who, const float* pred, const float* uh, const float* vh, const float* wh, const float* mask, float* out,
                       float* dpred, float* scratch, int N, int64_t V, int D, int H, int W, float div_w, int nparts, void* stream,
                       float nf_w = 1.f, int out_act = FDN_ACT_NONE, int kind = FDN_LOSS_MSE, float kind_param = 0.f) {
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(scratch, 0, (size_t)N * 8 * sizeof(float), s);
    if (e != hipSuccess) { fdn_set_error("%s: memset: %s", who, hipGetErrorString(e)); return FDN_ERR_HIP; }
    const int gx = grid_for(V, FDN_LOSS_BLOCKS);
    // (16 blocks per sample: with 256 the 2 x 256 x N atomics on 2 N words took longer than reading the mask -- 29 us at cfg2)
    hipLaunchKernelGGL(mask_sums_kernel, dim3(gx < 16 ? gx : 16, N), dim3(256), 0, s, mask, scratch, V);
    FDN_CHECK_LAUNCH("mask_sums_kernel");
    hipLaunchKernelGGL(loss_main_kernel, dim3(gx, N), dim3(256), 0, s, pred, uh, vh, wh, mask, scratch, dpred, V, D, H, W, div_w, nparts,
                       nf_w, out_act, kind, kind_param);
    FDN_CHECK_LAUNCH("loss_main_kernel");
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(N), dim3(64), 0, s, (const float*)scratch, out, N, gx, nparts, div_w, nf_w);
    FDN_CHECK_LAUNCH("loss_finalize_kernel");
    return FDN_OK;
}

extern "C" int fdn_loss_metrics(const float* pred, const float* uh, const float* vh, const float* wh, const float* mask,
                                float* out, float* dpred, float* scratch, int N, int64_t V, void* stream) {
    FDN_REQUIRE(pred && uh && vh && wh && mask && out && scratch && N > 0 && V > 0, "fdn_loss_metrics: bad argument");
    // (the extents only matter to the divergence pass, which div_w = 0 switches off)
    return loss_launch("fdn_loss_metrics", pred, uh, vh, wh, mask, out, dpred, scratch, N, V, 1, 1, 1, 0.f, 3, stream);
}

// The checks of the three entry points that take extents, under the called one's name, then the launches.  An entry point without kind,
// non_fluid_weight or out_act passes the value that means "as before" (FDN_LOSS_MSE and 0, 1, FDN_ACT_NONE), which passes its check.
static int loss_checked(const char* who, const float* pred, const float* uh, const float* vh, const float* wh, const float* mask, int kind,
                        float kind_param, float div_weight, float non_fluid_weight, int out_act, float* out, float* dpred, float* scratch, int N,
                        int D, int H, int W, void* stream) {
    FDN_REQUIRE(pred && uh && vh && wh && mask && out && scratch, "%s: NULL operand", who);
    FDN_REQUIRE(kind == FDN_LOSS_MSE || kind == FDN_LOSS_MAE || kind == FDN_LOSS_HUBER || kind == FDN_LOSS_CHARBONNIER,
                "%s: kind %d is not a loss (FDN_LOSS_MSE, _MAE, _HUBER or _CHARBONNIER)", who, kind);
    if (kind == FDN_LOSS_HUBER || kind == FDN_LOSS_CHARBONNIER)
        FDN_REQUIRE(__builtin_isfinite(kind_param) && kind_param > 0.f, "%s: %s %g must be finite and > 0", who,
                    kind == FDN_LOSS_HUBER ? "the Huber delta" : "the Charbonnier epsilon", (double)kind_param);
    else
        FDN_REQUIRE(kind_param == 0.f, "%s: %s takes no parameter, kind_param %g must be 0", who,
                    kind == FDN_LOSS_MSE ? "FDN_LOSS_MSE" : "FDN_LOSS_MAE", (double)kind_param);
    FDN_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "%s: extents N=%d D=%d H=%d W=%d must be positive", who, N, D, H, W);
    FDN_REQUIRE((int64_t)D * H * W <= (int64_t)INT32_MAX, "%s: %d x %d x %d voxels per sample exceed 2^31 - 1", who, D, H, W);
    FDN_REQUIRE(__builtin_isfinite(div_weight) && div_weight >= 0.f, "%s: div_weight %g must be finite and >= 0", who, (double)div_weight);
    FDN_REQUIRE(__builtin_isfinite(non_fluid_weight) && non_fluid_weight >= 0.f, "%s: non_fluid_weight %g must be finite and >= 0", who,
                (double)non_fluid_weight);
    if (out_act != FDN_ACT_NONE && out_act != FDN_ACT_TANH) {
        fdn_set_error("%s: out_act %d is not an activation of the heads (FDN_ACT_NONE or FDN_ACT_TANH)", who, out_act);
        return FDN_ERR_UNSUPPORTED;
    }
    return loss_launch(who, pred, uh, vh, wh, mask, out, dpred, scratch, N, (int64_t)D * H * W, D, H, W, div_weight, 5, stream, non_fluid_weight,
                       out_act, kind, kind_param);
}

extern "C" int fdn_loss_metrics_div(const float* pred, const float* uh, const float* vh, const float* wh, const float* mask,
                                    float div_weight, float* out, float* dpred, float* scratch, int N, int D, int H, int W,
                                    void* stream) {
    return loss_checked("fdn_loss_metrics_div", pred, uh, vh, wh, mask, FDN_LOSS_MSE, 0.f, div_weight, 1.f, FDN_ACT_NONE, out, dpred, scratch, N, D,
                        H, W, stream);
}

// the loss with the reference's non_fluid_weight and the heads' activation: the same three launches
extern "C" int fdn_loss_metrics_act(const float* pred, const float* uh, const float* vh, const float* wh, const float* mask,
                                    float div_weight, float non_fluid_weight, int out_act, float* out, float* dpred, float* scratch,
                                    int N, int D, int H, int W, void* stream) {
    return loss_checked("fdn_loss_metrics_act", pred, uh, vh, wh, mask, FDN_LOSS_MSE, 0.f, div_weight, non_fluid_weight, out_act, out, dpred,
                        scratch, N, D, H, W, stream);
}

// the data term under another penalty (FDN_LOSS_*): fdn_loss_metrics_act's checks, launches and buffers; FDN_LOSS_MSE is that call
extern "C" int fdn_loss_metrics_kind(const float* pred, const float* uh, const float* vh, const float* wh, const float* mask, int kind,
                                     float kind_param, float div_weight, float non_fluid_weight, int out_act, float* out, float* dpred,
                                     float* scratch, int N, int D, int H, int W, void* stream) {
    return loss_checked("fdn_loss_metrics_kind", pred, uh, vh, wh, mask, kind, kind_param, div_weight, non_fluid_weight, out_act, out, dpred,
                        scratch, N, D, H, W, stream);
}

extern "C" int fdn_volume_metrics(const void* pred, int pred_is_f64, const float* truth, const float* mask, int mask_frames,
                                  double* out, double* scratch, int F, int X, int Y, int Z, void* stream) {
    FDN_REQUIRE(pred, "fdn_volume_metrics: pred is NULL");
    FDN_REQUIRE(truth, "fdn_volume_metrics: truth is NULL");
    FDN_REQUIRE(mask, "fdn_volume_metrics: mask is NULL");
    FDN_REQUIRE(out, "fdn_volume_metrics: out is NULL");
    FDN_REQUIRE(scratch, "fdn_volume_metrics: scratch is NULL");
    FDN_REQUIRE(F > 0 && X > 0 && Y > 0 && Z > 0, "fdn_volume_metrics: extents F=%d X=%d Y=%d Z=%d must be positive", F, X, Y, Z);
    FDN_REQUIRE((int64_t)X * Y * Z <= (int64_t)INT32_MAX, "fdn_volume_metrics: X*Y*Z = %d x %d x %d voxels per frame exceed 2^31 - 1", X, Y,
                Z);
    FDN_REQUIRE(mask_frames == 1 || mask_frames == F, "fdn_volume_metrics: mask_frames=%d must be 1 or F=%d", mask_frames, F);
    FDN_REQUIRE(pred_is_f64 == 0 || pred_is_f64 == 1, "fdn_volume_metrics: pred_is_f64=%d must be 0 or 1", pred_is_f64);
    hipStream_t s = (hipStream_t)stream;
    const int gx = grid_for((int64_t)X * Y * Z, FDN_LOSS_BLOCKS);
    VolumeMetrics a{pred, truth, mask, scratch, out, 0, pred_is_f64, mask_frames != 1 ? 1 : 0, X, Y, Z};
    hipLaunchKernelGGL(volume_mask_sums_kernel, dim3(gx, F), dim3(256), 0, s, a);
    FDN_CHECK_LAUNCH("volume_mask_sums_kernel");
    for (a.pass = 1; a.pass <= 5; ++a.pass) {                            // columns 3-8, 9-10, then the five moments of u, v, w
        hipLaunchKernelGGL(volume_metrics_kernel, dim3(gx, F), dim3(256), 0, s, a);
        FDN_CHECK_LAUNCH("volume_metrics_kernel");
    }
    hipLaunchKernelGGL(volume_finalize_kernel, dim3(F), dim3(64), 0, s, a, gx);
    FDN_CHECK_LAUNCH("volume_finalize_kernel");
    return FDN_OK;
}

extern "C" int fdn_l2_sumsq(const float* w, const uint8_t* is_kernel, int64_t n, float* out, void* stream) {
    FDN_REQUIRE(w && is_kernel && out && n > 0, "fdn_l2_sumsq: bad argument");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(l2_sumsq_kernel, dim3(1), dim3(1024), 0, s, w, is_kernel, n, out);
    FDN_CHECK_LAUNCH("l2_sumsq_kernel");
    return FDN_OK;
}

extern "C" int fdn_l2_sumsq_partials(const float* w, const uint8_t* is_kernel, int64_t n, float* sumsq_partials, void* stream) {
    FDN_REQUIRE(w && is_kernel && sumsq_partials && n > 0, "fdn_l2_sumsq_partials: bad argument");
    hipLaunchKernelGGL(l2_sumsq_partials_kernel, dim3(FDN_ADAM_PARTIALS), dim3(256), 0, (hipStream_t)stream, w, is_kernel, n, sumsq_partials);
    FDN_CHECK_LAUNCH("l2_sumsq_partials_kernel");
    return FDN_OK;
}

// adam_kernel's parameters by name (the kernel keeps its flat list): an Adam entry point sets the options it has, the rest stay "absent".
struct AdamOperands {
    float *w = nullptr, *m = nullptr, *v = nullptr, *sumsq = nullptr, *ema = nullptr;
    const float *g = nullptr, *lr_t_dev = nullptr, *l2_scale_dev = nullptr, *g_scale_dev = nullptr;
    const uint8_t *is_kernel = nullptr, *frozen = nullptr;
    int64_t n = 0;
    float lr_t = 0.f, b1 = 0.f, b2 = 0.f, eps = 0.f, l2_grad_scale = 0.f, clip_value = 0.f, ema_momentum = 0.f;
    int ema_init = 0;
};

// The one place adam_kernel is launched from.
static int launch_adam(const AdamOperands& a, int grid, hipStream_t stream, const char* what) {
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, stream, a.w, a.g, a.m, a.v, a.is_kernel, a.n, a.lr_t, a.lr_t_dev, a.b1, a.b2,
                       a.eps, a.l2_grad_scale, a.l2_scale_dev, a.sumsq, a.frozen, a.g_scale_dev, a.clip_value,
                       a.ema, a.ema_momentum, a.ema_init);
    FDN_CHECK_LAUNCH(what);
    return FDN_OK;
}

// The grid of the four Adam steps: fixed at FDN_ADAM_PARTIALS blocks when partials are requested (blocks beyond the data write 0).
static int adam_step_grid(int64_t n, const float* sumsq_partials) { return sumsq_partials ? FDN_ADAM_PARTIALS : grid_for(n, 2048); }

extern "C" int fdn_adam_step(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, int64_t n, float lr_t,
                             float b1, float b2, float eps, float l2_grad_scale, const float* l2_scale_dev,
                             float* sumsq_partials, void* stream) {
    FDN_REQUIRE(w && g && m && v && is_kernel && n > 0, "fdn_adam_step: bad argument");
    AdamOperands a;
    a.w = w, a.g = g, a.m = m, a.v = v, a.is_kernel = is_kernel, a.n = n, a.b1 = b1, a.b2 = b2, a.eps = eps;
    a.l2_grad_scale = l2_grad_scale, a.l2_scale_dev = l2_scale_dev, a.sumsq = sumsq_partials, a.lr_t = lr_t;
    return launch_adam(a, adam_step_grid(n, sumsq_partials), (hipStream_t)stream, "adam_kernel");
}

extern "C" int fdn_adam_step_dev(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, int64_t n,
                                 const float* lr_t_dev, float b1, float b2, float eps, float l2_grad_scale,
                                 const float* l2_scale_dev, float* sumsq_partials, void* stream) {
    FDN_REQUIRE(w && g && m && v && is_kernel, "fdn_adam_step_dev: NULL operand");
    FDN_REQUIRE(lr_t_dev, "fdn_adam_step_dev: lr_t_dev is NULL (fdn_adam_step takes the step size by value)");
    FDN_REQUIRE(n > 0, "fdn_adam_step_dev: n=%lld must be positive", (long long)n);
    AdamOperands a;
    a.w = w, a.g = g, a.m = m, a.v = v, a.is_kernel = is_kernel, a.n = n, a.b1 = b1, a.b2 = b2, a.eps = eps;
    a.l2_grad_scale = l2_grad_scale, a.l2_scale_dev = l2_scale_dev, a.sumsq = sumsq_partials, a.lr_t_dev = lr_t_dev;
    return launch_adam(a, adam_step_grid(n, sumsq_partials), (hipStream_t)stream, "adam_kernel");
}

extern "C" int fdn_adam_step_masked(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, const uint8_t* frozen, int64_t n,
                                    float lr_t, const float* lr_t_dev, float b1, float b2, float eps, float l2_grad_scale,
                                    const float* l2_scale_dev, float* sumsq_partials, void* stream) {
    FDN_REQUIRE(w, "fdn_adam_step_masked: w is NULL");
    FDN_REQUIRE(g, "fdn_adam_step_masked: g is NULL");
    FDN_REQUIRE(m, "fdn_adam_step_masked: m is NULL");
    FDN_REQUIRE(v, "fdn_adam_step_masked: v is NULL");
    FDN_REQUIRE(is_kernel, "fdn_adam_step_masked: is_kernel is NULL");
    FDN_REQUIRE(frozen, "fdn_adam_step_masked: frozen is NULL (fdn_adam_step / fdn_adam_step_dev update every element)");
    FDN_REQUIRE(n > 0, "fdn_adam_step_masked: n=%lld must be positive", (long long)n);
    AdamOperands a;
    a.w = w, a.g = g, a.m = m, a.v = v, a.is_kernel = is_kernel, a.n = n, a.b1 = b1, a.b2 = b2, a.eps = eps;
    a.l2_grad_scale = l2_grad_scale, a.l2_scale_dev = l2_scale_dev, a.sumsq = sumsq_partials;
    a.lr_t = lr_t, a.lr_t_dev = lr_t_dev, a.frozen = frozen;
    return launch_adam(a, adam_step_grid(n, sumsq_partials), (hipStream_t)stream, "adam_kernel (masked)");
}

extern "C" int fdn_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream) {
    FDN_REQUIRE(acc, "fdn_grad_accumulate: acc is NULL");
    FDN_REQUIRE(g, "fdn_grad_accumulate: g is NULL");
    FDN_REQUIRE(n > 0, "fdn_grad_accumulate: n=%lld must be positive", (long long)n);
    FDN_REQUIRE(first == 0 || first == 1, "fdn_grad_accumulate: first=%d must be 0 or 1", first);
    // (compared as integers: the two pointers need not belong to one allocation; n floats from either never wrap, checked first)
    const uintptr_t a = (uintptr_t)acc, b = (uintptr_t)g, bytes = (uintptr_t)n * sizeof(float);
    FDN_REQUIRE((uint64_t)n <= (UINTPTR_MAX - (a > b ? a : b)) / sizeof(float), "fdn_grad_accumulate: n=%lld floats run past the address space", (long long)n);
    FDN_REQUIRE((a > b ? a - b : b - a) >= bytes, "fdn_grad_accumulate: acc and g overlap (%lld bytes apart, n=%lld floats): an in-place call would double the buffer",
                (long long)(a > b ? a - b : b - a), (long long)n);
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, acc, g, n, first);
    FDN_CHECK_LAUNCH("grad_accumulate_kernel");
    return FDN_OK;
}

extern "C" int fdn_sum_partials(const float* partials, int n, float* out, void* stream) {
    FDN_REQUIRE(partials && out && n > 0, "fdn_sum_partials: bad argument");
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n, out);
    FDN_CHECK_LAUNCH("sum_partials_kernel");
    return FDN_OK;
}

// Gradient clipping (tf.keras.optimizers.Adam(global_clipnorm= / clipvalue=), TrainerController.py:73): three launches -- the sum of
// squares of the step's gradient (grad_sumsq_partials_kernel), norm and scale (clip_scale_kernel), and the clipped step (adam_kernel).
// The scale stays on the device between the second and the third.
extern "C" int fdn_grad_sumsq_partials(const float* g, const float* w, const uint8_t* is_kernel, const uint8_t* frozen, int64_t n,
                                       float l2_grad_scale, const float* l2_scale_dev, float* partials, void* stream) {
    FDN_REQUIRE(g, "fdn_grad_sumsq_partials: g is NULL");
    FDN_REQUIRE(w, "fdn_grad_sumsq_partials: w is NULL");
    FDN_REQUIRE(is_kernel, "fdn_grad_sumsq_partials: is_kernel is NULL");
    FDN_REQUIRE(partials, "fdn_grad_sumsq_partials: partials is NULL");
    FDN_REQUIRE(n > 0, "fdn_grad_sumsq_partials: n=%lld must be positive", (long long)n);
    hipLaunchKernelGGL(grad_sumsq_partials_kernel, dim3(FDN_ADAM_PARTIALS), dim3(256), 0, (hipStream_t)stream, g, w, is_kernel, frozen, n,
                       l2_grad_scale, l2_scale_dev, partials);
    FDN_CHECK_LAUNCH("grad_sumsq_partials_kernel");
    return FDN_OK;
}

extern "C" int fdn_clip_scale(const float* partials, int n_partials, float clip_norm, float* out, void* stream) {
    FDN_REQUIRE(partials, "fdn_clip_scale: partials is NULL");
    FDN_REQUIRE(out, "fdn_clip_scale: out is NULL");
    FDN_REQUIRE(n_partials > 0, "fdn_clip_scale: n_partials=%d must be positive", n_partials);
    FDN_REQUIRE(__builtin_isfinite(clip_norm) && clip_norm > 0.f, "fdn_clip_scale: clip_norm=%g must be finite and > 0", (double)clip_norm);
    hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, out, clip_norm);
    FDN_CHECK_LAUNCH("clip_scale_kernel");
    return FDN_OK;
}

extern "C" int fdn_adam_step_clipped(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, const uint8_t* frozen, int64_t n,
                                     float lr_t, const float* lr_t_dev, float b1, float b2, float eps, float l2_grad_scale,
                                     const float* l2_scale_dev, const float* g_scale_dev, float clip_value, float* sumsq_partials,
                                     void* stream) {
    FDN_REQUIRE(w, "fdn_adam_step_clipped: w is NULL");
    FDN_REQUIRE(g, "fdn_adam_step_clipped: g is NULL");
    FDN_REQUIRE(m, "fdn_adam_step_clipped: m is NULL");
    FDN_REQUIRE(v, "fdn_adam_step_clipped: v is NULL");
    FDN_REQUIRE(is_kernel, "fdn_adam_step_clipped: is_kernel is NULL");
    FDN_REQUIRE(n > 0, "fdn_adam_step_clipped: n=%lld must be positive", (long long)n);
    FDN_REQUIRE(clip_value >= 0.f, "fdn_adam_step_clipped: clip_value=%g must be >= 0 (0 = off)", (double)clip_value);      // (false for NaN)
    AdamOperands a;
    a.w = w, a.g = g, a.m = m, a.v = v, a.is_kernel = is_kernel, a.n = n, a.b1 = b1, a.b2 = b2, a.eps = eps;
    a.l2_grad_scale = l2_grad_scale, a.l2_scale_dev = l2_scale_dev, a.sumsq = sumsq_partials;
    a.lr_t = lr_t, a.lr_t_dev = lr_t_dev, a.frozen = frozen, a.g_scale_dev = g_scale_dev, a.clip_value = clip_value;
    return launch_adam(a, adam_step_grid(n, sumsq_partials), (hipStream_t)stream, "adam_kernel (clipped)");
}

// Weight EMA (tf.keras.optimizers.Adam(use_ema=True, ema_momentum=)): the clipped step with the average as one more option of adam_kernel.
// The widest form: frozen, lr_t_dev, g_scale_dev and l2_scale_dev may be NULL, clip_value may be 0.
extern "C" int fdn_adam_step_ema(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, const uint8_t* frozen, int64_t n,
                                 float lr_t, const float* lr_t_dev, float b1, float b2, float eps, float l2_grad_scale,
                                 const float* l2_scale_dev, const float* g_scale_dev, float clip_value, float* ema, float ema_momentum,
                                 int ema_init, float* sumsq_partials, void* stream) {
    FDN_REQUIRE(w, "fdn_adam_step_ema: w is NULL");
    FDN_REQUIRE(g, "fdn_adam_step_ema: g is NULL");
    FDN_REQUIRE(m, "fdn_adam_step_ema: m is NULL");
    FDN_REQUIRE(v, "fdn_adam_step_ema: v is NULL");
    FDN_REQUIRE(is_kernel, "fdn_adam_step_ema: is_kernel is NULL");
    FDN_REQUIRE(ema, "fdn_adam_step_ema: ema is NULL (fdn_adam_step_clipped is the step without an average)");
    FDN_REQUIRE(n > 0, "fdn_adam_step_ema: n=%lld must be positive", (long long)n);
    FDN_REQUIRE(ema_momentum >= 0.f && ema_momentum < 1.f, "fdn_adam_step_ema: ema_momentum=%g must lie in [0, 1)", (double)ema_momentum);  // (false for NaN)
    FDN_REQUIRE(clip_value >= 0.f, "fdn_adam_step_ema: clip_value=%g must be >= 0 (0 = off)", (double)clip_value);          // (false for NaN)
    AdamOperands a;
    a.w = w, a.g = g, a.m = m, a.v = v, a.is_kernel = is_kernel, a.n = n, a.b1 = b1, a.b2 = b2, a.eps = eps;
    a.l2_grad_scale = l2_grad_scale, a.l2_scale_dev = l2_scale_dev, a.sumsq = sumsq_partials;
    a.lr_t = lr_t, a.lr_t_dev = lr_t_dev, a.frozen = frozen, a.g_scale_dev = g_scale_dev, a.clip_value = clip_value;
    a.ema = ema, a.ema_momentum = ema_momentum, a.ema_init = ema_init != 0;
    return launch_adam(a, adam_step_grid(n, sumsq_partials), (hipStream_t)stream, "adam_kernel (ema)");
}

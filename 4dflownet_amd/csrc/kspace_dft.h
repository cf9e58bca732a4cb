// Low-res synthesis on the device (prepare_data/fft_downsampling.py:6-137): the stage of fdn_kspace_downsample, the body of
// kspace_stage_kernel<inverse> (kspace.hip).
//
// Per axis the reference's fftn -> fftshift -> centre crop -> fftshift is ONE truncated DFT: with half = N / 2, c the crop half-width and
// M = 2c, output k' in 0..M-1 is frequency k = k' (k' < c) or k' - M (else), F[k'] = sum_n x[n] exp(-2 pi i ((k n) mod N) / N), and the
// cropped ifftn is z[m] = (1/M) sum_k' F[k'] exp(+2 pi i ((k' m) mod M) / M).  The volumes are small (84 x 76 x 72 -> 42 x 38 x 36: 39 M
// complex multiply-adds), so a stage is a plain VALU sum, one output element per thread and step, walking one axis of a (outer, N, inner)
// array with the N (or M) unit roots in dynamic LDS: entry r = sincospif(2.f * r / N), the index (k n) mod N kept in integers.
//   forward:  first = 1 forms x = mag * mag_scale * exp(i pi vel / venc) on the way in (sincospif(vel / venc): the reduction by pi
//             is exact, |vel| > venc wraps as in the reference); last = 1 leaves one partial sum of |F|^2 per workgroup.
//   inverse:  first = 1 reads sigma = sqrtf(sum|F|^2 / count / snr_linear) on the device and adds sigma * g to Re F on the way in
//             (real noise on the complex spectrum, fft_downsampling.py:63-69); last = 1 writes |z| * ratio and
//             atan2(Im z, Re z) / pi * venc instead of z.
// blockIdx.y is the volume of the batch; blockIdx.x strides over that volume's outputs.
#pragma once
#include "fdn_common.h"

#define FDN_KS_MAX_EXTENT 1024        // per axis: the twiddle table is at most 8 KB of LDS
#define FDN_KS_MAX_BLOCKS 128         // workgroups per volume and stage (every thread strides over the volume's outputs)

struct KspaceGeom {
    const void* in0;                            // first forward stage: vel (nvol,X,Y,Z) fp32; else the stage's input (nvol, outer, N, inner), complex fp32
    const float* in1;                           // first forward stage: mag (X,Y,Z); first inverse stage: the noise (nvol,Mx,My,Mz) or NULL
    void* out0;                                 // the stage's output (nvol, outer, M, inner), complex fp32; last inverse stage: out_vel
    float* out1;                                // last forward stage: partials (nvol, gridDim.x); first inverse: sigma_out or NULL; last inverse: out_mag
    const float* params;                        // (nvol,4): venc, mag_scale, snr_linear, 0
    const float* sums;                          // first inverse stage: sum |F|^2 per volume
    uint64_t seed, stream_id;
    int32_t outer, inner;
    int32_t N, M, c;                            // input extent, output extent and crop half-width along the axis (inverse: N == M)
    int32_t first, last;
    float count, ratio;                         // Mx My Mz, and Mx My Mz / (X Y Z)
};

// Philox4x32-10 (Salmon et al., SC'11), words 0 and 1 of the output block, as a standard normal by Box-Muller:
// counter (e lo, e hi, stream lo, stream hi), key (seed lo, seed hi); u1 = ((x0 >> 9) + 0.5) 2^-23 in (0,1), u2 = (x1 >> 8) 2^-24 in [0,1).
__device__ __forceinline__ float fdn_ks_normal(uint64_t e, uint64_t seed, uint64_t stream) {
    uint32_t c0 = (uint32_t)e, c1 = (uint32_t)(e >> 32), c2 = (uint32_t)stream, c3 = (uint32_t)(stream >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const float u1 = ((float)(c0 >> 9) + 0.5f) * 0x1p-23f, u2 = (float)(c1 >> 8) * 0x1p-24f;
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// lds: 2 * max(N, M) floats of twiddles, then 4 floats for the workgroup's sum.  256 threads.
template <bool inverse> __device__ __forceinline__ void fdn_ks_stage(const KspaceGeom& g, float* lds) {
    float2* tw = (float2*)lds;
    const int N = g.N, M = g.M, inner = g.inner;
    for (int r = threadIdx.x; r < N; r += 256) {
        float s, c;
        sincospif(2.f * r / N, &s, &c);
        tw[r] = make_float2(c, inverse ? s : -s);
    }
    __syncthreads();
    const int v = blockIdx.y;
    const int line = M * inner;                                         // <= 2^30, like the two below: 32-bit indices inside a volume
    const int per = g.outer * line;                                     // this stage's outputs per volume
    const int per_in = g.outer * N * inner;                             // and its inputs
    const float venc = g.params[4 * v], mag_scale = g.params[4 * v + 1];
    float sigma = 0.f;
    if (inverse && g.first) {
        sigma = sqrtf(g.sums[v] / g.count / g.params[4 * v + 2]);
        if (g.out1 && blockIdx.x == 0 && threadIdx.x == 0) g.out1[v] = sigma;
    }
    const float scale = inverse ? 1.f / (float)M : 1.f;
    float ss = 0.f;
    const float* in0 = (const float*)g.in0 + (int64_t)v * per_in * (!inverse && g.first ? 1 : 2);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256) {
        const int o = i / line, rem = i - o * line;
        const int kp = rem / inner;
        const int k = inverse || kp < g.c ? kp : kp - M + N;            // the frequency mod N
        int s = o * N * inner + rem - kp * inner;                       // element n = 0 of the line inside its volume
        int idx = 0;
        float ar = 0.f, ai = 0.f;
        for (int n = 0; n < N; ++n, s += inner) {
            float xr, xi;
            if (!inverse && g.first) {
                float sn, cs;
                sincospif(in0[s] / venc, &sn, &cs);
                const float m = g.in1[s] * mag_scale;
                xr = m * cs; xi = m * sn;
            } else {
                const float2 x = ((const float2*)in0)[s];
                xr = x.x; xi = x.y;
                if (inverse && g.first) {
                    const int64_t e = (int64_t)v * per_in + s;          // the element's index in the call's (nvol,Mx,My,Mz) array
                    xr += sigma * (g.in1 ? g.in1[e] : fdn_ks_normal((uint64_t)e, g.seed, g.stream_id));
                }
            }
            const float2 t = tw[idx];
            ar += xr * t.x - xi * t.y;
            ai += xr * t.y + xi * t.x;
            idx += k;
            if (idx >= N) idx -= N;
        }
        ar *= scale; ai *= scale;
        const int64_t d = (int64_t)v * per + i;
        if (inverse && g.last) {
            g.out1[d] = sqrtf(ar * ar + ai * ai) * g.ratio;
            ((float*)g.out0)[d] = atan2f(ai, ar) / 3.14159265358979323846f * venc;
        } else {
            ((float2*)g.out0)[d] = make_float2(ar, ai);
        }
        ss += ar * ar + ai * ai;
    }
    if (!inverse && g.last) {                                           // block-uniform: the sum of this workgroup, in a fixed order
        float* red = lds + 2 * N;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
        __syncthreads();
        if (threadIdx.x == 0) g.out1[(int64_t)v * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// How v_mfma_f32_16x16x32_bf16 rounds D = C + sum_k a_k b_k when the products lie far below C (the situation of the bf16 x 3 Winograd
// products, FDN_ALGO_WINO_BF16X3: the five small cross terms are added to an accumulator that holds hi.hi).  Every lane holds the same eight
// (a_j, b_j) pairs, so each of the 256 outputs is C + 4 sum_j a_j b_j, with exact bf16 operands chosen to put the exact sum at a known
// fraction of an ulp of C.  Printed per case: (D - C) / ulp(C) beside what round-to-nearest-even of the exact sum gives.  Then four equal
// products of 2^-s ulp of C in all (the smallest product the accumulate still sees), and the signed error D - exact on random operands
// whose products lie 2^0 .. 2^-24 below C, C of either sign (argument: cases per row; 8000000 resolves 0.0005 ulp).
// Found on gfx950 (profiles/mfma_bf16_rounding.txt): not an fma chain -- every product is cut at the last place of the largest addend, and
// with products 2^-16 .. 2^-20 below C the result is low by 0.006 .. 0.008 ulp on average whatever the sign of C.
//   hipcc --offload-arch=gfx950 -O2 tools/mfma_bf16_rounding.hip -o mfma_bf16_rounding && ./mfma_bf16_rounding 8000000
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
struct Case { float c; float a[8]; float b[8]; };

__global__ __launch_bounds__(64) void k(const Case* cs, float* out) {
    const Case& q = cs[blockIdx.x];
    bf16x8 av, bv;
    for (int j = 0; j < 8; ++j) { av[j] = (__bf16)q.a[j]; bv[j] = (__bf16)q.b[j]; }
    f32x4 acc = {q.c, q.c, q.c, q.c};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) out[(blockIdx.x * 64 + threadIdx.x) * 4 + r] = acc[r];
}

__global__ __launch_bounds__(64) void k1(const Case* cs, float* out) {           // one output per case
    const Case& q = cs[blockIdx.x];
    bf16x8 av, bv;
    for (int j = 0; j < 8; ++j) { av[j] = (__bf16)q.a[j]; bv[j] = (__bf16)q.b[j]; }
    f32x4 acc = {q.c, q.c, q.c, q.c};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
    if (threadIdx.x == 0) out[blockIdx.x] = acc[0];
}

int main(int argc, char** argv) {
    const int kMax = 128;
    static Case cs[kMax];
    static double frac[kMax];              // exact sum of the products in ulps of C
    int n = 0;
    const float ulp = ldexpf(1.f, -23);    // of 1.5
    auto add = [&](float c, int quarters, int tiny_exp, int tiny_sign) {
        // quarters / 4 ulp of C from |quarters| pairs whose product is +-2^-27: each pair occurs at four k, 4 x 2^-27 = 1/4 ulp
        Case& q = cs[n];
        q.c = c;
        for (int j = 0; j < 8; ++j) { q.a[j] = 0.f; q.b[j] = 0.f; }
        const int m = quarters < 0 ? -quarters : quarters;
        for (int j = 0; j < m; ++j) { q.a[j] = ldexpf(1.f, -13); q.b[j] = ldexpf(quarters < 0 ? -1.f : 1.f, -14); }     // 4 x 2^-27 = 2^-25 = 1/4 ulp each
        double f = 0.25 * quarters;
        if (tiny_sign) { q.a[7] = ldexpf(1.f, -13); q.b[7] = ldexpf((float)tiny_sign, -14 - tiny_exp); f += tiny_sign * 0.25 * ldexp(1.0, -tiny_exp); }
        frac[n++] = f;
    };
    for (float c : {1.5f, -1.5f})
        for (int qt : {1, 2, 3, -1, -2, -3, 5, -5, 6, -6}) add(c, qt, 0, 0);
    for (float c : {1.5f, -1.5f})
        for (int g : {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 40})
            for (int s : {1, -1}) { add(c, 2, g, s); add(c, -2, g, s); }     // a tie plus / minus 2^-(g+2) ulp: which guard bits survive
    Case* d; float* o;
    hipMalloc(&d, sizeof(Case) * n); hipMalloc(&o, sizeof(float) * n * 256);
    hipMemcpy(d, cs, sizeof(Case) * n, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(n), dim3(64), 0, 0, d, o);
    static float h[kMax * 256];
    if (hipMemcpy(h, o, sizeof(float) * n * 256, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
    printf("# D = v_mfma_f32_16x16x32_bf16(A, B, C): C, exact sum of products [ulp of C], (D - C) / ulp, round-to-nearest-even, verdict\n");
    int off = 0;
    for (int i = 0; i < n; ++i) {
        bool same = true;
        for (int e = 1; e < 256; ++e) same = same && h[i * 256 + e] == h[i * 256];
        const double got = ((double)h[i * 256] - cs[i].c) / ulp;
        double want = nearbyint(frac[i]);                                  // ties to even: C = +-1.5 has an even last bit
        if (fabs(frac[i] - trunc(frac[i])) == 0.5) want = frac[i] > 0 ? floor(frac[i]) : ceil(frac[i]);
        if (fmod(fabs(want), 2.0) == 1.0 && fabs(frac[i]) - floor(fabs(frac[i])) == 0.5) want = frac[i] > 0 ? ceil(frac[i]) : floor(frac[i]);
        off += got != want;
        printf("%+.1f %+.12f %+.0f %+.0f %s%s\n", cs[i].c, frac[i], got, want, got == want ? "rne" : (got < want ? "BELOW" : "ABOVE"), same ? "" : " (outputs differ)");
    }
    printf("# %d of %d cases differ from round-to-nearest-even of the exact sum\n", off, n);
    // one product (x 4) of 2^-s ulp: the smallest product the accumulate still sees
    n = 0;
    for (float c : {1.5f, -1.5f})
        for (int s = -2; s <= 8; ++s)
            for (float sg : {1.f, -1.f}) {
                Case& q = cs[n];
                q.c = c;
                for (int j = 0; j < 8; ++j) { q.a[j] = 0.f; q.b[j] = 0.f; }
                q.a[0] = ldexpf(1.f, -12); q.b[0] = ldexpf(sg, -13 - s);          // 4 x 2^(-25-s) = 2^(-23-s)
                frac[n++] = sg * ldexp(1.0, -s);
            }
    hipMemcpy(d, cs, sizeof(Case) * n, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(n), dim3(64), 0, 0, d, o);
    if (hipMemcpy(h, o, sizeof(float) * n * 256, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
    printf("# four equal products, 2^-s ulp of C in all: C, exact sum [ulp], (D - C) / ulp\n");
    for (int i = 0; i < n; ++i) printf("%+.1f %+.6f %+.3f\n", cs[i].c, frac[i], ((double)h[i * 256] - cs[i].c) / ulp);
    // random operands: 8 random bf16 pairs (x 4) whose products are 2^-shift of C, C random in +-[1, 2): the signed error in ulps of D
    const int kRand = argc > 1 ? atoi(argv[1]) : 200000;           // cases per row
    Case* rc = new Case[kRand];
    float* rh = new float[kRand];
    Case* rd; float* ro;
    hipMalloc(&rd, sizeof(Case) * kRand); hipMalloc(&ro, sizeof(float) * kRand);
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (unsigned)(st >> 20); };
    auto bf = [&](int e) { return ldexpf((rnd() & 1 ? 1.f : -1.f) * (128 + rnd() % 128), e - 7); };       // 8 significant bits
    printf("# random operands: products / C, mean (D - exact) [ulp of D], mean (RNE(exact) - exact), share of D == RNE(exact), share of D below / above RNE(exact), the mean by sign of C, mean |D - exact|; %d cases per row\n", kRand);
    for (int shift : {0, 4, 8, 12, 16, 20, 24}) {
        for (int i = 0; i < kRand; ++i) {
            rc[i].c = ldexpf((rnd() & 1 ? 1.f : -1.f) * ((1u << 23) + rnd() % (1u << 23)), -23);
            for (int j = 0; j < 8; ++j) { rc[i].a[j] = bf(-2); rc[i].b[j] = bf(-shift - 2); }                 // |a b| in [2^-4, 2^-2) 2^-shift, 32 of them
        }
        hipMemcpy(rd, rc, sizeof(Case) * kRand, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k1, dim3(kRand), dim3(64), 0, 0, rd, ro);
        if (hipMemcpy(rh, ro, sizeof(float) * kRand, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
        double me = 0, mr = 0, mp = 0, mn = 0, ma = 0; int eq = 0, below = 0, above = 0, np = 0;
        for (int i = 0; i < kRand; ++i) {
            double ex = rc[i].c;
            for (int j = 0; j < 8; ++j) ex += 4.0 * (double)rc[i].a[j] * (double)rc[i].b[j];      // exact in double (<= 40 significant bits)
            const float r = (float)ex, g = rh[i];
            const double u = ldexp(1.0, ilogb(fabs(ex)) - 23);
            me += (g - ex) / u; mr += (r - ex) / u; ma += fabs(g - ex) / u;
            if (rc[i].c > 0) { mp += (g - ex) / u; ++np; } else mn += (g - ex) / u;
            eq += g == r; below += g < r; above += g > r;
        }
        printf("2^-%-2d %+.5f %+.5f %.4f %.4f %.4f  C > 0: %+.5f  C < 0: %+.5f  mean |D - exact| %.4f\n", shift, me / kRand, mr / kRand, (double)eq / kRand,
               (double)below / kRand, (double)above / kRand, mp / np, mn / (kRand - np), ma / kRand);
    }
    return 0;
}

// Low-res synthesis on the device (prepare_data/fft_downsampling.py:6-137): fdn_kspace_downsample as six launches of the truncated-DFT
// stage of kspace_dft.h -- three forward, three inverse -- the only kernels of the library launched with dynamic LDS (the twiddle table).
#include "fdn_common.h"
#include "kspace_dft.h"

// One stage along one axis, driven by the by-value KspaceGeom: blockIdx.y is the volume of the batch, blockIdx.x strides over its outputs.
template <bool inverse> __global__ __launch_bounds__(256) void kspace_stage_kernel(KspaceGeom kg) {
    extern __shared__ __attribute__((aligned(16))) float ks_lds[];
    fdn_ks_stage<inverse>(kg, ks_lds);
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
    struct Stage { bool inverse; int N, M, c, outer, inner; const void* in0; const float* in1; void* out0; float* out1; int first, last; };
    const Stage st[6] = {{false, X, Mx, cx, 1, Y * Z, vel, mag, A, nullptr, 1, 0},
                         {false, Y, My, cy, Mx, Z, A, nullptr, B, nullptr, 0, 0},
                         {false, Z, Mz, cz, Mx * My, 1, B, nullptr, A, partials, 0, 1},
                         {true, Mx, Mx, 0, 1, My * Mz, A, noise, B, sigma_out, 1, 0},
                         {true, My, My, 0, Mx, Mz, B, nullptr, A, nullptr, 0, 0},
                         {true, Mz, Mz, 0, Mx * My, 1, A, nullptr, out_vel, out_mag, 0, 1}};
    for (const Stage& s : st) {
        g.N = s.N; g.M = s.M; g.c = s.c; g.outer = s.outer; g.inner = s.inner; g.in0 = s.in0; g.in1 = s.in1; g.out0 = s.out0; g.out1 = s.out1;
        g.first = s.first; g.last = s.last;
        const unsigned nb = ks_blocks((int64_t)s.outer * s.M * s.inner);
        const unsigned lds = (unsigned)(2 * s.N + 4) * sizeof(float);
        hipLaunchKernelGGL(s.inverse ? kspace_stage_kernel<true> : kspace_stage_kernel<false>, dim3(nb, (unsigned)nvol), dim3(256), lds,
                           (hipStream_t)stream, g);
        FDN_CHECK_LAUNCH("kspace_stage_kernel");
        if (!s.inverse && s.last)                           // sum |F|^2 per volume: the partials in a fixed order (sum_partials_kernel)
            for (int v = 0; v < nvol; ++v) {
                const int rc = fdn_sum_partials(partials + (size_t)v * nb, (int)nb, sums + v, stream);
                if (rc != FDN_OK) return rc;
            }
    }
    return FDN_OK;
}

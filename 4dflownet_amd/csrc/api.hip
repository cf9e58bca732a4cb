// extern "C" boundary of lib4dflow_hip.so: argument validation, shape dispatch, error reporting.
// See include/fdn.h for the contract and the reference call sites each entry point replaces.
#include <stdarg.h>
#include <stdio.h>
#include <algorithm>
#include <mutex>
#include <set>
#include <string>
#include <string.h>
#include <type_traits>
#include <utility>
#include "fdn_common.h"
#include "thin_layers.h"
#include "wgrad64_plan.h"

static thread_local char g_err[512] = "";

void fdn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int fdn_func_max_lds(const void* fn, int bytes, const char* who) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;       // (device, kernel) pairs whose attribute is set
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({dev, fn})) return FDN_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) { fdn_set_error("%s: hipFuncSetAttribute(%d B of LDS): %s", who, bytes, hipGetErrorString(e)); return FDN_ERR_HIP; }
    done.insert({dev, fn});
    return FDN_OK;
}

FDN_HOOK_VAR(int, fdn_wgrad64_force_direct, 0);
#ifdef FDN_TEST_HOOKS
extern "C" int fdn_debug_set_wgrad64_direct(int on) { fdn_wgrad64_force_direct = on; return FDN_OK; }

// the launch-plan recorder (fdn_common.h: FDN_PLAN)
static std::mutex g_plan_mu;
static std::string g_plan_log;
static bool g_plan_on = false;

void fdn_plan_note(const char* fmt, ...) {
    std::lock_guard<std::mutex> lock(g_plan_mu);
    if (!g_plan_on) return;
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof(line), fmt, ap);
    va_end(ap);
    g_plan_log += line;
    g_plan_log += '\n';
}

int fdn_plan_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
}

// on != 0: start recording (and drop what was recorded); 0: stop
extern "C" int fdn_debug_plan_log(int on) {
    std::lock_guard<std::mutex> lock(g_plan_mu);
    g_plan_on = on != 0;
    if (g_plan_on) g_plan_log.clear();
    return FDN_OK;
}

// copies the recorded lines (NUL-terminated) into buf and clears the record when n > their length; returns that length either way
extern "C" size_t fdn_debug_plan_read(char* buf, size_t n) {
    std::lock_guard<std::mutex> lock(g_plan_mu);
    const size_t len = g_plan_log.size();
    if (buf && n > len) {
        memcpy(buf, g_plan_log.data(), len);
        buf[len] = 0;
        g_plan_log.clear();
    }
    return len;
}
#endif

extern "C" int fdn_version(void) { return FDN_VERSION; }   // 161: fdn_conv64_dgrad_fused_multi; 160: FDN_CONV64_PACK_FLOATS = 423 * 4096 (+ the bf16 x 3 stream), FDN_ALGO_WINO_BF16X3
extern "C" const char* fdn_last_error(void) { return g_err; }

// An operator that exists once per storage type (fdn_x / fdn_x_bf16) has ONE body below: a static function template on T = float /
// uint16_t (bf16 bits) that takes the called entry point's name as `who`; the extern "C" twins forward to it.  Where the two modes
// differ, the difference stands where it occurs: an `if constexpr (kBf16<T>)` or the overload pair wgrad64_launch.  The bf16 entry
// points take no algo and pass FDN_ALGO_AUTO.
template <typename T> constexpr bool kBf16 = sizeof(T) == 2;

// The 64->64 entry points: the checks they share, and their call descriptors -- a forward over the (N, D, H, W) grid, or a dgrad
// (op FDN_CONV64_DGRAD[_FUSED]) onto its padded (D+2, H+2, W+2) grid.  mask_act: act must be one a sign mask belongs to.  limit: the
// largest extent (1020: what a padded grid and the mask forms address; the plain forwards take 1022)
static int conv64_check(const char* who, int algo, int N, int D, int H, int W, int act, bool mask_act = false, int limit = 1020) {
    FDN_REQUIRE(algo >= FDN_ALGO_AUTO && algo <= FDN_ALGO_LAST, "%s: bad algo %d", who, algo);
    FDN_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && D <= limit && H <= limit && W <= limit, "%s: bad dims", who);
    if (mask_act) FDN_REQUIRE(act == FDN_ACT_RELU || act == FDN_ACT_LEAKY, "%s: a mask belongs to an activation (act %d)", who, act);
    else FDN_REQUIRE(act >= FDN_ACT_NONE && act <= FDN_ACT_LEAKY, "%s: bad act %d", who, act);
    return FDN_OK;
}

// what every call says: FdnConv64Call for float rows, FdnConv64BfCall for bf16 ones; the entry point adds the output and its own operands
template <typename T>
static std::conditional_t<kBf16<T>, FdnConv64BfCall, FdnConv64Call> conv64_call(FdnConv64Op op, const T* x, const T* wpack, int N, int D, int H,
                                                                                int W, int act, float alpha, void* stream) {
    const int pad = op == FDN_CONV64_FWD ? 0 : 2;
    std::conditional_t<kBf16<T>, FdnConv64BfCall, FdnConv64Call> c;
    c.op = op; c.x = x; c.wpack = wpack;
    c.N = N; c.ID = D; c.IH = H; c.IW = W; c.OD = D + pad; c.OH = H + pad; c.OW = W + pad;
    c.act = act; c.alpha = alpha; c.s = (hipStream_t)stream;
    return c;
}

// the checked 64->64 forward of either storage type; ymask: also write the sign mask of the output.  fp32 routes by algo, bf16 has one kernel
template <typename T>
static int conv64_fwd_launch(const T* x, const T* wpack, const float* bias, const T* residual, T* y, uint16_t* ymask, int N, int D, int H, int W,
                             int act, float alpha, int algo, void* stream) {
    auto c = conv64_call(FDN_CONV64_FWD, x, wpack, N, D, H, W, act, alpha, stream);
    c.y = y; c.bias = bias; c.residual = residual; c.ymask = ymask;
    if constexpr (kBf16<T>) return fdn_conv64_bf16_launch(c);
    else return fdn_conv64_launch_ex(c, 3, algo);
}

// y: T rows, except the heads' (Cout == 1) fp32 prediction in both modes
template <typename T>
static int conv3d_fwd(const char* who, const T* x, const T* x2, const float* w, const T* wpack, const float* bias, const T* residual, void* y,
                      int N, int D, int H, int W, int Cin, int Cout, int K, int ldy, int y_coff, int act, float alpha, int algo, void* stream) {
    FDN_REQUIRE(x && y, "%s: x/y is NULL", who);
    FDN_REQUIRE(algo >= FDN_ALGO_AUTO && algo <= FDN_ALGO_LAST, "%s: bad algo %d", who, algo);
    FDN_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims N=%d D=%d H=%d W=%d", who, N, D, H, W);
    // (FDN_ACT_TANH: the heads' route alone; elsewhere it is the bad act it was before it had a name)
    FDN_REQUIRE(act >= FDN_ACT_NONE && act <= ((Cin == 64 && Cout == 1 && K == 3) ? FDN_ACT_TANH : FDN_ACT_LEAKY),
                "%s: bad act %d%s", who, act, act == FDN_ACT_TANH ? " (FDN_ACT_TANH is the output activation of the (64,1,3) route only)" : "");
    hipStream_t s = (hipStream_t)stream;
    if (Cin == 64 && Cout == 64 && K == 3) {
        FDN_REQUIRE(wpack, "%s: the 64->64 MFMA path needs wpack (fdn_pack_conv64_weights%s)", who, kBf16<T> ? "_bf16" : "");
        FDN_REQUIRE(ldy == 64 && y_coff == 0, "%s: 64->64 path writes dense rows (ldy=64,y_coff=0)", who);
        FDN_REQUIRE(D <= 1022 && H <= 1022 && W <= 1022, "%s: dims too large", who);
        return conv64_fwd_launch(x, wpack, bias, residual, (T*)y, nullptr, N, D, H, W, act, alpha, algo, stream);
    }
    FDN_REQUIRE(residual == nullptr, "%s: residual only on the 64->64 path", who);
    if (Cin == 3 && Cout == 64 && K == 3) {
        FDN_REQUIRE(w && ldy == 64 && y_coff == 0, "%s(3->64): needs w, dense output", who);
        return fdn_conv_cin3_fwd_launch<T>(x, w, bias, (T*)y, N, D, H, W, act, alpha, s);
    }
    if (Cin == 64 && Cout == 1 && K == 3) {
        FDN_REQUIRE(w && ldy >= 1 && y_coff >= 0 && y_coff < ldy, "%s(64->1): bad w/ldy/y_coff", who);
        return fdn_conv_cout1_fwd_launch<T>(x, w, bias, (float*)y, N, D, H, W, ldy, y_coff, act, alpha, s);
    }
    if (Cin == 128 && Cout == 64 && K == 1) {
        FDN_REQUIRE(w && x2 && ldy == 64 && y_coff == 0, "%s(1x1 128->64): needs w, x2, dense output", who);
        return fdn_conv1x1_fwd_launch<T>(x, x2, w, bias, (T*)y, (int64_t)N * D * H * W, act, alpha, s);
    }
    fdn_set_error("%s: unsupported (Cin=%d,Cout=%d,K=%d)", who, Cin, Cout, K);
    return FDN_ERR_UNSUPPORTED;
}
extern "C" int fdn_conv3d_fwd(const float* x, const float* x2, const float* w, const float* wpack, const float* bias,
                              const float* residual, float* y, int N, int D, int H, int W, int Cin, int Cout, int K,
                              int ldy, int y_coff, int act, float alpha, int algo, void* stream) {
    return conv3d_fwd<float>("fdn_conv3d_fwd", x, x2, w, wpack, bias, residual, y, N, D, H, W, Cin, Cout, K, ldy, y_coff, act, alpha, algo, stream);
}
extern "C" int fdn_conv3d_fwd_bf16(const uint16_t* x, const uint16_t* x2, const float* w, const uint16_t* wpack,
                                   const float* bias, const uint16_t* residual, void* y, int N, int D, int H, int W, int Cin,
                                   int Cout, int K, int ldy, int y_coff, int act, float alpha, void* stream) {
    return conv3d_fwd<uint16_t>("fdn_conv3d_fwd_bf16", x, x2, w, wpack, bias, residual, y, N, D, H, W, Cin, Cout, K, ldy, y_coff, act, alpha,
                                FDN_ALGO_AUTO, stream);
}

extern "C" int fdn_conv3d_dgrad(const float* dz, const float* w, const float* wpack, float* dxpad, int N, int D,
                                int H, int W, int Cin, int Cout, int K, int lddz, int dz_coff, int algo, void* stream) {
    FDN_REQUIRE(dz && dxpad, "fdn_conv3d_dgrad: dz/dxpad is NULL");
    FDN_REQUIRE(algo >= FDN_ALGO_AUTO && algo <= FDN_ALGO_LAST, "fdn_conv3d_dgrad: bad algo %d", algo);
    FDN_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "fdn_conv3d_dgrad: bad dims");
    hipStream_t s = (hipStream_t)stream;
    if (Cin == 64 && Cout == 64 && K == 3) {
        FDN_REQUIRE(wpack, "fdn_conv3d_dgrad: the 64->64 MFMA path needs wpack = wp_dgrad");
        FDN_REQUIRE(lddz == 64 && dz_coff == 0, "fdn_conv3d_dgrad: 64->64 path reads dense rows");
        FDN_REQUIRE(D <= 1020 && H <= 1020 && W <= 1020, "fdn_conv3d_dgrad: dims too large");
        FdnConv64Call c = conv64_call(FDN_CONV64_DGRAD, dz, wpack, N, D, H, W, FDN_ACT_NONE, 0.f, stream);
        c.y = dxpad;
        return fdn_conv64_launch_ex(c, 3, algo);
    }
    if (Cin == 64 && Cout == 1 && K == 3) {
        FDN_REQUIRE(w, "fdn_conv3d_dgrad(64->1): needs w");
        return fdn_conv_cout1_dgrad_launch(dz, w, dxpad, N, D, H, W, lddz, dz_coff, s);
    }
    fdn_set_error("fdn_conv3d_dgrad: unsupported (Cin=%d,Cout=%d,K=%d)", Cin, Cout, K);
    return FDN_ERR_UNSUPPORTED;
}

extern "C" int fdn_conv3d_dgrad_fused(const float* dz, const float* wpack, float* dxpad, const float* skip,
                                      const float* y_prev, int act, float alpha, float* dz_prev, int N, int D, int H,
                                      int W, int algo, void* stream) {
    FDN_REQUIRE(dz && wpack && dxpad && dz_prev, "fdn_conv3d_dgrad_fused: NULL argument");
    if (int rc = conv64_check("fdn_conv3d_dgrad_fused", algo, N, D, H, W, act)) return rc;
    FdnConv64Call c = conv64_call(FDN_CONV64_DGRAD_FUSED, dz, wpack, N, D, H, W, act, alpha, stream);
    c.y = dxpad; c.fskip = skip; c.fy = y_prev; c.fout = dz_prev;
    return fdn_conv64_launch_ex(c, 3, algo);
}

// 64->64 forward that also writes the sign mask of its output, and the fused dgrad that reads the mask instead of y_prev (conv64_wino2d_kernel.h)
extern "C" int fdn_conv64_fwd_mask(const float* x, const float* wpack, const float* bias, const float* residual, float* y, uint16_t* y_mask,
                                   int N, int D, int H, int W, int act, float alpha, int algo, void* stream) {
    FDN_REQUIRE(x && wpack && y && y_mask, "fdn_conv64_fwd_mask: NULL argument");
    if (int rc = conv64_check("fdn_conv64_fwd_mask", algo, N, D, H, W, act)) return rc;
    return conv64_fwd_launch(x, wpack, bias, residual, y, y_mask, N, D, H, W, act, alpha, algo, stream);
}

extern "C" int fdn_conv64_dgrad_fused_mask(const float* dz, const float* wpack, float* dxpad, const float* skip, const uint16_t* y_mask,
                                           int act, float alpha, float* dz_prev, int N, int D, int H, int W, int algo, void* stream) {
    FDN_REQUIRE(dz && wpack && dxpad && dz_prev && y_mask, "fdn_conv64_dgrad_fused_mask: NULL argument");
    if (int rc = conv64_check("fdn_conv64_dgrad_fused_mask", algo, N, D, H, W, act, true)) return rc;
    FdnConv64Call c = conv64_call(FDN_CONV64_DGRAD_FUSED, dz, wpack, N, D, H, W, act, alpha, stream);
    c.y = dxpad; c.fskip = skip; c.fmask = y_mask; c.fout = dz_prev;
    return fdn_conv64_launch_ex(c, 3, algo);
}

extern "C" int fdn_conv64_dgrad_fused_multi(const float* const* dz, const float* const* wpack, int nsrc, float* dxpad, const float* skip,
                                            const float* y_prev, const uint16_t* y_mask, int act, float alpha, float* dz_prev, int N, int D,
                                            int H, int W, int algo, void* stream) {
    FDN_REQUIRE(dz && wpack && dxpad && dz_prev && nsrc >= 1 && nsrc <= 3, "fdn_conv64_dgrad_fused_multi: NULL argument or nsrc outside 1..3");
    if (int rc = conv64_check("fdn_conv64_dgrad_fused_multi", algo, N, D, H, W, act)) return rc;
    FDN_REQUIRE(!(y_mask && y_prev), "fdn_conv64_dgrad_fused_multi: y_prev OR its sign mask");
    FDN_REQUIRE(!y_mask || act == FDN_ACT_RELU || act == FDN_ACT_LEAKY, "fdn_conv64_dgrad_fused_multi: a mask belongs to an activation (act %d)", act);
    // the kernels address the further sources' weight streams as non-negative byte distances from source 0's: order by pack address
    // (the sum over the sources is formed in that order)
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < nsrc; ++i) FDN_REQUIRE(dz[i] && wpack[i], "fdn_conv64_dgrad_fused_multi: NULL pointer for source %d", i);
    for (int i = 1; i < nsrc; ++i)
        for (int j = i; j > 0 && wpack[ord[j]] < wpack[ord[j - 1]]; --j) { const int t = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = t; }
    FdnConv64Call c = conv64_call(FDN_CONV64_DGRAD_FUSED, dz[ord[0]], wpack[ord[0]], N, D, H, W, act, alpha, stream);
    c.y = dxpad; c.fskip = skip; c.fy = y_prev; c.fmask = y_mask; c.fout = dz_prev; c.nsrc = nsrc;
    for (int i = 1; i < nsrc; ++i) {
        const long long d = (long long)(wpack[ord[i]] - wpack[ord[0]]) * (long long)sizeof(float);
        FDN_REQUIRE(d >= 0 && d < (1ll << 30), "fdn_conv64_dgrad_fused_multi: the packs of the sources must lie within 1 GiB of each other (one fdn_pack_conv64_weights_batch buffer)");
        if (i == 1) { c.x1 = dz[ord[1]]; c.wd1 = (int)d; } else { c.x2 = dz[ord[2]]; c.wd2 = (int)d; }
    }
    return fdn_conv64_launch_ex(c, 3, algo);
}

extern "C" int fdn_conv3d_dgrad_fused_part(const float* dz, const float* wpack, float* dxpad, const float* skip,
                                           const float* y_prev, int act, float alpha, float* dz_prev, int N, int D, int H,
                                           int W, int parts, int algo, void* stream) {
    FDN_REQUIRE(dz && wpack && dxpad && dz_prev, "fdn_conv3d_dgrad_fused_part: NULL argument");
    if (int rc = conv64_check("fdn_conv3d_dgrad_fused_part", algo, N, D, H, W, act)) return rc;
    FDN_REQUIRE(parts >= 1 && parts <= 3, "fdn_conv3d_dgrad_fused_part: parts must be FDN_DGRAD_INNER | FDN_DGRAD_SHELL");
    FdnConv64Call c = conv64_call(FDN_CONV64_DGRAD_FUSED, dz, wpack, N, D, H, W, act, alpha, stream);
    c.y = dxpad; c.fskip = skip; c.fy = y_prev; c.fout = dz_prev;
    return fdn_conv64_launch_ex(c, parts, algo);
}

// ---- the bf16 64->64 entry points.  Unlike the fp32 ones they allow a NULL mask with any act (one entry point takes y_prev and the
// mask), refuse a mask with FDN_ACT_NONE, and hand the sources of a multi-source dgrad over as given ----
static int conv64_fwd_bf16(const char* who, const uint16_t* x, const uint16_t* wpack, const float* bias, const uint16_t* residual, uint16_t* y,
                           uint16_t* y_mask, int N, int D, int H, int W, int act, float alpha, void* stream) {
    FDN_REQUIRE(x && wpack && y, "%s: NULL argument", who);
    if (int rc = conv64_check(who, FDN_ALGO_AUTO, N, D, H, W, act, false, 1022)) return rc;
    return conv64_fwd_launch(x, wpack, bias, residual, y, y_mask, N, D, H, W, act, alpha, FDN_ALGO_AUTO, stream);
}
extern "C" int fdn_conv64_fwd_bf16_mask(const uint16_t* x, const uint16_t* wpack, const float* bias, const uint16_t* residual,
                                        uint16_t* y, uint16_t* y_mask, int N, int D, int H, int W, int act, float alpha, void* stream) {
    return conv64_fwd_bf16("fdn_conv64_fwd_bf16_mask", x, wpack, bias, residual, y, y_mask, N, D, H, W, act, alpha, stream);
}
extern "C" int fdn_conv64_fwd_bf16(const uint16_t* x, const uint16_t* wpack, const float* bias, const uint16_t* residual,
                                   uint16_t* y, int N, int D, int H, int W, int act, float alpha, void* stream) {
    return conv64_fwd_bf16("fdn_conv64_fwd_bf16", x, wpack, bias, residual, y, nullptr, N, D, H, W, act, alpha, stream);
}

// the fused dgrad of nsrc = 1..3 sources: the single-source entry points are tables of one
static int conv64_dgrad_fused_bf16(const char* who, const uint16_t* const* dz, const uint16_t* const* wpack, int nsrc, float* dxpad,
                                   const uint16_t* skip, const uint16_t* y_prev, const uint16_t* y_mask, int act, float alpha,
                                   uint16_t* dz_prev, int N, int D, int H, int W, void* stream) {
    FDN_REQUIRE(dz && wpack && dxpad && dz_prev && nsrc >= 1 && nsrc <= 3, "%s: NULL argument or nsrc outside 1..3", who);
    if (int rc = conv64_check(who, FDN_ALGO_AUTO, N, D, H, W, act)) return rc;
    FDN_REQUIRE(!(y_mask && act == FDN_ACT_NONE), "%s: a sign mask needs act = RELU or LEAKY", who);
    for (int i = 0; i < nsrc; ++i) FDN_REQUIRE(dz[i] && wpack[i], "%s: NULL pointer for source %d", who, i);
    FdnConv64BfCall c = conv64_call(FDN_CONV64_DGRAD_FUSED, dz[0], wpack[0], N, D, H, W, act, alpha, stream);
    c.ypad = dxpad; c.fskip = skip; c.fy = y_prev; c.fmask = y_mask; c.fout = dz_prev; c.nsrc = nsrc;
    if (nsrc > 1) { c.x1 = dz[1]; c.wp1 = wpack[1]; }
    if (nsrc > 2) { c.x2 = dz[2]; c.wp2 = wpack[2]; }
    return fdn_conv64_bf16_launch(c);
}
extern "C" int fdn_conv64_dgrad_fused_bf16_mask(const uint16_t* dz, const uint16_t* wpack, float* dxpad, const uint16_t* skip,
                                                const uint16_t* y_prev, const uint16_t* y_mask, int act, float alpha,
                                                uint16_t* dz_prev, int N, int D, int H, int W, void* stream) {
    return conv64_dgrad_fused_bf16("fdn_conv64_dgrad_fused_bf16_mask", &dz, &wpack, 1, dxpad, skip, y_prev, y_mask, act, alpha, dz_prev, N, D, H, W, stream);
}
extern "C" int fdn_conv64_dgrad_fused_bf16(const uint16_t* dz, const uint16_t* wpack, float* dxpad, const uint16_t* skip,
                                           const uint16_t* y_prev, int act, float alpha, uint16_t* dz_prev, int N, int D,
                                           int H, int W, void* stream) {
    return conv64_dgrad_fused_bf16("fdn_conv64_dgrad_fused_bf16", &dz, &wpack, 1, dxpad, skip, y_prev, nullptr, act, alpha, dz_prev, N, D, H, W, stream);
}
extern "C" int fdn_conv64_dgrad_fused_bf16_multi(const uint16_t* const* dz, const uint16_t* const* wpack, int nsrc, float* dxpad,
                                                 const uint16_t* skip, const uint16_t* y_prev, const uint16_t* y_mask, int act, float alpha,
                                                 uint16_t* dz_prev, int N, int D, int H, int W, void* stream) {
    return conv64_dgrad_fused_bf16("fdn_conv64_dgrad_fused_bf16_multi", dz, wpack, nsrc, dxpad, skip, y_prev, y_mask, act, alpha, dz_prev, N, D, H, W, stream);
}

// ---- the thin operators ----
template <typename T>
static int fold_halo_border(const char* who, const float* dxpad0, const float* dxpad1, const float* dxpad2, int nsrc, const T* skip,
                            const T* y_prev, int act, float alpha, T* dz_prev, int N, int D, int H, int W, void* stream) {
    FDN_REFUSE_TANH(act, who);
    FDN_REQUIRE(dxpad0 && dz_prev, "%s: NULL argument", who);
    FDN_REQUIRE(nsrc >= 1 && nsrc <= 3 && (nsrc < 2 || dxpad1) && (nsrc < 3 || dxpad2), "%s: bad nsrc %d", who, nsrc);
    FDN_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims", who);
    return fdn_fold_halo_border_launch(dxpad0, dxpad1, dxpad2, nsrc, skip, y_prev, act, alpha, dz_prev, N, D, H, W, (hipStream_t)stream);
}
extern "C" int fdn_fold_halo_border(const float* dxpad0, const float* dxpad1, const float* dxpad2, int nsrc,
                                    const float* skip, const float* y_prev, int act, float alpha, float* dz_prev, int N,
                                    int D, int H, int W, void* stream) {
    return fold_halo_border<float>("fdn_fold_halo_border", dxpad0, dxpad1, dxpad2, nsrc, skip, y_prev, act, alpha, dz_prev, N, D, H, W, stream);
}
extern "C" int fdn_fold_halo_border_bf16(const float* dxpad0, const float* dxpad1, const float* dxpad2, int nsrc,
                                         const uint16_t* skip, const uint16_t* y_prev, int act, float alpha,
                                         uint16_t* dz_prev, int N, int D, int H, int W, void* stream) {
    return fold_halo_border<uint16_t>("fdn_fold_halo_border_bf16", dxpad0, dxpad1, dxpad2, nsrc, skip, y_prev, act, alpha, dz_prev, N, D, H, W, stream);
}

template <typename T>
static int conv1x1_dgrad(const char* who, const T* dz, const float* w, const T* ya, const T* yb, T* dxa, T* dxb, int64_t nvox, void* stream) {
    FDN_REQUIRE(dz && w && ya && yb && dxa && dxb && nvox > 0, "%s: NULL argument or nvox<=0", who);
    return fdn_conv1x1_dgrad_launch<T>(dz, w, ya, yb, dxa, dxb, nvox, (hipStream_t)stream);
}
extern "C" int fdn_conv1x1_dgrad(const float* dz, const float* w, const float* ya, const float* yb, float* dxa, float* dxb,
                                 int64_t nvox, void* stream) {
    return conv1x1_dgrad<float>("fdn_conv1x1_dgrad", dz, w, ya, yb, dxa, dxb, nvox, stream);
}
extern "C" int fdn_conv1x1_dgrad_bf16(const uint16_t* dz, const float* w, const uint16_t* ya, const uint16_t* yb,
                                      uint16_t* dxa, uint16_t* dxb, int64_t nvox, void* stream) {
    return conv1x1_dgrad<uint16_t>("fdn_conv1x1_dgrad_bf16", dz, w, ya, yb, dxa, dxb, nvox, stream);
}

// The head's dgrad with the fold: act' from y_prev or from its sign mask.  fp32 has an entry point for either (mask_form: the mask
// and its activation are required), bf16 one that takes both pointers.  The launcher checks the operands and the workspace under `who`.
template <typename T>
static int conv_cout1_dgrad_folded(const char* who, bool mask_form, const float* dz, const float* w, const T* y_prev, const uint16_t* y_mask,
                                   int act, float alpha, T* dz_prev, float* dbias_prev, void* workspace, size_t workspace_bytes, int N,
                                   int D, int H, int W, int lddz, int dz_coff, void* stream) {
    if (mask_form) FDN_REQUIRE(y_mask && (act == FDN_ACT_RELU || act == FDN_ACT_LEAKY), "%s: a sign mask and act = RELU or LEAKY", who);
    else FDN_REQUIRE(!(y_mask && act == FDN_ACT_NONE), "%s: a sign mask needs act = RELU or LEAKY", who);
    FDN_REFUSE_TANH(act, who);
    return fdn_conv_cout1_dgrad_folded_launch<T>(who, dz, w, y_prev, act, alpha, dz_prev, dbias_prev, workspace, workspace_bytes, N, D, H, W,
                                                 lddz, dz_coff, (hipStream_t)stream, y_mask);
}
extern "C" int fdn_conv_cout1_dgrad_folded(const float* dz, const float* w, const float* y_prev, int act, float alpha,
                                           float* dz_prev, float* dbias_prev, void* workspace, size_t workspace_bytes, int N,
                                           int D, int H, int W, int lddz, int dz_coff, void* stream) {
    return conv_cout1_dgrad_folded<float>("fdn_conv_cout1_dgrad_folded", false, dz, w, y_prev, nullptr, act, alpha, dz_prev, dbias_prev, workspace,
                                          workspace_bytes, N, D, H, W, lddz, dz_coff, stream);
}
extern "C" int fdn_conv_cout1_dgrad_folded_mask(const float* dz, const float* w, const uint16_t* y_mask, int act, float alpha,
                                                float* dz_prev, float* dbias_prev, void* workspace, size_t workspace_bytes, int N,
                                                int D, int H, int W, int lddz, int dz_coff, void* stream) {
    return conv_cout1_dgrad_folded<float>("fdn_conv_cout1_dgrad_folded_mask", true, dz, w, nullptr, y_mask, act, alpha, dz_prev, dbias_prev,
                                          workspace, workspace_bytes, N, D, H, W, lddz, dz_coff, stream);
}
extern "C" int fdn_conv_cout1_dgrad_folded_bf16_mask(const float* dz, const float* w, const uint16_t* y_prev, const uint16_t* y_mask,
                                                     int act, float alpha, uint16_t* dz_prev, float* dbias_prev, void* workspace,
                                                     size_t workspace_bytes, int N, int D, int H, int W, int lddz, int dz_coff,
                                                     void* stream) {
    return conv_cout1_dgrad_folded<uint16_t>("fdn_conv_cout1_dgrad_folded_bf16_mask", false, dz, w, y_prev, y_mask, act, alpha, dz_prev, dbias_prev,
                                             workspace, workspace_bytes, N, D, H, W, lddz, dz_coff, stream);
}
extern "C" int fdn_conv_cout1_dgrad_folded_bf16(const float* dz, const float* w, const uint16_t* y_prev, int act, float alpha,
                                                uint16_t* dz_prev, float* dbias_prev, void* workspace, size_t workspace_bytes,
                                                int N, int D, int H, int W, int lddz, int dz_coff, void* stream) {
    return conv_cout1_dgrad_folded<uint16_t>("fdn_conv_cout1_dgrad_folded_bf16", false, dz, w, y_prev, nullptr, act, alpha, dz_prev, dbias_prev,
                                             workspace, workspace_bytes, N, D, H, W, lddz, dz_coff, stream);
}

// ---- weight gradients ----
// The 64->64 layers: fdn_wgrad64_plan (wgrad64_plan.h) decides kernels, chunks, splits and workspace; here the plan is walked.
static FdnWgrad64Hooks wgrad64_hooks() {
    FdnWgrad64Hooks hk;
    hk.force_direct = fdn_wgrad64_force_direct; hk.wino_nodep = fdn_wgrad64_wino_nodep_hook(); hk.bf16_variant = fdn_wgrad64_bf16_variant_hook();
    return hk;
}
static int wgrad64_step_launch(const FdnWgrad64Step& st, const float* const* x, const float* const* dz, float* const* dw, void* ws, size_t ws_bytes,
                               int N, int D, int H, int W, hipStream_t s) {
    return st.route == FDN_WG_DIRECT ? fdn_wgrad64_launch(st, x[0], dz[0], dw[0], ws, ws_bytes, N, D, H, W, s)
                                     : fdn_wgrad64_wino_launch(st, x, dz, dw, ws, ws_bytes, N, D, H, W, s);
}
static int wgrad64_step_launch(const FdnWgrad64Step& st, const uint16_t* const* x, const uint16_t* const* dz, float* const* dw, void* ws,
                               size_t ws_bytes, int N, int D, int H, int W, hipStream_t s) {
    return fdn_wgrad64_bf16_launch(st, x, dz, dw, ws, ws_bytes, N, D, H, W, s);
}
// every step of a plan in order, each reusing the workspace behind the one before (stream order); x, dz, dw: the tables of all layers
template <typename T>
static int wgrad64_walk(const char* who, const FdnWgrad64Plan& plan, const T* const* x, const T* const* dz, float* const* dw, void* ws,
                        size_t ws_bytes, int N, int D, int H, int W, hipStream_t s) {
    FDN_REQUIRE(plan.addr32_ok, "wgrad64: x of %dx%dx%dx%dx64 floats exceeds the 32-bit buffer addressing", N, D, H, W);
    for (const FdnWgrad64Step& st : plan.steps) {
        if (st.count == 1) FDN_REQUIRE(x[st.first] && dz[st.first] && dw[st.first], "%s: NULL pointer for layer %d", who, st.first);
        if (int rc = wgrad64_step_launch(st, x + st.first, dz + st.first, dw + st.first, ws, ws_bytes, N, D, H, W, s)) return rc;
    }
    return FDN_OK;
}

template <typename T>
static size_t conv3d_wgrad_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int K) {
    if (!(Cin == 64 && Cout == 64 && K == 3)) return fdn_small_wgrad_workspace_bytes(Cin, Cout, K);
    return fdn_wgrad64_bound(kBf16<T>, N, D, H, W);
}
extern "C" size_t fdn_conv3d_wgrad_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int K) {
    return conv3d_wgrad_workspace_bytes<float>(N, D, H, W, Cin, Cout, K);
}
extern "C" size_t fdn_conv3d_wgrad_bf16_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int K) {
    return conv3d_wgrad_workspace_bytes<uint16_t>(N, D, H, W, Cin, Cout, K);
}

// dz: T rows, except the heads' (Cout == 1) fp32 prediction gradient in both modes
template <typename T>
static int conv3d_wgrad(const char* who, const T* x, const T* x2, const void* dz, float* dw, float* dbias, void* workspace,
                        size_t workspace_bytes, int N, int D, int H, int W, int Cin, int Cout, int K, int lddz, int dz_coff, int algo,
                        void* stream) {
    FDN_REQUIRE(x && dz && dw, "%s: x/dz/dw is NULL", who);
    FDN_REQUIRE(algo >= FDN_ALGO_AUTO && algo <= FDN_ALGO_LAST, "%s: bad algo %d", who, algo);
    FDN_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims", who);
    const size_t need = conv3d_wgrad_workspace_bytes<T>(N, D, H, W, Cin, Cout, K);
    if (workspace_bytes < need || (need && !workspace)) {
        fdn_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
        return FDN_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const T* dzt = (const T*)dz;
    int rc;
    if (Cin == 64 && Cout == 1 && K == 3) {
        const float* dzf = (const float*)dz;
        rc = fdn_wgrad_cout1_launch<T>(x, dzf, dw, workspace, workspace_bytes, N, D, H, W, lddz, dz_coff, s);
        if (rc != FDN_OK || !dbias) return rc;
        return fdn_bias_grad_launch<float>(dzf, dbias, workspace, workspace_bytes, N, D, H, W, 1, lddz, dz_coff, s);
    }
    if (Cin == 64 && Cout == 64 && K == 3) {
        FDN_REQUIRE(lddz == 64 && dz_coff == 0, "%s: 64->64 path reads dense dz rows", who);
        rc = wgrad64_walk<T>(who, fdn_wgrad64_plan(kBf16<T>, 1, N, D, H, W, algo, wgrad64_hooks()), &x, &dzt, &dw, workspace, workspace_bytes, N, D, H, W, s);
    } else if (Cin == 3 && Cout == 64 && K == 3) {
        FDN_REQUIRE(lddz == 64 && dz_coff == 0, "%s(3->64): dense dz rows", who);
        rc = fdn_wgrad_cin3_launch<T>(x, dzt, dw, workspace, workspace_bytes, N, D, H, W, s);
    } else if (Cin == 128 && Cout == 64 && K == 1) {
        FDN_REQUIRE(x2 && lddz == 64 && dz_coff == 0, "%s(1x1): needs x2, dense dz rows", who);
        rc = fdn_wgrad_1x1_launch<T>(x, x2, dzt, dw, workspace, workspace_bytes, N, D, H, W, s);
    } else {
        fdn_set_error("%s: unsupported (Cin=%d,Cout=%d,K=%d)", who, Cin, Cout, K);
        return FDN_ERR_UNSUPPORTED;
    }
    if (rc != FDN_OK || !dbias) return rc;
    return fdn_bias_grad_launch<T>(dzt, dbias, workspace, workspace_bytes, N, D, H, W, Cout, lddz, dz_coff, s);
}
extern "C" int fdn_conv3d_wgrad(const float* x, const float* x2, const float* dz, float* dw, float* dbias,
                                void* workspace, size_t workspace_bytes, int N, int D, int H, int W, int Cin, int Cout,
                                int K, int lddz, int dz_coff, int algo, void* stream) {
    return conv3d_wgrad<float>("fdn_conv3d_wgrad", x, x2, dz, dw, dbias, workspace, workspace_bytes, N, D, H, W, Cin, Cout, K, lddz, dz_coff, algo, stream);
}
extern "C" int fdn_conv3d_wgrad_bf16(const uint16_t* x, const uint16_t* x2, const void* dz, float* dw, float* dbias,
                                     void* workspace, size_t workspace_bytes, int N, int D, int H, int W, int Cin, int Cout,
                                     int K, int lddz, int dz_coff, void* stream) {
    return conv3d_wgrad<uint16_t>("fdn_conv3d_wgrad_bf16", x, x2, dz, dw, dbias, workspace, workspace_bytes, N, D, H, W, Cin, Cout, K, lddz, dz_coff,
                                  FDN_ALGO_AUTO, stream);
}

// Weight gradients of n_layers 64->64 3x3x3 layers that share one grid: in batched launches (+ one reduction launch each) where the plan
// allows it, else layer by layer.  The batched fp32 kernel gives every layer 64 / layers splits of the voxel sum where the single-layer
// launch uses 64: equal to fp32 rounding, not bit for bit.
extern "C" size_t fdn_conv3d_wgrad_batch_workspace_bytes(int n_layers, int N, int D, int H, int W) {
    return fdn_wgrad64_batch_bound(false, n_layers, N, D, H, W, wgrad64_hooks());
}
extern "C" size_t fdn_conv3d_wgrad_bf16_batch_workspace_bytes(int n_layers, int N, int D, int H, int W) {
    return fdn_wgrad64_batch_bound(true, n_layers, N, D, H, W, wgrad64_hooks());
}

template <typename T>
static int conv3d_wgrad_batch(const char* who, const T* const* x, const T* const* dz, float* const* dw, float* const* dbias, int n_layers,
                              void* workspace, size_t workspace_bytes, int N, int D, int H, int W, int algo, void* stream) {
    FDN_REQUIRE(x && dz && dw && n_layers > 0, "%s: NULL table or n_layers <= 0", who);
    FDN_REQUIRE(algo >= FDN_ALGO_AUTO && algo <= FDN_ALGO_LAST, "%s: bad algo %d", who, algo);
    FDN_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims", who);
    const size_t need = fdn_wgrad64_batch_bound(kBf16<T>, n_layers, N, D, H, W, wgrad64_hooks());
    if (workspace_bytes < need || !workspace) {
        fdn_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
        return FDN_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const FdnWgrad64Plan plan = fdn_wgrad64_plan(kBf16<T>, n_layers, N, D, H, W, algo, wgrad64_hooks());
    if (int rc = wgrad64_walk<T>(who, plan, x, dz, dw, workspace, workspace_bytes, N, D, H, W, s)) return rc;
    if (dbias)                           // (stream-ordered behind the reduction: the workspace is free again)
        for (int i = 0; i < n_layers; ++i)
            if (dbias[i])
                if (int rc = fdn_bias_grad_launch<T>(dz[i], dbias[i], workspace, workspace_bytes, N, D, H, W, 64, 64, 0, s)) return rc;
    return FDN_OK;
}
extern "C" int fdn_conv3d_wgrad_batch(const float* const* x, const float* const* dz, float* const* dw, float* const* dbias, int n_layers,
                                      void* workspace, size_t workspace_bytes, int N, int D, int H, int W, int algo, void* stream) {
    return conv3d_wgrad_batch<float>("fdn_conv3d_wgrad_batch", x, dz, dw, dbias, n_layers, workspace, workspace_bytes, N, D, H, W, algo, stream);
}
extern "C" int fdn_conv3d_wgrad_bf16_batch(const uint16_t* const* x, const uint16_t* const* dz, float* const* dw, float* const* dbias,
                                           int n_layers, void* workspace, size_t workspace_bytes, int N, int D, int H, int W, void* stream) {
    return conv3d_wgrad_batch<uint16_t>("fdn_conv3d_wgrad_bf16_batch", x, dz, dw, dbias, n_layers, workspace, workspace_bytes, N, D, H, W,
                                        FDN_ALGO_AUTO, stream);
}

#ifdef FDN_TEST_HOOKS
// The plan of a call as text, one line per step and a last line with the plan's workspace_bytes, under the hooks as they are set; needs no
// device.  Returns the length of the text; it is written (NUL-terminated) when n exceeds that length.
extern "C" int fdn_debug_wgrad64_plan(int bf16, int n_layers, int N, int D, int H, int W, int algo, char* buf, size_t n) {
    const FdnWgrad64Plan plan = fdn_wgrad64_plan(bf16 != 0, n_layers, N, D, H, W, algo, wgrad64_hooks());
    std::string text;
    char line[256];
    for (const FdnWgrad64Step& st : plan.steps) {
        snprintf(line, sizeof(line), "route=%s first=%d count=%d splits=%d planes=%d grid=%d tiles=%d nseg=%d seg_len=%d partial_bytes=%zu\n",
                 fdn_wgrad64_route_name(st.route), st.first, st.count, st.splits, st.planes, st.grid, st.tiles, st.nseg, st.seg_len, st.partial_bytes);
        text += line;
    }
    snprintf(line, sizeof(line), "workspace_bytes=%zu addr32_ok=%d\n", plan.workspace_bytes, (int)plan.addr32_ok);
    text += line;
    if (buf && n > text.size()) memcpy(buf, text.c_str(), text.size() + 1);
    return (int)text.size();
}
#endif

// The thin layers -- the 3->64 input convs, the 1x1 (64+64)->64 fuse, the three 64->1 heads and the bias gradients -- between their
// translation units: the one declaration of every launcher that api.hip, small_convs.hip, cin3_mfma.hip, conv1x1_mfma.hip and
// heads_mfma.hip share, and fdn_thin_partials, the one place that says how many partial rows a launch writes into the caller's workspace.
// The launchers take their grid from it and check the workspace against it, the size query promises kThinRowsMax rows, and the
// static_asserts below hold every cap to that -- so no launch outgrows the bytes the query promised (tests/test_thin_partials.py, without a GPU).
#pragma once
#include "fdn_common.h"

// ---- partial rows (host only: no HIP calls, no globals) ----
constexpr int kThinRowsMax = 768;            // rows fdn_small_wgrad_workspace_bytes promises to every weight gradient and its bias gradient
constexpr int kThinBlocks = 512;             // the VALU weight gradients, the 3->64 MFMA one and the C = 1 bias gradient: two workgroups per CU
constexpr int kHeadWgradRowsF32 = 512;       // head_wgrad_kernel, persistent: two workgroups per CU for fp32 storage (54.5 KB of LDS) ...
constexpr int kHeadWgradRowsBf16 = 768;      // ... three for bf16 (37.6 KB, 153 VGPRs)
constexpr int kWgrad1x1Rows = 256;           // wgrad_1x1_mfma_kernel: one workgroup per CU (128 KB of LDS for the cross-wave sum)
constexpr int kBias64Rows = 256;             // bias_grad_kernel, C = 64
constexpr int kHeadDbiasRowsMax = 2048;      // rows of 64 floats include/fdn.h states for fdn_conv_cout1_dgrad_folded's dbias_prev
constexpr int kHeadDbiasRows = 1024;         // head_dgrad_kernel, persistent
constexpr int kHeadDbiasRowsValu = 2048;     // conv_cout1_dgrad_folded_kernel (test build)
static_assert(kThinBlocks <= kThinRowsMax && kHeadWgradRowsF32 <= kThinRowsMax && kHeadWgradRowsBf16 <= kThinRowsMax &&
              kWgrad1x1Rows <= kThinRowsMax && kBias64Rows <= kThinRowsMax, "a thin weight or bias gradient outgrows the size query");
static_assert(kHeadDbiasRows <= kHeadDbiasRowsMax && kHeadDbiasRowsValu <= kHeadDbiasRowsMax, "dbias_prev outgrows the rows fdn.h states");

// tiles of the three head kernels (heads_mfma.hip): 4 x 8 x 8 voxels
constexpr int kHeadTD = 4, kHeadTH = 8, kHeadTW = 8;
struct FdnHeadTiles {
    int ntd, nth, ntw;
    long long tiles;
    FdnHeadTiles(int N, int D, int H, int W)
        : ntd((D + kHeadTD - 1) / kHeadTD), nth((H + kHeadTH - 1) / kHeadTH), ntw((W + kHeadTW - 1) / kHeadTW), tiles((long long)N * ntd * nth * ntw) {}
};

enum FdnThinOp {
    FDN_THIN_WGRAD_CIN3,        // 3->64 weight gradient: rows of 81 * 64
    FDN_THIN_WGRAD_COUT1,       // 64->1 (head) weight gradient: 27 * 64
    FDN_THIN_WGRAD_1X1,         // 1x1 (64+64)->64 weight gradient: 128 * 64
    FDN_THIN_BIAS64,            // bias gradient of a 64-channel layer: 64
    FDN_THIN_BIAS1,             // ... of a head: 1
    FDN_THIN_HEAD_DBIAS,        // dbias_prev of the head's folded dgrad: 64
    FDN_THIN_OPS
};

struct FdnThinPartials {
    int rows, row_floats;
    size_t bytes() const { return (size_t)rows * row_floats * sizeof(float); }
};

// workgroups of a grid-stride launch: ceil(items / per_block) within 1 .. cap
inline int fdn_blocks_for(int64_t items, int per_block, int cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// The partial rows one launch of `op` over the (N, D, H, W) grid writes (= its grid) and their length.  mfma: the state of the op's
// fdn_*_use_mfma hook -- always on in the product library; off, the test build's VALU kernel runs.  Pure.
inline FdnThinPartials fdn_thin_partials(FdnThinOp op, bool bf16, int N, int D, int H, int W, bool mfma) {
    const int64_t nvox = (int64_t)N * D * H * W;
    auto least = [](long long a, long long cap) { return (int)(a < cap ? a : cap); };
    switch (op) {
    case FDN_THIN_WGRAD_CIN3: return {fdn_blocks_for(nvox, 4 * 32, kThinBlocks), 81 * 64};
    case FDN_THIN_WGRAD_COUT1:          // MFMA: one row per workgroup of the persistent grid; VALU: per (n, d, h) row of the padded grid
        if (mfma) return {least(FdnHeadTiles(N, D, H, W).tiles, bf16 ? kHeadWgradRowsBf16 : kHeadWgradRowsF32), 27 * 64};
        return {least((long long)N * (D + 2) * (H + 2), kThinBlocks), 27 * 64};
    case FDN_THIN_WGRAD_1X1:            // MFMA: >= 64 voxel pairs per wave
        if (mfma) return {fdn_blocks_for(nvox / 2, 256, kWgrad1x1Rows), 128 * 64};
        return {fdn_blocks_for(nvox, 32 * 4, kThinBlocks), 128 * 64};
    case FDN_THIN_BIAS64: return {fdn_blocks_for(nvox, 4 * 64, kBias64Rows), 64};
    case FDN_THIN_BIAS1: return {fdn_blocks_for(nvox, 256 * 16, kThinBlocks), 1};
    case FDN_THIN_HEAD_DBIAS:
        if (mfma) return {least(FdnHeadTiles(N, D, H, W).tiles, kHeadDbiasRows), 64};
        return {least((long long)N * D * H, kHeadDbiasRowsValu), 64};
    case FDN_THIN_OPS: break;
    }
    return {0, 0};
}

// what fdn_conv3d_wgrad[_bf16]_workspace_bytes answer off the 64->64 route: kThinRowsMax rows of the weights (>= 64 floats: the bias rows)
size_t fdn_small_wgrad_workspace_bytes(int Cin, int Cout, int K);

// ---- launchers of small_convs.hip, as api.hip calls them.  Templated on the activation storage type T (float, or uint16_t = bf16 bits);
// parameters, parameter gradients, the heads' output (the prediction) and its gradient are always fp32.  A launcher with (ws, ws_bytes)
// writes fdn_thin_partials rows there and answers FDN_ERR_WORKSPACE when they do not fit ----
template <typename T> int fdn_conv_cin3_fwd_launch(const T* x, const float* w, const float* bias, T* y, int N, int D, int H, int W, int act,
                                                   float alpha, hipStream_t s);
template <typename T> int fdn_conv_cout1_fwd_launch(const T* x, const float* w, const float* bias, float* y, int N, int D, int H, int W, int ldy,
                                                    int y_coff, int act, float alpha, hipStream_t s);
template <typename T> int fdn_conv1x1_fwd_launch(const T* xa, const T* xb, const float* w, const float* bias, T* y, int64_t nvox, int act,
                                                 float alpha, hipStream_t s);
template <typename T> int fdn_conv1x1_dgrad_launch(const T* dz, const float* w, const T* ya, const T* yb, T* dxa, T* dxb, int64_t nvox,
                                                   hipStream_t s);
int fdn_conv_cout1_dgrad_launch(const float* dz, const float* w, float* dxpad, int N, int D, int H, int W, int lddz, int dz_coff, hipStream_t s);
template <typename T> int fdn_wgrad_cin3_launch(const T* x, const T* dz, float* dw, void* ws, size_t ws_bytes, int N, int D, int H, int W,
                                                hipStream_t s);
template <typename T> int fdn_wgrad_cout1_launch(const T* x, const float* dz, float* dw, void* ws, size_t ws_bytes, int N, int D, int H, int W,
                                                 int lddz, int dz_coff, hipStream_t s);
template <typename T> int fdn_conv_cout1_dgrad_folded_launch(const char* who, const float* dz, const float* w, const T* y_prev, int act, float alpha,
                                                             T* dz_prev, float* dbias_prev, void* workspace, size_t workspace_bytes, int N, int D,
                                                             int H, int W, int lddz, int dz_coff, hipStream_t s, const uint16_t* ymask);
template <typename T> int fdn_wgrad_1x1_launch(const T* xa, const T* xb, const T* dz, float* dw, void* ws, size_t ws_bytes, int N, int D, int H,
                                               int W, hipStream_t s);
template <typename T> int fdn_bias_grad_launch(const T* dz, float* db, void* ws, size_t ws_bytes, int N, int D, int H, int W, int C, int lddz,
                                               int dz_coff, hipStream_t s);

// ---- the MFMA formulations (default; small_convs.hip forwards to them and keeps its VALU kernels selectable in the test build).  The
// weight gradients write `nblocks` (cin3, 1x1) resp. fdn_thin_partials (heads) partial rows, which the caller reduces ----
// cin3_mfma.hip: the two 3->64 kernels as im2col GEMMs (the weight gradient: even W)
template <typename T> int fdn_conv_cin3_fwd_mfma_launch(const T* x, const float* w, const float* bias, T* y, int N, int D, int H, int W, int act,
                                                        float alpha, hipStream_t s);
template <typename T> int fdn_wgrad_cin3_mfma_launch(const T* x, const T* dz, float* partial, int nblocks, int N, int D, int H, int W, hipStream_t s);
// conv1x1_mfma.hip
template <typename T> int fdn_conv1x1_fwd_mfma_launch(const T* xa, const T* xb, const float* w, const float* bias, T* y, int64_t nvox, int act,
                                                      float alpha, hipStream_t s);
template <typename T> int fdn_conv1x1_dgrad_mfma_launch(const T* dz, const float* w, const T* ya, const T* yb, T* dxa, T* dxb, int64_t nvox,
                                                        hipStream_t s);
template <typename T> int fdn_wgrad_1x1_mfma_launch(const T* xa, const T* xb, const T* dz, float* partial, int nblocks, int64_t nvox, hipStream_t s);
// heads_mfma.hip; bpart: the FDN_THIN_HEAD_DBIAS rows, or NULL
template <typename T> int fdn_head_fwd_launch(const T* x, const float* w, const float* bias, float* y, int N, int D, int H, int W, int ldy,
                                              int y_coff, int act, float alpha, hipStream_t s, int xcd_walk);
template <typename T> int fdn_head_dgrad_launch(const float* dz, const float* w, const T* y_prev, int act, float alpha, T* dz_prev, float* bpart,
                                                int N, int D, int H, int W, int lddz, int dz_coff, hipStream_t s, const uint16_t* ymask);
template <typename T> int fdn_head_wgrad_launch(const T* x, const float* dz, float* partial, int N, int D, int H, int W, int lddz, int dz_coff,
                                                hipStream_t s);

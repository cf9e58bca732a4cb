// The host plan of the 64->64 3x3x3 weight gradient: which kernel runs (route), how a batch of layers goes out (chunks), how many
// splits of the voxel sum each launch gets, and the workspace bytes its partial sums take.  fdn_wgrad64_plan is the one place that
// decides these; api.hip walks its steps, the launchers (wgrad64_mfma.hip, wgrad64_wino.hip, wgrad64_bf16.hip) fill their kernel
// arguments from a step and check the workspace against the step's partial_bytes, and the public size queries are maxima over the
// same steps -- so every launch of a call fits the bytes the size query promised.  Host only: no HIP calls, no globals.
#pragma once
#include <stddef.h>
#include <vector>
#include "fdn.h"

// tile extents the split counts depend on (the kernels' own constants)
namespace fdn_wg {
constexpr int kTH = 4, kTW = 8;                         // direct kernel (wgrad64_mfma.hip): tiles of 1 x 4 x 8 voxels
constexpr int WTH = 6, WTG = 2, WTW = 4 * WTG;          // Winograd kernels (wgrad64_wino.hip): 1 x 6 x 8 voxels (plane pairs with the depth transform)
constexpr int TD = 2, TH = 8, TW = 8;                   // bf16 kernels (wgrad64_bf16.hip): 2 x 8 x 8 (register-staged) / 1 x 8 x 8 (LDS-DMA)
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
}  // namespace fdn_wg

constexpr int kWgBatchMax = 32;          // layers of one fp32 batched launch (the pointer tables of WgWinoBatch)
constexpr int kWgBfBatchMax = 8;         // pointer-table size of Wgrad64BfBatch ...
constexpr int kWgBfChunkMax = 7;         // ... of which a chunk fills at most 7 (3 S layers ~ 504 workgroups)

enum FdnWgrad64Route {
    FDN_WG_DIRECT,          // fp32 direct kernel, 3 depth taps x S
    FDN_WG_WINO_W,          // fp32 F(3,4) along W, 3 depth taps x S
    FDN_WG_WINO_DEP,        // ... with F(3,2) along D on top (even D), 4 depth coordinates x S
    FDN_WG_WINO_BATCH,      // the same kernel over `count` layers of one grid in one launch
    FDN_WG_BF16_DMA,        // bf16 LDS-DMA kernel (one-plane tiles, depth segments)
    FDN_WG_BF16_REG,        // bf16 register-staged kernel (two-plane tiles): tensors of 4 GB and more
    FDN_WG_BF16_BATCH       // the LDS-DMA kernel over `count` layers in one launch
};
inline const char* fdn_wgrad64_route_name(FdnWgrad64Route r) {
    static const char* const names[] = {"direct", "wino_w", "wino_dep", "wino_batch", "bf16_dma", "bf16_reg", "bf16_batch"};
    return names[r];
}

// the test build's route-forcing switches (each lives in its translation unit; all zero in the product library)
struct FdnWgrad64Hooks { int force_direct = 0, wino_nodep = 0, bf16_variant = 0; };

// one launch (+ its reduction) over the layers [first, first + count)
struct FdnWgrad64Step {
    FdnWgrad64Route route;
    int first, count;
    int splits;              // S: walks of the tile list per layer
    int planes;              // 64 x 64 partial planes per split: 27 taps, or 36 = 4 depth coordinates x 9
    int grid, tiles;         // workgroups of the launch; tiles of one layer
    int nseg, seg_len;       // LDS-DMA kernels: depth segments of the (n, th, tw) columns
    size_t partial_bytes;    // count x splits x planes x 4096 floats at the start of the workspace
};

struct FdnWgrad64Plan {
    std::vector<FdnWgrad64Step> steps;       // in launch order; they cover the layers 0 .. n_layers - 1 once each
    size_t workspace_bytes = 0;              // the largest partial_bytes (the steps reuse the workspace one after the other)
    bool addr32_ok = true;                   // false: the fp32 kernels' 32-bit buffer offsets do not reach the end of x
};

// the kernel of a single layer
inline FdnWgrad64Route fdn_wgrad64_single_route(bool bf16, int N, int D, int H, int W, int algo, FdnWgrad64Hooks hk) {
    // bf16: the LDS-DMA kernel addresses x / dz through 32-bit buffer offsets; tensors of 4 GB and more keep the register-staged kernel
    if (bf16) return ((long long)N * D * H * W * 128 < (1ll << 32) - 4096 && !hk.bf16_variant) ? FDN_WG_BF16_DMA : FDN_WG_BF16_REG;
    if (hk.force_direct || algo == FDN_ALGO_DIRECT) return FDN_WG_DIRECT;
    // F(3,2) along D on top of F(3,4) along W whenever D is even (FDN_ALGO_WINO_W keeps the W-only kernel selectable)
    return (D >= 2 && (D & 1) == 0 && algo != FDN_ALGO_WINO_W && !hk.wino_nodep) ? FDN_WG_WINO_DEP : FDN_WG_WINO_W;
}

// whether n_layers layers of one grid go out in batched launches (else layer by layer).  fp32: the depth-transformed kernel applies,
// W % 4 == 0 and the layers fit the pointer tables; bf16: the LDS-DMA kernel applies and a layer has >= 4 * 80 one-plane tiles (every
// walk of every chunk size gets >= 4)
inline bool fdn_wgrad64_batchable(bool bf16, int n_layers, int N, int D, int H, int W, int algo, FdnWgrad64Hooks hk) {
    if (n_layers < 2) return false;
    if (bf16) {
        const long long tiles1 = (long long)N * D * fdn_wg::cdiv(H, fdn_wg::TH) * fdn_wg::cdiv(W, fdn_wg::TW);
        return fdn_wgrad64_single_route(true, N, D, H, W, algo, hk) == FDN_WG_BF16_DMA && tiles1 >= 4 * 80;
    }
    return n_layers <= kWgBatchMax && (W & 3) == 0 && fdn_wgrad64_single_route(false, N, D, H, W, algo, hk) == FDN_WG_WINO_DEP;
}

// layers of the next batched launch when `rem` are left (1: a lone layer, which takes the single-layer kernel)
inline int fdn_wgrad64_chunk(bool bf16, int rem) {
    if (bf16) return rem > kWgBfChunkMax ? (rem == 8 ? 4 : kWgBfChunkMax) : rem;           // (8 = 4 + 4 rather than 7 + 1)
    // fp32: the batched kernel gives every layer 64 / c splits x 4 coordinates: c = 11 fills 220 of the 256 CUs.  Such a batch goes out
    // in chunks that fill the chip (>= 63 of 64 split slots: 1, 2, 3, 4, 7, 8, 9, 16 layers), a batch at >= 15/16 as it is.
    auto fill64 = [](int c) { return (64 / c) * c; };
    int c = rem;
    if (fill64(rem) < 60) { c = rem - 1; while (c > 1 && fill64(c) < 63) --c; }
    return c;
}

// the geometry of one launch of `route` over `count` layers
inline FdnWgrad64Step fdn_wgrad64_step(FdnWgrad64Route route, int first, int count, int N, int D, int H, int W) {
    using namespace fdn_wg;
    FdnWgrad64Step st = {route, first, count, 0, 27, 0, 0, 0, 0, 0};
    long long tiles = 0, S = 0;
    int per = 3;                           // workgroups per split: the depth taps, or the 4 depth coordinates
    switch (route) {
    case FDN_WG_DIRECT:
        tiles = (long long)N * D * cdiv(H, kTH) * cdiv(W, kTW);
        // 3 tap groups x S workgroups; two workgroups fit a CU -> aim for ~512 resident, at least 8 tiles each
        S = 170;                           // 3*170 = 510 workgroups ~ 2 per CU
        if (tiles / 8 < S) S = tiles / 8 > 0 ? tiles / 8 : 1;
        break;
    case FDN_WG_WINO_W:
        tiles = (long long)N * D * cdiv(H, WTH) * cdiv(W, WTW);
        S = 85;                            // 3 * 85 = 255 workgroups: one (8 waves, 126 KB of LDS) per CU
        if (tiles < S) S = tiles > 0 ? tiles : 1;
        break;
    case FDN_WG_WINO_DEP:
    case FDN_WG_WINO_BATCH:
        tiles = (long long)N * (D / 2) * cdiv(H, WTH) * cdiv(W, WTW);       // of plane pairs
        S = 64 / count;                    // 4 S count <= 256 workgroups: one per CU, the chip filled once
        if (S < 1) S = 1;
        if (tiles < S) S = tiles > 0 ? tiles : 1;
        st.planes = 36; per = 4;
        break;
    case FDN_WG_BF16_DMA:
    case FDN_WG_BF16_REG:
    case FDN_WG_BF16_BATCH: {
        const long long tiles2 = (long long)N * cdiv(D, TD) * cdiv(H, TH) * cdiv(W, TW);
        tiles = route == FDN_WG_BF16_REG ? tiles2 : (long long)N * D * cdiv(H, TH) * cdiv(W, TW);
        if (route == FDN_WG_BF16_BATCH) {
            S = (168 / count) & ~7;        // 3 S count ~ 504 workgroups, a multiple of 8 per layer
            if (S < 8) S = 8;
        } else {
            // (counted in two-plane tiles for both kernels: the one-plane kernel then has >= 4 tiles per walk)
            S = 168;                       // 3*168 = 504 workgroups ~ 2 per CU; a multiple of 8 (one walk set per XCD)
            while (S > 8 && tiles2 / 2 < S) S -= 8;
        }
        if (route != FDN_WG_BF16_REG && D > 0) {
            // depth segments: long enough for the plane reuse between the taps (<= 32 planes), short enough that every walk of
            // every XCD gets >= ~4 units
            int want = (int)(tiles / (S * 4));
            want = want < 1 ? 1 : (want > 32 ? 32 : want);
            st.nseg = cdiv(D, want);
            st.seg_len = cdiv(D, st.nseg);
            st.nseg = cdiv(D, st.seg_len);
        }
        break;
    }
    }
    st.splits = (int)S;
    st.tiles = (int)tiles;
    st.grid = per * st.splits * count;
    st.partial_bytes = (size_t)count * st.splits * st.planes * 4096 * sizeof(float);
    return st;
}

// The plan of a call: n_layers = 1 for fdn_conv3d_wgrad[_bf16], the layers of fdn_conv3d_wgrad[_bf16]_batch.  Pure.
inline FdnWgrad64Plan fdn_wgrad64_plan(bool bf16, int n_layers, int N, int D, int H, int W, int algo, FdnWgrad64Hooks hk) {
    FdnWgrad64Plan p;
    p.addr32_ok = bf16 || (long long)N * D * H * W * 256 < (1ll << 32);
    const FdnWgrad64Route single = fdn_wgrad64_single_route(bf16, N, D, H, W, algo, hk);
    const bool batch = fdn_wgrad64_batchable(bf16, n_layers, N, D, H, W, algo, hk);
    for (int first = 0; first < n_layers;) {
        const int c = batch ? fdn_wgrad64_chunk(bf16, n_layers - first) : 1;
        p.steps.push_back(fdn_wgrad64_step(c == 1 ? single : (bf16 ? FDN_WG_BF16_BATCH : FDN_WG_WINO_BATCH), first, c, N, D, H, W));
        if (p.steps.back().partial_bytes > p.workspace_bytes) p.workspace_bytes = p.steps.back().partial_bytes;
        first += c;
    }
    return p;
}

// What the public size queries answer.  Python asks for bytes without an algo (and before a test sets a hook), so these are upper
// bounds: over the single-layer plans of every algo -- the hooks force no route an algo does not also select -- and, where the layers
// can be batched, over every chunk size a plan of <= n_layers layers can hold, built by the same fdn_wgrad64_step the plan launches from.
inline size_t fdn_wgrad64_bound(bool bf16, int N, int D, int H, int W) {
    size_t b = 0;
    for (int algo : {FDN_ALGO_AUTO, FDN_ALGO_DIRECT, FDN_ALGO_WINO_W}) {
        const size_t a = fdn_wgrad64_step(fdn_wgrad64_single_route(bf16, N, D, H, W, algo, FdnWgrad64Hooks()), 0, 1, N, D, H, W).partial_bytes;
        if (a > b) b = a;
    }
    return b;
}
inline size_t fdn_wgrad64_batch_bound(bool bf16, int n_layers, int N, int D, int H, int W, FdnWgrad64Hooks hk) {
    if (n_layers <= 0 || N <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    size_t b = fdn_wgrad64_bound(bf16, N, D, H, W);
    if (fdn_wgrad64_batchable(bf16, n_layers, N, D, H, W, FDN_ALGO_AUTO, hk))
        for (int c = 2; c <= n_layers && c <= (bf16 ? kWgBfChunkMax : kWgBatchMax); ++c) {
            const size_t a = fdn_wgrad64_step(bf16 ? FDN_WG_BF16_BATCH : FDN_WG_WINO_BATCH, 0, c, N, D, H, W).partial_bytes;
            if (a > b) b = a;
        }
    return b;
}

/* lib4dflow_hip.so -- C-ABI of the MI355X-native 4DFlowNet hot path.
 *
 * The reference (EdwardFerdian/4DFlowNet) has no FFI: it calls TensorFlow/Keras ops from Python.
 * Each entry point below replaces the TF op(s) the reference invokes implicitly at the cited
 * file:line (paths relative to the reference root).  Conventions:
 *   - every pointer is a DEVICE pointer to fp32 data owned by the caller (torch tensors);
 *     the library allocates nothing and keeps no global mutable state (the only process-wide
 *     data is a lock-protected record of which kernels already had their LDS attribute set,
 *     per device).  Entry points are re-entrant per (device, stream) from any host thread;
 *   - scratch memory is caller-owned too: SURVEY.md 8(b) sketched fdn_workspace_create/destroy,
 *     which this ABI deliberately replaces by explicit `workspace` arguments sized by
 *     fdn_*_workspace_bytes() -- the caller's allocator (torch's caching allocator) already
 *     recycles such buffers stream-safely, and a library-held handle would be global state;
 *   - there is NO CPU build of these symbols (SURVEY.md 8(b) asked for a g++/OpenMP one so tests
 *     could run without a GPU): a second implementation behind the same names is exactly the
 *     silent-fallback hazard the parity claims must exclude.  Without a GPU the tests check that
 *     the library builds, loads and exports every symbol declared here (tests/test_abi.py); the
 *     arithmetic is checked on the GPU against oracle/ (a separate, test-only restatement);
 *   - the variant-forcing / ablation switches used by tests and tools (fdn_debug_*) are NOT
 *     part of this ABI and are not exported by lib4dflow_hip.so; they exist only in
 *     lib4dflow_hip_test.so (same sources, -DFDN_TEST_HOOKS);
 *   - tensors are NDHWC, channel innermost; conv kernels are Keras layout (kd,kh,kw,Cin,Cout);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: FDN_OK or a negative error code; fdn_last_error() gives a message
 *     (thread-local).  No exceptions cross the boundary;
 *   - memory contract: an entry point reads no byte outside the extents its arguments describe (N, D, H, W, channel counts,
 *     ld* / *_coff, element counts, descriptor tables) and writes no byte outside its outputs and the first
 *     fdn_*_workspace_bytes() bytes of its workspace (a fixed size where this header states one, e.g. 2048 * 64 floats);
 *     it never reads workspace or output memory before writing it, so neither needs initialising and whatever lies beside
 *     an operand -- NaN, Inf, another tensor -- cannot reach a result.  Tile overhangs are served by offsets that fall
 *     outside the buffer range ("reads zero") or by clamped indices with predicated stores, never by a load of a
 *     neighbour times zero (tests/test_gpu_guard_bands.py, DESIGN.md "Memory contract").
 */
#ifndef FDN_H
#define FDN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FDN_OK 0
#define FDN_ERR_BAD_ARG (-1)
#define FDN_ERR_UNSUPPORTED (-2)
#define FDN_ERR_HIP (-3)
#define FDN_ERR_WORKSPACE (-4)

#define FDN_ACT_NONE 0
#define FDN_ACT_RELU 1  /* Conv3D(activation='relu')            src/Network/SR4DFlowNet.py:17-25,39,42,45 */
#define FDN_ACT_LEAKY 2 /* tf.keras.layers.LeakyReLU(alpha=0.2) src/Network/SR4DFlowNet.py:113,118 */
/* Conv3D(activation='tanh'): the bounded output of the three 64->1 heads (the first set of published weights was trained with it;
 * README.md:11,23 of the reference).  Accepted by fdn_conv3d_fwd / fdn_conv3d_fwd_bf16 on the (64,1,3) route and, as out_act, by
 * fdn_loss_metrics_act.  Everywhere else it is refused before the device is touched, under the entry point's name: FDN_ERR_BAD_ARG
 * where an act outside NONE..LEAKY always was (the other routes of the two forwards, the 64->64 entry points, fdn_conv_cout1_dgrad_folded_mask),
 * FDN_ERR_UNSUPPORTED where an unknown act used to mean "none" (fdn_fold_halo[_border][_bf16], fdn_upsample_trilinear_bwd[_bf16],
 * fdn_conv_cout1_dgrad_folded[_bf16][_mask]).  y = tanh(z) of the value FDN_ACT_NONE stores: odd bit for bit, |y| <= 1, exactly +-1 for |z| >= 9.02 (+-inf included), NaN
 * only from NaN, within 3 ulp of tanh. */
#define FDN_ACT_TANH 3

/* Algorithm selector of the 64->64 3x3x3 entry points (fdn_conv3d_fwd / _dgrad / _dgrad_fused[_part] / _wgrad; ignored by
 * every other (Cin,Cout,K)).  Per call, no global state.
 *   FDN_ALGO_AUTO   : the planner's choice.  Forward / dgrad: 2-D Winograd, F(4,3) along H x F(4,3) along W (a quarter of the
 *                     direct multiplies) when H and W are multiples of 4, F(2,3) along H x F(4,3) along W (a third) when H is
 *                     only even, else 1-D Winograd along W (F(4,3): half the multiplies) when W is a multiple of 4, else
 *                     direct.  wgrad: F(3,4) along W when W is a multiple of 4 (+ F(3,2) along D when D is even).
 *                     fp32 error up to ~1e-6 of sum|x||w| (F(4,3) x F(4,3)) instead of ~1e-7;
 *   FDN_ALGO_DIRECT : always the direct convolution (plain fp32 FMA chains over the 27 taps, no transform) -- for
 *                     parity-critical runs and for layers whose operands are too ill-conditioned for the transform;
 *   FDN_ALGO_WINO_W : Winograd along W only (the 1-D kernels), never the H transform;
 *   FDN_ALGO_WINO_H2: like AUTO, but never more than F(2,3) along H (round 4's kernels; a third of the error of F(4,3) x F(4,3));
 *   FDN_ALGO_WINO_BF16X3: like AUTO, but where AUTO takes F(4,3) x F(4,3) (forward, dgrad inner box) the Winograd-domain products run
 *                     on the bf16 matrix pipe: both operands (fp32, transformed exactly as under AUTO) are split EXACTLY into three
 *                     bf16 pieces v = hi + mid + lo, and the six cross terms hi.hi, mid.hi, lo.hi, hi.mid, mid.mid, hi.lo are
 *                     accumulated in fp32 (a bf16 x bf16 product is exact in fp32; the three dropped terms are <= 2^-25 |u||v|, below
 *                     the half ulp an fp32 multiply rounds away).  Inputs, outputs, transforms and accumulation stay fp32.  Every
 *                     other grid and the weight gradient behave as under AUTO. */
#define FDN_ALGO_AUTO 0
#define FDN_ALGO_DIRECT 1
#define FDN_ALGO_WINO_W 2
#define FDN_ALGO_WINO_H2 3
#define FDN_ALGO_WINO_BF16X3 4
#define FDN_ALGO_LAST FDN_ALGO_WINO_BF16X3

/* Version of this header; fdn_version() returns the version the library was built from.  A caller must see the two equal:
 * 140 -> 150 and 150 -> 160 grew FDN_CONV64_PACK_FLOATS (a pack buffer sized by an older header is too small for this library). */
#define FDN_VERSION 161
int fdn_version(void);
const char* fdn_last_error(void);

/* speed/mag/pcmr + the two channel concats.  src/Network/SR4DFlowNet.py:10-15.
 * u..mw: (nvox) each; phase, pc: (nvox,3). */
int fdn_input_features(const float* u, const float* v, const float* w, const float* mu, const float* mv,
                       const float* mw, float* phase, float* pc, int64_t nvox, void* stream);

/* Re-layout one 3x3x3 64->64 Keras kernel (27,64,64) into the MFMA operand streams used by
 * fdn_conv3d_fwd (wp_fwd) and fdn_conv3d_dgrad / fdn_conv3d_dgrad_fused (wp_dgrad: taps flipped,
 * Cin/Cout swapped).  Each output is FDN_CONV64_PACK_FLOATS floats: the direct-convolution stream
 * (27 taps), the Winograd F(4,3)-along-W stream U = G g (9 (kd,kh) taps x 6 transform coordinates)
 * and the two 2-D streams U = Gh g Gw^T (3 kd taps x 4 x 6 coordinates for F(2,3) along H, 3 x 6 x 6
 * for F(4,3) along H), and the F(4,3) x F(4,3) stream once more as three bf16 pieces per value (FDN_ALGO_WINO_BF16X3:
 * 162 * 4096 float-sized slots); the conv entry points select among them by the extents (see FDN_ALGO_*).
 * Either output may be NULL. */
#define FDN_CONV64_PACK_FLOATS (423 * 64 * 64)
int fdn_pack_conv64_weights(const float* w, float* wp_fwd, float* wp_dgrad, void* stream);
/* The same for n_layers kernels in ONE launch (after every optimizer step): layer i lives at
 * w_base + w_offsets[i] (w_offsets: DEVICE array of n_layers float offsets), its two streams at
 * packs + i * 2 * FDN_CONV64_PACK_FLOATS (forward stream first, dgrad stream second). */
int fdn_pack_conv64_weights_batch(const float* w_base, const int64_t* w_offsets, int n_layers, float* packs,
                                  void* stream);
/* A pack holds five streams and a given grid reads one or two of them.  fdn_conv64_pack_streams says which: the streams
 * (FDN_PACK_STREAM_* bits) that fdn_conv3d_fwd (role FDN_ROLE_FWD, reads wp_fwd), fdn_conv3d_dgrad (FDN_ROLE_DGRAD) or
 * fdn_conv3d_dgrad_fused[_part] (FDN_ROLE_DGRAD_FUSED; both read wp_dgrad) read for a 64->64 layer on an (N,D,H,W) grid
 * under `algo` -- answered by the launcher's own selection code, so it cannot drift from it; negative = error code.
 * fdn_pack_conv64_weights_batch_streams is fdn_pack_conv64_weights_batch restricted to the named streams of the forward
 * and of the dgrad packs (the others keep whatever they held: a caller that narrows the set must re-pack before a
 * grid that needs more).  cfg2 reads F(4,3)xF(4,3) forward and F(4,3)xF(4,3) + 1-D Winograd (shell faces) in dgrad: 270 of
 * the 846 x 4096 floats per layer.  The per-step re-pack after the optimizer, TrainerController.py:225. */
#define FDN_PACK_STREAM_DIRECT 1
#define FDN_PACK_STREAM_WINO_W 2
#define FDN_PACK_STREAM_WINO_H2 4
#define FDN_PACK_STREAM_WINO_H4 8
#define FDN_PACK_STREAM_WINO_H4S 16 /* F(4,3) x F(4,3), three bf16 pieces per value (FDN_ALGO_WINO_BF16X3) */
#define FDN_PACK_STREAM_ALL 31
#define FDN_ROLE_FWD 0
#define FDN_ROLE_DGRAD 1
#define FDN_ROLE_DGRAD_FUSED 2
int fdn_conv64_pack_streams(int N, int D, int H, int W, int algo, int role);
int fdn_pack_conv64_weights_batch_streams(const float* w_base, const int64_t* w_offsets, int n_layers, float* packs,
                                          int streams_fwd, int streams_dgrad, void* stream);

/* y = act(conv3d(sym_pad(x), w) + bias + residual).
 * Replaces tf.pad(SYMMETRIC,p=(K-1)/2) + Conv3D(valid) + BiasAdd + activation, and the
 * resnet_block add + LeakyReLU when `residual` is given.  src/Network/SR4DFlowNet.py:93-120.
 * Supported (Cin,Cout,K): (64,64,3) [MFMA path; needs wpack from fdn_pack_conv64_weights],
 * (3,64,3), (64,1,3), (128,64,1) [x = first 64 input channels, x2 = last 64: the concat at
 * SR4DFlowNet.py:23 is never materialised].  x2, wpack, bias, residual may be NULL where unused.
 * Output rows are written at y[voxel*ldy + y_coff + c] (ldy=Cout,y_coff=0 for a dense tensor;
 * the three 64->1 heads write straight into the (N,V,3) prediction: SR4DFlowNet.py:49).
 * algo: FDN_ALGO_AUTO | FDN_ALGO_DIRECT | FDN_ALGO_WINO_W, consulted by the (64,64,3) path only (see above); here and in the entry points below.
 * Arithmetic of the (64,1,3) head, whatever `algo`: x . w is formed on the bf16 matrix pipe with fp32 accumulation -- fp32 storage: x and w
 * each split exactly into three bf16 pieces, six of the nine cross terms, every product within 2^-22 of the fp32 operands' exact product;
 * bf16 storage (fdn_conv3d_fwd_bf16): w as two pieces, within 2^-16 -- and, like every conv, fold and upsample entry point of this header,
 * the result commutes bit for bit with power-of-two scalings of its operands; both hold, and are tested, for non-zero operands with
 * 2^-46 <= |v| < 2^47 (values of 2^-6 <= |v| < 2^7 scaled by up to 2^+-40) whose two scales multiply to within 2^+-60. */
int fdn_conv3d_fwd(const float* x, const float* x2, const float* w, const float* wpack, const float* bias,
                   const float* residual, float* y, int N, int D, int H, int W, int Cin, int Cout, int K,
                   int ldy, int y_coff, int act, float alpha, int algo, void* stream);

/* Gradient w.r.t. the PADDED conv input (Conv3DBackpropInputV2): dxpad (N,D+2,H+2,W+2,Cin) for K=3.
 * dz rows are read at dz[voxel*lddz + dz_coff + c].  Fold the halo with fdn_fold_halo.
 * Supported (Cin,Cout,K): (64,64,3) [needs wpack = wp_dgrad], (64,1,3). */
int fdn_conv3d_dgrad(const float* dz, const float* w, const float* wpack, float* dxpad, int N, int D, int H,
                     int W, int Cin, int Cout, int K, int lddz, int dz_coff, int algo, void* stream);

/* The 64->1 head conv's input gradient with the halo fold and the producer's activation gradient fused
 * (no padded intermediate): dz_prev[i] = act'(y_prev[i]) * sum_{(o,t): clamp(o+t-1)=i} w[t] * dz[o].
 * dz rows at dz[voxel*lddz + dz_coff]; y_prev may be NULL.  If dbias_prev != NULL it also receives
 * BiasAddGrad of the producing layer (per-channel sum of dz_prev, 64 floats), using `workspace`
 * (>= 2048*64*4 bytes).  SR4DFlowNet.py:39-46 under tape.gradient. */
int fdn_conv_cout1_dgrad_folded(const float* dz, const float* w, const float* y_prev, int act, float alpha,
                                float* dz_prev, float* dbias_prev, void* workspace, size_t workspace_bytes, int N,
                                int D, int H, int W, int lddz, int dz_coff, void* stream);
/* ... reading the producer's sign mask (fdn_conv64_fwd_mask: planar [cout / 16][voxel] words; W % 4 == 0) instead of y_prev: eight 8-B loads
 * per 16 voxels and lane instead of 32 rows, 7 MB instead of 226 MB per (8,48^3) launch.  Bit-identical to the y_prev form. */
int fdn_conv_cout1_dgrad_folded_mask(const float* dz, const float* w, const uint16_t* y_mask, int act, float alpha,
                                     float* dz_prev, float* dbias_prev, void* workspace, size_t workspace_bytes, int N,
                                     int D, int H, int W, int lddz, int dz_coff, void* stream);

/* MirrorPadGrad + gradient fan-in + activation gradient in one pass:
 * dz_prev[i] = (sum_s sum_{P: clamp(P)=i} dxpad_s[P] + skip[i]) * act'(y_prev[i]).
 * nsrc in 1..3; skip, y_prev may be NULL (act' = 1). */
int fdn_fold_halo(const float* dxpad0, const float* dxpad1, const float* dxpad2, int nsrc, const float* skip,
                  const float* y_prev, int act, float alpha, float* dz_prev, int N, int D, int H, int W,
                  int C, void* stream);

/* 64->64 dgrad with MirrorPadGrad fused for the voxels strictly inside the volume (each receives exactly one
 * contribution): there  dz_prev[i] = (dgrad[i] + skip[i]) * act'(y_prev[i])  is written by the conv epilogue;
 * every other padded position is written to dxpad (N,D+2,H+2,W+2,64) and finished by fdn_fold_halo_border,
 * which applies the same formula on the surface voxels with up to 3 padded sources.  skip may alias dz_prev
 * (gradient fan-in over several consumers: call with y_prev=NULL for all but the last).  wpack = wp_dgrad. */
int fdn_conv3d_dgrad_fused(const float* dz, const float* wpack, float* dxpad, const float* skip, const float* y_prev,
                           int act, float alpha, float* dz_prev, int N, int D, int H, int W, int algo, void* stream);
/* The same in two independent pieces, for callers that overlap them on two streams (they write disjoint positions; both must
 * have completed before fdn_fold_halo_border): FDN_DGRAD_INNER = the D x H x W box (finishes the interior of dz_prev, writes its
 * surface voxels to dxpad), FDN_DGRAD_SHELL = the one-voxel shell of the padded grid (dxpad only; ignores skip / y_prev). */
#define FDN_DGRAD_INNER 1
#define FDN_DGRAD_SHELL 2
int fdn_conv3d_dgrad_fused_part(const float* dz, const float* wpack, float* dxpad, const float* skip, const float* y_prev,
                                int act, float alpha, float* dz_prev, int N, int D, int H, int W, int parts, int algo,
                                void* stream);
int fdn_fold_halo_border(const float* dxpad0, const float* dxpad1, const float* dxpad2, int nsrc, const float* skip,
                         const float* y_prev, int act, float alpha, float* dz_prev, int N, int D, int H, int W,
                         void* stream);
/* Sign masks for the activation gradient (training; the fp32 twin of the bf16 mode's).  act'(y) needs one bit of y, and at the large
 * grids an epilogue operand costs the fused dgrad what streaming it from HBM costs: the forward of a 64->64 layer can write, beside y,
 * the mask y_mask[c / 16][voxel] (uint16_t words, N*D*H*W per plane, 4 planes: bit b of word (p, v) = (y[v][16 p + b] > 0); 8 B per voxel)
 * and the fused dgrad of its consumer read that instead of y_prev.  Only the plain F(4,3) x F(4,3) kernels do (H and W multiples of 4,
 * FDN_ALGO_AUTO): fdn_conv64_mask_ok says 1 when BOTH entry points below are available for the grid, 0 when the caller must keep to
 * fdn_conv3d_fwd / fdn_conv3d_dgrad_fused (they return FDN_ERR_UNSUPPORTED otherwise).  fdn_fold_halo_border still reads y_prev (surface
 * voxels only).  Results are bit-identical to the y_prev forms.  src/Network/SR4DFlowNet.py:93-120 and their gradients. */
int fdn_conv64_mask_ok(int N, int D, int H, int W, int algo);
int fdn_conv64_fwd_mask(const float* x, const float* wpack, const float* bias, const float* residual, float* y, uint16_t* y_mask,
                        int N, int D, int H, int W, int act, float alpha, int algo, void* stream);
int fdn_conv64_dgrad_fused_mask(const float* dz, const float* wpack, float* dxpad, const float* skip, const uint16_t* y_mask,
                                int act, float alpha, float* dz_prev, int N, int D, int H, int W, int algo, void* stream);
/* Fused dgrad of up to three 64->64 layers that share their INPUT (the u, v, w heads' first convs all read the last ResBlock's output,
 * src/Network/SR4DFlowNet.py:39-46; under tape.gradient their input gradients add up, TrainerController.py:223):
 *   dz_prev = (MirrorPadGrad(sum_s Conv3DBackpropInput(dz[s], W_s)) + skip) * act'(y_prev)
 * as ONE launch + one fdn_fold_halo_border instead of nsrc chained fdn_conv3d_dgrad_fused calls (each re-reading the running sum as
 * `skip` and writing it back): the kernel walks the sources inside its tile and keeps the sum in its output registers.  dz / wpack:
 * host arrays of nsrc (1..3) device pointers, wpack[s] = the dgrad pack of layer s; the packs must come from one
 * fdn_pack_conv64_weights_batch buffer (within 1 GiB of each other).  y_prev or y_mask (fdn_conv64_fwd_mask's) or neither (act =
 * FDN_ACT_NONE).  Available where fdn_conv64_mask_ok(N, D, H, W, algo) says 1 (FDN_ERR_UNSUPPORTED elsewhere: chain the single-source
 * entry point).  Equal to the chained launches to fp32 rounding (the sum is formed in the Winograd domain, in pack-address order). */
int fdn_conv64_dgrad_fused_multi(const float* const* dz, const float* const* wpack, int nsrc, float* dxpad, const float* skip,
                                 const float* y_prev, const uint16_t* y_mask, int act, float alpha, float* dz_prev, int N, int D,
                                 int H, int W, int algo, void* stream);

/* 1x1x1 128->64 conv backward w.r.t. its two 64-channel inputs, fused with their ReLU masks:
 * dxa = (dz . W[0:64,:]^T) * (ya>0), dxb = (dz . W[64:128,:]^T) * (yb>0).  SR4DFlowNet.py:23-24. */
int fdn_conv1x1_dgrad(const float* dz, const float* w, const float* ya, const float* yb, float* dxa,
                      float* dxb, int64_t nvox, void* stream);

/* dW (K,K,K,Cin,Cout) = Conv3DBackpropFilterV2(sym_pad(x), dz); dbias (Cout) = BiasAddGrad(dz) if
 * dbias != NULL.  Same (Cin,Cout,K) support and x/x2 convention as fdn_conv3d_fwd.
 * workspace: caller-owned scratch of at least fdn_conv3d_wgrad_workspace_bytes(...). */
size_t fdn_conv3d_wgrad_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int K);

/* The weight gradients of n_layers 64->64 3x3x3 layers that share one (N, D, H, W) grid, as ONE launch + one reduction where the
 * Winograd kernel applies (W % 4 == 0, D even, algo AUTO / WINO_H2 / WINO_BF16X3), else layer by layer.  Results equal n_layers calls
 * of fdn_conv3d_wgrad to fp32 rounding, not bit for bit, where the batched kernel runs: it gives every layer 64 / n_layers splits of the
 * voxel sum, the single-layer launch 63 (the layer-by-layer fall-back IS those calls).  x, dz, dw (and dbias, which may be NULL or hold NULL entries): HOST arrays of n_layers device pointers
 * (dz rows dense, 64 channels).  Why: at the low-res grid of cfg2 (8 x 24^3) a layer that has the chip to itself gives a workgroup
 * 4.6 tiles between its prologue and its output transform; batched, the ResBlock layers of one gradient bucket share the chip and
 * each workgroup walks n_layers times more tiles of its layer.  src/Network/TrainerController.py:223 (tape.gradient). */
size_t fdn_conv3d_wgrad_batch_workspace_bytes(int n_layers, int N, int D, int H, int W);
int fdn_conv3d_wgrad_batch(const float* const* x, const float* const* dz, float* const* dw, float* const* dbias, int n_layers,
                           void* workspace, size_t workspace_bytes, int N, int D, int H, int W, int algo, void* stream);
int fdn_conv3d_wgrad(const float* x, const float* x2, const float* dz, float* dw, float* dbias,
                     void* workspace, size_t workspace_bytes, int N, int D, int H, int W, int Cin, int Cout,
                     int K, int lddz, int dz_coff, int algo, void* stream);

/* upsample3d: trilinear, align_corners=True, integer factor R.  src/Network/SR4DFlowNet.py:53-90.
 * fwd: x (N,D,H,W,C) -> y (N,DR,HR,WR,C).
 * bwd: dx = U^T dy, optionally * act'(y_prev) with y_prev (N,D,H,W,C). */
int fdn_upsample_trilinear_fwd(const float* x, float* y, int N, int D, int H, int W, int C, int R, void* stream);
int fdn_upsample_trilinear_bwd(const float* dy, const float* y_prev, int act, float alpha, float* dx, int N,
                               int D, int H, int W, int C, int R, void* stream);

/* Loss + metric + dPred in one call.  src/Network/TrainerController.py:84-127,143-156,
 * src/Network/loss_utils.py:64-103.
 * pred (N,V,3); uh,vh,wh (N,V); mask (N,V).  out (N,4) = {mse loss, rel-error %, sum(mask), sum(nonfluid)}.
 * dpred (N,V,3) = d(sum_b loss_b)/dpred, or NULL (test_step).  scratch: FDN_LOSS_SCRATCH_FLOATS(N) floats (per-block
 * partial sums, added up in a fixed order: the reported values are run-to-run identical). */
#define FDN_LOSS_BLOCKS 256
#define FDN_LOSS_SCRATCH_FLOATS(N) ((N) * (8 + 3 * FDN_LOSS_BLOCKS))
int fdn_loss_metrics(const float* pred, const float* uh, const float* vh, const float* wh, const float* mask,
                     float* out, float* dpred, float* scratch, int N, int64_t V, void* stream);

/* fdn_loss_metrics + the divergence loss the reference defines (src/Network/loss_utils.py:4-62) and weights into the loss
 * (src/Network/TrainerController.py:84-127, the lines 111-120 it ships commented out).  pred (N,D,H,W,3); uh,vh,wh,mask (N,D,H,W).
 * Along the axis paired with each channel (u: D, v: H, w: W) (Da x)[k] = x[clamp(k-1)] - x[clamp(k+1)] (SYMMETRIC pad 1 + the
 * conv3d cross-correlation); per voxel d = sum_c (Da pred_c - Da truth_c)^2; per sample
 * div_b = div_weight * (sum(mask d) / (sum(mask) + 1) + sum(nf d) / (sum(nf) + 1)), nf = mask < 0.5.
 * out (N,5) = {mse loss, rel-error %, sum(mask), sum(nonfluid), div_b}; the sample's loss is out[0] + out[4].
 * dpred (N,D,H,W,3) = d(sum_b (mse_b + div_b))/dpred, or NULL.  scratch: FDN_LOSS_DIV_SCRATCH_FLOATS(N) floats.  div_weight == 0:
 * columns 0-3 and dpred equal fdn_loss_metrics' bit for bit, column 4 is 0.  D*H*W < 2^31.  Run-to-run identical like
 * fdn_loss_metrics (no atomics beyond the mask counts).  Refuses NULL operands, non-positive extents and a non-finite or negative
 * weight before it touches the device. */
#define FDN_LOSS_DIV_SCRATCH_FLOATS(N) ((N) * (8 + 5 * FDN_LOSS_BLOCKS))
int fdn_loss_metrics_div(const float* pred, const float* uh, const float* vh, const float* wh, const float* mask,
                         float div_weight, float* out, float* dpred, float* scratch, int N, int D, int H, int W, void* stream);

/* fdn_loss_metrics_div with the reference's non_fluid_weight ("Weighting for non fluid region", src/Network/TrainerController.py:24)
 * and the activation of the heads that produced pred.  Same operands, out (N,5) layout, scratch size and determinism.  Per sample
 *   out[0] = sum(mask e^2) / (sum(mask) + 1) + non_fluid_weight * sum(nf e^2) / (sum(nf) + 1)
 *   out[4] = div_weight * (sum(mask d) / (sum(mask) + 1) + non_fluid_weight * sum(nf d) / (sum(nf) + 1));
 * the relative-error column and the two counts do not change.  dpred = d(sum_b (out[0] + out[4])) / d(head PRE-activations): with
 * out_act == FDN_ACT_TANH every component of the gradient w.r.t. pred is multiplied by fmaf(-y, y, 1.f), y that component of pred
 * (TensorFlow's TanhGrad: from the output; exactly 0 where y is exactly +-1); with FDN_ACT_NONE the two gradients are the same.
 * non_fluid_weight == 1 and out_act == FDN_ACT_NONE: out and dpred equal fdn_loss_metrics_div's bit for bit (at div_weight == 0 also
 * fdn_loss_metrics' columns 0-3 and dpred).  Refused before the device is touched: NULL operands, non-positive extents, D*H*W > 2^31 - 1,
 * a weight that is negative or not finite, an out_act other than FDN_ACT_NONE / FDN_ACT_TANH (FDN_ERR_UNSUPPORTED). */
int fdn_loss_metrics_act(const float* pred, const float* uh, const float* vh, const float* wh, const float* mask, float div_weight,
                         float non_fluid_weight, int out_act, float* out, float* dpred, float* scratch, int N, int D, int H, int W,
                         void* stream);

/* fdn_loss_metrics_act with a choice of the data term's penalty.  Per component of the residual d = pred_c - truth_c:
 *   FDN_LOSS_MSE          rho = d^2                                                   psi = 2 d     (TrainerController.calculate_mse)
 *   FDN_LOSS_MAE          rho = |d|                                                   psi = sign(d), psi(0) = 0 (tf.abs' gradient)
 *   FDN_LOSS_HUBER        rho = d^2 / 2 if |d| <= delta, else delta (|d| - delta / 2) psi = d, else delta sign(d)   (tf.keras.losses.Huber)
 *   FDN_LOSS_CHARBONNIER  rho = sqrt(d^2 + eps^2)                                     psi = d / sqrt(d^2 + eps^2)
 * kind_param: delta (Huber) or eps (Charbonnier), finite and > 0; 0 for MSE and MAE, which have none.  On velocities normalised to
 * [-1, 1] a delta of 1 (Keras' default) makes Huber half the MSE almost everywhere: choose a smaller one.
 * Per voxel e = sum_c rho(d_c), and e takes the place of e^2 in fdn_loss_metrics_act's column 0:
 *   out[0] = sum(mask e) / (sum(mask) + 1) + non_fluid_weight * sum(nf e) / (sum(nf) + 1).
 * The divergence term (out[4]) keeps its squared form for every kind; the relative-error column and the two counts do not depend on
 * the kind.  dpred = d(sum_b (out[0] + out[4])) / d(head pre-activations) with psi in the data term's part, exactly 0 where d is 0
 * (and div_weight is 0).  Same operands, out (N,5) layout, scratch size (FDN_LOSS_DIV_SCRATCH_FLOATS(N)), launches and determinism as
 * fdn_loss_metrics_act; kind == FDN_LOSS_MSE is that call, bit for bit.  Refused before the device is touched: NULL operands, an
 * unknown kind, a delta / eps that is not finite or <= 0, a non-zero kind_param for MSE / MAE, and everything fdn_loss_metrics_act
 * refuses. */
#define FDN_LOSS_MSE 0
#define FDN_LOSS_MAE 1
#define FDN_LOSS_HUBER 2
#define FDN_LOSS_CHARBONNIER 3
int fdn_loss_metrics_kind(const float* pred, const float* uh, const float* vh, const float* wh, const float* mask, int kind,
                          float kind_param, float div_weight, float non_fluid_weight, int out_act, float* out, float* dpred,
                          float* scratch, int N, int D, int H, int W, void* stream);

/* Whole-volume evaluation of a stitched prediction against the high-resolution truth: 26 sums per frame, from which the host derives the
 * reference's loss and metric (src/Network/TrainerController.py:96-107, src/Network/loss_utils.py:64-101), the divergence term, RMSE
 * and the regression line of prediction on truth.  pred (F,3,X,Y,Z) planar, fp32 (pred_is_f64 = 0) or float64 (1) -- what
 * predict_volume returns --; truth (F,3,X,Y,Z) fp32 in the same units; mask (mask_frames,X,Y,Z) fp32, mask_frames = 1 (one mask for
 * all frames) or F.  All arithmetic is in double (fp32 inputs convert exactly).  Per voxel, with p_c, t_c the prediction and truth of
 * component c and m the mask: e_c = p_c - t_c, q = e_u^2 + e_v^2 + e_w^2, nf = [m < 0.5] (TrainerController.py:96), fl = [m == 1.0]
 * (loss_utils.py:91); corr the relative error of loss_utils.py:64-92: diff = sqrt(q), actual = sqrt(sum t_c^2),
 * rel = clip(diff / (actual + 1e-5), 0, 1), corr = actual != 0 ? rel : diff, corr = rint(corr * 1e4) / 1e4; g_c = (Da e_c), the clamped
 * central difference of fdn_loss_metrics_div (e[clamp(k-1)] - e[clamp(k+1)]) along the axis paired with the component (u: X, v: Y,
 * w: Z; 0 on an axis of extent 1), d = sum_c g_c^2.  out (F,26) float64 on the device, sums over the frame:
 *   0,1,2: m, nf, fl    3,4: q m, q nf    5: corr fl    6,7,8: e_c^2 fl (c = u,v,w)    9,10: d m, d nf
 *   11+5c .. 15+5c: t_c fl, p_c fl, t_c^2 fl, p_c^2 fl, t_c p_c fl.
 * scratch: FDN_VOLUME_METRICS_SCRATCH_DOUBLES(F) caller-owned doubles of per-block partials, added in a fixed order (no atomics): two
 * calls give identical bits.  Three kernels of its own (volume_mask_sums, volume_metrics, volume_finalize); the main one runs once per group of
 * columns (3-8, 9-10, then the five moments of each component), and no column depends on that grouping.  At most FDN_LOSS_BLOCKS blocks per
 * frame.  Refused before the device is touched: NULL operands, non-positive extents, X*Y*Z > 2^31 - 1, mask_frames not in {1, F},
 * pred_is_f64 not in {0, 1}. */
#define FDN_VOLUME_METRICS_COLUMNS 26
#define FDN_VOLUME_METRICS_SCRATCH_DOUBLES(F) ((F) * FDN_VOLUME_METRICS_COLUMNS * FDN_LOSS_BLOCKS)
int fdn_volume_metrics(const void* pred, int pred_is_f64, const float* truth, const float* mask, int mask_frames,
                       double* out, double* scratch, int F, int X, int Y, int Z, void* stream);

/* On-device input pipeline: the per-sample slicing / np.rot90 / sign / normalisation / mask threshold of
 * PatchHandler3D.load_patches_from_index_file (src/Network/PatchHandler3D.py:49-160) as one gather per output
 * tensor.  desc: B device-resident descriptors of 56 bytes each
 *   { const float* src (T,X,Y,Z volume); int32 X,Y,Z,t, x0,y0,z0, plane (0 none,1:(0,1),2:(0,2),3:(1,2)), k (rot90 count),
 *     mode (0: out = sign*(v/div), 1: out = v >= div ? 1 : 0); float sign, div }
 * out: (B,S,S,S) patches, S = patch edge. */
int fdn_gather_patches(const void* desc, float* out, int B, int S, void* stream);

/* Sliding-window inference on the device (src/Network/PatchGenerator.py:13-40,53-86,116-154 and src/predictor.py:67-115): the patches of
 * the tiler are never materialised.  frames: (F,6,X,Y,Z) fp32, channels u,v,w,mag_u,mag_v,mag_w as ImageDataset.load_vectorfield
 * normalises them.  The window of edge P advances by E = P - 4 over the volume padded by 2 voxels per side (+ the far pad that makes
 * the stride tile it: nx,ny,nz patches per axis, tiler.PatchGenerator.plan).  Global patch g: frame f = g / (nx*ny*nz), then (i,j,k)
 * with k fastest; its voxel (a,b,c) reads source (i*E + a - 2, j*E + b - 2, k*E + c - 2), 0 outside [0,X)x[0,Y)x[0,Z).
 * The volume form of the input features: phase, pc (count,P,P,P,3) of patches g0 .. g0 + count - 1, equal bit for bit to
 * PatchGenerator.patchify followed by the plain entry point on those patches.  Its own kernel, input_features_volume_kernel (a by-value geometry).
 * Refused before the device is touched: NULL pointers, P <= 4, non-positive extents / counts, count <= 0, g0 < 0,
 * g0 + count > F*nx*ny*nz. */
int fdn_input_features_volume(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz, int64_t g0,
                              int count, float* phase, float* pc, void* stream);
/* Stitch (src/Network/PatchGenerator.py:13-40,53-86,116-154, src/predictor.py:67-115): pred (count,S,S,S,3) fp32, the predictions of
 * global patches g0 .. g0 + count - 1; vol (F,3,Xo,Yo,Zo) fp32.  With core = S - 2*side (side = 2 * res_increase HR voxels stripped per
 * patch side), core voxel (a,b,c) of patch (f,i,j,k) and component m goes to vol[f][m][i*core + a][j*core + b][k*core + c] iff that
 * lies inside (Xo,Yo,Zo): the crop of the far pad.  Patches write disjoint voxels (no atomics; any chunking gives the same volume); a
 * patch wholly inside the cropped region writes nothing.  The values are copied unchanged: de-normalisation stays with the caller.
 * Kernel: stitch_patches_kernel<false>.  Refused before the device is touched: NULL pointers, S <= 2*side,
 * count <= 0, g0 < 0, g0 + count > F*nx*ny*nz, an output extent <= 0 or > n*core. */
int fdn_stitch_patches(const float* pred, float* vol, int F, int Xo, int Yo, int Zo, int S, int side, int nx, int ny, int nz,
                       int64_t g0, int count, void* stream);
/* fdn_stitch_patches with the predictor's post-processing folded into the write (src/predictor.py:103-107, src/utils/ImageDataset.py:31):
 * vol (F,3,Xo,Yo,Zo) is FLOAT64 and frame_scale a caller-owned DEVICE table (F,2) of doubles {venc_f, threshold_f}.  A core voxel of
 * frame f with prediction p is written as d = (double)p * venc_f, or as +0.0 when fabs(d) < threshold_f (strict: a product equal to the
 * threshold is kept; a threshold of 0 zeroes nothing, round_small_values=False) -- the bits of
 * `v = stitched.astype(float64) * venc; v[abs(v) < velocity_per_px] = 0` on the host.  Geometry, crop rule and refusals are those of
 * fdn_stitch_patches, plus a NULL frame_scale.  side = 0 is legal in both: cores packed by fdn_pack_patch_cores are stitched with S = core.
 * Kernel: stitch_patches_kernel<true>, the same element walk. */
int fdn_stitch_patches_finish(const float* pred, double* vol, const double* frame_scale, int F, int Xo, int Yo, int Zo,
                              int S, int side, int nx, int ny, int nz, int64_t g0, int count, void* stream);
/* The cores of predicted patches, contiguous: pred (count,S,S,S,3) fp32 -> cores (count,c,c,c,3), c = S - 2*side,
 * cores[n][a][b][k][m] = pred[n][side+a][side+b][side+k][m].  The unit a data-parallel rank sends to the rank that stitches (patch 24
 * at x2: 40^3 of 48^3 voxels, 1.73x less transport); stitching the cores with side = 0 equals stitching pred with `side`, and finishing
 * them (src/predictor.py:103-107) is fdn_stitch_patches_finish on the receiver.  A pure copy (pack_patch_cores_kernel).
 * Refused before the device is touched: NULL pointers, side < 0, S <= 2*side, S > 512, count <= 0. */
int fdn_pack_patch_cores(const float* pred, float* cores, int S, int side, int count, void* stream);

/* Geometric self-ensemble: inference averaged over the patch rotations the loader trains with (PatchHandler3D.apply_rotation,
 * src/Network/PatchHandler3D.py:97-108,166-274).  An orientation is (plane, k): (0,0) the identity, else plane 1:(0,1), 2:(0,2), 3:(1,2)
 * (np.rot90 axes) with k = 1..3 quarter turns; (p,0), (0,k) and anything else are refused.  Each orientation has a component permutation
 * `perm` and a sign rule `sign` (the table of data._ROT); a patch v turns into  v'[i] = sign[i] * rot90(v[perm[i]], k, axes)  -- the
 * magnitudes with the same permutation and no sign -- and a prediction p' made in that frame turns back as
 * q[perm[i]] = sign[i] * rot90(p'[..., i], 4 - k, axes).
 *
 * fdn_input_features_volume with the window patch turned first: voxel (a,b,c) of patch g reads the window voxel np.rot90 puts there
 * (zero outside the volume), THEN the six values are permuted and the velocities multiplied by their sign -- a padded zero under a
 * negative sign is -0.0 -- and the norms are taken of the permuted components in their new order.  phase, pc equal, bit for bit and sign
 * of zero included, PatchGenerator.patchify -> apply_rotation -> fdn_input_features on those patches.  Orientation (0,0) is
 * fdn_input_features_volume itself.  The same kernel (the by-value geometry carries the orientation).  Refusals: those of
 * fdn_input_features_volume, and an orientation outside the set. */
int fdn_input_features_volume_oriented(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz, int64_t g0,
                                       int count, int plane, int k, float* phase, float* pc, void* stream);
/* The fan-in of the ensemble, the inverse of apply_rotation (src/Network/PatchHandler3D.py:97-108,166-274) on a prediction: pred and acc
 * are (count,S,S,S,3) fp32, pred the predictions made under orientation (plane, k).  For every
 * element of acc:  t = the element of q above (sign * pred at the rotated index and permuted component);  v = first ? t : acc + t;
 * acc = divisor > 1 ? v / (float)divisor : v.  Plain IEEE fp32 -- one add, and one correctly rounded divide on the call that carries the
 * count of orientations -- so numpy float32 reproduces it bit for bit; with first = 1 acc is not read.  (0,0), first = 1, divisor = 1 is a
 * copy.  The destination is walked (contiguous writes, no atomics; unrotate_accumulate_kernel).  Refused before the device is
 * touched: NULL pointers, count <= 0, S <= 0 or S > 512, an orientation outside the set, first not 0 or 1, divisor < 1, pred and acc
 * ranges that overlap. */
int fdn_unrotate_accumulate(const float* pred, float* acc, int count, int S, int plane, int k, int first, int divisor, void* stream);

/* Overlap-add stitching: neighbouring cores overlap by b low-res voxels and are cross-faded, which removes the step a one-verdict-per-voxel
 * stitch leaves at every core boundary.  With E = P - 4 the window advances by stride = E - b (1 <= stride <= E, 2b <= E: at most two cores
 * overlap per axis, eight per voxel); per axis nr = max(1, ceil((n - E) / stride) + 1) patches (tiler.PatchGenerator.plan_blend).
 *
 * fdn_input_features_volume_oriented with the window advancing by `stride`: voxel (a,b,c) of patch (i,j,k) reads source
 * (i*stride + a - 2, j*stride + b - 2, k*stride + c - 2), zero outside the volume.  stride == P - 4 equals the oriented entry point bit
 * for bit (and with (plane,k) = (0,0) the plain one).  The same kernel (the by-value geometry carries the stride).  Refusals:
 * those of fdn_input_features_volume_oriented, and stride < 1 or stride > P - 4. */
int fdn_input_features_volume_strided(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz, int64_t g0,
                                      int count, int stride, int plane, int k, float* phase, float* pc, void* stream);
/* The weighted accumulate.  pred (count,S,S,S,3) fp32, the predictions of global patches g0 .. g0 + count - 1; acc (F,3,Xo,Yo,Zo) fp32,
 * zeroed by the caller once per volume.  core = S - 2*side, stride_hr = stride * res_increase, r = core - stride_hr the ramp width.  Core
 * voxel t (per axis, 0 <= t < core) of patch i of nr has the weight  (float)(2t+1) / (float)(2r)  for t < r when i > 0 (a lower neighbour),
 * (float)(2(core-t)-1) / (float)(2r)  for t >= core - r when i < nr - 1 (an upper neighbour), 1 elsewhere: one correctly rounded fp32
 * divide each, the two ramps of an overlap sum to 1, and a volume face has no ramp.  The voxel weight is w = fl(fl(wx*wy)*wz).  For
 * every output voxel and component the call does  acc = acc + fl(w_g * p_g)  for the patches g of the call whose core covers the voxel, in
 * ascending g, the multiply and the add rounded separately (never fused).  The destination is walked -- each voxel finds its at most eight
 * covering patches from its coordinates and keeps those inside [g0, g0 + count) -- over the slab of the frames the patches of the call can
 * touch: no atomics, no two threads on one voxel, and after all patches of a volume the bits of acc do not depend on how [0, total) was
 * cut into calls, as long as the calls come in ascending g0; numpy float32 reproduces them exactly.  Voxels no patch of the call covers
 * are not written.  side = 0 with S = core blends cores packed by fdn_pack_patch_cores.  stride_hr == core is the disjoint stitch
 * (acc = 0 + p).  Kernel: blend_patches_kernel.  Refused before the device is touched: what fdn_stitch_patches refuses (with the
 * extent limit (n-1)*stride_hr + core per axis: extents the counts do not cover), stride_hr < 1, stride_hr > core, 2*(core - stride_hr) > core. */
int fdn_blend_patches(const float* pred, float* acc, int F, int Xo, int Yo, int Zo, int S, int side, int stride_hr, int nx, int ny, int nz,
                      int64_t g0, int count, void* stream);
/* The predictor's post-processing (src/predictor.py:103-107, src/utils/ImageDataset.py:31) on an accumulated volume: acc (F,3,Xo,Yo,Zo) fp32
 * -> vol of the same shape in FLOAT64 with the device table frame_scale (F,2) of doubles {venc_f, threshold_f}: d = (double)acc * venc_f,
 * +0.0 where fabs(d) < threshold_f (strict) -- the rule of fdn_stitch_patches_finish, word for word.  Kernel:
 * finish_volume_kernel.  Refused before the device is touched: NULL pointers, non-positive F or extents. */
int fdn_finish_volume(const float* acc, double* vol, const double* frame_scale, int F, int Xo, int Yo, int Zo, void* stream);

/* Low-res synthesis (prepare_data/fft_downsampling.py:6-137, downsample_phase_img): nvol velocity volumes vel (nvol,X,Y,Z) that share one
 * magnitude volume mag (X,Y,Z) -> out_vel, out_mag (nvol,2cx,2cy,2cz), all fp32 on the device.  params is a DEVICE table (nvol,4) of
 * {venc, mag_scale, snr_linear = 10^(SNRdb/10), 0}.  The crop half-widths are integers, c = int((N / 2) * crop_ratio) as the reference
 * computes them.  Per volume, in this order:
 *   1. x = mag * mag_scale * exp(i pi vel / venc)                         (sincospif(vel / venc): |vel| > venc wraps as in the reference)
 *   2. along X, Y, Z the truncated DFT that equals fftn -> fftshift -> centre crop -> fftshift: with M = 2c,
 *      F[k'] = sum_n x[n] exp(-2 pi i ((k n) mod N) / N),  k = k' for k' < c, else k' - M  (frequencies 0..c-1, -c..-1),  k' in 0..M-1
 *   3. P = mean |F|^2 over the 2cx*2cy*2cz samples, sigma = sqrt(P / snr_linear)   (per-workgroup partial sums, added in a fixed order by
 *      the kernel behind fdn_sum_partials: no atomics, reproducible bit for bit; sigma stays on the device)
 *   4. Re F += sigma * g: real noise on the complex spectrum (fft_downsampling.py:63-69).  g = noise[e], a caller's array of standard
 *      normals (nvol,2cx,2cy,2cz), or with noise == NULL generated in the kernel: e the element's linear index in that array,
 *      (x0,x1,..) = Philox4x32-10(counter (e lo32, e hi32, stream_id lo32, stream_id hi32), key (seed lo32, seed hi32)),
 *      u1 = ((x0 >> 9) + 0.5f) 2^-23, u2 = (x1 >> 8) 2^-24, g = sqrtf(-2 logf(u1)) cospif(2 u2)
 *   5. along X, Y, Z  z[m] = (1/M) sum_k' F[k'] exp(+2 pi i ((k' m) mod M) / M)
 *   6. out_mag = |z| * (2cx*2cy*2cz)/(X*Y*Z),  out_vel = atan2(Im z, Re z) / pi * venc
 * Six launches of kspace_stage_kernel (three forward, three inverse; the N or M unit roots of a stage sit in dynamic LDS, entry r =
 * sincospif(2.f * r / N), the index (k n) mod N formed in integers) with complex fp32 intermediates in `workspace`
 * (fdn_kspace_downsample_workspace_bytes, 16-byte aligned, caller-owned), plus the one-block sums.  No host synchronisation, no memcpy.
 * sigma_out (nvol floats on the device) may be NULL.
 * Refused before the device is touched, the message naming the argument: NULL vel, mag, params, out_vel, out_mag or workspace,
 * nvol outside 1..65535, an extent outside 1..1024, a crop outside 1..N/2, an output range that overlaps an input range or the other
 * output.  The workspace query returns 0 for arguments the call would refuse. */
size_t fdn_kspace_downsample_workspace_bytes(int nvol, int X, int Y, int Z, int cx, int cy, int cz);
int fdn_kspace_downsample(const float* vel, const float* mag, const float* params, int nvol, int X, int Y, int Z, int cx, int cy, int cz,
                          const float* noise, uint64_t seed, uint64_t stream_id, float* out_vel, float* out_mag, float* sigma_out,
                          void* workspace, void* stream);

/* sum of squares of the kernel (non-bias) parameters: the l2(5e-7) regulariser value is 5e-7 * out[0].
 * src/Network/TrainerController.py:129-141.  is_kernel: one byte per parameter. */
int fdn_l2_sumsq(const float* w, const uint8_t* is_kernel, int64_t n, float* out, void* stream);

/* Keras Adam on one flat buffer, with the L2-regulariser gradient folded in:
 * g' = g + l2_grad_scale * w (kernels only); m,v EMA; w -= lr_t * m / (sqrt(v) + eps).
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is computed by the caller.  If l2_scale_dev != NULL the scale is
 * l2_grad_scale * l2_scale_dev[0], read on the device (data-parallel: the global batch size rides in the
 * all-reduced gradient buffer, so no host synchronisation is needed).  TrainerController.py:73,225. */
int fdn_adam_step(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, int64_t n,
                  float lr_t, float b1, float b2, float eps, float l2_grad_scale, const float* l2_scale_dev,
                  float* sumsq_partials, void* stream);
/* If sumsq_partials != NULL (FDN_ADAM_PARTIALS floats) the step also leaves per-block sums of the UPDATED
 * kernel parameters' squares there; fdn_sum_partials adds them up in a fixed order (deterministic):
 * 5e-7 * that sum is the regulariser value of the next step's loss, so fdn_l2_sumsq need not stream the
 * parameters again.  src/Network/TrainerController.py:129-141. */
#define FDN_ADAM_PARTIALS 2048
/* fdn_adam_step with the step size read on the device: lr_t_dev[0] (one float, must not be NULL) instead of the by-value lr_t.
 * For a launch that is captured into a HIP graph and replayed: the caller rewrites that float before every replay.  Same
 * kernel, same arithmetic: with lr_t_dev[0] == (float)lr_t the update is bit-identical to fdn_adam_step. */
int fdn_adam_step_dev(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, int64_t n,
                      const float* lr_t_dev, float b1, float b2, float eps, float l2_grad_scale,
                      const float* l2_scale_dev, float* sumsq_partials, void* stream);
/* fdn_adam_step for fine-tuning (`layer.trainable = False`, TrainerController.py:223-225 update model.trainable_variables only):
 * frozen holds one byte per parameter like is_kernel.  An option of the same kernel, taken when frozen != NULL, on the grid of
 * fdn_adam_step (FDN_ADAM_PARTIALS blocks when partials are requested).  lr_t_dev != NULL: the step size is lr_t_dev[0], read on the
 * device as in fdn_adam_step_dev (a captured launch); otherwise the by-value lr_t.
 *   frozen[i] == 0: the arithmetic of fdn_adam_step -- w, m and v come out bit-identical to fdn_adam_step[_dev] on the same operands.
 *   frozen[i] != 0: w[i], m[i] and v[i] keep their bits; g[i], m[i] and v[i] are neither read nor written (a NaN or an uninitialised
 *                   gradient there is harmless).  The element still adds w[i]^2 to its block's partial when is_kernel[i].
 * The regulariser value covers every kernel, frozen or not (TrainerController.py:129-141 loops over all layers): sumsq_partials equals
 * fdn_l2_sumsq_partials of the resulting w bit for bit, as after fdn_adam_step.  The L2 gradient reaches unfrozen kernels only.
 * Refused before the device is touched, the message naming the argument: NULL w, g, m, v, is_kernel or frozen, n <= 0. */
int fdn_adam_step_masked(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, const uint8_t* frozen, int64_t n,
                         float lr_t, const float* lr_t_dev, float b1, float b2, float eps, float l2_grad_scale,
                         const float* l2_scale_dev, float* sumsq_partials, void* stream);
int fdn_sum_partials(const float* partials, int n, float* out, void* stream);
/* acc[i] = first ? g[i] : acc[i] + g[i], i in [0, n).  One fp32 add per element (IEEE, round-to-nearest-even):
 * first = 1 is a bit copy (no memset of acc is needed), first = 0 equals numpy's float32 acc + g bit for bit.
 * The sum of the micro-batch gradients of one optimiser step: TrainerController.py:223 (tape.gradient of the (B,)
 * loss vector = gradient of sum_b loss_b), :245-249 (L2 counted once per sample: the batch-size slot adds up too).
 * acc and g may sit at any float offset (gradient-bucket slices).  Kernel: grad_accumulate_kernel.
 * Refused before the device is touched: NULL acc or g, n <= 0, first not in {0, 1}, ranges that overlap (|acc - g| < n floats:
 * an in-place call would double a buffer silently). */
int fdn_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream);
/* The same FDN_ADAM_PARTIALS per-block sums for parameters no fdn_adam_step has touched yet (first step, after loading a
 * checkpoint): the multi-block form of fdn_l2_sumsq, which needs no scratch and runs as ONE block.  Follow with fdn_sum_partials. */
int fdn_l2_sumsq_partials(const float* w, const uint8_t* is_kernel, int64_t n, float* sumsq_partials, void* stream);

/* Gradient clipping: what tf.keras.optimizers.Adam(global_clipnorm=c) / Adam(clipvalue=c) do to the gradient before the update
 * (the reference builds its optimizer at TrainerController.py:73 and applies tape.gradient's result at :223-225; the L2 regulariser's
 * gradient is part of that result, so it is part of what is clipped).  The step's gradient is
 *     g'_i = g_i + l2s * w_i for kernel elements, g_i for biases,   l2s = l2_grad_scale * l2_scale_dev[0] (l2_grad_scale alone if NULL),
 * formed in fp32 as fdn_adam_step forms it, over the elements with frozen[i] == 0 (every element if frozen == NULL).
 *
 * fdn_grad_sumsq_partials: partials[b] (FDN_ADAM_PARTIALS floats) = block b's sum of g'_i^2 on the blocking of fdn_adam_step with
 * partials (block b takes the elements b * 256 + t + k * FDN_ADAM_PARTIALS * 256); no atomics, a fixed order, blocks beyond the data write 0.
 * Where frozen[i] != 0, g[i] is not read (a NaN there is harmless) and the element adds +0.  Nothing but partials is written.  Kernel:
 * grad_sumsq_partials_kernel.  TrainerController.py:73,223-225.
 * Refused before the device is touched, the message naming the argument: NULL g, w, is_kernel or partials, n <= 0. */
int fdn_grad_sumsq_partials(const float* g, const float* w, const uint8_t* is_kernel, const uint8_t* frozen /* NULL ok */, int64_t n,
                            float l2_grad_scale, const float* l2_scale_dev /* NULL ok */, float* partials, void* stream);
/* tf.clip_by_global_norm's factor from those partials, one block, the fixed order of fdn_sum_partials (clip_scale_kernel):
 *     out[0] = N = sqrtf(sum of the n_partials partials) = sqrt(sum g'_i^2),     out[1] = s = clip_norm / max(N, clip_norm).
 * s is exactly 1.0f whenever N <= clip_norm: an inactive clip changes no bit.  TF writes clip_norm * min(1 / N, 1 / clip_norm), which
 * rounds twice where this rounds once; the two agree to rounding.  Non-finite rule: if N is not finite (an inf or NaN gradient, or
 * squares that overflow fp32), s = NaN, and the clipped step makes every unfrozen parameter NaN -- TF: "entries are all set to NaN to
 * signify that an error occurred".  Both floats stay on the device: out[0] is for telemetry, out + 1 is the g_scale_dev of
 * fdn_adam_step_clipped.  TrainerController.py:73,223-225.
 * Refused before the device is touched: NULL partials or out, n_partials <= 0, clip_norm not finite or <= 0. */
int fdn_clip_scale(const float* partials, int n_partials, float clip_norm, float* out /* 2 floats */, void* stream);
/* The Adam step on the clipped gradient (TrainerController.py:73,223-225): the operands of fdn_adam_step_masked (frozen and lr_t_dev may
 * be NULL here) and
 *     g_scale_dev != NULL: g''_i = g'_i * g_scale_dev[0]  (global_clipnorm: one fp32 multiply behind the L2 term, s of fdn_clip_scale);
 *     clip_value > 0:      g''_i = g'_i > clip_value ? clip_value : (g'_i < -clip_value ? -clip_value : g'_i)  (clipvalue: comparisons,
 *                          so a NaN gradient stays NaN);   with both, the multiply comes first.
 * Everything behind g'' is fdn_adam_step's arithmetic statement for statement: m, v, the update, sumsq_partials of the new parameters.
 * With g_scale_dev == NULL and clip_value == 0 the results are bit-identical to fdn_adam_step / fdn_adam_step_dev /
 * fdn_adam_step_masked on the same operands; so they are with g_scale_dev[0] == 1.0f.  Non-finite rule: g_scale_dev[0] = NaN makes
 * w, m and v of every unfrozen element NaN; frozen elements keep their bits.
 * Refused before the device is touched, the message naming the argument: NULL w, g, m, v or is_kernel, n <= 0, clip_value negative or NaN. */
int fdn_adam_step_clipped(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, const uint8_t* frozen /* NULL ok */,
                          int64_t n, float lr_t, const float* lr_t_dev /* NULL ok */, float b1, float b2, float eps, float l2_grad_scale,
                          const float* l2_scale_dev /* NULL ok */, const float* g_scale_dev /* NULL ok */, float clip_value,
                          float* sumsq_partials /* NULL ok */, void* stream);
/* Weight EMA: what tf.keras.optimizers.Adam(use_ema=True, ema_momentum=mom) keeps beside the weights ([TF]-unpinned: TensorFlow is
 * absent, the recurrence below is the specification).  fdn_adam_step_clipped's operands -- the widest form: frozen, lr_t_dev,
 * l2_scale_dev and g_scale_dev may be NULL, clip_value may be 0 -- and the average ema (n floats), an option of the same kernel.  With
 * wi the weight the element held before the step and wn the weight the step stores, in fp32:
 *     ema_init == 0:    ema[i] = ema_momentum * ema[i] + (1.f - ema_momentum) * wn   (a_t = mom * a_{t-1} + (1 - mom) * w_t);
 *     ema_init != 0:    ema[i] = ema_momentum * wi + (1.f - ema_momentum) * wn       (the first step with an average: a_0 = w_0, the
 *                       weights before the step; ema[i] is not read, so the buffer may be uninitialised);
 *     frozen[i] != 0:   ema[i] = wi, a store of the value already loaded: the average of a currently frozen parameter is its weight,
 *                       whatever was trainable earlier.  g[i], m[i] and v[i] stay unread.
 * The average is formed from wn in the register, right behind the store of w[i]; nothing else depends on it: with ema the call leaves
 * bit-identical w, m, v, partials to the same call of fdn_adam_step_clipped without it.  Once per optimiser step; no collective
 * (data-parallel ranks form identical averages from identical weights).
 * Refused before the device is touched, the message naming the argument: NULL w, g, m, v, is_kernel or ema, n <= 0, ema_momentum outside
 * [0, 1) or NaN, clip_value negative or NaN. */
int fdn_adam_step_ema(float* w, const float* g, float* m, float* v, const uint8_t* is_kernel, const uint8_t* frozen /* NULL ok */,
                      int64_t n, float lr_t, const float* lr_t_dev /* NULL ok */, float b1, float b2, float eps, float l2_grad_scale,
                      const float* l2_scale_dev /* NULL ok */, const float* g_scale_dev /* NULL ok */, float clip_value,
                      float* ema, float ema_momentum, int ema_init, float* sumsq_partials /* NULL ok */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 activation path (BASELINE.json configs[3]: patch 32, res x4, bf16).  The reference has no bf16
 * mode (TF runs fp32); semantics = the fp32 entry points above with every activation / activation-gradient
 * tensor stored as bfloat16 (uint16_t bit patterns, round-to-nearest-even on store), fp32 accumulation,
 * fp32 parameters, gradients of parameters and optimizer state.
 * ------------------------------------------------------------------------------------------------ */

/* fp32 Keras kernel (27,64,64) -> bf16 operand streams (27*64*64 uint16_t each) for the two entry points below. */
int fdn_pack_conv64_weights_bf16(const float* w, uint16_t* wp_fwd, uint16_t* wp_dgrad, void* stream);
/* The same for n_layers kernels in ONE launch (after every optimizer step, TrainerController.py:225): layer i at
 * w_base + w_offsets[i] (DEVICE array of float offsets), its streams at packs + i * 2 * 27*64*64 (forward, then dgrad). */
int fdn_pack_conv64_weights_bf16_batch(const float* w_base, const int64_t* w_offsets, int n_layers, uint16_t* packs,
                                       void* stream);

/* fdn_conv3d_fwd for (Cin,Cout,K) = (64,64,3) with bf16 x / residual / y.  SR4DFlowNet.py:93-120. */
int fdn_conv64_fwd_bf16(const uint16_t* x, const uint16_t* wpack, const float* bias, const uint16_t* residual,
                        uint16_t* y, int N, int D, int H, int W, int act, float alpha, void* stream);

/* fdn_conv3d_dgrad_fused / fdn_fold_halo_border with bf16 dz / skip / y_prev / dz_prev; the padded scratch
 * dxpad (N,D+2,H+2,W+2,64) stays fp32 (only positions the border fold reads are written). */
int fdn_conv64_dgrad_fused_bf16(const uint16_t* dz, const uint16_t* wpack, float* dxpad, const uint16_t* skip,
                                const uint16_t* y_prev, int act, float alpha, uint16_t* dz_prev, int N, int D, int H,
                                int W, void* stream);
int fdn_fold_halo_border_bf16(const float* dxpad0, const float* dxpad1, const float* dxpad2, int nsrc,
                              const uint16_t* skip, const uint16_t* y_prev, int act, float alpha, uint16_t* dz_prev,
                              int N, int D, int H, int W, void* stream);
/* Sign masks.  The activation gradient of SR4DFlowNet.py:113,118 (LeakyReLU) / :17-25 (ReLU) needs one bit of the producer's
 * output: y > 0.  fdn_conv64_fwd_bf16_mask is fdn_conv64_fwd_bf16 that also writes, when y_mask != NULL, 64 bits per voxel
 * -- four uint16_t words [voxel][cout / 16], bit c % 16 = (the stored bf16 y[c] > 0) -- i.e. (N*D*H*W*4) uint16_t;
 * fdn_conv64_dgrad_fused_bf16_mask reads that mask for act' instead of the 128-B rows of y_prev when y_mask != NULL
 * (y_prev may then be NULL; act must be RELU or LEAKY).  Same results bit for bit; at (4,128^3) the launch is 0.14 ms
 * (8 %) shorter -- an epilogue operand of these kernels costs what streaming its 1.07 GB costs.  The border fold
 * (fdn_fold_halo_border_bf16) still takes y_prev itself: it touches the surface voxels only. */
int fdn_conv64_fwd_bf16_mask(const uint16_t* x, const uint16_t* wpack, const float* bias, const uint16_t* residual,
                             uint16_t* y, uint16_t* y_mask, int N, int D, int H, int W, int act, float alpha,
                             void* stream);
int fdn_conv64_dgrad_fused_bf16_mask(const uint16_t* dz, const uint16_t* wpack, float* dxpad, const uint16_t* skip,
                                     const uint16_t* y_prev, const uint16_t* y_mask, int act, float alpha,
                                     uint16_t* dz_prev, int N, int D, int H, int W, void* stream);
/* fdn_conv64_dgrad_fused_multi for bf16 activations: the fused dgrad of up to three 64->64 layers that share their input as ONE launch
 * (+ one fdn_fold_halo_border_bf16), the sum over the sources kept in the fp32 accumulators -- the chained launches round the running sum
 * to bf16 after every source, so this form is the more accurate one (it differs from the chain by bf16 roundings of the partial sums).
 * Every grid (all kernel variants of the bf16 path walk the sources).  y_prev or y_mask or neither. */
int fdn_conv64_dgrad_fused_bf16_multi(const uint16_t* const* dz, const uint16_t* const* wpack, int nsrc, float* dxpad,
                                      const uint16_t* skip, const uint16_t* y_prev, const uint16_t* y_mask, int act, float alpha,
                                      uint16_t* dz_prev, int N, int D, int H, int W, void* stream);

/* The remaining entry points of the path in bf16 storage: same contracts as the fp32 functions of the same
 * name.  Parameters, parameter gradients, the 64->1 heads' output (the prediction, `y` of Cout=1) and its
 * gradient (`dz` of Cout=1) stay fp32. */
int fdn_input_features_bf16(const float* u, const float* v, const float* w, const float* mu, const float* mv,
                            const float* mw, uint16_t* phase, uint16_t* pc, int64_t nvox, void* stream);
/* The volume form with bf16 phase / pc (src/Network/PatchGenerator.py:13-40,53-86,116-154, src/predictor.py:67-115); frames stay fp32. */
int fdn_input_features_volume_bf16(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz, int64_t g0,
                                   int count, uint16_t* phase, uint16_t* pc, void* stream);
/* fdn_input_features_volume_oriented with bf16 phase / pc (src/Network/PatchHandler3D.py:97-108,166-274); frames stay fp32. */
int fdn_input_features_volume_oriented_bf16(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz, int64_t g0,
                                            int count, int plane, int k, uint16_t* phase, uint16_t* pc, void* stream);
/* fdn_input_features_volume_strided with bf16 phase / pc; frames stay fp32. */
int fdn_input_features_volume_strided_bf16(const float* frames, int F, int X, int Y, int Z, int P, int nx, int ny, int nz, int64_t g0,
                                           int count, int stride, int plane, int k, uint16_t* phase, uint16_t* pc, void* stream);
int fdn_conv3d_fwd_bf16(const uint16_t* x, const uint16_t* x2, const float* w, const uint16_t* wpack, const float* bias,
                        const uint16_t* residual, void* y, int N, int D, int H, int W, int Cin, int Cout, int K, int ldy,
                        int y_coff, int act, float alpha, void* stream);
size_t fdn_conv3d_wgrad_bf16_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int K);
int fdn_conv3d_wgrad_bf16(const uint16_t* x, const uint16_t* x2, const void* dz, float* dw, float* dbias, void* workspace,
                          size_t workspace_bytes, int N, int D, int H, int W, int Cin, int Cout, int K, int lddz,
                          int dz_coff, void* stream);
/* fdn_conv3d_wgrad_batch for bf16 activations: the weight gradients (TrainerController.py:223) of several 64->64 3x3x3 layers of
 * ONE grid -- x, dz, dw, dbias: HOST arrays of n_layers device pointers (dbias or its entries may be NULL) -- in chunks of up to
 * seven layers per launch (+ one reduction per chunk) where the grid allows, else layer by layer; results equal
 * fdn_conv3d_wgrad_bf16 per layer to fp32 rounding (a different split of the voxel sum). */
size_t fdn_conv3d_wgrad_bf16_batch_workspace_bytes(int n_layers, int N, int D, int H, int W);
int fdn_conv3d_wgrad_bf16_batch(const uint16_t* const* x, const uint16_t* const* dz, float* const* dw, float* const* dbias,
                                int n_layers, void* workspace, size_t workspace_bytes, int N, int D, int H, int W,
                                void* stream);
int fdn_conv_cout1_dgrad_folded_bf16(const float* dz, const float* w, const uint16_t* y_prev, int act, float alpha,
                                     uint16_t* dz_prev, float* dbias_prev, void* workspace, size_t workspace_bytes,
                                     int N, int D, int H, int W, int lddz, int dz_coff, void* stream);
/* ... with the sign mask of y_prev (written by fdn_conv64_fwd_bf16_mask for the 64->64 head conv that produced it) read for act'
 * instead of its 128-B rows when y_mask != NULL; same results bit for bit. */
int fdn_conv_cout1_dgrad_folded_bf16_mask(const float* dz, const float* w, const uint16_t* y_prev, const uint16_t* y_mask,
                                          int act, float alpha, uint16_t* dz_prev, float* dbias_prev, void* workspace,
                                          size_t workspace_bytes, int N, int D, int H, int W, int lddz, int dz_coff,
                                          void* stream);
int fdn_conv1x1_dgrad_bf16(const uint16_t* dz, const float* w, const uint16_t* ya, const uint16_t* yb, uint16_t* dxa,
                           uint16_t* dxb, int64_t nvox, void* stream);
int fdn_upsample_trilinear_fwd_bf16(const uint16_t* x, uint16_t* y, int N, int D, int H, int W, int C, int R, void* stream);
int fdn_upsample_trilinear_bwd_bf16(const uint16_t* dy, const uint16_t* y_prev, int act, float alpha, uint16_t* dx, int N,
                                    int D, int H, int W, int C, int R, void* stream);

#ifdef __cplusplus
}
#endif
#endif

"""Host-side mirror of src/Network/SR4DFlowNet.py: the network graph, expressed as a fixed schedule of calls
into lib4dflow_hip.so.  Same names and argument meaning as the reference (SR4DFlowNet(res_increase)
.build_network(u, v, w, u_mag, v_mag, w_mag, low_resblock, hi_resblock, channel_nr)); the returned model is
callable on 6 arrays (B,P,P,P,1), has .predict(list), .trainable_variables, .save / .load_weights, and adds
.backward(dpred) (what tape.gradient does in TrainerController.py:223).

Parameters live in ONE flat fp32 device buffer in layer CREATION order (kernel, bias per layer: conv3d, conv3d_1, ...
conv3d_35), gradients in a second flat buffer of the same layout, so the data-parallel all-reduce and the Adam step are one
call each.  Keras' own `trainable_variables` order (depth-sorted layers, keras_layer_order) differs from creation order and
is what optimizer.pkl uses: keras_variable_order() / trainable_variable_names() translate between the two.

Fine-tuning: every layer has the Keras `trainable` flag (model.layers[i].trainable = False, or set_trainable).  trainable_variables and
the two helpers above then cover the trainable layers only, `variables` / get_weights / save all of them; backward_plan says what
backward() launches and forward(training=True) retains for a given set."""
import contextlib
import math
import os

import numpy as np
import torch

from . import ops, ops_bf16
from ._lib import FdnError

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH = ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY, ops.ACT_TANH


def output_activation_code(name):
    """('linear' | 'tanh', ACT_*) of the heads' output activation: None and 'linear' are the reference's v2 network (README.md:11), 'tanh'
    the bounded heads its first published weights were trained with (Keras' Conv3D(activation='tanh'))."""
    if name is None or name == "linear":
        return "linear", ACT_NONE
    if name == "tanh":
        return "tanh", ACT_TANH
    raise ValueError("output_activation must be None, 'linear' or 'tanh', got %r" % (name,))


class Input:
    """Placeholder with the role of tf.keras.layers.Input(shape=..., name=...) (TrainerController.py:38-44)."""

    def __init__(self, shape, name=None):
        self.shape = (None,) + tuple(shape)
        self.name = name


def layer_specs(low_resblock=8, hi_resblock=4):
    """[(name, K, Cin, Cout, use_bias)] in Keras creation order (SR4DFlowNet.py:17-46)."""
    specs = []

    def add(k, cin, cout, bias):
        i = len(specs)
        specs.append(("conv3d" if i == 0 else "conv3d_%d" % i, k, cin, cout, bias))

    add(3, 3, 64, True); add(3, 64, 64, True)        # pc path        :17-18
    add(3, 3, 64, True); add(3, 64, 64, True)        # phase path     :20-21
    add(1, 128, 64, True); add(3, 64, 64, True)      # concat fuse    :24-25
    for _ in range(low_resblock + hi_resblock):      # ResBlocks      :29-30,35-36 (no bias)
        add(3, 64, 64, False); add(3, 64, 64, False)
    for _ in range(3):                               # u,v,w heads    :39-46
        add(3, 64, 64, True); add(3, 64, 1, True)
    return specs


def keras_layer_order(low_resblock=8, hi_resblock=4):
    """Indices (into layer_specs) of the conv layers in the order tf.keras lists them in `model.layers` -- and hence their
    variables in `model.trainable_variables` / `optimizer.get_weights()` (TrainerController.py:223,347-394).

    A functional Keras model sorts its layers by depth from the output, deepest first, and within one depth by the order
    in which a depth-first walk from the output reaches them [TF 2.x `Network._map_graph_network` / `_build_map`; restated from
    the published algorithm, TensorFlow is absent here].  Only layers at EQUAL depth can change places relative to creation
    order, and the graph of SR4DFlowNet.py:7-51 has two such groups:
      * the pc and phase branches -- the walk enters `concatenate([phase, pc])` (:23) through `phase` first, so at each depth
        the phase conv precedes the pc conv: conv3d_2, conv3d, conv3d_3, conv3d_1;
      * the three heads -- `concatenate([u_path, v_path, w_path])` (:49) is entered through u first: the three 64->64 convs
        (conv3d_30, _32, _34 at cfg2), then the three 64->1 convs (conv3d_31, _33, _35).
    tests/golden/make_golden_tf.py stores the variable names a real TensorFlow produces; tests/test_tf_golden.py checks this
    function against them when that file exists."""
    n_trunk = 6 + 2 * (low_resblock + hi_resblock)
    h = n_trunk
    return [2, 0, 3, 1] + list(range(4, n_trunk)) + [h, h + 2, h + 4, h + 1, h + 3, h + 5]


def trainable_flags(spec, low_resblock=8, hi_resblock=4):
    """One bool per layer of layer_specs (creation order) for a FlowNetModel.set_trainable spec: "all", "hires" (the hi-res ResBlocks and the
    six head layers), "heads" (the six head layers), or an iterable of layer names (ValueError for a name the model does not have)."""
    names = [s[0] for s in layer_specs(low_resblock, hi_resblock)]
    n = len(names)
    if spec is None or (isinstance(spec, str) and spec == "all"):
        return [True] * n
    if isinstance(spec, str) and spec == "hires":
        return [i >= 6 + 2 * low_resblock for i in range(n)]
    if isinstance(spec, str) and spec == "heads":
        return [i >= n - 6 for i in range(n)]
    if isinstance(spec, str):
        raise ValueError("set_trainable: %r is not 'all', 'hires', 'heads' or an iterable of layer names" % (spec,))
    want = set(spec)
    unknown = sorted(str(k) for k in want if k not in names)
    if unknown:
        raise ValueError("set_trainable: unknown layer(s) %s" % unknown)
    return [nm in want for nm in names]


def variable_names(low_resblock=8, hi_resblock=4, flags=None):
    """Keras variable names ('conv3d_7/kernel:0', 'conv3d_7/bias:0') in creation order, of the layers whose flag is set (None: all)."""
    out = []
    for i, (name, _, _, _, ub) in enumerate(layer_specs(low_resblock, hi_resblock)):
        if flags is None or flags[i]:
            out.append("%s/kernel:0" % name)
            if ub:
                out.append("%s/bias:0" % name)
    return out


def keras_variable_positions(low_resblock=8, hi_resblock=4, flags=None):
    """Positions into variable_names(..., flags) in Keras `trainable_variables` order: keras_layer_order restricted to the flagged layers
    (Keras lists the variables of the trainable layers in the order of model.layers, so a subset keeps its relative order)."""
    first = {}
    k = 0
    for i, (_, _, _, _, ub) in enumerate(layer_specs(low_resblock, hi_resblock)):
        if flags is None or flags[i]:
            first[i] = (k, 2 if ub else 1)
            k += first[i][1]
    out = []
    for i in keras_layer_order(low_resblock, hi_resblock):
        if i in first:
            out.extend(range(first[i][0], first[i][0] + first[i][1]))
    return out


def backward_plan(low_resblock, hi_resblock, flags, upsample=True):
    """What backward() has to launch, and forward(training=True) to retain, when only the layers with flags[i] set are trainable.  Pure:
    no tensors, no device.  Layer i (creation order) gets
      wgrad[i]   its weight (+bias) gradient is computed: the layer is trainable;
      dgrad[i]   the gradient w.r.t. its input is computed: some trainable layer lies upstream of that input.
    The graph (SR4DFlowNet.py:7-51): pc -> 0 -> 1 and phase -> 2 -> 3 meet in the 1x1 layer 4, then 5, then the ResBlocks (two layers
    each; the skip adds nothing upstream that the convs do not have), the upsample behind block `low_resblock`, and the three heads
    (64->64 then 64->1) on the last trunk tensor.  Every layer below layer i of the trunk is upstream of it, so in the trunk
    dgrad[i] = any(flags[:i]); backward stops at the lowest trainable layer.
    Derived facts: any_trainable; heads_to_trunk (the heads' input gradient is formed); need_at[k] (the gradient of trunk tensor k is
    needed: k = 0 the output of layer 5, k = j that of block j); through_upsample; conv1x1_dgrad; branch_phase / branch_pc (descend that
    branch behind the 1x1); dbias_prev[h] (head h's 64->64 bias gradient, emitted by the folded 64->1 dgrad).
    keep / masks: for each tensor / sign mask forward(training=True) can retain, whether backward reads it: phase, pc, a0, a1, p0, p1,
    c0, trunk[k], up_out, h[j] (a block's inner activation), heads[h].  `upsample`: res_increase > 1 (there is an up_out)."""
    LB, HB = int(low_resblock), int(hi_resblock)
    nb = LB + HB
    nt = 6 + 2 * nb
    n = nt + 6
    t = [bool(f) for f in flags]
    if len(t) != n:
        raise ValueError("backward_plan: %d flags for %d layers" % (len(t), n))
    below = [any(t[:i]) for i in range(n + 1)]            # below[i]: a layer of index < i is trainable
    dgrad = [False, t[0], False, t[2]] + [below[i] for i in range(4, nt)]
    for h in range(3):
        dgrad += [below[nt], below[nt] or t[nt + 2 * h]]
    need_at = [below[6 + 2 * k] for k in range(nb + 1)]
    head1 = any(t[nt + 2 * h] for h in range(3))
    keep = dict(phase=t[2], pc=t[0], a0=t[1] or dgrad[1], p0=t[3] or dgrad[3], a1=t[4] or dgrad[4], p1=t[4] or dgrad[4], c0=t[5] or dgrad[5],
                trunk=[], up_out=False, h=[t[7 + 2 * j] or dgrad[7 + 2 * j] for j in range(nb)],
                heads=[t[nt + 2 * h + 1] or dgrad[nt + 2 * h + 1] for h in range(3)])
    masks = dict(trunk=[], h=[dgrad[7 + 2 * j] for j in range(nb)], heads=[dgrad[nt + 2 * h + 1] for h in range(3)])
    for k in range(nb + 1):
        # readers of trunk tensor k: the upsample's act' (it feeds the upsample), else the next block's first layer (x of its weight
        # gradient, act' of its dgrad) or, for the last one, the heads (x of the three 64->64 weight gradients, act' of their dgrad)
        if upsample and k == LB:
            keep["trunk"].append(need_at[k])
            masks["trunk"].append(False)
            # linear producer: read as x of a weight gradient only -- and, where the heads sit on it, as the shape of their input gradient
            keep["up_out"] = (head1 or below[nt]) if k == nb else t[6 + 2 * k]
        elif k == nb:
            keep["trunk"].append(head1 or below[nt])
            masks["trunk"].append(below[nt])
        else:
            keep["trunk"].append(t[6 + 2 * k] or dgrad[6 + 2 * k])
            masks["trunk"].append(dgrad[6 + 2 * k])
    return dict(wgrad=t, dgrad=dgrad, any_trainable=below[n], all_trainable=all(t), heads_to_trunk=below[nt], need_at=need_at,
                through_upsample=need_at[LB], conv1x1_dgrad=below[4], branch_phase=t[2] or t[3], branch_pc=t[0] or t[1],
                dbias_prev=[t[nt + 2 * h] for h in range(3)], keep=keep, masks=masks)


def slow_grid_warning(N, D, H, W):
    """The warning for an fp32 (N, D, H, W) grid whose 64->64 layers FDN_ALGO_AUTO runs off the 2-D Winograd kernels -- all of them on the
    direct kernels, or on the 1-D Winograd kernels -- or None.  The library's own selection decides (fdn_conv64_pack_streams)."""
    how = {ops.PACK_STREAM_DIRECT: "the direct kernels (about 3x the time of the 2-D Winograd kernels)",
           ops.PACK_STREAM_WINO_W: "the 1-D Winograd kernels (about 1.5x the time of the 2-D Winograd kernels)"}.get(
        ops.conv64_pack_streams(N, D, H, W, ops.ALGO_AUTO, ops.ROLE_FWD))
    if how is None:
        return None
    return ("4dflownet_amd: the 64->64 3x3x3 layers of the %dx%dx%d grid run on %s: FDN_ALGO_AUTO takes the 2-D Winograd kernels "
            "only where W %% 4 == 0 and H is even (fastest: H %% 4 == 0 as well).  patch_size * res_increase (and patch_size "
            "itself for the low-res stack) a multiple of 4 avoids this." % (D, H, W, how))


class _Layer:
    """`trainable` (default True) is the Keras flag: `model.layers[i].trainable = False` freezes the layer from the next forward(training=True)."""
    __slots__ = ("name", "k", "cin", "cout", "w", "b", "gw", "gb", "wp_f", "wp_d", "w_off", "b_off", "trainable")


class _T:
    """An activation tensor + the activation of the op that produced it (needed to form act'(y) in backward) + (bf16 mode, training) the
    sign mask its 64->64 producer wrote beside it: the fused dgrad reads 8 B per voxel of that instead of the 128-B rows of y (ops_bf16)."""
    __slots__ = ("t", "act", "mask")

    def __init__(self, t, act, mask=None):
        self.t = t
        self.act = act
        self.mask = mask


class FlowNetModel:
    def __init__(self, res_increase, low_resblock=8, hi_resblock=4, device=None, seed=0, dtype="float32", conv_algo=None,
                 output_activation=None):
        """dtype: storage type of activations and activation gradients -- "float32" (the reference's arithmetic) or
        "bfloat16" (BASELINE.json configs[3]; parameters, their gradients, the prediction and the optimizer stay fp32).
        conv_algo (fp32 mode): algorithm of the 64->64 3x3x3 layers -- "auto" (FDN_ALGO_AUTO: 2-D Winograd forward / dgrad, F(4,3) along
        H x F(4,3) along W where H and W are multiples of 4, F(2,3) along H where H is only even, Winograd along W where only W allows
        it, else direct -- forward() warns once per grid that falls off the 2-D kernels), "winograd_h2" (FDN_ALGO_WINO_H2: never more
        than F(2,3) along H, round 4's kernels), "winograd_w" (FDN_ALGO_WINO_W: the 1-D kernels only), "direct" (FDN_ALGO_DIRECT
        everywhere), or a dict {layer name: "direct"} that pins single layers (forward, dgrad and wgrad of that layer) to the direct
        kernels; None reads FDN_CONV_ALGO (default "auto").
        output_activation: None / 'linear' (the reference's network) or 'tanh' (bounded heads, FDN_ACT_TANH in the heads' epilogue); kept
        as self.output_activation, its ACT_* code as self.out_act -- what ops.loss_metrics(out_act=) needs to hand backward() the
        gradient w.r.t. the heads' pre-activations."""
        self.output_activation, self.out_act = output_activation_code(output_activation)
        if not torch.cuda.is_available():
            raise FdnError("FlowNetModel needs a ROCm GPU: the hot path is HIP-only (no CPU fallback)")
        dtype = {"float32": "float32", "fp32": "float32", "f32": "float32", torch.float32: "float32",
                 "bfloat16": "bfloat16", "bf16": "bfloat16", torch.bfloat16: "bfloat16"}.get(dtype)
        if dtype is None:
            raise ValueError("dtype must be 'float32' or 'bfloat16'")
        self.dtype = dtype
        self.ops = ops if dtype == "float32" else ops_bf16
        self.act_dtype = self.ops.ACT_DTYPE
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.res_increase = int(res_increase)
        self.low_resblock = int(low_resblock)
        self.hi_resblock = int(hi_resblock)
        self.specs = layer_specs(low_resblock, hi_resblock)
        n = sum(k ** 3 * ci * co + (co if ub else 0) for _, k, ci, co, ub in self.specs)
        self.n_params = n
        self.flat_w = torch.zeros(n, device=self.device, dtype=torch.float32)
        # gradient buffer + one trailing slot that carries the per-rank batch size through the data-parallel all-reduce
        self.flat_g_ext = torch.zeros(n + 1, device=self.device, dtype=torch.float32)
        self.flat_g = self.flat_g_ext[:n]
        self.batch_slot = self.flat_g_ext[n:n + 1]
        is_kernel = np.zeros(n, dtype=np.uint8)
        self.layers = []
        off = 0
        n64 = sum(1 for _, k, ci, co, _ in self.specs if (k, ci, co) == (3, 64, 64))
        # (zero-filled: a pack holds five streams and only the ones the model's grids read are kept current -- _pack_streams below; the others
        # stay zero, not garbage.  The packs are private to forward() / backward(): read L.wp_f / L.wp_d elsewhere only through
        # _require_pack_streams, or re-pack everything with ops.pack_conv64_weights_batch(..., streams=None).)
        self._packs = torch.zeros((n64, 2, self.ops.PACK_ELEMS), device=self.device, dtype=self.act_dtype)
        i64 = 0
        for name, k, ci, co, ub in self.specs:
            L = _Layer()
            L.name, L.k, L.cin, L.cout = name, k, ci, co
            L.trainable = True
            sz = k ** 3 * ci * co
            L.w_off = off
            L.w = self.flat_w[off:off + sz].view(k, k, k, ci, co)
            L.gw = self.flat_g[off:off + sz].view(k, k, k, ci, co)
            is_kernel[off:off + sz] = 1
            off += sz
            if ub:
                L.b_off = off
                L.b = self.flat_w[off:off + co]
                L.gb = self.flat_g[off:off + co]
                off += co
            else:
                L.b_off = -1
                L.b = L.gb = None
            if (k, ci, co) == (3, 64, 64):
                L.wp_f, L.wp_d = self._packs[i64, 0], self._packs[i64, 1]
                i64 += 1
            else:
                L.wp_f = L.wp_d = None
            self.layers.append(L)
        assert off == n
        self.is_kernel = torch.tensor(is_kernel, device=self.device)
        self._w64_offsets = torch.tensor([L.w_off for L in self.layers if L.wp_f is not None], device=self.device, dtype=torch.int64)
        # fine-tuning: the flags the current plan was made for (layer.trainable is compared against them, _sync_trainable), what backward()
        # launches and forward(training=True) retains under them (backward_plan), the device byte map of frozen parameters (None: none
        # frozen) and the contiguous runs of trainable 64->64 layers in _packs
        self._flags = (True,) * len(self.layers)
        self._plan = backward_plan(self.low_resblock, self.hi_resblock, self._flags, upsample=self.res_increase > 1)
        self._frozen_map = None
        self._pack_runs = [(0, n64)] if n64 else []
        self.weights_version = 0       # bumped by weights_changed(): lets the trainer know whether Adam's sum-of-squares is current
        self._ws = None
        self._ws_bias = None
        self._side = None              # second HIP stream for the weight-gradient launches
        # weight gradients of 64->64 layers on small grids are collected per gradient bucket and issued as ONE batched launch
        # (fdn_conv3d_wgrad_batch): at 8 x 24^3 a layer alone on the chip leaves a workgroup 4.6 tiles between prologue and output
        # transform.  The batch ends where the bucket does, so the data-parallel all-reduce of a bucket starts as early as before.
        self.batch_wgrad = os.environ.get("FDN_BATCH_WGRAD", "1") not in ("", "0")
        # the input gradients of the three heads' 64->64 convs (they all read the last ResBlock's output) as ONE multi-source launch
        # (FDN_MULTI_DGRAD=0: three chained launches; equal to fp32 rounding in fp32, bf16 roundings of the partial sums apart in bf16 mode)
        self.multi_dgrad = os.environ.get("FDN_MULTI_DGRAD", "1") not in ("", "0")
        self.batch_wgrad_max_voxels = 1 << 18          # per launch; the 48^3 layers of cfg2 (8 x 110 592 voxels) fill the chip on their own
        self._wg_pending = []
        # weight gradients on a second HIP stream (they are leaves of the backward graph: they fill the tails of the dgrad launches and
        # the gaps the thin kernels leave; bit-identical results).  FDN_OVERLAP_WGRAD=0 issues everything on one stream -- what a
        # per-kernel timing pass wants (bench.py takes its HIP-event pass that way, in steps of its own).
        self.overlap_wgrad = os.environ.get("FDN_OVERLAP_WGRAD", "1") not in ("", "0")
        self._ws_side = None           # the side stream's own workspace (allocated and re-allocated under that stream: see _workspace)
        self._side_keep = []           # operands of side-stream launches, kept alive until the streams are joined
        self._side_busy = False        # the side stream has been given work since the last join
        self.set_conv_algo(conv_algo)
        self._cache = None
        # Gradient buckets in the order backward() completes them: slices [lo, hi) of flat_g_ext that are final when the hi-res part
        # (heads + hi-res blocks, together with the trailing batch slot), the upper half of the low-res blocks and the rest are done.
        # The data-parallel trainer starts one all-reduce per bucket as soon as it is final (trainer.train_step).
        cut_hi = self.layers[6 + 2 * self.low_resblock].w_off
        cut_mid = self.layers[6 + 2 * (self.low_resblock // 2)].w_off
        self.grad_buckets = [b for b in ((cut_hi, n + 1), (cut_mid, cut_hi), (0, cut_mid)) if b[1] > b[0]]
        self._slow_warned = set()
        # streams of the 64->64 packs that are kept current (fp32 mode): [forward packs, dgrad packs].  A pack holds four streams
        # and a grid reads one or two of them, so the per-step re-pack writes only what forward() has found the grids of this model
        # to read (_require_pack_streams asks the library's own selection code, widens the set and re-packs when a new grid or
        # algorithm needs more); nothing else reads the packs.
        self._pack_streams = [0, 0]
        # bf16 training: 64->64 layers write a sign mask beside their output and the fused dgrad reads it for act' instead of the output
        # (FDN_BF16_SIGN_MASK=0: read y, the round-4 behaviour -- same results bit for bit, for A/B timing)
        self.sign_masks = os.environ.get("FDN_BF16_SIGN_MASK" if dtype == "bfloat16" else "FDN_SIGN_MASK", "1") not in ("", "0")
        self._mask_ok_cache = {}
        self._pack_need_cache = {}
        self.glorot_uniform_init(seed)

    def set_conv_algo(self, conv_algo=None):
        """See __init__.  Takes effect from the next forward()."""
        if conv_algo is None:
            conv_algo = os.environ.get("FDN_CONV_ALGO", "auto")
        names = {"auto": ops.ALGO_AUTO, "winograd": ops.ALGO_AUTO, "direct": ops.ALGO_DIRECT, "winograd_w": ops.ALGO_WINO_W, "winograd_h2": ops.ALGO_WINO_H2,
                 "winograd_bf16x3": ops.ALGO_WINO_BF16X3}
        per_layer = {}
        if isinstance(conv_algo, dict):
            per_layer, conv_algo = conv_algo, conv_algo.get("*", "auto")
        if conv_algo not in names or any(v not in names for v in per_layer.values()):
            raise ValueError("conv_algo must be 'auto', 'winograd_bf16x3', 'winograd_h2', 'winograd_w', 'direct' or {layer name: one of these}")
        known = set(L.name for L in self.layers)
        unknown = [k for k in per_layer if k != "*" and k not in known]
        if unknown:
            raise ValueError("conv_algo: unknown layer(s) %s" % unknown)
        self.conv_algo = dict((L.name, names[per_layer.get(L.name, conv_algo)]) for L in self.layers)
        # FDN_ALGO_WINO_BF16X3 runs persistent workgroups that hold every CU's registers and LDS for the whole launch: a weight-gradient
        # launch on the second stream cannot share a CU with them and the two streams take turns badly (measured 28.9 ms one stream,
        # 39.4 ms two at cfg2).  Models that use it keep everything on one stream unless FDN_OVERLAP_WGRAD says otherwise.
        if ops.ALGO_WINO_BF16X3 in self.conv_algo.values() and "FDN_OVERLAP_WGRAD" not in os.environ and hasattr(self, "overlap_wgrad"):
            self.overlap_wgrad = False

    # ------------------------------------------------------------------ parameters
    def glorot_uniform_init(self, seed=0):
        """Keras default for kernel_initializer=None: GlorotUniform, zero bias (SR4DFlowNet.py:104).
        Drawn with numpy default_rng(seed) layer by layer in creation order."""
        rng = np.random.default_rng(seed)
        flat = np.zeros(self.n_params, dtype=np.float32)
        for L in self.layers:
            fan_in, fan_out = L.k ** 3 * L.cin, L.k ** 3 * L.cout
            limit = math.sqrt(6.0 / (fan_in + fan_out))
            wv = rng.uniform(-limit, limit, size=(L.k, L.k, L.k, L.cin, L.cout)).astype(np.float32)
            flat[L.w_off:L.w_off + wv.size] = wv.reshape(-1)
        self.flat_w.copy_(torch.from_numpy(flat))
        self.weights_changed()

    def weights_changed(self, trainable_only=False):
        """Re-derive the MFMA operand streams after any parameter update (Adam step, load_weights).  trainable_only (the trainer, after an
        optimiser step): frozen layers did not move, so only the trainable 64->64 layers are re-packed -- one launch per contiguous run of
        them in the pack buffer; with every layer trainable that is the one launch over all of them."""
        self.weights_version += 1
        if not self._w64_offsets.numel():
            return
        if not trainable_only:                             # all 64->64 layers, the streams in use (fp32), one launch
            self.ops.pack_conv64_weights_batch(self.flat_w, self._w64_offsets, self._packs, streams=self._pack_streams)
            return
        self._sync_trainable()
        for a, b in self._pack_runs:
            if (a, b) == (0, self._w64_offsets.numel()):
                self.ops.pack_conv64_weights_batch(self.flat_w, self._w64_offsets, self._packs, streams=self._pack_streams)
            else:
                self.ops.pack_conv64_weights_batch(self.flat_w, self._w64_offsets[a:b], self._packs[a:b], streams=self._pack_streams)

    # ------------------------------------------------------------------ fine-tuning: frozen layers
    def set_trainable(self, spec):
        """Which layers train: "all", "hires" (the hi-res ResBlocks and the six head layers), "heads" (the six head layers) or an iterable
        of layer names (ValueError for an unknown one).  The same as setting layer.trainable on every layer; takes effect from the next
        forward(training=True)."""
        for L, f in zip(self.layers, trainable_flags(spec, self.low_resblock, self.hi_resblock)):
            L.trainable = f
        self._sync_trainable()

    def _sync_trainable(self):
        """Bring the plan, the frozen byte map and the pack runs in line with the layers' `trainable` flags.  On a change the gradient
        ranges of frozen layers are zeroed once: backward() never writes them afterwards, so accumulation and the data-parallel
        all-reduce work on them unchanged."""
        flags = tuple(bool(L.trainable) for L in self.layers)
        if flags == self._flags:
            return
        self._flags = flags
        self._plan = backward_plan(self.low_resblock, self.hi_resblock, flags, upsample=self.res_increase > 1)
        self._cache = None                                 # retained under another plan
        frozen = np.zeros(self.n_params, dtype=np.uint8)
        for L, f in zip(self.layers, flags):
            if not f:
                hi = L.b_off + L.cout if L.b is not None else L.w_off + L.w.numel()
                frozen[L.w_off:hi] = 1
                self.flat_g[L.w_off:hi].zero_()
        self._frozen_map = None if all(flags) else torch.from_numpy(frozen).to(self.device)
        runs = []
        f64 = [f for L, f in zip(self.layers, flags) if L.wp_f is not None]
        for i, f in enumerate(f64):
            if f and runs and runs[-1][1] == i:
                runs[-1] = (runs[-1][0], i + 1)
            elif f:
                runs.append((i, i + 1))
        self._pack_runs = runs

    @property
    def any_trainable(self):
        self._sync_trainable()
        return self._plan["any_trainable"]

    @property
    def frozen_map(self):
        """One uint8 per parameter (like is_kernel), 1 in the ranges of frozen layers, on the device -- or None while every layer trains."""
        self._sync_trainable()
        return self._frozen_map

    @property
    def variables(self):
        """Kernel, bias per layer, ALL layers in creation order (get_weights / set_weights / save / load_weights follow this, whatever is
        frozen -- unlike Keras, which lists the non-trainable weights last; the weight files go by layer name anyway)."""
        out = []
        for L in self.layers:
            out.append(L.w)
            if L.b is not None:
                out.append(L.b)
        return out

    def variable_names(self):
        """Keras variable names ('conv3d_7/kernel:0', 'conv3d_7/bias:0'), one per entry of self.variables."""
        return variable_names(self.low_resblock, self.hi_resblock)

    @property
    def trainable_variables(self):
        """The variables of the trainable layers, creation order (TrainerController.py:223-225 differentiates and updates these)."""
        out = []
        for L in self.layers:
            if L.trainable:
                out.append(L.w)
                if L.b is not None:
                    out.append(L.b)
        return out

    def keras_variable_order(self):
        """Positions (into self.trainable_variables) in Keras `trainable_variables` order: see keras_layer_order."""
        return keras_variable_positions(self.low_resblock, self.hi_resblock, [bool(L.trainable) for L in self.layers])

    def trainable_variable_names(self):
        """Keras variable names ('conv3d_7/kernel:0', 'conv3d_7/bias:0'), one per entry of self.trainable_variables (creation order)."""
        return variable_names(self.low_resblock, self.hi_resblock, [bool(L.trainable) for L in self.layers])

    def get_weights(self):
        return [t.detach().cpu().numpy().copy() for t in self.variables]

    def set_weights(self, arrays):
        tv = self.variables
        if len(arrays) != len(tv):
            raise ValueError("set_weights: expected %d arrays, got %d" % (len(tv), len(arrays)))
        for t, a in zip(tv, arrays):
            a = np.asarray(a, dtype=np.float32)
            if tuple(a.shape) != tuple(t.shape):
                raise ValueError("set_weights: shape mismatch %s vs %s" % (a.shape, tuple(t.shape)))
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self.weights_changed()

    def save(self, path):
        from . import weights_io
        weights_io.save_model_weights(self, path)

    def load_weights(self, path):
        from . import weights_io
        weights_io.load_model_weights(self, path)

    # ------------------------------------------------------------------ forward
    def _to_dev(self, a):
        if isinstance(a, torch.Tensor):
            t = a.to(device=self.device, dtype=torch.float32)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(self.device)
        return t.contiguous()

    def _warn_slow_grid(self, N, D, H, W):
        """FDN_ALGO_AUTO picks the 64->64 kernel by the grid's extents (include/fdn.h); a grid that falls off the 2-D Winograd kernels is
        a silent 1.5x - 3x slowdown of every such layer -- say so once per grid (only for launches big enough to matter)."""
        if self.dtype != "float32" or (D, H, W) in self._slow_warned or N * D * H * W < (1 << 15):
            return
        self._slow_warned.add((D, H, W))
        if not any(a == ops.ALGO_AUTO for a in self.conv_algo.values()):
            return
        msg = slow_grid_warning(N, D, H, W)
        if msg:
            import warnings
            warnings.warn(msg, RuntimeWarning, stacklevel=4)

    def _require_pack_streams(self, N, D, H, W, training):
        """Make sure the pack streams the 64->64 layers read on this grid are current (see __init__; a bf16 pack has none to select)."""
        algos = tuple(sorted(set(self.conv_algo[L.name] for L in self.layers if L.wp_f is not None)))
        key = (N, D, H, W, training, algos)
        need = self._pack_need_cache.get(key)
        if need is None:
            f = d = 0
            for a in algos:
                f |= self.ops.conv64_pack_streams(N, D, H, W, a, ops.ROLE_FWD)
                if training:
                    d |= self.ops.conv64_pack_streams(N, D, H, W, a, ops.ROLE_DGRAD_FUSED)
            need = self._pack_need_cache[key] = (f, d)
        new = [need[0] & ~self._pack_streams[0], need[1] & ~self._pack_streams[1]]
        if new[0] or new[1]:
            self._pack_streams = [self._pack_streams[0] | new[0], self._pack_streams[1] | new[1]]
            if self._w64_offsets.numel():
                self.ops.pack_conv64_weights_batch(self.flat_w, self._w64_offsets, self._packs, streams=new)

    def _conv(self, x, L, act, residual=None, x2=None, out=None, ldy=None, y_coff=0, mask=None):
        """mask (training, a dense 64->64 layer): also receives the sign mask of the output."""
        return self.ops.conv3d_fwd(x, L.w, L.b, act, ops.LEAKY_ALPHA, residual, x2, L.wp_f, out, ldy, y_coff, algo=self.conv_algo[L.name],
                                   mask=mask)

    def _mask_ok(self, x, L):
        """Do the forward and the fused dgrad of this grid write / read sign masks (fp32: the plain F(4,3) x F(4,3) kernels; bf16: all)?"""
        key = (tuple(x.shape[:4]), self.conv_algo[L.name])
        ok = self._mask_ok_cache.get(key)
        if ok is None:
            ok = self._mask_ok_cache[key] = self.ops.conv64_mask_ok(*key[0], key[1])
        return ok

    def _conv_m(self, x, L, act, residual=None, want_mask=False):
        """A 64->64 layer and, in training, the sign mask of its output (None where the kernels of the grid do not write one)."""
        if want_mask and self.sign_masks and act != ACT_NONE and self._mask_ok(x, L):
            mask = self.ops.new_sign_mask(x)
            return self._conv(x, L, act, residual=residual, mask=mask), mask
        return self._conv(x, L, act, residual=residual), None

    def forward(self, inputs, training=False):
        """inputs: [u, v, w, u_mag, v_mag, w_mag], each (B,P,P,P,1) or (B,P,P,P).  Returns a device tensor
        (B,PR,PR,PR,3).  With training=True every activation backward needs is kept in self._cache."""
        u, v, w, mu, mv, mw = [self._to_dev(a) for a in inputs]
        if u.dim() == 5:
            B, D, H, W = u.shape[:4]
        else:
            B, D, H, W = u.shape
        self._prepare_grid(B, D, H, W, training)
        phase = torch.empty((B, D, H, W, 3), device=self.device, dtype=self.act_dtype)
        pc = torch.empty((B, D, H, W, 3), device=self.device, dtype=self.act_dtype)
        self.ops.input_features(u, v, w, mu, mv, mw, phase, pc)
        return self._forward_body(phase, pc, training)

    def _prepare_grid(self, B, D, H, W, training):
        """Slow-grid warnings and pack streams of the LR grid and of the upsampled one."""
        R = self.res_increase
        self._warn_slow_grid(B, D, H, W)
        self._require_pack_streams(B, D, H, W, training)
        if R > 1:                                          # (the three head convs run on the upsampled grid whatever hi_resblock is)
            if self.hi_resblock > 0:
                self._warn_slow_grid(B, D * R, H * R, W * R)
            self._require_pack_streams(B, D * R, H * R, W * R, training)

    def forward_features(self, phase, pc, training=False):
        """forward() entered behind input_features: phase, pc (B,P,P,P,3) device tensors of the activation dtype, e.g. from
        ops.input_features_volume (the sliding window of predictor.predict_volume).  Same result as forward() on the inputs they
        were computed from."""
        want = (self.device, self.act_dtype)
        for n, t in (("phase", phase), ("pc", pc)):
            if t.dim() != 5 or t.shape[4] != 3 or (t.device, t.dtype) != want or not t.is_contiguous():
                raise FdnError("forward_features: %s must be a contiguous (B,D,H,W,3) %s tensor on %s" % (n, want[1], want[0]))
        if phase.shape != pc.shape:
            raise FdnError("forward_features: phase %s and pc %s differ" % (tuple(phase.shape), tuple(pc.shape)))
        self._prepare_grid(*phase.shape[:4], training)
        return self._forward_body(phase, pc, training)

    def _forward_body(self, phase, pc, training):
        R = self.res_increase
        Ls = self.layers
        # training with frozen layers: retain, and request sign masks for, only what the plan says backward() reads.  With every layer
        # trainable (`full`) the cache and the masks are what they always were.
        full = True
        if training:
            self._sync_trainable()
            full = self._plan["all_trainable"]
            keep, masks = self._plan["keep"], self._plan["masks"]
        kept = lambda t, what, i=None: t if full or (keep[what] if i is None else keep[what][i]) else None
        linear = _T(None, ACT_NONE)                        # stands for the upsample's output where only its (absent) activation matters
        want = lambda what, i: training and (full or masks[what][i])
        a0 = self._conv(pc, Ls[0], ACT_RELU)
        a1 = self._conv(a0, Ls[1], ACT_RELU)
        p0 = self._conv(phase, Ls[2], ACT_RELU)
        p1 = self._conv(p0, Ls[3], ACT_RELU)
        if training:
            a0, p0, phase, pc = kept(a0, "a0"), kept(p0, "p0"), kept(phase, "phase"), kept(pc, "pc")
        c0 = self._conv(p1, Ls[4], ACT_RELU, x2=a1)          # concat [phase, pc] never materialised (:23)
        if training:
            a1, p1 = kept(a1, "a1"), kept(p1, "p1")
        c1, m_c1 = self._conv_m(c0, Ls[5], ACT_RELU, want_mask=want("trunk", 0))
        if training:
            c0 = kept(c0, "c0")
        rb = _T(c1, ACT_RELU, m_c1)
        rb_is = ("trunk", 0)                               # what rb is to the plan: trunk tensor k, or the upsample's output
        if not full:
            c1 = None                                      # (backward reads it through the trunk tensors below)
        del m_c1
        blocks = []
        hmasks = []                                        # bf16 training: sign mask of every block's inner activation h (else None)
        up = None
        li = 6
        nb = self.low_resblock + self.hi_resblock
        for i in range(nb + 1):
            if i == self.low_resblock and R > 1:
                up_out = _T(self.ops.upsample_trilinear_fwd(rb.t, R), ACT_NONE)
                up = (rb, up_out) if not training else (kept(rb, "trunk", i), kept(up_out, "up_out"))
                rb, rb_is = up_out, ("up_out", None)
                del up_out
            if i == nb:
                break
            h, m_h = self._conv_m(rb.t, Ls[li], ACT_LEAKY, want_mask=want("h", i))
            out, m_out = self._conv_m(h, Ls[li + 1], ACT_LEAKY, residual=rb.t, want_mask=want("trunk", i + 1))
            if full:
                blocks.append((rb, h, out))
            elif training:
                blocks.append((kept(rb, *rb_is) or (linear if rb.act == ACT_NONE else None), kept(h, "h", i), None))
            hmasks.append(m_h)
            rb, rb_is = _T(out, ACT_LEAKY, m_out), ("trunk", i + 1)
            del h, m_h, out, m_out
            li += 2
        pred = torch.empty(tuple(rb.t.shape[:4]) + (3,), device=self.device)
        heads = []
        gmasks = []                                         # bf16 training: sign masks of the three head activations (else None)
        for hidx in range(3):
            g, m_g = self._conv_m(rb.t, Ls[li], ACT_RELU, want_mask=want("heads", hidx))
            self._conv(g, Ls[li + 1], self.out_act, out=pred, ldy=3, y_coff=hidx)
            heads.append(g if not training else kept(g, "heads", hidx))
            gmasks.append(m_g)
            del g, m_g
            li += 2
        if training:
            rb = kept(rb, *rb_is)
            self._cache = dict(phase=phase, pc=pc, a0=a0, a1=a1, p0=p0, p1=p1, c0=c0, c1=c1, blocks=blocks, up=up,
                               rb=rb, heads=heads, hmasks=hmasks, gmasks=gmasks)
        return pred

    __call__ = forward

    def predict(self, inputs, batch_size=None):
        """Keras Model.predict: numpy in, numpy out (predictor.py:87)."""
        n = len(inputs[0])
        bs = n if not batch_size else batch_size
        outs = []
        for s in range(0, n, bs):
            outs.append(self.forward([a[s:s + bs] for a in inputs]).cpu().numpy())
        return np.concatenate(outs, axis=0)

    # ------------------------------------------------------------------ backward
    def _workspace(self, nbytes, side=False):
        """Scratch of the weight-gradient launches.  One block per stream, each allocated (and, when a later layer needs more,
        re-allocated) while ITS stream is current: the caching allocator then hands a freed block only to later work of the same
        stream, i.e. behind the kernels that may still be using it."""
        if side:
            if self._ws_side is None or self._ws_side.numel() * 4 < nbytes:
                with torch.cuda.stream(self._side):
                    self._ws_side = torch.empty((nbytes + 3) // 4, device=self.device, dtype=torch.float32)
            return self._ws_side
        if self._ws is None or self._ws.numel() * 4 < nbytes:
            self._ws = torch.empty((nbytes + 3) // 4, device=self.device, dtype=torch.float32)
        return self._ws

    @contextlib.contextmanager
    def _on_side(self):
        """Run the body on the second HIP stream, behind everything the current stream has been given; _join_side() brings it back."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(torch.cuda.current_stream())
        self._side_busy = True
        with torch.cuda.stream(self._side):
            yield

    def _wgrad(self, x, dz, L, x2=None, lddz=None, dz_coff=0, bias=True):
        """Weight (+bias) gradient of layer L into the flat gradient buffer.  Weight gradients are leaves of the backward
        graph (nothing downstream reads them before the optimizer), so they run on a second HIP stream and fill the tails
        of the dgrad chain's kernels; backward() joins the streams before returning."""
        N, D, H, W = x.shape[:4]
        if (self.batch_wgrad and (L.k, L.cin, L.cout) == (3, 64, 64) and x2 is None and lddz is None and
                N * D * H * W <= self.batch_wgrad_max_voxels and self.ops.conv64_wgrad_batch_ok(self.conv_algo[L.name])):
            self._wg_pending.append((x, dz, L, bias))        # issued by _flush_wgrads() at the end of the gradient bucket
            return
        nws = self.ops.wgrad_workspace_bytes(N, D, H, W, L.cin, L.cout, L.k)
        with self._on_side() if self.overlap_wgrad else contextlib.nullcontext():      # (side stream: behind the main one, so dz is ready)
            self.ops.conv3d_wgrad(x, dz, L.k, L.cin, L.cout, x2=x2, dw=L.gw, dbias=L.gb if bias else None,
                                  workspace=self._workspace(nws, side=self.overlap_wgrad), lddz=lddz, dz_coff=dz_coff, algo=self.conv_algo[L.name])
        if self.overlap_wgrad:
            self._side_keep.extend(t for t in (x, dz, x2) if t is not None)     # alive until the streams are joined (see _join_side)

    def _flush_wgrads(self):
        """Issue the collected weight gradients: layers of one grid and algorithm as one batched launch, a lone layer as before."""
        pending, self._wg_pending = self._wg_pending, []
        groups = {}
        for x, dz, L, bias in pending:
            groups.setdefault((tuple(x.shape[:4]), self.conv_algo[L.name]), []).append((x, dz, L, bias))
        for (shape, algo), items in groups.items():
            N, D, H, W = shape
            side = self.overlap_wgrad
            with self._on_side() if side else contextlib.nullcontext():
                if len(items) == 1:
                    x, dz, L, bias = items[0]
                    ws = self._workspace(self.ops.wgrad_workspace_bytes(N, D, H, W, 64, 64, 3), side=side)
                    self.ops.conv3d_wgrad(x, dz, 3, 64, 64, dw=L.gw, dbias=L.gb if bias else None, workspace=ws, algo=algo)
                else:
                    ws = self._workspace(self.ops.wgrad_batch_workspace_bytes(len(items), N, D, H, W), side=side)
                    self.ops.conv3d_wgrad_batch([i[0] for i in items], [i[1] for i in items], [i[2].gw for i in items],
                                                [i[2].gb if i[3] else None for i in items], workspace=ws, algo=algo)
            if side:
                for x, dz, _, _ in items:
                    self._side_keep.extend((x, dz))

    def _join_side(self):
        """The main stream waits for everything the side stream has been given; the operands of those launches may be freed after it.
        (Holding references until the join instead of Tensor.record_stream: with record_stream the caching allocator could not reuse a
        block until the side stream had passed its free point, took fresh device memory for the main stream meanwhile and never came
        back -- 0.8 GB per step, 96 GB reserved after 120 cfg2 steps, and one 2.9-s step when it finally had to give the cache back.)"""
        if self._side is not None and self._side_busy:    # (an idle side stream is not waited for: under stream capture it has not
            torch.cuda.current_stream().wait_stream(self._side)          # joined the capture, and a wait for it would end the capture)
            self._side_busy = False
        self._side_keep.clear()

    def _pad_like(self, t):
        N, D, H, W, C = t.shape
        return torch.empty((N, D + 2, H + 2, W + 2, C), device=t.device, dtype=torch.float32)

    def _dgrad_fused(self, dz, L, pad, out, skip, y_prev, act, mask):
        """One fused dgrad launch of the 64->64 layer L into out / pad: act'(y_prev) from `mask`, the sign mask of y_prev, where there is one
        and the kernels of this grid and algorithm read masks, else from y_prev (None: the producer was linear)."""
        if mask is not None and (y_prev is None or not self._mask_ok(dz, L)):
            mask = None
        self.ops.conv3d_dgrad_fused(dz, L.wp_d, pad, out, skip=skip, y_prev=y_prev, act=act, algo=self.conv_algo[L.name], mask=mask)

    def _dgrad_fold(self, dz, L, skip, y_prev, act, mask=None):
        """dz_prev = (MirrorPadGrad(Conv3DBackpropInput(dz)) + skip) * act'(y_prev) for a 64->64 layer: interior voxels
        are finished by the conv epilogue, the surface by one small border kernel.  mask: the sign mask of y_prev, read by the conv
        epilogue instead of y_prev itself (bf16 mode; fp32 on the grids of the F(4,3) x F(4,3) kernels)."""
        out = torch.empty_like(dz)
        pad = self._pad_like(dz)
        self._dgrad_fused(dz, L, pad, out, skip, y_prev, act, mask)
        self.ops.fold_halo_border([pad], out, skip, y_prev, act)
        return out

    def backward(self, dpred, grad_ready=None):
        """Fill self.flat_g with d(sum_b loss_b)/d(params) given dpred (B,PR,PR,PR,3); L2 is NOT included here
        (it is folded into the Adam kernel).  Consumes the cache of the last forward(training=True).
        dpred is the gradient w.r.t. the heads' PRE-activations: what ops.loss_metrics(..., out_act=self.out_act) returns.  For the
        linear model that is the gradient w.r.t. the prediction; under output_activation='tanh' the loss pass has already multiplied
        it by 1 - pred^2, and nothing below knows about the activation.
        grad_ready(lo, hi), if given, is called once per entry of self.grad_buckets, in that order, as soon as every launch that
        writes flat_g_ext[lo:hi] has been enqueued.
        STREAM of the callback: with overlap_wgrad on (and a weight-gradient stream in existence) it runs with that SIDE stream
        current, right after the side stream has been made to wait for the main one -- so what it launches is ordered behind every
        writer of the bucket on both streams, and the dgrad chain on the main stream does not stop for it.  Otherwise it runs on the
        main stream.  The JOIN (main waits for side, _join_side) sits after the last weight gradient and BEFORE the callbacks of the
        buckets still open at that point: those callbacks again put work on the side stream, which backward() does not join.  A caller
        whose callback launches more than a collective it later waits for (the trainer's accumulate of a bucket, accum_steps > 1) joins
        once more itself (_join_side) before the main stream consumes the result."""
        def bucket_done(k):
            self._flush_wgrads()                            # the batched weight gradients of this bucket's layers
            if grad_ready is not None and k < len(self.grad_buckets):
                if self._side is not None and self.overlap_wgrad:
                    # the bucket is complete once BOTH streams have run what they hold: the callback (the trainer starts the bucket's
                    # all-reduce in it) is issued from the side stream after that stream has been made to wait for the main one, so the
                    # collective is ordered behind both and the dgrad chain on the main stream does not stop for it
                    with self._on_side():
                        grad_ready(*self.grad_buckets[k])
                else:
                    grad_ready(*self.grad_buckets[k])
        done = 0
        c = self._cache
        if c is None:
            raise FdnError("backward() without forward(training=True)")
        self._cache = None
        # what to launch (backward_plan): a frozen layer gets no weight gradient -- its range of flat_g stays the zeros _sync_trainable
        # left --, and no input gradient is formed below the lowest trainable layer.  forward(training=True) retained under the same plan.
        plan = self._plan
        wg, dg = plan["wgrad"], plan["dgrad"]
        Ls = self.layers
        R = self.res_increase
        rb = c["rb"]
        li = len(Ls) - 6
        def act_of(t):                     # (tensor for act', act) of a producer; linear producers need no mask
            return (t.t if t.act != ACT_NONE else None), t.act

        # three heads fan into rb: chain the interior accumulation through `dz` (skip aliases the output),
        # apply act'(rb) on the last one, then one border fold over the three padded scratches
        to_trunk = plan["heads_to_trunk"]
        dz = torch.empty_like(rb.t) if to_trunk else None
        pads = []
        # ONE multi-source launch forms the sum of the three input gradients in its registers (ops.conv3d_dgrad_fused_multi; fp32: on the
        # grids of the F(4,3) x F(4,3) kernels) instead of three chained launches that re-read and re-write the running sum
        multi = (to_trunk and self.multi_dgrad and self.ops.conv64_dgrad_multi_ok([self.conv_algo[Ls[li + 2 * h].name] for h in range(3)])
                 and self._mask_ok(rb.t, Ls[li]))
        dz_gs = []
        for hidx in range(3):
            L1, L2 = Ls[li], Ls[li + 1]
            g = c["heads"][hidx]
            c["heads"][hidx] = None
            if wg[li + 1]:
                self._wgrad(g, dpred, L2, lddz=3, dz_coff=hidx)
            m_g = c["gmasks"][hidx]
            c["gmasks"][hidx] = None
            if not dg[li + 1]:                 # this head's 64->64 conv and everything below it are frozen
                del g, m_g
                li += 2
                continue
            # the folded head dgrad also emits the bias gradient of the 64->64 head conv (sum of dz_g) while it has it in registers
            if self._ws_bias is None:
                self._ws_bias = torch.empty(2048 * 64, device=self.device, dtype=torch.float32)
            mk = {} if m_g is None else {"mask": m_g}          # (bf16 mode: the head activation's sign mask instead of its rows)
            dz_g = self.ops.conv_cout1_dgrad_folded(dpred, L2.w, tuple(g.shape[:4]), g, ACT_RELU, lddz=3, dz_coff=hidx,
                                               dbias_prev=L1.gb if wg[li] else None, workspace=self._ws_bias, **mk)
            del m_g, mk
            del g
            if wg[li]:
                self._wgrad(rb.t, dz_g, L1, bias=False)
            if not to_trunk:
                del dz_g
                li += 2
                continue
            if multi:
                dz_gs.append(dz_g)
                del dz_g
                li += 2
                continue
            pad = self._pad_like(rb.t)
            y_m, a_m = act_of(rb) if hidx == 2 else (None, ACT_NONE)
            self._dgrad_fused(dz_g, L1, pad, dz, dz if hidx > 0 else None, y_m, a_m, rb.mask)
            pads.append(pad)
            del dz_g
            li += 2
        if to_trunk:
            y_m, a_m = act_of(rb)
            if multi:
                pad = self._pad_like(rb.t)
                use_mask = y_m is not None and rb.mask is not None
                self.ops.conv3d_dgrad_fused_multi(dz_gs, [Ls[li - 6 + 2 * h].wp_d for h in range(3)], pad, dz, y_prev=None if use_mask else y_m, act=a_m,
                                                  mask=rb.mask if use_mask else None, algo=self.conv_algo[Ls[li - 6].name])
                pads.append(pad)
                del dz_gs
            self.ops.fold_halo_border(pads, dz, None, y_m, a_m)
            del pads, pad
        li = len(Ls) - 6
        nb = self.low_resblock + self.hi_resblock
        up = c["up"]
        need_at = plan["need_at"]
        for i in range(nb, -1, -1):
            if i == self.low_resblock or (done == 1 and i == self.low_resblock // 2 and len(self.grad_buckets) == 3):
                bucket_done(done)
                done += 1
            if not need_at[i]:                 # nothing at or below trunk tensor i trains: the chain ends here
                dz = None
                break
            if up is not None and i == self.low_resblock:
                # dz currently holds d(up_out) (linear producer): pull it through the upsample
                y_m, a_m = act_of(up[0])
                dz = self.ops.upsample_trilinear_bwd(dz, R, y_m, a_m)
            if i == 0:
                break
            x, h, out = c["blocks"][i - 1]
            m_h = c["hmasks"][i - 1]
            c["blocks"][i - 1] = c["hmasks"][i - 1] = None
            li -= 2
            La, Lb = Ls[li], Ls[li + 1]
            if wg[li + 1]:
                self._wgrad(h, dz, Lb)
            if not dg[li + 1]:                 # only the block's second conv trains
                dz = None
                break
            dz_h = self._dgrad_fold(dz, Lb, None, h, ACT_LEAKY, mask=m_h)
            del m_h
            if wg[li]:
                self._wgrad(x.t, dz_h, La)
            if not dg[li]:
                dz = None
                break
            y_m, a_m = act_of(x)
            dz = self._dgrad_fold(dz_h, La, dz, y_m, a_m, mask=x.mask)
            del dz_h
        if dz is not None:
            assert li == 6
            # dz == dz_c1
            if wg[5]:
                self._wgrad(c["c0"], dz, Ls[5])
            if dg[5]:
                dz_c0 = self._dgrad_fold(dz, Ls[5], None, c["c0"], ACT_RELU)
                if wg[4]:
                    self._wgrad(c["p1"], dz_c0, Ls[4], x2=c["a1"])
                if dg[4]:
                    dz_p1, dz_a1 = self.ops.conv1x1_dgrad(dz_c0, Ls[4].w, c["p1"], c["a1"])
                    for (i1, src, dzz, go) in ((2, "p", dz_p1, plan["branch_phase"]), (0, "a", dz_a1, plan["branch_pc"])):
                        if not go:                  # the whole branch is frozen
                            continue
                        first, second = Ls[i1], Ls[i1 + 1]
                        x0 = c[src + "0"]
                        if wg[i1 + 1]:
                            self._wgrad(x0, dzz, second)
                        if dg[i1 + 1]:
                            dz0 = self._dgrad_fold(dzz, second, None, x0, ACT_RELU)
                            self._wgrad(c["phase"] if src == "p" else c["pc"], dz0, first)
        self._flush_wgrads()
        self._join_side()                                            # all weight gradients have landed in flat_g
        while done < len(self.grad_buckets):
            bucket_done(done)
            done += 1
        return self.flat_g


class SR4DFlowNet:
    """Same constructor / build_network signature as the reference (SR4DFlowNet.py:4-7).  The six leading
    arguments are placeholders there (Keras Inputs); here they are accepted and only used to sanity-check
    the patch shape.  channel_nr is forced to 64 exactly like SR4DFlowNet.py:8."""

    def __init__(self, res_increase):
        self.res_increase = res_increase

    def build_network(self, u, v, w, u_mag, v_mag, w_mag, low_resblock=8, hi_resblock=4, channel_nr=64, device=None,
                      seed=0, dtype="float32", conv_algo=None, output_activation=None):
        """output_activation: None / 'linear' (SR4DFlowNet.py:40,43,46 as shipped) or 'tanh' (the first published weights)."""
        channel_nr = 64   # noqa: F841  (the reference overwrites the argument)
        output_activation_code(output_activation)         # (refused before anything needs a GPU)
        for t in (u, v, w, u_mag, v_mag, w_mag):
            shp = getattr(t, "shape", None)
            if shp is not None and len(shp) == 5 and shp[-1] != 1:
                raise ValueError("inputs must have a single channel, got shape %s" % (tuple(shp),))
        return FlowNetModel(self.res_increase, low_resblock, hi_resblock, device=device, seed=seed, dtype=dtype, conv_algo=conv_algo,
                            output_activation=output_activation)

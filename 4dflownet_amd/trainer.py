"""Host-side mirror of src/Network/TrainerController.py: same constructor, same methods
(init_model_dir, restore_model, train_network, train_step, test_step, save_best_model, quicksave), same loss.csv
columns; the arithmetic runs in lib4dflow_hip.so.

Differences that are deliberate and documented in DESIGN.md:
  * the TensorBoard epoch scalars (:181-182, :396-412) are written by tfevents.SummaryWriter -- same directories, tags,
    steps and TF2 scalar encoding, no TensorFlow dependency;
  * metrics accumulate on the device and are only synchronised when .result() is read, so a training loop that
    does not print every step never stalls the GPU (the reference forces a sync per step, :290);
  * with torch.distributed initialised, train_step sum-all-reduces the flat gradient over RCCL before Adam;
  * accum_steps = K > 1 (no counterpart in the reference): K train_step calls form ONE optimiser step on the sum of their gradients;
  * fine-tuning: `trainable=` / model.set_trainable / `layer.trainable = False` freeze layers as in Keras (:223-225 differentiate and
    update model.trainable_variables only); backward skips what a frozen layer does not need and Adam leaves its parameters and slots;
  * gradient clipping: `global_clipnorm=` / `clipvalue=` are the arguments of the same name of tf.keras.optimizers.Adam (:73), applied on
    the device to the gradient Adam is about to consume, the L2 term included;
  * weight EMA: `use_ema=` / `ema_momentum=` / `ema_overwrite_frequency=` are the arguments of the same name of
    tf.keras.optimizers.Adam (:73); the average is formed inside the Adam launch, `ema_weights()` evaluates under it."""
import contextlib
import ctypes
import datetime
import os
import pickle
import shutil
import time

import numpy as np
import torch

from . import ops, parallel, tfevents
from .network import Input, SR4DFlowNet

L2_LAMBDA = 5e-7                      # SR4DFlowNet.py:99
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-7   # tf.keras.optimizers.Adam defaults (TrainerController.py:73)


def _clip_arguments(global_clipnorm, clipvalue):
    """The two clipping arguments of tf.keras.optimizers.Adam as (float or None, float or None): each None or a number that is finite
    and > 0 as the float32 the device receives, and at most one of them set.  (Keras' per-variable `clipnorm` needs one norm per
    variable and is not offered.)"""
    out = []
    for name, c in (("global_clipnorm", global_clipnorm), ("clipvalue", clipvalue)):
        if c is None:
            out.append(None)
            continue
        try:
            cf = ctypes.c_float(float(c)).value
        except (TypeError, ValueError):
            raise ValueError("%s must be None or a finite number > 0, got %r" % (name, c)) from None
        if isinstance(c, (bool, str, bytes)) or not np.isfinite(cf) or cf <= 0:
            raise ValueError("%s must be None or a finite number > 0, got %r" % (name, c))
        out.append(cf)
    if out[0] is not None and out[1] is not None:
        raise ValueError("global_clipnorm and clipvalue are both set (%r, %r): at most one kind of gradient clipping" % (global_clipnorm, clipvalue))
    return tuple(out)


def _ema_arguments(use_ema, ema_momentum, ema_overwrite_frequency, ema_validation=False):
    """The weight-EMA arguments as (bool, float, int or None, bool): use_ema and ema_validation are bools, ema_momentum is a finite real
    in [0, 1) as the float32 the device receives (0.999999999 rounds to 1.0f and is refused), ema_overwrite_frequency is None or an
    integer >= 1 (tf.keras.optimizers.Adam(use_ema=, ema_momentum=, ema_overwrite_frequency=)); ema_validation needs use_ema."""
    for name, b in (("use_ema", use_ema), ("ema_validation", ema_validation)):
        if not isinstance(b, (bool, np.bool_)):
            raise ValueError("%s must be True or False, got %r" % (name, b))
    mom = ema_momentum
    try:
        mom32 = ctypes.c_float(float(mom)).value
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ema_momentum must be a real number in [0, 1) as float32, got %r" % (mom,)) from None
    if isinstance(mom, (bool, np.bool_, str, bytes)) or not 0.0 <= mom32 < 1.0:                      # (false for NaN)
        raise ValueError("ema_momentum must be a real number in [0, 1) as float32, got %r" % (mom,))
    k = ema_overwrite_frequency
    if k is not None and (isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1):
        raise ValueError("ema_overwrite_frequency must be None or an integer >= 1, got %r" % (k,))
    if ema_validation and not use_ema:
        raise ValueError("ema_validation=True validates under the averaged weights and needs use_ema=True")
    return bool(use_ema), mom32, None if k is None else int(k), bool(ema_validation)


class Mean:
    """tf.keras.metrics.Mean: running mean over every element ever passed to update_state."""

    def __init__(self, name, device):
        self.name = name
        self.device = device
        self.reset_states()

    def reset_states(self):
        # zeroed in place: the tensor result() reads stays the same object over epochs (a step recorded into a HIP graph accumulates into it)
        if getattr(self, "_total", None) is None:
            self._total = torch.zeros((), device=self.device, dtype=torch.float64)
        else:
            self._total.zero_()
        self._count = 0

    def update_state(self, values):
        if isinstance(values, torch.Tensor):
            self._total += values.sum().to(torch.float64)
            self._count += values.numel()
        else:
            self._total += float(values)
            self._count += 1

    def result(self):
        return float(self._total.item()) / self._count if self._count else 0.0

    def result_global(self):
        """Mean over every rank's elements (collective: every rank must call it).  Single process == result()."""
        total, count = parallel.allreduce_sum_host([float(self._total.item()), float(self._count)])
        return total / count if count else 0.0


class _Optimizer:
    """Keras-Adam state on one flat buffer.  `weights` mirrors optimizer.weights = [iterations, m..., v...]."""

    def __init__(self, model, lr):
        self.lr = float(lr)
        self.iterations = 0
        self.m = torch.zeros_like(model.flat_w)
        self.v = torch.zeros_like(model.flat_w)

    def lr_t(self):
        t = self.iterations
        return self.lr * np.sqrt(1.0 - ADAM_B2 ** t) / (1.0 - ADAM_B1 ** t)


class TrainerController:
    loss, loss_param = 'mse', None     # the data term's penalty: instance attributes, read on every step (see __init__)

    def __init__(self, patch_size, res_increase, initial_learning_rate=1e-4, quicksave_enable=True,
                 network_name='4DFlowNet', low_resblock=8, hi_resblock=4, device=None, seed=0, dtype='float32',
                 bucketed_allreduce=None, conv_algo=None, div_weight=0, accum_steps=1, trainable=None, global_clipnorm=None,
                 clipvalue=None, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None, ema_validation=False,
                 output_activation=None, non_fluid_weight=1, loss='mse', loss_param=None):
        """Reference arguments: TrainerController.py:18.  Extra (keyword-only in spirit): device, seed (Glorot draw), dtype
        (activation storage, 'float32' | 'bfloat16'), bucketed_allreduce (data parallel only: True = one asynchronous SUM
        all-reduce per gradient bucket started inside backward -- the default --, False = ONE all-reduce of the whole buffer
        after backward; env FDN_DP_BUCKETED=0 selects the latter when the argument is None), conv_algo ('auto' | 'direct' |
        {layer name: ...}: algorithm of the 64->64 layers, see FlowNetModel), div_weight (weight of the divergence loss,
        TrainerController.py:23,84-127 with :111-120 live; 0 = the reference's shipped loss.  The attribute of the same name is
        read on every step, so setting it later works too), accum_steps (gradient accumulation: K >= 1 consecutive train_step
        calls -- micro-batches -- form ONE optimiser step on the sum of their gradient buffers, batch-size slot included, which is the
        reference's step on the concatenated batch: tape.gradient of the (B,) loss vector is the gradient of sum_b loss_b and no layer
        couples samples, TrainerController.py:223,245-249.  1 = every call is an optimiser step, nothing is allocated or launched for
        accumulation.  The attribute of the same name is read when a group starts: a change made mid-group applies from the next
        group.  See train_step and apply_accumulated), trainable (fine-tuning: None or "all" = every layer, "hires" = the hi-res ResBlocks
        and the heads, "heads" = the six head layers, or an iterable of layer names -- FlowNetModel.set_trainable; the same as setting
        `layer.trainable` on self.model.layers as one does in Keras.  Frozen layers get no gradient, no update and no optimiser slots in
        optimizer.pkl; optimizer.iterations and the bias correction stay global; l2_reg_loss still covers every kernel),
        global_clipnorm / clipvalue (gradient clipping, the arguments of tf.keras.optimizers.Adam at TrainerController.py:73; at most one,
        finite and > 0, None = off.  The clipped gradient is the one tape.gradient returns at :223, i.e. flat_g + B 2 lambda w on the
        trainable kernels -- after accumulation and after the all-reduce, once per optimiser step, on the device.  global_clipnorm = c
        scales it by c / max(N, c), N its L2 norm over all trainable variables (tf.clip_by_global_norm); clipvalue = c clamps every
        element to [-c, c].  With global_clipnorm set, last_grad_norm is a view of N on the device and grad_norm_metric its running
        mean, written as '<name>/grad_norm'; a very large finite value logs the norm without ever clipping.  Keras' per-variable
        `clipnorm` is not offered.  The attributes of the same names are read on every optimiser step),
        use_ema / ema_momentum / ema_overwrite_frequency (weight EMA, the arguments of tf.keras.optimizers.Adam at
        TrainerController.py:73 [TF]: with use_ema every optimiser step also moves self.ema, a flat fp32 buffer like optimizer.m,
        a_t = ema_momentum * a_{t-1} + (1 - ema_momentum) * w_t in fp32 inside the Adam launch, a_0 = the weights before the first such
        step; the average of a frozen parameter is its weight.  The buffer is allocated by the first optimiser step that runs with
        use_ema; the average restarts from the weights whenever they were changed outside the optimiser (load_weights, set_weights).
        ema_overwrite_frequency = k: after every optimiser step with iterations % k == 0 the weights are overwritten with the average.
        finalize_ema() does so on demand, `with ema_weights():` evaluates under the average and restores the weights.  The
        attributes of the same names are read on every optimiser step), ema_validation (True: train_network runs the validation
        loop, the best-model decision and quicksave under the averaged weights), output_activation (None / 'linear' = the reference's v2
        network, 'tanh' = the bounded heads its first published weights were trained with; see FlowNetModel), non_fluid_weight
        ("Weighting for non fluid region", TrainerController.py:24: a finite number >= 0 on the non-fluid part of the MSE and of the
        divergence term; 1 = the reference's shipped loss, 0 = a fluid-only loss.  Like div_weight the attribute is read on every
        step), loss / loss_param (the penalty of the data term, per component of pred - truth: 'mse' = the reference's calculate_mse,
        'mae' |d|, 'huber' with loss_param = delta (None = 1.0, tf.keras.losses.Huber's default; on velocities normalised to [-1, 1]
        that is MSE / 2 almost everywhere, so choose a smaller delta), 'charbonnier' sqrt(d^2 + eps^2) with loss_param = eps (None =
        1e-3); 'mse' and 'mae' take no parameter.  The divergence term stays squared and the relative-error metric does not depend on
        the choice.  The names of loss_metrics and the columns of loss.csv stay the reference's: train_mse / val_mse hold the data term
        under the chosen penalty, and val_loss, the model-selection metric, is in the chosen loss's units, so values of runs with
        different losses do not compare.  Whether any of them improves accuracy over 'mse' is unmeasured.  Both attributes are read on
        every step: train_step, test_step and quicksave follow a later assignment)."""
        self.use_ema = use_ema
        self.ema_momentum = ema_momentum
        self.ema_overwrite_frequency = ema_overwrite_frequency
        self.ema_validation = ema_validation
        self._checked_ema()
        self.ema = None                # the average, (n_params,) like optimizer.m: allocated by the first optimiser step that runs with use_ema
        self._ema_version = -1         # model.weights_version the average belongs to (another one: the next step starts it afresh)
        self._ema_spare = None         # ema_weights(): where the weights wait
        self._ema_active = False       # inside ema_weights()
        self.global_clipnorm = global_clipnorm
        self.clipvalue = clipvalue
        self._checked_clip()
        self._clip_partials = None     # fdn_grad_sumsq_partials' per-block sums and fdn_clip_scale's (norm, scale): allocated by the first
        self._clip_out = None          # optimiser step that runs with global_clipnorm set
        self.last_grad_norm = None     # 0-d view of the norm the last clipped step saw (device; reading it synchronises)
        self.div_weight = div_weight   # TrainerController.py:23
        self._checked_div_weight()
        self.accum_steps = accum_steps
        self._checked_accum_steps()
        self.accum_g_ext = None        # the accumulator, (n_params + 1,) like model.flat_g_ext: allocated by the first micro-step of a group of K > 1
        self._accum_k = 1              # accum_steps as read when the running group started
        self._accum_count = 0          # micro-steps of the running group so far (0: no group is open)
        self._accum_has = False        # the accumulator holds a contribution of the running group (an empty shard contributes nothing)
        self.non_fluid_weight = non_fluid_weight   # TrainerController.py:24
        self._checked_non_fluid_weight()
        self.loss = loss
        self.loss_param = loss_param
        self._checked_loss()
        self.res_increase = res_increase
        self.patch_size = patch_size
        self.QUICKSAVE_ENABLED = quicksave_enable
        self.network_name = network_name

        input_shape = (patch_size, patch_size, patch_size, 1)
        u, v, w = Input(input_shape, 'u'), Input(input_shape, 'v'), Input(input_shape, 'w')
        u_mag, v_mag, w_mag = Input(input_shape, 'u_mag'), Input(input_shape, 'v_mag'), Input(input_shape, 'w_mag')
        net = SR4DFlowNet(res_increase)
        self.model = net.build_network(u, v, w, u_mag, v_mag, w_mag, low_resblock, hi_resblock, device=device, seed=seed,
                                       dtype=dtype, conv_algo=conv_algo, output_activation=output_activation)
        self.device = self.model.device
        if trainable is not None:
            self.model.set_trainable(trainable)

        names = ['train_loss', 'val_loss', 'train_accuracy', 'val_accuracy', 'train_mse', 'val_mse', 'train_div',
                 'val_div', 'l2_reg_loss']
        self.loss_metrics = dict((n, Mean(n, self.device)) for n in names)
        self.accuracy_metric = 'val_loss'
        self.learning_rate = initial_learning_rate
        self.grad_norm_metric = Mean('grad_norm', self.device)     # outside loss_metrics: the columns of loss.csv stay the reference's
        self.optimizer = _Optimizer(self.model, initial_learning_rate)
        self._l2_buf = torch.zeros(1, device=self.device)
        self._l2_partials = torch.zeros(ops.ADAM_PARTIALS, device=self.device)   # sum(w^2) blocks left by the last Adam step
        self._l2_version = -1          # model.weights_version those partials belong to
        self.unique_model_name = network_name
        self.model_dir = None
        if bucketed_allreduce is None:
            bucketed_allreduce = os.environ.get("FDN_DP_BUCKETED", "1") not in ("0", "false", "no")
        self.bucketed_allreduce = bool(bucketed_allreduce)
        # bench / diagnosis: with profile_allreduce set, every train_step appends a pair of HIP events that bracket the point where
        # the compute stream waits for the gradient all-reduce(s): their distance is the EXPOSED collective time of that step
        self.profile_allreduce = False
        self.allreduce_wait_events = []

    # ------------------------------------------------------------------ steps
    def _unpack(self, data_pairs):
        arrs = [self.model._to_dev(a) for a in data_pairs]
        u, v, w, u_mag, v_mag, w_mag, u_hr, v_hr, w_hr, venc, mask = arrs
        return (u, v, w, u_mag, v_mag, w_mag), (u_hr, v_hr, w_hr), venc, mask

    def calculate_regularizer_loss(self):
        """5e-7 * sum(kernel^2) as a 0-d device tensor (TrainerController.py:129-141)."""
        if self._l2_version != self.model.weights_version:         # first step, or weights were loaded / re-initialised: stream them once
            ops.l2_sumsq_partials(self.model.flat_w, self.model.is_kernel, self._l2_partials)
            self._l2_version = self.model.weights_version
        ops.sum_partials(self._l2_partials, self._l2_buf)          # (else the Adam kernel left the per-block sums behind)
        return self._l2_buf[0] * L2_LAMBDA

    def _checked_div_weight(self):
        w = self.div_weight
        try:
            wf = float(w)
        except (TypeError, ValueError):
            raise ValueError("div_weight must be a finite number >= 0, got %r" % (w,)) from None
        if not np.isfinite(wf) or wf < 0:
            raise ValueError("div_weight must be a finite number >= 0, got %r" % (w,))
        return wf

    def _checked_non_fluid_weight(self):
        w = self.non_fluid_weight
        try:
            wf = float(w)
        except (TypeError, ValueError):
            raise ValueError("non_fluid_weight must be a finite number >= 0, got %r" % (w,)) from None
        if not np.isfinite(wf) or wf < 0:
            raise ValueError("non_fluid_weight must be a finite number >= 0, got %r" % (w,))
        return wf

    def _checked_loss(self):
        """(name, parameter or None) of the data term's penalty as the attributes stand, validated: ops.checked_loss_kind."""
        kind, _, param = ops.checked_loss_kind(self.loss, self.loss_param, who="TrainerController: loss / loss_param", error=ValueError)
        return kind, (param if kind in ops.LOSS_PARAM_DEFAULTS else None)

    def _checked_accum_steps(self):
        k = self.accum_steps
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("accum_steps must be an integer >= 1, got %r" % (k,))
        return int(k)

    def _checked_clip(self):
        """(global_clipnorm, clipvalue) as floats or None, validated: see _clip_arguments."""
        return _clip_arguments(self.global_clipnorm, self.clipvalue)

    def _checked_ema(self):
        """(use_ema, ema_momentum as float32, ema_overwrite_frequency, ema_validation), validated: see _ema_arguments."""
        return _ema_arguments(self.use_ema, self.ema_momentum, self.ema_overwrite_frequency, self.ema_validation)

    def _loss_call(self, hires, predictions, mask, want_grad):
        """The loss pass of every step and of quicksave: div_weight, non_fluid_weight and loss / loss_param as the attributes stand now,
        the activation the model's heads ended in -- so dpred is the gradient w.r.t. their pre-activations, what model.backward takes.
        At the defaults (1, linear, 'mse') ops.loss_metrics is called as it always was and makes the calls it always made.  Returns
        (out, dpred, div_weight)."""
        div_weight = self._checked_div_weight()
        kind, param = self._checked_loss()
        more = {} if kind == 'mse' else {'kind': kind, 'kind_param': param}
        out, dpred = ops.loss_metrics(predictions, hires[0], hires[1], hires[2], mask, want_grad=want_grad, div_weight=div_weight,
                                      non_fluid_weight=self._checked_non_fluid_weight(), out_act=self.model.out_act, **more)
        return out, dpred, div_weight

    def calculate_and_update_metrics(self, hires, predictions, mask, metric_set, want_grad):
        """TrainerController.py:84-127 (loss_function, the divergence term live when div_weight != 0), :243-256 (metrics)."""
        out, dpred, div_weight = self._loss_call(hires, predictions, mask, want_grad)
        mse, rel_error = out[:, 0], out[:, 1]
        div = out[:, 4] if div_weight != 0 else None
        loss = mse if div is None else mse + div
        if metric_set == 'train':
            l2 = self.calculate_regularizer_loss()
            self.loss_metrics['l2_reg_loss'].update_state(l2.reshape(1))
            loss = loss + l2
        self.loss_metrics['%s_loss' % metric_set].update_state(loss)
        self.loss_metrics['%s_mse' % metric_set].update_state(mse)
        self.loss_metrics['%s_div' % metric_set].update_state(0.0 if div is None else div)
        self.loss_metrics['%s_accuracy' % metric_set].update_state(rel_error)
        return loss, dpred

    def train_step(self, data_pairs):
        """TrainerController.py:209-225: forward, loss (+L2), gradient of sum_b loss_b, Adam.

        With accum_steps = K > 1 every call handles one micro-batch: forward, loss, metrics and backward as always (the weights do not
        move inside a group, so the L2 term and the per-sample losses are those of the big batch), and model.flat_g_ext is left holding
        this micro-batch's own local gradient and batch size.  Calls 1 .. K-1 add it into self.accum_g_ext (fdn_grad_accumulate) and
        stop there: no collective, no Adam launch, optimizer.iterations / flat_w / m / v / weights_version / the packs untouched.  Call K
        accumulates and closes the step (_close_step) on the ACCUMULATOR, whose trailing slot is then the group's global batch size.
        apply_accumulated() closes a group early.  K = 1 is the same body with model.flat_g_ext as the step buffer (_step_buffer) and
        nothing to accumulate: every call closes.

        The trailing slot of the gradient buffer carries this rank's batch size; after the SUM all-reduce the step buffer's slot holds
        the global batch size, which the Adam kernel reads on the device -- no host synchronisation per step.

        Data parallel with bucketed_allreduce, on the closing call: one SUM all-reduce per bucket of the step buffer, started inside
        backward()'s grad_ready callback as soon as the bucket's last launch has been enqueued (RCCL works on its own stream: the hi-res
        bucket travels while the low-res layers are still computing).  Every rank issues the same buckets in the same order, also a rank
        whose shard of a ragged batch is empty.  Otherwise ONE all-reduce of the whole step buffer after backward (_close_step).

        Stream order of the accumulate (K > 1): where no per-bucket collective runs -- calls 1 .. K-1, and a closing call that is not
        both data parallel and bucketed -- ONE launch over the whole buffer on the main stream after backward() has returned, i.e. behind
        its join of the weight-gradient stream.  Else the accumulate of bucket [lo, hi) is issued inside the grad_ready callback, on the
        stream that callback runs on (the weight-gradient stream once it has been made to wait for the main one, see
        FlowNetModel.backward): behind every writer of the bucket and behind the earlier micro-steps' accumulates, ahead of the bucket's
        all-reduce, which is started from the same stream right after it; _close_step then joins that stream before Adam."""
        if not self.model.any_trainable:                            # Keras: "No gradients provided for any variable"
            raise ValueError("train_step: no layer of the model is trainable (layer.trainable / set_trainable), there is nothing to update")
        self._checked_clip()                                        # (a bad clipping argument stops the step before anything is launched)
        self._checked_ema()
        if self._ema_active:
            raise RuntimeError("train_step inside `with ema_weights():` -- the model holds the averaged weights, leave the context first")
        if self._accum_count == 0:                                  # a group starts: this is where accum_steps is read
            self._accum_k = self._checked_accum_steps()
        inputs, hires, venc, mask = self._unpack(data_pairs)
        B = inputs[0].shape[0]
        m = self.model
        m.batch_slot.fill_(float(B))
        buf = self._step_buffer()
        closing = self._accum_count + 1 >= self._accum_k            # (K = 1: always)
        first = not self._accum_has
        contribute = None                                           # (K = 1: the gradient already is where the step reads it)
        if self._accum_k > 1:
            def contribute(lo, hi):
                ops.grad_accumulate(buf[lo:hi], m.flat_g_ext[lo:hi], first)
        pending = on_bucket = None
        if closing and self.bucketed_allreduce and parallel.world_size() > 1:
            pending = []

            def on_bucket(lo, hi):
                if contribute is not None and B > 0:
                    contribute(lo, hi)
                pending.append(parallel.allreduce_sum_start(buf[lo:hi]))
        if B > 0:
            pred = m.forward(inputs, training=True)
            loss, dpred = self.calculate_and_update_metrics(hires, pred, mask, 'train', True)
            m.backward(dpred, grad_ready=on_bucket)
            if contribute is not None:
                if on_bucket is None:
                    contribute(0, buf.numel())
                self._accum_has = True
        else:                                   # ragged tail on this rank: a zero gradient, which contributes nothing to an accumulator;
            m.flat_g.zero_()                    # the rank still joins the step's collectives
            loss = None
            if on_bucket is not None:
                if contribute is not None and first:        # every micro-batch of this rank's group was empty: it reduces zeros
                    buf.zero_()
                    self._accum_has = True
                for lo, hi in m.grad_buckets:
                    on_bucket(lo, hi)
        if contribute is not None:
            self._accum_count += 1
        if closing:
            self._close_step(pending)
        return loss

    def _step_buffer(self):
        """What the running step's collectives reduce and its Adam launch reads, (n_params + 1,): model.flat_g_ext when every call is a
        step, else the accumulator (allocated by the first micro-step of the first group; never memset: the first contribution of a
        group is a copy)."""
        if self._accum_k == 1:
            return self.model.flat_g_ext
        if self.accum_g_ext is None:
            self.accum_g_ext = torch.empty_like(self.model.flat_g_ext)
        return self.accum_g_ext

    def _close_step(self, pending=None):
        """The end of an optimiser step: reduce the step buffer over the ranks (pending: the per-bucket collectives the closing call
        has already started; None: one all-reduce of the whole buffer here), wait, and run ONE Adam step on it, one iteration."""
        m, buf = self.model, self._step_buffer()
        grouped = self._accum_k > 1
        dp = parallel.world_size() > 1
        if pending is None:
            pending = []
            if grouped and not self._accum_has:
                buf.zero_()
            if dp:
                pending.append(parallel.allreduce_sum_start(buf))
        self._wait_allreduce(pending, dp)
        if grouped:                             # the accumulates the grad_ready callbacks put on the weight-gradient stream: ahead of Adam
            m._join_side()                      # whatever the transport (K = 1 puts only collectives there, and those were just waited for)
        self.optimizer.iterations += 1
        n = m.n_params
        overwritten = self._adam(buf[:n], buf[n:n + 1])
        self._l2_version = -1 if overwritten else m.weights_version      # (the partials Adam left are those of the weights it wrote)
        self._accum_count = 0
        self._accum_has = False

    def _adam(self, g, batch_slot):
        """One Adam launch on the flat buffers and the re-pack of what moved; the L2 regulariser's gradient is formed inside it: the (B,)
        loss vector carries the scalar L2 term B times (:249) -> B_global * 2 lambda w, B_global read from batch_slot.
        With frozen layers: the masked path of the same kernel (their parameters and slots keep their bits, the L2 gradient reaches
        trainable kernels only, the sum of squares it leaves still covers all kernels) and a re-pack of the trainable 64->64 layers only.
        global_clipnorm: two launches ahead of Adam's -- per-block sums of squares of g + B 2 lambda w over the trainable elements, then
        norm and scale by one block -- and Adam reads the scale from the device: no host synchronisation, and every rank of a
        data-parallel run computes the same bits from the same all-reduced buffer.  clipvalue: Adam's launch alone.
        use_ema: the same single launch through the entry point that also moves self.ema (w, m, v and the partials keep their bits);
        ema_init whenever the average does not belong to the weights the step starts from.  With ema_overwrite_frequency = k and
        iterations % k == 0 the weights then become a bit copy of the average, ahead of the step's one re-pack; returns True in that
        case: the partials the launch left are no longer those of the weights."""
        m, opt = self.model, self.optimizer
        use_ema, ema_momentum, ema_every, _ = self._checked_ema()
        frozen = m.frozen_map
        clipnorm, clipvalue = self._checked_clip()
        kw = {} if frozen is None else {"frozen": frozen}
        if clipnorm is not None:
            if self._clip_out is None:
                self._clip_partials = torch.zeros(ops.ADAM_PARTIALS, device=self.device)
                self._clip_out = torch.zeros(2, device=self.device)
                self.last_grad_norm = self._clip_out[0]
            ops.grad_sumsq_partials(g, m.flat_w, m.is_kernel, 2.0 * L2_LAMBDA, batch_slot, self._clip_partials, frozen=frozen)
            ops.clip_scale(self._clip_partials, clipnorm, self._clip_out)
            self.grad_norm_metric.update_state(self._clip_out[0:1])
            kw["g_scale_dev"] = self._clip_out[1:2]
        elif clipvalue is not None:
            kw["clip_value"] = clipvalue
        if use_ema:
            if self.ema is None:
                self.ema = torch.empty_like(m.flat_w)
            kw.update(ema=self.ema, ema_momentum=ema_momentum, ema_init=self._ema_version != m.weights_version)
        ops.adam_step(m.flat_w, g, opt.m, opt.v, m.is_kernel, opt.lr_t(), ADAM_B1, ADAM_B2, ADAM_EPS,
                      2.0 * L2_LAMBDA, batch_slot, sumsq_partials=self._l2_partials, **kw)
        overwrite = use_ema and ema_every is not None and opt.iterations % ema_every == 0
        if overwrite:
            ops.grad_accumulate(m.flat_w, self.ema, first=True)     # (a frozen parameter's average is its weight: only trainable layers move)
        m.weights_changed(trainable_only=frozen is not None)
        if use_ema:
            self._ema_version = m.weights_version
        return overwrite

    # ------------------------------------------------------------------ weight EMA
    @property
    def ema_current(self):
        """An average exists and belongs to the weights the model holds (not before the first optimiser step with use_ema, and not after
        the weights were changed outside the optimiser)."""
        return self.ema is not None and self._ema_version == self.model.weights_version

    def _require_ema(self, who):
        if self._ema_active:
            raise RuntimeError("%s inside `with ema_weights():` -- the model already holds the averaged weights" % who)
        if not self.ema_current:
            raise RuntimeError("%s: there is no weight average yet (use_ema=True and one optimiser step create it; loading weights "
                               "restarts it)" % who)

    def finalize_ema(self):
        """Overwrite the weights with their average (Keras: optimizer.finalize_variable_values): a bit copy and one re-pack.  The
        average stays and now equals the weights.  Not called by train_network."""
        self._require_ema("finalize_ema")
        m = self.model
        ops.grad_accumulate(m.flat_w, self.ema, first=True)
        m.weights_changed()                                         # (the L2 partials Adam left are stale now: another weights_version)
        self._ema_version = m.weights_version

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside, the model holds the averaged weights (forward, predict, save, test_step); on exit it holds the exact bits it held
        before.  Two bit copies and a re-pack each way, no torch arithmetic.  train_step, apply_accumulated and a nested entry raise
        inside; entering raises when there is no average yet."""
        self._require_ema("ema_weights")
        m = self.model
        if self._ema_spare is None:
            self._ema_spare = torch.empty_like(m.flat_w)
        l2_current = self._l2_version == m.weights_version
        ops.grad_accumulate(self._ema_spare, m.flat_w, first=True)
        ops.grad_accumulate(m.flat_w, self.ema, first=True)
        m.weights_changed()
        self._ema_active = True
        try:
            yield self
        finally:
            self._ema_active = False
            ops.grad_accumulate(m.flat_w, self._ema_spare, first=True)
            m.weights_changed()
            self._ema_version = m.weights_version                   # the same weights as on entry: the average and the L2 partials
            if l2_current:                                          # of the last Adam step still belong to them
                self._l2_version = m.weights_version

    def _wait_allreduce(self, pending, dp):
        """The current stream waits for the collectives in `pending` (no host synchronisation under nccl)."""
        if dp and self.profile_allreduce:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for h in pending:
            parallel.allreduce_wait(h)
        if dp and self.profile_allreduce:
            e1.record()
            self.allreduce_wait_events.append((e0, e1))
            del self.allreduce_wait_events[:-4096]          # a diagnostic left on outside the bench must not grow without bound

    def apply_accumulated(self):
        """Apply whatever the running group has accumulated as a shorter group: one accumulator all-reduce if data parallel (every
        rank must call it: the ranks see the same number of micro-steps), one Adam step, one iteration.  A strict no-op when nothing
        is pending (accum_steps == 1, or the last train_step closed its group): returns False and touches no state.  train_network
        calls it after the last training batch of every epoch, so no gradient crosses a validation pass, a best-model save or an
        epoch boundary."""
        if self._accum_count == 0:
            return False
        if self._ema_active:
            raise RuntimeError("apply_accumulated inside `with ema_weights():` -- the model holds the averaged weights, leave the context first")
        self._close_step()
        return True

    def test_step(self, data_pairs):
        """TrainerController.py:227-239: forward + metrics, no L2, no update."""
        inputs, hires, venc, mask = self._unpack(data_pairs)
        if inputs[0].shape[0] == 0:             # ragged tail on this rank (data parallel): nothing to evaluate
            return None
        pred = self.model.forward(inputs, training=False)
        self.calculate_and_update_metrics(hires, pred, mask, 'val', False)
        return pred

    def reset_metrics(self):
        for k in self.loss_metrics:
            self.loss_metrics[k].reset_states()
        self.grad_norm_metric.reset_states()

    # ------------------------------------------------------------------ directories / logging
    def init_model_dir(self, base_dir="../models"):
        timestamp = datetime.datetime.now().strftime("%Y%m%d-%H%M")
        self.unique_model_name = '%s_%s' % (self.network_name, timestamp)
        self.model_dir = "%s/%s" % (base_dir, self.unique_model_name)
        self.model_path = "%s/%s" % (self.model_dir, self.network_name)
        if parallel.rank() == 0:
            os.makedirs(self.model_dir, exist_ok=True)
            self._prepare_logfile_and_summary()

    def _log(self, msg):
        with open(self.logfile, 'a') as f:
            f.write(msg)

    def _prepare_logfile_and_summary(self):
        # TrainerController.py:181-182: one event file per writer under <model_dir>/tensorboard/{train,validate}
        self.train_writer = tfevents.SummaryWriter(self.model_dir + '/tensorboard/train')
        self.val_writer = tfevents.SummaryWriter(self.model_dir + '/tensorboard/validate')
        self.logfile = self.model_dir + '/loss.csv'
        self._log('Network: %s\n' % self.network_name)
        self._log('Initial learning rate: %s\n' % self.learning_rate)
        self._log('Accuracy metric: %s\n' % self.accuracy_metric)
        self._log('Divergence weight: %s\n' % self.div_weight)
        if self._checked_non_fluid_weight() != 1:
            self._log('Non fluid weight: %s\n' % self.non_fluid_weight)
        kind, param = self._checked_loss()
        if kind != 'mse':
            self._log('Loss: %s%s\n' % (kind, '' if param is None else ' (%s=%s)' % ('delta' if kind == 'huber' else 'epsilon', param)))
        if self.model.output_activation != 'linear':
            self._log('Output activation: %s\n' % self.model.output_activation)
        clipnorm, clipvalue = self._checked_clip()
        if clipnorm is not None or clipvalue is not None:
            self._log('Gradient clipping: %s\n' % ('global_clipnorm=%s' % self.global_clipnorm if clipnorm is not None else
                                                   'clipvalue=%s' % self.clipvalue))
        use_ema, ema_momentum, ema_every, ema_validation = self._checked_ema()
        if use_ema:
            self._log('Weight EMA: momentum=%s, overwrite_frequency=%s, validation=%s\n' % (self.ema_momentum, ema_every, ema_validation))
        stat_names = ','.join(self.loss_metrics.keys())
        self._log('epoch, %s, learning rate, elapsed (sec), best_model, benchmark_err, benchmark_rel_err, '
                  'benchmark_mse, benchmark_divloss\n' % stat_names)
        # source backup like TrainerController.py:196-206 (our package instead of ./Network)
        here = os.path.dirname(os.path.abspath(__file__))
        dest = os.path.join(self.model_dir, "backup_source")
        os.makedirs(dest, exist_ok=True)
        for fname in os.listdir(here):
            if fname.endswith(".py"):
                shutil.copy2(os.path.join(here, fname), os.path.join(dest, fname))

    def _update_summary_logging(self, epoch, results=None, grad_norm=None):
        """TrainerController.py:396-412: epoch-level scalars.  Train writer: '<name>/learning_rate' and every 'train_*' metric
        with the prefix stripped ('<name>/loss', '/accuracy', '/mse', '/div'); validate writer: the 'val_*' metrics likewise;
        step = the 0-based epoch.  ('l2_reg_loss' has neither prefix, so the reference does not log it -- nor do we.)
        results: metric name -> value (the rank-combined epoch means); defaults to this process's running means.
        grad_norm: the epoch mean of the gradient norm, written as '<name>/grad_norm' on the train writer when global_clipnorm is set
        (no counterpart in the reference, which does not clip); defaults to this process's running mean."""
        if results is None:
            results = dict((k, v.result()) for k, v in self.loss_metrics.items())
        self.train_writer.scalar("%s/learning_rate" % self.network_name, self.optimizer.lr, epoch)
        if self._checked_clip()[0] is not None:
            self.train_writer.scalar("%s/grad_norm" % self.network_name,
                                     self.grad_norm_metric.result() if grad_norm is None else grad_norm, epoch)
        for k in self.loss_metrics:
            if k.startswith('train_'):
                self.train_writer.scalar("%s/%s" % (self.network_name, k.replace('train_', '')), results[k], epoch)
        for k in self.loss_metrics:
            if k.startswith('val_'):
                self.val_writer.scalar("%s/%s" % (self.network_name, k.replace('val_', '')), results[k], epoch)
        self.train_writer.flush()
        self.val_writer.flush()

    # ------------------------------------------------------------------ input staging
    def device_batches(self, dataset):
        """Iterate `dataset` ONE BATCH AHEAD of the consumer: while step k computes, batch k + 1 is copied to the device on a copy stream
        of its own -- non-blocking from the host loader's pinned ring (data.PatchHandler3D(..., pinned=True): a slot stays untouched
        until two more batches were requested, which covers the copy in flight), staged by torch otherwise.  Batches that already live on
        the device (DevicePatchHandler3D) pass through untouched.  What tf.data's prefetch-to-device does for the reference
        (PatchHandler3D.py:26-35 ends in .prefetch); FDN_H2D_PREFETCH=0 yields the dataset's own batches (one blocking copy per tensor
        inside train_step)."""
        if os.environ.get("FDN_H2D_PREFETCH", "1") in ("", "0"):
            yield from dataset
            return
        copy_stream = None

        def upload(batch):
            nonlocal copy_stream
            if all(isinstance(a, torch.Tensor) and a.is_cuda for a in batch):
                return batch, None
            if copy_stream is None:
                copy_stream = torch.cuda.Stream(device=self.device)
            # destinations come from the consumer stream's pool (and go back to it): the copy stream first waits for what that stream has
            # been given so far -- a recycled block may still be read by it -- which is at most the step before the one this batch feeds
            src = [a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in batch]
            dev = [torch.empty(t.shape, device=self.device, dtype=torch.float32) for t in src]
            copy_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(copy_stream):
                for d, t in zip(dev, src):
                    d.copy_(t, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            return tuple(dev), ev

        it = iter(dataset)
        try:
            nxt = upload(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur, ev = nxt
            if ev is not None:
                ev.synchronize()                           # `cur` has left its pinned slot (a copy-stream event: no wait for compute) before
            try:                                           # the loader is asked for more -- the ring's lifetime contract, kept by construction
                nxt = upload(next(it))                     # requested before the consumer gets `cur`: the copy runs beside its step
            except StopIteration:
                nxt = None
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
            yield cur

    # ------------------------------------------------------------------ training loop
    def train_network(self, trainset, valset, n_epoch, testset=None, verbose=True):
        """TrainerController.py:263-343.  trainset/valset: iterables of 11-tuples (PatchHandler3D datasets)."""
        if self.model_dir is None:
            self.init_model_dir()
        is0 = parallel.rank() == 0
        if is0:
            print("==================== TRAINING =================")
            print('Learning rate %.7f' % self.optimizer.lr)
            print("Start training at %s - %s\n" % (time.ctime(), self.unique_model_name))
        start_time = time.time()
        previous_loss = np.inf
        total_batch_train = len(trainset) if hasattr(trainset, "__len__") else -1
        total_batch_val = len(valset) if hasattr(valset, "__len__") else -1
        for epoch in range(n_epoch):
            self.reset_metrics()
            start_loop = time.time()
            for i, data_pairs in enumerate(self.device_batches(trainset)):
                self.train_step(data_pairs)
                if verbose and is0:
                    print("\rEpoch %d Train batch %d/%d | loss: %.5f (%.1f %%) - %.1f secs" % (
                        epoch + 1, i + 1, total_batch_train, self.loss_metrics['train_loss'].result(),
                        self.loss_metrics['train_accuracy'].result(), time.time() - start_loop), end='')
            self.apply_accumulated()                       # accum_steps > 1: a ragged last group is applied before validation
            # ema_validation: the validation loop, and with it the best-model decision, sees the averaged weights
            with self._validation_weights():
                for i, data_pairs in enumerate(self.device_batches(valset)):
                    self.test_step(data_pairs)
                    if verbose and is0:
                        print("\rEpoch %d Validation batch %d/%d | loss: %.5f (%.1f %%) - %.1f secs" % (
                            epoch + 1, i + 1, total_batch_val, self.loss_metrics['val_loss'].result(),
                            self.loss_metrics['val_accuracy'].result(), time.time() - start_loop), end='')
            # data parallel: every rank saw a shard of each global batch -> combine (total, count) over ranks, so
            # loss.csv and the best-model decision do not depend on the world size
            res = dict((k, v.result_global()) for k, v in self.loss_metrics.items())
            grad_norm = self.grad_norm_metric.result_global() if self._checked_clip()[0] is not None else None
            message = "\rEpoch %d Train loss: %.5f (%.1f %%), Val loss: %.5f (%.1f %%) - %.1f secs" % (
                epoch + 1, res['train_loss'], res['train_accuracy'], res['val_loss'], res['val_accuracy'],
                time.time() - start_loop)
            loss_str = ','.join('%.5f' % res[k] for k in self.loss_metrics)
            log_line = "%d,%s,%.6f,%.1f" % (epoch + 1, loss_str, self.optimizer.lr, time.time() - start_loop)
            if is0:
                self._update_summary_logging(epoch, res, grad_norm)
            if res[self.accuracy_metric] < previous_loss:
                if is0:
                    self.save_best_model()
                previous_loss = res[self.accuracy_metric]
                message += ' **'
                log_line += ',**'
                if self.QUICKSAVE_ENABLED and testset is not None and is0:
                    with self._validation_weights():
                        ql, qa, qm, qd = self.quicksave(testset, epoch + 1)
                    message += ' Benchmark loss: %.5f (%.1f %%)' % (np.mean(ql), np.mean(qa))
                    log_line += ', %.7f, %.2f%%, %.7f, %.7f' % (np.mean(ql), np.mean(qa), np.mean(qm), np.mean(qd))
            if is0:
                print(message)
                self._log(log_line + "\n")
        if is0:
            el = time.time() - start_time
            hrs, mins = el // 3600, (el % 3600) // 60
            msg = "\nTraining %s completed! - name: %s" % (self.network_name, self.unique_model_name)
            msg += "\nTotal training time: %d hrs %d mins %d secs." % (hrs, mins, int(el - hrs * 3600 - mins * 60))
            msg += "\nFinished at %s\n==================== END TRAINING =================" % time.ctime()
            self._log(msg)
            print(msg)

    def _validation_weights(self):
        """ema_weights() when ema_validation is set and an average exists (none before the first optimiser step), else nothing."""
        if self._checked_ema()[3] and self.ema_current:
            return self.ema_weights()
        return contextlib.nullcontext()

    # ------------------------------------------------------------------ checkpoints
    def save_latest_model(self, epoch):
        """TrainerController.py:78-82 (defined but never called by the reference's loop; kept for API parity)."""
        if epoch > 0 and epoch % 10 == 0:
            self.model.save('%s-latest.h5' % self.model_path)
            print('Saving current model - %s\n' % time.ctime())

    def save_best_model(self):
        """TrainerController.py:347-363: '<dir>/<name>-best.h5' + optimizer.pkl = [iterations, m..., v...].

        ORDER of the m / v arrays: Keras writes `optimizer.get_weights()`, whose slots follow `model.trainable_variables`, i.e. the
        functional model's depth-sorted layer list -- NOT creation order: the phase convs precede the pc convs of equal depth and the
        three heads interleave (network.keras_layer_order).  The pickle is written (and read back by restore_model) in that order, so
        a restart file can travel between the reference and this implementation.  [TF]: the order is restated from Keras' published
        graph-sorting algorithm, TensorFlow is absent here; tests/test_tf_golden.py checks it against real variable names the day
        tests/golden/tf_golden.npz exists.  Several layers share a shape, so a wrong order cannot be detected from shapes alone.

        Gradient accumulation: a partial group is never checkpointed -- the accumulator is not part of the files.  train_network applies
        the pending group before it gets here; a caller of its own does the same with apply_accumulated().

        Weight EMA: when an average exists, '<dir>/<name>-best-ema.h5' holds it in the same Keras layout (the predictor loads it like
        any weights file); '-best.h5' and optimizer.pkl are what they are without it."""
        self.model.save('%s-best.h5' % self.model_path)
        if self.ema_current:
            with self.ema_weights():
                self.model.save('%s-best-ema.h5' % self.model_path)
        # slots of the TRAINABLE variables only: Keras creates slots for the variables it is given (frozen layers have none)
        where = self._trainable_slices()
        m_flat, v_flat = self.optimizer.m.cpu().numpy(), self.optimizer.v.cpu().numpy()
        m = [m_flat[o:o + k].reshape(s) for o, k, s in where]
        v = [v_flat[o:o + k].reshape(s) for o, k, s in where]
        order = self.model.keras_variable_order()
        weight_values = [np.int64(self.optimizer.iterations)] + [m[i] for i in order] + [v[i] for i in order]
        with open('%s/optimizer.pkl' % self.model_dir, 'wb') as f:
            pickle.dump(weight_values, f)
        # The pickle itself stays what Keras writes (a bare list).  A sidecar names the slots, so restore_model can map by NAME and
        # a file in another order (creation order: this repository before round 3) is re-ordered or refused instead of silently
        # mis-assigned -- conv3d / conv3d_2 etc. share shapes, so shapes cannot tell.
        names = self.model.trainable_variable_names()
        with open('%s/optimizer_order.txt' % self.model_dir, 'w') as f:
            f.write("# optimizer.pkl slot order: [iterations] + m slots + v slots, each in this variable order (Keras trainable_variables)\n")
            f.write("\n".join(names[i] for i in order) + "\n")

    def _trainable_slices(self):
        """(offset, numel, shape) in the flat buffers of every entry of model.trainable_variables (creation order)."""
        out = []
        for L in self.model.layers:
            if L.trainable:
                out.append((L.w_off, L.w.numel(), tuple(L.w.shape)))
                if L.b is not None:
                    out.append((L.b_off, L.b.numel(), tuple(L.b.shape)))
        return out

    def restore_model(self, old_model_dir, old_model_file):
        """TrainerController.py:365-394.  optimizer.pkl slots are in Keras trainable_variables order (see save_best_model).
        A checkpoint never holds a partial accumulation group: a group that is open here is dropped, the next train_step starts one.
        Weight EMA: with use_ema set and '<stem>-ema.h5' beside old_model_file (save_best_model writes it), that file becomes the
        average; otherwise the average restarts from the loaded weights at the next optimiser step."""
        if self._ema_active:
            raise RuntimeError("restore_model inside `with ema_weights():` -- leave the context first")
        with open("%s/optimizer.pkl" % old_model_dir, 'rb') as f:
            opt_weights = pickle.load(f)
        tv = self.model.trainable_variables
        n = len(tv)
        order = self.model.keras_variable_order()
        names = self.model.trainable_variable_names()
        side = "%s/optimizer_order.txt" % old_model_dir
        legacy = os.environ.get("FDN_OPTIMIZER_PKL_ORDER", "")
        listed = None
        if os.path.exists(side):                              # written by save_best_model: map the slots by variable name
            listed = [l.strip() for l in open(side) if l.strip() and not l.startswith("#")]
            if sorted(listed) != sorted(names):               # (the slots are those of the variables that were trainable when it was saved)
                diff = sorted(set(listed) ^ set(names))
                raise ValueError("optimizer_order.txt names %d variables that are not this model's trainable variables (set the same "
                                 "layers trainable as when it was saved): %s" % (len(diff), ", ".join(diff)))
        if len(opt_weights) != 1 + 2 * n:
            raise ValueError("optimizer.pkl holds %d arrays, expected %d" % (len(opt_weights), 1 + 2 * n))
        if listed is not None:
            order = [names.index(nm) for nm in listed]
        elif legacy == "creation":                            # a pickle of this repository before round 3 (no sidecar, creation order)
            order = list(range(n))
        elif legacy not in ("", "keras"):
            raise ValueError("FDN_OPTIMIZER_PKL_ORDER must be 'keras' or 'creation'")
        else:
            import warnings
            warnings.warn("optimizer.pkl without optimizer_order.txt: assuming Keras trainable_variables order (what the reference writes); "
                          "set FDN_OPTIMIZER_PKL_ORDER=creation for a file written by this repository before round 3")
        m_k, v_k = list(opt_weights[1:1 + n]), list(opt_weights[1 + n:])
        m, v = [None] * n, [None] * n
        for slot, i in enumerate(order):
            for name, src, dst in (("m", m_k, m), ("v", v_k, v)):
                if tuple(np.shape(src[slot])) != tuple(tv[i].shape):
                    raise ValueError("optimizer.pkl: %s slot %d has shape %s, expected %s (slots follow Keras trainable_variables order, "
                                     "see save_best_model)" % (name, slot, tuple(np.shape(src[slot])), tuple(tv[i].shape)))
                dst[i] = src[slot]
        self.optimizer.iterations = int(opt_weights[0])
        # (into the trainable variables' ranges of the flat slots; a frozen layer has no slots in the file and keeps what it holds)
        for dst, arrs in ((self.optimizer.m, m), (self.optimizer.v, v)):
            host = dst.cpu().numpy()
            for (o, k, _), a in zip(self._trainable_slices(), arrs):
                host[o:o + k] = np.asarray(a, np.float32).reshape(-1)
            dst.copy_(torch.from_numpy(host))
        ema_file = "%s/%s-ema.h5" % (old_model_dir, os.path.splitext(old_model_file)[0])
        have_ema = self._checked_ema()[0] and os.path.exists(ema_file)
        if have_ema:                                          # through the model's own reader: the file has the layout of a weights file
            self.model.load_weights(ema_file)
            if self.ema is None:
                self.ema = torch.empty_like(self.model.flat_w)
            ops.grad_accumulate(self.ema, self.model.flat_w, first=True)
        self.model.load_weights("%s/%s" % (old_model_dir, old_model_file))
        if have_ema:
            self._ema_version = self.model.weights_version
        self._accum_count = 0
        self._accum_has = False

    def quicksave(self, testset, epoch_nr):
        """TrainerController.py:415-454: predict the first benchmark batch, append to quicksave_<name>.h5."""
        from . import h5io
        for data_pairs in testset:
            inputs, hires, venc, mask = self._unpack(data_pairs)
            preds_t = self.model.forward(inputs)
            out, _, div_weight = self._loss_call(hires, preds_t, mask, False)
            break
        out = out.cpu().numpy()
        preds = preds_t.cpu().numpy()
        path = os.path.join(self.model_dir, "quicksave_%s.h5" % self.network_name)
        cols = []
        sv = lambda name, arr: cols.append((name, np.asarray(arr)))
        sv("epoch", np.asarray([epoch_nr]))
        pe = np.expand_dims(preds, 0)
        sv("u", pe[..., 0]); sv("v", pe[..., 1]); sv("w", pe[..., 2])
        if epoch_nr == 1:
            cpu = lambda t: t.cpu().numpy()
            sv("lr_u", cpu(inputs[0])); sv("lr_v", cpu(inputs[1])); sv("lr_w", cpu(inputs[2]))
            sv("hr_u", np.squeeze(cpu(hires[0]), -1)); sv("hr_v", np.squeeze(cpu(hires[1]), -1))
            sv("hr_w", np.squeeze(cpu(hires[2]), -1))
            sv("venc", cpu(venc)); sv("mask", cpu(mask))
        h5io.append_datasets(path, cols, compression='gzip')      # one pass over the file for all columns
        if div_weight != 0:                                       # (loss, rel-error, mse, divergence loss) per sample
            return out[:, 0] + out[:, 4], out[:, 1], out[:, 0], out[:, 4]
        return out[:, 0], out[:, 1], out[:, 0], np.zeros_like(out[:, 0])

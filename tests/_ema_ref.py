"""Float64 restatement of the weight average fdn_adam_step_ema keeps (tf.keras.optimizers.Adam(use_ema=True, ema_momentum=mom), [TF]:
TensorFlow is absent, the recurrence is the specification), and the bound the GPU tests hold the fp32 kernel to.

    a_0 = w_0 (the weights before the first step with an average);    a_t = mom32 * a_{t-1} + (1 - mom32) * w_t;
    frozen elements: a_t = w_t (= w_{t-1}: a frozen weight does not move), whatever the element's history.

mom32 is the momentum as the float32 the device receives; the w_t are the fp32 weights the device wrote, read back exactly."""
import numpy as np

U = 2.0 ** -24                                   # unit roundoff of float32


def mom32(momentum):
    return float(np.float32(momentum))


def ema_step(a, w_before, w_after, momentum, init=False, frozen=None):
    """One step, float64, out of place.  a: the average so far (ignored, and may hold anything, with init); w_before / w_after: the weights
    the step found and left; frozen: None or a mask (non-zero = frozen).  Returns the new average."""
    mom = mom32(momentum)
    w_before, w_after = np.asarray(w_before, np.float64), np.asarray(w_after, np.float64)
    prev = w_before if init else np.asarray(a, np.float64)
    new = mom * prev + (1.0 - mom) * w_after
    if frozen is not None:
        new = np.where(np.asarray(frozen) != 0, w_before, new)
    return new


def ema_chain(weights, momentum, frozen=None):
    """weights = [w_0, w_1, .., w_T]: the averages [a_1, .., a_T], the first step with init."""
    out, a = [], None
    for t in range(1, len(weights)):
        a = ema_step(a, weights[t - 1], weights[t], momentum, init=t == 1, frozen=frozen)
        out.append(a)
    return out


def ema_bound(weights, averages):
    """Per element: 4 T 2^-24 max_t(|w_t|, |a_t|), T = len(averages).  A step rounds at most three operations of its own -- the two products
    and the sum -- and inherits the rounding of 1.f - mom32, each relative to a value bounded by that maximum (|mom32| < 1, and a convex
    combination does not exceed its operands); the error carried in from a_{t-1} is multiplied by mom32 < 1.  Contraction to FMA only
    removes roundings."""
    big = np.zeros_like(np.asarray(weights[0], np.float64))
    for x in list(weights) + list(averages):
        big = np.maximum(big, np.abs(np.asarray(x, np.float64)))
    return 4.0 * len(averages) * U * big

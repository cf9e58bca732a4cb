"""Float64 restatement of "clip the gradient, then Keras Adam" -- what tf.keras.optimizers.Adam(global_clipnorm=c) / Adam(clipvalue=c)
compute for the reference's step (src/Network/TrainerController.py:73,223-225) -- on flat buffers, built on
oracle.flownet_oracle.adam_step_tf.  [TF]: restated from TensorFlow's published source (tf.clip_by_global_norm, tf.clip_by_value);
TensorFlow is absent here.

The gradient that is clipped is the one tape.gradient returns: g + l2s * w on the kernels (the L2 regulariser's part, l2s = B 2 lambda),
g on the biases, over the trainable elements only."""
import numpy as np

from oracle import flownet_oracle as O


def step_gradient(g, w, isk, l2s, live=None):
    """g' in float64; elements outside `live` (bool, None = all) are 0."""
    gp = np.asarray(g, np.float64) + float(l2s) * np.asarray(w, np.float64) * np.asarray(isk, np.float64)
    if live is not None:
        gp = np.where(live, gp, 0.0)
    return gp


def global_norm(gp):
    return float(np.sqrt(np.sum(np.square(np.asarray(gp, np.float64)))))


BLOCKS, THREADS = 2048, 256          # FDN_ADAM_PARTIALS blocks of 256 threads: the grid of fdn_grad_sumsq_partials
U = 2.0 ** -24                       # unit roundoff of fp32


def l2s_f32(l2_grad_scale, slot):
    """l2s as the kernels form it: the fp32 product of the by-value scale and the batch-size slot (slot None: the by-value scale alone)."""
    s = np.float32(l2_grad_scale)
    return float(s if slot is None else s * np.float32(slot))


def norm_roundings(n):
    """The longest chain of fp32 roundings between a term g'_i^2 and the norm the device reports, from the summation order of
    fdn_grad_sumsq_partials followed by fdn_clip_scale:
      ceil(n / (2048 * 256))  adds of one thread's chain over its trips of the grid-stride loop,
      6 + 2                   the shuffle tree of a 64-lane wave, then (red0 + red1) + (red2 + red3) over the block's four waves,
      8 + 6 + 2               the 2048 partials summed by one block of 256: 8 per thread, the same tree, the same four waves,
      4                       forming the term: the product l2s * w and the add to g round once each and squaring doubles a relative
                              error (the square itself is fused into the chain's add, and where it is not, the chain's first add,
                              0 + x, is exact and pays for it),
      1                       the sqrtf.
    |N_dev^2 - sum g'_i^2| <= norm_roundings(n) * 2^-24 * sum (|g_i| + |l2s w_i|)^2 to first order in 2^-24: every rounding moves the
    running sum by at most 2^-24 of the sum of the terms' magnitudes, and a term's magnitude is at most (|g| + |l2s w|)^2."""
    return -(-n // (BLOCKS * THREADS)) + (6 + 2) + (8 + 6 + 2) + 4 + 1


def norm_check(norm_dev, g, w, isk, l2s, live=None):
    """(|N_dev^2 - S|, bound) with S = sum g'^2 in float64 and the bound of norm_roundings; l2s is the fp32 value of l2s_f32."""
    g, w, k = np.asarray(g, np.float64), np.asarray(w, np.float64), np.asarray(isk, np.float64)
    mag = (np.abs(g) + np.abs(float(l2s) * w) * k) ** 2
    if live is not None:
        mag = np.where(live, mag, 0.0)
    S = float(np.sum(np.square(step_gradient(g, w, isk, l2s, live))))
    return abs(float(norm_dev) ** 2 - S), norm_roundings(g.size) * U * float(mag.sum())


def clip_scale(norm, c):
    """s = c / max(N, c); NaN when N is not finite (TF: the entries are all set to NaN to signify that an error occurred)."""
    if not np.isfinite(norm):
        return float("nan")
    return float(c) / max(float(norm), float(c))


def clip_scale_tf(norm, c):
    """A literal transcription of tf.clip_by_global_norm's factor: clip_norm * minimum(1 / use_norm, 1 / clip_norm)."""
    if not np.isfinite(norm):
        return float("nan")
    return float(c) * min(1.0 / float(norm), 1.0 / float(c))


def clip_by_global_norm(gp, c):
    n = global_norm(gp)
    return gp * clip_scale(n, c), n


def clip_by_value(gp, c):
    """Comparisons, so that NaN stays NaN."""
    gp = np.asarray(gp, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(gp > c, c, np.where(gp < -c, -c, gp))


def clipped_adam_step(w, g, m, v, isk, t, lr, l2s, global_clipnorm=None, clipvalue=None, live=None):
    """One step in place on float64 w, m, v (elements outside `live` untouched).  Returns the global norm of the step's gradient."""
    assert global_clipnorm is None or clipvalue is None
    gp = step_gradient(g, w, isk, l2s, live)
    norm = global_norm(gp)
    if global_clipnorm is not None:
        gp = gp * clip_scale(norm, global_clipnorm)
    if clipvalue is not None:
        gp = clip_by_value(gp, clipvalue)
    if live is None:
        O.adam_step_tf(w, gp, m, v, t, lr)
    else:
        ws, ms, vs = w[live], m[live], v[live]
        O.adam_step_tf(ws, gp[live], ms, vs, t, lr)
        w[live], m[live], v[live] = ws, ms, vs
    return norm

"""Gradient clipping on the GPU, kernel level: fdn_grad_sumsq_partials, fdn_clip_scale and fdn_adam_step_clipped.

The norm is compared against float64 at a bound derived from the summation order (tests/_clip_ref.py: norm_roundings); everything that is
the same statement on the same operands is compared bit for bit -- an inactive clip against the unclipped entry points, a device scale
against torch's multiply, clip_value against torch.clamp, a recorded chain of the three launches against eager ones; the general case
against the float64 "clip, then Keras Adam" of tests/_clip_ref.py at the bounds of test_gpu_kernels.py::test_adam_and_l2."""
import importlib

import numpy as np
import pytest
import torch

import _clip_ref as R

pytestmark = pytest.mark.gpu

ops = importlib.import_module("4dflownet_amd.ops")
SIZES = [1, 1000, 2 * 2048 * 256 + 77]         # the last: every thread of the 2048-block launch takes a third trip, some of them
PATTERNS = ["none", "all", "alternating", "ranges"]
SENTINEL = -7.25
LR_T = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
# (l2_grad_scale, batch-size slot): l2s = 0.4 -- the L2 term carries about a third of the norm, a norm of g alone misses the bound by
# orders of magnitude --, the production scale 2 * 5e-7 with a global batch of 8, and the by-value form without a slot
SCALES = {"heavy": (0.05, 8.0), "production": (2 * 5e-7, 8.0), "by_value": (0.4, None)}
_cache = {}


def _mask(n, pattern):
    f = np.zeros(n, np.uint8)
    if pattern == "all":
        f[:] = 1
    elif pattern == "alternating":
        f[::2] = 1
    elif pattern == "ranges":                    # two contiguous ranges whose ends are no multiples of 64
        for lo, hi in ((n // 7 + 3, n // 3 + 37), (n // 2 + 5, (3 * n) // 4 + 29)):
            f[lo:hi] = 1
    else:
        assert pattern == "none"
    return f


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _operands(n):
    """Shared, never modified: the tests work on clones.  Host copies ride along for the float64 references."""
    if n not in _cache:
        rng = np.random.default_rng(n)
        h = dict(w=rng.standard_normal(n).astype(np.float32), g=rng.standard_normal(n).astype(np.float32),
                 m=(0.01 * rng.standard_normal(n)).astype(np.float32), v=(1e-4 * rng.random(n)).astype(np.float32),
                 isk=(rng.random(n) < 0.9).astype(np.uint8))
        o = dict((k, _dev(a)) for k, a in h.items())
        o["host"] = h
        o["slots"] = {8.0: torch.tensor([8.0], device="cuda")}
        _cache[n] = o
    return _cache[n]


def _slot(o, slot):
    return None if slot is None else o["slots"][slot]


def _bits(t):
    return t.view(torch.int32)


def _nan_partials():
    return torch.full((ops.ADAM_PARTIALS,), float("nan"), device="cuda")


def _norm_and_scale(g, w, isk, l2gs, slot, c, frozen=None):
    part = ops.grad_sumsq_partials(g, w, isk, l2gs, slot, _nan_partials(), frozen=frozen)
    out = ops.clip_scale(part, c, torch.full((2,), float("nan"), device="cuda"))
    return part, out


# ------------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("scale", sorted(SCALES))
@pytest.mark.parametrize("n", SIZES)
def test_norm_against_float64_at_the_bound_of_the_summation_order(n, scale):
    """|N^2 - sum g'^2| <= norm_roundings(n) 2^-24 sum (|g| + |l2s w|)^2, g' = g + l2s_f32 w k in float64: the derivation is in
    tests/_clip_ref.py::norm_roundings (n = 1, 1000: 1 + 8 + 16 + 4 + 1 = 30 roundings; the large size: 32)."""
    o, (l2gs, slot) = _operands(n), SCALES[scale]
    h = o["host"]
    w0, g0 = o["w"].clone(), o["g"].clone()
    part, out = _norm_and_scale(o["g"], o["w"], o["isk"], l2gs, _slot(o, slot), 1e30)
    l2s = R.l2s_f32(l2gs, slot)
    err, bound = R.norm_check(float(out[0]), h["g"], h["w"], h["isk"], l2s)
    print("n %d %s: |N^2 - S| %.3e, bound %.3e (%d roundings), N %.9g" % (n, scale, err, bound, R.norm_roundings(n), float(out[0])))
    assert err <= bound
    if scale != "production":                                        # ... and the L2 term is in it: the norm of g alone is far outside
        err_g, _ = R.norm_check(float(out[0]), h["g"], h["w"], np.zeros(n), 0.0)
        assert err_g > 100 * bound or not (h["isk"] != 0).any()
    assert bool(torch.isfinite(part).all())
    used = -(-n // R.THREADS)
    assert not bool(part[used:].any())                               # blocks beyond the data write 0
    assert float(out[1]) == 1.0
    assert torch.equal(_bits(o["w"]), _bits(w0)) and torch.equal(_bits(o["g"]), _bits(g0))      # nothing but the partials is written
    part2, out2 = _norm_and_scale(o["g"], o["w"], o["isk"], l2gs, _slot(o, slot), 1e30)      # repeat launches: the same bits
    assert torch.equal(_bits(part), _bits(part2)) and torch.equal(_bits(out), _bits(out2))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_frozen_elements_are_left_out_of_the_norm_and_their_gradient_is_not_read(n, pattern):
    o = _operands(n)
    h = o["host"]
    l2gs, slot = SCALES["heavy"]
    fz_h = _mask(n, pattern)
    frozen = _dev(fz_h)
    fz = frozen.bool()
    g_nan = torch.where(fz, torch.full_like(o["g"], float("nan")), o["g"])
    part, out = _norm_and_scale(g_nan, o["w"], o["isk"], l2gs, _slot(o, slot), 1e30, frozen=frozen)
    # an unmasked launch on operands whose masked elements have g = 0, is_kernel = 0: the same partials bit for bit
    g_zero = torch.where(fz, torch.zeros_like(o["g"]), o["g"])
    isk_zero = torch.where(fz, torch.zeros_like(o["isk"]), o["isk"])
    part_ref, out_ref = _norm_and_scale(g_zero, o["w"], isk_zero, l2gs, _slot(o, slot), 1e30)
    assert bool(torch.isfinite(part).all())
    assert torch.equal(_bits(part), _bits(part_ref)) and torch.equal(_bits(out), _bits(out_ref))
    live = fz_h == 0
    err, bound = R.norm_check(float(out[0]), h["g"], h["w"], h["isk"], R.l2s_f32(l2gs, slot), live)
    assert err <= bound
    if pattern == "all" or not live.any():
        assert float(out[0]) == 0.0 and _bits(out)[1].item() == 0x3F800000       # nothing trainable: norm 0, scale exactly 1


# ------------------------------------------------------------------------------------------------ the scale
def test_scale_is_exactly_one_when_inactive_and_brings_the_norm_to_c_when_active():
    o = _operands(1000)
    l2gs, slot = SCALES["heavy"]
    part = ops.grad_sumsq_partials(o["g"], o["w"], o["isk"], l2gs, _slot(o, slot), _nan_partials())
    N = float(ops.clip_scale(part, 1e30)[0])
    assert np.isfinite(N) and N > 10
    one = 0x3F800000
    for c in (N, N * (1 + 2.0 ** -20), 4 * N, 1e30):                 # N <= c (N == c included): 1.0f as bits
        out = ops.clip_scale(part, c)
        assert float(out[0]) == N and _bits(out)[1].item() == one, c
    zero = torch.zeros(ops.ADAM_PARTIALS, device="cuda")
    for c in (1e-30, 1.0, 1e30):                                     # N = 0
        out = ops.clip_scale(zero, c)
        assert float(out[0]) == 0.0 and _bits(out)[1].item() == one, c
    for c in (N * (1 - 2.0 ** -20), 0.25 * N, 0.3137 * N, 1.0, 1e-3, 1e-30):      # N > c: N * s within 2 ulp of c
        c32 = float(np.float32(c))
        out = ops.clip_scale(part, c)
        s = float(out[1])
        assert float(out[0]) == N and 0 < s < 1
        assert abs(N * s - c32) <= 2 * float(np.spacing(np.float32(c32))), (c, N * s)
    # hand-made partials: the fixed order adds 2048 equal values exactly
    quarter = torch.full((ops.ADAM_PARTIALS,), 0.25, device="cuda")
    out = ops.clip_scale(quarter, 2.0)
    assert float(out[0]) == float(np.sqrt(np.float32(512.0)))        # sqrtf is correctly rounded
    assert abs(float(out[1]) - 2.0 / np.sqrt(512.0)) <= float(np.spacing(np.float32(2.0 / np.sqrt(512.0))))


@pytest.mark.parametrize("bad", [float("inf"), -float("inf"), float("nan")])
def test_a_non_finite_gradient_gives_a_nan_scale(bad):
    o = _operands(1000)
    g = o["g"].clone()
    g[577] = bad
    l2gs, slot = SCALES["production"]
    _, out = _norm_and_scale(g, o["w"], o["isk"], l2gs, _slot(o, slot), 1.0)
    assert not np.isfinite(float(out[0])) and np.isnan(float(out[1]))
    frozen = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    frozen[577] = 1                                                  # ... and harmless under the mask
    _, out = _norm_and_scale(g, o["w"], o["isk"], l2gs, _slot(o, slot), 1.0, frozen=frozen)
    assert np.isfinite(float(out[0])) and 0 < float(out[1]) < 1


# ------------------------------------------------------------------------------------------------ Adam: an inactive clip is invisible
@pytest.mark.parametrize("mode", ["scale_one", "clip_value_above_all"])
@pytest.mark.parametrize("lr_on_device", [False, True])
@pytest.mark.parametrize("partials", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_inactive_clip_gives_the_bits_of_the_unclipped_entry_points(n, masked, partials, lr_on_device, mode):
    """fdn_adam_step (by value), fdn_adam_step_dev (lr_t_dev) and fdn_adam_step_masked (frozen, with and without lr_t_dev) against
    fdn_adam_step_clipped with a device scale of 1.0 -- what fdn_clip_scale leaves when N <= c -- or a clip_value above every |g'|."""
    o = _operands(n)
    h = o["host"]
    l2gs, slot = SCALES["heavy"]
    kw = {}
    if masked:
        kw["frozen"] = _dev(_mask(n, "ranges"))
    if lr_on_device:
        kw["lr_t_dev"] = torch.tensor([LR_T], device="cuda", dtype=torch.float32)
    res = []
    for clipped in (False, True):
        w, m, v = o["w"].clone(), o["m"].clone(), o["v"].clone()
        part = _nan_partials() if partials else None
        ckw = {}
        if clipped and mode == "scale_one":
            _, out = _norm_and_scale(o["g"], o["w"], o["isk"], l2gs, _slot(o, slot), 1e30, frozen=kw.get("frozen"))
            ckw["g_scale_dev"] = out[1:2]
        elif clipped:
            gp = R.step_gradient(h["g"], h["w"], h["isk"], R.l2s_f32(l2gs, slot))
            ckw["clip_value"] = 1.001 * float(np.abs(gp).max())
        ops.adam_step(w, o["g"], m, v, o["isk"], LR_T, 0.9, 0.999, 1e-7, l2gs, _slot(o, slot), sumsq_partials=part, **kw, **ckw)
        res.append((w, m, v, part))
    (wa, ma, va, pa), (wb, mb, vb, pb) = res
    assert torch.equal(_bits(wa), _bits(wb)) and torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
    assert not torch.equal(wa, o["w"]) and bool(torch.isfinite(wa).all())
    if partials:
        assert bool(torch.isfinite(pa).all()) and torch.equal(_bits(pa), _bits(pb))


# ------------------------------------------------------------------------------------------------ Adam: single statements to the bit
@pytest.mark.parametrize("n", SIZES)
def test_device_scale_is_one_fp32_multiply(n):
    """l2_grad_scale = 0: g' = g, so a device scale of 0.37 must give the bits of the unclipped entry point on torch's fp32 g * 0.37."""
    o = _operands(n)
    scale = torch.tensor([0.37], device="cuda", dtype=torch.float32)
    wa, ma, va, pa = o["w"].clone(), o["m"].clone(), o["v"].clone(), _nan_partials()
    ops.adam_step(wa, o["g"] * 0.37, ma, va, o["isk"], LR_T, 0.9, 0.999, 1e-7, 0.0, sumsq_partials=pa)
    wb, mb, vb, pb = o["w"].clone(), o["m"].clone(), o["v"].clone(), _nan_partials()
    ops.adam_step(wb, o["g"], mb, vb, o["isk"], LR_T, 0.9, 0.999, 1e-7, 0.0, sumsq_partials=pb, g_scale_dev=scale)
    assert torch.equal(_bits(wa), _bits(wb)) and torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
    assert torch.equal(_bits(pa), _bits(pb))
    wc, mc, vc = o["w"].clone(), o["m"].clone(), o["v"].clone()      # ... and the scale does act
    ops.adam_step(wc, o["g"], mc, vc, o["isk"], LR_T, 0.9, 0.999, 1e-7, 0.0)
    assert not torch.equal(mc, mb)


@pytest.mark.parametrize("n", SIZES)
def test_clip_value_is_torch_clamp_and_keeps_nan(n):
    """l2_grad_scale = 0, clip_value = 0.5 (about 62 % of a standard normal gradient lies inside): the bits of the unclipped entry point on
    torch.clamp(g, -c, c); a NaN gradient stays NaN through the comparisons and lands in w."""
    o = _operands(n)
    c = 0.5
    g = o["g"].clone()
    nan_at = n // 2
    g[nan_at] = float("nan")
    wa, ma, va = o["w"].clone(), o["m"].clone(), o["v"].clone()
    ops.adam_step(wa, torch.clamp(g, -c, c), ma, va, o["isk"], LR_T, 0.9, 0.999, 1e-7, 0.0)
    wb, mb, vb = o["w"].clone(), o["m"].clone(), o["v"].clone()
    ops.adam_step(wb, g, mb, vb, o["isk"], LR_T, 0.9, 0.999, 1e-7, 0.0, clip_value=c)
    ok = torch.ones(n, dtype=torch.bool, device="cuda")
    ok[nan_at] = False
    for a, b in ((wa, wb), (ma, mb), (va, vb)):
        assert torch.equal(_bits(a)[ok], _bits(b)[ok])
        assert bool(torch.isnan(a[nan_at])) and bool(torch.isnan(b[nan_at]))
    assert bool(torch.isfinite(wb[ok]).all())
    if n > 1:
        assert float(mb[ok].abs().max()) <= 0.9 * float(o["m"].abs().max()) + 0.1 * c * (1 + 1e-6)     # |m'| <= b1 |m| + (1 - b1) c


# ------------------------------------------------------------------------------------------------ Adam: the general case
@pytest.mark.parametrize("pattern", ["none", "ranges"])
@pytest.mark.parametrize("kind", ["global_clipnorm", "clipvalue"])
def test_three_clipped_steps_against_float64_clip_then_keras_adam(kind, pattern):
    """L2 on (l2s = 0.4) and the clip active: global_clipnorm = a quarter of the float64 norm of the first step's gradient (the reference
    alone decides that it is active, and says so), clipvalue = 0.5.  Measure and bounds of test_gpu_kernels.py::test_adam_and_l2:
    max |error| over max |reference|, w 5e-5, m 1e-5, v 5e-5."""
    rng = np.random.default_rng(13)
    n = 10007
    w = rng.normal(size=n).astype(np.float32)
    isk = rng.uniform(size=n) < 0.8
    grads = [rng.normal(size=n).astype(np.float32) for _ in range(3)]
    fz_h = _mask(n, pattern)
    live = fz_h == 0
    frozen = _dev(fz_h) if pattern != "none" else None
    l2gs, slot = 0.05, torch.tensor([8.0], device="cuda")
    l2s = R.l2s_f32(l2gs, 8.0)
    c = 0.25 * R.global_norm(R.step_gradient(grads[0], w, isk, l2s, live)) if kind == "global_clipnorm" else 0.5
    wr, mr, vr = w.astype(np.float64), np.zeros(n), np.zeros(n)
    dw, dm, dv, dk = _dev(w), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), _dev(isk.astype(np.uint8))
    part, out = _nan_partials(), torch.zeros(2, device="cuda")
    fkw = {} if frozen is None else {"frozen": frozen}
    for t, g in enumerate(grads, 1):
        lr_t = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        w_before = wr.copy()
        norm = R.clipped_adam_step(wr, g, mr, vr, isk, t, 1e-3, l2s, live=live, **{kind: c})
        dg = _dev(g)
        if kind == "global_clipnorm":
            assert norm > 2 * c                                      # active, by the reference's own norm
            ops.grad_sumsq_partials(dg, dw, dk, l2gs, slot, part, **fkw)
            ops.clip_scale(part, c, out)
            ops.adam_step(dw, dg, dm, dv, dk, lr_t, 0.9, 0.999, 1e-7, l2gs, slot, g_scale_dev=out[1:2], **fkw)
            err, bound = R.norm_check(float(out[0]), g, w_before, isk, l2s, live)
            assert err <= bound
            assert abs(float(out[1]) - R.clip_scale(norm, c)) <= 1e-6 * R.clip_scale(norm, c)
        else:
            gp = R.step_gradient(g, w_before, isk, l2s, live)
            assert 0.2 < np.mean(np.abs(gp[live]) > c) < 0.8         # active
            ops.adam_step(dw, dg, dm, dv, dk, lr_t, 0.9, 0.999, 1e-7, l2gs, slot, clip_value=c, **fkw)
    rel = lambda got, ref: np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30)
    ew, em, ev = rel(dw, wr), rel(dm, mr), rel(dv, vr)
    print("%s %s: w %.3e, m %.3e, v %.3e" % (kind, pattern, ew, em, ev))
    assert ew <= 5e-5 and em <= 1e-5 and ev <= 5e-5
    # the clip is visible at these bounds: the unclipped slots are far away
    mu, vu = np.zeros(n), np.zeros(n)
    wu = w.astype(np.float64)
    for t, g in enumerate(grads, 1):
        R.clipped_adam_step(wu, g, mu, vu, isk, t, 1e-3, l2s, live=live)
    assert rel(dm, mu) > 1e-2 and rel(dv, vu) > 1e-2
    if frozen is not None:
        fzb = frozen.bool()
        assert torch.equal(_bits(dw[fzb]), _bits(_dev(w)[fzb])) and not bool(dm[fzb].any()) and not bool(dv[fzb].any())


# ------------------------------------------------------------------------------------------------ a non-finite norm
@pytest.mark.parametrize("n", SIZES[1:])
def test_non_finite_norm_turns_every_unfrozen_parameter_into_nan_and_leaves_frozen_ones_alone(n):
    o = _operands(n)
    l2gs, slot = SCALES["production"]
    fz_h = _mask(n, "ranges")
    frozen = _dev(fz_h)
    fz = frozen.bool()
    g = o["g"].clone()
    g[int(np.flatnonzero(fz_h == 0)[-1])] = float("inf")
    w = o["w"].clone()
    m = torch.where(fz, torch.full_like(o["m"], SENTINEL), o["m"])
    v = torch.where(fz, torch.full_like(o["v"], SENTINEL), o["v"])
    m0, v0 = m.clone(), v.clone()
    part, out = _norm_and_scale(g, w, o["isk"], l2gs, _slot(o, slot), 1.0, frozen=frozen)
    assert np.isnan(float(out[1]))
    ops.adam_step(w, g, m, v, o["isk"], LR_T, 0.9, 0.999, 1e-7, l2gs, _slot(o, slot), frozen=frozen, g_scale_dev=out[1:2])
    assert bool(torch.isnan(w[~fz]).all())
    assert torch.equal(_bits(w[fz]), _bits(o["w"][fz])) and torch.equal(_bits(m[fz]), _bits(m0[fz])) and torch.equal(_bits(v[fz]), _bits(v0[fz]))


# ------------------------------------------------------------------------------------------------ captured
def test_recorded_chain_of_the_three_launches_follows_gradient_and_step_size_between_replays():
    """Sum of squares, norm and scale, clipped Adam recorded into one HIP graph on one stream (a linear chain: no parallel branches) and
    replayed three times with a new gradient and a new step size, against eager launches with the step size by value."""
    n = 300_007
    rng = np.random.default_rng(5)
    w0, m0, v0 = _dev(rng.standard_normal(n).astype(np.float32)), _dev((0.01 * rng.standard_normal(n)).astype(np.float32)), _dev((1e-4 * rng.random(n)).astype(np.float32))
    isk = _dev((rng.random(n) < 0.9).astype(np.uint8))
    frozen = _dev(_mask(n, "ranges"))
    grads = [_dev((s * rng.standard_normal(n)).astype(np.float32)) for s in (1.0, 0.01, 3.0)]      # norms about 440, 160 (the L2 term alone), 1300: the middle one is below c
    lrs = [1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) for t in (1, 2)] + [3.3e-4]
    l2gs, slot, c = 0.05, torch.tensor([8.0], device="cuda"), 300.0
    wa, ma, va = w0.clone(), m0.clone(), v0.clone()
    wb, mb, vb = w0.clone(), m0.clone(), v0.clone()
    g_static, lr_dev = torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
    clip_a, out_a, part_a = _nan_partials(), torch.zeros(2, device="cuda"), _nan_partials()
    clip_b, out_b, part_b = _nan_partials(), torch.zeros(2, device="cuda"), _nan_partials()

    def chain(w, g, m, v, clip_part, out, part, lr_t, lr_t_dev):
        ops.grad_sumsq_partials(g, w, isk, l2gs, slot, clip_part, frozen=frozen)
        ops.clip_scale(clip_part, c, out)
        ops.adam_step(w, g, m, v, isk, lr_t, 0.9, 0.999, 1e-7, l2gs, slot, sumsq_partials=part, lr_t_dev=lr_t_dev, frozen=frozen,
                      g_scale_dev=out[1:2])
    # one eager pass on copies first: loading the library and its code object must not fall into the capture
    chain(wb.clone(), g_static, mb.clone(), vb.clone(), clip_b.clone(), out_b.clone(), part_b.clone(), 0.0, lr_dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):          # recording executes nothing
        chain(wb, g_static, mb, vb, clip_b, out_b, part_b, 0.0, lr_dev)
    torch.cuda.synchronize()
    assert torch.equal(wa, wb)
    scales = []
    for g, lr_t in zip(grads, lrs):
        chain(wa, g, ma, va, clip_a, out_a, part_a, lr_t, None)
        g_static.copy_(g)
        lr_dev.fill_(lr_t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(wa), _bits(wb)) and torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
        assert torch.equal(_bits(part_a), _bits(part_b)) and torch.equal(_bits(clip_a), _bits(clip_b)) and torch.equal(_bits(out_a), _bits(out_b))
        scales.append(float(out_b[1]))
    assert scales[0] < 1 and scales[1] == 1.0 and scales[2] < scales[0]
    fz = frozen.bool()
    assert torch.equal(wb[fz], w0[fz]) and torch.equal(mb[fz], m0[fz]) and not torch.equal(wb[~fz], w0[~fz])

"""Weight EMA on the GPU, kernel level: fdn_adam_step_ema through ops.adam_step(ema=).

What is the same statement on the same operands is compared bit for bit -- w, m, v and the partials against the entry points without an
average, a frozen element's average against its weight, momentum 0 against the weights, a recorded launch against eager ones; the average
itself against the float64 recurrence of tests/_ema_ref.py, fed the exact fp32 weights the device wrote, at the bound derived there."""
import importlib

import numpy as np
import pytest
import torch

import _ema_ref as E

pytestmark = pytest.mark.gpu

ops = importlib.import_module("4dflownet_amd.ops")
SIZES = [1, 1000, 2 * 2048 * 256 + 77]         # the last: every thread of the 2048-block launch takes a third trip, some of them
PATTERNS = ["none", "all", "alternating", "ranges"]
MOMENTA = [0.0, 0.5, 0.99, 0.999]
LR_T = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
L2GS, SLOT = 0.05, 8.0                         # l2s = 0.4: the L2 term is a visible part of the gradient
T = 5
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
    """Shared, never modified: the tests work on clones."""
    if n not in _cache:
        rng = np.random.default_rng(n + 1)
        h = dict(w=rng.standard_normal(n).astype(np.float32), g=rng.standard_normal(n).astype(np.float32),
                 m=(0.01 * rng.standard_normal(n)).astype(np.float32), v=(1e-4 * rng.random(n)).astype(np.float32),
                 isk=(rng.random(n) < 0.9).astype(np.uint8), a=rng.standard_normal(n).astype(np.float32))
        o = dict((k, _dev(x)) for k, x in h.items())
        o["slot"] = torch.tensor([SLOT], device="cuda")
        o["grads"] = [o["g"]] + [_dev(rng.standard_normal(n).astype(np.float32)) for _ in range(T - 1)]
        _cache[n] = o
    return _cache[n]


def _bits(t):
    return t.view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _nan(n):
    return torch.full((n,), float("nan"), device="cuda")


def _step(o, w, m, v, g=None, **kw):
    ops.adam_step(w, o["g"] if g is None else g, m, v, o["isk"], LR_T, 0.9, 0.999, 1e-7, L2GS, o["slot"], **kw)


def _within(got, ref, bound, what):
    err = np.abs(_np(got).astype(np.float64) - ref)
    worst = int(np.argmax(err))
    print("%s: max |ema - ref| %.3e, bound there %.3e, least slack %.3e" % (what, err[worst], bound[worst], (bound - err).min()))
    assert np.isfinite(err).all() and (err <= bound).all(), what


# ------------------------------------------------------------------------------------------------ (a) nothing but ema changes
@pytest.mark.parametrize("route", ["plain", "g_scale_dev", "clip_value", "lr_t_dev"])
@pytest.mark.parametrize("pattern", ["none", "ranges"])
@pytest.mark.parametrize("n", SIZES)
def test_w_m_v_and_partials_get_the_bits_of_the_call_without_ema(n, pattern, route):
    """fdn_adam_step / _dev / _masked / _clipped without an average against fdn_adam_step_ema on the same operands, the average running
    (ema_init = 0) and starting (ema_init = 1)."""
    o = _operands(n)
    kw = {}
    if pattern != "none":
        kw["frozen"] = _dev(_mask(n, pattern))
    if route == "g_scale_dev":
        kw["g_scale_dev"] = torch.tensor([0.37], device="cuda")
    elif route == "clip_value":
        kw["clip_value"] = 0.5
    elif route == "lr_t_dev":
        kw["lr_t_dev"] = torch.tensor([LR_T], device="cuda", dtype=torch.float32)
    res = []
    for ekw in (None, dict(ema_momentum=0.99, ema_init=False), dict(ema_momentum=0.5, ema_init=True)):
        w, m, v, part = o["w"].clone(), o["m"].clone(), o["v"].clone(), _nan(ops.ADAM_PARTIALS)
        ema = None
        if ekw is not None:
            ema = o["a"].clone()
            ekw = dict(ekw, ema=ema)
        _step(o, w, m, v, sumsq_partials=part, **kw, **(ekw or {}))
        res.append((w, m, v, part, ema))
    w0, m0, v0, p0, _ = res[0]
    assert bool(torch.isfinite(p0).all()) and not torch.equal(w0, o["w"])
    for w, m, v, part, ema in res[1:]:
        assert torch.equal(_bits(w), _bits(w0)) and torch.equal(_bits(m), _bits(m0)) and torch.equal(_bits(v), _bits(v0))
        assert torch.equal(_bits(part), _bits(p0))
        assert bool(torch.isfinite(ema).all()) and not torch.equal(ema, o["a"])       # ... and the average did move
    # without partials (the other grid) too
    wa, ma, va = o["w"].clone(), o["m"].clone(), o["v"].clone()
    _step(o, wa, ma, va, **kw)
    wb, mb, vb, eb = o["w"].clone(), o["m"].clone(), o["v"].clone(), o["a"].clone()
    _step(o, wb, mb, vb, ema=eb, ema_momentum=0.99, **kw)
    assert torch.equal(_bits(wa), _bits(wb)) and torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
    assert torch.equal(_bits(eb), _bits(res[1][4]))                                    # the same average on either grid


# ------------------------------------------------------------------------------------------------ (b) the first step
@pytest.mark.parametrize("momentum", MOMENTA)
@pytest.mark.parametrize("n", SIZES)
def test_first_step_starts_from_the_weights_and_never_reads_the_buffer(n, momentum):
    o = _operands(n)
    w, m, v, ema = o["w"].clone(), o["m"].clone(), o["v"].clone(), _nan(n)
    _step(o, w, m, v, ema=ema, ema_momentum=momentum, ema_init=True)
    assert bool(torch.isfinite(ema).all())
    weights = [_np(o["w"]), _np(w)]
    ref = E.ema_chain(weights, momentum)
    _within(ema, ref[0], E.ema_bound(weights, ref), "n %d momentum %g" % (n, momentum))
    if momentum == 0.0:
        assert torch.equal(_bits(ema), _bits(w))
    else:
        assert not torch.equal(ema, w) and not torch.equal(ema, o["w"])
    # ... while without ema_init the old contents are what is averaged
    w2, m2, v2, ema2 = o["w"].clone(), o["m"].clone(), o["v"].clone(), _nan(n)
    _step(o, w2, m2, v2, ema=ema2, ema_momentum=0.5, ema_init=False)
    assert bool(torch.isnan(ema2).all()) and torch.equal(_bits(w2), _bits(w))


# ------------------------------------------------------------------------------------------------ (c) the recurrence
@pytest.mark.parametrize("momentum", MOMENTA)
@pytest.mark.parametrize("n", SIZES)
def test_five_chained_steps_against_the_float64_recurrence_on_the_weights_read_back(n, momentum):
    """|ema - ref| <= 4 T 2^-24 max_t(|w_t|, |a_t|) per element (tests/_ema_ref.py::ema_bound), checked after every step with the T
    reached so far; momentum 0: the average is the weights, bit for bit."""
    o = _operands(n)
    w, m, v, ema = o["w"].clone(), o["m"].clone(), o["v"].clone(), _nan(n)
    weights = [_np(w)]
    for t in range(1, T + 1):
        _step(o, w, m, v, g=o["grads"][t - 1], ema=ema, ema_momentum=momentum, ema_init=t == 1)
        weights.append(_np(w))
        ref = E.ema_chain(weights, momentum)
        _within(ema, ref[-1], E.ema_bound(weights, ref), "n %d momentum %g step %d" % (n, momentum, t))
        if momentum == 0.0:
            assert torch.equal(_bits(ema), _bits(w))
    assert not np.array_equal(weights[-1], weights[0])
    if momentum >= 0.5 and n > 1:                                            # the average lags: it is neither the first nor the last weights
        a = _np(ema).astype(np.float64)
        assert np.abs(a - weights[-1]).max() > 1e-4 and np.abs(a - weights[0]).max() > (1 - momentum) * 1e-4


# ------------------------------------------------------------------------------------------------ (d) frozen elements
@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS[1:])
@pytest.mark.parametrize("n", SIZES)
def test_a_frozen_elements_average_is_its_weight_and_its_g_m_v_stay_unread(n, pattern, init):
    o = _operands(n)
    fz_h = _mask(n, pattern)
    frozen = _dev(fz_h)
    fz = frozen.bool()
    nan = _nan(n)
    g = torch.where(fz, nan, o["g"])
    w, m, v = o["w"].clone(), torch.where(fz, nan, o["m"]), torch.where(fz, nan, o["v"])
    ema = _nan(n) if init else o["a"].clone()
    part = _nan(ops.ADAM_PARTIALS)
    _step(o, w, m, v, g=g, frozen=frozen, ema=ema, ema_momentum=0.99, ema_init=init, sumsq_partials=part)
    assert torch.equal(_bits(ema[fz]), _bits(o["w"][fz])) and torch.equal(_bits(w[fz]), _bits(o["w"][fz]))
    assert bool(torch.isnan(m[fz]).all()) and bool(torch.isnan(v[fz]).all())            # neither read nor written
    assert bool(torch.isfinite(ema).all()) and bool(torch.isfinite(w).all()) and bool(torch.isfinite(part).all())
    live = fz_h == 0
    if live.any():
        weights = [_np(o["w"]), _np(w)]
        prev = weights[0] if init else _np(o["a"])
        ref = E.ema_step(prev, weights[0], weights[1], 0.99, init=init, frozen=fz_h)
        _within(ema, ref, E.ema_bound(weights + [prev], [ref]), "n %d %s init %d" % (n, pattern, init))
        assert not torch.equal(ema[~fz], w[~fz])
    # the unfrozen elements: the bits of the masked step without an average
    w2, m2, v2, p2 = o["w"].clone(), torch.where(fz, nan, o["m"]), torch.where(fz, nan, o["v"]), _nan(ops.ADAM_PARTIALS)
    _step(o, w2, m2, v2, g=g, frozen=frozen, sumsq_partials=p2)
    assert torch.equal(_bits(w), _bits(w2)) and torch.equal(_bits(m), _bits(m2)) and torch.equal(_bits(v), _bits(v2))
    assert torch.equal(_bits(part), _bits(p2))


# ------------------------------------------------------------------------------------------------ (e) captured
def test_recorded_launch_replayed_equals_eager_bits():
    """One launch with an average recorded into a HIP graph on one stream (a single node: no parallel branches) and replayed three times
    with a new gradient and a new step size, against eager launches with the step size by value."""
    n = 300_007
    rng = np.random.default_rng(5)
    w0, m0, v0 = _dev(rng.standard_normal(n).astype(np.float32)), _dev((0.01 * rng.standard_normal(n)).astype(np.float32)), _dev((1e-4 * rng.random(n)).astype(np.float32))
    a0 = _dev(rng.standard_normal(n).astype(np.float32))
    isk = _dev((rng.random(n) < 0.9).astype(np.uint8))
    frozen = _dev(_mask(n, "ranges"))
    slot = torch.tensor([SLOT], device="cuda")
    grads = [_dev((s * rng.standard_normal(n)).astype(np.float32)) for s in (1.0, 0.01, 3.0)]
    lrs = [1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) for t in (1, 2)] + [3.3e-4]
    wa, ma, va, ea, pa = w0.clone(), m0.clone(), v0.clone(), a0.clone(), _nan(ops.ADAM_PARTIALS)
    wb, mb, vb, eb, pb = w0.clone(), m0.clone(), v0.clone(), a0.clone(), _nan(ops.ADAM_PARTIALS)
    g_static, lr_dev = torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")

    def launch(w, g, m, v, ema, part, lr_t, lr_t_dev):
        ops.adam_step(w, g, m, v, isk, lr_t, 0.9, 0.999, 1e-7, L2GS, slot, sumsq_partials=part, lr_t_dev=lr_t_dev, frozen=frozen,
                      ema=ema, ema_momentum=0.99, ema_init=False)
    # one eager pass on copies first: loading the library and its code object must not fall into the capture
    launch(wb.clone(), g_static, mb.clone(), vb.clone(), eb.clone(), pb.clone(), 0.0, lr_dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):          # recording executes nothing
        launch(wb, g_static, mb, vb, eb, pb, 0.0, lr_dev)
    torch.cuda.synchronize()
    assert torch.equal(wa, wb) and torch.equal(ea, eb)
    for g, lr_t in zip(grads, lrs):
        launch(wa, g, ma, va, ea, pa, lr_t, None)
        g_static.copy_(g)
        lr_dev.fill_(lr_t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(wa), _bits(wb)) and torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
        assert torch.equal(_bits(ea), _bits(eb)) and torch.equal(_bits(pa), _bits(pb))
    fz = frozen.bool()
    assert torch.equal(_bits(eb[fz]), _bits(w0[fz])) and not torch.equal(eb[~fz], a0[~fz]) and not torch.equal(eb[~fz], wb[~fz])

"""fdn_adam_step_masked on the GPU.  Unfrozen elements: the bits of fdn_adam_step[_dev] on the same operands (the same kernel and the same
statements; derived, not measured).  Frozen elements: w, m and v keep their bits although the gradient there is NaN and m, v hold a
sentinel -- they are not read.  The per-block sums of squares cover every kernel element, frozen or not: the bits of
fdn_l2_sumsq_partials of the resulting w (the same blocking and the same summation statement)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ops = importlib.import_module("4dflownet_amd.ops")
SIZES = [1, 1000, 2 * 2048 * 256 + 77]         # the last: every thread of the 2048-block launch takes a third trip, some of them
SENTINEL = -7.25
LR_T = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
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
            assert n < 100 or (lo % 64 and hi % 64 and hi > lo)
    else:
        assert pattern == "none"
    return f


def _operands(n):
    """Shared, never modified: the tests work on clones."""
    if n not in _cache:
        rng = np.random.default_rng(n)
        dev = lambda a: torch.from_numpy(a).cuda()
        _cache[n] = dict(w=dev(rng.standard_normal(n).astype(np.float32)), g=dev(rng.standard_normal(n).astype(np.float32)),
                         m=dev((0.01 * rng.standard_normal(n)).astype(np.float32)), v=dev((1e-4 * rng.random(n)).astype(np.float32)),
                         isk=dev((rng.random(n) < 0.9).astype(np.uint8)), slot=torch.tensor([8.0], device="cuda"))
    return _cache[n]


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("lr_on_device", [False, True])
@pytest.mark.parametrize("partials", [False, True])
@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "ranges"])
@pytest.mark.parametrize("n", SIZES)
def test_masked_step(n, pattern, partials, lr_on_device):
    o = _operands(n)
    frozen = torch.from_numpy(_mask(n, pattern)).cuda()
    fz = frozen.bool()
    lr_dev = torch.tensor([LR_T], device="cuda", dtype=torch.float32) if lr_on_device else None
    lr_kw = {"lr_t_dev": lr_dev} if lr_on_device else {}
    # reference: the unmasked entry point on copies
    wr, mr, vr = o["w"].clone(), o["m"].clone(), o["v"].clone()
    ops.adam_step(wr, o["g"], mr, vr, o["isk"], LR_T, 0.9, 0.999, 1e-7, 1e-6, o["slot"], **lr_kw)
    # masked: NaN gradients and sentinel slots wherever the element is frozen
    w = o["w"].clone()
    g = torch.where(fz, torch.full_like(o["g"], float("nan")), o["g"])
    m = torch.where(fz, torch.full_like(o["m"], SENTINEL), o["m"])
    v = torch.where(fz, torch.full_like(o["v"], SENTINEL), o["v"])
    g0 = g.clone()
    part = torch.full((ops.ADAM_PARTIALS,), float("nan"), device="cuda") if partials else None
    ops.adam_step(w, g, m, v, o["isk"], LR_T, 0.9, 0.999, 1e-7, 1e-6, o["slot"], sumsq_partials=part, frozen=frozen, **lr_kw)
    live = ~fz
    assert torch.equal(_bits(w)[live], _bits(wr)[live]) and torch.equal(_bits(m)[live], _bits(mr)[live]) and torch.equal(_bits(v)[live], _bits(vr)[live])
    assert torch.equal(_bits(w)[fz], _bits(o["w"])[fz])
    assert bool((m[fz] == SENTINEL).all()) and bool((v[fz] == SENTINEL).all())
    assert torch.equal(_bits(g), _bits(g0))                            # the gradient is only read
    if bool(live.any()):
        assert not torch.equal(w[live], o["w"][live])                  # ... and the step did move what it may move
    assert bool(torch.isfinite(w).all())
    if partials:
        want = ops.l2_sumsq_partials(w, o["isk"], torch.zeros(ops.ADAM_PARTIALS, device="cuda"))
        assert bool(torch.isfinite(part).all()) and torch.equal(_bits(part), _bits(want))
        assert float(part.sum()) > 0 or not bool(o["isk"].any())


def test_recorded_masked_launch_follows_the_step_size_between_replays():
    """One masked Adam launch captured into a HIP graph (a single node: no parallel branches) and replayed with a new gradient and a new
    step size each time, against eager by-value launches of the same entry point."""
    n = 300_007
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(a).cuda()
    o = _operands(1000)                            # (only the batch-size slot is taken from it)
    w0, m0, v0 = dev(rng.standard_normal(n).astype(np.float32)), dev((0.01 * rng.standard_normal(n)).astype(np.float32)), dev((1e-4 * rng.random(n)).astype(np.float32))
    isk = dev((rng.random(n) < 0.9).astype(np.uint8))
    frozen = torch.from_numpy(_mask(n, "ranges")).cuda()
    grads = [dev(rng.standard_normal(n).astype(np.float32)) for _ in range(3)]
    lrs = [1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) for t in (1, 2)] + [3.3e-4]
    wa, ma, va = w0.clone(), m0.clone(), v0.clone()
    wb, mb, vb = w0.clone(), m0.clone(), v0.clone()
    g_static = torch.zeros(n, device="cuda")
    lr_dev = torch.zeros(1, device="cuda")
    part, part_ref = torch.zeros(ops.ADAM_PARTIALS, device="cuda"), torch.zeros(ops.ADAM_PARTIALS, device="cuda")
    args = (isk, 0.0, 0.9, 0.999, 1e-7, 1e-6, o["slot"])
    # one eager launch on copies first: loading the library and its code object must not fall into the capture
    ops.adam_step(wb.clone(), g_static, mb.clone(), vb.clone(), *args, sumsq_partials=part.clone(), lr_t_dev=lr_dev, frozen=frozen)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):          # recording executes nothing
        ops.adam_step(wb, g_static, mb, vb, *args, sumsq_partials=part, lr_t_dev=lr_dev, frozen=frozen)
    torch.cuda.synchronize()
    assert torch.equal(wa, wb)
    for g, lr_t in zip(grads, lrs):
        ops.adam_step(wa, g, ma, va, isk, lr_t, 0.9, 0.999, 1e-7, 1e-6, o["slot"], sumsq_partials=part_ref, frozen=frozen)
        g_static.copy_(g)
        lr_dev.fill_(lr_t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(part, part_ref)
    fz = frozen.bool()
    assert torch.equal(wb[fz], w0[fz]) and torch.equal(mb[fz], m0[fz]) and not torch.equal(wb[~fz], w0[~fz])

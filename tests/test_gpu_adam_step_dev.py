"""fdn_adam_step_dev on the GPU: the same update as fdn_adam_step bit for bit, and -- what it exists for -- a launch recorded into a HIP graph
whose step size can still change between replays.  Bit for bit is a derived condition: it is the same kernel, the step size reaches it as the
same fp32 value (float64 -> fp32 once, by the argument conversion or by fill_), and every other operand is identical."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ops = importlib.import_module("4dflownet_amd.ops")
N = 300_007                      # not a multiple of the block size; several trips of the grid-stride loop with the fixed grid


def _state(seed):
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.from_numpy(a).cuda()
    w = dev(rng.standard_normal(N).astype(np.float32))
    m = dev((0.01 * rng.standard_normal(N)).astype(np.float32))
    v = dev((1e-4 * rng.random(N)).astype(np.float32))
    isk = dev((rng.random(N) < 0.9).astype(np.uint8))
    grads = [dev(rng.standard_normal(N).astype(np.float32)) for _ in range(4)]
    return w, m, v, isk, grads


LR_T = [1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) for t in (1, 2, 3)] + [3.3e-4]      # float64 values, the last one a changed learning rate


@pytest.mark.parametrize("partials", [False, True])
def test_device_step_size_gives_the_by_value_update(partials):
    slot = torch.tensor([8.0], device="cuda")
    wa, ma, va, isk, grads = _state(1)
    wb, mb, vb = wa.clone(), ma.clone(), va.clone()
    pa = torch.zeros(ops.ADAM_PARTIALS, device="cuda") if partials else None
    pb = torch.zeros(ops.ADAM_PARTIALS, device="cuda") if partials else None
    lr_dev = torch.zeros(1, device="cuda")
    for g, lr_t in zip(grads, LR_T):
        ops.adam_step(wa, g, ma, va, isk, lr_t, 0.9, 0.999, 1e-7, 1e-6, slot, sumsq_partials=pa)
        lr_dev.fill_(lr_t)
        ops.adam_step(wb, g, mb, vb, isk, 123.0, 0.9, 0.999, 1e-7, 1e-6, slot, sumsq_partials=pb, lr_t_dev=lr_dev)     # (lr_t itself is ignored)
        assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(va, vb)
        if partials:
            assert torch.equal(pa, pb)
    assert not torch.equal(wa, _state(1)[0])


def test_recorded_launch_follows_the_step_size_between_replays():
    """One Adam launch captured into a HIP graph (a single node: no parallel branches) and replayed with a new gradient and a new step size each
    time, against by-value launches.  With the by-value entry point the first step size would be frozen into the graph."""
    slot = torch.tensor([8.0], device="cuda")
    wa, ma, va, isk, grads = _state(2)
    wb, mb, vb = wa.clone(), ma.clone(), va.clone()
    g_static = torch.zeros(N, device="cuda")
    lr_dev = torch.zeros(1, device="cuda")
    part = torch.zeros(ops.ADAM_PARTIALS, device="cuda")
    part_ref = torch.zeros(ops.ADAM_PARTIALS, device="cuda")
    # one eager launch on copies first: loading the library and its code object must not fall into the capture
    ops.adam_step(wb.clone(), g_static, mb.clone(), vb.clone(), isk, 0.0, 0.9, 0.999, 1e-7, 1e-6, slot, sumsq_partials=part.clone(), lr_t_dev=lr_dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):          # recording executes nothing
        ops.adam_step(wb, g_static, mb, vb, isk, 0.0, 0.9, 0.999, 1e-7, 1e-6, slot, sumsq_partials=part, lr_t_dev=lr_dev)
    torch.cuda.synchronize()
    assert torch.equal(wa, wb)
    for g, lr_t in zip(grads, LR_T):
        ops.adam_step(wa, g, ma, va, isk, lr_t, 0.9, 0.999, 1e-7, 1e-6, slot, sumsq_partials=part_ref)
        g_static.copy_(g)
        lr_dev.fill_(lr_t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(part, part_ref)

"""Gradient accumulation under data parallelism: two ranks run TrainerController(accum_steps=2).train_step on their shards of two
groups of global micro-batches.  Collectives happen only when a group is applied, and on the accumulator; an empty shard contributes
nothing, also when it is the rank's FIRST micro-batch of the group (the `first` hand-over).

Spawned the way tests/test_gpu_parallel.py spawns its ranks: with >= 2 GPUs one GPU each over nccl (= RCCL), on a 1-GPU box both ranks on
cuda:0 over gloo with host staging."""
import importlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import flownet_oracle as O

pytestmark = pytest.mark.gpu

P, R, LB, HB = 8, 2, 1, 1
LR = 1e-4


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _init(rank, world, port):
    ngpu = torch.cuda.device_count()
    backend = "nccl" if ngpu >= world else "gloo"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank % ngpu), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(rank % ngpu)
    parallel = importlib.import_module("4dflownet_amd.parallel")
    parallel.init_from_env(backend=backend)
    return parallel


def _groups():
    """Group A: a global micro-batch of 4 rows, then one of 2 -> rank 1's SECOND shard is empty.  Group B: 2 rows, then 4 -> rank 1's FIRST
    shard is empty."""
    sb = lambda n, seed: O.synthetic_batch(n, P, R, seed=seed)
    return [[sb(4, 31), sb(2, 32)], [sb(2, 34), sb(4, 35)]]


def _tc(trainer, **kw):
    return trainer.TrainerController(P, R, initial_learning_rate=LR, quicksave_enable=False, low_resblock=LB, hi_resblock=HB, seed=0, **kw)


def _worker(rank, world, port, q, bucketed):
    parallel = _init(rank, world, port)
    trainer = importlib.import_module("4dflownet_amd.trainer")
    started = []
    start = parallel.allreduce_sum_start

    def counting_start(flat):
        started.append(flat.numel())
        return start(flat)
    parallel.allreduce_sum_start = counting_start
    tc = _tc(trainer, accum_steps=2, bucketed_allreduce=bucketed)
    out = []
    for group in _groups():
        snaps, counts = [], []
        for gb in group:
            rows = next(iter(parallel.ShardedIndexSampler(len(gb[0]), 2, shuffle=False)))      # this rank's slice of the global micro-batch
            tc.train_step(tuple(a[rows] for a in gb))
            snaps.append((len(rows), tc.model.flat_g_ext.cpu().numpy().copy()))
            counts.append(len(started))
        out.append((snaps, counts, tc.accum_g_ext.cpu().numpy().copy(), tc.optimizer.iterations))
    torch.cuda.synchronize()
    parallel.barrier()
    q.put((rank, out, tc.model.flat_w.cpu().numpy().copy(), list(started), list(tc.model.grad_buckets)))
    torch.distributed.destroy_process_group()


def _run(target, world=2, extra=()):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(extra)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return res


@pytest.fixture(scope="module")
def single():
    """The same rows in one process: accumulated (accum_steps = 2 on the global micro-batches) and as one big batch per group."""
    trainer = importlib.import_module("4dflownet_amd.trainer")
    tc = _tc(trainer, accum_steps=2)
    accs = []
    for group in _groups():
        for gb in group:
            tc.train_step(gb)
        accs.append(tc.accum_g_ext.cpu().numpy().copy())
    big = _tc(trainer)
    big_g = []
    for group in _groups():
        big.train_step(tuple(np.concatenate([a, b], 0) for a, b in zip(*group)))
        big_g.append(big.model.flat_g_ext.cpu().numpy().copy())
    return {"accs": accs, "big_g": big_g, "big_w": big.model.flat_w.cpu().numpy().copy()}


@pytest.mark.parametrize("bucketed", [True, False])
def test_dp2_accumulated_groups(fdn, single, bucketed):
    res = _run(_worker, extra=(bucketed,))
    buckets = res[0][4]
    per_apply = len(buckets) if bucketed else 1
    assert [[n for n, _ in g[0]] for g in res[0][1]] == [[2, 2], [2, 2]]
    assert [[n for n, _ in g[0]] for g in res[1][1]] == [[2, 0], [0, 2]]                   # rank 1: second shard of A, FIRST shard of B empty
    for r in range(2):
        before = 0
        for k, (snaps, counts, acc, iterations) in enumerate(res[r][1]):
            assert counts[0] == before                                 # no collective after the first micro-step of a group
            assert counts[1] - counts[0] == per_apply >= 1             # the group's collectives, on its closing micro-step
            before = counts[1]
            assert iterations == k + 1
        n_ext = len(res[r][1][0][2])
        assert res[r][3] == ([hi - lo for lo, hi in buckets] if bucketed else [n_ext]) * 2          # slices of the accumulator, in bucket order
    for k in range(2):
        acc0, acc1 = res[0][1][k][2], res[1][1][k][2]
        assert np.array_equal(acc0.view(np.int32), acc1.view(np.int32))            # both ranks hold identical accumulators
        assert acc0[-1] == 6.0
        # exact: s_r = the float32 sum, in feeding order, of rank r's own micro-batch buffers (an empty shard contributes nothing); a
        # 2-rank SUM is one fp32 add per element
        s = []
        for r in range(2):
            mine = [g for n, g in res[r][1][k][0] if n > 0]
            tot = mine[0].copy()
            for g in mine[1:]:
                tot = tot + g
            s.append(tot)
            for n, g in res[r][1][k][0]:
                assert g[-1] == float(n) and (n > 0 or not g.any())                # flat_g_ext: the micro-batch's own local gradient
        assert np.array_equal((s[0] + s[1]).view(np.int32), acc0.view(np.int32))
        ref = single["accs"][k][:-1].astype(np.float64)
        d = acc0[:-1].astype(np.float64) - ref
        print("group %d vs single-process accumulation: rel L2 %.3e, rel max %.3e" % (k, np.linalg.norm(d) / np.linalg.norm(ref), np.abs(d).max() / np.abs(ref).max()))
        assert single["accs"][k][-1] == 6.0
        assert np.linalg.norm(d) <= 1e-3 * np.linalg.norm(ref)
        assert np.abs(d).max() <= 1e-3 * np.abs(ref).max()
    # weights after both groups: identical on both ranks; against the single-process big-batch run within 2.1 lr per step (Adam moves a
    # weight by ~lr sign(g) in its first steps: an element whose gradient is summation-order noise may go either way), every
    # well-conditioned element to 1e-6 (tests/test_gpu_parallel.py)
    assert np.array_equal(res[0][2].view(np.int32), res[1][2].view(np.int32))
    dw = np.abs(res[0][2].astype(np.float64) - single["big_w"])
    g = np.abs(single["big_g"][0][:-1])
    good = g >= 1e-3 * g.max()
    print("weights: max |dw| %.3e (%.2f lr), well-conditioned %.1f %%, max |dw| there %.3e" % (dw.max(), dw.max() / LR, 100.0 * good.mean(), dw[good].max()))
    assert dw.max() <= 4.2 * LR
    assert good.sum() > 0.2 * good.size
    assert dw[good].max() <= 1e-6

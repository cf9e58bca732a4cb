"""The predictor's shared machinery on its own: the copy-out pipeline (predictor._CopyOut), the per-network state (predictor._PredictorState)
and the one transport of a shard's rows to rank 0 on its host-staged route (gloo with a network on the device)."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import test_gpu_shard_tiler as st

pytestmark = pytest.mark.gpu

predictor = importlib.import_module("4dflownet_amd.predictor")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_copy_out_delivers_every_chunk_once_in_order(dtype):
    """Five chunks (3, 3, 3, 3 and 1 rows of (4,4,4,3)) through two slots of three rows: each slot is used at least twice and the last chunk
    is ragged.  Every chunk is written by a device op queued right before its push.  push(k) runs the host work of chunk k - 1 -- the order
    the predictor's loops rely on: host work of one chunk behind the production of the next --, so four chunks have arrived when the loop
    ends and flush() delivers what is still owed; after it the last two chunks, the full one and the ragged one, are there like the rest."""
    net = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()))
    predictor._CopyOut(net, predictor._state(net).pinned("chunks", (3, 4, 4, 4, 3), dtype, count=2)).flush()      # nothing was pushed
    pipe = predictor._CopyOut(net, predictor._state(net).pinned("chunks", (3, 4, 4, 4, 3), dtype, count=2))
    counts = (3, 3, 3, 3, 1)
    base = np.arange(3 * 4 * 4 * 4 * 3, dtype=np.float64).reshape(3, 4, 4, 4, 3)
    dbase = torch.from_numpy(base).cuda()
    seen = []
    for k, cnt in enumerate(counts):
        chunk = torch.empty((cnt, 4, 4, 4, 3), device="cuda", dtype=dtype)
        chunk.copy_(dbase[:cnt] * (k + 1) + 1000 * k)                      # integers below 2^24: exact in both dtypes
        pipe.push(chunk, cnt, lambda view, k=k: seen.append((k, view.copy())))
        assert [j for j, _ in seen] == list(range(k))
    pipe.flush()
    pipe.flush()                                                             # nothing is owed any more
    assert [j for j, _ in seen] == [0, 1, 2, 3, 4]
    for (k, got), cnt in zip(seen, counts):
        want = (base[:cnt] * (k + 1) + 1000 * k).astype(np.float64 if dtype == torch.float64 else np.float32)
        assert got.dtype == want.dtype and got.shape == (cnt, 4, 4, 4, 3)
        assert got.tobytes() == want.tobytes(), k
    assert [tuple(b.shape) for b in net._predictor_state.pinned_buffers["chunks"]] == [(3, 4, 4, 4, 3)] * 2


def test_switching_the_finish_keeps_the_pinned_pairs_and_the_one_copy_stream(tmp_path, monkeypatch):
    """predict_file(device_tiler=True), one row per group, under FDN_DEVICE_FINISH=1, 0 and 1 again (two calls each): the float64 pair of
    group buffers is the one of the first call -- the fp32 pair lives beside it --, and everything shares one copy stream."""
    src = str(tmp_path / "in.h5")
    st._write_rows(src, (12, 20, 5), (1.5, 0.9, 2.25), seed=11)
    net = predictor.prepare_network(12, 2, 2, 1)
    seen = []
    for phase, finish in enumerate(("1", "0", "1")):
        monkeypatch.setenv("FDN_DEVICE_FINISH", finish)
        for call in range(2):
            vols = predictor.predict_file(net, src, str(tmp_path / ("out_%d_%d.h5" % (phase, call))), 12, 2, batch_size=4, verbose=False,
                                          device_tiler=True, frames_per_group=1)
            assert len(vols) == 3
        state = net._predictor_state
        pair = state.pinned_buffers["groups", torch.float64]
        assert [tuple(b.shape) for b in pair] == [(1, 3, 24, 40, 10)] * 2 and all(b.is_pinned() for b in pair)
        seen.append(([b.data_ptr() for b in pair], state.stream))
    assert seen[2][0] == seen[0][0] and len(set(seen[0][0])) == 2
    assert [tuple(b.shape) for b in state.pinned_buffers["groups", torch.float32]] == [(1, 3, 24, 40, 10)] * 2
    streams = [v for v in vars(state).values() if isinstance(v, torch.cuda.Stream)]
    assert len(streams) == 1 and seen[0][1] is seen[2][1] is streams[0]
    assert not [name for name in vars(net) if name.startswith("_predict_")]      # no cache beside the state object


N_PATCHES, P, R = 5, 8, 2


def _stacks():
    rng = np.random.default_rng(5)
    return [rng.standard_normal((N_PATCHES, P, P, P, 1)).astype(np.float32) for _ in range(6)]


def _gloo_worker(rank, world, port, q):
    """Two ranks on ONE device over gloo, whatever the number of devices: the host-staged route of _send_rows / _recv_rows."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    parallel = importlib.import_module("4dflownet_amd.parallel")
    parallel.init_from_env(backend="gloo")
    pred = importlib.import_module("4dflownet_amd.predictor")
    net = pred.prepare_network(P, R, 1, 1)
    stacks = _stacks()
    res = [pred.predict_patches(net, [s[:n] for s in stacks[:3]], [s[:n] for s in stacks[3:]], 2) for n in (1, N_PATCHES)]
    torch.cuda.synchronize()
    parallel.barrier()
    q.put((rank, res, torch.distributed.get_backend(), sorted(str(name) for name in pred._state(net).pinned_buffers)))
    torch.distributed.destroy_process_group()


def test_gloo_with_a_network_on_the_device_and_an_empty_shard():
    """predict_patches on ONE patch -- shard_bounds(1, 2) == [0, 1, 1]: rank 1 owns nothing, neither sends nor is waited for -- and on five
    patches at batch 2: shards 3 + 2, a ragged last batch on both ranks.  Rank 0's array has the bytes of the single process; rank 1
    returns None, and all it pinned is the transport buffer its fp32 rows travelled through."""
    assert predictor.shard_bounds(1, 2) == [0, 1, 1] and predictor.shard_bounds(N_PATCHES, 2) == [0, 3, 5]
    res = st._run(_gloo_worker)
    assert res[0][2] == res[1][2] == "gloo"
    assert res[1][1] == [None, None] and res[1][3] == ["transport"] and res[0][3] == ["rows", "transport"]
    net = predictor.prepare_network(P, R, 1, 1)
    stacks = _stacks()
    for n, got in zip((1, N_PATCHES), res[0][1]):
        want = predictor.predict_patches(net, [s[:n] for s in stacks[:3]], [s[:n] for s in stacks[3:]], 2)
        assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (n, 16, 16, 16, 3)
        assert np.abs(want).max() > 0 and got.tobytes() == want.tobytes(), n

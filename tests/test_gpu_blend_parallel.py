"""Overlap-add stitching in a data-parallel run: two ranks, rank 1 sends the cores of its patches and rank 0 blends them with side 0 behind
its own batches -- ascending patch order, so the file has the bits of the single process (the spawn helpers of tests/test_gpu_shard_tiler.py)."""
import importlib
import os

import numpy as np
import pytest
import torch

import test_gpu_shard_tiler as st

pytestmark = pytest.mark.gpu

h5io = importlib.import_module("4dflownet_amd.h5io")
predictor = importlib.import_module("4dflownet_amd.predictor")

P, R, BLEND, BATCH, SHAPE = 8, 2, 1, 4, (9, 6, 5)


def _blend_worker(rank, world, port, q, outdir):
    parallel = st._init(rank, world, port)
    pred = importlib.import_module("4dflownet_amd.predictor")
    net = pred.prepare_network(P, R, 1, 1)
    vols = pred.predict_file(net, os.path.join(outdir, "two.h5"), os.path.join(outdir, "two_dp.h5"), P, R, batch_size=BATCH, verbose=False,
                             frames_per_group=2, blend=BLEND)
    torch.cuda.synchronize()
    parallel.barrier()
    q.put((rank, [tuple(np.asarray(v) for v in row) for row in vols], torch.distributed.get_backend()))
    torch.distributed.destroy_process_group()


def test_two_ranks_predict_file_with_blend_equals_the_single_process(tmp_path):
    """Two rows of (9,6,5) at patch 8, blend 1: 3x2x2 = 12 patches per row in one group, 24 split 12 + 12 -- rank 1 owns exactly row 1, whose
    cores rank 0 blends at patch 12 -- and the boundary is a multiple of the batch 4, so every batch holds what it holds in the single
    process."""
    st._write_rows(str(tmp_path / "two.h5"), SHAPE, (1.5, 0.9), seed=31)
    res = st._run(_blend_worker, extra=(str(tmp_path),))
    assert res[1][1] == []                                         # rank 1 sent its cores; it neither blends nor writes
    net = predictor.prepare_network(P, R, 1, 1)
    single = predictor.predict_file(net, str(tmp_path / "two.h5"), str(tmp_path / "two_single.h5"), P, R, batch_size=BATCH, verbose=False,
                                    frames_per_group=2, blend=BLEND)
    got = res[0][1]
    assert len(got) == len(single) == 2
    for va, vb in zip(got, single):
        for x, y in zip(va, vb):
            assert x.dtype == y.dtype == np.float64 and x.shape == y.shape == (1, 18, 12, 10)
            assert x.tobytes() == y.tobytes() and np.abs(y).max() > 0
    a, b = h5io.read_all(str(tmp_path / "two_dp.h5")), h5io.read_all(str(tmp_path / "two_single.h5"))
    assert sorted(a) == sorted(b) == ["dx", "u", "v", "w"]
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key
    plain = predictor.predict_file(net, str(tmp_path / "two.h5"), str(tmp_path / "two_plain.h5"), P, R, batch_size=BATCH, verbose=False,
                                   device_tiler=True, frames_per_group=2)
    assert plain[0][0].tobytes() != single[0][0].tobytes()        # the option reached the volume

"""The device tiler under data parallelism and its finish on the device:
  1. fdn_pack_patch_cores followed by a stitch with side 0 == the direct stitch (both pure copies: equal bits);
  2. fdn_stitch_patches_finish == the host finish of predict_file on the fp32 stitch (predictor.py:103-107, ImageDataset.py:31), as
     int64 bit patterns, the strict comparison pinned by elements forced onto the threshold, a zero threshold, untouched voxels;
  3. predict_cores over simulated shards, stitched and finished with side 0 == predict_volume(frame_scale=...);
  4. two real ranks through predict_file(device_tiler=True) == the single-process device tiler, file and volumes.

Shapes (P, R, LR shape, F): (8,2,(7,10,13),2) plans to 24 patches per frame with a cropped far pad on every axis; (8,2,(4,4,4),1) to 8, seven
of them wholly inside the crop; (12,3,(9,8,17),1) to 6 with S = 36, core 24 and a zero far pad on one axis."""
import importlib
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

fdn = importlib.import_module("4dflownet_amd")
ops = importlib.import_module("4dflownet_amd.ops")
tiler = importlib.import_module("4dflownet_amd.tiler")
h5io = importlib.import_module("4dflownet_amd.h5io")
predictor = importlib.import_module("4dflownet_amd.predictor")

CASES = [(8, 2, (7, 10, 13), 2), (8, 2, (4, 4, 4), 1), (12, 3, (9, 8, 17), 1)]
PER_FRAME = {(7, 10, 13): 24, (4, 4, 4): 8, (9, 8, 17): 6}
SENTINEL = 7.25e300                    # no product of an fp32 value and a venc


def _geometry(P, R, shape, F):
    counts, _, extents = tiler.PatchGenerator(P, R).plan(shape)
    n = counts[0] * counts[1] * counts[2]
    assert n == PER_FRAME[shape] and extents == tuple(R * s for s in shape)
    return counts, n, (F, 3) + extents


def _guarded(shape, dtype, fill, guard=1024):
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * guard,), fill, device="cuda", dtype=dtype)
    return buf, buf[guard:guard + numel].view(shape), guard, numel


def _stitch_chunks(pred, vol, side, counts, lo, hi, chunk, pack=False, frame_scale=None):
    """Patches [lo, hi) of pred (rows are GLOBAL patch numbers) in chunks of `chunk` with a ragged tail; chunk boundaries fall inside frames."""
    for g0 in range(lo, hi, chunk):
        part = pred[g0:min(g0 + chunk, hi)]
        if pack:
            ops.stitch_patches(ops.pack_patch_cores(part, side), vol, 0, counts, g0, frame_scale=frame_scale)
        else:
            ops.stitch_patches(part, vol, side, counts, g0, frame_scale=frame_scale)


@pytest.mark.parametrize("P,R,shape,F", CASES)
def test_pack_then_stitch_with_side_0_equals_the_direct_stitch(P, R, shape, F):
    counts, n, vshape = _geometry(P, R, shape, F)
    S, side = P * R, 2 * R
    c = S - 2 * side
    rng = np.random.default_rng(3 + P)
    pred = rng.standard_normal((F * n, S, S, S, 3)).astype(np.float32)
    dpred = torch.from_numpy(pred).cuda()
    assert (F * n) % 5 != 0 and n % 5 != 0                                  # a ragged tail, chunk starts off the frame boundary
    # the packed cores themselves: contiguous (count,c,c,c,3), out= honoured, nothing outside written
    buf, out, guard, numel = _guarded((F * n, c, c, c, 3), torch.float32, float("nan"))
    got = ops.pack_patch_cores(dpred, side, out=out)
    assert got.data_ptr() == out.data_ptr() and got.is_contiguous()
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(pred[:, side:S - side, side:S - side, side:S - side]).tobytes()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + numel:]).all())
    one = ops.pack_patch_cores(dpred[F * n - 1:], side)                       # out=None, the last patch alone
    assert tuple(one.shape) == (1, c, c, c, 3) and torch.equal(one[0], got[-1])
    # stitch(pack(pred), side 0) == stitch(pred, side)
    _, direct, _, _ = _guarded(vshape, torch.float32, float("nan"))
    _stitch_chunks(dpred, direct, side, counts, 0, F * n, 5)
    assert not bool(torch.isnan(direct).any())
    gbuf, packed, guard, numel = _guarded(vshape, torch.float32, float("nan"))
    _stitch_chunks(dpred, packed, side, counts, 0, F * n, 5, pack=True)
    assert np.array_equal(packed.cpu().numpy().view(np.int32), direct.cpu().numpy().view(np.int32))
    assert bool(torch.isnan(gbuf[:guard]).all()) and bool(torch.isnan(gbuf[guard + numel:]).all()), "a write outside the volume"


def _host_finish(stitched32, vencs, thresholds):
    """_predict_file_device.finish before this entry point: per frame `v = host.astype(float64) * venc; v[abs(v) < vpp] = 0`."""
    out = np.empty(stitched32.shape, np.float64)
    for f in range(stitched32.shape[0]):
        v = stitched32[f].astype(np.float64) * vencs[f]
        if thresholds[f] is not None:
            v[np.abs(v) < thresholds[f]] = 0
        out[f] = v
    return out


@pytest.mark.parametrize("P,R,shape,F", CASES)
def test_stitch_finish_equals_the_host_finish_bit_for_bit(P, R, shape, F):
    counts, n, vshape = _geometry(P, R, shape, F)
    S, side = P * R, 2 * R
    rng = np.random.default_rng(11 + P + F)
    pred = rng.uniform(-1e-3, 1e-3, (F * n, S, S, S, 3)).astype(np.float32)
    vencs = [np.float32(v) for v in ((1.5, 2.0) if F == 2 else (2.0,))]          # fp32 values, as ImageDataset leaves them
    thr = [v / 2048 for v in vencs]                                              # ImageDataset.py:31 (np.float32)
    fb = F - 1                                                                   # the frame with venc 2.0
    assert vencs[fb] == 2.0 and thr[fb].dtype == np.float32 and float(thr[fb]) == 2.0 ** -10
    # elements on the boundary, in patch (0,0,0) of that frame (its first core voxels are never cropped): p = 2^-11 gives a product
    # EQUAL to the threshold and is kept, the fp32 value just below it is zeroed; the same for their negatives
    edge = np.float32(2.0 ** -11)
    below = np.nextafter(edge, np.float32(0))
    assert below < edge and np.float64(below) * 2.0 < 2.0 ** -10
    g = fb * n
    pred[g, side, side, side, 0], pred[g, side, side, side, 1], pred[g, side, side, side, 2] = edge, below, -edge
    pred[g, side, side, side + 1, 0] = -below
    dpred = torch.from_numpy(pred).cuda()
    _, v32, _, _ = _guarded(vshape, torch.float32, float("nan"))
    _stitch_chunks(dpred, v32, side, counts, 0, F * n, 5)
    stitched32 = v32.cpu().numpy()
    assert not np.isnan(stitched32).any()
    want = _host_finish(stitched32, vencs, thr)
    assert want[fb, 0, 0, 0, 0] == 2.0 ** -10 and want[fb, 2, 0, 0, 0] == -(2.0 ** -10)
    assert want[fb, 1, 0, 0, 0] == 0 and want[fb, 0, 0, 0, 1] == 0
    zeroed = float((want == 0).mean())
    assert 0.35 < zeroed < 0.65, zeroed                                          # both branches run
    scale = torch.tensor([[float(v), float(t)] for v, t in zip(vencs, thr)], dtype=torch.float64).cuda()
    for pack in (False, True):                                                   # full patches with side 2R; packed cores with side 0
        buf, vol, guard, numel = _guarded(vshape, torch.float64, SENTINEL)
        _stitch_chunks(dpred, vol, side, counts, 0, F * n, 5, pack=pack, frame_scale=scale)
        got = vol.cpu().numpy()
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), pack     # bit patterns: zeroed voxels are +0.0
        assert not np.signbit(got[want == 0]).any()
        assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + numel:] == SENTINEL).all()), "a write outside the volume"
    # threshold 0 zeroes nothing (round_small_values=False)
    scale0 = torch.tensor([[float(v), 0.0] for v in vencs], dtype=torch.float64).cuda()
    _, vol, _, _ = _guarded(vshape, torch.float64, SENTINEL)
    _stitch_chunks(dpred, vol, side, counts, 0, F * n, 5, frame_scale=scale0)
    want0 = _host_finish(stitched32, vencs, [None] * F)
    assert np.array_equal(vol.cpu().numpy().view(np.int64), want0.view(np.int64))
    assert (want0 == 0).sum() == 0 and (want == 0).sum() > 0
    # a part of the patch list: what the other patches own keeps the sentinel written beforehand
    # ((4,4,4): patch 0 owns the whole frame and the seven others write nothing, so the range leaves patch 0 out)
    lo, hi = (1, F * n) if shape == (4, 4, 4) else (2, F * n - 3)
    _, part32, _, _ = _guarded(vshape, torch.float32, float("nan"))
    _stitch_chunks(dpred, part32, side, counts, lo, hi, 5)
    written = ~np.isnan(part32.cpu().numpy())
    assert not written.all() and bool(written.any()) == (shape != (4, 4, 4))
    _, vol, _, _ = _guarded(vshape, torch.float64, SENTINEL)
    _stitch_chunks(dpred, vol, side, counts, lo, hi, 5, frame_scale=scale)
    assert np.array_equal(vol.cpu().numpy().view(np.int64), np.where(written, want, SENTINEL).view(np.int64))


# ---- simulated shards in one process ----
SHAPE3, VENCS3 = (7, 10, 13), (1.5, 2.0, 0.9)
_shared = {}


def _net_frames_and_reference():
    """prepare_network(8,2,1,1), three random frames and predict_volume(frame_scale=...) at batch 4: computed once, left unchanged."""
    if not _shared:
        rng = np.random.default_rng(5)
        frames = np.concatenate([rng.uniform(-1, 1, (3, 3) + SHAPE3), rng.uniform(0, 0.07, (3, 3) + SHAPE3)], axis=1).astype(np.float32)
        net = predictor.prepare_network(8, 2, 1, 1)
        scale = [(np.float32(v), np.float32(v) / 2048) for v in VENCS3]
        ref = predictor.predict_volume(net, frames, 8, 4, frame_scale=scale)
        assert ref.dtype == torch.float64 and tuple(ref.shape) == (3, 3, 14, 20, 26)
        ref = ref.cpu().numpy()
        ref.setflags(write=False)
        _shared.update(net=net, frames=frames, scale=scale, ref=ref)
    return _shared["net"], _shared["frames"], _shared["scale"], _shared["ref"]


def test_predict_volume_with_frame_scale_equals_the_host_finish_of_the_fp32_volume():
    net, frames, scale, ref = _net_frames_and_reference()
    v32 = predictor.predict_volume(net, frames, 8, 4)
    assert v32.dtype == torch.float32
    want = _host_finish(v32.cpu().numpy(), [s[0] for s in scale], [s[1] for s in scale])
    assert np.array_equal(ref.view(np.int64), want.view(np.int64))
    # patch_range: the two halves into one output == the whole
    out = torch.full(ref.shape, SENTINEL, device="cuda", dtype=torch.float64)
    predictor.predict_volume(net, frames, 8, 4, out=out, frame_scale=scale, patch_range=(0, 36))
    half = out.cpu().numpy()
    assert (half == SENTINEL).any() and np.array_equal(half[0], ref[0])
    predictor.predict_volume(net, frames, 8, 4, out=out, frame_scale=scale, patch_range=(36, 72))
    assert np.array_equal(out.cpu().numpy().view(np.int64), ref.view(np.int64))


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_simulated_shards_equal_predict_volume(world):
    net, frames, scale, ref = _net_frames_and_reference()
    counts, n, vshape = _geometry(8, 2, SHAPE3, 3)
    bounds = predictor.shard_bounds(3 * n, world)
    dscale = torch.tensor([[float(v), float(t)] for v, t in scale], dtype=torch.float64).cuda()
    for batch in (4, 5):
        vol = torch.full(vshape, SENTINEL, device="cuda", dtype=torch.float64)
        for r in range(world):
            lo, hi = bounds[r], bounds[r + 1]
            if hi == lo:
                continue
            f0, f1 = predictor.shard_frame_span(lo, hi, n)
            cores = predictor.predict_cores(net, frames[f0:f1], 8, batch, lo, hi, first_frame=f0)     # only the frames the shard touches
            assert tuple(cores.shape) == (hi - lo, 8, 8, 8, 3) and cores.dtype == torch.float32 and cores.is_contiguous()
            ops.stitch_patches(cores, vol, 0, counts, lo, frame_scale=dscale)
        got = vol.cpu().numpy()
        assert not (got == SENTINEL).any()
        if batch == 4 and world in (1, 2, 3):                # shard boundaries 72, 36, 24: every batch holds the patches it holds in predict_volume
            assert all(b % 4 == 0 for b in bounds)
            assert np.array_equal(got.view(np.int64), ref.view(np.int64)), (world, batch)
        err = np.abs(got - ref).max()
        print("world %d batch %d: max |got - ref| = %.3e, max |ref| = %.3e" % (world, batch, err, np.abs(ref).max()))
        assert err <= 1e-5 * np.abs(ref).max(), (world, batch, err)      # the bound of test_dp2_predict_file_equals_single_process


# ---- two ranks ----
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


def _write_rows(path, shape, vencs, seed):
    rng = np.random.default_rng(seed)
    rows = len(vencs)
    tree = {"dx": np.full((rows, 3), 1.5, dtype=np.float32)}
    for n, scale in (("u", 1.0), ("v", 0.5), ("w", 0.75)):
        tree[n] = np.stack([rng.uniform(-v, v, shape) for v in vencs]).astype(np.float32)
        tree["venc_" + n] = (np.asarray(vencs) * scale).astype(np.float32)
        tree["mag_" + n] = rng.uniform(0, 300, (rows,) + shape).astype(np.float32)
    h5io.write_file(path, tree)


def _predict_worker(rank, world, port, q, outdir):
    parallel = _init(rank, world, port)
    pred = importlib.import_module("4dflownet_amd.predictor")
    net = pred.prepare_network(8, 2, 1, 1)
    res = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for name in ("three", "one"):
            vols = pred.predict_file(net, os.path.join(outdir, name + ".h5"), os.path.join(outdir, name + "_dp.h5"), 8, 2, batch_size=4,
                                     verbose=False, device_tiler=True, frames_per_group=3)
            res.append([tuple(np.asarray(v) for v in row) for row in vols])
    torch.cuda.synchronize()
    parallel.barrier()
    package = os.path.dirname(os.path.abspath(pred.__file__))
    q.put((rank, res, [str(w.message) for w in caught if (w.filename or "").startswith(package) or "tiler" in str(w.message)],
           torch.distributed.get_backend()))
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
                p.join(timeout=10)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return res


def test_two_ranks_predict_file_with_the_device_tiler_equals_the_single_process(tmp_path):
    """Three rows of (7,10,13) in one group: 72 patches split 36 + 36, rank 1 starts in the middle of frame 1 and loads rows 1 and 2 only; the
    boundary 36 is a multiple of the batch 4, so every batch holds what it holds in the single process.  One row of (4,4,4): 8 patches, 4 + 4
    (seven of them write nothing).  nccl with two GPUs, else both ranks on cuda:0 over gloo through pinned host memory."""
    _write_rows(str(tmp_path / "three.h5"), (7, 10, 13), (1.5, 0.9, 2.25), seed=21)
    _write_rows(str(tmp_path / "one.h5"), (4, 4, 4), (1.25,), seed=22)
    res = _run(_predict_worker, extra=(str(tmp_path),))
    assert res[1][1] == [[], []]                                   # rank 1 sent its cores; it neither stitches nor writes
    assert res[0][2] == [] and res[1][2] == [], (res[0][2], res[1][2])          # no warning, no fallback to the host tiler
    assert res[0][3] == ("nccl" if torch.cuda.device_count() >= 2 else "gloo")
    net = predictor.prepare_network(8, 2, 1, 1)
    for k, (name, rows, hr) in enumerate((("three", 3, (14, 20, 26)), ("one", 1, (8, 8, 8)))):
        single = predictor.predict_file(net, str(tmp_path / (name + ".h5")), str(tmp_path / (name + "_single.h5")), 8, 2, batch_size=4,
                                        verbose=False, device_tiler=True, frames_per_group=3)
        got = res[0][1][k]
        assert len(got) == len(single) == rows
        for va, vb in zip(got, single):
            for x, y in zip(va, vb):
                assert x.dtype == y.dtype == np.float64 and x.shape == y.shape == (1,) + hr
                assert np.array_equal(x.view(np.int64), y.view(np.int64))
                assert np.abs(y).max() > 0
        a, b = h5io.read_all(str(tmp_path / (name + "_dp.h5"))), h5io.read_all(str(tmp_path / (name + "_single.h5")))
        assert sorted(a) == sorted(b) == ["dx", "u", "v", "w"]
        for key in a:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (name, key)

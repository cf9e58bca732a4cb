"""Sliding-window inference with the tiler on the device == the host tiler (tiler.PatchGenerator, the oracle-checked yardstick), bit for bit:
fdn_input_features_volume against patchify + fdn_input_features, fdn_stitch_patches against _patchup_with_overlap, predict_file with the
device tiler against the host path, and the old entry points of the two shared kernels against a recorded run of the previous library.

Which single-line change of the index rules makes which case fail (each rule with that one change was run in numpy against the host
tiler on these cases; the stitch ones without the 24^3 case):
  source coordinate without `- 2`             -> every patchify case, every sub-case;
  stride P instead of E = P - 4               -> every patchify case, every sub-case;
  i fastest instead of k fastest              -> every patchify case in the all-patches and the frame-crossing sub-case (the last patch is the
                                                 last patch in either order); every stitch case but (4,4,4), where only patch 0 of a frame writes;
  frame from g / nx instead of g / (nx*ny*nz) -> every patchify case in the all-patches and the frame-crossing sub-case;
  no zero outside the volume                  -> every patchify case, every sub-case (values of the neighbouring row / plane / channel appear);
  core offset `side` dropped in the stitch    -> every stitch case;
  destination i*S instead of i*core           -> every stitch case but (4,4,4) (only patch (0,0,0) of a frame writes there);
  the extent test dropped in the stitch       -> every stitch case: cropped voxels overwrite their neighbours or the NaN guard regions, and
                                                 (4,4,4), whose seven far patches per frame lie wholly in the crop, is overwritten whole."""
import importlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")
RECORDED = os.path.join(HERE, "golden", "device_tiler_old_entry_points.npz")

fdn = importlib.import_module("4dflownet_amd")
ops = importlib.import_module("4dflownet_amd.ops")
ops_bf16 = importlib.import_module("4dflownet_amd.ops_bf16")
tiler = importlib.import_module("4dflownet_amd.tiler")
data = importlib.import_module("4dflownet_amd.data")
ddev = importlib.import_module("4dflownet_amd.data_device")
h5io = importlib.import_module("4dflownet_amd.h5io")
predictor = importlib.import_module("4dflownet_amd.predictor")

CASES = [(8, 2, (7, 10, 13)), (12, 3, (9, 8, 17)), (24, 2, (42, 38, 36)), (8, 2, (4, 4, 4)), (12, 2, (12, 20, 5))]
F = 2
NAMES = ("u", "v", "w", "mag_u", "mag_v", "mag_w")


class _Vol:
    pass


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


_frames_cache = {}


def _frames_and_host_patches(P, R, shape):
    """Random frames (F,6,X,Y,Z) and what the host tiler makes of them: six stacks (F*n,P,P,P,1), frame after frame.  Computed once per case."""
    key = (P, R, shape)
    if key not in _frames_cache:
        rng = np.random.default_rng(1000 * P + shape[0])
        frames = rng.standard_normal((F, 6) + shape).astype(np.float32)
        pg = tiler.PatchGenerator(P, R)
        per_frame = []
        for f in range(F):
            v = _Vol()
            for c, n in enumerate(NAMES):
                setattr(v, n, frames[f, c])
            vel, mag = pg.patchify(v)
            per_frame.append(list(vel) + list(mag))
        stacks = [np.concatenate([pf[c] for pf in per_frame], axis=0) for c in range(6)]
        for s in stacks:
            s.setflags(write=False)
        frames.setflags(write=False)
        _frames_cache[key] = (frames, stacks, (pg.nr_x, pg.nr_y, pg.nr_z), pg.padding)
    return _frames_cache[key]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("P,R,shape", CASES)
def test_input_features_volume_equals_patchify_then_input_features(P, R, shape, dtype):
    frames, stacks, counts, _ = _frames_and_host_patches(P, R, shape)
    assert tiler.PatchGenerator(P, R).plan(shape)[0] == counts
    o = ops if dtype == "float32" else ops_bf16
    n = counts[0] * counts[1] * counts[2]
    dframes = torch.from_numpy(frames).cuda()
    dstacks = [torch.from_numpy(s).cuda() for s in stacks]
    ref_phase, ref_pc = o.input_features(*dstacks)
    assert tuple(ref_phase.shape) == (F * n, P, P, P, 3)
    # all patches; from the middle of frame 0 across the frame boundary; the last patch alone
    for g0, count in ((0, F * n), (n // 2, n), (F * n - 1, 1)):
        assert g0 + count <= F * n
        phase, pc = o.input_features_volume(dframes, P, counts, g0, count)
        assert tuple(phase.shape) == tuple(pc.shape) == (count, P, P, P, 3) and phase.dtype == ref_phase.dtype
        assert np.array_equal(_bits(phase), _bits(ref_phase[g0:g0 + count])), (g0, count, "phase")
        assert np.array_equal(_bits(pc), _bits(ref_pc[g0:g0 + count])), (g0, count, "pc")
    # count=None: everything from g0 on
    phase, _ = o.input_features_volume(dframes, P, counts, n + 1)
    assert phase.shape[0] == n - 1 and np.array_equal(_bits(phase), _bits(ref_phase[n + 1:]))


@pytest.mark.parametrize("P,R,shape", CASES)
def test_stitch_patches_equals_patchup_with_overlap(P, R, shape):
    _, _, counts, padding = _frames_and_host_patches(P, R, shape)
    n = counts[0] * counts[1] * counts[2]
    S, side = P * R, 2 * R
    extents = tuple(R * s for s in shape)
    rng = np.random.default_rng(7)
    pred = rng.standard_normal((F * n, S, S, S, 3)).astype(np.float32)
    pg = tiler.PatchGenerator(P, R)
    pg.padding = padding
    ref = np.stack([np.stack([pg._patchup_with_overlap(pred[f * n:(f + 1) * n, :, :, :, c], *counts) for c in range(3)]) for f in range(F)])
    assert ref.shape == (F, 3) + extents
    if shape == (4, 4, 4):                                     # the far patches lie wholly in the cropped region
        assert counts == (2, 2, 2) and extents == (8, 8, 8) and S - 2 * side == 8
    if P == 24:                                                # more elements than the 4096 x 256 grid covers in one pass
        assert F * n * (S - 2 * side) ** 3 * 3 > 4096 * 256
    dpred = torch.from_numpy(pred).cuda()
    numel, guard = int(np.prod(ref.shape)), 1024
    for chunk in (1, 5, F * n):
        buf = torch.full((numel + 2 * guard,), float("nan"), device="cuda")
        vol = buf[guard:guard + numel].view(ref.shape)
        for g0 in range(0, F * n, chunk):
            ops.stitch_patches(dpred[g0:g0 + chunk], vol, side, counts, g0)
        got = vol.cpu().numpy()
        assert not np.isnan(got).any(), "chunk %d: %d voxels unwritten" % (chunk, int(np.isnan(got).sum()))
        assert got.tobytes() == ref.tobytes(), "chunk %d" % chunk
        assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + numel:]).all()), "chunk %d: a write outside the volume" % chunk


def _write_rows(path, shape, vencs, seed):
    rng = np.random.default_rng(seed)
    rows = len(vencs)
    tree = {"dx": np.full((rows, 3), 1.5, dtype=np.float32)}
    for n, scale in (("u", 1.0), ("v", 0.5), ("w", 0.75)):
        tree[n] = np.stack([rng.uniform(-v, v, shape) for v in vencs]).astype(np.float32)
        tree["venc_" + n] = (np.asarray(vencs) * scale).astype(np.float32)
        tree["mag_" + n] = rng.uniform(0, 300, (rows,) + shape).astype(np.float32)
    h5io.write_file(path, tree)


def _same_volumes(a, b):
    assert len(a) == len(b)
    for va, vb in zip(a, b):
        for x, y in zip(va, vb):
            assert x.dtype == y.dtype == np.float64 and x.shape == y.shape
            assert x.tobytes() == y.tobytes()


def test_predict_file_with_the_device_tiler_equals_the_host_path_on_the_same_batches(tmp_path):
    """Three frames of LR shape (12,20,5) -- 6 patches each, another venc per row -- at patch 12, batch 4, ONE group: the batches are
    patches 0-3, 4-7 (frames 0 and 1), 8-11, 12-15 (frames 1 and 2), 16-17.  The host path fed the same composition: predict_patches on
    the three frames' stacks concatenated, then the per-frame stitch, de-normalisation and zeroing of predict_file."""
    P, R, B, shape, vencs = 12, 2, 4, (12, 20, 5), (1.5, 0.9, 2.25)
    src = str(tmp_path / "in.h5")
    _write_rows(src, shape, vencs, seed=11)
    net = predictor.prepare_network(P, R, 2, 1)
    ds = data.ImageDataset()
    pg = tiler.PatchGenerator(P, R)
    stacks, meta = [], []
    for row in range(3):
        ds.load_vectorfield(src, row)
        vel, mag = pg.patchify(ds)
        stacks.append(list(vel) + list(mag))
        meta.append((ds.venc, ds.velocity_per_px))
    assert (pg.nr_x, pg.nr_y, pg.nr_z) == (2, 3, 1) and len(set(float(m[0]) for m in meta)) == 3
    cat = [np.concatenate([s[c] for s in stacks], axis=0) for c in range(6)]
    res = predictor.predict_patches(net, cat[:3], cat[3:], B)
    assert res.shape == (18, 24, 24, 24, 3) and res.dtype == np.float64
    want = []
    for row, (venc, vpp) in enumerate(meta):
        vols = []
        for i in range(3):
            v = pg._patchup_with_overlap(res[6 * row:6 * row + 6, :, :, :, i], 2, 3, 1)
            v = v * venc
            v[np.abs(v) < vpp] = 0
            vols.append(np.expand_dims(v, axis=0))
        want.append(tuple(vols))
    assert want[0][0].shape == (1, 24, 40, 10)
    out = str(tmp_path / "device" / "out.h5")
    got = predictor.predict_file(net, src, out, P, R, batch_size=B, verbose=False, device_tiler=True, frames_per_group=3)
    _same_volumes(got, want)
    back = h5io.read_all(out)
    for i, n in enumerate(("u", "v", "w")):
        assert back[n].shape == (3, 24, 40, 10) and back[n].dtype == np.float32
        assert back[n].tobytes() == np.concatenate([w[i] for w in want]).astype(np.float32).tobytes()
    assert back["dx"].shape == (3, 3) and np.array_equal(back["dx"], np.full((3, 3), 0.75, np.float32))
    # the byte budget puts these three small frames into one group as well
    got2 = predictor.predict_file(net, src, str(tmp_path / "budget.h5"), P, R, batch_size=B, verbose=False, device_tiler=True)
    _same_volumes(got2, want)
    # one frame per group (three groups: both staging buffers are reused) == the host path, whose batches are then the same 4 + 2 per row;
    # the switch by the environment
    host = predictor.predict_file(net, src, str(tmp_path / "host.h5"), P, R, batch_size=B, verbose=False)
    os.environ["FDN_DEVICE_TILER"] = "1"
    try:
        got3 = predictor.predict_file(net, src, str(tmp_path / "env.h5"), P, R, batch_size=B, verbose=False, frames_per_group=1)
    finally:
        del os.environ["FDN_DEVICE_TILER"]
    assert tuple(net._predictor_state.pinned_buffers["groups", torch.float64][0].shape) == (1, 3, 24, 40, 10)   # the device path ran
    _same_volumes(got3, host)
    a, b = h5io.read_all(str(tmp_path / "env.h5")), h5io.read_all(str(tmp_path / "host.h5"))
    assert sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


def test_predict_volume_returns_the_stitched_device_tensor():
    P, R, shape = 12, 2, (12, 20, 5)
    frames, stacks, counts, padding = _frames_and_host_patches(P, R, shape)
    net = predictor.prepare_network(P, R, 1, 1)
    vol = predictor.predict_volume(net, frames, P, 5)                  # 12 patches as 5 + 5 + 2
    assert vol.is_cuda and vol.dtype == torch.float32 and tuple(vol.shape) == (F, 3, 24, 40, 10)
    pg = tiler.PatchGenerator(P, R)
    pg.padding = padding
    for g0, cnt in ((0, 5), (5, 5), (10, 2)):                          # the same batches through forward()
        pred = net.forward([s[g0:g0 + cnt] for s in stacks]).cpu().numpy()
        for b in range(cnt):
            f, r = divmod(g0 + b, 6)
            i, rem = divmod(r, counts[1] * counts[2])
            j, k = divmod(rem, counts[2])
            core = pred[b, 4:-4, 4:-4, 4:-4]
            x0, y0, z0 = i * 16, j * 16, k * 16
            want = core[:max(0, min(16, 24 - x0)), :max(0, min(16, 40 - y0)), :max(0, min(16, 10 - z0))]
            got = vol[f, :, x0:x0 + 16, y0:y0 + 16, z0:z0 + 16].permute(1, 2, 3, 0).cpu().numpy()
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (g0, b)


def test_example_volume_with_the_device_tiler_equals_the_host_path(tmp_path):
    """example_data.h5 at patch 24, batch 8, one frame per group: shape (84,76,72), all three components, returned volumes and file."""
    net = predictor.prepare_network(24, 2, 2, 1)
    src = os.path.join(DATA, "example_data.h5")
    host = predictor.predict_file(net, src, str(tmp_path / "host.h5"), 24, 2, batch_size=8, verbose=False)
    dev = predictor.predict_file(net, src, str(tmp_path / "dev.h5"), 24, 2, batch_size=8, verbose=False, device_tiler=True, frames_per_group=1)
    assert len(host) == 1 and host[0][0].shape == (1, 84, 76, 72)
    _same_volumes(dev, host)
    a, b = h5io.read_all(str(tmp_path / "dev.h5")), h5io.read_all(str(tmp_path / "host.h5"))
    assert sorted(a) == sorted(b) == ["dx", "u", "v", "w"]
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ---- the old entry points of the two shared kernels: a tripwire against a recorded run of the library before the device tiler ----
def run_old_entry_points(lib):
    """fdn_input_features (fp32 and bf16) and fdn_gather_patches on fixed small inputs through `lib` (a ctypes library with the prototypes
    of _lib.SIGNATURES attached).  Returns {name: numpy array of raw bits}."""
    rng = np.random.default_rng(2024)
    nvox = 2 * 5 * 6 * 7
    ins = [torch.from_numpy(rng.standard_normal(nvox).astype(np.float32)).cuda() for _ in range(6)]
    ins[0][3] = 0.0; ins[1][3] = 0.0; ins[2][3] = 0.0                  # a zero velocity: speed +0
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, fn, dt in (("f32", lib.fdn_input_features, torch.float32), ("bf16", lib.fdn_input_features_bf16, torch.bfloat16)):
        phase = torch.zeros((nvox, 3), device="cuda", dtype=dt)
        pc = torch.zeros((nvox, 3), device="cuda", dtype=dt)
        assert fn(*[t.data_ptr() for t in ins], phase.data_ptr(), pc.data_ptr(), nvox, stream) == 0
        out["features_%s_phase" % name], out["features_%s_pc" % name] = _bits(phase), _bits(pc)
    T, X, Y, Z, S = 2, 9, 8, 7, 5
    vol = torch.from_numpy(rng.uniform(-2, 2, (T, X, Y, Z)).astype(np.float32)).cuda()
    desc = np.zeros(6, ddev.DESC_DTYPE)
    #            t  x0 y0 z0 plane k mode sign  div
    rows = [(0, 0, 0, 0, 0, 0, 0, 1.0, 1.5), (1, 4, 3, 2, 1, 1, 0, -1.0, 0.7), (0, 2, 1, 0, 2, 2, 0, 1.0, 4095.0),
            (1, 1, 3, 2, 3, 3, 0, -1.0, 2.0), (0, 3, 2, 1, 1, 3, 1, 1.0, 0.25), (1, 4, 0, 2, 0, 0, 1, 1.0, -0.5)]
    for b, (t, x0, y0, z0, plane, k, mode, sign, div) in enumerate(rows):
        desc[b] = (vol.data_ptr(), X, Y, Z, t, x0, y0, z0, plane, k, mode, sign, div)
    table = torch.from_numpy(desc.view(np.uint8)).cuda()
    got = torch.zeros((6, S, S, S), device="cuda")
    assert lib.fdn_gather_patches(table.data_ptr(), got.data_ptr(), 6, S, stream) == 0
    torch.cuda.synchronize()
    out["gather"] = _bits(got)
    return out


def test_old_entry_points_of_the_shared_kernels_equal_the_recorded_run():
    want = np.load(RECORDED)
    got = run_old_entry_points(fdn._lib.load())
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape and np.array_equal(want[k], got[k]), k

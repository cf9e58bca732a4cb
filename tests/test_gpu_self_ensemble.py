"""Geometric self-ensemble on the device, bit for bit (the sign of zero counts; tests/_self_ensemble.py holds the numpy restatement):
  1. oriented window features == host patchify -> data.rotate_vector_field -> ops.input_features, all ten orientations, fp32 and bf16;
  2. fdn_unrotate_accumulate == numpy float32 (store, add, divide; -0.0, infinities, 2^+-40; past the grid cap);
  3. predict_volume(self_ensemble=) == the composed path from public pieces with the same batch boundaries: host patches rotated,
     network.forward, numpy inverse, fp32 sum in list order, fp32 divide, _patchup_with_overlap -- as the fp32 volume and finished;
  4. predict_cores over a shard, and predict_file / evaluate_file on a two-row file;
  5. one bf16-network run of 3.
Every reference is computed once and shared."""
import importlib
import os

import numpy as np
import pytest
import torch

import _self_ensemble as se

pytestmark = pytest.mark.gpu

ops = importlib.import_module("4dflownet_amd.ops")
ops_bf16 = importlib.import_module("4dflownet_amd.ops_bf16")
tiler = importlib.import_module("4dflownet_amd.tiler")
data = importlib.import_module("4dflownet_amd.data")
h5io = importlib.import_module("4dflownet_amd.h5io")
predictor = importlib.import_module("4dflownet_amd.predictor")

F, SHAPE = 2, (9, 6, 5)
NAMES = ("u", "v", "w", "mag_u", "mag_v", "mag_w")
SUBSET = [(0, 0), (2, 3), (1, 2)]
P_NET, R, BATCH = 8, 2, 5


class _Vol:
    pass


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


_cache = {}


def _frames():
    if "frames" not in _cache:
        frames = np.random.default_rng(77).standard_normal((F, 6) + SHAPE).astype(np.float32)
        frames.setflags(write=False)
        _cache["frames"] = frames
    return _cache["frames"]


def _host_patches(frames, P):
    """What the host tiler makes of frames (F,6,X,Y,Z): six stacks (F*n,P,P,P), frame after frame; the patch counts; the padding."""
    key = ("patches", P, frames.tobytes())
    if key not in _cache:
        pg = tiler.PatchGenerator(P, R)
        per_frame = []
        for f in range(frames.shape[0]):
            v = _Vol()
            for c, n in enumerate(NAMES):
                setattr(v, n, frames[f, c])
            vel, mag = pg.patchify(v)
            per_frame.append(list(vel) + list(mag))
        stacks = [np.concatenate([pf[c] for pf in per_frame], axis=0)[..., 0] for c in range(6)]
        for s in stacks:
            s.setflags(write=False)
        _cache[key] = (stacks, (pg.nr_x, pg.nr_y, pg.nr_z), pg.padding)
    return _cache[key]


def _rotated(stacks, orientation):
    """Every host patch through data.rotate_vector_field (the velocities signed, the magnitudes not): six stacks again."""
    plane, k = orientation
    n = stacks[0].shape[0]
    vel = [data.rotate_vector_field([stacks[c][b] for c in range(3)], k, plane, True) for b in range(n)]
    mag = [data.rotate_vector_field([stacks[3 + c][b] for c in range(3)], k, plane, False) for b in range(n)]
    return ([np.ascontiguousarray(np.stack([vel[b][c] for b in range(n)])) for c in range(3)] +
            [np.ascontiguousarray(np.stack([mag[b][c] for b in range(n)])) for c in range(3)])


# ---- 1. oriented features ----
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_oriented_features_equal_host_patches_rotated_then_input_features(dtype):
    P = 6
    frames = _frames()
    stacks, counts, _ = _host_patches(frames, P)
    assert counts == tiler.PatchGenerator(P, 2).plan(SHAPE)[0]
    n = counts[0] * counts[1] * counts[2]
    assert n > 7 and stacks[0].shape == (F * n, P, P, P)
    o = ops if dtype == "float32" else ops_bf16
    dframes = torch.from_numpy(frames).cuda()
    plain = None
    # all patches; g0 = 3, count = 4; and, the frame boundary lying at patch n > 7, the nearest range of four that crosses it
    ranges = ((0, F * n), (3, 4), (n - 3, 4))
    assert ranges[2][0] < n < ranges[2][0] + 4
    for orientation in se.ROT90:
        ref_phase, ref_pc = o.input_features(*[torch.from_numpy(s).cuda() for s in _rotated(stacks, orientation)])
        if orientation == (0, 0):
            plain = o.input_features_volume(dframes, P, counts)                     # no keyword: the existing path
        for g0, count in ranges:
            phase, pc = o.input_features_volume(dframes, P, counts, g0, count, orientation=orientation)
            assert tuple(phase.shape) == tuple(pc.shape) == (count, P, P, P, 3) and phase.dtype == pc.dtype == ref_phase.dtype
            assert np.array_equal(_bits(phase), _bits(ref_phase[g0:g0 + count])), (orientation, g0, count, "phase")
            assert np.array_equal(_bits(pc), _bits(ref_pc[g0:g0 + count])), (orientation, g0, count, "pc")
            if orientation == (0, 0) and g0 == 0:
                assert np.array_equal(_bits(phase), _bits(plain[0])) and np.array_equal(_bits(pc), _bits(plain[1]))
        if orientation != (0, 0):
            # the window is padded with zeros: under a negative sign they are -0.0, and the comparison above saw them
            neg = [i for i in range(3) if se.TABLE[orientation][1][i] < 0]
            ph = ref_phase.float().cpu().numpy()
            assert any(np.signbit(ph[..., i][ph[..., i] == 0]).any() for i in neg), orientation
            assert not np.array_equal(_bits(ref_phase), _bits(plain[0]))


# ---- 2. accumulate ----
def _operand(rng, shape):
    a = rng.standard_normal(shape).astype(np.float32)
    flat = a.reshape(-1)
    idx = rng.permutation(flat.size)[:60]
    special = np.float32([0.0, -0.0, np.inf, -np.inf, 2.0 ** 40, -2.0 ** 41, 2.0 ** -40, -2.0 ** -42, 3.0 * 2.0 ** 40, 2.0 ** 100])
    flat[idx] = np.tile(special, 6)
    return a


def _same_metrics(a, b):
    return len(a) == len(b) and all(list(x) == list(y) and all(x[k] == y[k] or (np.isnan(x[k]) and np.isnan(y[k])) for k in x)
                                    for x, y in zip(a, b))


def _acc_call(pred, acc, orientation, first, divisor=1):
    d = torch.from_numpy(acc).cuda()
    got = ops.unrotate_accumulate(torch.from_numpy(pred).cuda(), d, orientation, first, divisor)
    assert got is d
    return d.cpu().numpy()


def test_unrotate_accumulate_equals_numpy_float32():
    rng = np.random.default_rng(21)
    shape = (3, 6, 6, 6, 3)
    pred, acc = _operand(rng, shape), _operand(rng, shape)
    pred[2], acc[2] = np.inf, -np.inf              # the last patch: inf - inf where the sign rule keeps +inf, -inf where it flips it
    junk = np.full(shape, np.nan, np.float32)
    for orientation in se.ROT90:
        got = _acc_call(pred, junk, orientation, True)                      # first: the accumulator is not read
        assert se.same_bits(got, se.accumulate(pred, None, orientation, True)), orientation
        assert not np.isnan(got).any()
        got = _acc_call(pred, acc, orientation, False)
        want = se.accumulate(pred, acc, orientation, False)
        assert se.same_bits(got, want), orientation
        assert np.isnan(want).any() and np.isinf(want).any()               # inf - inf and inf + finite both occur
        got = _acc_call(pred, acc, orientation, False, 10)
        assert se.same_bits(got, se.accumulate(pred, acc, orientation, False, 10)), orientation
        got = _acc_call(pred, junk, orientation, True, 10)                  # a one-call ensemble would divide as well
        assert se.same_bits(got, se.accumulate(pred, None, orientation, True, 10)), orientation
    # the identity with first = 1, divisor = 1 is a copy
    assert np.array_equal(_acc_call(pred, junk, (0, 0), True).view(np.int32), pred.view(np.int32))
    assert np.array_equal(_acc_call(pred, junk, None, True).view(np.int32), pred.view(np.int32))


def test_three_orientations_with_an_inexact_quotient():
    rng = np.random.default_rng(22)
    shape = (3, 6, 6, 6, 3)
    preds = [rng.standard_normal(shape).astype(np.float32) for _ in SUBSET]
    preds[1].reshape(-1)[:7] = np.float32([0.0, -0.0, 2.0 ** 40, 2.0 ** -40, 1.0, 1e-30, -5.0])
    acc = torch.full(shape, float("nan"), device="cuda")
    for j, (p, o) in enumerate(zip(preds, SUBSET)):
        ops.unrotate_accumulate(torch.from_numpy(p).cuda(), acc, o, j == 0, 3 if j == 2 else 1)
    want = se.mean(preds, SUBSET)
    assert se.same_bits(acc.cpu().numpy(), want)
    s = (se.inverse(preds[0], SUBSET[0], 1) + se.inverse(preds[1], SUBSET[1], 1)).astype(np.float32) + se.inverse(preds[2], SUBSET[2], 1)
    assert (want.astype(np.float64) * 3 != s.astype(np.float64)).any()     # the quotient was rounded somewhere


def test_unrotate_accumulate_past_the_grid_cap():
    shape = (4, 48, 48, 48, 3)
    assert int(np.prod(shape)) == 1327104 > 4096 * 256
    rng = np.random.default_rng(23)
    pred, acc = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    guard = 4096
    buf = torch.full((pred.size + 2 * guard,), float("nan"), device="cuda")
    dacc = buf[guard:guard + pred.size].view(shape)
    dacc.copy_(torch.from_numpy(acc))
    ops.unrotate_accumulate(torch.from_numpy(pred).cuda(), dacc, (3, 1), False, 3)
    assert se.same_bits(dacc.cpu().numpy(), se.accumulate(pred, acc, (3, 1), False, 3))
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + pred.size:]).all()), "a write outside the accumulator"


# ---- 3 - 5. the predictor ----
def _net(dtype="float32"):
    key = ("net", dtype)
    if key not in _cache:
        _cache[key] = predictor.prepare_network(P_NET, R, 1, 1, dtype=dtype)
    return _cache[key]


def _reference(frames, orientations, dtype="float32", tag=None):
    """The composed path over frames (F,6,X,Y,Z): per batch of BATCH consecutive global patches and per orientation the host patches
    rotated, network.forward, the numpy inverse; the fp32 sum in list order and one fp32 divide.  Returns the mean patches
    (F*n,S,S,S,3) fp32 and the stitched volume (F,3,X*R,Y*R,Z*R) fp32 (_patchup_with_overlap per frame and component)."""
    key = ("ref", tag or frames.tobytes(), tuple(orientations), dtype)
    if key not in _cache:
        net = _net(dtype)
        stacks, counts, padding = _host_patches(frames, P_NET)
        n = counts[0] * counts[1] * counts[2]
        total = frames.shape[0] * n
        rotated = [_rotated(stacks, o) for o in orientations]
        patches = np.empty((total, P_NET * R, P_NET * R, P_NET * R, 3), np.float32)
        for g0 in range(0, total, BATCH):
            e = min(g0 + BATCH, total)
            preds = [net.forward([s[g0:e] for s in rot]).cpu().numpy() for rot in rotated]
            patches[g0:e] = se.mean(preds, orientations)
        pg = tiler.PatchGenerator(P_NET, R)
        pg.padding = padding
        vol = np.stack([np.stack([pg._patchup_with_overlap(patches[f * n:(f + 1) * n, ..., c], *counts) for c in range(3)])
                        for f in range(frames.shape[0])]).astype(np.float32)
        patches.setflags(write=False)
        vol.setflags(write=False)
        _cache[key] = (patches, vol, counts)
    return _cache[key]


def _finish(vol, scale):
    """predictor.py's post-processing on a stitched fp32 volume (F,3,...): * venc in float64, +0.0 below the threshold."""
    out = np.empty(vol.shape, np.float64)
    for f, (venc, thr) in enumerate(scale):
        v = vol[f].astype(np.float64) * venc
        v[np.abs(v) < thr] = 0
        out[f] = v
    return out


@pytest.mark.parametrize("which", ["rot90", "subset"])
def test_predict_volume_equals_the_composed_path_on_the_same_batches(which):
    option = "rot90" if which == "rot90" else SUBSET
    orientations = se.ROT90 if which == "rot90" else SUBSET
    frames = _frames()
    _, want, counts = _reference(frames, orientations)
    assert counts == (3, 2, 2) and F * 12 % BATCH != 0 and 12 % BATCH != 0          # ragged; batches span the frames
    net = _net()
    vol = predictor.predict_volume(net, frames, P_NET, BATCH, self_ensemble=option)
    assert vol.dtype == torch.float32 and tuple(vol.shape) == want.shape == (F, 3, 18, 12, 10)
    assert se.same_bits(vol.cpu().numpy(), want)
    assert np.abs(want).max() > 0 and not np.isnan(want).any()
    held = net._predictor_state.device_buffers
    assert tuple(held["ensemble"][0].shape) == (BATCH, 16, 16, 16, 3)               # one accumulator, kept on the network
    kept = held["ensemble"][0].data_ptr()
    # finished: thresholds at the medians of the de-normalised frames zero about half of the voxels
    vencs = (1.5, 0.75)
    scale = [(v, float(np.median(np.abs(want[f].astype(np.float64) * v)))) for f, v in enumerate(vencs)]
    fin_want = _finish(want, scale)
    zeroed = (fin_want == 0).mean()
    assert 0.3 < zeroed < 0.7, zeroed
    fin = predictor.predict_volume(net, frames, P_NET, BATCH, frame_scale=scale, self_ensemble=option)
    assert fin.dtype == torch.float64 and se.same_bits(fin.cpu().numpy(), fin_want)
    assert held["ensemble"][0].data_ptr() == kept
    if which == "subset":                                                           # the ensemble is not the plain prediction
        plain = predictor.predict_volume(net, frames, P_NET, BATCH)
        assert not se.same_bits(plain.cpu().numpy(), want)


def test_identity_alone_and_off_take_the_plain_path():
    frames = _frames()
    net = _net()
    predictor._state(net).device_buffers.pop("ensemble", None)
    plain = predictor.predict_volume(net, frames, P_NET, BATCH).cpu().numpy()
    for option in (None, False, [(0, 0)], ((0, 0),)):
        got = predictor.predict_volume(net, frames, P_NET, BATCH, self_ensemble=option)
        assert se.same_bits(got.cpu().numpy(), plain), option
    assert "ensemble" not in predictor._state(net).device_buffers                   # no accumulator: the plain loop ran
    _, want, _ = _reference(frames, [(0, 0)])                                       # and the composed path with one orientation agrees
    assert se.same_bits(plain, want)
    with pytest.raises(ValueError, match="self_ensemble"):
        predictor.predict_volume(net, frames, P_NET, BATCH, self_ensemble="rot180")
    with pytest.raises(ValueError, match="self_ensemble"):
        predictor.predict_cores(net, frames, P_NET, BATCH, 0, 4, self_ensemble=[(0, 1)])


def test_predict_cores_over_a_shard_equals_the_same_patches():
    """Patches [7, 21) in batches of 5 from 7: other batch boundaries than case 3's, so the reference is the mean PATCHES of case 3 only
    where a patch's value does not depend on its batch -- it does not: every patch of a batch is computed on its own."""
    frames = _frames()
    patches, _, counts = _reference(frames, se.ROT90)
    lo, hi = 7, 21
    net = _net()
    cores = predictor.predict_cores(net, frames, P_NET, BATCH, lo, hi, self_ensemble="rot90")
    assert tuple(cores.shape) == (hi - lo, 8, 8, 8, 3)
    want = patches[lo:hi, 4:-4, 4:-4, 4:-4]
    assert se.same_bits(cores.cpu().numpy(), np.ascontiguousarray(want))
    # stitched with side 0 at g0 = lo: the voxels of those patches in case 3's volume, the rest untouched
    _, vol_want, _ = _reference(frames, se.ROT90)
    vol = torch.full((F, 3, 18, 12, 10), float("nan"), device="cuda")
    ops.stitch_patches(cores, vol, 0, counts, lo)
    got = vol.cpu().numpy()
    written = ~np.isnan(got)
    only = torch.full((F, 3, 18, 12, 10), float("nan"), device="cuda")
    ops.stitch_patches(torch.from_numpy(np.ascontiguousarray(patches[lo:hi])).cuda(), only, 4, counts, lo)
    assert np.array_equal(written, ~np.isnan(only.cpu().numpy())) and written.any() and not written.all()
    assert se.same_bits(got[written], vol_want[written])
    # frames cut to the shard's span, as a data-parallel peer loads them
    f0, f1 = predictor.shard_frame_span(13, 21, 12)
    assert (f0, f1) == (1, 2)
    part = predictor.predict_cores(net, frames[f0:f1], P_NET, BATCH, 13, 21, first_frame=f0, self_ensemble="rot90")
    assert se.same_bits(part.cpu().numpy(), np.ascontiguousarray(patches[13:21, 4:-4, 4:-4, 4:-4]))


def test_predict_file_and_evaluate_file_on_a_two_row_file(tmp_path, capsys):
    rng = np.random.default_rng(41)
    vencs = (1.5, 0.9)
    lr, hr = str(tmp_path / "two.h5"), str(tmp_path / "two_HR.h5")
    tree = {"dx": np.full((2, 3), 1.5, dtype=np.float32)}
    for n, s in (("u", 1.0), ("v", 0.5), ("w", 0.75)):
        tree[n] = np.stack([rng.uniform(-v, v, SHAPE) for v in vencs]).astype(np.float32)
        tree["venc_" + n] = (np.asarray(vencs) * s).astype(np.float32)
        tree["mag_" + n] = rng.uniform(0, 300, (2,) + SHAPE).astype(np.float32)
    h5io.write_file(lr, tree)
    hr_shape = tuple(R * s for s in SHAPE)
    truth = {n: np.stack([rng.uniform(-0.02 * v, 0.02 * v, hr_shape) for v in vencs]).astype(np.float32) for n in ("u", "v", "w")}
    truth["mask"] = rng.choice(np.array([0.0, 0.3, 1.0], np.float32), size=(1,) + hr_shape, p=[0.5, 0.1, 0.4])
    truth["dx"] = np.full((2, 3), 0.75, dtype=np.float32)
    h5io.write_file(hr, truth)
    # the frames as the predictor loads them, and case 3's path on them
    ds = data.ImageDataset()
    frames = np.empty((2, 6) + SHAPE, np.float32)
    scale = []
    for row in range(2):
        ds.load_vectorfield(lr, row)
        for c, n in enumerate(NAMES):
            frames[row, c] = getattr(ds, n)
        scale.append((ds.venc, ds.velocity_per_px))
    _, vol, _ = _reference(frames, se.ROT90)
    want = _finish(vol, scale)
    assert 0 < (want == 0).mean() < 1
    net = _net()
    out = str(tmp_path / "out.h5")
    # device_tiler is left False: the option takes the file through the device path by itself
    got = predictor.predict_file(net, lr, out, P_NET, R, batch_size=BATCH, verbose=True, frames_per_group=2, self_ensemble="rot90")
    assert "24 patches x 10 orientations" in capsys.readouterr().out
    assert len(got) == 2
    for row in range(2):
        for c in range(3):
            assert got[row][c].dtype == np.float64 and se.same_bits(got[row][c][0], want[row, c]), (row, c)
    back = h5io.read_all(out)
    for c, n in enumerate(("u", "v", "w")):
        assert back[n].tobytes() == want[:, c].astype(np.float32).tobytes()
    # the host finish (FDN_DEVICE_FINISH=0) keeps working and gives the same volumes
    os.environ["FDN_DEVICE_FINISH"] = "0"
    try:
        got0 = predictor.predict_file(net, lr, str(tmp_path / "out0.h5"), P_NET, R, batch_size=BATCH, verbose=False, frames_per_group=2,
                                      self_ensemble="rot90")
    finally:
        del os.environ["FDN_DEVICE_FINISH"]
    assert all(se.same_bits(got0[row][c], got[row][c]) for row in range(2) for c in range(3))
    # evaluate_file: the sums are ops.volume_metrics on that finished volume
    metrics, sums = predictor.evaluate_file(net, lr, hr, P_NET, R, batch_size=BATCH, frames_per_group=2, verbose=False, return_sums=True,
                                            self_ensemble="rot90")
    dtruth = torch.from_numpy(np.stack([truth[n] for n in ("u", "v", "w")], axis=1)).cuda()
    ref_sums = ops.volume_metrics(torch.from_numpy(want).cuda(), dtruth, torch.from_numpy(truth["mask"]).cuda()).cpu().numpy()
    assert sums.shape == ref_sums.shape == (2, len(predictor.VOLUME_SUM_NAMES)) and se.same_bits(sums, ref_sums)
    assert len(metrics) == 2 and _same_metrics(metrics, predictor.metrics_from_sums(sums))
    plain_sums = predictor.evaluate_file(net, lr, hr, P_NET, R, batch_size=BATCH, frames_per_group=2, verbose=False, return_sums=True)[1]
    assert not se.same_bits(plain_sums, sums)                                       # the option reached the prediction


def test_bf16_network_with_the_subset_list():
    frames = _frames()
    _, want, _ = _reference(frames, SUBSET, dtype="bfloat16")
    net = _net("bfloat16")
    vol = predictor.predict_volume(net, frames, P_NET, BATCH, self_ensemble=SUBSET)
    assert vol.dtype == torch.float32 and se.same_bits(vol.cpu().numpy(), want)
    _, want32, _ = _reference(frames, SUBSET)
    assert not se.same_bits(want, want32)                                           # another network arithmetic, the same ensemble

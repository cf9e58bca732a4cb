"""Overlap-add stitching on the device against tests/_blend_ref.py (written from the definition, nothing from the package):
fdn_input_features_volume_strided == host patchify(blend=) + fdn_input_features, bit for bit; fdn_blend_patches == the float32 emulation in
ascending patch order, bit for bit, within 16 x 2^-24 x sum w|p| of the float64 sum, whatever the chunking, with packed cores, and without
a write outside the accumulator; fdn_finish_volume == the host rule; and the predictor with blend= from predict_volume up to predict_file
and evaluate_file against the composition by hand -- forward on the host tiler's patches, then the reference blend."""
import importlib
import os

import numpy as np
import pytest
import torch

import _blend_ref as br
import _guarded as gd
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
_cache = {}


class _Vol:
    pass


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def _host_patches(frames, P, R, b):
    """What the host tiler makes of frames (F,6,X,Y,Z) with blend=b: six stacks (F*n,P,P,P), frame after frame, and the patch counts."""
    pg = tiler.PatchGenerator(P, R, blend=b)
    per_frame = []
    for f in range(frames.shape[0]):
        v = _Vol()
        for c, n in enumerate(NAMES):
            setattr(v, n, frames[f, c])
        vel, mag = pg.patchify(v)
        per_frame.append(list(vel) + list(mag))
    stacks = [np.ascontiguousarray(np.concatenate([pf[c] for pf in per_frame], axis=0)[..., 0]) for c in range(6)]
    return stacks, (pg.nr_x, pg.nr_y, pg.nr_z)


def _rotated(stacks, orientation):
    """Every host patch through data.rotate_vector_field (the velocities signed, the magnitudes not): six stacks again."""
    plane, k = orientation
    if plane == 0:
        return stacks
    n = stacks[0].shape[0]
    vel = [data.rotate_vector_field([stacks[c][b] for c in range(3)], k, plane, True) for b in range(n)]
    mag = [data.rotate_vector_field([stacks[3 + c][b] for c in range(3)], k, plane, False) for b in range(n)]
    return ([np.ascontiguousarray(np.stack([vel[b][c] for b in range(n)])) for c in range(3)] +
            [np.ascontiguousarray(np.stack([mag[b][c] for b in range(n)])) for c in range(3)])


# ---- 1. strided features ----
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_strided_features_equal_host_patchify_then_input_features(dtype):
    """P = 8 over two frames of (9,6,5) at strides 4, 3 and 2.  The bf16 twin against the existing bf16 twin on the same host patches: the
    fp32 values rounded as that one rounds them."""
    P, R = 8, 2
    frames = np.random.default_rng(5).standard_normal((F, 6) + SHAPE).astype(np.float32)
    dframes = torch.from_numpy(frames).cuda()
    o = ops if dtype == "float32" else ops_bf16
    for stride in (4, 3, 2):
        b = P - 4 - stride
        stacks, counts = _host_patches(frames, P, R, b)
        assert counts == br.counts(SHAPE, P, b) if b else counts == tiler.PatchGenerator(P, R).plan(SHAPE)[0]
        n = counts[0] * counts[1] * counts[2]
        ranges = ((0, F * n), (n - 2, 5), (F * n - 1, 1))                         # all; across the frame boundary; the last patch
        for orientation in ((0, 0), (1, 1), (2, 2), (3, 3)):
            ref_phase, ref_pc = o.input_features(*[torch.from_numpy(s).cuda() for s in _rotated(stacks, orientation)])
            for g0, count in ranges:
                phase, pc = o.input_features_volume(dframes, P, counts, g0, count, orientation=orientation, stride=stride)
                assert tuple(phase.shape) == tuple(pc.shape) == (count, P, P, P, 3) and phase.dtype == pc.dtype == ref_phase.dtype
                assert np.array_equal(_bits(phase), _bits(ref_phase[g0:g0 + count])), (stride, orientation, g0, "phase")
                assert np.array_equal(_bits(pc), _bits(ref_pc[g0:g0 + count])), (stride, orientation, g0, "pc")
            if stride == 4:                                                       # the existing entry points, reached without the keyword
                phase, pc = o.input_features_volume(dframes, P, counts, orientation=orientation, stride=4)
                old = o.input_features_volume(dframes, P, counts, orientation=orientation)
                assert np.array_equal(_bits(phase), _bits(old[0])) and np.array_equal(_bits(pc), _bits(old[1])), orientation
        if stride == 3:                                                           # the same counts as the plain window, another window
            assert counts == tiler.PatchGenerator(P, R).plan(SHAPE)[0]
            assert not np.array_equal(_bits(o.input_features_volume(dframes, P, counts, stride=3)[0]),
                                      _bits(o.input_features_volume(dframes, P, counts)[0]))


# ---- 2. blend_patches ----
BLEND_CASES = [(8, 2, 1), (8, 2, 2), (8, 4, 1), (12, 2, 4)]                      # (P, R, b); (12,2,4): 2b = E, the two ramps of a core touch


def _blend_case(P, R, b):
    key = ("blend", P, R, b)
    if key not in _cache:
        nr = br.counts(SHAPE, P, b)
        n = nr[0] * nr[1] * nr[2]
        S, side, sh = P * R, 2 * R, (P - 4 - b) * R
        ext = tuple(R * s for s in SHAPE)
        pred = np.random.default_rng(1000 * P + 10 * R + b).standard_normal((F * n, S, S, S, 3)).astype(np.float32)     # mixed sign
        want = br.blend32(pred, F, nr, side, sh, ext)
        val64, mag64 = br.blend64(pred, F, nr, side, sh, ext)
        for a in (pred, want, val64, mag64):
            a.setflags(write=False)
        _cache[key] = (nr, n, S, side, sh, ext, pred, want, val64, mag64)
    return _cache[key]


def _blend_chunks(dpred, nr, side, sh, ext, chunk, total):
    h = gd.guarded((F, 3) + ext, torch.float32, gd.NAN, "cuda")
    h.t.zero_()
    for g0 in range(0, total, chunk):
        ops.blend_patches(dpred[g0:g0 + chunk], h.t, side, sh, nr, g0)
    return h


@pytest.mark.parametrize("P,R,b", BLEND_CASES)
def test_blend_patches_equals_the_float32_reference_whatever_the_chunking(P, R, b):
    nr, n, S, side, sh, ext, pred, want, val64, mag64 = _blend_case(P, R, b)
    tp = tiler.PatchGenerator(P, R, blend=b).plan(SHAPE)
    assert tp[0] == nr and tp[2] == ext and any(p > 0 for p in tp[1])             # a far pad is cropped
    assert all((q - 1) * sh + S - 2 * side >= e for q, e in zip(nr, ext))
    assert n % 3 or n % 5                                                         # a batch crosses the frame boundary
    dpred = torch.from_numpy(pred.copy()).cuda()                                  # (the cached array is read-only)
    total = F * n
    first = None
    for chunk in (1, 3, 5, total):
        h = _blend_chunks(dpred, nr, side, sh, ext, chunk, total)
        got = h.t.cpu().numpy()
        assert gd.intact(h), ("a write outside the accumulator", chunk, h.damaged())
        assert br.same_bits(got, want), "chunk %d: %d voxels differ" % (chunk, int((got != want).sum()))
        first = got if first is None else first
        assert br.same_bits(got, first), chunk
    ok, worst = br.within_bound(first, val64, mag64)
    print("P=%d R=%d b=%d: largest error %.2f x 2^-24 sum w|p|" % (P, R, b, worst))
    assert ok, worst
    # the cores alone, packed, with side 0 and S = core
    cores = ops.pack_patch_cores(dpred, side)
    assert tuple(cores.shape) == (total, S - 2 * side, S - 2 * side, S - 2 * side, 3)
    h = gd.guarded((F, 3) + ext, torch.float32, gd.SENTINEL, "cuda")
    h.t.zero_()
    for g0 in range(0, total, 5):
        ops.blend_patches(cores[g0:g0 + 5], h.t, 0, sh, nr, g0)
    assert gd.intact(h) and br.same_bits(h.t.cpu().numpy(), want)
    # a call in the middle of the list touches the voxels of its patches alone
    h = gd.guarded((F, 3) + ext, torch.float32, gd.NAN, "cuda")
    h.t.zero_()
    ops.blend_patches(dpred[n - 1:n + 1], h.t, side, sh, nr, n - 1)               # the last patch of frame 0, the first of frame 1
    touched = h.t.cpu().numpy() != 0                                              # (no product w * p of these predictions is zero)
    only = br.blend64(np.ones((2, S, S, S, 3), np.float32), F, nr, side, sh, ext, g0=n - 1)[1] > 0
    assert gd.intact(h) and np.array_equal(touched, only) and only.any() and not only.all()


def test_blend_with_the_stride_of_the_core_is_the_plain_stitch():
    P, R = 8, 2
    pg = tiler.PatchGenerator(P, R)
    nr, _, ext = pg.plan(SHAPE)
    n = nr[0] * nr[1] * nr[2]
    pred = np.random.default_rng(12).standard_normal((F * n, 16, 16, 16, 3)).astype(np.float32)
    pred[0, 4:8, 4:8, 4:8] = -0.0                                                 # 0 + (-0.0) = +0.0: equal as numbers
    dpred = torch.from_numpy(pred).cuda()
    stitched = torch.full((F, 3) + ext, float("nan"), device="cuda")
    ops.stitch_patches(dpred, stitched, 4, nr, 0)
    acc = torch.zeros((F, 3) + ext, device="cuda")
    for g0 in range(0, F * n, 7):
        ops.blend_patches(dpred[g0:g0 + 7], acc, 4, 8, nr, g0)
    a, s = acc.cpu().numpy(), stitched.cpu().numpy()
    assert not np.isnan(s).any() and np.array_equal(a, s)
    assert np.signbit(s).any() and (s == 0).any()


# ---- 3. finish_volume ----
def test_finish_volume_equals_the_host_rule_around_the_threshold():
    rng = np.random.default_rng(21)
    ext = (6, 5, 7)
    acc = rng.uniform(-1, 1, (F, 3) + ext).astype(np.float32)
    vencs = (1.5, 0.3)
    scale = []
    for f, venc in enumerate(vencs):
        d = np.abs(acc[f].astype(np.float64) * venc)
        thr = float(np.sort(d.ravel())[d.size // 2])                              # a product EQUAL to the threshold: it stays (strict <)
        scale.append((venc, thr))
        assert (d == thr).any() and (d < thr).any() and (d > thr).any()
    acc[0, 0, 0, 0, 0] = -0.0
    acc[1, 2, 1, 1, 1] = 0.0
    want = br.finish(acc, scale)
    assert 0.3 < (want == 0).mean() < 0.7 and not np.signbit(want[want == 0]).any()
    for f, (venc, thr) in enumerate(scale):
        assert (np.abs(want[f]) == thr).any()
    dscale = torch.tensor(scale, dtype=torch.float64, device="cuda")
    h = gd.guarded(acc.shape, torch.float64, gd.NAN, "cuda")
    got = ops.finish_volume(torch.from_numpy(acc).cuda(), dscale, out=h.t)
    assert got is h.t and gd.intact(h) and br.same_bits(got.cpu().numpy(), want)
    fresh = ops.finish_volume(torch.from_numpy(acc).cuda(), dscale)
    assert fresh.dtype == torch.float64 and br.same_bits(fresh.cpu().numpy(), want)
    # a threshold of 0 zeroes nothing
    none = ops.finish_volume(torch.from_numpy(acc).cuda(), torch.tensor([(v, 0.0) for v in vencs], dtype=torch.float64, device="cuda"))
    assert br.same_bits(none.cpu().numpy(), br.finish(acc, [(v, 0.0) for v in vencs]))


# ---- 4. the predictor ----
P_NET, R_NET, B_NET, LR = 12, 2, 2, (12, 20, 5)
VENCS = (1.5, 0.9, 2.25)
BATCH = 4


def _net():
    if "net" not in _cache:
        _cache["net"] = predictor.prepare_network(P_NET, R_NET, 1, 1)
    return _cache["net"]


def _write_rows(path, shape, vencs, seed):
    rng = np.random.default_rng(seed)
    rows = len(vencs)
    tree = {"dx": np.full((rows, 3), 1.5, dtype=np.float32)}
    for n, scale in (("u", 1.0), ("v", 0.5), ("w", 0.75)):
        tree[n] = np.stack([rng.uniform(-v, v, shape) for v in vencs]).astype(np.float32)
        tree["venc_" + n] = (np.asarray(vencs) * scale).astype(np.float32)
        tree["mag_" + n] = rng.uniform(0, 300, (rows,) + shape).astype(np.float32)
    h5io.write_file(path, tree)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """The three-row file, its frames as the predictor loads them, the host tiler's patches with blend=2, the per-row (venc, threshold),
    and the composition by hand: network.forward on the host patches in batches of BATCH, then the reference blend and finish."""
    d = tmp_path_factory.mktemp("blend")
    src = str(d / "in.h5")
    _write_rows(src, LR, VENCS, seed=11)
    ds = data.ImageDataset()
    frames = np.empty((3, 6) + LR, np.float32)
    scale, dxs = [], []
    for row in range(3):
        ds.load_vectorfield(src, row)
        for c, n in enumerate(NAMES):
            frames[row, c] = getattr(ds, n)
        scale.append((ds.venc, ds.velocity_per_px))
        dxs.append(ds.dx)
    stacks, counts = _host_patches(frames, P_NET, R_NET, B_NET)
    assert counts == (2, 3, 1) == br.counts(LR, P_NET, B_NET) and stacks[0].shape == (18, 12, 12, 12)
    net = _net()
    pred = np.concatenate([net.forward([s[g0:g0 + BATCH] for s in stacks]).cpu().numpy() for g0 in range(0, 18, BATCH)])
    ext = tuple(R_NET * s for s in LR)
    vol = br.blend32(pred, 3, counts, 2 * R_NET, (P_NET - 4 - B_NET) * R_NET, ext)
    return dict(dir=d, src=src, frames=frames, scale=scale, dxs=dxs, stacks=stacks, counts=counts, pred=pred, vol=vol,
                finished=br.finish(vol, scale), ext=ext)


def test_predict_volume_with_blend_equals_the_composition_by_hand(rows):
    net = _net()
    frames, want = rows["frames"], rows["vol"]
    assert np.abs(want).max() > 0 and not np.isnan(want).any()
    vol = predictor.predict_volume(net, frames, P_NET, BATCH, blend=B_NET)
    assert vol.dtype == torch.float32 and tuple(vol.shape) == (3, 3) + rows["ext"] == want.shape
    assert br.same_bits(vol.cpu().numpy(), want)
    # another batch size: the same bytes
    assert br.same_bits(predictor.predict_volume(net, frames, P_NET, 5, blend=B_NET).cpu().numpy(), want)
    # finished
    assert 0 < (rows["finished"] == 0).mean() < 1
    fin = predictor.predict_volume(net, frames, P_NET, BATCH, frame_scale=rows["scale"], blend=B_NET)
    assert fin.dtype == torch.float64 and br.same_bits(fin.cpu().numpy(), rows["finished"])
    # patch_range halves, blended in order into one accumulator, are the whole
    acc = predictor.predict_volume(net, frames, P_NET, BATCH, patch_range=(0, 7), blend=B_NET)
    assert not br.same_bits(acc.cpu().numpy(), want)
    again = predictor.predict_volume(net, frames, P_NET, BATCH, out=acc, patch_range=(7, 18), blend=B_NET)
    assert again is acc and br.same_bits(acc.cpu().numpy(), want)
    # the cores of a shard, blended with side 0 at its first patch after the patches before it (a data-parallel peer)
    acc = predictor.predict_volume(net, frames, P_NET, BATCH, patch_range=(0, 7), blend=B_NET)
    cores = predictor.predict_cores(net, frames[1:], P_NET, BATCH, 7, 18, first_frame=1, blend=B_NET)
    assert tuple(cores.shape) == (11, 16, 16, 16, 3)
    assert br.same_bits(cores.cpu().numpy(), np.ascontiguousarray(rows["pred"][7:18, 4:-4, 4:-4, 4:-4]))
    ops.blend_patches(cores, acc, 0, (P_NET - 4 - B_NET) * R_NET, rows["counts"], 7)
    assert br.same_bits(acc.cpu().numpy(), want)
    # the blended volume is not the plain one, and has no more patches than the overlap asks for
    plain = predictor.predict_volume(net, frames, P_NET, BATCH)
    assert tuple(plain.shape) == tuple(vol.shape) and not br.same_bits(plain.cpu().numpy(), want)


def test_blend_zero_is_the_existing_path(rows):
    net = _net()
    frames = rows["frames"]
    plain = predictor.predict_volume(net, frames, P_NET, BATCH)                   # no keyword
    assert br.same_bits(predictor.predict_volume(net, frames, P_NET, BATCH, blend=0).cpu().numpy(), plain.cpu().numpy())
    fin = predictor.predict_volume(net, frames, P_NET, BATCH, frame_scale=rows["scale"])
    fin0 = predictor.predict_volume(net, frames, P_NET, BATCH, frame_scale=rows["scale"], blend=0)
    assert br.same_bits(fin0.cpu().numpy(), fin.cpu().numpy())
    # ... which is the stitch of forward() on the plain window's patches
    stacks, counts = _host_patches(frames, P_NET, R_NET, 0)
    n = counts[0] * counts[1] * counts[2]
    pred = np.concatenate([net.forward([s[g0:g0 + BATCH] for s in stacks]).cpu().numpy() for g0 in range(0, 3 * n, BATCH)])
    pg = tiler.PatchGenerator(P_NET, R_NET)
    pg.padding = pg.plan(LR)[1]
    want = np.stack([np.stack([pg._patchup_with_overlap(pred[f * n:(f + 1) * n, ..., c], *counts) for c in range(3)]) for f in range(3)])
    assert br.same_bits(plain.cpu().numpy(), want.astype(np.float32))
    cores = predictor.predict_cores(net, frames, P_NET, BATCH, 2, 9)
    assert br.same_bits(predictor.predict_cores(net, frames, P_NET, BATCH, 2, 9, blend=0).cpu().numpy(), cores.cpu().numpy())
    out, out0 = str(rows["dir"] / "plain.h5"), str(rows["dir"] / "plain0.h5")
    predictor.predict_file(net, rows["src"], out, P_NET, R_NET, batch_size=BATCH, verbose=False)
    predictor.predict_file(net, rows["src"], out0, P_NET, R_NET, batch_size=BATCH, verbose=False, blend=0)
    a, b = h5io.read_all(out), h5io.read_all(out0)
    assert sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


def test_self_ensemble_composes_with_blend(rows):
    net = _net()
    orientations = [(0, 0), (1, 1)]
    stacks = rows["stacks"]
    rotated = [_rotated(stacks, o) for o in orientations]
    mean = np.empty_like(rows["pred"])
    for g0 in range(0, 18, BATCH):
        preds = [net.forward([s[g0:g0 + BATCH] for s in rot]).cpu().numpy() for rot in rotated]
        mean[g0:g0 + BATCH] = se.mean(preds, orientations)
    want = br.blend32(mean, 3, rows["counts"], 2 * R_NET, (P_NET - 4 - B_NET) * R_NET, rows["ext"])
    vol = predictor.predict_volume(net, rows["frames"], P_NET, BATCH, self_ensemble=orientations, blend=B_NET)
    assert br.same_bits(vol.cpu().numpy(), want) and not br.same_bits(want, rows["vol"])


def _same_files(a, b):
    a, b = h5io.read_all(a), h5io.read_all(b)
    assert sorted(a) == sorted(b) == ["dx", "u", "v", "w"]
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_predict_file_with_blend_equals_the_host_tiler_and_the_composition_by_hand(rows, tmp_path):
    net = _net()
    src, stacks, counts = rows["src"], rows["stacks"], rows["counts"]
    # the host tiler: PatchGenerator(blend=2).patchify (the stacks) -> predict_patches on the same batches -> its patchup per row and
    # component -> de-normalise, zero, append: the lines of predict_file's host loop
    res = predictor.predict_patches(net, [s[..., None] for s in stacks[:3]], [s[..., None] for s in stacks[3:]], BATCH)
    assert res.shape == (18, 24, 24, 24, 3) and res.dtype == np.float64
    pg = tiler.PatchGenerator(P_NET, R_NET, blend=B_NET)
    pg.padding = pg.plan(LR)[1]
    host = str(tmp_path / "host.h5")
    ds = data.ImageDataset()
    want = []
    for row, (venc, vpp) in enumerate(rows["scale"]):
        vols, cols = [], []
        for i in range(3):
            v = pg._patchup_with_overlap(res[6 * row:6 * row + 6, :, :, :, i], *counts)
            assert v.dtype == np.float64
            v = v * venc
            v[np.abs(v) < vpp] = 0
            v = np.expand_dims(v, axis=0)
            vols.append(v)
            cols.append((ds.velocity_colnames[i], v))
        cols.append((ds.dx_colname, np.expand_dims(rows["dxs"][row] / R_NET, axis=0)))
        h5io.append_datasets(host, cols, compression='gzip')
        want.append(tuple(vols))
    for row in range(3):                                                          # the host tiler == the composition by hand
        for i in range(3):
            assert br.same_bits(want[row][i][0], rows["finished"][row, i]), (row, i)
    # the device: device_tiler is left False, blend takes the file through the device path by itself
    for tag, kw in (("b4", dict(batch_size=4, frames_per_group=3)), ("b5", dict(batch_size=5, frames_per_group=3)),
                    ("budget", dict(batch_size=4)), ("g1", dict(batch_size=4, frames_per_group=1))):
        out = str(tmp_path / (tag + ".h5"))
        got = predictor.predict_file(net, src, out, P_NET, R_NET, verbose=False, blend=B_NET, **kw)
        assert len(got) == 3
        for row in range(3):
            for i in range(3):
                assert got[row][i].dtype == np.float64 and br.same_bits(got[row][i], want[row][i]), (tag, row, i)
        _same_files(out, host)
    # the host finish (FDN_DEVICE_FINISH=0) gives the same file
    os.environ["FDN_DEVICE_FINISH"] = "0"
    try:
        out0 = str(tmp_path / "finish0.h5")
        predictor.predict_file(net, src, out0, P_NET, R_NET, batch_size=4, verbose=False, frames_per_group=2, blend=B_NET)
    finally:
        del os.environ["FDN_DEVICE_FINISH"]
    _same_files(out0, host)
    plain = str(tmp_path / "plain.h5")
    predictor.predict_file(net, src, plain, P_NET, R_NET, batch_size=4, verbose=False)
    assert h5io.read_all(plain)["u"].tobytes() != h5io.read_all(host)["u"].tobytes()


def test_evaluate_file_scores_the_blended_volume(rows, tmp_path):
    net = _net()
    rng = np.random.default_rng(43)
    hr = str(tmp_path / "in_HR.h5")
    hr_shape = rows["ext"]
    truth = {n: np.stack([rng.uniform(-0.02 * v, 0.02 * v, hr_shape) for v in VENCS]).astype(np.float32) for n in ("u", "v", "w")}
    truth["mask"] = rng.choice(np.array([0.0, 0.3, 1.0], np.float32), size=(1,) + hr_shape, p=[0.5, 0.1, 0.4])
    truth["dx"] = np.full((3, 3), 0.75, dtype=np.float32)
    h5io.write_file(hr, truth)
    metrics, sums = predictor.evaluate_file(net, rows["src"], hr, P_NET, R_NET, batch_size=BATCH, frames_per_group=2, verbose=False,
                                            return_sums=True, blend=B_NET)
    vol = predictor.predict_volume(net, rows["frames"], P_NET, BATCH, frame_scale=rows["scale"], blend=B_NET)
    assert br.same_bits(vol.cpu().numpy(), rows["finished"])
    dtruth = torch.from_numpy(np.stack([truth[n] for n in ("u", "v", "w")], axis=1)).cuda()
    ref = ops.volume_metrics(vol, dtruth, torch.from_numpy(truth["mask"]).cuda()).cpu().numpy()
    assert sums.shape == ref.shape == (3, len(predictor.VOLUME_SUM_NAMES)) and br.same_bits(sums, ref)
    assert len(metrics) == 3
    plain = predictor.evaluate_file(net, rows["src"], hr, P_NET, R_NET, batch_size=BATCH, frames_per_group=2, verbose=False, return_sums=True)[1]
    assert not br.same_bits(plain, sums)                                          # the option reached the prediction

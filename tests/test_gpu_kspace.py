"""Low-res synthesis on the device (fdn_kspace_downsample, kspace_stage_kernel) against the float64 pipeline of
tests/_kspace_ref.py, which tests/test_kspace_host.py ties to fft_downsampling.downsample_phase_img.

Results are compared in the complex plane -- z = mag_out / ratio * exp(i pi vel_out / venc), E = max|z_dev - z_ref64| / max|z_ref64| --
because the angle of a small z is ill-conditioned and z is not.  The bound is E_dev <= 8 * E_c64, E_c64 being the error of the SAME
statements in complex64 (numpy) on the same operands, computed here: the factor covers a sequential fp32 sum of up to 84 terms against
numpy's blocked sums and twiddles that come from sincospif instead of rounded float64 values.  Every operand sits between guard bands
(tests/_guarded.py) and the workspace is exactly as large as the library asks.

GRID_CAP: a stage launches at most 128 workgroups of 256 threads per volume (FDN_KS_MAX_BLOCKS, csrc/kspace_dft.h) and strides beyond;
the example frame's smallest stage has 42*38*36 = 57456 outputs per volume = 225 workgroups' worth, so every stage of it crosses the cap."""
import functools
import importlib
import os
import random
import shutil

import numpy as np
import pytest
import torch

import _kspace_ref as ref
from _guarded import NAN, SENTINEL, exact_workspace, guarded, guarded_like, intact, unchanged

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HR_FILE = os.path.join(HERE, "golden", "data", "example_data_HR.h5")
GRID_CAP = 128
_lib = importlib.import_module("4dflownet_amd._lib")
ops = importlib.import_module("4dflownet_amd.ops")
h5io = importlib.import_module("4dflownet_amd.h5io")
data = importlib.import_module("4dflownet_amd.data")
prep = importlib.import_module("4dflownet_amd.prepare_lowres")
fft = importlib.import_module("4dflownet_amd.fft_downsampling")
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _hr():
    return h5io.read_all(HR_FILE)


@functools.lru_cache(maxsize=None)
def _operands(case):
    """(vel (nvol,X,Y,Z), mag (X,Y,Z), venc, mag_scale, snr_db per volume, crops), everything fp32-representable."""
    rng = np.random.RandomState(17)
    if case == "odd":                               # odd extents, nothing a multiple of 4, velocities to +-1.2 venc (wrap)
        shape, crops, venc, scale, snr = (21, 18, 15), (5, 4, 3), [1.5], [1.0], [15.0]
    elif case == "third":                           # ratio 1/3, three volumes with their own venc / mag_scale / SNR
        shape, crops, venc, scale, snr = (20, 14, 13), (3, 2, 2), [0.6, 1.5, 3.0], [60.0, 120.0, 240.0], [14.0, 15.3, 16.9]
    elif case == "full":                            # full crops, no noise to speak of: z returns x
        shape, crops, venc, scale, snr = (8, 8, 8), (4, 4, 4), [1.0], [1.0], [300.0]
    else:                                           # frame 0 of the shipped high-res example, u, v, w in one call, mask x 120
        hr = _hr()
        vel = np.stack([hr[n][0] for n in "uvw"]).astype(f32)
        return vel, hr["mask"][0].astype(f32), [1.5, 1.0, 1.5], [120.0] * 3, [15.0, 14.2, 16.1], (21, 19, 18)
    assert crops == ref.crops_of(shape, {"odd": 1 / 2, "third": 1 / 3, "full": 1.0}[case])
    n = len(venc)
    vel = (rng.uniform(-1.2, 1.2, (n,) + shape) * np.asarray(venc)[:, None, None, None]).astype(f32)
    mag = rng.uniform(0.2, 1.0, shape).astype(f32) * (f32(100) if scale[0] == 1.0 else f32(1))
    return vel, mag, venc, scale, snr, crops


def _params(venc, scale, snr):
    t = np.zeros((len(venc), 4), np.float64)
    t[:, 0], t[:, 1], t[:, 2] = venc, scale, 10.0 ** (np.asarray(snr) / 10.0)
    return t.astype(f32)


@functools.lru_cache(maxsize=None)
def _reference(case, noise):
    """Per volume the float64 pipeline and its complex64 restatement on the operands the device gets.  noise: "supplied" (fp32 normals
    from numpy) or (seed, stream_id): the helper's float64 Philox normals."""
    vel, mag, venc, scale, snr, crops = _operands(case)
    p = _params(venc, scale, snr)
    lr = tuple(2 * c for c in crops)
    if noise == "supplied":
        g = np.random.RandomState(23).normal(0, 1, (len(venc),) + lr).astype(f32)
    else:
        g = ref.philox_normals(len(venc) * int(np.prod(lr)), *noise).reshape((len(venc),) + lr)
    r64 = [ref.pipeline(vel[v], mag, p[v, 0], crops, p[v, 2], g[v], p[v, 1]) for v in range(len(venc))]
    r32 = [ref.pipeline(vel[v], mag, p[v, 0], crops, p[v, 2], g[v], p[v, 1], single=True) for v in range(len(venc))]
    e_c64 = [float(np.abs(b["z"] - a["z"]).max() / np.abs(a["z"]).max()) for a, b in zip(r64, r32)]
    return g, r64, e_c64


def _run(case, noise, seed=0, stream_id=0):
    """One call of the C entry point on guarded operands; checks bands and inputs, returns (out_vel, out_mag, sigma) as numpy."""
    vel, mag, venc, scale, snr, crops = _operands(case)
    nvol, (X, Y, Z) = vel.shape[0], mag.shape
    lr = (nvol,) + tuple(2 * c for c in crops)
    dev = lambda a, fill: guarded_like(torch.from_numpy(np.ascontiguousarray(a)).cuda(), fill)
    ins = [dev(vel, NAN), dev(mag, SENTINEL), dev(_params(venc, scale, snr), NAN)]
    if noise is not None:
        ins.append(dev(noise, SENTINEL))
    snaps = [h.t.clone() for h in ins]
    outs = [guarded(lr, torch.float32, NAN, "cuda"), guarded(lr, torch.float32, SENTINEL, "cuda"), guarded((nvol,), torch.float32, NAN, "cuda")]
    lib = _lib.load()
    need = lib.fdn_kspace_downsample_workspace_bytes(nvol, X, Y, Z, *crops)
    assert need > 0
    ws = exact_workspace(need, NAN, SENTINEL, "cuda")
    _lib.check(lib.fdn_kspace_downsample(ins[0].t.data_ptr(), ins[1].t.data_ptr(), ins[2].t.data_ptr(), nvol, X, Y, Z, *crops,
                                         ins[3].t.data_ptr() if noise is not None else None, seed, stream_id, outs[0].t.data_ptr(),
                                         outs[1].t.data_ptr(), outs[2].t.data_ptr(), ws.t.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "fdn_kspace_downsample")
    torch.cuda.synchronize()
    for h in ins + outs + [ws]:
        assert intact(h), h.damaged()
    for h, s in zip(ins, snaps):
        assert unchanged(h, s)
    return tuple(o.t.cpu().numpy() for o in outs)


@functools.lru_cache(maxsize=None)
def _device(case):
    return _run(case, _reference(case, "supplied")[0])


def _errors(case, got, refs):
    """E per volume and the device's z."""
    vel, mag, venc, scale, snr, crops = _operands(case)
    p = _params(venc, scale, snr)
    zs = [ref.rebuild(got[0][v], got[1][v], p[v, 0], r["ratio"]) for v, r in enumerate(refs)]
    return [float(np.abs(z - r["z"]).max() / np.abs(r["z"]).max()) for z, r in zip(zs, refs)], zs


CASES = ["odd", "third", "full", "example"]


@pytest.mark.parametrize("case", CASES)
def test_device_result_is_within_eight_complex64_errors_of_float64(case):
    _, refs, e_c64 = _reference(case, "supplied")
    got = _device(case)
    assert all(np.isfinite(a).all() for a in got)
    e_dev, _ = _errors(case, got, refs)
    print(case, "E_dev", e_dev, "E_c64", e_c64)
    for e, c in zip(e_dev, e_c64):
        assert e <= 8 * c, (case, e_dev, e_c64)
    if case == "example":                                               # every stage strides: see GRID_CAP
        assert min(refs[0]["z"].size, 2 * 21 * 76 * 72) > GRID_CAP * 256


@pytest.mark.parametrize("case", CASES)
def test_velocities_agree_where_the_phase_is_well_conditioned(case):
    vel, mag, venc, scale, snr, crops = _operands(case)
    p = _params(venc, scale, snr)
    _, refs, e_c64 = _reference(case, "supplied")
    got = _device(case)
    for v, r in enumerate(refs):
        a = np.abs(r["z"])
        keep = a >= 1e-3 * a.max()
        assert 1 - keep.mean() <= 0.01, (case, v, 1 - keep.mean())
        bound = float(p[v, 0]) / np.pi * 8 * e_c64[v] * a.max() / a[keep]
        d = np.abs(got[0][v].astype(np.float64) - r["lr_vel"])[keep]
        print(case, v, "max dvel / bound", float((d / bound).max()), "left out", float(1 - keep.mean()))
        assert np.all(d <= bound), (case, v, float((d / bound).max()))


@pytest.mark.parametrize("case", CASES)
def test_sigma_formed_on_the_device(case):
    _, refs, e_c64 = _reference(case, "supplied")
    sigma = _device(case)[2]
    for v, r in enumerate(refs):
        F = np.abs(r["F"])
        bound = 4 * e_c64[v] * F.max() / np.sqrt(np.mean(F ** 2))
        print(case, v, "sigma rel err", abs(sigma[v] / r["sigma"] - 1), "bound", bound)
        assert abs(float(sigma[v]) / float(r["sigma"]) - 1) <= bound, (case, v, sigma[v], r["sigma"])


def test_full_crop_without_noise_returns_the_input_image():
    """Catches the frequency ordering, the -c term and the 1/M factors on their own."""
    vel, mag, venc, scale, snr, crops = _operands("full")
    _, refs, e_c64 = _reference("full", "supplied")
    x = mag.astype(np.float64) * np.exp(1j * np.pi * vel[0].astype(np.float64) / venc[0])
    assert np.abs(refs[0]["z"] - x).max() <= 1e-12 * np.abs(x).max() and refs[0]["ratio"] == 1.0
    _, zs = _errors("full", _device("full"), refs)
    assert np.abs(zs[0] - x).max() <= 8 * e_c64[0] * np.abs(x).max()
    assert float(_device("full")[2][0]) < 1e-9


@pytest.mark.parametrize("case", ["odd", "third", "example"])
def test_philox_noise_generated_in_the_kernel(case):
    seed, stream = (0xA4093822 << 32) | 12345, (7 << 32) | 3            # both halves of both words are in use
    _, refs, e_c64 = _reference(case, (seed, stream))
    got = _run(case, None, seed, stream)
    e_dev, _ = _errors(case, got, refs)
    allow = [8 * c + 4e-6 * float(r["sigma"]) / np.abs(r["z"]).max() for c, r in zip(e_c64, refs)]
    print(case, "E_dev", e_dev, "allowed", allow)
    for e, a in zip(e_dev, allow):
        assert e <= a, (case, e_dev, allow)
    again = _run(case, None, seed, stream)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))  # reproducible bit for bit
    other = _run(case, None, seed, stream + 1)
    assert not np.array_equal(other[0], got[0]) and not np.array_equal(other[1], got[1])
    assert other[2].tobytes() == got[2].tobytes()                       # sigma does not depend on the noise


def test_operator_equals_the_entry_point_and_refuses_what_it_cannot_run():
    vel, mag, venc, scale, snr, crops = _operands("third")
    g = _reference("third", "supplied")[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lv, lm, sg = ops.kspace_downsample(t(vel), t(mag), venc, snr, crops, noise=t(g), mag_scale=scale)
    for a, b in zip((lv, lm, sg), _device("third")):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    assert ops.kspace_crops((20, 14, 13), 1 / 3) == crops
    with pytest.raises(_lib.FdnError, match="GPU"):
        ops.kspace_downsample(torch.from_numpy(vel), t(mag), venc, snr, crops)
    with pytest.raises(_lib.FdnError, match="out of range"):
        ops.kspace_downsample(t(vel), t(mag), venc, snr, (11, 2, 2))
    with pytest.raises(_lib.FdnError, match="noise must be"):
        ops.kspace_downsample(t(vel), t(mag), venc, snr, crops, noise=t(g[:2]))
    with pytest.raises(_lib.FdnError, match="one value per volume"):
        ops.kspace_downsample(t(vel), t(mag), [1.0, 2.0], snr, crops)


def test_prepare_lowres_dataset_with_the_hip_engine(tmp_path):
    hr = _hr()
    random.seed(3); np.random.seed(3)
    a = h5io.read_all(prep.prepare_lowres_dataset(HR_FILE, str(tmp_path / "numpy.h5"), downsample=2))
    random.seed(3); np.random.seed(3)
    b = h5io.read_all(prep.prepare_lowres_dataset(HR_FILE, str(tmp_path / "hip.h5"), downsample=2, engine="hip"))
    next_hip = np.random.random()
    assert set(a) == set(b)
    n = hr["u"].shape[0]
    for k in ("u", "v", "w", "mag_u", "mag_v", "mag_w"):                # the layout test_prepare_lowres_dataset_writes_reference_layout expects
        assert b[k].shape == a[k].shape == (n,) + tuple(s // 2 for s in hr["u"].shape[1:]) and b[k].dtype == np.float32
    for k in ("venc_u", "venc_v", "venc_w", "SNRdb"):
        assert b[k].shape == (n,) and b[k].dtype == a[k].dtype and np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["mask"], b["mask"])
    # the draws of that run, once more, for the helper: E_c64 on the same operands
    random.seed(3); np.random.seed(3)
    for idx in range(n):
        snr_db = np.random.randint(140, 170) / 10
        vencs = prep.pick_vencs(*[hr[c + "_max"][idx] * 1.1 for c in "uvw"], prep.choose_venc())
        mag = hr["mask"][0] * prep.MAG_VALUES[idx % 5]
        for c, venc in zip("uvw", vencs):
            assert f32(venc) == a["venc_" + c][idx] and f32(snr_db) == a["SNRdb"][idx]
            g = np.random.normal(0, 1, a["u"].shape[1:])
            r64 = ref.pipeline(hr[c][idx], mag, venc, (21, 19, 18), 10 ** (snr_db / 10), g)
            r32 = ref.pipeline(hr[c][idx], mag, venc, (21, 19, 18), 10 ** (snr_db / 10), g, single=True)
            scale = np.abs(r64["z"]).max()
            e_c64 = np.abs(r32["z"] - r64["z"]).max() / scale
            z_np = ref.rebuild(a[c][idx], a["mag_" + c][idx], venc, r64["ratio"])
            z_hip = ref.rebuild(b[c][idx], b["mag_" + c][idx], venc, r64["ratio"])
            print(c, "hip vs numpy file", np.abs(z_hip - z_np).max() / scale, "hip vs float64", np.abs(z_hip - r64["z"]).max() / scale, "E_c64", e_c64)
            assert np.abs(z_hip - r64["z"]).max() <= 8 * e_c64 * scale
            assert np.abs(z_hip - z_np).max() <= 8 * e_c64 * scale
    assert np.random.random() == next_hip                               # the same host random stream, to the end


INDEX_ROWS = [(0, 12, 20, 0, 0, 0), (30, 26, 24, 0, 0, 0), (0, 12, 20, 1, 1, 1), (30, 26, 24, 1, 2, 2), (14, 6, 3, 1, 3, 3)]


def _loader_dir(tmp_path, name, lr_vencs=None):
    """A data directory with the high-res example alone, or with a prepared low-res file of the given VENC rows beside it."""
    d = tmp_path / name
    d.mkdir()
    shutil.copy(HR_FILE, str(d / "hr.h5"))
    if lr_vencs is not None:
        zeros = np.zeros((1, 42, 38, 36), f32)
        for k in ("u", "v", "w", "mag_u", "mag_v", "mag_w"):
            h5io.append_dataset(str(d / "lr.h5"), k, zeros)
        for c, k in enumerate(("venc_u", "venc_v", "venc_w")):
            h5io.append_dataset(str(d / "lr.h5"), k, np.asarray(lr_vencs[:, c]))
    return str(d)


def test_device_loader_resynthesises_the_low_res_side_every_pass(tmp_path):
    ddev = importlib.import_module("4dflownet_amd.data_device")
    P, R, B = 12, 2, 3
    index = np.array([["lr.h5", "hr.h5", "0"] + [str(x) for x in row] + ["0.7"] for row in INDEX_ROWS])
    make = lambda: ddev.DevicePatchHandler3D(_loader_dir(tmp_path, "only_hr_%d" % len(os.listdir(str(tmp_path)))), P, R, B,
                                             resynthesize=dict(seed=1))
    h = make()
    assert not os.path.exists(os.path.join(h.data_directory, "lr.h5"))
    ds = h.initialize_dataset(index, shuffle=False, shard=(0, 1))
    passes = [[tuple(t.cpu().numpy() for t in b) for b in ds] for _ in range(2)]
    assert [len(b[0]) for b in passes[0]] == [3, 2]
    hr = _hr()
    for epoch, batches in enumerate(passes):
        snr, vencs, mags = prep.draw_degradations(hr["u_max"], hr["v_max"], hr["w_max"], seed=1, epoch=epoch)
        vencs32 = vencs.astype(f32)
        g = ref.philox_normals(3 * 42 * 38 * 36, 1, epoch << 32).reshape(3, 42, 38, 36)
        snr_lin = f32(10.0 ** (snr[0] / 10.0))
        mask = hr["mask"][0]
        r64 = [ref.pipeline(hr[c][0], mask, vencs32[0, i], (21, 19, 18), snr_lin, g[i], f32(mags[0])) for i, c in enumerate("uvw")]
        r32 = [ref.pipeline(hr[c][0], mask, vencs32[0, i], (21, 19, 18), snr_lin, g[i], f32(mags[0]), single=True) for i, c in enumerate("uvw")]
        e_c64 = [np.abs(b["z"] - a["z"]).max() / np.abs(a["z"]).max() for a, b in zip(r64, r32)]
        allow = [(8 * e + 4e-6 * float(r["sigma"]) / np.abs(r["z"]).max()) * np.abs(r["z"]).max() for e, r in zip(e_c64, r64)]
        venc = vencs32[0].max()
        rows = iter(INDEX_ROWS)
        for batch in batches:
            assert np.array_equal(batch[9], np.full(len(batch[0]), venc, f32))
            for s in range(len(batch[0])):
                x0, y0, z0, rot, plane, k = next(rows)
                sl = np.index_exp[x0:x0 + P, y0:y0 + P, z0:z0 + P]
                perm = data._ROT[(plane, k)][0] if rot else (0, 1, 2)
                want_v = tuple(r["lr_vel"][sl] for r in r64)
                want_m = tuple(r["lr_mag"][sl] for r in r64)
                if rot:
                    want_v = data.rotate_vector_field(want_v, k, plane, True)
                    want_m = data.rotate_vector_field(want_m, k, plane, False)
                for i in range(3):
                    src = perm[i]
                    z_dev = ref.rebuild(batch[i][s, ..., 0].astype(np.float64) * venc, batch[3 + i][s, ..., 0].astype(np.float64) * 4095,
                                        vencs32[0, src], r64[src]["ratio"])
                    z_ref = ref.rebuild(want_v[i], want_m[i], vencs32[0, src], r64[src]["ratio"])
                    assert np.abs(z_dev - z_ref).max() <= allow[src], (epoch, s, i, np.abs(z_dev - z_ref).max(), allow[src])
        if epoch == 0:
            # the high-res side, the mask and the venc vector are those of a plain handler on a prepared pair with these VENC rows
            plain = ddev.DevicePatchHandler3D(_loader_dir(tmp_path, "pair", vencs32), P, R, B)
            for got, want in zip(batches, plain.initialize_dataset(index, shuffle=False, shard=(0, 1))):
                for i in (6, 7, 8, 9, 10):
                    assert got[i].tobytes() == want[i].cpu().numpy().tobytes(), i
                assert len(got) == len(want) == 11 and all(tuple(a.shape) == tuple(b.shape) for a, b in zip(got, want))
    for i in range(6):                                                  # two passes: another degradation
        assert not np.array_equal(passes[0][0][i], passes[1][0][i]), i
    assert np.array_equal(passes[0][0][10], passes[1][0][10])           # (the high-res patches are divided by the epoch's venc)
    ds2 = make().initialize_dataset(index, shuffle=False, shard=(0, 1))
    for want in passes:                                                 # a second handler with the same seed: both passes bit for bit
        for got, w in zip(ds2, want):
            assert all(a.cpu().numpy().tobytes() == b.tobytes() for a, b in zip(got, w))

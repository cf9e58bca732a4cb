"""CPU-side checks of the device low-res synthesis: the float64 reference the GPU tests compare against equals the reference's own
pipeline (fft_downsampling.downsample_phase_img) under the same seed, the Philox generator and its normal mapping, the two entry points
in the header and the ctypes table with every refusal made before the device is touched (fake pointers, no GPU), and the host random
streams of the new Python paths."""
import ctypes
import importlib
import os
import random
import re

import numpy as np
import pytest

import _kspace_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
NAMES = ("fdn_kspace_downsample_workspace_bytes", "fdn_kspace_downsample")
fft = importlib.import_module("4dflownet_amd.fft_downsampling")
prep = importlib.import_module("4dflownet_amd.prepare_lowres")


def _operands(shape, seed):
    rng = np.random.RandomState(seed)
    vel = rng.uniform(-1.2, 1.2, shape)
    mag = rng.uniform(0.2, 1.0, shape) * 120
    return vel, mag


@pytest.mark.parametrize("shape,ratio", [((21, 18, 15), 1 / 2), ((20, 14, 13), 1 / 3), ((24, 24, 24), 1 / 4)])
def test_float64_reference_equals_downsample_phase_img_under_the_same_seed(shape, ratio):
    vel, mag = _operands(shape, 5)
    venc, snr_db = 1.0, 15.5
    crops = ref.crops_of(shape, ratio)
    np.random.seed(11)
    want_vel, want_mag = fft.downsample_phase_img(vel, mag, venc, ratio, snr_db)
    np.random.seed(11)
    g = np.random.normal(0, 1, tuple(2 * c for c in crops))             # normal(0, sigma) is sigma times this draw
    r = ref.pipeline(vel, mag, venc, crops, 10 ** (snr_db / 10), g)
    assert r["lr_vel"].shape == want_vel.shape == tuple(2 * c for c in crops)
    z_want = ref.rebuild(want_vel, want_mag, venc, r["ratio"])
    scale = np.abs(z_want).max()
    assert np.abs(r["z"] - z_want).max() <= 1e-12 * scale
    assert np.abs(ref.rebuild(r["lr_vel"], r["lr_mag"], venc, r["ratio"]) - z_want).max() <= 1e-12 * scale


def test_philox_known_answers():
    h = lambda ws: " ".join("%08x" % w for w in ws)
    assert h(ref.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert h(ref.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert h(ref.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # the vectorised form used for whole arrays agrees with the integer one, 64-bit element indices and keys included
    for e, seed, stream in ((0, 0, 0), (5, 7, 9), ((3 << 32) | 17, (0xa4093822 << 32) | 5, (1 << 40) | 3)):
        x0, x1 = ref._philox_words(np.array([e], np.uint64), seed, stream)
        want = ref.philox4x32_10((e & ref.MASK, e >> 32, stream & ref.MASK, stream >> 32), (seed & ref.MASK, seed >> 32))
        assert (int(x0[0]), int(x1[0])) == want[:2]


def test_philox_normals_have_the_moments_of_a_standard_normal():
    n = 57456                                                            # 42 * 38 * 36
    g = ref.philox_normals(n, seed=1, stream_id=2)
    assert np.isfinite(g).all()
    assert abs(g.mean()) < 0.02 and abs(g.var() - 1) < 0.03              # 5 sigma: 5 / sqrt(n), 5 sqrt(2 / n)
    assert np.array_equal(ref.philox_normals(100, 1, 2, first=50), g[50:150])
    assert not np.array_equal(ref.philox_normals(100, 1, 3), g[:100])


def test_header_and_ctypes_table_hold_the_two_entry_points(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    lib = fdn._lib.load()
    for n in NAMES:
        assert n in declared and n in fdn._lib.SIGNATURES and hasattr(lib, n), n
    assert declared == set(fdn._lib.SIGNATURES)
    sig = fdn._lib.SIGNATURES
    assert sig[NAMES[0]] == (ctypes.c_size_t, [ctypes.c_int] * 7)
    assert len(sig[NAMES[1]][1]) == 18 and sig[NAMES[1]][1][11:13] == [ctypes.c_uint64] * 2
    proto = header[:header.index("size_t " + NAMES[0] + "(")]
    comment = proto[proto.rindex("/*"):]
    for words in ("fft_downsampling.py", "Philox4x32-10", "sincospif", "mod N", "Refused before the device is touched"):
        assert words in comment, words
    assert int(re.search(r"#define FDN_VERSION (\d+)", header).group(1)) == lib.fdn_version() == fdn._lib.FDN_VERSION == 161


def test_workspace_bytes_is_positive_and_monotone_in_nvol(fdn):
    ws = fdn._lib.load().fdn_kspace_downsample_workspace_bytes
    sizes = [ws(n, 21, 18, 15, 10, 9, 7) for n in (1, 2, 3, 7)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    # room for the two complex fp32 volumes the stages alternate between, at least
    assert sizes[0] >= 8 * (20 * 18 * 15 + 20 * 18 * 15)
    assert ws(1, 1024, 1024, 1024, 512, 512, 512) > 2 ** 34             # size_t: no 32-bit wrap
    for bad in ((0, 21, 18, 15, 10, 9, 7), (1, 1025, 18, 15, 10, 9, 7), (1, 21, 18, 15, 11, 9, 7), (1, 21, 18, 15, 10, 0, 7)):
        assert ws(*bad) == 0, bad


def test_kspace_downsample_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    name = NAMES[1]
    err = lambda: lib.fdn_last_error().decode()
    hr, lr = 21 * 18 * 15 * 4, 3 * 10 * 8 * 6 * 4
    good = dict(vel=0x10000000, mag=0x20000000, params=0x30000000, nvol=3, X=21, Y=18, Z=15, cx=5, cy=4, cz=3, noise=0x40000000, seed=1,
                stream_id=2, out_vel=0x50000000, out_mag=0x60000000, sigma_out=0x70000000, workspace=0x80000000)
    order = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fdn_kspace_downsample(*[a[k] for k in order], None)

    def named(rc, *words):
        return rc == BAD_ARG and err().startswith(name + ":") and all(w in err() for w in words)

    for p in ("vel", "mag", "params", "out_vel", "out_mag", "workspace"):
        assert named(call(**{p: None}), p, "NULL"), (p, err())
    for nvol in (0, -1):
        assert named(call(nvol=nvol), "nvol=%d" % nvol), err()
    for ax in "XYZ":
        for n in (0, -3, 1025, 4096):
            assert named(call(**{ax: n}), "%s=%d" % (ax, n)), err()
    for ax, half in (("x", 10), ("y", 9), ("z", 7)):
        for c in (0, -1, half + 1):
            assert named(call(**{"c" + ax: c}), "c%s=%d" % (ax, c)), err()
    # an output that overlaps an input, from either side and by one float
    for out, nbytes in (("out_vel", lr), ("out_mag", lr), ("sigma_out", 12)):
        for inp, ibytes in (("vel", 3 * hr), ("mag", hr), ("params", 48), ("noise", lr)):
            for at in (good[inp], good[inp] + ibytes - 4, good[inp] - nbytes + 4):
                assert named(call(**{out: at}), "overlap", out, inp), (out, inp, err())
    assert named(call(out_mag=good["out_vel"] + lr - 4), "overlap", "out_vel", "out_mag"), err()
    # noise and sigma_out may be NULL
    assert named(call(noise=None, sigma_out=None, nvol=0), "nvol=0"), err()


def test_device_path_leaves_the_global_random_stream_where_downsample_phase_img_leaves_it(monkeypatch):
    """noise="numpy" draws normal(0, 1) of the cropped shape once per volume; noise="philox" draws nothing.  The kernel call is stubbed."""
    import torch
    ops = importlib.import_module("4dflownet_amd.ops")
    seen = {}

    def stub(vel, mag, venc, snr_db, crops, noise=None, seed=0, stream_id=0, mag_scale=None):
        seen.update(noise=noise, crops=crops, seed=seed, stream_id=stream_id, venc=venc)
        shape = (vel.shape[0],) + tuple(2 * c for c in crops)
        return torch.zeros(shape), torch.zeros(shape), torch.zeros(vel.shape[0])
    monkeypatch.setattr(ops, "kspace_downsample", stub)
    shape, ratio = (20, 14, 13), 1 / 3
    vel, mag = _operands(shape, 2)
    np.random.seed(21)
    fft.downsample_phase_img(vel, mag, 1.5, ratio, 15.0)
    want_next = np.random.normal()
    np.random.seed(21)
    lv, lm = fft.downsample_phase_img_device(vel, mag, 1.5, ratio, 15.0, noise="numpy", device="cpu")
    assert np.random.normal() == want_next
    assert lv.shape == lm.shape == (6, 4, 4) and isinstance(lv, np.ndarray) and seen["crops"] == (3, 2, 2)
    np.random.seed(21)
    want = np.random.normal(0, 1, (6, 4, 4)).astype(np.float32)
    assert np.array_equal(seen["noise"][0].numpy(), want)                # the standard draw itself, as float32
    # three volumes in one call consume what three calls of the reference consume
    np.random.seed(22)
    for _ in range(3):
        fft.downsample_phase_img(vel, mag, 1.5, ratio, 15.0)
    want_next = np.random.normal()
    np.random.seed(22)
    lv, _ = fft.downsample_phase_img_device(np.stack([vel] * 3), mag, (1.5, 2.0, 2.5), ratio, 15.0, device="cpu")
    assert np.random.normal() == want_next and lv.shape == (3, 6, 4, 4)
    np.random.seed(23)
    want_next = np.random.normal()
    np.random.seed(23)
    fft.downsample_phase_img_device(vel, mag, 1.5, ratio, 15.0, noise="philox", seed=5, stream_id=6, device="cpu")
    assert np.random.normal() == want_next and seen["noise"] is None and (seen["seed"], seen["stream_id"]) == (5, 6)
    with pytest.raises(ValueError, match="noise"):
        fft.downsample_phase_img_device(vel, mag, 1.5, ratio, 15.0, noise="torch", device="cpu")


def test_prepare_lowres_engine_is_checked():
    with pytest.raises(ValueError, match="engine"):
        prep.prepare_lowres_dataset("missing.h5", "out.h5", engine="torch")


def test_resynthesis_draws_are_private_reproducible_and_differ_across_epochs():
    umax, vmax, wmax = np.array([0.93, 1.7, 0.2, 2.6, 0.5, 1.1, 0.4]), np.array([0.55, 0.3, 0.1, 1.2, 0.5, 2.2, 0.4]), np.array([0.62, 0.9, 0.25, 0.7, 2.5, 0.3, 0.4])
    random.seed(8); np.random.seed(8)
    want_py, want_np = random.random(), np.random.random()
    random.seed(8); np.random.seed(8)
    a = prep.draw_degradations(umax, vmax, wmax, seed=1, epoch=0)
    b = prep.draw_degradations(umax, vmax, wmax, seed=1, epoch=0)
    c = prep.draw_degradations(umax, vmax, wmax, seed=1, epoch=1)
    d = prep.draw_degradations(umax, vmax, wmax, seed=2, epoch=0)
    e = prep.draw_degradations(umax, vmax, wmax, seed=1, epoch=0, ordinal=1)
    assert (random.random(), np.random.random()) == (want_py, want_np)  # the global generators were not touched
    same = lambda p, q: all(np.array_equal(x, y) for x, y in zip(p, q))
    assert same(a, b) and not same(a, c) and not same(a, d) and not same(a, e)
    snr, vencs, mags = a
    assert snr.shape == (7,) and vencs.shape == (7, 3) and mags.shape == (7,)
    assert np.all((snr >= 14.0) & (snr <= 16.9)) and np.array_equal(snr * 10, np.round(snr * 10))
    assert np.array_equal(mags, prep.MAG_VALUES[np.arange(7) % 5])
    assert np.all(np.isin(vencs, prep.VENC_VALUES))
    assert np.all(vencs > 1.1 * np.stack([umax, vmax, wmax], axis=1))   # every venc lies above the frame's (scaled) peak velocity
    # the procedure of prepare_lowres_dataset: the same draws from the global generators seeded alike give the same rows
    seq = np.random.RandomState([1, 0, 0, 0])
    assert snr[0] == seq.randint(140, 170) / 10


def test_device_loader_refuses_a_bad_resynthesize_argument_without_a_gpu():
    ddev = importlib.import_module("4dflownet_amd.data_device")
    for bad in (dict(), dict(sed=1), dict(seed=1, downsample=3)):
        with pytest.raises(ValueError, match="resynthesize"):
            ddev.DevicePatchHandler3D("/d", 12, 2, 4, device="cpu", resynthesize=bad)
    h = ddev.DevicePatchHandler3D("/d", 12, 2, 4, device="cpu", resynthesize=dict(seed=1))
    assert h.resynthesize == dict(seed=1, downsample=2)
    assert ddev.DevicePatchHandler3D("/d", 12, 2, 4, device="cpu").resynthesize is None

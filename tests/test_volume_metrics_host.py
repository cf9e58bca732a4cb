"""CPU checks of the whole-volume evaluation: the float64 yardstick (tests/_volume_metrics.py) against the project's oracle and the
divergence helper, predictor.metrics_from_sums against hand-computed values, the refusals of fdn_volume_metrics before the device is
touched (the pointers here are never dereferenced), and evaluate_file's file checks before any GPU work."""
import os
import re
from importlib import import_module

import numpy as np
import pytest

from _divergence import divergence_loss
from _volume_metrics import COLUMNS, relative_error_terms, volume_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=3, N=2, shape=(5, 4, 6)):
    """Channels-last (N,D,H,W,3) float64 prediction / truth with some truth vectors exactly zero, and a mask with 0, 1 and values between."""
    rng = np.random.default_rng(seed)
    pred = rng.uniform(-1, 1, (N,) + shape + (3,))
    truth = rng.uniform(-1, 1, (N,) + shape + (3,))
    truth[rng.random((N,) + shape) < 0.2] = 0.0                      # actual == 0: corr = diff
    mask = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], size=(N,) + shape, p=[0.3, 0.1, 0.1, 0.1, 0.4])
    return pred, truth, mask


def test_yardstick_equals_the_oracle_and_the_divergence_helper(oracle):
    predictor = import_module("4dflownet_amd.predictor")
    pred, truth, mask = _case()
    planar = lambda a: np.ascontiguousarray(np.moveaxis(a, -1, 1))  # (N,D,H,W,3) -> (F,3,X,Y,Z)
    sums, mags, band = volume_sums(planar(pred), planar(truth), mask)
    assert sums.shape == mags.shape == (2, COLUMNS) and band.shape == (2,)
    assert (band == 0).all()                                        # no rounding of corr is a coin toss: both recipes round alike
    got = predictor.metrics_from_sums(sums)
    mse, _ = oracle.masked_mse_loss_fwd_bwd(pred, truth, mask)
    rel = oracle.relative_error(pred, truth, mask)
    div, _ = divergence_loss(pred, truth, mask, 1.0)
    for f in range(2):
        assert abs(got[f]["mse"] - mse[f]) <= 1e-12 * abs(mse[f])
        assert abs(got[f]["rel_error"] - rel[f]) <= 1e-12 * abs(rel[f])
        assert abs(got[f]["div"] - div[f]) <= 1e-12 * abs(div[f])
        assert mse[f] > 0 and rel[f] > 0 and div[f] > 0
    # the term before the rounding, against the oracle's expression voxel by voxel
    raw, corr = relative_error_terms(planar(pred), planar(truth))
    diff = np.sqrt(((pred - truth) ** 2).sum(axis=-1))
    actual = np.sqrt((truth ** 2).sum(axis=-1))
    want = np.where(actual != 0, np.clip(diff / (actual + 1e-5), 0, 1), diff)
    assert np.array_equal(raw, want) and (actual == 0).any() and (raw == 1.0).any() and (raw < 1.0).any()
    assert np.array_equal(corr, np.round(want * 1e4) / 1e4)
    # a one-row mask is the same mask for every frame
    s1, _, _ = volume_sums(planar(pred), planar(truth), mask[:1])
    s2, _, _ = volume_sums(planar(pred), planar(truth), np.stack([mask[0], mask[0]]))
    assert np.array_equal(s1, s2) and not np.array_equal(s1[1], sums[1])


def test_yardstick_counts_the_voxels_whose_rounding_is_a_coin_toss():
    truth = np.zeros((1, 3, 1, 1, 2))                                # actual == 0: corr = diff = |e_u|
    pred = np.zeros((1, 3, 1, 1, 2))
    pred[0, 0, 0, 0, 0] = 0.12345                                    # 1234.5: on the half-integer
    pred[0, 0, 0, 0, 1] = 0.12344
    _, _, band = volume_sums(pred, truth, np.ones((1, 1, 1, 2)))
    assert band.tolist() == [1]
    _, _, band = volume_sums(pred, truth, np.array([0.75, 1.0]).reshape(1, 1, 1, 2))      # the voxel on the edge is not fl
    assert band.tolist() == [0]


def _sums_of(t, p, n_total=None, m_extra=0.0):
    """Sums of a frame whose fl voxels hold truth t and prediction p (each (n,3)); every other voxel has mask 0 and zero error."""
    t, p = np.asarray(t, np.float64), np.asarray(p, np.float64)
    n = len(t)
    S = np.zeros(COLUMNS)
    S[0], S[1], S[2] = n + m_extra, (n_total or n) - n, n
    e = p - t
    S[6:9] = (e ** 2).sum(axis=0)
    S[3] = S[6:9].sum()
    for c in range(3):
        S[11 + 5 * c:16 + 5 * c] = [t[:, c].sum(), p[:, c].sum(), (t[:, c] ** 2).sum(), (p[:, c] ** 2).sum(), (t[:, c] * p[:, c]).sum()]
    return S


def test_metrics_from_sums_matches_hand_computed_values():
    predictor = import_module("4dflownet_amd.predictor")
    assert len(predictor.VOLUME_SUM_NAMES) == COLUMNS == len(set(predictor.VOLUME_SUM_NAMES))
    t = np.array([[0.0, 1.0, 2.0], [1.0, 1.0, 0.0], [2.0, 1.0, 1.0], [3.0, 1.0, 4.0]])
    p = np.empty_like(t)
    p[:, 0] = 2.0 * t[:, 0] + 0.5                                    # an exact line: k 2, b 0.5, R^2 1
    p[:, 1] = [1.0, 2.0, 3.0, 4.0]                                   # the truth has no variance
    p[:, 2] = [1.0, 0.0, 2.0, 3.0]                                   # t_w = 2,0,1,4: k = 5.5/8.75, b = 1.5 - k 1.75, r^2 = 5.5^2/(8.75 5)
    S = _sums_of(t, p, n_total=10)
    S[4], S[5], S[9], S[10] = 0.75, 1.25, 3.0, 14.0
    (m,) = predictor.metrics_from_sums(S)
    assert list(m) == list(predictor.METRIC_NAMES)
    e2 = ((p - t) ** 2).sum(axis=0)
    assert m["mse"] == e2.sum() / 5 + 0.75 / 7 and m["rel_error"] == 100 * 1.25 / 5 and m["div"] == 3.0 / 5 + 14.0 / 7
    assert [m["rmse_u"], m["rmse_v"], m["rmse_w"]] == [np.sqrt(v / 4) for v in e2] and m["rmse"] == np.sqrt(e2.sum() / 4)
    assert m["n_fluid"] == 4
    assert abs(m["k_u"] - 2.0) < 1e-14 and abs(m["b_u"] - 0.5) < 1e-14 and abs(m["r2_u"] - 1.0) < 1e-14
    assert np.isnan(m["k_v"]) and np.isnan(m["b_v"]) and np.isnan(m["r2_v"])
    k = 5.5 / 8.75
    assert abs(m["k_w"] - k) < 1e-14 and abs(m["b_w"] - (1.5 - k * 1.75)) < 1e-14 and abs(m["r2_w"] - 5.5 ** 2 / (8.75 * 5.0)) < 1e-14
    # numpy's own fit agrees
    kk, bb = np.polyfit(t[:, 2], p[:, 2], 1)
    assert abs(m["k_w"] - kk) < 1e-12 and abs(m["b_w"] - bb) < 1e-12
    # no fluid voxel: RMSEs 0, regression NaN, the means still defined through their + 1
    Z = np.zeros(COLUMNS)
    Z[1], Z[4], Z[10] = 9.0, 5.0, 2.0
    (z,) = predictor.metrics_from_sums(Z.reshape(1, COLUMNS))
    assert z["rmse"] == z["rmse_u"] == z["rmse_v"] == z["rmse_w"] == 0.0 and z["n_fluid"] == 0 and z["mse"] == 0.5 and z["div"] == 0.2
    assert all(np.isnan(z[key + c]) for key in ("k_", "b_", "r2_") for c in "uvw")
    # several frames at once
    both = predictor.metrics_from_sums(np.stack([S, Z]))
    assert len(both) == 2 and both[0]["k_u"] == m["k_u"] and both[1]["mse"] == 0.5


def test_header_and_ctypes_table_hold_the_entry_point(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    assert "fdn_volume_metrics" in set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header)) and "fdn_volume_metrics" in fdn._lib.SIGNATURES
    proto = header[:header.index("int fdn_volume_metrics(")]
    comment = proto[proto.rindex("/*"):]
    for cite in ("TrainerController.py:96", "loss_utils.py:64-92", "loss_utils.py:91"):
        assert cite in comment, cite
    assert "#define FDN_VOLUME_METRICS_SCRATCH_DOUBLES(F) ((F) * FDN_VOLUME_METRICS_COLUMNS * FDN_LOSS_BLOCKS)" in header
    assert "#define FDN_VOLUME_METRICS_COLUMNS 26" in header
    ops = import_module("4dflownet_amd.ops")
    assert ops.volume_metrics_scratch_doubles(3) == 3 * 26 * 256 and ops.VOLUME_METRICS_COLUMNS == COLUMNS
    assert hasattr(fdn._lib.load(), "fdn_volume_metrics") and fdn._lib.load().fdn_version() == 161


def test_volume_metrics_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    f = lib.fdn_volume_metrics
    err = lambda: lib.fdn_last_error().decode()
    good = dict(pred=0x1000, f64=1, truth=0x2000, mask=0x3000, mf=1, out=0x4000, scratch=0x5000, F=2, X=3, Y=4, Z=5)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["pred"], a["f64"], a["truth"], a["mask"], a["mf"], a["out"], a["scratch"], a["F"], a["X"], a["Y"], a["Z"], None)

    for name in ("pred", "truth", "mask", "out", "scratch"):
        assert call(**{name: None}) == -1 and "fdn_volume_metrics" in err() and name in err() and "NULL" in err(), name
    for bad in (dict(F=0), dict(X=0), dict(Y=-1), dict(Z=0)):
        (k, v), = bad.items()
        assert call(**bad) == -1 and "fdn_volume_metrics" in err() and "%s=%d" % (k, v) in err() and "positive" in err(), bad
    assert call(X=2048, Y=1024, Z=1024) == -1 and "X*Y*Z" in err() and "2^31" in err()           # 2^31 voxels: one too many
    for mf in (0, 3, -1):
        assert call(mf=mf) == -1 and "mask_frames=%d" % mf in err() and "F=2" in err()
    for v in (2, -1):
        assert call(f64=v) == -1 and "pred_is_f64=%d" % v in err()


def test_ops_volume_metrics_refuses_host_tensors_and_bad_layouts(fdn):
    import torch
    z = torch.zeros
    with pytest.raises(fdn.FdnError, match="GPU"):
        fdn.ops.volume_metrics(z(1, 3, 2, 2, 2), z(1, 3, 2, 2, 2), z(1, 2, 2, 2))
    with pytest.raises(fdn.FdnError, match=r"\(F,3,X,Y,Z\)"):
        fdn.ops.volume_metrics(z(1, 2, 2, 2, 3), z(1, 2, 2, 2, 3), z(1, 2, 2, 2))
    with pytest.raises(fdn.FdnError, match="float32 or float64"):
        fdn.ops.volume_metrics(z(1, 3, 2, 2, 2, dtype=torch.float16), z(1, 3, 2, 2, 2), z(1, 2, 2, 2))
    with pytest.raises(fdn.FdnError, match="truth"):
        fdn.ops.volume_metrics(z(2, 3, 2, 2, 2), z(1, 3, 2, 2, 2), z(1, 2, 2, 2))
    with pytest.raises(fdn.FdnError, match="mask"):
        fdn.ops.volume_metrics(z(3, 3, 2, 2, 2), z(3, 3, 2, 2, 2), z(2, 2, 2, 2))
    with pytest.raises(fdn.FdnError, match="mask"):
        fdn.ops.volume_metrics(z(1, 3, 2, 2, 2), z(1, 3, 2, 2, 2), z(1, 2, 2, 3))


class _NoDevice:
    """A network stand-in: any use of it is a failure of the test."""
    def __getattr__(self, name):
        raise AssertionError("evaluate_file touched the network (%s) before it checked the files" % name)


def _write(h5io, path, rows, shape, mask_rows=None):
    rng = np.random.default_rng(rows + shape[0])
    tree = {n: rng.uniform(-1, 1, (rows,) + shape).astype(np.float32) for n in ("u", "v", "w")}
    if mask_rows is None:
        for n in ("u", "v", "w"):
            tree["venc_" + n] = np.full((rows,), 1.5, np.float32)
            tree["mag_" + n] = rng.uniform(0, 300, (rows,) + shape).astype(np.float32)
    else:
        tree["mask"] = (rng.random((mask_rows,) + shape) < 0.5).astype(np.float32)
    h5io.write_file(path, tree)


def test_evaluate_file_checks_the_two_files_before_any_gpu_work(tmp_path):
    predictor = import_module("4dflownet_amd.predictor")
    h5io = import_module("4dflownet_amd.h5io")
    lr = str(tmp_path / "lr.h5")
    _write(h5io, lr, 2, (4, 5, 6))
    cases = {"rows": (3, (8, 10, 12), 1, "rows"), "shape": (2, (8, 10, 13), 1, "2 x"), "factor": (2, (12, 15, 18), 2, "2 x"),
             "mask": (2, (8, 10, 12), 3, "mask")}
    for name, (rows, shape, mask_rows, word) in cases.items():
        hr = str(tmp_path / (name + ".h5"))
        _write(h5io, hr, rows, shape, mask_rows=mask_rows)
        with pytest.raises(ValueError, match=word):
            predictor.evaluate_file(_NoDevice(), lr, hr, 8, 2, verbose=False, csv_path=str(tmp_path / "never.csv"))
    assert not os.path.exists(str(tmp_path / "never.csv"))

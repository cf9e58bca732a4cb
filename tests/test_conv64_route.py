"""The fp32 64->64 route selection (conv64_mfma.hip: conv64_route) answered without a GPU: fdn_conv64_pack_streams and fdn_conv64_mask_ok
against a table recorded from the library before the selection became one function (tests/golden/make_conv64_route_golden.py), and the
model's slow-grid warning, which asks the library instead of restating its rule."""
import importlib
import json
import os
import types
import warnings

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv64_route_golden.json")


def test_pack_streams_and_mask_ok_match_the_recorded_table(fdn):
    lib = fdn._lib.load()
    ps, ok = lib.fdn_conv64_pack_streams, lib.fdn_conv64_mask_ok
    g = json.load(open(GOLDEN))
    hws = g["grid"]["HW"]
    grid = [(H, W) for H in hws for W in hws]
    bad = []
    for key, row in g["pack_streams"].items():
        N, D, algo, role = map(int, key.split())
        bad += [("pack_streams", N, D, H, W, algo, role, want, have)
                for (H, W), want in zip(grid, row) for have in [ps(N, D, H, W, algo, role)] if want != have]
    for key, row in g["mask_ok"].items():
        N, D, algo = map(int, key.split())
        bad += [("mask_ok", N, D, H, W, algo, want, have) for (H, W), want in zip(grid, row) for have in [ok(N, D, H, W, algo)] if want != have]
    for N, S, algo, *want in g["big"]:
        have = [ps(N, S, S, S, algo, role) for role in range(3)] + [ok(N, S, S, S, algo)]
        if have != want:
            bad.append(("big", N, S, algo, want, have))
    for N, D, H, W, algo, role, *want in g["invalid"]:
        have = [ps(N, D, H, W, algo, role), ok(N, D, H, W, algo)]
        if have != want:
            bad.append(("invalid", N, D, H, W, algo, role, want, have))
    assert not bad, "%d answers differ from the recorded table, first: %s" % (len(bad), bad[:10])
    assert len(g["pack_streams"]) == 3 * 2 * 5 * 3 and len(g["mask_ok"]) == 3 * 2 * 5 and len(g["big"]) == 3 * 2 * 5
    assert all(v[6] < 0 for v in g["invalid"])


def test_slow_grid_warning_follows_the_library(fdn):
    net = importlib.import_module("4dflownet_amd.network")
    assert net.slow_grid_warning(6, 18, 18, 18) is None           # W % 4 != 0: aligned 16 x 16 box on F(4,3) x F(4,3), strips direct
    assert net.slow_grid_warning(6, 16, 16, 16) is None
    msg = net.slow_grid_warning(70, 14, 6, 6)                     # too small an aligned box: all direct
    assert "direct kernels" in msg and "14x6x6" in msg and "W % 4 == 0" in msg
    msg = net.slow_grid_warning(8, 24, 23, 24)                    # odd H: 1-D Winograd
    assert "1-D Winograd" in msg and "24x23x24" in msg
    assert "1-D Winograd" in net.slow_grid_warning(1, 168, 168, 168)    # a sample above 2^22 voxels falls off the 2-D kernels


def test_slow_grid_warning_once_per_grid_above_the_size_floor(fdn):
    net = importlib.import_module("4dflownet_amd.network")
    ops = fdn.ops
    model = types.SimpleNamespace(dtype="float32", _slow_warned=set(), conv_algo={"conv3d_1": ops.ALGO_AUTO})
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        net.FlowNetModel._warn_slow_grid(model, 2, 14, 6, 6)      # 2 352 voxels: below the floor, and not marked as seen
        assert not model._slow_warned
        net.FlowNetModel._warn_slow_grid(model, 70, 14, 6, 6)
        net.FlowNetModel._warn_slow_grid(model, 70, 14, 6, 6)
        model.conv_algo = {"conv3d_1": ops.ALGO_DIRECT}
        net.FlowNetModel._warn_slow_grid(model, 8, 24, 23, 24)    # no layer on FDN_ALGO_AUTO: silent
    hits = [str(i.message) for i in w if issubclass(i.category, RuntimeWarning)]
    assert len(hits) == 1 and "14x6x6" in hits[0] and "direct kernels" in hits[0], hits

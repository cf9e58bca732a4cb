"""CPU-side checks of overlap-add stitching (tiler.PatchGenerator(blend=), fdn_input_features_volume_strided, fdn_blend_patches,
fdn_finish_volume): the plan of the overlapping window, the host tiler's patchify / patchup against tests/_blend_ref.py -- bit for bit in
float32 and within the rounding bound of the float64 sum --, the three entry points in the header and the ctypes table with every refusal
of theirs reported before the device is touched (the pointers here are never dereferenced), and ValueError for a bad blend at every
public function that takes one."""
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest

import _blend_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tiler = import_module("4dflownet_amd.tiler")
NAMES = ("u", "v", "w", "mag_u", "mag_v", "mag_w")
NEW = ("fdn_input_features_volume_strided", "fdn_input_features_volume_strided_bf16", "fdn_blend_patches", "fdn_finish_volume")
BAD_ARG = -1                                   # FDN_ERR_BAD_ARG


class _Vol:
    pass


def _dataset(frame):
    v = _Vol()
    for c, n in enumerate(NAMES):
        setattr(v, n, frame[c])
    return v


# ---- the plan ----
@pytest.mark.parametrize("P", [8, 12, 16, 24])
def test_cores_cover_the_axis_overlap_by_blend_and_none_is_spare(P):
    E = P - 4
    for b in range(1, E // 2 + 1):
        pg = tiler.PatchGenerator(P, 2, blend=b)
        s = E - b
        assert pg.stride == s and pg.blend == b
        for n in range(1, 101):
            (nr, one, _), pad, ext = pg.plan((n, 3, 3))
            assert pg.plan_blend((n, 3, 3)) == ((nr, one, one), pad, ext)
            assert (nr, s, pad[0] // 2) == br.axis_plan(n, P, b) and pad[0] % 2 == 0 and ext == (2 * n, 6, 6)
            cores = [(i * s, i * s + E) for i in range(nr)]
            cover = np.zeros(n + 2 * P, int)
            for lo, hi in cores:
                cover[lo:hi] += 1
            assert (cover[:n] >= 1).all() and cover.max() <= 2, (P, b, n)
            assert cores[-1][1] - n == pad[0] // 2 >= 0                              # the far pad is what the last core overhangs
            for (lo0, hi0), (lo1, hi1) in zip(cores, cores[1:]):
                assert hi0 - lo1 == b                                                # consecutive cores overlap by exactly b
            if nr > 1:
                assert n - cores[-1][0] > b                                          # the last core reaches beyond its overlap
            # no patch is spare.  Without the last one the end of the axis is bare; without an inner one the voxels between its two
            # ramps are -- there are E - 2b of them, so at the limit 2b == E the neighbours of an inner patch touch and only the first
            # and the last patch are irreplaceable there.
            for drop in range(nr):
                left = np.zeros(n + 2 * P, int)
                for i, (lo, hi) in enumerate(cores):
                    if i != drop:
                        left[lo:hi] += 1
                inner = 0 < drop < nr - 1
                if inner and 2 * b == E:
                    assert (left[:n] >= 1).all()
                else:
                    assert (left[:n] == 0).any(), (P, b, n, drop)


def _reference_rule_counts(n, P):
    """The plan of the window without overlap, as the reference pads (PatchGenerator.py:53-86): written out here, not taken from the tiler."""
    E = P - 4
    padded = n + 4
    res = padded % E
    far = P - res if res > 4 else 4 - res
    return (padded + far - 4) // E, far


@pytest.mark.parametrize("P", [8, 12, 16, 24])
def test_blend_zero_is_the_existing_plan(P):
    old, new = tiler.PatchGenerator(P, 2), tiler.PatchGenerator(P, 2, blend=0)
    assert new.blend == 0 and new.stride == P - 4
    for n in range(1, 101):
        shape = (n, (n * 7) % 31 + 1, 5)
        assert old.plan(shape) == new.plan(shape)
        nr, pad, ext = new.plan(shape)
        want = [_reference_rule_counts(m, P) for m in shape]
        assert nr == tuple(w[0] for w in want) and pad == tuple(2 * w[1] for w in want) and ext == tuple(2 * m for m in shape)
        if P > 8:                                                        # E > 4: the rule of the overlapping window at b = 0 agrees
            assert nr[0] == br.axis_plan(n, P, 0)[0]
    if P == 8:                                                           # ... and at P = 8 it does not: the reference adds a patch
        assert new.plan((8, 8, 8))[0][0] == br.axis_plan(8, 8, 0)[0] + 1


def test_blend_zero_patchify_and_patchup_are_the_existing_ones():
    rng = np.random.default_rng(3)
    frame = rng.standard_normal((6, 9, 6, 5)).astype(np.float32)
    old, new = tiler.PatchGenerator(8, 2), tiler.PatchGenerator(8, 2, blend=0)
    a, b = old.patchify(_dataset(frame)), new.patchify(_dataset(frame))
    assert all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a[0] + a[1], b[0] + b[1]))
    assert (old.nr_x, old.nr_y, old.nr_z, old.padding) == (new.nr_x, new.nr_y, new.nr_z, new.padding)
    pred = rng.standard_normal((len(a[0][0]), 16, 16, 16)).astype(np.float64)
    assert old._patchup_with_overlap(pred, old.nr_x, old.nr_y, old.nr_z).tobytes() == new._patchup_with_overlap(pred, new.nr_x, new.nr_y, new.nr_z).tobytes()


# ---- patchify and patchup ----
CASES = [(8, 2, 1, (9, 6, 5)), (8, 2, 2, (9, 6, 5)), (8, 4, 1, (9, 6, 5)), (12, 2, 4, (9, 6, 5)), (12, 2, 2, (12, 20, 5))]


@pytest.mark.parametrize("P,R,b,shape", CASES)
def test_patchify_reads_the_overlapping_window(P, R, b, shape):
    rng = np.random.default_rng(P + b)
    frame = rng.standard_normal((6,) + shape).astype(np.float32)
    pg = tiler.PatchGenerator(P, R, blend=b)
    vel, mag = pg.patchify(_dataset(frame))
    nr = br.counts(shape, P, b)
    assert (pg.nr_x, pg.nr_y, pg.nr_z) == nr == pg.plan(shape)[0] and pg.padding == pg.plan(shape)[1]
    for c, stack in enumerate(vel + mag):
        want = br.patches(frame[c], P, b)
        assert stack.shape == want.shape + (1,) and stack.dtype == np.float32 and stack[..., 0].tobytes() == want.tobytes(), c


def _upsample(a, R, axes):
    for ax in axes:
        a = np.repeat(a, R, axis=ax)
    return a


@pytest.mark.parametrize("P,R,b,shape", CASES)
def test_patches_that_upsample_their_own_input_give_the_upsampled_volume(P, R, b, shape):
    rng = np.random.default_rng(10 * P + b)
    frame = rng.standard_normal((6,) + shape).astype(np.float32)
    pg = tiler.PatchGenerator(P, R, blend=b)
    vel, _ = pg.patchify(_dataset(frame))
    pred = _upsample(vel[0][..., 0], R, (1, 2, 3))                               # (n,S,S,S): nearest neighbour of the patch's own input
    got = pg._patchup_with_overlap(pred, pg.nr_x, pg.nr_y, pg.nr_z)
    want = _upsample(frame[0], R, (0, 1, 2)).astype(np.float64)
    assert got.shape == want.shape and got.dtype == np.float32
    # every covering patch holds the same value v at a voxel and the weights sum to 1: the sum is v, sum w |p| is |v|
    err = np.abs(got.astype(np.float64) - want)
    print("largest error: %.2f x 2^-24 |v|" % float((err[want != 0] / (br.EPS * np.abs(want[want != 0]))).max()))
    assert (err <= br.BOUND_ROUNDINGS * br.EPS * np.abs(want)).all()


def test_two_patches_of_constants_give_the_linear_ramp():
    """P = 8, b = 2, R = 2 over 6 x 4 x 4 voxels: two patches along x and one along y and z.  C = 8, ramp r = 4, HR stride 4: patch 0 holds a
    = 1, patch 1 holds b = 3, and over the four shared voxels the volume climbs a + (b - a)(2t + 1)/8 -- eighths, exact in float32."""
    pg = tiler.PatchGenerator(8, 2, blend=2)
    nr, pad, ext = pg.plan((6, 4, 4))
    assert nr == (2, 1, 1) and pad == (0, 0, 0) and ext == (12, 8, 8)
    pg.padding = pad
    pred = np.empty((2, 16, 16, 16), np.float32)
    pred[0], pred[1] = 1.0, 3.0
    got = pg._patchup_with_overlap(pred, *nr)
    want = np.array([1, 1, 1, 1, 1.25, 1.75, 2.25, 2.75, 3, 3, 3, 3], np.float32)
    assert got.shape == (12, 8, 8) and np.array_equal(got, np.broadcast_to(want[:, None, None], got.shape))


@pytest.mark.parametrize("P,R,b,shape", CASES)
def test_the_tilers_volume_equals_the_reference_bit_for_bit_and_keeps_the_float64_bound(P, R, b, shape):
    rng = np.random.default_rng(100 * P + b)
    pg = tiler.PatchGenerator(P, R, blend=b)
    nr, pad, ext = pg.plan(shape)
    pg.padding = pad
    n = nr[0] * nr[1] * nr[2]
    S = P * R
    pred = rng.standard_normal((n, S, S, S, 3)).astype(np.float32)               # mixed sign
    want32 = br.blend32(pred, 1, nr, 2 * R, (P - 4 - b) * R, ext)
    val64, mag64 = br.blend64(pred, 1, nr, 2 * R, (P - 4 - b) * R, ext)
    for dtype in (np.float32, np.float64):                                       # predict_patches hands float64 that holds fp32 values
        for c in range(3):
            got = pg._patchup_with_overlap(pred[..., c].astype(dtype), *nr)
            assert got.dtype == dtype and got.shape == ext
            assert br.same_bits(got.astype(np.float32), want32[0, c]), (dtype, c)
    ok, worst = br.within_bound(want32, val64, mag64)
    print("largest error: %.2f x 2^-24 sum w|p|" % worst)
    assert ok, worst
    # unpatchify is the same stitch per component
    pg.nr_x, pg.nr_y, pg.nr_z = nr
    u, v, w = pg.unpatchify(pred)
    assert br.same_bits(v, want32[0, 1])


# ---- the ABI ----
def test_header_and_ctypes_table_hold_the_new_entry_points(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    lib = fdn._lib.load()
    for n in NEW:
        assert n in declared and n in fdn._lib.SIGNATURES and hasattr(lib, n), n
    assert declared == set(fdn._lib.SIGNATURES)
    sig = fdn._lib.SIGNATURES
    assert sig["fdn_input_features_volume_strided"] == sig["fdn_input_features_volume_strided_bf16"]
    oriented = sig["fdn_input_features_volume_oriented"][1]
    assert sig["fdn_input_features_volume_strided"][1] == oriented[:11] + [fdn._lib.c_i] + oriented[11:]       # + the stride
    stitch = sig["fdn_stitch_patches"][1]
    assert sig["fdn_blend_patches"][1] == stitch[:8] + [fdn._lib.c_i] + stitch[8:]                             # + stride_hr behind side
    assert fdn._lib.FDN_VERSION == 161 == lib.fdn_version()


@pytest.mark.parametrize("name", NEW[:2])
def test_strided_features_refuse_bad_arguments_before_they_touch_the_device(fdn, name):
    lib = fdn._lib.load()
    fn = getattr(lib, name)
    err = lambda: lib.fdn_last_error().decode()
    good = dict(frames=0x1000, F=2, X=9, Y=6, Z=5, P=8, nx=3, ny=2, nz=2, g0=0, count=24, stride=3, plane=0, k=0, phase=0x2000, pc=0x3000)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["frames"], a["F"], a["X"], a["Y"], a["Z"], a["P"], a["nx"], a["ny"], a["nz"], a["g0"], a["count"], a["stride"],
                  a["plane"], a["k"], a["phase"], a["pc"], None)

    for stride in (0, -1, 5, 8):                                                 # stride < 1, stride > P - 4
        assert call(stride=stride) == BAD_ARG and name + ":" in err() and "stride=%d" % stride in err(), stride
    assert call(P=12, stride=9) == BAD_ARG and "stride=9" in err()
    # ... and everything the oriented entry point refuses
    for bad in (dict(frames=None), dict(phase=None), dict(pc=None)):
        assert call(**bad) == BAD_ARG and name + ":" in err() and "NULL" in err(), bad
    for bad in (dict(F=0), dict(X=0), dict(Y=-1), dict(Z=0), dict(P=4), dict(nx=0), dict(ny=0), dict(nz=-2), dict(count=0), dict(g0=-1),
                dict(g0=20, count=5), dict(plane=1, k=0), dict(plane=0, k=2), dict(plane=4, k=1)):
        assert call(**bad) == BAD_ARG and name + ":" in err(), bad


def test_blend_patches_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    name = "fdn_blend_patches"
    err = lambda: lib.fdn_last_error().decode()
    # P = 8, R = 2, b = 1 over (9,6,5): counts (3,2,2), S = 16, side 4, core 8, HR stride 6; covered extents (20,14,14)
    good = dict(pred=0x1000, acc=0x2000, F=2, Xo=18, Yo=12, Zo=10, S=16, side=4, stride=6, nx=3, ny=2, nz=2, g0=0, count=24)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fdn_blend_patches(a["pred"], a["acc"], a["F"], a["Xo"], a["Yo"], a["Zo"], a["S"], a["side"], a["stride"], a["nx"],
                                     a["ny"], a["nz"], a["g0"], a["count"], None)

    # the refusals of fdn_stitch_patches
    for bad in (dict(pred=None), dict(acc=None)):
        assert call(**bad) == BAD_ARG and name in err() and "NULL" in err(), bad
    for S, side in ((8, 4), (7, 4), (16, 8), (0, 0), (513, 0)):
        assert call(S=S, side=side) == BAD_ARG and name in err() and "S=%d" % S in err(), (S, side)
    assert call(side=-1) == BAD_ARG and name in err() and "side=-1" in err()
    for count in (0, -1):
        assert call(count=count) == BAD_ARG and name in err() and "count=%d" % count in err()
    assert call(g0=-2) == BAD_ARG and name in err() and "g0=-2" in err()
    assert call(g0=20, count=5) == BAD_ARG and name in err() and "[20, 25)" in err()
    for bad in (dict(F=0), dict(nx=0), dict(ny=-1), dict(nz=0)):
        assert call(**bad) == BAD_ARG and name in err(), bad
    for bad in (dict(Xo=0), dict(Yo=-4), dict(Zo=0)):
        assert call(**bad) == BAD_ARG and name in err() and "extents" in err(), bad
    # output extents the counts do not cover: (n - 1) * stride_hr + core per axis
    for bad in (dict(Xo=21), dict(Yo=15), dict(Zo=15)):
        assert call(**bad) == BAD_ARG and name in err() and "extents" in err(), bad
    # the stride
    for stride in (0, -3):                                                       # stride_hr < 1
        assert call(stride=stride) == BAD_ARG and name in err() and "stride_hr=%d" % stride in err(), stride
    assert call(stride=9) == BAD_ARG and name in err() and "stride_hr=9" in err()            # stride_hr > S - 2*side
    assert call(stride=3) == BAD_ARG and name in err() and "more than two cores" in err()    # 2 * (8 - 3) > 8
    # side 0 (packed cores, S = core 8): the same limits
    for bad in (dict(Xo=21), dict(stride=9), dict(stride=3), dict(stride=0)):
        assert call(S=8, side=0, **bad) == BAD_ARG and name in err(), bad


def test_finish_volume_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    err = lambda: lib.fdn_last_error().decode()
    good = dict(acc=0x1000, vol=0x2000, scale=0x3000, F=2, Xo=18, Yo=12, Zo=10)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fdn_finish_volume(a["acc"], a["vol"], a["scale"], a["F"], a["Xo"], a["Yo"], a["Zo"], None)

    for bad in (dict(acc=None), dict(vol=None), dict(scale=None)):
        assert call(**bad) == BAD_ARG and "fdn_finish_volume" in err() and "NULL" in err(), bad
    for bad in (dict(F=0), dict(Xo=0), dict(Yo=-1), dict(Zo=0)):
        assert call(**bad) == BAD_ARG and "fdn_finish_volume" in err(), bad


def test_ops_refuse_host_tensors_and_bad_layouts(fdn):
    import torch
    ops, ops_bf16 = fdn.ops, import_module("4dflownet_amd.ops_bf16")
    assert ops_bf16.blend_patches is ops.blend_patches and ops_bf16.finish_volume is ops.finish_volume      # fp32 in both modes
    assert inspect.signature(ops.input_features_volume) == inspect.signature(ops_bf16.input_features_volume)
    assert inspect.signature(ops.input_features_volume).parameters["stride"].default is None
    frames = torch.zeros(1, 6, 4, 4, 4)
    for m in (ops, ops_bf16):
        for stride in (0, 5, -1, 2.0, True, "2"):
            with pytest.raises(ValueError, match="stride"):
                m.input_features_volume(frames, 8, (2, 2, 2), stride=stride)
        with pytest.raises(fdn.FdnError, match="GPU"):
            m.input_features_volume(frames, 8, (2, 2, 2), stride=3)
    with pytest.raises(fdn.FdnError, match=r"\(count,S,S,S,3\)"):
        ops.blend_patches(torch.zeros(2, 16, 16, 15, 3), torch.zeros(1, 3, 8, 8, 8), 4, 6, (1, 1, 1))
    with pytest.raises(fdn.FdnError, match=r"\(F,3,Xo,Yo,Zo\)"):
        ops.blend_patches(torch.zeros(2, 16, 16, 16, 3), torch.zeros(1, 8, 8, 8), 4, 6, (1, 1, 1))
    with pytest.raises(fdn.FdnError, match="GPU"):
        ops.blend_patches(torch.zeros(1, 16, 16, 16, 3), torch.zeros(1, 3, 8, 8, 8), 4, 6, (1, 1, 1))
    scale = torch.ones(1, 2, dtype=torch.float64)
    with pytest.raises(fdn.FdnError, match=r"\(F,2\)"):
        ops.finish_volume(torch.zeros(2, 3, 8, 8, 8), scale)
    with pytest.raises(fdn.FdnError, match="out must be"):
        ops.finish_volume(torch.zeros(1, 3, 8, 8, 8), scale, out=torch.zeros(1, 3, 8, 8, 7, dtype=torch.float64))
    with pytest.raises(fdn.FdnError, match="GPU"):
        ops.finish_volume(torch.zeros(1, 3, 8, 8, 8), scale)


# ---- a bad blend ----
BAD_BLENDS = (-1, 3, 2.0, "2", None, True)          # P = 8: 2 * 3 > 4


def test_a_bad_blend_raises_value_error_at_every_public_function_that_takes_it(fdn, tmp_path):
    predictor = import_module("4dflownet_amd.predictor")
    frames = np.zeros((1, 6, 4, 4, 4), np.float32)
    missing = str(tmp_path / "missing.h5")
    for bad in BAD_BLENDS:
        with pytest.raises(ValueError, match="blend"):
            tiler.PatchGenerator(8, 2, blend=bad)
        # before the network, the frames or a file are touched: None stands in for the network, the files do not exist
        with pytest.raises(ValueError, match="blend"):
            predictor.predict_volume(None, frames, 8, 4, blend=bad)
        with pytest.raises(ValueError, match="blend"):
            predictor.predict_cores(None, frames, 8, 4, 0, 1, blend=bad)
        with pytest.raises(ValueError, match="blend"):
            predictor.predict_file(None, missing, missing, 8, 2, blend=bad)
        with pytest.raises(ValueError, match="blend"):
            predictor.evaluate_file(None, missing, missing, 8, 2, blend=bad)
        with pytest.raises(ValueError, match="blend"):
            predictor.main(patch_size=8, blend=bad)
        with pytest.raises(ValueError, match="blend"):
            predictor.evaluate_main(patch_size=8, blend=bad)
    for ok in (0, 1, 2, np.int64(2)):
        assert tiler.PatchGenerator(8, 2, blend=ok).blend == int(ok)
    assert tiler.PatchGenerator(24, 2, blend=10).stride == 10
    with pytest.raises(ValueError, match="blend"):
        tiler.PatchGenerator(24, 2, blend=11)
    for fn in (predictor.predict_volume, predictor.predict_cores, predictor.predict_file, predictor.evaluate_file, predictor.main,
               predictor.evaluate_main, predictor._predict_file_device):
        assert inspect.signature(fn).parameters["blend"].default == 0, fn.__name__


def test_the_scripts_read_the_blend_switch():
    import importlib.util
    for script in ("predictor.py", "evaluate.py"):
        spec = importlib.util.spec_from_file_location("blend_script_" + script[:-3], os.path.join(ROOT, "scripts", script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)                                             # the __main__ guard keeps it from running
        assert mod._blend([]) == 0 and mod._blend(["--self-ensemble"]) == 0
        assert mod._blend(["--blend", "4"]) == 4 and mod._blend(["--self-ensemble", "rot90", "--blend", "2"]) == 2
        for argv in (["--blend"], ["--blend", "two"], ["--blend", "--self-ensemble"]):
            with pytest.raises(SystemExit):
                mod._blend(argv)

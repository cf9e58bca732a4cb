"""CPU-side checks of the device tiler's boundary: PatchGenerator.plan against patchify, the three new entry points in the header and the
ctypes table, and every argument error of theirs reported before the device is touched (the pointers here are never dereferenced)."""
import os
import re
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdn_input_features_volume", "fdn_input_features_volume_bf16", "fdn_stitch_patches")
# (P, R, LR shape): both branches of _far_pad and a zero far pad on one axis (12,3,(9,8,17)); the example volume; a volume with a fully
# cropped patch (8,2,(4,4,4)); one patch along an axis (12,2,(12,20,5))
CASES = [(8, 2, (7, 10, 13)), (12, 3, (9, 8, 17)), (24, 2, (42, 38, 36)), (8, 2, (4, 4, 4)), (12, 2, (12, 20, 5))]


class _Vol:
    pass


@pytest.mark.parametrize("P,R,shape", CASES)
def test_plan_equals_what_patchify_reports(P, R, shape):
    tiler = import_module("4dflownet_amd.tiler")
    rng = np.random.default_rng(1)
    v = _Vol()
    for n in ("u", "v", "w", "mag_u", "mag_v", "mag_w"):
        setattr(v, n, rng.uniform(-1, 1, shape).astype(np.float32))
    pg = tiler.PatchGenerator(P, R)
    vel, _ = pg.patchify(v)
    counts, padding, extents = tiler.PatchGenerator(P, R).plan(shape)          # a fresh generator: from the shape alone
    assert counts == (pg.nr_x, pg.nr_y, pg.nr_z) and padding == pg.padding
    assert len(vel[0]) == counts[0] * counts[1] * counts[2]
    assert extents == tuple(R * n for n in shape)
    S = P * R
    stitched = pg._patchup_with_overlap(np.zeros((len(vel[0]), S, S, S)), *counts)
    assert stitched.shape == extents
    assert (pg.nr_x, pg.nr_y, pg.nr_z) == counts and pg.padding == padding          # plan() left the generator's state alone


def test_header_and_ctypes_table_hold_the_three_entry_points(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    for n in NAMES:
        assert n in declared and n in fdn._lib.SIGNATURES, n
        proto = header[:header.index("int " + n + "(")]
        comment = proto[proto.rindex("/*"):]
        assert "PatchGenerator.py:13-40,53-86,116-154" in comment and "predictor.py:67-115" in comment, n
    assert fdn._lib.SIGNATURES["fdn_input_features_volume"][1] == fdn._lib.SIGNATURES["fdn_input_features_volume_bf16"][1]
    for n in NAMES:
        assert hasattr(fdn._lib.load(), n)


@pytest.mark.parametrize("name", NAMES[:2])
def test_input_features_volume_refuses_bad_arguments_before_it_touches_the_device(fdn, name):
    lib = fdn._lib.load()
    f = getattr(lib, name)
    err = lambda: lib.fdn_last_error().decode()
    frames, phase, pc = 0x1000, 0x2000, 0x3000
    good = dict(frames=frames, F=2, X=7, Y=10, Z=13, P=8, nx=2, ny=3, nz=4, g0=0, count=48, phase=phase, pc=pc)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["frames"], a["F"], a["X"], a["Y"], a["Z"], a["P"], a["nx"], a["ny"], a["nz"], a["g0"], a["count"], a["phase"], a["pc"], None)

    for bad in (dict(frames=None), dict(phase=None), dict(pc=None)):
        assert call(**bad) == -1 and name in err() and "NULL" in err(), bad
    for P in (4, 0, -8):
        assert call(P=P) == -1 and name in err() and "P=%d" % P in err()
    for count in (0, -3):
        assert call(count=count) == -1 and name in err() and "count=%d" % count in err()
    assert call(g0=-1) == -1 and name in err() and "g0=-1" in err()
    assert call(g0=1) == -1 and name in err() and "[1, 49)" in err() and "48" in err()          # g0 + count > F*nx*ny*nz
    assert call(g0=47, count=2) == -1 and "[47, 49)" in err()
    for bad in (dict(F=0), dict(X=0), dict(Y=-1), dict(Z=0)):
        assert call(**bad) == -1 and name in err() and "frames" in err(), bad
    for bad in (dict(nx=0), dict(ny=0), dict(nz=-2)):
        assert call(**bad) == -1 and name in err() and "counts" in err(), bad


def test_stitch_patches_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    f = lib.fdn_stitch_patches
    err = lambda: lib.fdn_last_error().decode()
    good = dict(pred=0x1000, vol=0x2000, F=2, Xo=14, Yo=20, Zo=26, S=16, side=4, nx=2, ny=3, nz=4, g0=0, count=48)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["pred"], a["vol"], a["F"], a["Xo"], a["Yo"], a["Zo"], a["S"], a["side"], a["nx"], a["ny"], a["nz"], a["g0"], a["count"], None)

    for bad in (dict(pred=None), dict(vol=None)):
        assert call(**bad) == -1 and "fdn_stitch_patches" in err() and "NULL" in err(), bad
    for S, side in ((8, 4), (7, 4), (16, 8), (0, 0)):                      # S <= 2*side
        assert call(S=S, side=side) == -1 and "fdn_stitch_patches" in err() and "S=%d" % S in err(), (S, side)
    for count in (0, -1):
        assert call(count=count) == -1 and "count=%d" % count in err()
    assert call(g0=-2) == -1 and "g0=-2" in err()
    assert call(g0=40, count=9) == -1 and "[40, 49)" in err()
    # extents: (nx,ny,nz) * core = (16,24,32) is the most the patches can fill
    for bad in (dict(Xo=17), dict(Yo=25), dict(Zo=33), dict(Xo=0), dict(Yo=-4), dict(Zo=0)):
        assert call(**bad) == -1 and "fdn_stitch_patches" in err() and "extents" in err(), bad
    for bad in (dict(F=0), dict(nx=0), dict(ny=-1), dict(nz=0)):
        assert call(**bad) == -1 and "fdn_stitch_patches" in err(), bad


def test_ops_refuse_host_tensors_and_bad_layouts(fdn):
    """No CPU fallback, and the shape checks of the operator layer come before the library."""
    import torch
    with pytest.raises(fdn.FdnError, match="GPU"):
        fdn.ops.input_features_volume(torch.zeros(1, 6, 4, 4, 4), 8, (2, 2, 2), phase=torch.zeros(8, 8, 8, 8, 3), pc=torch.zeros(8, 8, 8, 8, 3))
    with pytest.raises(fdn.FdnError, match=r"\(F,6,X,Y,Z\)"):
        fdn.ops.input_features_volume(torch.zeros(1, 5, 4, 4, 4), 8, (2, 2, 2))
    with pytest.raises(fdn.FdnError, match=r"\(F,6,X,Y,Z\)"):
        import_module("4dflownet_amd.ops_bf16").input_features_volume(torch.zeros(6, 4, 4, 4), 8, (2, 2, 2))
    with pytest.raises(fdn.FdnError, match=r"\(count,S,S,S,3\)"):
        fdn.ops.stitch_patches(torch.zeros(2, 16, 16, 15, 3), torch.zeros(1, 3, 8, 8, 8), 4, (2, 2, 2))
    with pytest.raises(fdn.FdnError, match=r"\(F,3,Xo,Yo,Zo\)"):
        fdn.ops.stitch_patches(torch.zeros(2, 16, 16, 16, 3), torch.zeros(3, 8, 8, 8), 4, (2, 2, 2))
    with pytest.raises(fdn.FdnError, match="GPU"):
        fdn.ops.stitch_patches(torch.zeros(2, 16, 16, 16, 3), torch.zeros(1, 3, 8, 8, 8), 4, (2, 2, 2))

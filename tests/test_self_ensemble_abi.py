"""CPU-side checks of the self-ensemble's boundary: the three entry points in the header and the ctypes table, every argument error of
theirs reported as FDN_ERR_BAD_ARG with the function and the argument named before the device is touched (the pointers here are never
dereferenced), and the refusals of the operator layer."""
import os
import re
from importlib import import_module

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIENTED = ("fdn_input_features_volume_oriented", "fdn_input_features_volume_oriented_bf16")
NAMES = ORIENTED + ("fdn_unrotate_accumulate",)
BAD_ARG = -1                                                                # FDN_ERR_BAD_ARG
VALID = [(0, 0)] + [(p, k) for p in (1, 2, 3) for k in (1, 2, 3)]
INVALID = [(0, 1), (0, 3), (1, 0), (3, 0), (4, 1), (1, 4), (-1, 1), (2, -2), (4, 0)]


def test_header_and_ctypes_table_hold_the_three_entry_points(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    assert re.search(r"#define FDN_ERR_BAD_ARG\s+\(?-1\)?", header) or re.search(r"FDN_ERR_BAD_ARG\s*=\s*-1", header)
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    lib = fdn._lib.load()
    for n in NAMES:
        assert n in declared and n in fdn._lib.SIGNATURES, n
        assert hasattr(lib, n), n
        proto = header[:header.index("int " + n + "(")]
        assert "PatchHandler3D.py:97-108,166-274" in proto[proto.rindex("/*"):], n          # the contract names what it mirrors
    assert declared == set(fdn._lib.SIGNATURES)
    sig = fdn._lib.SIGNATURES
    assert sig[ORIENTED[0]][1] == sig[ORIENTED[1]][1]
    # the oriented form is the volume form with (plane, k) in front of the outputs
    base = sig["fdn_input_features_volume"][1]
    assert sig[ORIENTED[0]][1] == base[:11] + [fdn._lib.c_i, fdn._lib.c_i] + base[11:]
    assert len(sig["fdn_unrotate_accumulate"][1]) == 9
    header_version = int(re.search(r"#define FDN_VERSION (\d+)", header).group(1))
    assert lib.fdn_version() == header_version == fdn._lib.FDN_VERSION


@pytest.mark.parametrize("name", ORIENTED)
def test_oriented_features_refuse_bad_arguments_before_they_touch_the_device(fdn, name):
    lib = fdn._lib.load()
    f = getattr(lib, name)
    err = lambda: lib.fdn_last_error().decode()
    good = dict(frames=0x1000, F=2, X=7, Y=10, Z=13, P=8, nx=2, ny=3, nz=4, g0=0, count=48, plane=2, k=3, phase=0x2000, pc=0x3000)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["frames"], a["F"], a["X"], a["Y"], a["Z"], a["P"], a["nx"], a["ny"], a["nz"], a["g0"], a["count"], a["plane"], a["k"],
                 a["phase"], a["pc"], None)

    def named(rc):                                   # the function under its own name, not the plain one's
        return rc == BAD_ARG and err().startswith(name + ":")

    for bad in (dict(frames=None), dict(phase=None), dict(pc=None)):
        assert named(call(**bad)) and "NULL" in err(), bad
    for P in (4, 0, -8):
        assert named(call(P=P)) and "P=%d" % P in err()
    for bad in (dict(F=0), dict(X=0), dict(Y=-1), dict(Z=0)):
        assert named(call(**bad)) and "frames" in err(), bad
    for bad in (dict(nx=0), dict(ny=0), dict(nz=-2)):
        assert named(call(**bad)) and "counts" in err(), bad
    for count in (0, -3):
        assert named(call(count=count)) and "count=%d" % count in err()
    assert named(call(g0=-1)) and "g0=-1" in err()
    assert named(call(g0=1)) and "[1, 49)" in err() and "48" in err()                  # g0 + count > F*nx*ny*nz
    assert named(call(g0=47, count=2)) and "[47, 49)" in err()
    for plane, k in INVALID:
        assert named(call(plane=plane, k=k)) and "orientation" in err() and "plane=%d" % plane in err() and "k=%d" % k in err(), (plane, k)
    # a valid orientation with one bad argument more is still refused for that argument: nothing is launched for any of the ten
    for plane, k in VALID:
        assert named(call(plane=plane, k=k, count=0)) and "count=0" in err(), (plane, k)


def test_unrotate_accumulate_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    name = "fdn_unrotate_accumulate"
    err = lambda: lib.fdn_last_error().decode()
    bytes_ = 3 * 6 * 6 * 6 * 3 * 4
    good = dict(pred=0x100000, acc=0x200000, count=3, S=6, plane=1, k=2, first=0, divisor=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fdn_unrotate_accumulate(a["pred"], a["acc"], a["count"], a["S"], a["plane"], a["k"], a["first"], a["divisor"], None)

    def named(rc):
        return rc == BAD_ARG and err().startswith(name + ":")

    for bad in (dict(pred=None), dict(acc=None)):
        assert named(call(**bad)) and "NULL" in err(), bad
    for count in (0, -2):
        assert named(call(count=count)) and "count=%d" % count in err()
    for S in (0, -6, 513, 4096):
        assert named(call(S=S)) and "S=%d" % S in err()
    for plane, k in INVALID:
        assert named(call(plane=plane, k=k)) and "orientation" in err() and "plane=%d" % plane in err() and "k=%d" % k in err(), (plane, k)
    for first in (2, -1, 10):
        assert named(call(first=first)) and "first=%d" % first in err()
    for divisor in (0, -1, -10):
        assert named(call(divisor=divisor)) and "divisor=%d" % divisor in err()
    # overlapping ranges: the same buffer, acc inside pred's range from either side, one byte of overlap at either end
    base = good["pred"]
    for acc in (base, base + 4, base + bytes_ - 4, base - 4, base - bytes_ + 4):
        assert named(call(acc=acc)) and "overlap" in err(), acc - base
    for plane, k in VALID:                                                  # as above: refused for the other argument
        assert named(call(plane=plane, k=k, divisor=0)) and "divisor=0" in err(), (plane, k)
    # touching ranges do not overlap; S = 512 is inside the limit: neither is refused for THAT reason (they fail on a later check)
    assert named(call(acc=base + bytes_, first=7)) and "first=7" in err()
    assert named(call(acc=base - bytes_, first=7)) and "first=7" in err()
    assert named(call(S=512, acc=1 << 44, first=7)) and "first=7" in err()


def test_the_plain_entry_points_keep_their_names_and_refusals(fdn):
    lib = fdn._lib.load()
    err = lambda: lib.fdn_last_error().decode()
    for name in ("fdn_input_features_volume", "fdn_input_features_volume_bf16"):
        f = getattr(lib, name)
        assert f(None, 2, 7, 10, 13, 8, 2, 3, 4, 0, 48, 0x2000, 0x3000, None) == BAD_ARG and err().startswith(name + ":") and "NULL" in err()
        assert f(0x1000, 2, 7, 10, 13, 4, 2, 3, 4, 0, 48, 0x2000, 0x3000, None) == BAD_ARG and err().startswith(name + ":") and "P=4" in err()


def test_ops_refuse_host_tensors_bad_layouts_and_bad_orientations(fdn):
    """No CPU fallback, and the checks of the operator layer come before the library."""
    import torch
    ops = fdn.ops
    ops_bf16 = import_module("4dflownet_amd.ops_bf16")
    frames = torch.zeros(1, 6, 4, 4, 4)
    for m in (ops, ops_bf16):
        for bad in ((0, 1), (1, 0), (4, 1), (1,), "rot90", 3):
            with pytest.raises(ValueError, match="orientation"):
                m.input_features_volume(frames, 8, (2, 2, 2), orientation=bad)
        with pytest.raises(fdn.FdnError, match="GPU"):
            m.input_features_volume(frames, 8, (2, 2, 2), orientation=(2, 1))
        with pytest.raises(fdn.FdnError, match=r"\(F,6,X,Y,Z\)"):
            m.input_features_volume(torch.zeros(1, 5, 4, 4, 4), 8, (2, 2, 2), orientation=(2, 1))
    pred, acc = torch.zeros(2, 6, 6, 6, 3), torch.zeros(2, 6, 6, 6, 3)
    with pytest.raises(fdn.FdnError, match="GPU"):
        ops.unrotate_accumulate(pred, acc, (1, 1), True)
    with pytest.raises(fdn.FdnError, match=r"\(count,S,S,S,3\)"):
        ops.unrotate_accumulate(torch.zeros(2, 6, 6, 5, 3), acc, (1, 1), True)
    with pytest.raises(fdn.FdnError, match="like pred"):
        ops.unrotate_accumulate(pred, torch.zeros(3, 6, 6, 6, 3), (1, 1), True)
    with pytest.raises(ValueError, match="orientation"):
        ops.unrotate_accumulate(pred, acc, (0, 2), True)
    assert ops_bf16.unrotate_accumulate is ops.unrotate_accumulate                      # the prediction is fp32 in both modes

"""CPU-side checks of the data-parallel device tiler's boundary: fdn_pack_patch_cores and fdn_stitch_patches_finish in the header and the
ctypes table, every argument error of theirs reported before the device is touched (the pointers here are never dereferenced), the
refusals of the operator layer, and the shard arithmetic of predictor._predict_file_device (shard_bounds, shard_frame_span)."""
import os
import re
from importlib import import_module

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fdn_pack_patch_cores", "fdn_stitch_patches_finish")


def test_header_and_ctypes_table_hold_the_two_entry_points(fdn):
    header = open(os.path.join(ROOT, "include", "fdn.h")).read()
    declared = set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", header))
    for n in NAMES:
        assert n in declared and n in fdn._lib.SIGNATURES, n
        proto = header[:header.index("int " + n + "(")]
        comment = proto[proto.rindex("/*"):]
        assert "predictor.py:103-107" in comment, n
        assert hasattr(fdn._lib.load(), n)
    finish = header[:header.index("int fdn_stitch_patches_finish(")]
    assert "ImageDataset.py:31" in finish[finish.rindex("/*"):]
    # the finish entry point is fdn_stitch_patches with a float64 volume and one more pointer
    sig, base = fdn._lib.SIGNATURES["fdn_stitch_patches_finish"], fdn._lib.SIGNATURES["fdn_stitch_patches"]
    assert sig[0] == base[0] and len(sig[1]) == len(base[1]) + 1 and sig[1][3:] == base[1][2:]
    assert declared == set(fdn._lib.SIGNATURES)


def test_pack_patch_cores_refuses_bad_arguments_before_it_touches_the_device(fdn):
    lib = fdn._lib.load()
    err = lambda: lib.fdn_last_error().decode()
    good = dict(pred=0x1000, cores=0x2000, S=16, side=4, count=5)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fdn_pack_patch_cores(a["pred"], a["cores"], a["S"], a["side"], a["count"], None)

    for bad in (dict(pred=None), dict(cores=None)):
        assert call(**bad) == -1 and "fdn_pack_patch_cores" in err() and "NULL" in err(), bad
    for S, side in ((8, 4), (7, 4), (16, 8), (0, 0), (513, 2), (600, 0)):            # S <= 2*side, S > 512
        assert call(S=S, side=side) == -1 and "fdn_pack_patch_cores" in err() and "S=%d" % S in err(), (S, side)
    for side in (-1, -8):
        assert call(side=side) == -1 and "fdn_pack_patch_cores" in err() and "side=%d" % side in err(), side
    for count in (0, -3):
        assert call(count=count) == -1 and "fdn_pack_patch_cores" in err() and "count=%d" % count in err(), count


def test_stitch_patches_finish_refuses_bad_arguments_before_it_touches_the_device(fdn):
    """Every refusal of fdn_stitch_patches (tests/test_infer_abi.py), under the new name, plus the NULL table."""
    lib = fdn._lib.load()
    name = "fdn_stitch_patches_finish"
    err = lambda: lib.fdn_last_error().decode()
    good = dict(pred=0x1000, vol=0x2000, scale=0x3000, F=2, Xo=14, Yo=20, Zo=26, S=16, side=4, nx=2, ny=3, nz=4, g0=0, count=48)

    def call(**kw):
        a = dict(good, **kw)
        return lib.fdn_stitch_patches_finish(a["pred"], a["vol"], a["scale"], a["F"], a["Xo"], a["Yo"], a["Zo"], a["S"], a["side"],
                                             a["nx"], a["ny"], a["nz"], a["g0"], a["count"], None)

    for bad in (dict(pred=None), dict(vol=None), dict(scale=None)):
        assert call(**bad) == -1 and name in err() and "NULL" in err(), bad
    for S, side in ((8, 4), (7, 4), (16, 8), (0, 0), (513, 0)):
        assert call(S=S, side=side) == -1 and name in err() and "S=%d" % S in err(), (S, side)
    assert call(side=-1) == -1 and name in err() and "side=-1" in err()
    for count in (0, -1):
        assert call(count=count) == -1 and name in err() and "count=%d" % count in err()
    assert call(g0=-2) == -1 and name in err() and "g0=-2" in err()
    assert call(g0=40, count=9) == -1 and name in err() and "[40, 49)" in err()
    for bad in (dict(Xo=17), dict(Yo=25), dict(Zo=33), dict(Xo=0), dict(Yo=-4), dict(Zo=0)):
        assert call(**bad) == -1 and name in err() and "extents" in err(), bad
    # side 0 (packed cores, S = core 8): the same limits
    for bad in (dict(Xo=17), dict(Zo=33)):
        assert call(S=8, side=0, **bad) == -1 and name in err() and "extents" in err(), bad
    for bad in (dict(F=0), dict(nx=0), dict(ny=-1), dict(nz=0)):
        assert call(**bad) == -1 and name in err(), bad
    # the plain entry point still reports under its own name
    assert lib.fdn_stitch_patches(None, 0x2000, 2, 14, 20, 26, 16, 4, 2, 3, 4, 0, 48, None) == -1
    assert "fdn_stitch_patches:" in err() and "NULL" in err()


def test_ops_refuse_host_tensors_and_bad_layouts(fdn):
    """No CPU fallback, and the checks of the operator layer come before the library."""
    import torch
    ops = fdn.ops
    with pytest.raises(fdn.FdnError, match="GPU"):
        ops.pack_patch_cores(torch.zeros(2, 16, 16, 16, 3), 4)
    with pytest.raises(fdn.FdnError, match=r"\(count,S,S,S,3\)"):
        ops.pack_patch_cores(torch.zeros(2, 16, 16, 15, 3), 4)
    with pytest.raises(fdn.FdnError, match=r"\(count,S,S,S,3\)"):
        ops.pack_patch_cores(torch.zeros(2, 16, 16, 16), 4)
    with pytest.raises(fdn.FdnError, match="S=16"):
        ops.pack_patch_cores(torch.zeros(2, 16, 16, 16, 3), 8)
    with pytest.raises(fdn.FdnError, match="out must be"):
        ops.pack_patch_cores(torch.zeros(2, 16, 16, 16, 3), 4, out=torch.zeros(2, 8, 8, 7, 3))
    scale = torch.ones(1, 2, dtype=torch.float64)
    with pytest.raises(fdn.FdnError, match="float64"):                      # a float32 volume with frame_scale
        ops.stitch_patches(torch.zeros(2, 16, 16, 16, 3), torch.zeros(1, 3, 8, 8, 8), 4, (2, 2, 2), frame_scale=scale)
    with pytest.raises(fdn.FdnError, match=r"\(count,S,S,S,3\)"):
        ops.stitch_patches(torch.zeros(2, 16, 16, 15, 3), torch.zeros(1, 3, 8, 8, 8, dtype=torch.float64), 4, (2, 2, 2), frame_scale=scale)
    with pytest.raises(fdn.FdnError, match=r"\(F,2\)"):
        ops.stitch_patches(torch.zeros(2, 16, 16, 16, 3), torch.zeros(1, 3, 8, 8, 8, dtype=torch.float64), 4, (2, 2, 2),
                           frame_scale=torch.ones(2, 2, dtype=torch.float64))
    with pytest.raises(fdn.FdnError, match="GPU"):                          # host tensors
        ops.stitch_patches(torch.zeros(2, 16, 16, 16, 3), torch.zeros(1, 3, 8, 8, 8, dtype=torch.float64), 4, (2, 2, 2), frame_scale=scale)
    assert import_module("4dflownet_amd.ops_bf16").pack_patch_cores is ops.pack_patch_cores      # the prediction is fp32 in both modes


@pytest.mark.parametrize("total,per_frame,world", [(72, 24, 2), (72, 24, 3), (8, 8, 2), (5, 24, 8), (1, 1, 2)])
def test_shards_tile_the_patch_list_and_rebased_patches_are_the_global_ones(total, per_frame, world):
    predictor = import_module("4dflownet_amd.predictor")
    bounds = predictor.shard_bounds(total, world)
    assert len(bounds) == world + 1 and bounds[0] == 0 and bounds[-1] == total
    assert all(bounds[r] <= bounds[r + 1] for r in range(world))                       # contiguous ranges that tile [0, total)
    covered = [g for r in range(world) for g in range(bounds[r], bounds[r + 1])]
    assert covered == list(range(total))
    nframes = total // per_frame if total % per_frame == 0 else None                   # (5,24,8): a made-up partial frame, spans only
    for r in range(world):
        lo, hi = bounds[r], bounds[r + 1]
        f0, f1 = predictor.shard_frame_span(lo, hi, per_frame)
        if hi == lo:                                                                   # an empty shard: nothing to load, send or wait for
            assert (f0, f1) == (0, 0)
            continue
        assert 0 <= f0 < f1 and (nframes is None or f1 <= nframes)
        # the span is tight, and local patch g - f0 * per_frame of the loaded frames is global patch g: same frame, same place in it
        assert f0 == lo // per_frame and f1 - 1 == (hi - 1) // per_frame
        for g in range(lo, hi):
            local = g - f0 * per_frame
            assert 0 <= local < (f1 - f0) * per_frame
            assert (f0 + local // per_frame, local % per_frame) == (g // per_frame, g % per_frame)
    empty = [r for r in range(world) if bounds[r + 1] == bounds[r]]
    if (total, world) == (5, 8):
        assert empty == [5, 6, 7]                                                      # one patch each for ranks 0-4
    if (total, world) == (1, 2):
        assert empty == [1]
    if (total, per_frame, world) == (72, 24, 2):
        assert bounds == [0, 36, 72]
        assert predictor.shard_frame_span(36, 72, 24) == (1, 3)                        # rank 1 starts in the middle of frame 1

"""Host-side argument checks of the C-ABI entry points that exist once per storage type (csrc/api.hip): every case below must be
refused BEFORE any HIP call, with the exact return code, and fdn_last_error() must name the function that was called.

The pointers are made-up integers and are never dereferenced (the pattern of test_abi.py::
test_mask_query_and_multi_source_argument_checks_need_no_gpu).  A case that slipped past its check would launch a kernel on addresses
that are not memory, so the module skips itself where a GPU is present: it is a host-logic test for the CPU machine."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-logic test: fake pointers must never reach a device")

OK, BAD_ARG, UNSUPPORTED, HIP, WORKSPACE = 0, -1, -2, -3, -4
NONE, RELU, LEAKY = 0, 1, 2
P = [0x10000 * (i + 1) for i in range(12)]          # distinct fake device addresses
N, D, H, W = 2, 8, 8, 8
BIG = 1 << 30                                       # a workspace size no check of these grids exceeds


def table(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


class Entry:
    """An entry point with a full set of acceptable arguments, by name: case(**changes) gives the positional list with those replaced."""

    def __init__(self, name, **base):
        self.name, self.base = name, base

    def args(self, **changes):
        unknown = set(changes) - set(self.base)
        assert not unknown, (self.name, unknown)
        return list({**self.base, **changes}.values())


def dims(**kw):
    return dict(dict(N=N, D=D, H=H, W=W), **kw)


# ---- the generic convolution entry points: fdn_conv3d_fwd[_bf16], fdn_conv3d_wgrad[_bf16] ----
def fwd(name, algo):
    tail = dict(algo=0, stream=None) if algo else dict(stream=None)
    return Entry(name, x=P[0], x2=None, w=P[1], wpack=P[2], bias=None, residual=None, y=P[3], **dims(), Cin=64, Cout=64, K=3, ldy=64,
                 y_coff=0, act=RELU, alpha=0.2, **tail)


def wgrad(name, algo):
    tail = dict(algo=0, stream=None) if algo else dict(stream=None)
    return Entry(name, x=P[0], x2=None, dz=P[1], dw=P[2], dbias=None, workspace=P[3], workspace_bytes=BIG, **dims(), Cin=64, Cout=64, K=3,
                 lddz=64, dz_coff=0, **tail)


SHAPES = dict(c64=dict(Cin=64, Cout=64, K=3), cin3=dict(Cin=3, Cout=64, K=3), head=dict(Cin=64, Cout=1, K=3),
              c1x1=dict(Cin=128, Cout=64, K=1))


def fwd_cases(e, algo):
    c = [("x_null", BAD_ARG, dict(x=None)), ("y_null", BAD_ARG, dict(y=None)), ("zero_extent", BAD_ARG, dict(H=0)),
         ("negative_extent", BAD_ARG, dict(N=-1)), ("act_3", BAD_ARG, dict(act=3)), ("act_minus_1", BAD_ARG, dict(act=-1)),
         ("c64_ldy_32", BAD_ARG, dict(ldy=32)), ("c64_y_coff_1", BAD_ARG, dict(y_coff=1)), ("c64_wpack_null", BAD_ARG, dict(wpack=None)),
         ("c64_D_1023", BAD_ARG, dict(D=1023)), ("c64_H_1023", BAD_ARG, dict(H=1023)), ("c64_W_1023", BAD_ARG, dict(W=1023)),
         ("cin3_residual", BAD_ARG, dict(residual=P[4], **SHAPES["cin3"])), ("cin3_w_null", BAD_ARG, dict(w=None, **SHAPES["cin3"])),
         ("cin3_ldy_32", BAD_ARG, dict(ldy=32, **SHAPES["cin3"])), ("cin3_y_coff_1", BAD_ARG, dict(y_coff=1, **SHAPES["cin3"])),
         ("head_w_null", BAD_ARG, dict(w=None, ldy=3, **SHAPES["head"])), ("head_ldy_0", BAD_ARG, dict(ldy=0, **SHAPES["head"])),
         ("head_y_coff_is_ldy", BAD_ARG, dict(ldy=3, y_coff=3, **SHAPES["head"])),
         ("head_y_coff_negative", BAD_ARG, dict(ldy=3, y_coff=-1, **SHAPES["head"])),
         ("c1x1_x2_null", BAD_ARG, dict(x2=None, **SHAPES["c1x1"])), ("c1x1_w_null", BAD_ARG, dict(x2=P[5], w=None, **SHAPES["c1x1"])),
         ("c1x1_ldy_128", BAD_ARG, dict(x2=P[5], ldy=128, **SHAPES["c1x1"])),
         ("unsupported_5_64_3", UNSUPPORTED, dict(Cin=5)), ("unsupported_64_64_1", UNSUPPORTED, dict(K=1)),
         ("unsupported_64_2_3", UNSUPPORTED, dict(Cout=2))]
    if algo:
        c += [("algo_5", BAD_ARG, dict(algo=5)), ("algo_minus_1", BAD_ARG, dict(algo=-1))]
    return [(e, i, rc, ch, None) for i, rc, ch in c]


def wgrad_cases(e, algo):
    c = [("x_null", BAD_ARG, dict(x=None)), ("dz_null", BAD_ARG, dict(dz=None)), ("dw_null", BAD_ARG, dict(dw=None)),
         ("zero_extent", BAD_ARG, dict(W=0)), ("c64_lddz_32", BAD_ARG, dict(lddz=32)), ("c64_dz_coff_1", BAD_ARG, dict(dz_coff=1)),
         ("cin3_lddz_32", BAD_ARG, dict(lddz=32, **SHAPES["cin3"])), ("cin3_dz_coff_1", BAD_ARG, dict(dz_coff=1, **SHAPES["cin3"])),
         ("c1x1_x2_null", BAD_ARG, dict(**SHAPES["c1x1"])), ("c1x1_lddz_32", BAD_ARG, dict(x2=P[5], lddz=32, **SHAPES["c1x1"])),
         ("unsupported_5_64_3", UNSUPPORTED, dict(Cin=5)), ("unsupported_64_64_1", UNSUPPORTED, dict(K=1))]
    if algo:
        c += [("algo_5", BAD_ARG, dict(algo=5)), ("algo_minus_1", BAD_ARG, dict(algo=-1))]
    # a workspace one byte short of what <name>_workspace_bytes asks for, or none at all: filled in by the test ("need")
    for tag, shp in SHAPES.items():
        c += [(tag + "_workspace_short", WORKSPACE, dict(workspace_bytes="need-1", **shp)),
              (tag + "_workspace_null", WORKSPACE, dict(workspace=None, workspace_bytes="need", **shp))]
    return [(e, i, rc, ch, None) for i, rc, ch in c]


def wgrad_batch(name, algo):
    tail = dict(algo=0, stream=None) if algo else dict(stream=None)
    return Entry(name, x=table(P[0], P[1]), dz=table(P[2], P[3]), dw=table(P[4], P[5]), dbias=None, n_layers=2, workspace=P[6],
                 workspace_bytes=BIG, **dims(), **tail)


def wgrad_batch_cases(e, algo):
    # (layer_0_null: one layer on a grid off the batched kernels' raster -- W = 6 -- takes the per-layer loop, which looks at the
    # layer's pointers before it launches anything)
    c = [("x_table_null", BAD_ARG, dict(x=None)), ("dz_table_null", BAD_ARG, dict(dz=None)), ("dw_table_null", BAD_ARG, dict(dw=None)),
         ("no_layers", BAD_ARG, dict(n_layers=0)), ("zero_extent", BAD_ARG, dict(D=0)),
         ("workspace_short", WORKSPACE, dict(workspace_bytes="need-1")), ("workspace_null", WORKSPACE, dict(workspace=None)),
         ("layer_0_null", BAD_ARG, dict(x=table(None), dz=table(P[2]), dw=table(P[4]), n_layers=1, W=6))]
    if algo:
        c += [("algo_5", BAD_ARG, dict(algo=5))]
    return [(e, i, rc, ch, None) for i, rc, ch in c]


# ---- the 64->64 entry points of both storage types ----
C64_FWD_MASK = Entry("fdn_conv64_fwd_mask", x=P[0], wpack=P[1], bias=None, residual=None, y=P[2], y_mask=P[3], **dims(), act=RELU, alpha=0.2,
                     algo=0, stream=None)
C64_FWD_BF16 = Entry("fdn_conv64_fwd_bf16", x=P[0], wpack=P[1], bias=None, residual=None, y=P[2], **dims(), act=RELU, alpha=0.2, stream=None)
C64_FWD_BF16_MASK = Entry("fdn_conv64_fwd_bf16_mask", x=P[0], wpack=P[1], bias=None, residual=None, y=P[2], y_mask=P[3], **dims(), act=RELU,
                          alpha=0.2, stream=None)
DGRAD_FUSED = Entry("fdn_conv3d_dgrad_fused", dz=P[0], wpack=P[1], dxpad=P[2], skip=None, y_prev=P[3], act=RELU, alpha=0.2, dz_prev=P[4],
                    **dims(), algo=0, stream=None)
DGRAD_FUSED_PART = Entry("fdn_conv3d_dgrad_fused_part", dz=P[0], wpack=P[1], dxpad=P[2], skip=None, y_prev=P[3], act=RELU, alpha=0.2,
                         dz_prev=P[4], **dims(), parts=3, algo=0, stream=None)
DGRAD_FUSED_MASK = Entry("fdn_conv64_dgrad_fused_mask", dz=P[0], wpack=P[1], dxpad=P[2], skip=None, y_mask=P[3], act=RELU, alpha=0.2,
                         dz_prev=P[4], **dims(), algo=0, stream=None)
DGRAD_FUSED_BF16 = Entry("fdn_conv64_dgrad_fused_bf16", dz=P[0], wpack=P[1], dxpad=P[2], skip=None, y_prev=P[3], act=RELU, alpha=0.2,
                         dz_prev=P[4], **dims(), stream=None)
DGRAD_FUSED_BF16_MASK = Entry("fdn_conv64_dgrad_fused_bf16_mask", dz=P[0], wpack=P[1], dxpad=P[2], skip=None, y_prev=None, y_mask=P[3], act=RELU,
                              alpha=0.2, dz_prev=P[4], **dims(), stream=None)
MULTI = Entry("fdn_conv64_dgrad_fused_multi", dz=table(P[0], P[1]), wpack=table(P[2], P[3]), nsrc=2, dxpad=P[4], skip=None, y_prev=None,
              y_mask=P[5], act=RELU, alpha=0.2, dz_prev=P[6], **dims(), algo=0, stream=None)
MULTI_BF16 = Entry("fdn_conv64_dgrad_fused_bf16_multi", dz=table(P[0], P[1]), wpack=table(P[2], P[3]), nsrc=2, dxpad=P[4], skip=None,
                   y_prev=None, y_mask=P[5], act=RELU, alpha=0.2, dz_prev=P[6], **dims(), stream=None)


def c64_cases(e, nulls, limit, algo, extra=()):
    c = [(n + "_null", BAD_ARG, {n: None}) for n in nulls]
    c += [("zero_extent", BAD_ARG, dict(D=0)), ("act_3", BAD_ARG, dict(act=3)), ("act_minus_1", BAD_ARG, dict(act=-1))]
    c += [("%s_%d" % (ax, limit + 1), BAD_ARG, {ax: limit + 1}) for ax in "DHW"]
    if algo:
        c += [("algo_5", BAD_ARG, dict(algo=5)), ("algo_minus_1", BAD_ARG, dict(algo=-1))]
    return [(e, i, rc, ch, None) for i, rc, ch in c] + [(e,) + tuple(x) for x in extra]


def multi_cases(e, algo):
    extra = [("nsrc_0", BAD_ARG, dict(nsrc=0), "1..3"), ("nsrc_4", BAD_ARG, dict(nsrc=4), "1..3"),
             ("mask_with_act_none", BAD_ARG, dict(act=NONE), None),
             ("source_1_null", BAD_ARG, dict(dz=table(P[0], None)), "source 1"),
             ("pack_1_null", BAD_ARG, dict(wpack=table(P[2], None)), "source 1")]
    if algo:                 # fp32 only: y_prev excludes the mask; the packs lie within 1 GiB of each other
        extra += [("y_prev_and_mask", BAD_ARG, dict(y_prev=P[7]), None),
                  ("packs_2_GiB_apart", BAD_ARG, dict(wpack=table(P[2], P[2] + (1 << 31))), "1 GiB")]
    return c64_cases(e, ["dz", "wpack", "dxpad", "dz_prev"], 1020, algo, extra)


# ---- fold_halo_border, conv1x1_dgrad, conv_cout1_dgrad_folded ----
def fold(name):
    return Entry(name, dxpad0=P[0], dxpad1=P[1], dxpad2=P[2], nsrc=3, skip=None, y_prev=None, act=RELU, alpha=0.2, dz_prev=P[3], **dims(),
                 stream=None)


def fold_cases(e):
    c = [("dxpad0_null", BAD_ARG, dict(dxpad0=None)), ("dz_prev_null", BAD_ARG, dict(dz_prev=None)), ("nsrc_0", BAD_ARG, dict(nsrc=0)),
         ("nsrc_4", BAD_ARG, dict(nsrc=4)), ("nsrc_2_dxpad1_null", BAD_ARG, dict(nsrc=2, dxpad1=None)),
         ("nsrc_3_dxpad2_null", BAD_ARG, dict(dxpad2=None)), ("zero_extent", BAD_ARG, dict(N=0))]
    return [(e, i, rc, ch, None) for i, rc, ch in c]


def c1x1(name):
    return Entry(name, dz=P[0], w=P[1], ya=P[2], yb=P[3], dxa=P[4], dxb=P[5], nvox=N * D * H * W, stream=None)


def c1x1_cases(e):
    c = [(n + "_null", BAD_ARG, {n: None}) for n in ("dz", "w", "ya", "yb", "dxa", "dxb")]
    c += [("nvox_0", BAD_ARG, dict(nvox=0)), ("nvox_negative", BAD_ARG, dict(nvox=-1))]
    return [(e, i, rc, ch, None) for i, rc, ch in c]


def cout1(name, **operands):
    return Entry(name, dz=P[0], w=P[1], **operands, act=RELU, alpha=0.2, dz_prev=P[3], dbias_prev=None, workspace=None, workspace_bytes=0,
                 **dims(), lddz=3, dz_coff=0, stream=None)


COUT1 = cout1("fdn_conv_cout1_dgrad_folded", y_prev=P[2])
COUT1_MASK = cout1("fdn_conv_cout1_dgrad_folded_mask", y_mask=P[2])
COUT1_BF16 = cout1("fdn_conv_cout1_dgrad_folded_bf16", y_prev=P[2])
COUT1_BF16_MASK = cout1("fdn_conv_cout1_dgrad_folded_bf16_mask", y_prev=None, y_mask=P[2])
# (the operand and workspace checks of the four live in their common launcher, small_convs.hip, which reports under the caller's name)


def cout1_cases(e, extra=()):
    c = [("dz_null", BAD_ARG, dict(dz=None)), ("w_null", BAD_ARG, dict(w=None)), ("dz_prev_null", BAD_ARG, dict(dz_prev=None)),
         ("zero_extent", BAD_ARG, dict(H=0)), ("dbias_without_workspace", WORKSPACE, dict(dbias_prev=P[4])),
         ("dbias_workspace_1_byte", WORKSPACE, dict(dbias_prev=P[4], workspace=P[5], workspace_bytes=1))]
    return [(e, i, rc, ch, None) for i, rc, ch in c] + [(e,) + tuple(x) for x in extra]


CASES = (
    fwd_cases(fwd("fdn_conv3d_fwd", True), True) + fwd_cases(fwd("fdn_conv3d_fwd_bf16", False), False) +
    wgrad_cases(wgrad("fdn_conv3d_wgrad", True), True) + wgrad_cases(wgrad("fdn_conv3d_wgrad_bf16", False), False) +
    wgrad_batch_cases(wgrad_batch("fdn_conv3d_wgrad_batch", True), True) +
    wgrad_batch_cases(wgrad_batch("fdn_conv3d_wgrad_bf16_batch", False), False) +
    c64_cases(C64_FWD_MASK, ["x", "wpack", "y", "y_mask"], 1020, True) +
    c64_cases(C64_FWD_BF16, ["x", "wpack", "y"], 1022, False) +
    c64_cases(C64_FWD_BF16_MASK, ["x", "wpack", "y"], 1022, False) +
    c64_cases(DGRAD_FUSED, ["dz", "wpack", "dxpad", "dz_prev"], 1020, True) +
    c64_cases(DGRAD_FUSED_PART, ["dz", "wpack", "dxpad", "dz_prev"], 1020, True,
              [("parts_0", BAD_ARG, dict(parts=0), None), ("parts_4", BAD_ARG, dict(parts=4), None)]) +
    c64_cases(DGRAD_FUSED_MASK, ["dz", "wpack", "dxpad", "dz_prev", "y_mask"], 1020, True, [("mask_with_act_none", BAD_ARG, dict(act=NONE), None)]) +
    c64_cases(DGRAD_FUSED_BF16, ["dz", "wpack", "dxpad", "dz_prev"], 1020, False) +
    c64_cases(DGRAD_FUSED_BF16_MASK, ["dz", "wpack", "dxpad", "dz_prev"], 1020, False, [("mask_with_act_none", BAD_ARG, dict(act=NONE), None)]) +
    multi_cases(MULTI, True) + multi_cases(MULTI_BF16, False) +
    fold_cases(fold("fdn_fold_halo_border")) + fold_cases(fold("fdn_fold_halo_border_bf16")) +
    c1x1_cases(c1x1("fdn_conv1x1_dgrad")) + c1x1_cases(c1x1("fdn_conv1x1_dgrad_bf16")) +
    cout1_cases(COUT1) + cout1_cases(COUT1_BF16) +
    cout1_cases(COUT1_MASK, [("mask_null", BAD_ARG, dict(y_mask=None), None), ("mask_with_act_none", BAD_ARG, dict(act=NONE), None),
                             ("mask_with_act_3", BAD_ARG, dict(act=3), None), ("mask_W_6", BAD_ARG, dict(W=6), "W % 4")]) +
    cout1_cases(COUT1_BF16_MASK, [("mask_with_act_none", BAD_ARG, dict(act=NONE), None)]))


@pytest.fixture(scope="module")
def lib(fdn):
    return fdn._lib.load()


def _workspace_need(lib, e, a):
    """What the entry point's own *_workspace_bytes asks for the case's shape."""
    if "batch" in e.name:
        return getattr(lib, e.name + "_workspace_bytes")(a["n_layers"], a["N"], a["D"], a["H"], a["W"])
    return getattr(lib, e.name + "_workspace_bytes")(a["N"], a["D"], a["H"], a["W"], a["Cin"], a["Cout"], a["K"])


@pytest.mark.parametrize("e,rc,changes,who", [pytest.param(e, rc, ch, who, id="%s-%s" % (e.name, i)) for e, i, rc, ch, who in CASES])
def test_refused_before_any_hip_call(lib, e, rc, changes, who):
    changes = dict(changes)
    wsb = changes.get("workspace_bytes")
    if isinstance(wsb, str):
        need = _workspace_need(lib, e, {**e.base, **changes})
        assert need > 0, "%s asks for no workspace here: the case cannot come one byte short" % e.name
        changes["workspace_bytes"] = need - 1 if wsb == "need-1" else need
    got = getattr(lib, e.name)(*e.args(**changes))
    err = lib.fdn_last_error().decode()
    assert got == rc, (got, err)
    # the name is followed by ':' or '(' -- `fdn_x: ...` does not pass for a call of fdn_x_mask -- and by the words a caller's handler matches
    assert err.startswith(e.name) and err[len(e.name)] in ":(", err
    assert who is None or who in err, err


def test_workspace_queries_of_the_twins_agree_where_the_kernels_are_shared(lib):
    """The thin layers' weight gradients run the same templated kernels in both modes and ask for the same workspace; a batch never
    asks for less than one of its layers; nonsense asks for nothing."""
    f32, b16 = lib.fdn_conv3d_wgrad_workspace_bytes, lib.fdn_conv3d_wgrad_bf16_workspace_bytes
    for shp in ("cin3", "head", "c1x1"):
        s = SHAPES[shp]
        assert f32(N, D, H, W, s["Cin"], s["Cout"], s["K"]) == b16(N, D, H, W, s["Cin"], s["Cout"], s["K"]) > 0, shp
    assert f32(N, D, H, W, 5, 64, 3) == b16(N, D, H, W, 5, 64, 3)
    for one, batch in ((f32, lib.fdn_conv3d_wgrad_batch_workspace_bytes), (b16, lib.fdn_conv3d_wgrad_bf16_batch_workspace_bytes)):
        for n in (1, 2, 3, 7, 11):
            for g in ((2, 8, 8, 8), (8, 24, 24, 24), (1, 5, 7, 6), (4, 32, 32, 32)):
                assert batch(n, *g) >= one(*g, 64, 64, 3) > 0, (n, g)
        assert batch(0, N, D, H, W) == 0 and batch(2, N, 0, H, W) == 0 and batch(2, 0, D, H, W) == 0

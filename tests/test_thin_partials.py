"""The partial rows of the thin layers (csrc/thin_layers.h: fdn_thin_partials) answered without a GPU, through fdn_debug_thin_partials
of the test build:

  1. rows and row_floats of every op, both storage types and both states of the fdn_debug_set_*_mfma hooks are what the table below
     says: the kernels' grid rules, restated here;
  2. the bytes of every weight-gradient and bias op fit what fdn_conv3d_wgrad_workspace_bytes and fdn_conv3d_wgrad_bf16_workspace_bytes
     answer for the layer the op belongs to, and the dbias_prev rows of the head's folded dgrad fit the 2048 * 64 floats include/fdn.h states;
  3. the two public queries answer 768 * max(K^3 * Cin * Cout, 64) * 4 bytes for the thin layers."""
import ctypes
import importlib
import itertools

import pytest

_lib = importlib.import_module("4dflownet_amd._lib")

# FdnThinOp
WGRAD_CIN3, WGRAD_COUT1, WGRAD_1X1, BIAS64, BIAS1, HEAD_DBIAS = OPS = range(6)
ROW_FLOATS = {WGRAD_CIN3: 81 * 64, WGRAD_COUT1: 27 * 64, WGRAD_1X1: 128 * 64, BIAS64: 64, BIAS1: 1, HEAD_DBIAS: 64}
# the (Cin, Cout, K) whose weight gradient the op is, or rides on (the bias gradient reuses the weight gradient's workspace)
LAYERS = {WGRAD_CIN3: [(3, 64, 3)], WGRAD_COUT1: [(64, 1, 3)], WGRAD_1X1: [(128, 64, 1)], BIAS64: [(3, 64, 3), (128, 64, 1), (64, 64, 3)],
          BIAS1: [(64, 1, 3)]}
HEAD_WS_BYTES = 2048 * 64 * 4
HOOKS = ("cin3_mfma", "conv1x1_mfma", "heads_mfma")

# either side of every cap: the shapes of tests/test_gpu_head_walks.py (512, 513, 768, 770, 1024, 1025, 2600, 8448 head tiles), the
# largest product step, grids of one voxel / one tile, odd W and W % 4 != 0, and sizes around the voxel-count caps
# (256 * 256 = 65536 for the C = 64 bias, 128 * 512 = 65536 for the 3->64 and VALU 1x1 rows, 512 * 256 = 131072 for the MFMA 1x1 rows,
# 4096 * 512 = 2097152 for the C = 1 bias)
NAMED = [(4, 8, 64, 64), (1, 9, 65, 148), (6, 8, 64, 64), (2, 17, 49, 84), (8, 8, 64, 64), (1, 17, 33, 324), (13, 5, 33, 156),
         (1, 129, 128, 128), (4, 128, 128, 128), (8, 48, 48, 48), (1, 1, 1, 1), (1, 1, 1, 2), (1, 4, 8, 8), (1, 4, 8, 9), (1, 5, 9, 9),
         (1, 1, 255, 257), (1, 1, 256, 256), (1, 1, 1, 65537), (1, 2, 256, 256), (1, 1, 2, 65537), (1, 1, 1, 131073), (2, 1, 1024, 1024),
         (1, 1, 2049, 1024), (1, 2046, 1, 1), (1, 2, 1024, 1), (3, 683, 1, 7), (1, 510, 1, 3), (1, 17, 28, 5), (1, 16, 30, 7)]
SWEEP = sorted(set(NAMED) | set(itertools.product((1, 2, 3, 5, 8, 13), (1, 3, 4, 5, 8, 17, 24), (1, 5, 8, 9, 33, 64, 65), (1, 2, 5, 7, 8, 10, 33, 64, 150))))


def cdiv(a, b):
    return -(-a // b)


def clamp(v, cap):
    return max(1, min(v, cap))


def table(op, bf16, N, D, H, W, mfma):
    """rows: the grid of the op's kernel."""
    nvox = N * D * H * W
    tiles = N * cdiv(D, 4) * cdiv(H, 8) * cdiv(W, 8)
    if op == WGRAD_CIN3:
        return clamp(cdiv(nvox, 128), 512)
    if op == WGRAD_COUT1:
        return min(tiles, 768 if bf16 else 512) if mfma else min(N * (D + 2) * (H + 2), 512)
    if op == WGRAD_1X1:
        return clamp((nvox // 2 + 255) // 256, 256) if mfma else clamp(cdiv(nvox, 128), 512)
    if op == BIAS64:
        return clamp(cdiv(nvox, 256), 256)
    if op == BIAS1:
        return clamp(cdiv(nvox, 4096), 512)
    return min(tiles, 1024) if mfma else min(N * D * H, 2048)


@pytest.fixture
def tlib():
    with _lib.test_build() as lib:
        try:
            yield lib
        finally:
            for name in HOOKS:
                getattr(lib, "fdn_debug_set_" + name)(1)


_out = (ctypes.c_longlong * 3)()


def partials(lib, op, bf16, N, D, H, W):
    assert lib.fdn_debug_thin_partials(op, int(bf16), N, D, H, W, _out) == 0
    return tuple(_out)


def test_rows_match_the_table_and_fit_the_promised_workspace(tlib):
    query = {False: tlib.fdn_conv3d_wgrad_workspace_bytes, True: tlib.fdn_conv3d_wgrad_bf16_workspace_bytes}
    seen, peak = 0, {}
    for mfma in (1, 0):
        for name in HOOKS:
            assert getattr(tlib, "fdn_debug_set_" + name)(mfma) == 0
        for (N, D, H, W), op, bf16 in itertools.product(SWEEP, OPS, (False, True)):
            rows, row_floats, nbytes = partials(tlib, op, bf16, N, D, H, W)
            where = (op, bf16, N, D, H, W, mfma)
            want = table(op, bf16, N, D, H, W, mfma)
            assert (rows, row_floats) == (want, ROW_FLOATS[op]) and nbytes == rows * row_floats * 4 and rows >= 1, where + (rows, row_floats, nbytes)
            if op == HEAD_DBIAS:
                assert nbytes <= HEAD_WS_BYTES, where
            else:
                for Cin, Cout, K in LAYERS[op]:
                    for q in query.values():                   # (the bias of a head is fp32 in both modes: either query may size its workspace)
                        assert nbytes <= q(N, D, H, W, Cin, Cout, K), where + (Cin, Cout, K)
            peak[(op, bf16, mfma)] = max(rows, peak.get((op, bf16, mfma), 0))
            seen += 1
    assert seen == 2 * len(SWEEP) * 6 * 2 and len(SWEEP) > 2000
    # the sweep reaches the cap of every path
    caps = {(WGRAD_CIN3, 1): 512, (WGRAD_CIN3, 0): 512, (WGRAD_COUT1, 0): 512, (WGRAD_1X1, 1): 256, (WGRAD_1X1, 0): 512, (BIAS64, 1): 256,
            (BIAS64, 0): 256, (BIAS1, 1): 512, (BIAS1, 0): 512, (HEAD_DBIAS, 1): 1024, (HEAD_DBIAS, 0): 2048}
    for (op, bf16, mfma), rows in peak.items():
        assert rows == ((768 if bf16 else 512) if (op, mfma) == (WGRAD_COUT1, 1) else caps[(op, mfma)]), (op, bf16, mfma, rows)
    assert len(peak) == 6 * 2 * 2


def test_named_grids(tlib):
    """The grids the GPU tests launch, as numbers: the caps from either side, and the clamp to one row."""
    rows = lambda op, bf16, dims: partials(tlib, op, bf16, *dims)[0]
    assert [rows(WGRAD_COUT1, False, d) for d in ((4, 8, 64, 64), (1, 9, 65, 148), (1, 129, 128, 128))] == [512, 512, 512]
    assert [rows(WGRAD_COUT1, True, d) for d in ((4, 8, 64, 64), (6, 8, 64, 64), (2, 17, 49, 84))] == [512, 768, 768]
    assert [rows(HEAD_DBIAS, False, d) for d in ((6, 8, 64, 64), (8, 8, 64, 64), (1, 17, 33, 324), (4, 128, 128, 128))] == [768, 1024, 1024, 1024]
    assert partials(tlib, WGRAD_COUT1, True, 4, 128, 128, 128) == (768, 27 * 64, 768 * 27 * 64 * 4)       # fills the promised workspace exactly
    assert partials(tlib, WGRAD_COUT1, True, 4, 128, 128, 128)[2] == tlib.fdn_conv3d_wgrad_bf16_workspace_bytes(4, 128, 128, 128, 64, 1, 3)
    assert rows(BIAS1, False, (1, 128, 128, 128)) == 512 and rows(BIAS1, False, (1, 129, 128, 128)) == 512 and rows(BIAS1, False, (1, 127, 128, 128)) == 508
    for op in OPS:                                                                     # one voxel: one row
        assert rows(op, False, (1, 1, 1, 1)) == 1 and rows(op, True, (1, 1, 1, 1)) == 1
    assert (1 // 2 + 255) // 256 == 0 and rows(WGRAD_1X1, False, (1, 1, 1, 1)) == 1    # (the MFMA 1x1 count is 0 there before the clamp)
    assert tlib.fdn_debug_thin_partials(6, 0, 1, 1, 1, 1, _out) != 0 and tlib.fdn_debug_thin_partials(-1, 0, 1, 1, 1, 1, _out) != 0


def test_size_queries_answer_as_before(fdn):
    lib = fdn._lib.load()
    for Cin, Cout, K in ((3, 64, 3), (64, 1, 3), (128, 64, 1)):
        want = 768 * max(K ** 3 * Cin * Cout, 64) * 4
        for dims in ((1, 1, 1, 1), (8, 24, 24, 24), (4, 128, 128, 128)):
            assert lib.fdn_conv3d_wgrad_workspace_bytes(*dims, Cin, Cout, K) == want
            assert lib.fdn_conv3d_wgrad_bf16_workspace_bytes(*dims, Cin, Cout, K) == want

"""The host plan of the 64->64 weight gradient (csrc/wgrad64_plan.h: fdn_wgrad64_plan) answered without a GPU:

  1. the four public size queries against a table recorded from the library before the plan existed (tests/golden/make_wgrad64_plan_golden.py);
  2. every step of every plan of the sweep (fdn_debug_wgrad64_plan on the test build: each algo, each route-forcing hook off and on, both
     storage types) fits the plan's workspace_bytes, and that fits what the matching public size query returns;
  3. the chunk and route rules the comments state;
  4. the weight-gradient launch plans tests/test_gpu_plan_coverage.py commits (PLAN_CASES) are what the plan produces for their shapes."""
import contextlib
import ctypes
import importlib
import itertools
import json
import os
import re

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad64_plan_golden.json")
_lib = importlib.import_module("4dflownet_amd._lib")

AUTO, DIRECT, WINO_W, WINO_H2, WINO_BF16X3 = range(5)
BATCH_MAX = {False: 32, True: 7}                     # layers of one launch: kWgBatchMax, kWgBfChunkMax
INT_FIELDS = ("first", "count", "splits", "planes", "grid", "tiles", "nseg", "seg_len", "partial_bytes")
HOOKS = ("wgrad64_direct", "wgrad64_wino_nodep", "wgrad64_bf16_variant")


@pytest.fixture
def tlib():
    with _lib.test_build() as lib:
        yield lib


@contextlib.contextmanager
def hooks(lib, **on):
    try:
        for name in HOOKS:
            assert getattr(lib, "fdn_debug_set_" + name)(int(on.get(name, 0))) == 0
        yield
    finally:
        for name in HOOKS:
            getattr(lib, "fdn_debug_set_" + name)(0)


_buf = ctypes.create_string_buffer(1 << 14)
_STEP = re.compile("route=(\\w+) " + " ".join(k + "=(\\d+)" for k in INT_FIELDS) + "\n")
_LAST = re.compile("workspace_bytes=(\\d+) addr32_ok=(\\d)\n$")


def plan(lib, bf16, n, N, D, H, W, algo=AUTO):
    """(steps, workspace_bytes, addr32_ok) of fdn_wgrad64_plan under the hooks as set."""
    size = lib.fdn_debug_wgrad64_plan(int(bf16), n, N, D, H, W, algo, _buf, len(_buf))
    assert 0 < size < len(_buf)
    text = _buf.value.decode()
    steps = [dict(zip(INT_FIELDS, map(int, m[1:])), route=m[0]) for m in _STEP.findall(text)]
    ws, ok = _LAST.search(text).groups()
    assert text.count("\n") == len(steps) + 1
    return steps, int(ws), int(ok)


def counts(lib, bf16, n, dims, algo=AUTO):
    return [s["count"] for s in plan(lib, bf16, n, *dims, algo)[0]]


# ------------------------------------------------------------------------------------------------ 1. the size queries answer as before
def test_size_queries_match_the_recorded_table(fdn):
    lib = fdn._lib.load()
    g = json.load(open(GOLDEN))
    unit, hws, layers = g["unit"], g["grid"]["HW"], g["grid"]["layers"]
    grid = [(H, W) for H in hws for W in hws]
    single = {"f32": lib.fdn_conv3d_wgrad_workspace_bytes, "bf16": lib.fdn_conv3d_wgrad_bf16_workspace_bytes}
    batch = {"f32": lib.fdn_conv3d_wgrad_batch_workspace_bytes, "bf16": lib.fdn_conv3d_wgrad_bf16_batch_workspace_bytes}
    bad, checked = [], 0
    for dt in ("f32", "bf16"):
        for key, row in g["single"][dt].items():
            N, D = map(int, key.split())
            bad += [("single", dt, N, D, H, W, want * unit, have)
                    for (H, W), want in zip(grid, row) for have in [single[dt](N, D, H, W, 64, 64, 3)] if want * unit != have]
            checked += len(row)
        for key, idx in g["batch"][dt].items():
            N, D = map(int, key.split())
            assert len(idx) == len(layers)
            for n, i in zip(layers, idx):
                row = g["batch_rows"][i]
                bad += [("batch", dt, n, N, D, H, W, want * unit, have)
                        for (H, W), want in zip(grid, row) for have in [batch[dt](n, N, D, H, W)] if want * unit != have]
                checked += len(row)
    for q, args, want in g["other"]:
        have = getattr(lib, q)(*args)
        if have != want:
            bad.append((q, args, want, have))
    assert not bad, "%d answers differ from the recorded table, first: %s" % (len(bad), bad[:10])
    assert checked == 2 * 16 * 49 * (1 + 13) and len(g["other"]) == 96
    assert g["grid"] == {"N": [1, 2, 5, 8], "D": [1, 5, 8, 24], "HW": [5, 8, 12, 16, 24, 32, 48], "layers": [0, 1, 2, 3, 7, 8, 9, 11, 15, 16, 17, 32, 33]}


# ------------------------------------------------------------------------------------------------ 2. every step fits
def _check_plans(lib, bf16, g, algos):
    """Every plan of the sweep under the hooks as set; returns the number of plans checked."""
    single = lib.fdn_conv3d_wgrad_bf16_workspace_bytes if bf16 else lib.fdn_conv3d_wgrad_workspace_bytes
    batch = lib.fdn_conv3d_wgrad_bf16_batch_workspace_bytes if bf16 else lib.fdn_conv3d_wgrad_batch_workspace_bytes
    hws, seen = g["HW"], 0
    for N, D, H, W in itertools.product(g["N"], g["D"], hws, hws):
        bound1 = single(N, D, H, W, 64, 64, 3)
        for n in g["layers"]:
            boundn = batch(n, N, D, H, W)
            for algo in algos:
                steps, ws, _ = plan(lib, bf16, n, N, D, H, W, algo)
                where = (bf16, n, N, D, H, W, algo, steps)
                nxt = 0
                for s in steps:                                    # the layers 0 .. n - 1 once each, in order
                    assert s["first"] == nxt and 1 <= s["count"] <= BATCH_MAX[bf16], where
                    assert s["partial_bytes"] == s["count"] * s["splits"] * s["planes"] * 4096 * 4 and s["planes"] in (27, 36), where
                    assert s["partial_bytes"] <= ws, where
                    nxt += s["count"]
                assert nxt == n, where
                assert ws == max([s["partial_bytes"] for s in steps], default=0), where
                assert ws <= boundn, where + (ws, boundn)
                if n == 1:
                    assert ws <= bound1, where + (ws, bound1)
                seen += 1
    return seen


def test_every_step_fits_the_workspace_the_size_query_promises(tlib):
    g = json.load(open(GOLDEN))["grid"]
    per = 4 * 4 * 49 * 13
    # fp32 plans read force_direct and wino_nodep, bf16 plans bf16_variant (below: the other storage type's hooks change nothing)
    for direct, nodep in itertools.product((0, 1), repeat=2):
        with hooks(tlib, wgrad64_direct=direct, wgrad64_wino_nodep=nodep):
            assert _check_plans(tlib, False, g, range(5)) == per * 5
    for variant in (0, 1):
        with hooks(tlib, wgrad64_bf16_variant=variant):
            assert _check_plans(tlib, True, g, (AUTO,)) == per
    dims = (5, 24, 16, 16)
    with hooks(tlib):
        f32 = [plan(tlib, False, 11, *dims, a) for a in range(5)]
        bf16 = [plan(tlib, True, 11, *dims, a) for a in range(5)]
    assert all(p == bf16[0] for p in bf16)                         # the bf16 entry points take no algo
    with hooks(tlib, wgrad64_bf16_variant=1):
        assert [plan(tlib, False, 11, *dims, a) for a in range(5)] == f32
    with hooks(tlib, wgrad64_direct=1, wgrad64_wino_nodep=1):
        assert plan(tlib, True, 11, *dims) == bf16[0]


# ------------------------------------------------------------------------------------------------ 3. the rules the comments state
def test_fp32_chunk_and_route_rules(tlib):
    dims = (8, 24, 24, 24)
    with hooks(tlib):
        assert counts(tlib, False, 11, dims) == [9, 2]
        assert counts(tlib, False, 8, dims) == [8]
        steps = plan(tlib, False, 17, *dims)[0]
        assert [(s["count"], s["route"]) for s in steps] == [(16, "wino_batch"), (1, "wino_dep")]
        assert [s["route"] for s in plan(tlib, False, 11, *dims)[0]] == ["wino_batch"] * 2
        for algo in (WINO_H2, WINO_BF16X3):                          # every algo but direct / winograd_w plans as auto does
            assert plan(tlib, False, 11, *dims, algo) == plan(tlib, False, 11, *dims, AUTO)
        for n in (2, 11, 32):
            for algo, route in ((DIRECT, "direct"), (WINO_W, "wino_w")):   # direct and winograd_w never batch
                assert [(s["count"], s["route"]) for s in plan(tlib, False, n, *dims, algo)[0]] == [(1, route)] * n
            assert [(s["count"], s["route"]) for s in plan(tlib, False, n, 8, 5, 24, 24)[0]] == [(1, "wino_w")] * n       # odd D
            assert [(s["count"], s["route"]) for s in plan(tlib, False, n, 8, 24, 24, 10)[0]] == [(1, "wino_dep")] * n    # W % 4 != 0
        assert counts(tlib, False, 32, dims) == [32]
        assert [(s["count"], s["route"]) for s in plan(tlib, False, 33, *dims)[0]] == [(1, "wino_dep")] * 33       # more than kWgBatchMax layers
    for on in ({"wgrad64_direct": 1}, {"wgrad64_wino_nodep": 1}):
        with hooks(tlib, **on):
            assert counts(tlib, False, 11, dims) == [1] * 11


def test_bf16_chunk_and_route_rules(tlib):
    dims = (4, 32, 32, 32)
    with hooks(tlib):
        assert counts(tlib, True, 8, dims) == [4, 4]
        assert counts(tlib, True, 11, dims) == [7, 4]
        # 15 = 7 + 4 + 4: the 8 left behind the first chunk go out as 4 + 4, as 8 layers do.  No layer count leaves a lone bf16 layer behind
        # chunks (a remainder above 7 loses 7 until it is 8 or less, and 8 never becomes 7 + 1), so bf16 single steps exist only unbatched.
        assert [(s["count"], s["route"]) for s in plan(tlib, True, 15, *dims)[0]] == [(7, "bf16_batch"), (4, "bf16_batch"), (4, "bf16_batch")]
        for n in range(2, 70):
            assert min(counts(tlib, True, n, dims)) >= 2 and max(counts(tlib, True, n, dims)) <= 7
        assert counts(tlib, True, 7, dims) == [7]
        assert counts(tlib, True, 11, (5, 16, 16, 16)) == [7, 4]              # 5 * 16 * 2 * 2 = 320 one-plane tiles: the smallest batch
        assert counts(tlib, True, 11, (4, 16, 16, 16)) == [1] * 11            # 256 tiles
        assert counts(tlib, True, 11, (1, 320, 8, 8)) == [7, 4] and counts(tlib, True, 11, (1, 319, 8, 8)) == [1] * 11
        big = plan(tlib, True, 3, 16, 128, 128, 128)                            # 4 GB of rows: the register-staged kernel, layer by layer
        assert [(s["count"], s["route"]) for s in big[0]] == [(1, "bf16_reg")] * 3 and big[2] == 1
        assert plan(tlib, False, 1, 16, 128, 128, 128)[2] == 0                  # fp32: 8 GB of rows are refused (32-bit buffer addressing)
        assert plan(tlib, False, 1, 4, 128, 128, 128)[2] == 1
    with hooks(tlib, wgrad64_bf16_variant=1):
        assert [(s["count"], s["route"]) for s in plan(tlib, True, 11, *dims)[0]] == [(1, "bf16_reg")] * 11


# ------------------------------------------------------------------------------------------------ 4. the committed launch plans
def test_plan_reproduces_the_committed_launch_plans(tlib):
    """Every wgrad_* key of test_gpu_plan_coverage.PLAN_CASES (recorded from launches on the device): the plan of the case's shape holds a
    step with the key's route, layers, splits and nseg, its tile walk ends as the key says, and it fills the 256 CUs as the key says."""
    cases = importlib.import_module("test_gpu_plan_coverage").PLAN_CASES
    keys = [k for k in cases if " fam=wgrad_" in k]
    assert len(keys) >= 23
    for key in keys:
        entry, rec = key.split()[0], dict(kv.split("=") for kv in key.split()[1:])
        dt, algo, N, D, H, W, nl = cases[key]
        route = {"wgrad_direct": "direct", "wgrad_wino": "wino_dep" if rec.get("dep") == "1" else "wino_w", "wgrad_wino_batch": "wino_batch",
                 "wgrad_bf16_dma": "bf16_dma", "wgrad_bf16_reg": "bf16_reg", "wgrad_bf16_batch": "bf16_batch"}[rec["fam"]]
        with hooks(tlib):
            steps = plan(tlib, dt == "bf16", nl if entry.endswith("_batch") else 1, N, D, H, W, {"auto": AUTO, "direct": DIRECT}[algo])[0]
        hit = [s for s in steps if s["route"] == route and s["count"] == int(rec.get("layers", 1)) and s["splits"] == int(rec["splits"])
               and ("nseg" not in rec or s["nseg"] == int(rec["nseg"]))
               and ("partial" if s["tiles"] % s["splits"] else "full") == rec["tail"] and ("one" if s["grid"] <= 256 else "several") == rec["rounds"]]
        assert hit, (key, cases[key], steps)

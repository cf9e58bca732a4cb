"""Regenerates wgrad64_plan_golden.json: what the four weight-gradient size queries answer over a sweep of grids (no GPU needed).

    python tests/golden/make_wgrad64_plan_golden.py [REPO_ROOT]

REPO_ROOT (default: this checkout) is the tree whose library answers; the committed table was recorded from the library before route,
chunks, splits and workspace of the 64->64 weight gradient moved into one function (csrc/wgrad64_plan.h: fdn_wgrad64_plan), and
tests/test_wgrad64_plan.py holds every later library to it.

Layout: every 64->64 answer is a whole number of UNIT = 9 x 64 x 64 floats and is stored in that unit.  "single": one row per (N, D),
H-major over HWS x HWS.  "batch": per (N, D) and layer count an index into "batch_rows", the distinct rows of that kind (most layer
counts of a grid share one: the single-layer bound dominates).  "other": [query, arguments, bytes] for the rest."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "wgrad64_plan_golden.json")

UNIT = 9 * 64 * 64 * 4
NS = (1, 2, 5, 8)
DS = (1, 5, 8, 24)
HWS = (5, 8, 12, 16, 24, 32, 48)
LAYERS = (0, 1, 2, 3, 7, 8, 9, 11, 15, 16, 17, 32, 33)
SINGLE = {"f32": "fdn_conv3d_wgrad_workspace_bytes", "bf16": "fdn_conv3d_wgrad_bf16_workspace_bytes"}
BATCH = {"f32": "fdn_conv3d_wgrad_batch_workspace_bytes", "bf16": "fdn_conv3d_wgrad_bf16_batch_workspace_bytes"}
SMALL = ((3, 64, 3), (128, 64, 1), (64, 1, 3), (64, 64, 1), (32, 32, 3))          # the non-64->64 shapes (the last two: unsupported)
BIG = ((1, 128, 128, 128), (4, 128, 128, 128), (16, 128, 128, 128), (3, 256, 256, 256))      # 128^3; the last two: 4 GB of bf16 rows and more


def other_cases():
    """[(query, args)]: the non-64->64 shapes, the invalid extents (0, -1) in every position, 128^3 and grids past 4 GB."""
    cases = []
    for q in SINGLE.values():
        cases += [(q, (N, D, D, D) + ckk) for ckk in SMALL for (N, D) in ((1, 8), (8, 24))]
        cases += [(q, tuple(bad if i == pos else v for i, v in enumerate((8, 24, 24, 24))) + (64, 64, 3)) for pos in range(4) for bad in (0, -1)]
        cases += [(q, g + (64, 64, 3)) for g in BIG]
    for q in BATCH.values():
        cases += [(q, tuple(bad if i == pos else v for i, v in enumerate((8, 8, 24, 24, 24)))) for pos in range(5) for bad in (0, -1)]
        cases += [(q, (n,) + g) for g in BIG for n in (1, 2, 8, 11)]
    return cases


def record(lib):
    grid = {"N": NS, "D": DS, "HW": HWS, "layers": LAYERS}

    def units(v):
        assert v % UNIT == 0, v
        return v // UNIT

    single = {dt: {"%d %d" % (N, D): [units(getattr(lib, q)(N, D, H, W, 64, 64, 3)) for H in HWS for W in HWS] for N in NS for D in DS}
              for dt, q in SINGLE.items()}
    rows, batch = [], {}
    for dt, q in BATCH.items():
        batch[dt] = {}
        for N in NS:
            for D in DS:
                idx = []
                for n in LAYERS:
                    row = [units(getattr(lib, q)(n, N, D, H, W)) for H in HWS for W in HWS]
                    if row not in rows:
                        rows.append(row)
                    idx.append(rows.index(row))
                batch[dt]["%d %d" % (N, D)] = idx
    other = [[q, list(a), int(getattr(lib, q)(*a))] for q, a in other_cases()]
    return {"grid": grid, "unit": UNIT, "single": single, "batch": batch, "batch_rows": rows, "other": other}


def dump(table, f):
    """One row per line."""
    def rows_of(v):
        if isinstance(v, dict):
            return "{\n%s\n  }" % ",\n".join("    %s: %s" % (json.dumps(k), json.dumps(r, separators=(",", ":"))) for k, r in v.items())
        return "[\n%s\n  ]" % ",\n".join("    " + json.dumps(r, separators=(",", ":")) for r in v)

    parts = []
    for k, v in table.items():
        if k in ("single", "batch"):
            body = "{\n%s\n  }" % ",\n".join("  %s: %s" % (json.dumps(dt), rows_of(t).replace("\n", "\n  ")) for dt, t in v.items())
        elif k in ("batch_rows", "other"):
            body = rows_of(v)
        else:
            body = json.dumps(v, separators=(",", ":"))
        parts.append("  %s: %s" % (json.dumps(k), body))
    f.write("{\n%s\n}\n" % ",\n".join(parts))


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, root)
    lib = importlib.import_module("4dflownet_amd._lib").load()
    with open(OUT, "w") as f:
        dump(record(lib), f)
    json.load(open(OUT))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

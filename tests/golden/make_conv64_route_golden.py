"""Regenerates conv64_route_golden.json: what fdn_conv64_pack_streams and fdn_conv64_mask_ok answer over a sweep of grids (no GPU needed).

    python tests/golden/make_conv64_route_golden.py [REPO_ROOT]

REPO_ROOT (default: this checkout) is the tree whose library answers; the committed table was recorded from the library before the
fp32 64->64 selection moved into one function (conv64_route), and tests/test_conv64_route.py holds every later library to it."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "conv64_route_golden.json")

NS = (1, 8, 64)                                          # both sides of the 24 576-voxel threshold of the aligned-box split
DS = (5, 24)
HWS = (5, 6, 8, 9, 10, 12, 14, 18, 22, 24, 48)
BIG = (160, 162)                                         # 160^3 < 2^22 voxels < 162^3: the sample limit of the 2-D kernels
ALGOS = range(5)
ROLES = range(3)
INVALID = [(0, 24, 24, 24, 0, 0), (8, 0, 24, 24, 0, 0), (8, 24, -1, 24, 0, 0), (8, 24, 24, 1021, 0, 0), (8, 24, 24, 24, -1, 0),
           (8, 24, 24, 24, 5, 0), (8, 24, 24, 24, 0, -1), (8, 24, 24, 24, 0, 3), (1, 300, 300, 300, 0, 0), (1, 300, 300, 300, 0, 2)]


def record(lib):
    ps, ok = lib.fdn_conv64_pack_streams, lib.fdn_conv64_mask_ok
    grid = {"N": NS, "D": DS, "HW": HWS, "big": BIG}
    streams, masks = {}, {}
    for N in NS:
        for D in DS:
            for algo in ALGOS:
                for role in ROLES:              # one row per (N, D, algo, role): H-major over HWS x HWS
                    streams["%d %d %d %d" % (N, D, algo, role)] = [ps(N, D, H, W, algo, role) for H in HWS for W in HWS]
                masks["%d %d %d" % (N, D, algo)] = [ok(N, D, H, W, algo) for H in HWS for W in HWS]
    big = [[N, S, algo] + [ps(N, S, S, S, algo, role) for role in ROLES] + [ok(N, S, S, S, algo)]
           for N in NS for S in BIG for algo in ALGOS]
    invalid = [list(a) + [ps(*a), ok(*a[:5])] for a in INVALID]
    return {"grid": grid, "pack_streams": streams, "mask_ok": masks, "big": big, "invalid": invalid}


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, root)
    lib = importlib.import_module("4dflownet_amd._lib").load()
    table = record(lib)
    with open(OUT, "w") as f:
        f.write("{\n")
        items = list(table.items())
        for i, (k, v) in enumerate(items):
            if isinstance(v, dict):
                rows = ",\n".join("    %s: %s" % (json.dumps(rk), json.dumps(rv, separators=(",", ":"))) for rk, rv in v.items())
                body = "{\n%s\n  }" % rows
            else:
                body = json.dumps(v, separators=(",", ":"))
            f.write("  %s: %s%s\n" % (json.dumps(k), body, "," if i + 1 < len(items) else ""))
        f.write("}\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

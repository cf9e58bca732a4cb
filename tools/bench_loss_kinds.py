"""Times of the loss call for every penalty of the data term (mse, mae, huber, charbonnier) at the cfg2 shape (8,48^3) and at (4,128^3), with
and without dpred, and -- with --old-lib, a library built from the parent commit -- the MSE calls through that library in the same
process, alternating, on the same box, with a bit-for-bit comparison of what the two libraries return.  --extra-lib NAME=PATH times the
MSE calls of further builds of this source (a variant under study) the same way.
   python tools/bench_loss_kinds.py [--old-lib path/to/lib4dflow_hip.so] [--extra-lib NAME=PATH ...] [--calls 200] [--reps 5]"""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
fdn = importlib.import_module("4dflownet_amd")
build = importlib.import_module("4dflownet_amd.build")
ACT_NONE, ACT_TANH = 0, 3
KINDS = [("mse", 0, 0.0), ("mae", 1, 0.0), ("huber 0.25", 2, 0.25), ("charbonnier 1e-3", 3, 1e-3)]
OLD_ENTRIES = ("fdn_loss_metrics", "fdn_loss_metrics_div", "fdn_loss_metrics_act")


def load_other(path):
    lib = ctypes.CDLL(path)
    for name in OLD_ENTRIES:
        res, args = fdn._lib.SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def timed(fn, calls, reps):
    """Median over reps of the mean time of `calls` back-to-back launches, in ms."""
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record(); b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-lib")
    ap.add_argument("--extra-lib", action="append", default=[])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    new = fdn._lib.load()
    others = ([("old", load_other(a.old_lib))] if a.old_lib else []) + [(s.split("=", 1)[0], load_other(s.split("=", 1)[1])) for s in a.extra_lib]
    print("# %s; library stamp %s (sources in the tree: %s)" % (torch.cuda.get_device_name(0), build.built_stamp()[:16], build.source_stamp()[:16]))
    if a.old_lib and os.path.exists(a.old_lib + ".stamp"):
        print("# old library stamp %s" % open(a.old_lib + ".stamp").read()[:16])
    print("# median of %d reps of %d calls, best of 2 alternating passes; ms per call (memset + 3 launches)" % (a.reps, a.calls))
    st = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr() if x is not None else None
    for N, S in ((8, 48), (4, 128)):
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s: torch.rand(*s, device="cuda", generator=g) * 1.8 - 0.9
        pred, t = rnd(N, S, S, S, 3), [rnd(N, S, S, S) for _ in range(3)]
        mask = (torch.rand(N, S, S, S, device="cuda", generator=g) < 0.3).float()
        out, dp, scratch = torch.empty(N, 5, device="cuda"), torch.empty_like(pred), torch.empty(N * (8 + 5 * 256), device="cuda")
        plain = lambda lib, d: lib.fdn_loss_metrics(P(pred), P(t[0]), P(t[1]), P(t[2]), P(mask), P(out), P(d), P(scratch), N, S ** 3, st)
        div = lambda lib, d: lib.fdn_loss_metrics_div(P(pred), P(t[0]), P(t[1]), P(t[2]), P(mask), 0.8, P(out), P(d), P(scratch), N, S, S, S, st)
        act = lambda lib, d, w=0.0: lib.fdn_loss_metrics_act(P(pred), P(t[0]), P(t[1]), P(t[2]), P(mask), w, 0.25, ACT_TANH, P(out), P(d), P(scratch),
                                                             N, S, S, S, st)
        kind = lambda k, kp, w, d: new.fdn_loss_metrics_kind(P(pred), P(t[0]), P(t[1]), P(t[2]), P(mask), k, kp, w, 0.25, ACT_TANH, P(out), P(d),
                                                             P(scratch), N, S, S, S, st)
        # what the MSE entry points return: the same bits from every library
        for label, call in (("plain", plain), ("div 0.8", div), ("act nf 0.25 tanh", act), ("act div 0.8 nf 0.25 tanh", lambda lib, d: act(lib, d, 0.8))):
            ref = None
            for name, lib in [("new", new)] + others:
                out.fill_(-1); dp.fill_(-1)
                assert call(lib, dp) == 0, (label, name)
                torch.cuda.synchronize()
                got = (out.clone(), dp.clone())
                if ref is None:
                    ref = got
                else:
                    same = torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
                    print("# (%d,%d^3) %-26s new vs %-6s: %s" % (N, S, label, name, "bit-identical out and dpred" if same else "DIFFERENT"))
        rows = []
        for gname, d in (("dpred", dp), ("no dpred", None)):
            for name, lib in [("new", new)] + others:
                rows.append(("mse plain, %s" % gname, name, lambda lib=lib, d=d: plain(lib, d)))
                rows.append(("mse div 0.8, %s" % gname, name, lambda lib=lib, d=d: div(lib, d)))
                rows.append(("mse act nf 0.25 tanh, %s" % gname, name, lambda lib=lib, d=d: act(lib, d)))
                rows.append(("mse act div 0.8 nf 0.25 tanh, %s" % gname, name, lambda lib=lib, d=d: act(lib, d, 0.8)))
            for kname, k, kp in KINDS:
                for w in (0.0, 0.8):
                    rows.append(("%s kind div %g nf 0.25 tanh, %s" % (kname, w, gname), "new", lambda k=k, kp=kp, w=w, d=d: kind(k, kp, w, d)))
        for r in rows:
            assert r[2]() == 0, (r[0], r[1], new.fdn_last_error())
        torch.cuda.synchronize()
        res = {}
        for _ in range(2):
            for label, name, fn in rows:
                ms = timed(fn, a.calls, a.reps)
                res[(label, name)] = min(ms, res.get((label, name), 1e9))
        print("# (%d,%d^3)" % (N, S))
        for label, name, _ in rows:
            print("%-52s %-6s %.4f ms" % (label, name, res[(label, name)]))


if __name__ == "__main__":
    main()

"""Times of the loss call and of head_fwd at (8,48^3) with and without the output-activation / non_fluid_weight options, and -- with
--old-lib, a library built from another commit -- the same calls through that library in the same process, alternating, on the same
box.   python tools/bench_output_activation.py [--old-lib path/to/lib4dflow_hip.so] [--calls 200] [--reps 5]"""
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
ACT_NONE, ACT_TANH = 0, 3


def load_old(path):
    lib = ctypes.CDLL(path)
    for name in ("fdn_loss_metrics", "fdn_loss_metrics_div", "fdn_conv3d_fwd", "fdn_conv3d_fwd_bf16"):
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    new = fdn._lib.load()
    libs = [("new", new)] + ([("old", load_old(a.old_lib))] if a.old_lib else [])
    N, S = 8, 48
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g) * 1.8 - 0.9
    pred, t, mask = rnd(N, S, S, S, 3), [rnd(N, S, S, S) for _ in range(3)], (torch.rand(N, S, S, S, device="cuda", generator=g) < 0.3).float()
    out, dp, scratch = torch.empty(N, 5, device="cuda"), torch.empty_like(pred), torch.empty(N * (8 + 5 * 256), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()
    rows = []
    for name, lib in libs:
        rows.append(("loss plain", name, lambda lib=lib: lib.fdn_loss_metrics(P(pred), P(t[0]), P(t[1]), P(t[2]), P(mask), P(out), P(dp), P(scratch), N, S ** 3, st)))
        rows.append(("loss div 0.8", name, lambda lib=lib: lib.fdn_loss_metrics_div(P(pred), P(t[0]), P(t[1]), P(t[2]), P(mask), 0.8, P(out), P(dp), P(scratch), N, S, S, S, st)))
    for label, dw, nfw, act in (("loss act div 0 nf 0.25", 0.0, 0.25, ACT_NONE), ("loss act div 0 tanh", 0.0, 1.0, ACT_TANH),
                                ("loss act div 0.8 nf 0.25 tanh", 0.8, 0.25, ACT_TANH)):
        rows.append((label, "new", lambda dw=dw, nfw=nfw, act=act: new.fdn_loss_metrics_act(P(pred), P(t[0]), P(t[1]), P(t[2]), P(mask), dw, nfw, act, P(out),
                                                                                             P(dp), P(scratch), N, S, S, S, st)))
    x = torch.randn(N, S, S, S, 64, device="cuda", generator=g)
    xb = x.to(torch.bfloat16)
    w, b, y = torch.randn(3, 3, 3, 64, 1, device="cuda", generator=g) * 0.05, torch.zeros(1, device="cuda"), torch.empty(N, S, S, S, 3, device="cuda")
    for name, lib in libs:
        for act in ((ACT_NONE, ACT_TANH) if name == "new" else (ACT_NONE,)):
            rows.append(("head_fwd f32 act %d" % act, name, lambda lib=lib, act=act: lib.fdn_conv3d_fwd(P(x), None, P(w), None, P(b), None, P(y), N, S, S, S, 64, 1, 3, 3, 1, act, 0.2, 0, st)))
            rows.append(("head_fwd bf16 act %d" % act, name, lambda lib=lib, act=act: lib.fdn_conv3d_fwd_bf16(P(xb), None, P(w), None, P(b), None, P(y), N, S, S, S, 64, 1, 3, 3, 1, act, 0.2, st)))
    for r in rows:
        assert r[2]() == 0, (r[0], r[1])
    torch.cuda.synchronize()
    # two alternating passes over all rows, the better of the two per row
    res = {}
    for _ in range(2):
        for label, name, fn in rows:
            ms = timed(fn, a.calls, a.reps)
            res[(label, name)] = min(ms, res.get((label, name), 1e9))
    print("# %s, (8,48^3), median of %d reps of %d calls, best of 2 alternating passes" % (torch.cuda.get_device_name(0), a.reps, a.calls))
    for label, name, _ in rows:
        print("%-34s %-3s %.4f ms" % (label, name, res[(label, name)]))


if __name__ == "__main__":
    main()

"""Gradient accumulation priced: one optimiser step on a fixed global batch, split into accum_steps micro-batches.
python tools/bench_accum.py [--steps N] [--cases cfg2,cfg4] [--only-plain]
  cfg2 (patch 24, res x2, 8+4 blocks, float32), global batch 8 as 1x8, 2x4, 4x2, 8x1 (accum_steps x micro-batch)
  cfg4 (patch 32, res x4, 8+4 blocks, bfloat16), global batch 4 as 1x4, 2x2, 4x1
Per case (its own controller, the peak counters reset after the weights exist): wall time per optimiser step and patches/s over N
optimiser steps in three runs, torch.cuda.max_memory_allocated / max_memory_reserved, and the HIP-event time of one
fdn_grad_accumulate over that configuration's parameter count + 1 (median of 200 calls).
--only-plain: the cfg2 1x8 case alone, seven runs -- the line a same-box A/B against another commit compares (tools/ab_files.sh)."""
import argparse
import importlib
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
trainer = importlib.import_module("4dflownet_amd.trainer")
build = importlib.import_module("4dflownet_amd.build")

CONFIGS = {"cfg2": dict(P=24, R=2, LB=8, HB=4, dtype="float32", batch=8, splits=(1, 2, 4, 8)),
           "cfg4": dict(P=32, R=4, LB=8, HB=4, dtype="bfloat16", batch=4, splits=(1, 2, 4))}


def synthetic(B, P, R, rng):
    f = lambda lo, hi, s: rng.uniform(lo, hi, s).astype(np.float32)
    S = P * R
    return tuple([f(-1, 1, (B, P, P, P, 1)) for _ in range(3)] + [f(0, 0.016, (B, P, P, P, 1)) for _ in range(3)] +
                 [f(-0.45, 0.45, (B, S, S, S, 1)) for _ in range(3)] + [np.full((B,), 1.5, np.float32), (rng.random((B, S, S, S)) < 0.12).astype(np.float32)])


def time_accumulate(tc, calls=200):
    ops = trainer.ops
    if not hasattr(ops, "grad_accumulate"):
        return None
    g = tc.model.flat_g_ext
    acc = torch.empty_like(g)
    ops.grad_accumulate(acc, g, True)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record(); ops.grad_accumulate(acc, g, False); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3          # us


def run_case(name, K, steps, runs):
    c = CONFIGS[name]
    kw = {"accum_steps": K} if K > 1 else {}                      # (K = 1 also runs on a tree without the argument: the A/B's other side)
    tc = trainer.TrainerController(c["P"], c["R"], quicksave_enable=False, low_resblock=c["LB"], hi_resblock=c["HB"], dtype=c["dtype"], **kw)
    mb = c["batch"] // K
    rng = np.random.default_rng(1234)
    whole = synthetic(c["batch"], c["P"], c["R"], rng)
    micro = [tuple(tc.model._to_dev(a[k * mb:(k + 1) * mb]) for a in whole) for k in range(K)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step = lambda: [tc.train_step(b) for b in micro]
    for _ in range(3):
        step()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    assert tc.optimizer.iterations == (3 + runs * steps)
    alloc, reserved = torch.cuda.max_memory_allocated(), torch.cuda.max_memory_reserved()
    us = time_accumulate(tc)
    med = float(np.median(ms))
    print("%s %dx%d  optimiser step: runs %s ms; median %.3f ms (min %.3f .. max %.3f) = %.1f patches/s | peak allocated %.3f GB, reserved %.3f GB | "
          "fdn_grad_accumulate over %d floats: %s" % (name, K, mb, " ".join("%.3f" % m for m in ms), med, min(ms), max(ms), c["batch"] / med * 1e3,
                                                      alloc / 1e9, reserved / 1e9, tc.model.n_params + 1, "n/a" if us is None else "%.1f us" % us), flush=True)
    del tc, micro
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--cases", default="cfg2,cfg4")
    ap.add_argument("--only-plain", action="store_true")
    a = ap.parse_args()
    commit = os.environ.get("FDN_COMMIT")                  # a snapshot of the tree without its history: the caller names the commit
    if not commit:
        r = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        d = subprocess.run(["git", "status", "--porcelain"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() + ("+dirty" if d.stdout.strip() else "") if r.returncode == 0 else "unknown"
    print("# commit %s lib_source_stamp %s" % (commit, build.source_stamp()))
    print("# tools/bench_accum.py %s: %s, host wall time between device synchronisations, batches resident on the device" % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)))
    if a.only_plain:
        run_case("cfg2", 1, a.steps or 30, 7)
        return
    for name in a.cases.split(","):
        for K in CONFIGS[name]["splits"]:
            run_case(name, K, a.steps or (30 if name == "cfg2" else 12), 3)


if __name__ == "__main__":
    main()

"""Fine-tuning priced: the cfg2 train step (patch 24, res x2, 8+4 blocks, float32, batch 8) with every layer trainable, with the low-res
stack frozen ("hires") and with everything but the six head layers frozen ("heads").
python tools/bench_finetune.py [--steps N] [--presets all,hires,heads] [--only-all]
Per preset (its own controller, the peak counters reset after the weights exist): wall time per optimiser step over N steps in three runs
and their median, patches/s, torch.cuda.max_memory_allocated / max_memory_reserved.
--only-all: the all-trainable case alone, built without the `trainable` argument, so it also runs on a tree that has no fine-tuning: the
line a same-box A/B against the parent commit compares (three runs on each side; the parent's spread is the yardstick)."""
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

CFG2 = dict(P=24, R=2, LB=8, HB=4, dtype="float32", batch=8)


def synthetic(B, P, R, rng):
    f = lambda lo, hi, s: rng.uniform(lo, hi, s).astype(np.float32)
    S = P * R
    return tuple([f(-1, 1, (B, P, P, P, 1)) for _ in range(3)] + [f(0, 0.016, (B, P, P, P, 1)) for _ in range(3)] +
                 [f(-0.45, 0.45, (B, S, S, S, 1)) for _ in range(3)] + [np.full((B,), 1.5, np.float32), (rng.random((B, S, S, S)) < 0.12).astype(np.float32)])


def run_case(preset, steps, runs):
    c = CFG2
    kw = {} if preset == "all" else {"trainable": preset}         # ("all" also runs on a tree without the argument: the A/B's other side)
    tc = trainer.TrainerController(c["P"], c["R"], quicksave_enable=False, low_resblock=c["LB"], hi_resblock=c["HB"], dtype=c["dtype"], **kw)
    batch = tuple(tc.model._to_dev(a) for a in synthetic(c["batch"], c["P"], c["R"], np.random.default_rng(1234)))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(3):
        tc.train_step(batch)
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps):
            tc.train_step(batch)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    assert tc.optimizer.iterations == 3 + runs * steps
    alloc, reserved = torch.cuda.max_memory_allocated(), torch.cuda.max_memory_reserved()
    med = float(np.median(ms))
    n_train = sum(t.numel() for t in tc.model.trainable_variables)
    print("cfg2 trainable=%-5s (%d of %d parameters)  optimiser step: runs %s ms; median %.3f ms (min %.3f .. max %.3f) = %.1f patches/s | "
          "peak allocated %.3f GB, reserved %.3f GB" % (preset, n_train, tc.model.n_params, " ".join("%.3f" % m for m in ms), med, min(ms), max(ms),
                                                        c["batch"] / med * 1e3, alloc / 1e9, reserved / 1e9), flush=True)
    del tc, batch
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--presets", default="all,hires,heads")
    ap.add_argument("--only-all", action="store_true")
    a = ap.parse_args()
    commit = os.environ.get("FDN_COMMIT")                  # a snapshot of the tree without its history: the caller names the commit
    if not commit:
        r = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        d = subprocess.run(["git", "status", "--porcelain"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() + ("+dirty" if d.stdout.strip() else "") if r.returncode == 0 else "unknown"
    print("# commit %s lib_source_stamp %s" % (commit, build.source_stamp()))
    print("# tools/bench_finetune.py %s: %s, host wall time between device synchronisations, batch resident on the device" % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)))
    for preset in (["all"] if a.only_all else a.presets.split(",")):
        run_case(preset, a.steps, 3)


if __name__ == "__main__":
    main()

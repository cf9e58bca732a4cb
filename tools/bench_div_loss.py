"""Cost of the divergence loss (fdn_loss_metrics_div): ops.loss_metrics plain and with the term, and the cfg2 train step with
div_weight 0 and 0.5, alternating in one process.
python tools/bench_div_loss.py [--commit SHA] [--calls 400] [--reps 5] [--steps 30]
Per loss shape: HIP events around each call (dpred written, as in train_step), 20 warm-up calls, median of --calls calls.
Train step: --reps rounds of --steps steps per weight after 5 warm-up steps, the order of the two weights alternating per round."""
import argparse
import importlib
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ops = importlib.import_module("4dflownet_amd.ops")
build = importlib.import_module("4dflownet_amd.build")
trainer = importlib.import_module("4dflownet_amd.trainer")


def commit():
    try:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        if r.returncode == 0:
            d = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True, text=True)
            return r.stdout.strip() + ("+dirty" if d.stdout.strip() else "")
    except OSError:
        pass
    return "unknown"


def time_calls(fn, calls, warmup=20):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def loss_shapes(calls):
    rng = np.random.default_rng(7)
    for N, S in ((8, 48), (4, 128)):
        shp = (N, S, S, S)
        pred = torch.from_numpy(rng.uniform(-0.5, 0.5, shp + (3,)).astype(np.float32)).cuda()
        t = [torch.from_numpy(rng.uniform(-0.45, 0.45, shp).astype(np.float32)).cuda() for _ in range(3)]
        mask = torch.from_numpy((rng.random(shp) < 0.12).astype(np.float32)).cuda()
        out4, out5 = torch.empty((N, 4), device="cuda"), torch.empty((N, 5), device="cuda")
        s3, s5 = torch.empty(N * (8 + 3 * 256), device="cuda"), torch.empty(N * (8 + 5 * 256), device="cuda")
        dp = torch.empty_like(pred)
        plain = lambda: ops.loss_metrics(pred, t[0], t[1], t[2], mask, out=out4, dpred=dp, scratch=s3)
        div = lambda: ops.loss_metrics(pred, t[0], t[1], t[2], mask, out=out5, dpred=dp, scratch=s5, div_weight=0.5)
        res = {}
        for rep in range(2):                                  # alternate: clock drift must not pick the winner
            for name, fn in ((("plain", plain), ("div", div)) if rep == 0 else (("div", div), ("plain", plain))):
                res.setdefault(name, []).append(time_calls(fn, calls))
        p, d = min(res["plain"]), min(res["div"])
        nbytes = N * S ** 3 * 4 * (3 + 3 + 1 + 3)            # pred, truth, mask read once, dpred written
        print("loss_metrics (%d,%d^3): plain %.4f ms  div %.4f ms  ratio %.2f  (plain-pass bytes %.1f MB: %.0f / %.0f GB/s)  "
              "[median of %d calls, best of 2 alternating runs]" % (N, S, p, d, d / p, nbytes / 1e6, nbytes / p / 1e6, nbytes / d / 1e6,
                                                                   calls), flush=True)


def train_steps(reps, steps):
    P, R, B, LB, HB = 24, 2, 8, 8, 4                           # cfg2
    rng = np.random.default_rng(1234)
    f = lambda lo, hi, s: rng.uniform(lo, hi, s).astype(np.float32)
    batch = tuple([f(-1, 1, (B, P, P, P, 1)) for _ in range(3)] + [f(0, 0.016, (B, P, P, P, 1)) for _ in range(3)] +
                  [f(-0.45, 0.45, (B, P * R, P * R, P * R, 1)) for _ in range(3)] +
                  [np.full((B,), 1.5, np.float32), (rng.random((B, P * R, P * R, P * R)) < 0.12).astype(np.float32)])
    tc = trainer.TrainerController(P, R, quicksave_enable=False, low_resblock=LB, hi_resblock=HB)
    dev = tuple(tc.model._to_dev(a) for a in batch)
    res = {0.0: [], 0.5: []}
    for rep in range(reps):
        for w in ((0.0, 0.5) if rep % 2 == 0 else (0.5, 0.0)):
            tc.div_weight = w
            for _ in range(5):
                tc.train_step(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                tc.train_step(dev)
            e1.record()
            torch.cuda.synchronize()
            res[w].append(e0.elapsed_time(e1) / steps)
            print("cfg2 train_step div_weight=%.1f: %.3f ms/step" % (w, res[w][-1]), flush=True)
    for w in (0.0, 0.5):
        print("cfg2 train_step div_weight=%.1f: median %.3f ms/step, min %.3f, max %.3f over %d runs of %d steps" % (
            w, np.median(res[w]), min(res[w]), max(res[w]), reps, steps))
    print("cfg2 step growth with the divergence term: %+.3f ms (medians)" % (np.median(res[0.5]) - np.median(res[0.0])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    assert a.calls >= 200
    print("# commit %s lib_source_stamp %s" % (a.commit or commit(), build.source_stamp()), flush=True)
    print("# %s, tools/bench_div_loss.py --calls %d --reps %d --steps %d" % (torch.cuda.get_device_name(0), a.calls, a.reps, a.steps),
          flush=True)
    loss_shapes(a.calls)
    if not a.skip_train:
        train_steps(a.reps, a.steps)

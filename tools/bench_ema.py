"""Cost of the weight EMA: the optimiser launch alone on the cfg2 parameter buffer with and without an average, the copies and re-packs
of ema_weights(), and the cfg2 train step with use_ema off / on, alternating in one process.
python tools/bench_ema.py [--commit SHA] [--calls 400] [--reps 5] [--steps 30]
Launches: HIP events around each call, 20 warm-up calls, median of --calls calls, best of two alternating runs.
Train step: --reps rounds of --steps steps per setting after 5 warm-up steps, the order of the settings alternating per round."""
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

P, R, B, LB, HB = 24, 2, 8, 8, 4                           # cfg2
SETTINGS = (("off", False), ("on", True))


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


def optimiser_launches(tc, calls):
    """The optimiser launch on buffers of the model's size (copies: the model itself is left alone)."""
    m = tc.model
    n = m.n_params
    w, isk = m.flat_w.clone(), m.is_kernel
    g = torch.from_numpy((1e-3 * np.random.default_rng(7).standard_normal(n)).astype(np.float32)).cuda()
    mm, vv, ema, spare = torch.zeros_like(w), torch.zeros_like(w), w.clone(), torch.empty_like(w)
    slot = torch.tensor([float(B)], device="cuda")
    part = torch.zeros(ops.ADAM_PARTIALS, device="cuda")
    l2gs = 2.0 * trainer.L2_LAMBDA
    lr_t = 1e-4                                               # (a fixed step size: the buffers must not drift into denormals over the calls)
    adam = lambda **kw: ops.adam_step(w, g, mm, vv, isk, lr_t, 0.9, 0.999, 1e-7, l2gs, slot, sumsq_partials=part, **kw)
    fns = (("off", adam), ("ema", lambda: adam(ema=ema, ema_momentum=0.99)), ("ema, first step (ema_init)", lambda: adam(ema=ema, ema_momentum=0.99, ema_init=True)),
           ("one bit copy of the parameters (grad_accumulate first)", lambda: ops.grad_accumulate(spare, w, True)))
    res = {}
    for rep in range(2):                                      # alternate: clock drift must not pick the winner
        for name, fn in (fns if rep == 0 else fns[::-1]):
            res.setdefault(name, []).append(time_calls(fn, calls))
    base = min(res["off"])
    for name, _ in fns:
        t = min(res[name])
        print("optimiser launch, %d parameters (%.1f MB), %s: %.4f ms  (%+.4f ms against off)  [median of %d calls, best of 2 "
              "alternating runs]" % (n, 4 * n / 1e6, name, t, t - base, calls), flush=True)


def train_steps(tc, reps, steps, calls):
    rng = np.random.default_rng(1234)
    f = lambda lo, hi, s: rng.uniform(lo, hi, s).astype(np.float32)
    batch = tuple([f(-1, 1, (B, P, P, P, 1)) for _ in range(3)] + [f(0, 0.016, (B, P, P, P, 1)) for _ in range(3)] +
                  [f(-0.45, 0.45, (B, P * R, P * R, P * R, 1)) for _ in range(3)] +
                  [np.full((B,), 1.5, np.float32), (rng.random((B, P * R, P * R, P * R)) < 0.12).astype(np.float32)])
    dev = tuple(tc.model._to_dev(a) for a in batch)
    res = dict((name, []) for name, _ in SETTINGS)
    for rep in range(reps):
        for name, on in (SETTINGS if rep % 2 == 0 else SETTINGS[::-1]):
            tc.use_ema = on
            for _ in range(5):
                tc.train_step(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                tc.train_step(dev)
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / steps)
            print("cfg2 train_step use_ema %s: %.3f ms/step" % (name, res[name][-1]), flush=True)
    for name, _ in SETTINGS:
        print("cfg2 train_step use_ema %s: median %.3f ms/step, min %.3f, max %.3f over %d runs of %d steps" % (
            name, np.median(res[name]), min(res[name]), max(res[name]), reps, steps))
    print("cfg2 step growth with use_ema: %+.3f ms (medians)" % (np.median(res["on"]) - np.median(res["off"])))

    def enter_and_leave():
        with tc.ema_weights():
            pass
    tc.use_ema = True
    tc.train_step(dev)
    print("ema_weights() entered and left (three bit copies, two re-packs of all 64->64 layers): %.4f ms  [median of %d calls]"
          % (time_calls(enter_and_leave, calls), calls))


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
    print("# %s, tools/bench_ema.py --calls %d --reps %d --steps %d" % (torch.cuda.get_device_name(0), a.calls, a.reps, a.steps), flush=True)
    tc = trainer.TrainerController(P, R, quicksave_enable=False, low_resblock=LB, hi_resblock=HB)
    optimiser_launches(tc, a.calls)
    if not a.skip_train:
        train_steps(tc, a.reps, a.steps, a.calls)

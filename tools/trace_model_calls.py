"""Which library calls does a train step make?  Wraps what _lib.load() returns in a recording proxy and prints one line per call of
lib4dflow_hip.so: the entry point, every integer / float argument, for the pointer arguments NULL or a letter (equal letters = equal
pointers within that call; no addresses) and the stream, main or side.  Per case: sha256 of that trace, of an inference prediction, of
flat_g after train step 1 and of flat_w after train step 2, and torch.cuda.max_memory_allocated().  Two checkouts that print the same
table issue the same launches with the same arguments in the same order and compute the same bits: what a refactor of ops.py /
ops_bf16.py / network.py has to show.  A second group of cases, step_*, does the same for the optimiser step (what runs between
backward() and the moved weights), where a refactor of trainer.py has to show it.

    python tools/trace_model_calls.py [--dump DIR] [--only SUBSTRING]

Cases: LB = HB = 1, B = 2, both dtypes, P=8 R=2 (8^3 / 16^3: sign masks, batched weight gradients and the multi-source head dgrad all
apply), P=6 R=2 (6^3 falls off the Winograd kernels, 12^3 does not), P=5 R=1 (odd extents: chained heads, no batch); the defaults, each of
sign_masks / multi_dgrad / batch_wgrad / overlap_wgrad switched off on its own, conv_algo "direct", "winograd_w" and {first head: "direct"}.

step_* cases: fp32, P=8 R=2, LB = HB = 1, B = 2.  Per case: sha256 of the trace, of flat_w, optimizer.m, optimizer.v and the step buffer
(accum_g_ext where there is one, else flat_g_ext) after the last call, optimizer.iterations and max_memory_allocated.
  accum2                 accum_steps=2: three train_step calls, then apply_accumulated() twice (a full group, a ragged flush, a no-op)
  heads                  trainable="heads"
  clipnorm / clipvalue   an active clip: a quarter of the norm / of the largest |gradient| a probe step with a huge clipnorm reports
  accum2_heads_clipnorm  the three together
  dp_<bucketed|whole>_k<1|2>[_...]   the data-parallel ORDER in one process, without a process group: parallel.world_size is 2,
      allreduce_sum_start / allreduce_wait only record `allreduce_start(<g|acc>, offset, numel) @main|@side` / `allreduce_wait`, and a call
      of model._join_side records `join(busy=...)` -- where collectives and joins sit among the library calls.  With bucketed_allreduce
      on and off, K = 1 (two steps; a step and an empty-shard step, B = 0 rows) and K = 2 (three calls and a flush; groups whose first,
      whose closing and whose every micro-batch is empty)."""
import argparse
import contextlib
import ctypes
import functools
import gc
import hashlib
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_lib = importlib.import_module("4dflownet_amd._lib")
network = importlib.import_module("4dflownet_amd.network")
trainer = importlib.import_module("4dflownet_amd.trainer")
parallel = importlib.import_module("4dflownet_amd.parallel")


class Recorder:
    """Stands in for the ctypes library: every attribute is the library's function behind a wrapper that appends one line to .lines."""

    def __init__(self, lib):
        self._lib = lib
        self.lines = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        argtypes = _lib.SIGNATURES.get(name, (None, None))[1]
        if argtypes is None:
            return fn

        def call(*args):
            types, vals = list(argtypes), list(args)
            has_stream = bool(types) and types[-1] is ctypes.c_void_p            # every launching entry point ends with its stream
            if has_stream:
                types, vals = types[:-1], vals[:-1]
            letters, out = {}, []
            label = lambda p: "NULL" if not p else letters.setdefault(int(p), chr(ord("a") + len(letters)))
            for t, v in zip(types, vals):
                if t is not ctypes.c_void_p:
                    out.append(repr(float(v)) if t is ctypes.c_float else str(int(v)))
                elif isinstance(v, ctypes.Array):                               # a host table of device pointers
                    out.append("[" + " ".join(label(p) for p in v) + "]")
                else:
                    out.append(label(v))
            where = ""
            if has_stream:
                where = " @main" if torch.cuda.current_stream() == torch.cuda.default_stream() else " @side"
            self.lines.append("%s(%s)%s" % (name, ", ".join(out), where))
            return fn(*args)
        return call


def batch(B, P, R, seed):
    rng = np.random.default_rng(seed)
    lr = lambda lo, hi: rng.uniform(lo, hi, size=(B, P, P, P, 1)).astype(np.float32)
    hr = lambda: rng.uniform(-0.45, 0.45, size=(B, P * R, P * R, P * R, 1)).astype(np.float32)
    low = [lr(-1, 1), lr(-1, 1), lr(-1, 1), lr(0, 0.016), lr(0, 0.016), lr(0, 0.016)]
    return tuple(low + [hr(), hr(), hr(), np.full((B,), 1.5, np.float32), (rng.uniform(size=(B, P * R, P * R, P * R)) < 0.12).astype(np.float32)])


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


@contextlib.contextmanager
def recording():
    rec = Recorder(_lib.load())
    real_load, _lib.load = _lib.load, lambda: rec
    try:
        yield rec
    finally:
        _lib.load = real_load


def run_case(dtype, P, R, attr, conv_algo):
    with recording() as rec:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        tc = trainer.TrainerController(P, R, initial_learning_rate=1e-3, quicksave_enable=False, low_resblock=1, hi_resblock=1, seed=7,
                                       dtype=dtype, conv_algo=conv_algo)
        if attr:
            assert getattr(tc.model, attr) is True, attr
            setattr(tc.model, attr, False)
        data = batch(2, P, R, seed=11)
        pred = sha(tc.model.forward(tc._unpack(data)[0]))
        tc.train_step(data)
        flat_g = sha(tc.model.flat_g)
        tc.train_step(data)
        flat_w = sha(tc.model.flat_w)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
    del tc
    gc.collect()
    return rec.lines, pred, flat_g, flat_w, peak


STEP_P, STEP_R = 8, 2


def step_controller(**kw):
    return trainer.TrainerController(STEP_P, STEP_R, initial_learning_rate=1e-3, quicksave_enable=False, low_resblock=1, hi_resblock=1,
                                     seed=7, dtype="float32", **kw)


@functools.lru_cache(None)
def probe(trainable):
    """(gradient norm, largest |gradient|) of the first step on the cases' first batch, from a step that logs the norm and never clips."""
    tc = step_controller(trainable=trainable, global_clipnorm=1e30)
    tc.train_step(batch(2, STEP_P, STEP_R, seed=11))
    return float(tc.last_grad_norm), float(tc.model.flat_g.abs().max())


@contextlib.contextmanager
def recorded_collectives(rec, tc):
    """A world of two ranks as far as the trainer can tell: the collectives and the model's joins become lines of the trace."""
    where = lambda: "@main" if torch.cuda.current_stream() == torch.cuda.default_stream() else "@side"

    def start(t):
        acc = tc.accum_g_ext
        inside = lambda b: b is not None and b.data_ptr() <= t.data_ptr() < b.data_ptr() + 4 * b.numel()
        name, base = ("acc", acc) if inside(acc) else ("g", tc.model.flat_g_ext)
        assert inside(base), "a collective on neither gradient buffer"
        rec.lines.append("allreduce_start(%s, %d, %d) %s" % (name, (t.data_ptr() - base.data_ptr()) // 4, t.numel(), where()))

    def join():
        rec.lines.append("join(busy=%s) %s" % (tc.model._side_busy, where()))
        real_join()
    real_join = tc.model._join_side
    saved = parallel.world_size, parallel.allreduce_sum_start, parallel.allreduce_wait
    parallel.world_size, parallel.allreduce_sum_start, parallel.allreduce_wait = (lambda: 2), start, lambda h: rec.lines.append("allreduce_wait")
    tc.model._join_side = join
    try:
        yield
    finally:
        parallel.world_size, parallel.allreduce_sum_start, parallel.allreduce_wait = saved
        del tc.model._join_side


def step_cases():
    """(name, TrainerController keywords, data parallel?, calls): a call is a batch size (train_step on that many rows) or "apply"."""
    group = [2, 2, 2, "apply", "apply"]
    clipnorm = lambda trainable: {"global_clipnorm": 0.25 * probe(trainable)[0]}
    cases = [("accum2", lambda: dict(accum_steps=2), False, group),
             ("heads", lambda: dict(trainable="heads"), False, [2, 2]),
             ("clipnorm", lambda: clipnorm(None), False, [2, 2]),
             ("clipvalue", lambda: dict(clipvalue=0.25 * probe(None)[1]), False, [2, 2]),
             ("accum2_heads_clipnorm", lambda: dict(accum_steps=2, trainable="heads", **clipnorm("heads")), False, group)]
    for bucketed in (True, False):
        for K, tag, calls in ((1, "", [2, 2]), (1, "_empty", [2, 0]), (2, "", [2, 2, 2, "apply"]), (2, "_first_empty", [0, 2]),
                              (2, "_closing_empty", [2, 0]), (2, "_all_empty", [0, 0])):
            kw = dict(accum_steps=K, bucketed_allreduce=bucketed)
            cases.append(("dp_%s_k%d%s" % ("bucketed" if bucketed else "whole", K, tag), lambda kw=kw: kw, True, calls))
    return cases


def run_step_case(make_kw, dp, calls):
    kw = make_kw()                                              # (a probe step, where the case needs one, stays outside the trace)
    gc.collect()
    with recording() as rec:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        tc = step_controller(**kw)
        with recorded_collectives(rec, tc) if dp else contextlib.nullcontext():
            for i, c in enumerate(calls):
                if c == "apply":
                    rec.lines.append("apply_accumulated() -> %s" % tc.apply_accumulated())
                else:
                    tc.train_step(batch(c, STEP_P, STEP_R, seed=11 + i))
        buf = tc.accum_g_ext if tc.accum_g_ext is not None else tc.model.flat_g_ext
        out = [sha(t) for t in (tc.model.flat_w, tc.optimizer.m, tc.optimizer.v, buf)] + [tc.optimizer.iterations]
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
    del tc, buf
    gc.collect()
    return rec.lines, out, peak


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dump", help="write every case's trace to DIR/<case>.txt")
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    args = ap.parse_args()
    for v in ("FDN_SIGN_MASK", "FDN_BF16_SIGN_MASK", "FDN_MULTI_DGRAD", "FDN_BATCH_WGRAD", "FDN_OVERLAP_WGRAD", "FDN_CONV_ALGO"):
        os.environ.pop(v, None)                                 # the defaults are the baseline of the matrix

    def trace_hash(case, lines):
        text = "\n".join(lines) + "\n"
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, case + ".txt"), "w") as f:
                f.write(text)
        return hashlib.sha256(text.encode()).hexdigest()[:16]
    first_head = network.layer_specs(1, 1)[-6][0]
    settings = [("default", None, None)] + [("no_" + a, a, None) for a in ("sign_masks", "multi_dgrad", "batch_wgrad", "overlap_wgrad")]
    settings += [("direct", None, "direct"), ("winograd_w", None, "winograd_w"), ("head_direct", None, {first_head: "direct"})]
    print("%-34s %-16s %-16s %-16s %-16s %s" % ("case", "trace", "prediction", "flat_g step 1", "flat_w step 2", "max_memory_allocated"))
    for dtype in ("float32", "bfloat16"):
        for P, R in ((8, 2), (6, 2), (5, 1)):
            for name, attr, algo in settings:
                case = "%s_P%dR%d_%s" % (dtype, P, R, name)
                if args.only not in case:
                    continue
                lines, pred, flat_g, flat_w, peak = run_case(dtype, P, R, attr, algo)
                print("%-34s %s %s %s %s %d  (%d calls)" % (case, trace_hash(case, lines), pred[:16], flat_g[:16], flat_w[:16], peak,
                                                            len(lines)), flush=True)
    print("%-34s %-16s %-16s %-16s %-16s %-16s %-10s %s" % ("case", "trace", "flat_w", "optimizer.m", "optimizer.v", "step buffer", "iterations",
                                                           "max_memory_allocated"))
    for name, make_kw, dp, calls in step_cases():
        case = "step_" + name
        if args.only not in case:
            continue
        lines, (w, m, v, buf, iterations), peak = run_step_case(make_kw, dp, calls)
        print("%-34s %s %s %s %s %s %-10d %d  (%d lines)" % (case, trace_hash(case, lines), w[:16], m[:16], v[:16], buf[:16], iterations, peak,
                                                            len(lines)), flush=True)


if __name__ == "__main__":
    main()

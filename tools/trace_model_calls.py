"""Which library calls does a train step make?  Wraps what _lib.load() returns in a recording proxy and prints one line per call of
lib4dflow_hip.so: the entry point, every integer / float argument, for the pointer arguments NULL or a letter (equal letters = equal
pointers within that call; no addresses) and the stream, main or side.  Per case: sha256 of that trace, of an inference prediction, of
flat_g after train step 1 and of flat_w after train step 2, and torch.cuda.max_memory_allocated().  Two checkouts that print the same
table issue the same launches with the same arguments in the same order and compute the same bits: what a refactor of ops.py /
ops_bf16.py / network.py has to show.

    python tools/trace_model_calls.py [--dump DIR] [--only SUBSTRING]

Cases: LB = HB = 1, B = 2, both dtypes, P=8 R=2 (8^3 / 16^3: sign masks, batched weight gradients and the multi-source head dgrad all
apply), P=6 R=2 (6^3 falls off the Winograd kernels, 12^3 does not), P=5 R=1 (odd extents: chained heads, no batch); the defaults, each of
sign_masks / multi_dgrad / batch_wgrad / overlap_wgrad switched off on its own, conv_algo "direct", "winograd_w" and {first head: "direct"}."""
import argparse
import ctypes
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


def run_case(dtype, P, R, attr, conv_algo):
    rec = Recorder(_lib.load())
    real_load, _lib.load = _lib.load, lambda: rec
    try:
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
    finally:
        _lib.load = real_load
    del tc
    gc.collect()
    return rec.lines, pred, flat_g, flat_w, peak


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dump", help="write every case's trace to DIR/<case>.txt")
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    args = ap.parse_args()
    for v in ("FDN_SIGN_MASK", "FDN_BF16_SIGN_MASK", "FDN_MULTI_DGRAD", "FDN_BATCH_WGRAD", "FDN_OVERLAP_WGRAD", "FDN_CONV_ALGO"):
        os.environ.pop(v, None)                                 # the defaults are the baseline of the matrix
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
                text = "\n".join(lines) + "\n"
                if args.dump:
                    os.makedirs(args.dump, exist_ok=True)
                    with open(os.path.join(args.dump, case + ".txt"), "w") as f:
                        f.write(text)
                print("%-34s %s %s %s %s %d  (%d calls)" % (case, hashlib.sha256(text.encode()).hexdigest()[:16], pred[:16], flat_g[:16],
                                                            flat_w[:16], peak, len(lines)), flush=True)


if __name__ == "__main__":
    main()

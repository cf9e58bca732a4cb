"""cfg5: full-volume sliding-window inference throughput (patch 24, res x2, batch 8, 8+4 ResBlocks, fp32).
Times predictor.predict_patches (tiler -> batched HIP forward -> gather) on the shipped example volume (12 patches) and on a
synthetic 100x100x100 volume (125 patches); prints patches/s.  Launch under torch.distributed.run to shard patches over ranks.

--device-tiler [--runs N] (single process): whole-job wall time of predictor.predict_file without the HDF5 write, host tiler and device
tiler (device_tiler=True) alternately, N >= 3 timed runs each after one warm-up of both, on the example volume and on the synthetic 100^3
volume as a four-frame file; prints every run, the median, the spread (min .. max) and patches/s."""
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
parallel = importlib.import_module("4dflownet_amd.parallel")
predictor = importlib.import_module("4dflownet_amd.predictor")
data = importlib.import_module("4dflownet_amd.data")
tiler = importlib.import_module("4dflownet_amd.tiler")


class _Vol:
    pass


def _synthetic_file(path, frames=4, n=100):
    h5io = importlib.import_module("4dflownet_amd.h5io")
    rng = np.random.default_rng(0)
    tree = {"dx": np.full((frames, 3), 1.0, np.float32)}
    for c in ("u", "v", "w"):
        tree[c] = rng.uniform(-1, 1, (frames, n, n, n)).astype(np.float32)
        tree["mag_" + c] = rng.uniform(0, 65, (frames, n, n, n)).astype(np.float32)
        tree["venc_" + c] = np.full(frames, 1.0, np.float32)
    h5io.write_file(path, tree)


def device_tiler_leg(net, dtype, runs):
    """predict_file end to end (load, patchify, forward, stitch, post-processing) with the file append replaced by a no-op."""
    import statistics
    import tempfile
    build = importlib.import_module("4dflownet_amd.build")
    import subprocess
    commit = os.environ.get("FDN_COMMIT")                  # a snapshot of the tree without its history: the caller names the commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        d = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True, text=True)
        commit = r.stdout.strip() + ("+dirty" if d.stdout.strip() else "") if r.returncode == 0 else "unknown"
    print("# commit %s lib_source_stamp %s" % (commit, build.source_stamp()))
    print("# tools/bench_predictor.py --device-tiler --runs %d%s: predict_file wall time without the HDF5 write, patch 24, res x2, batch 8, "
          "8+4 ResBlocks, %s, %s" % (runs, " --bf16" if dtype != "float32" else "", dtype, torch.cuda.get_device_name(0)))
    predictor.h5io = type("NoWrite", (), {"append_datasets": staticmethod(lambda *a, **k: None)})
    with tempfile.TemporaryDirectory() as tmp:
        synth = os.path.join(tmp, "synthetic_4x100.h5")
        _synthetic_file(synth)
        for name, path, patches in (("example_data.h5 (1 x 42x38x36)", os.path.join(ROOT, "tests", "golden", "data", "example_data.h5"), 12),
                                    ("synthetic (4 x 100^3)", synth, 4 * 125)):
            times = {"host": [], "device": []}
            for r in range(runs + 1):                          # run 0 warms both legs up (file decode, pack streams, staging buffers)
                for leg in ("host", "device"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    vols = predictor.predict_file(net, path, os.path.join(tmp, "unused.h5"), 24, 2, batch_size=8, verbose=False,
                                                  device_tiler=(leg == "device"))
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if r:
                        times[leg].append(dt)
                    del vols
            for leg in ("host", "device"):
                t = times[leg]
                med = statistics.median(t)
                print("%-32s %-6s tiler: runs %s s; median %.3f s (min %.3f .. max %.3f) = %.1f patches/s"
                      % (name, leg, " ".join("%.3f" % x for x in t), med, min(t), max(t), patches / med))
            print("%-32s device / host median wall time: %.3f" % (name, statistics.median(times["device"]) / statistics.median(times["host"])))


def main():
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(local)
    dtype = "bfloat16" if "--bf16" in sys.argv else "float32"
    net = predictor.prepare_network(24, 2, 8, 4, dtype=dtype)
    if "--device-tiler" in sys.argv:
        if world != 1:
            raise SystemExit("--device-tiler measures the single-process path")
        runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 3
        device_tiler_leg(net, dtype, max(runs, 3))
        return
    cases = []
    ds = data.ImageDataset()
    ds.load_vectorfield(os.path.join(ROOT, "tests", "golden", "data", "example_data.h5"), 0)
    cases.append(("example_data.h5 (42x38x36)", ds))
    rng = np.random.default_rng(0)
    v = _Vol()
    for n in ("u", "v", "w"):
        setattr(v, n, rng.uniform(-1, 1, (100, 100, 100)).astype(np.float32))
    for n in ("mag_u", "mag_v", "mag_w"):
        setattr(v, n, rng.uniform(0, 0.016, (100, 100, 100)).astype(np.float32))
    cases.append(("synthetic 100^3", v))
    for name, vol in cases:
        pg = tiler.PatchGenerator(24, 2)
        vel, mag = pg.patchify(vol)
        predictor.predict_patches(net, vel, mag, 8)            # warm-up
        torch.cuda.synchronize(); parallel.barrier()
        t0 = time.perf_counter()
        res = predictor.predict_patches(net, vel, mag, 8)
        torch.cuda.synchronize(); parallel.barrier()
        dt = time.perf_counter() - t0
        t1 = time.perf_counter()
        out = pg.unpatchify(res)
        ts = time.perf_counter() - t1
        if rank == 0:
            print("%-28s %4d patches on %d GPU(s), %s: forward+gather %.3f s = %.1f patches/s; stitch %.3f s -> %s"
                  % (name, len(res), world, dtype, dt, len(res) / dt, ts, out[0].shape))


if __name__ == "__main__":
    main()

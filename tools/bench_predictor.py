"""cfg5: full-volume sliding-window inference throughput (patch 24, res x2, batch 8, 8+4 ResBlocks, fp32).
Times predictor.predict_patches (tiler -> batched HIP forward -> gather) on the shipped example volume (12 patches) and on a
synthetic 100x100x100 volume (125 patches); prints patches/s.  Launch under torch.distributed.run to shard patches over ranks.

--device-tiler [--runs N]: whole-job wall time of predictor.predict_file without the HDF5 write, on the example volume and on the synthetic
100^3 volume as a four-frame file; the legs run alternately, N >= 3 timed runs each after one warm-up of all of them; prints every run, the
median, the spread (min .. max) and patches/s.  Single process: host tiler, device tiler with the host finish (FDN_DEVICE_FINISH=0) and
device tiler with the finish inside the stitch launch (the default).  Under torch.distributed.run: the data-parallel host tiler (whole
patches to rank 0, stitched on its host) and the data-parallel device tiler (cores to rank 0, stitched and finished on its device); with
fewer devices than ranks the lines are marked oversubscribed and are no scaling numbers.

--self-ensemble [--runs N] [--plain-only]: the geometric self-ensemble (predict_volume(self_ensemble="rot90")) at the cfg5 shapes, single
process.  Per batch of 8 patches (24^3 -> 48^3), by device events: the forward, and for each of the ten orientations the oriented window
features and the rotate-back-and-accumulate launch, with the two new paths together as a share of the forward.  Then predict_volume on
synthetic 100^3 frames, plain (four frames, 500 patches) and with the ten orientations (one frame, 125 patches), alternately, N >= 3 timed
runs each: every run, median, spread and patches/s.  --plain-only: the plain leg alone (the command of a tools/ab_source.sh comparison).

--blend [--runs N]: overlap-add stitching (predict_volume(blend=)) on the example volume, single process, randomly initialised weights.
For blend 0, 2 and 4: patches per volume and the wall time of one finished volume, alternately, N >= 3 timed runs each; the stitch launches
of one volume alone by device events (blend_patches + finish_volume against stitch_patches(frame_scale=)); and the seam figure for blend 0
against 4 -- the mean absolute step across the planes where two cores of the plain tiling meet over that across all other planes, per axis."""
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


# (label, device_tiler, FDN_DEVICE_FINISH or None = leave unset)
LEGS_SINGLE = (("host", False, None), ("device, host finish", True, "0"), ("device, device finish", True, "1"))
LEGS_DP = (("dp host", False, None), ("dp device", True, "1"))


def _stamp_line():
    """The first line of a profile: the commit (FDN_COMMIT where the tree is a snapshot without its history) and the library source stamp."""
    import subprocess
    build = importlib.import_module("4dflownet_amd.build")
    commit = os.environ.get("FDN_COMMIT")                  # a snapshot of the tree without its history: the caller names the commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        d = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True, text=True)
        commit = r.stdout.strip() + ("+dirty" if d.stdout.strip() else "") if r.returncode == 0 else "unknown"
    return "# commit %s lib_source_stamp %s" % (commit, build.source_stamp())


def _event_us(fn, reps=50, warm=5):
    """Mean device time of fn() in microseconds: `reps` calls between two events on the current stream, after `warm` calls."""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def self_ensemble_leg(net, dtype, runs, plain_only=False):
    """The cost of predict_volume(self_ensemble="rot90") at the cfg5 shapes; see the module docstring."""
    import statistics
    P, R, B = 24, 2, 8
    print(_stamp_line())
    print("# tools/bench_predictor.py --self-ensemble --runs %d%s%s: patch 24, res x2, batch 8, 8+4 ResBlocks, %s, %s"
          % (runs, " --plain-only" if plain_only else "", " --bf16" if dtype != "float32" else "", dtype, torch.cuda.get_device_name(0)))
    rng = np.random.default_rng(0)
    frames = np.concatenate([rng.uniform(-1, 1, (4, 3, 100, 100, 100)), rng.uniform(0, 0.016, (4, 3, 100, 100, 100))], axis=1).astype(np.float32)
    dframes = torch.from_numpy(frames).cuda()
    counts, _, extents = tiler.PatchGenerator(P, R).plan((100, 100, 100))
    per_frame = counts[0] * counts[1] * counts[2]
    orientations = net.ops.self_ensemble_orientations("rot90")
    if not plain_only:
        g0 = per_frame // 2 - B // 2                           # a batch from the middle of the volume
        phase, pc = net.ops.input_features_volume(dframes, P, counts, g0, B)
        pred = net.forward_features(phase, pc).clone()
        acc = torch.empty_like(pred)
        fwd = _event_us(lambda: net.forward_features(phase, pc), reps=20)
        print("per batch of %d patches: forward %.1f us" % (B, fwd))
        feat, unrot = {}, {}
        for o in orientations:
            feat[o] = _event_us(lambda: net.ops.input_features_volume(dframes, P, counts, g0, B, phase=phase, pc=pc, orientation=o))
            unrot[o] = _event_us(lambda: net.ops.unrotate_accumulate(pred, acc, o, False, 10 if o == orientations[-1] else 1))
            print("  orientation (%d,%d): oriented features %6.1f us, rotate back + accumulate %6.1f us, together %.2f %% of the forward"
                  % (o[0], o[1], feat[o], unrot[o], 100.0 * (feat[o] + unrot[o]) / fwd))
        new = sum(feat[o] + unrot[o] for o in orientations)
        print("ten orientations: the two new paths %.1f us against ten forwards %.1f us = %.2f %%; the plain features alone %.1f us"
              % (new, 10 * fwd, 100.0 * new / (10 * fwd), feat[(0, 0)]))
    legs = [("plain", None, 4)] + ([] if plain_only else [("rot90", "rot90", 1)])
    outs = {nf: torch.empty((nf, 3) + extents, device="cuda") for _, _, nf in legs}
    times = dict((leg[0], []) for leg in legs)
    for r in range(runs + 1):                                  # run 0 warms both legs up
        for leg, option, nf in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            predictor.predict_volume(net, dframes[:nf], P, B, out=outs[nf], self_ensemble=option)
            torch.cuda.synchronize()
            if r:
                times[leg].append(time.perf_counter() - t0)
    rate = {}
    for leg, option, nf in legs:
        t = times[leg]
        med = statistics.median(t)
        rate[leg] = nf * per_frame / med
        print("predict_volume %-5s (%d x 100^3, %d patches%s): runs %s s; median %.3f s (min %.3f .. max %.3f) = %.1f patches/s"
              % (leg, nf, nf * per_frame, "" if option is None else " x %d orientations" % len(orientations),
                 " ".join("%.3f" % x for x in t), med, min(t), max(t), rate[leg]))
    if not plain_only:
        print("rot90 / plain patches/s: %.4f (1/K = %.4f)" % (rate["rot90"] / rate["plain"], 1.0 / len(orientations)))


def blend_leg(net, dtype, runs, blends=(0, 2, 4)):
    """The cost and the effect of predict_volume(blend=) on the example volume at the cfg5 shapes; see the module docstring."""
    import statistics
    P, R, B = 24, 2, 8
    print(_stamp_line())
    print("# tools/bench_predictor.py --blend --runs %d%s: example_data.h5 row 0, patch 24, res x2, batch 8, 8+4 ResBlocks, %s, randomly "
          "initialised weights, %s" % (runs, " --bf16" if dtype != "float32" else "", dtype, torch.cuda.get_device_name(0)))
    ds = data.ImageDataset()
    ds.load_vectorfield(os.path.join(ROOT, "tests", "golden", "data", "example_data.h5"), 0)
    frames = np.stack([ds.u, ds.v, ds.w, ds.mag_u, ds.mag_v, ds.mag_w])[None].astype(np.float32)
    dframes = torch.from_numpy(frames).cuda()
    scale = predictor._frame_scale_tensor([(ds.venc, ds.velocity_per_px)], 1, dframes.device)
    E = P - 4
    plans = {b: tiler.PatchGenerator(P, R, blend=b) for b in blends}
    times = {b: [] for b in blends}
    for r in range(runs + 1):                                  # run 0 warms every leg up
        for b in blends:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            predictor.predict_volume(net, dframes, P, B, frame_scale=scale, blend=b)
            torch.cuda.synchronize()
            if r:
                times[b].append(time.perf_counter() - t0)
    base = statistics.median(times[blends[0]])
    for b in blends:
        counts, _, extents = plans[b].plan(frames.shape[2:])
        n = counts[0] * counts[1] * counts[2]
        t = times[b]
        med = statistics.median(t)
        print("predict_volume blend=%d: %s = %3d patches per volume ((E/(E-b))^3 = %.2f); runs %s s; median %.3f s per volume (min %.3f .. "
              "max %.3f) = %.2f x blend=%d" % (b, "x".join(str(c) for c in counts), n, (E / (E - b)) ** 3, " ".join("%.3f" % x for x in t),
                                               med, min(t), max(t), med / base, blends[0]))
    # the stitch launches of one volume alone, by device events, on one batch of random predictions
    pred = torch.from_numpy(np.random.default_rng(0).standard_normal((B, P * R, P * R, P * R, 3)).astype(np.float32)).cuda()
    for b in blends:
        counts, _, extents = plans[b].plan(frames.shape[2:])
        n = counts[0] * counts[1] * counts[2]
        out64 = torch.empty((1, 3) + extents, device="cuda", dtype=torch.float64)
        if b == 0:
            def launches():
                for g0 in range(0, n, B):
                    net.ops.stitch_patches(pred[:min(B, n - g0)], out64, 2 * R, counts, g0, frame_scale=scale)
            what = "stitch_patches(frame_scale=)"
        else:
            acc = torch.zeros((1, 3) + extents, device="cuda")

            def launches():
                for g0 in range(0, n, B):
                    net.ops.blend_patches(pred[:min(B, n - g0)], acc, 2 * R, plans[b].stride * R, counts, g0)
                net.ops.finish_volume(acc, scale, out=out64)
            what = "blend_patches + one finish_volume"
        us = _event_us(launches, reps=20)
        print("blend=%d: the %d %s launches of one volume: %.1f us = %.2f %% of its wall time"
              % (b, (n + B - 1) // B, what, us, 100.0 * us * 1e-6 / statistics.median(times[b])))
    # the seam figure: mean |step| of the normalised prediction across the planes where two cores of the plain tiling (blend=0) meet, over the
    # mean |step| across all other planes, per axis -- 1.0 means the core boundaries cannot be told from the rest of the volume
    C = E * R
    for b in (blends[0], blends[-1]):
        vol = predictor.predict_volume(net, dframes, P, B, blend=b)[0].double()
        figs = []
        for ax in range(3):
            step = vol.diff(dim=ax + 1).abs().mean(dim=[d for d in range(4) if d != ax + 1])      # step[x]: between planes x and x + 1
            seam = torch.zeros_like(step, dtype=torch.bool)
            seam[C - 1::C] = True
            figs.append("%s %.4f (%d of %d planes)" % ("xyz"[ax], float(step[seam].mean() / step[~seam].mean()), int(seam.sum()), step.numel()))
        print("seam figure blend=%d: %s" % (b, ", ".join(figs)))


def device_tiler_leg(net, dtype, runs, rank=0, world=1):
    """predict_file end to end (load, patchify, forward, stitch, post-processing) with the file append replaced by a no-op."""
    import statistics
    import tempfile
    say = print if rank == 0 else (lambda *a, **k: None)
    say(_stamp_line())
    say("# tools/bench_predictor.py --device-tiler --runs %d%s: predict_file wall time without the HDF5 write, patch 24, res x2, batch 8, "
        "8+4 ResBlocks, %s, %s" % (runs, " --bf16" if dtype != "float32" else "", dtype, torch.cuda.get_device_name(0)))
    legs = LEGS_SINGLE
    if world > 1:
        legs = LEGS_DP
        ndev = torch.cuda.device_count()
        say("# %d ranks on %d device(s), backend %s%s" % (world, min(ndev, world), torch.distributed.get_backend(),
                                                          "" if ndev >= world else ": OVERSUBSCRIBED, no speed claim"))
    predictor.h5io = type("NoWrite", (), {"append_datasets": staticmethod(lambda *a, **k: None)})
    with tempfile.TemporaryDirectory() as tmp:
        synth = os.path.join(tmp, "synthetic_4x100.h5")
        if world > 1:                                          # one file for all ranks: rank 0 writes it where the others find it
            synth = os.path.join(tempfile.gettempdir(), "fdn_bench_synthetic_4x100_%s.h5" % os.environ.get("MASTER_PORT", "0"))
        if rank == 0:
            _synthetic_file(synth)
        parallel.barrier()
        for name, path, patches in (("example_data.h5 (1 x 42x38x36)", os.path.join(ROOT, "tests", "golden", "data", "example_data.h5"), 12),
                                    ("synthetic (4 x 100^3)", synth, 4 * 125)):
            times = dict((leg[0], []) for leg in legs)
            for r in range(runs + 1):                          # run 0 warms every leg up (file decode, pack streams, staging buffers)
                for leg, device, fin in legs:
                    if fin is None:
                        os.environ.pop("FDN_DEVICE_FINISH", None)
                    else:
                        os.environ["FDN_DEVICE_FINISH"] = fin
                    torch.cuda.synchronize(); parallel.barrier()
                    t0 = time.perf_counter()
                    vols = predictor.predict_file(net, path, os.path.join(tmp, "unused.h5"), 24, 2, batch_size=8, verbose=False,
                                                  device_tiler=device)
                    torch.cuda.synchronize(); parallel.barrier()
                    dt = time.perf_counter() - t0
                    if r:
                        times[leg].append(dt)
                    del vols
            os.environ.pop("FDN_DEVICE_FINISH", None)
            for leg, _, _ in legs:
                t = times[leg]
                med = statistics.median(t)
                say("%-32s %-22s tiler: runs %s s; median %.3f s (min %.3f .. max %.3f) = %.1f patches/s"
                    % (name, leg, " ".join("%.3f" % x for x in t), med, min(t), max(t), patches / med))
            base = statistics.median(times[legs[0][0]])
            for leg, _, _ in legs[1:]:
                say("%-32s %s / %s median wall time: %.3f" % (name, leg, legs[0][0], statistics.median(times[leg]) / base))
        parallel.barrier()
        if world > 1 and rank == 0:
            os.remove(synth)


def main():
    ndev = max(torch.cuda.device_count(), 1)
    # more ranks than devices (a self-test on one GPU): gloo, RCCL refuses two ranks on one device
    rank, world, local = parallel.init_from_env(backend="gloo" if int(os.environ.get("WORLD_SIZE", "1")) > ndev else None)
    torch.cuda.set_device(local % ndev)
    dtype = "bfloat16" if "--bf16" in sys.argv else "float32"
    net = predictor.prepare_network(24, 2, 8, 4, dtype=dtype)
    if "--self-ensemble" in sys.argv:
        if world > 1:
            raise SystemExit("--self-ensemble is a single-process measurement")
        runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 3
        self_ensemble_leg(net, dtype, max(runs, 3), plain_only="--plain-only" in sys.argv)
        return
    if "--blend" in sys.argv:
        if world > 1:
            raise SystemExit("--blend is a single-process measurement")
        runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 3
        blend_leg(net, dtype, max(runs, 3))
        return
    if "--device-tiler" in sys.argv:
        runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 3
        device_tiler_leg(net, dtype, max(runs, 3), rank, world)
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

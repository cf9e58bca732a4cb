"""Cost and accuracy of the low-res synthesis on the device (fdn_kspace_downsample).
python tools/bench_kspace.py [--commit SHA] [--reps 5] [--calls 50] [--out profiles/kspace.txt]
One frame of tests/golden/data/example_data_HR.h5 -- u, v, w (84,76,72) -> (42,38,36), mask x 120 -- through
  numpy (fft_downsampling.downsample_phase_img, three calls), torch.fft in complex128 (downsample_phase_img_gpu, three calls) and the HIP
  path (downsample_phase_img_device, one call): host arrays in, host arrays out, wall clock, best of --reps after one warm-up;
  the HIP kernels alone on resident volumes with Philox noise (ops.kspace_downsample): HIP events, median of --calls calls;
  one DevicePatchHandler3D.resynthesize_lowres of the example file: wall clock with a device synchronisation, best of --reps.
Then, per shape of tests/test_gpu_kspace.py, the device's error E in the complex plane against float64, the error E_c64 of the same
statements in complex64, and the relative error of sigma."""
import argparse
import importlib
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ops = importlib.import_module("4dflownet_amd.ops")
build = importlib.import_module("4dflownet_amd.build")
fft = importlib.import_module("4dflownet_amd.fft_downsampling")
h5io = importlib.import_module("4dflownet_amd.h5io")
ddev = importlib.import_module("4dflownet_amd.data_device")
HR_FILE = os.path.join(ROOT, "tests", "golden", "data", "example_data_HR.h5")


def commit():
    try:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        if r.returncode == 0:
            d = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True, text=True)
            return r.stdout.strip() + ("+dirty" if d.stdout.strip() else "")
    except OSError:
        pass
    return "unknown"


def best_wall(fn, reps):
    fn()
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def median_events(fn, calls, warmup=10):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main(a, say):
    hr = h5io.read_all(HR_FILE)
    vel = np.stack([hr[c][0] for c in "uvw"])
    mag = hr["mask"][0] * 120
    vencs, snr = (1.5, 1.0, 1.5), 15.0
    np.random.seed(0)
    say("one frame, u v w (84,76,72) -> (42,38,36), host arrays in and out:")
    say("  numpy, three calls of downsample_phase_img:            %8.2f ms" % best_wall(
        lambda: [fft.downsample_phase_img(vel[c], mag, vencs[c], 0.5, snr) for c in range(3)], a.reps))
    say("  torch.fft complex128, three calls of .._img_gpu:       %8.2f ms" % best_wall(
        lambda: [fft.downsample_phase_img_gpu(vel[c], mag, vencs[c], 0.5, snr) for c in range(3)], a.reps))
    say("  HIP, one call of downsample_phase_img_device (host noise): %4.2f ms" % best_wall(
        lambda: fft.downsample_phase_img_device(vel, mag, vencs, 0.5, snr), a.reps))
    dvel, dmag = torch.from_numpy(vel).cuda(), torch.from_numpy(hr["mask"][0]).cuda()
    crops = ops.kspace_crops(dmag.shape, 0.5)
    out = tuple(torch.empty((3, 42, 38, 36), device="cuda") for _ in range(2))
    ws = torch.empty((ops.kspace_workspace_bytes(3, dmag.shape, crops) + 3) // 4, device="cuda")
    say("  HIP kernels alone, resident volumes, Philox noise (six stage launches + three sums + the 48-byte table): %.4f ms  [median of %d calls]"
        % (median_events(lambda: ops.kspace_downsample(dvel, dmag, vencs, snr, crops, seed=1, stream_id=2, mag_scale=120.0, out=out, workspace=ws),
                         a.calls), a.calls))
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(HR_FILE, os.path.join(d, "hr.h5"))
        h = ddev.DevicePatchHandler3D(d, 12, 2, 4, resynthesize=dict(seed=1))
        index = np.array([["lr.h5", "hr.h5", "0", "0", "0", "0", "0", "0", "0", "0.7"]])
        epoch = iter(range(1 << 30))
        say("one resynthesize_lowres of the example file (1 frame; draws, staging copies, the call, six installs): %.3f ms"
            % best_wall(lambda: h.resynthesize_lowres(next(epoch), index), a.reps))
    T = importlib.import_module("test_gpu_kspace")
    say("accuracy per shape of tests/test_gpu_kspace.py (per volume; bound: E_dev <= 8 E_c64):")
    for case in T.CASES:
        _, refs, e_c64 = T._reference(case, "supplied")
        got = T._device(case)
        e_dev, _ = T._errors(case, got, refs)
        sig = [abs(float(got[2][v]) / float(r["sigma"]) - 1) for v, r in enumerate(refs)]
        say("  %-8s %-12s E_dev %s  E_c64 %s  sigma rel err %s" % (case, "x".join(str(n) for n in T._operands(case)[1].shape), " ".join("%.2e" % e for e in e_dev),
                                                               " ".join("%.2e" % e for e in e_c64), " ".join("%.1e" % s for s in sig)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kspace.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# commit %s lib_source_stamp %s" % (a.commit or commit(), build.source_stamp()))
    say("# %s, tools/bench_kspace.py --reps %d --calls %d" % (torch.cuda.get_device_name(0), a.reps, a.calls))
    main(a, say)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")

"""sha256 of what the predictor's public functions return and write, one `name digest` line per result: the evidence that a change to
4dflownet_amd/predictor.py leaves every output byte alone.  It uses the public names only, so the same script runs on two versions of that
file (bash tools/ab_source.sh 4dflownet_amd/predictor.py <the other version> 'python tools/predictor_digest.py'): every line must agree.

Setup: the seeded network of prepare_network(12, 2, 2, 1) and a three-row file of LR shape (12,20,5) with three vencs (6 patches per row),
beside it a high-resolution file with a one-row mask.  Single process: predict_patches at batch 4 on the three rows' stacks concatenated;
predict_file with the host tiler; with the device tiler at frames_per_group 1 and 3 under FDN_DEVICE_FINISH 1 and 0; with blend=2; with
self_ensemble=[(0,0),(1,1)] -- the returned volumes and the file's bytes each --; predict_volume(patch_range=) in two parts into one `out`;
predict_cores of the second part; the sums of evaluate_file(return_sums=True).
Under torch.distributed.run --nproc_per_node 2 (gloo; both ranks share a device where there is one): rank 0's predict_patches,
predict_file with the host tiler, the device tiler and blend, and evaluate_file."""
import hashlib
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
parallel = importlib.import_module("4dflownet_amd.parallel")
predictor = importlib.import_module("4dflownet_amd.predictor")
data = importlib.import_module("4dflownet_amd.data")
tiler = importlib.import_module("4dflownet_amd.tiler")
h5io = importlib.import_module("4dflownet_amd.h5io")

P, R, B, SHAPE, VENCS = 12, 2, 4, (12, 20, 5), (1.5, 0.9, 2.25)


def _write_files(lr_path, hr_path):
    rng = np.random.default_rng(11)
    rows = len(VENCS)
    tree = {"dx": np.full((rows, 3), 1.5, dtype=np.float32)}
    for n, scale in (("u", 1.0), ("v", 0.5), ("w", 0.75)):
        tree[n] = np.stack([rng.uniform(-v, v, SHAPE) for v in VENCS]).astype(np.float32)
        tree["venc_" + n] = (np.asarray(VENCS) * scale).astype(np.float32)
        tree["mag_" + n] = rng.uniform(0, 300, (rows,) + SHAPE).astype(np.float32)
    h5io.write_file(lr_path, tree)
    hr_shape = tuple(R * s for s in SHAPE)
    hr = {n: np.stack([rng.uniform(-v, v, hr_shape) for v in VENCS]).astype(np.float32) for n in "uvw"}
    hr["mask"] = rng.choice(np.array([0.0, 0.3, 1.0], np.float32), size=(1,) + hr_shape, p=[0.5, 0.1, 0.4])
    h5io.write_file(hr_path, hr)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s %s;" % (a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _file_sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, world, local = parallel.init_from_env(backend="gloo" if world > 1 else None)
    torch.cuda.set_device(local % torch.cuda.device_count())
    say = print if rank == 0 else (lambda *a: None)
    tmp = tempfile.mkdtemp(prefix="predictor_digest_%s_" % os.environ.get("MASTER_PORT", "0")) if rank == 0 else None
    if world > 1:                                                   # one set of files for both ranks
        box = [tmp]
        torch.distributed.broadcast_object_list(box, src=0)
        tmp = box[0]
    lr, hr = os.path.join(tmp, "in.h5"), os.path.join(tmp, "in_HR.h5")
    if rank == 0:
        _write_files(lr, hr)
    parallel.barrier()
    net = predictor.prepare_network(P, R, 2, 1)

    ds, pg = data.ImageDataset(), tiler.PatchGenerator(P, R)
    stacks = []
    for row in range(len(VENCS)):
        ds.load_vectorfield(lr, row)
        vel, mag = pg.patchify(ds)
        stacks.append(list(vel) + list(mag))
    cat = [np.concatenate([s[c] for s in stacks], axis=0) for c in range(6)]
    res = predictor.predict_patches(net, cat[:3], cat[3:], B)
    say("predict_patches", _sha(res) if rank == 0 else None)

    def file_leg(name, env=None, **options):
        out = os.path.join(tmp, name.replace(" ", "_") + ".h5")
        os.environ.pop("FDN_DEVICE_FINISH", None)
        if env is not None:
            os.environ["FDN_DEVICE_FINISH"] = env
        try:
            vols = predictor.predict_file(net, lr, out, P, R, batch_size=B, verbose=False, **options)
        finally:
            os.environ.pop("FDN_DEVICE_FINISH", None)
        parallel.barrier()
        if rank == 0:
            say("predict_file %s volumes" % name, _sha(*[v for row in vols for v in row]))
            say("predict_file %s file" % name, _file_sha(out))

    file_leg("host")
    if world == 1:
        for fpg in (1, 3):
            for fin in ("1", "0"):
                file_leg("device fpg=%d finish=%s" % (fpg, fin), env=fin, device_tiler=True, frames_per_group=fpg)
        file_leg("blend=2", blend=2)
        file_leg("self_ensemble", self_ensemble=[(0, 0), (1, 1)])
        frames = np.empty((len(VENCS), 6) + SHAPE, np.float32)
        for row in range(len(VENCS)):
            ds.load_vectorfield(lr, row)
            frames[row] = np.stack([ds.u, ds.v, ds.w, ds.mag_u, ds.mag_v, ds.mag_w])
        total, cut = 6 * len(VENCS), 7                               # the second part starts inside frame 1
        out = predictor.predict_volume(net, frames, P, B, patch_range=(0, cut))
        predictor.predict_volume(net, frames, P, B, out=out, patch_range=(cut, total))
        say("predict_volume two parts", _sha(out.cpu().numpy()))
        say("predict_cores second part", _sha(predictor.predict_cores(net, frames, P, B, cut, total).cpu().numpy()))
    else:
        file_leg("device", device_tiler=True)
        file_leg("blend=2", blend=2)
    sums = predictor.evaluate_file(net, lr, hr, P, R, batch_size=B, verbose=False, return_sums=True)[1]
    say("evaluate_file sums", _sha(sums) if rank == 0 else None)
    torch.cuda.synchronize()
    parallel.barrier()
    if rank == 0:
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

"""Every launch plan the product code reaches, checked against float64.

The launchers choose tile shapes, kernel variants and launch geometry from N and the grid at run time, so a batch size no parity test
runs (the predictor's tail chunk, a data-parallel shard, the ragged last batch of an epoch) can execute a plan no test has run.  The
test build of the library records every launch (fdn_debug_plan_log / fdn_debug_plan_read, FDN_PLAN in csrc/fdn_common.h): kernel
family, tile / variant, grid against tiles.  Here:

  1. the product paths (TrainerController forward + backward at every N = 1..B of cfg1 / cfg2 / cfg4, fp32 "auto" and "direct" and
     bf16; the inference forward the predictor runs on its chunks, N = 1..B) run once with the recorder on, and every launch becomes a
     plan key: C entry point + the record without N, D, H, W + "one round / several rounds" + "tail partial or full";
  2. PLAN_CASES (below, data) names for every key one case -- the cheapest product shape that reaches it;
  3. each case runs its entry point at that shape, confirms it reaches its key, and compares the result with float64 at sampled voxels
     (fp32: 2e-5 of scale; bf16: one bf16 ulp; weight gradients: 1e-5 of sum |x||dz| on picked rows);
     the two head gradients (fam=head_dgrad, head_wgrad: `walk` = the longest tile walk of a workgroup, 1 / 2 / >= 3) against tests/_head_ref.py;
  4. a product shape that reaches a key with no case fails test_every_product_plan_has_a_case, naming the key and the shapes.

After a planner change, regenerate the table: `python tests/test_gpu_plan_coverage.py` on a GPU prints it."""
import ctypes
import importlib
import os
import sys

if __name__ == "__main__":                             # (run as a script: the repository root and tests/ on the path, as under pytest)
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import pytest
import torch

import _head_ref as HR
from oracle import flownet_oracle as O
from test_gpu_fullsize import gather_rows, ref_dgrad, ref_forward, ref_wgrad_rows, sample_voxels

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("4dflownet_amd._lib")
ops = importlib.import_module("4dflownet_amd.ops")
bops = importlib.import_module("4dflownet_amd.ops_bf16")
trainer = importlib.import_module("4dflownet_amd.trainer")

RTOL = 2e-5
ULP = 2.0 ** -8
PICKS = [(0, 0, 0, 3), (1, 1, 1, 17), (2, 2, 2, 63), (0, 2, 1, 31), (2, 0, 1, 40), (1, 0, 2, 5)]
# (name, patch, res, batch, low_resblock, hi_resblock, dtypes): BASELINE.json configs; cfg2 and cfg3 share a per-rank shape
CONFIGS = [("cfg1", 16, 1, 2, 2, 1, ("float32",)), ("cfg2", 24, 2, 8, 8, 4, ("float32",)), ("cfg4", 32, 4, 4, 8, 4, ("float32", "bfloat16"))]
_SHAPE_FIELDS = ("N", "D", "H", "W", "nvox", "grid", "tiles", "cus", "last")


# ------------------------------------------------------------------------------------------------ recording
def parse_record(line):
    return dict(f.split("=", 1) for f in line.split())


def plan_key(entry, rec):
    """The plan of one launch: entry point + the record minus its shape + rounds over the chip + whether the tail is partial."""
    grid, cus = int(rec.get("grid", rec.get("tiles", 0))), int(rec["cus"])
    tiles = int(rec.get("tiles", grid))
    if "last" in rec:                                   # persistent head kernel: its last workgroup does `last` of `iters` tiles
        tail = int(rec["last"]) < int(rec["iters"])
    elif "splits" in rec:                               # weight gradients: tiles split over `splits` walks
        tail = tiles % int(rec["splits"]) != 0
    elif tiles > grid:                                  # persistent grid walking more blocks than it has workgroups
        tail = tiles % grid != 0
    else:
        tail = grid % cus != 0
    rest = " ".join("%s=%s" % (k, v) for k, v in rec.items() if k not in _SHAPE_FIELDS)
    return "%s %s rounds=%s tail=%s" % (entry, rest, "one" if grid <= cus else "several", "partial" if tail else "full")


class PlanTap:
    """Wrap every C entry point of the test library: after each call the launches it recorded are read back and tagged with the
    entry point's name (and, for the batched weight gradient, its layer count)."""

    def __init__(self, lib):
        self.lib, self.saved, self.records = lib, {}, []

    def read(self):
        n = self.lib.fdn_debug_plan_read(None, 0)
        if n == 0:
            return []
        buf = ctypes.create_string_buffer(n + 1)
        assert self.lib.fdn_debug_plan_read(buf, n + 1) == n
        return [parse_record(l) for l in buf.value.decode().splitlines() if l.strip()]

    def __enter__(self):
        for name in _lib.SIGNATURES:
            orig = getattr(self.lib, name)
            self.saved[name] = orig

            def call(*args, _f=orig, _n=name):
                rc = _f(*args)
                for rec in self.read():
                    if _n.startswith("fdn_conv3d_wgrad") and _n.endswith("_batch"):
                        rec["nl"] = str(args[4])
                    self.records.append((_n, rec))
                return rc
            setattr(self.lib, name, call)
        self.lib.fdn_debug_plan_log(1)
        return self

    def __exit__(self, *exc):
        self.lib.fdn_debug_plan_log(0)
        for name, orig in self.saved.items():
            setattr(self.lib, name, orig)

    def take(self):
        out, self.records = self.records, []
        return out


def _shape_of(rec):
    if "nvox" in rec:                                   # (the 1x1x1 conv: a flat voxel count; the layer grid is a cube)
        n = int(rec["nvox"]) // int(rec["Nctx"])
        p = round(n ** (1.0 / 3.0))
        return int(rec["Nctx"]), p, p, p
    return int(rec["N"]), int(rec["D"]), int(rec["H"]), int(rec["W"])


def collect_product_plans():
    """{plan key: sorted [(dt, algo, N, D, H, W, nl, context)]} over the product paths (see the module doc)."""
    plans = {}
    with _lib.test_build() as lib, PlanTap(lib) as tap:
        for name, P, R, B, LB, HB, dtypes in CONFIGS:
            for dtype in dtypes:
                tc = trainer.TrainerController(P, R, initial_learning_rate=1e-4, quicksave_enable=False, low_resblock=LB, hi_resblock=HB,
                                               seed=0, dtype=dtype)
                m = tc.model
                algos = ("auto", "direct") if dtype == "float32" else ("auto",)
                for algo in algos:
                    m.set_conv_algo(algo)
                    for N in range(1, B + 1):
                        batch = O.synthetic_batch(N, P, R, seed=N)
                        inputs, hires, venc, mask = tc._unpack(batch)
                        for ctx in ("train", "predict"):
                            tap.take()
                            if ctx == "train":
                                pred = m.forward(inputs, training=True)
                                out, dpred = m.ops.loss_metrics(pred, hires[0], hires[1], hires[2], mask)
                                m.backward(dpred)
                            else:                      # predictor.predict_patches -> network forward on each chunk of <= B patches
                                with torch.no_grad():
                                    m.forward(inputs)
                            torch.cuda.synchronize()
                            for entry, rec in tap.take():
                                rec["Nctx"] = str(N)
                                key = plan_key(entry, {k: v for k, v in rec.items() if k not in ("Nctx", "nl")})
                                shape = (rec["dt"], algo) + _shape_of(rec) + (int(rec.get("nl", 0)), "%s %s N=%d" % (name, ctx, N))
                                plans.setdefault(key, set()).add(shape)
                del tc, m
                torch.cuda.empty_cache()
    return {k: sorted(v) for k, v in plans.items()}


def missing_cases(plans, cases):
    """[(key, shapes)] of the product plans without a case."""
    return [(k, v) for k, v in sorted(plans.items()) if k not in cases]


def derive_cases(plans):
    """For every key the cheapest shape that reaches it (fewest voxels, then fewest layers)."""
    return {k: min(v, key=lambda s: (s[2] * s[3] * s[4] * s[5], s[6], s[1] != "auto"))[:7] for k, v in plans.items()}


# ------------------------------------------------------------------------------------------------ float64 parity of one case
def _leaky(z):
    return np.where(z > 0, z, 0.2 * z)


def _close(got, ref, bf16, name):
    if bf16:
        tol = ULP * np.abs(ref) + 3e-5 * np.abs(ref).max()
        bad = np.abs(got - ref) > tol
        assert not bad.any(), "%s: %d of %d sampled elements off by more than one bf16 ulp (worst %.3e of scale %.3e)" % (
            name, int(bad.sum()), bad.size, float(np.abs(got - ref).max()), float(np.abs(ref).max()))
    else:
        err = float(np.abs(got - ref).max())
        assert err <= RTOL * np.abs(ref).max(), "%s: %.3e of scale %.3e" % (name, err, float(np.abs(ref).max()))


def _wgrad_check(x, dz, dw, name):
    refw = ref_wgrad_rows(x, dz, PICKS)
    cond = ref_wgrad_rows(x.abs(), dz.abs(), PICKS)          # sum |x||dz|: the bound any fp32 summation order obeys
    got = np.asarray([dw[a, b, c, ci].double().cpu().numpy() for (a, b, c, ci) in PICKS])
    assert (np.abs(got - refw) <= 1e-5 * cond + 1e-30).all(), "%s: %.3e of bound" % (
        name, float((np.abs(got - refw) / np.maximum(cond, 1e-300)).max()))


def sign_mask_words(y, planar):
    """The sign mask of an (N,D,H,W,64) activation as the forward kernels write it: bit c % 16 of int16 word c / 16 = (y[v][c] > 0);
    planar (fp32 storage): [word][voxel], else (bf16 storage): [voxel][word]."""
    N, D, H, W = y.shape[:4]
    bits = (y.float() > 0).view(N * D * H * W, 4, 16).to(torch.int32)
    words = (bits << torch.arange(16, device=y.device, dtype=torch.int32)).sum(dim=2)
    words = torch.where(words >= 32768, words - 65536, words).to(torch.int16)
    return words.t().contiguous() if planar else words.view(N, D, H, W, 4).contiguous()


def run_case(key, case):
    """Run the case's entry point at its shape under the recorder; returns the plan keys it reached.  Asserts float64 parity."""
    dt, algo_name, N, D, H, W, nl = case
    entry, fam = key.split()[0], parse_record(" ".join(key.split()[1:]))["fam"]
    bf = dt == "bf16"
    o = bops if bf else ops
    algo = {"auto": ops.ALGO_AUTO, "direct": ops.ALGO_DIRECT}[algo_name]
    adt = torch.bfloat16 if bf else torch.float32
    g = torch.Generator(device="cuda").manual_seed(N * 1000 + D)
    rng = np.random.default_rng(D * 10 + N)
    dims = (N, D, H, W)
    pts = sample_voxels(N, D, H, W, 40, rng)

    def rnd(*shape, scale=1.0, dtype=adt):
        return (torch.randn(shape, device="cuda", generator=g) * scale).to(dtype)

    def wts(*shape):                                         # bf16 mode: weights the kernels hold exactly (bf16-representable)
        w = rnd(*shape, scale=0.03, dtype=torch.float32)
        return w.to(torch.bfloat16).float() if bf else w

    def act_d(y):
        return np.where(gather_rows(y, pts) > 0, 1.0, 0.2)

    name = "%s @ %s" % (key, case)
    with _lib.test_build() as lib, PlanTap(lib) as tap:
        tap.take()
        if fam == "head_fwd":
            x, w, b = rnd(N, D, H, W, 64), wts(3, 3, 3, 64, 1), wts(1)
            pred = torch.zeros((N, D, H, W, 3), device="cuda")
            o.conv3d_fwd(x, w, b, ops.ACT_NONE, out=pred, ldy=3, y_coff=1, algo=algo)
            ref = ref_forward(x, w.double().cpu().numpy(), pts, dims)[:, 0] + float(b[0])
            _close(gather_rows(pred, pts)[:, 1], ref, False, name)
        elif fam == "head_dgrad":                           # as the product calls it: the (N,V,3) prediction gradient, ReLU, the producer's bias gradient
            y, w, dpred = rnd(N, D, H, W, 64), wts(3, 3, 3, 64, 1), rnd(N, D, H, W, 3, dtype=torch.float32)
            mask = sign_mask_words(y, planar=not bf) if "mask=1" in key else None
            db = torch.full((64,), float("nan"), device="cuda")
            out = o.conv_cout1_dgrad_folded(dpred, w, dims, None if mask is not None else y, ops.ACT_RELU, lddz=3, dz_coff=1, dbias_prev=db, mask=mask)
            A = gather_rows(HR.head_fold(dpred[..., 1], dims), pts)
            _close(gather_rows(out, pts), (A @ w.double().cpu().numpy().reshape(27, 64)) * (gather_rows(y, pts) > 0), bf, name)
            if not bf:                                       # (bf16 storage: the kernel sums the values BEFORE they are rounded to bf16; test_gpu_head_walks.py has the float64 sums)
                o64 = out.double().reshape(-1, 64)
                assert ((db.double() - o64.sum(dim=0)).abs() <= 1e-5 * o64.abs().sum(dim=0) + 1e-30).all(), "%s: producer bias gradient" % name
        elif fam == "head_wgrad":
            x, dpred = rnd(N, D, H, W, 64), rnd(N, D, H, W, 3, dtype=torch.float32)
            dw, db = o.conv3d_wgrad(x, dpred, 3, 64, 1, want_bias=True, lddz=3, dz_coff=1)
            refw, cond = HR.head_wgrad_ref(x, dpred[..., 1]), HR.head_wgrad_bound(x, dpred[..., 1])      # (all 27 x 64 rows: the reference has them anyway)
            assert ((dw.double() - refw).abs() <= 1e-5 * cond + 1e-30).all(), "%s: %.3e of bound" % (
                name, float(((dw.double() - refw).abs() / cond.clamp_min(1e-300)).max()))
            dz64 = dpred[..., 1].double()
            assert abs(float(db[0]) - float(dz64.sum())) <= 1e-5 * float(dz64.abs().sum()), "%s: bias gradient" % name
        elif fam == "cin3_fwd":
            x, w, b = rnd(N, D, H, W, 3), wts(3, 3, 3, 3, 64), wts(64)
            y = o.conv3d_fwd(x, w, b, ops.ACT_RELU, algo=algo)
            ref = np.maximum(ref_forward(x, w.double().cpu().numpy(), pts, dims) + b.double().cpu().numpy(), 0)
            _close(gather_rows(y, pts), ref, bf, name)
        elif fam == "conv1x1_fwd":
            xa, xb, w, b = rnd(N, D, H, W, 64), rnd(N, D, H, W, 64), wts(1, 1, 1, 128, 64), wts(64)
            y = o.conv3d_fwd(xa, w, b, ops.ACT_RELU, x2=xb, algo=algo)
            w64 = w[0, 0, 0].double().cpu().numpy()
            ref = np.maximum(gather_rows(xa, pts) @ w64[:64] + gather_rows(xb, pts) @ w64[64:] + b.double().cpu().numpy(), 0)
            _close(gather_rows(y, pts), ref, bf, name)
        elif fam == "conv1x1_dgrad":
            dz, ya, yb, w = rnd(N, D, H, W, 64), rnd(N, D, H, W, 64), rnd(N, D, H, W, 64), wts(1, 1, 1, 128, 64)
            dxa, dxb = o.conv1x1_dgrad(dz, w, ya, yb)
            w64 = w[0, 0, 0].double().cpu().numpy()
            d = gather_rows(dz, pts)
            _close(gather_rows(dxa, pts), (d @ w64[:64].T) * (gather_rows(ya, pts) > 0), bf, name + " dxa")
            _close(gather_rows(dxb, pts), (d @ w64[64:].T) * (gather_rows(yb, pts) > 0), bf, name + " dxb")
        elif fam in ("upsample_fwd", "upsample_bwd"):
            R = int(parse_record(" ".join(key.split()[1:]))["R"])
            C8 = slice(0, 8)                                 # channels are independent: compare eight of them over the whole grid
            if fam == "upsample_fwd":
                x = rnd(N, D, H, W, 64)
                y = o.upsample_trilinear_fwd(x, R)
                ref = O.upsample_trilinear_fwd(x[..., C8].double().cpu().numpy(), R, f32_coeffs=True)
                got = y[..., C8].double().cpu().numpy()
            else:
                dy, yp = rnd(N, D * R, H * R, W * R, 64), rnd(N, D, H, W, 64)
                dx = o.upsample_trilinear_bwd(dy, R, yp, ops.ACT_RELU)
                ref = O.upsample_trilinear_bwd(dy[..., C8].double().cpu().numpy(), (D, H, W), R, f32_coeffs=True)
                ref = ref * (yp[..., C8].double().cpu().numpy() > 0)
                got = dx[..., C8].double().cpu().numpy()
            _close(got.reshape(-1, 8), ref.reshape(-1, 8), bf, name)
        elif entry.startswith("fdn_conv3d_wgrad"):
            L = nl if entry.endswith("_batch") else 1
            xs = [rnd(N, D, H, W, 64) for _ in range(L)]
            dzs = [rnd(N, D, H, W, 64) for _ in range(L)]
            dws = [torch.empty((3, 3, 3, 64, 64), device="cuda") for _ in range(L)]
            if L == 1:
                o.conv3d_wgrad(xs[0], dzs[0], 3, 64, 64, dw=dws[0], algo=algo)
            else:
                o.conv3d_wgrad_batch(xs, dzs, dws, algo=algo)
            torch.cuda.synchronize()
            for i in range(L):
                _wgrad_check(xs[i], dzs[i], dws[i], "%s layer %d" % (name, i))
        elif "op=fwd" in key:
            x, res, w, b = rnd(N, D, H, W, 64), rnd(N, D, H, W, 64), wts(3, 3, 3, 64, 64), wts(64)
            wf, _ = o.pack_conv64_weights(w)
            if "ymask=1" in key or ("_mask" in entry and "ymask=" not in key):     # (the bf16 ops reach the _mask entries with or without one)
                mask = o.new_sign_mask(x)
                y = o.conv3d_fwd(x, w, b, ops.ACT_LEAKY, 0.2, res, wpack=wf, algo=algo, mask=mask)
            elif entry == "fdn_conv64_fwd_bf16":
                y = bops.conv64_fwd(x, wf, b, ops.ACT_LEAKY, 0.2, res)
            else:
                y = o.conv3d_fwd(x, w, b, ops.ACT_LEAKY, 0.2, res, wpack=wf, algo=algo)
            z = ref_forward(x, w.double().cpu().numpy(), pts, dims) + b.double().cpu().numpy() + gather_rows(res, pts)
            _close(gather_rows(y, pts), _leaky(z), bf, name)
        else:                                                # fused dgrad: plain, with the sign mask, or multi-source
            nsrc = int(parse_record(" ".join(key.split()[1:])).get("nsrc", 1)) if "multi" in entry else 1
            x, skip = rnd(N, D, H, W, 64), rnd(N, D, H, W, 64)
            ws = [wts(3, 3, 3, 64, 64) for _ in range(nsrc)]
            dzs = [rnd(N, D, H, W, 64) for _ in range(nsrc)]
            packs = torch.zeros((nsrc, 2, ops.CONV64_PACK_FLOATS if not bf else 27 * 64 * 64), device="cuda", dtype=adt)
            for i in range(nsrc):
                o.pack_conv64_weights(ws[i], packs[i, 0], packs[i, 1])
            y = rnd(N, D, H, W, 64)                          # y_prev of act' (LeakyReLU)
            mask = None
            if "fmask=1" in key or ("_mask" in entry and "fmask=" not in key):
                mask = o.new_sign_mask(y)                    # the forward writes y and its sign mask together
                y = o.conv3d_fwd(x, ws[0], None, ops.ACT_LEAKY, 0.2, skip, wpack=packs[0, 0], algo=algo, mask=mask)
            pad = torch.empty((N, D + 2, H + 2, W + 2, 64), device="cuda")
            out = torch.empty_like(dzs[0])
            tap.take()
            if "multi" in entry:
                o.conv3d_dgrad_fused_multi(dzs, [packs[i, 1] for i in range(nsrc)], pad, out, y_prev=None if mask is not None else y,
                                           act=ops.ACT_LEAKY, algo=algo, mask=mask)
                o.fold_halo_border([pad], out, None, y, ops.ACT_LEAKY)
                refd = sum(ref_dgrad(dzs[i], ws[i].double().cpu().numpy(), pts, dims) for i in range(nsrc)) * act_d(y)
            else:
                kw = {} if mask is None else {"mask": mask}
                if not bf:
                    kw["algo"] = algo
                o.conv3d_dgrad_fused(dzs[0], packs[0, 1], pad, out, skip=skip, y_prev=y, act=ops.ACT_LEAKY, **kw)
                o.fold_halo_border([pad], out, skip, y, ops.ACT_LEAKY)
                refd = (ref_dgrad(dzs[0], ws[0].double().cpu().numpy(), pts, dims) + gather_rows(skip, pts)) * act_d(y)
            _close(gather_rows(out, pts), refd, bf, name)
        torch.cuda.synchronize()
        reached = {plan_key(e, {k: v for k, v in r.items() if k != "nl"}) for e, r in tap.records + tap.take()}
    return reached


# ------------------------------------------------------------------------------------------------ the committed table
# plan key -> (dt, algo, N, D, H, W, layers of a batched weight gradient): collected from the recorder (`python tests/test_gpu_plan_coverage.py`)
PLAN_CASES = {
    'fdn_conv1x1_dgrad fam=conv1x1_dgrad op=dgrad dt=f32 rounds=one tail=full': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv1x1_dgrad fam=conv1x1_dgrad op=dgrad dt=f32 rounds=several tail=full': ('f32', 'auto', 3, 24, 24, 24, 0),
    'fdn_conv1x1_dgrad fam=conv1x1_dgrad op=dgrad dt=f32 rounds=several tail=partial': ('f32', 'auto', 5, 24, 24, 24, 0),
    'fdn_conv1x1_dgrad_bf16 fam=conv1x1_dgrad op=dgrad dt=bf16 rounds=one tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv1x1_dgrad_bf16 fam=conv1x1_dgrad op=dgrad dt=bf16 rounds=several tail=full': ('bf16', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x1x2 nreg=7 r0=4x4x8 r1=1x10x10 r2=1x10x10 r3=12x1x10 r4=12x1x10 r5=8x16x1 r6=8x16x1 rounds=several tail=partial': ('f32', 'direct', 5, 48, 48, 48, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x1x2 nreg=7 r0=4x4x8 r1=1x10x10 r2=1x10x10 r3=8x1x10 r4=8x1x10 r5=8x12x1 r6=8x12x1 rounds=several tail=partial': ('f32', 'direct', 2, 48, 48, 48, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x1x2 nreg=7 r0=4x4x8 r1=1x10x12 r2=1x10x12 r3=16x1x8 r4=16x1x8 r5=8x16x1 r6=8x16x1 rounds=several tail=partial': ('f32', 'direct', 1, 128, 128, 128, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x1x2 nreg=7 r0=4x4x8 r1=1x5x17 r2=1x5x17 r3=11x1x7 r4=11x1x7 r5=8x8x1 r6=8x8x1 rounds=several tail=partial': ('f32', 'direct', 4, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x1x2 nreg=7 r0=4x4x8 r1=1x5x25 r2=1x5x25 r3=12x1x10 r4=12x1x10 r5=8x16x1 r6=8x16x1 rounds=several tail=partial': ('f32', 'direct', 6, 48, 48, 48, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x1x2 nreg=7 r0=4x4x8 r1=1x7x9 r2=1x7x9 r3=8x1x9 r4=8x1x9 r5=8x8x1 r6=8x8x1 rounds=several tail=partial': ('f32', 'direct', 3, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x1x2 nreg=7 r0=4x4x8 r1=1x9x9 r2=1x9x9 r3=6x1x13 r4=6x1x13 r5=6x12x1 r6=6x12x1 rounds=several tail=partial': ('f32', 'direct', 7, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x1x2 nreg=7 r0=4x4x8 r1=1x9x9 r2=1x9x9 r3=6x1x13 r4=6x1x13 r5=8x8x1 r6=8x8x1 rounds=several tail=partial': ('f32', 'direct', 6, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x3x6 r2=1x3x6 r3=4x1x3 r4=4x1x3 r5=4x4x1 r6=4x4x1 rounds=one tail=partial': ('f32', 'direct', 1, 16, 16, 16, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x3x6 r2=1x3x6 r3=4x1x6 r4=4x1x6 r5=4x4x1 r6=4x4x1 rounds=several tail=partial': ('f32', 'direct', 2, 16, 16, 16, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x3x7 r2=1x3x7 r3=6x1x3 r4=6x1x3 r5=4x4x1 r6=4x4x1 rounds=several tail=partial': ('f32', 'direct', 1, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x4x9 r2=1x4x9 r3=4x1x7 r4=4x1x7 r5=4x6x1 r6=4x6x1 rounds=several tail=partial': ('f32', 'direct', 2, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x4x9 r2=1x4x9 r3=4x1x9 r4=4x1x9 r5=6x6x1 r6=6x6x1 rounds=several tail=partial': ('f32', 'direct', 3, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x5x10 r2=1x5x10 r3=8x1x5 r4=8x1x5 r5=6x6x1 r6=6x6x1 rounds=several tail=partial': ('f32', 'direct', 1, 48, 48, 48, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x5x5 r2=1x5x5 r3=4x1x7 r4=4x1x7 r5=4x8x1 r6=4x8x1 rounds=several tail=partial': ('f32', 'direct', 1, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x6x10 r2=1x6x10 r3=6x1x10 r4=6x1x10 r5=8x8x1 r6=8x8x1 rounds=several tail=partial': ('f32', 'direct', 3, 48, 48, 48, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x7x7 r2=1x7x7 r3=6x1x7 r4=6x1x7 r5=6x6x1 r6=6x6x1 rounds=several tail=partial': ('f32', 'direct', 4, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x7x7 r2=1x7x7 r3=8x1x5 r4=8x1x5 r5=4x8x1 r6=4x8x1 rounds=several tail=partial': ('f32', 'direct', 2, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x7x9 r2=1x7x9 r3=6x1x9 r4=6x1x9 r5=6x8x1 r6=6x8x1 rounds=several tail=partial': ('f32', 'direct', 5, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=direct op=dgrad dt=f32 layout=1x2x2 nreg=7 r0=4x4x4 r1=1x7x9 r2=1x7x9 r3=6x1x9 r4=6x1x9 r5=8x8x1 r6=8x8x1 rounds=several tail=partial': ('f32', 'direct', 8, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=11x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=12x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 3, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=12x1x1 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 5, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=full': ('f32', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=0 nsrc=1 rounds=several tail=full': ('f32', 'auto', 4, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 3, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=4x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=6x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=8x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 2, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=8x1x2 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 4, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=8x1x2 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 8, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=2 tile=16x1x2 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 2, 48, 48, 48, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=2 tile=32x1x1 ymask=0 fmask=0 nsrc=1 rounds=several tail=full': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x10x6 r1=1x10x6 r2=16x1x4 r3=16x1x4 r4=6x10x1w nsrc=1 rounds=several tail=partial': ('f32', 'auto', 1, 48, 48, 48, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x18x2 r1=1x18x2 r2=16x1x4 r3=16x1x4 r4=6x9x1w nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x26x2 r1=1x26x2 r2=24x1x2 r3=24x1x2 r4=7x9x1w nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x26x2 r1=1x26x2 r2=24x1x2 r3=24x1x2 r4=7x9x1w nsrc=1 rounds=several tail=partial': ('f32', 'auto', 2, 24, 24, 24, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x4x16 r1=1x4x16 r2=64x1x1 r3=64x1x1 r4=6x10x1w nsrc=1 rounds=several tail=partial': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x7x8 r1=1x7x8 r2=32x1x2 r3=32x1x2 r4=7x9x1w nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv3d_dgrad_fused fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x7x8 r1=1x7x8 r2=32x1x2 r3=32x1x2 r4=7x9x1w nsrc=1 rounds=several tail=partial': ('f32', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv3d_fwd fam=cin3_fwd op=fwd dt=f32 rounds=one tail=full': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv3d_fwd fam=cin3_fwd op=fwd dt=f32 rounds=several tail=full': ('f32', 'auto', 3, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=cin3_fwd op=fwd dt=f32 rounds=several tail=partial': ('f32', 'auto', 5, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=conv1x1_fwd op=fwd dt=f32 rounds=one tail=full': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv3d_fwd fam=conv1x1_fwd op=fwd dt=f32 rounds=several tail=full': ('f32', 'auto', 3, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=conv1x1_fwd op=fwd dt=f32 rounds=several tail=partial': ('f32', 'auto', 5, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=direct op=fwd dt=f32 layout=1x1x2 nreg=1 r0=4x4x8 rounds=several tail=full': ('f32', 'direct', 3, 32, 32, 32, 0),
    'fdn_conv3d_fwd fam=direct op=fwd dt=f32 layout=1x1x2 nreg=1 r0=4x4x8 rounds=several tail=partial': ('f32', 'direct', 6, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=direct op=fwd dt=f32 layout=1x2x2 nreg=1 r0=4x4x4 rounds=one tail=partial': ('f32', 'direct', 1, 16, 16, 16, 0),
    'fdn_conv3d_fwd fam=direct op=fwd dt=f32 layout=1x2x2 nreg=1 r0=4x4x4 rounds=several tail=full': ('f32', 'direct', 1, 32, 32, 32, 0),
    'fdn_conv3d_fwd fam=direct op=fwd dt=f32 layout=1x2x2 nreg=1 r0=4x4x4 rounds=several tail=partial': ('f32', 'direct', 2, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=18 rounds=several tail=partial': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=3 rounds=one tail=full': ('f32', 'auto', 1, 48, 48, 48, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=3 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=3 rounds=several tail=full': ('f32', 'auto', 2, 48, 48, 48, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=33 rounds=several tail=partial': ('f32', 'auto', 2, 128, 128, 128, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=48 rounds=several tail=full': ('f32', 'auto', 3, 128, 128, 128, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=6 rounds=several tail=full': ('f32', 'auto', 4, 48, 48, 48, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=66 rounds=several tail=partial': ('f32', 'auto', 4, 128, 128, 128, 0),
    'fdn_conv3d_fwd fam=head_fwd op=fwd dt=f32 iters=9 rounds=several tail=full': ('f32', 'auto', 8, 48, 48, 48, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=11x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=12x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 3, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=12x1x1 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 5, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=full': ('f32', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=0 nsrc=1 rounds=several tail=full': ('f32', 'auto', 4, 32, 32, 32, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 3, 32, 32, 32, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=4x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=6x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=8x1x1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 2, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=8x1x2 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 4, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=8x1x2 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 8, 24, 24, 24, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=2 tile=16x1x2 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 2, 48, 48, 48, 0),
    'fdn_conv3d_fwd fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=2 tile=32x1x1 ymask=0 fmask=0 nsrc=1 rounds=several tail=full': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_fwd_bf16 fam=bf16_general op=fwd dt=bf16 mt=4 box=0 taps=020202 tile=2x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=one tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv3d_fwd_bf16 fam=bf16_mode2 op=fwd dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=one tail=full': ('bf16', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv3d_fwd_bf16 fam=bf16_mode2 op=fwd dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=several tail=full': ('bf16', 'auto', 4, 32, 32, 32, 0),
    'fdn_conv3d_fwd_bf16 fam=bf16_mode2 op=fwd dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('bf16', 'auto', 3, 32, 32, 32, 0),
    'fdn_conv3d_fwd_bf16 fam=bf16_mode2 op=fwd dt=bf16 mt=8 box=0 taps=020202 tile=8x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=several tail=full': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_fwd_bf16 fam=cin3_fwd op=fwd dt=bf16 rounds=one tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv3d_fwd_bf16 fam=cin3_fwd op=fwd dt=bf16 rounds=several tail=full': ('bf16', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv3d_fwd_bf16 fam=conv1x1_fwd op=fwd dt=bf16 rounds=one tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv3d_fwd_bf16 fam=conv1x1_fwd op=fwd dt=bf16 rounds=several tail=full': ('bf16', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv3d_fwd_bf16 fam=head_fwd op=fwd dt=bf16 iters=18 rounds=several tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_fwd_bf16 fam=head_fwd op=fwd dt=bf16 iters=33 rounds=several tail=partial': ('bf16', 'auto', 2, 128, 128, 128, 0),
    'fdn_conv3d_fwd_bf16 fam=head_fwd op=fwd dt=bf16 iters=48 rounds=several tail=full': ('bf16', 'auto', 3, 128, 128, 128, 0),
    'fdn_conv3d_fwd_bf16 fam=head_fwd op=fwd dt=bf16 iters=66 rounds=several tail=partial': ('bf16', 'auto', 4, 128, 128, 128, 0),
    'fdn_conv3d_wgrad fam=head_wgrad op=wgrad dt=f32 walk=1 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv3d_wgrad fam=head_wgrad op=wgrad dt=f32 walk=1 rounds=several tail=partial': ('f32', 'auto', 1, 48, 48, 48, 0),
    'fdn_conv3d_wgrad fam=head_wgrad op=wgrad dt=f32 walk=2 rounds=several tail=partial': ('f32', 'auto', 2, 48, 48, 48, 0),
    'fdn_conv3d_wgrad fam=head_wgrad op=wgrad dt=f32 walk=3 rounds=several tail=full': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_wgrad fam=head_wgrad op=wgrad dt=f32 walk=3 rounds=several tail=partial': ('f32', 'auto', 3, 48, 48, 48, 0),
    'fdn_conv3d_wgrad fam=wgrad_direct op=wgrad dt=f32 splits=108 rounds=several tail=full': ('f32', 'direct', 2, 24, 24, 24, 0),
    'fdn_conv3d_wgrad fam=wgrad_direct op=wgrad dt=f32 splits=128 rounds=several tail=full': ('f32', 'direct', 1, 32, 32, 32, 0),
    'fdn_conv3d_wgrad fam=wgrad_direct op=wgrad dt=f32 splits=16 rounds=one tail=full': ('f32', 'direct', 1, 16, 16, 16, 0),
    'fdn_conv3d_wgrad fam=wgrad_direct op=wgrad dt=f32 splits=162 rounds=several tail=full': ('f32', 'direct', 3, 24, 24, 24, 0),
    'fdn_conv3d_wgrad fam=wgrad_direct op=wgrad dt=f32 splits=170 rounds=several tail=partial': ('f32', 'direct', 4, 24, 24, 24, 0),
    'fdn_conv3d_wgrad fam=wgrad_direct op=wgrad dt=f32 splits=32 rounds=one tail=full': ('f32', 'direct', 2, 16, 16, 16, 0),
    'fdn_conv3d_wgrad fam=wgrad_direct op=wgrad dt=f32 splits=54 rounds=one tail=full': ('f32', 'direct', 1, 24, 24, 24, 0),
    'fdn_conv3d_wgrad fam=wgrad_wino op=wgrad dt=f32 dep=1 splits=64 rounds=one tail=full': ('f32', 'auto', 3, 48, 48, 48, 0),
    'fdn_conv3d_wgrad_batch fam=wgrad_wino_batch op=wgrad dt=f32 layers=2 splits=32 rounds=one tail=full': ('f32', 'auto', 2, 16, 16, 16, 2),
    'fdn_conv3d_wgrad_batch fam=wgrad_wino_batch op=wgrad dt=f32 layers=2 splits=32 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 2),
    'fdn_conv3d_wgrad_batch fam=wgrad_wino_batch op=wgrad dt=f32 layers=5 splits=12 rounds=one tail=full': ('f32', 'auto', 1, 16, 16, 16, 5),
    'fdn_conv3d_wgrad_batch fam=wgrad_wino_batch op=wgrad dt=f32 layers=8 splits=8 rounds=one tail=full': ('f32', 'auto', 1, 24, 24, 24, 8),
    'fdn_conv3d_wgrad_batch fam=wgrad_wino_batch op=wgrad dt=f32 layers=9 splits=7 rounds=one tail=full': ('f32', 'auto', 7, 24, 24, 24, 11),
    'fdn_conv3d_wgrad_batch fam=wgrad_wino_batch op=wgrad dt=f32 layers=9 splits=7 rounds=one tail=partial': ('f32', 'auto', 1, 24, 24, 24, 11),
    'fdn_conv3d_wgrad_bf16 fam=head_wgrad op=wgrad dt=bf16 walk=3 rounds=several tail=full': ('bf16', 'auto', 3, 128, 128, 128, 0),
    'fdn_conv3d_wgrad_bf16 fam=head_wgrad op=wgrad dt=bf16 walk=3 rounds=several tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_wgrad_bf16 fam=wgrad_bf16_dma op=wgrad dt=bf16 splits=168 nseg=4 rounds=several tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv3d_wgrad_bf16_batch fam=wgrad_bf16_batch op=wgrad dt=bf16 layers=4 splits=40 nseg=11 rounds=several tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 8),
    'fdn_conv3d_wgrad_bf16_batch fam=wgrad_bf16_batch op=wgrad dt=bf16 layers=4 splits=40 nseg=3 rounds=several tail=partial': ('bf16', 'auto', 4, 32, 32, 32, 8),
    'fdn_conv3d_wgrad_bf16_batch fam=wgrad_bf16_batch op=wgrad dt=bf16 layers=4 splits=40 nseg=4 rounds=several tail=partial': ('bf16', 'auto', 3, 32, 32, 32, 8),
    'fdn_conv3d_wgrad_bf16_batch fam=wgrad_bf16_batch op=wgrad dt=bf16 layers=4 splits=40 nseg=6 rounds=several tail=partial': ('bf16', 'auto', 2, 32, 32, 32, 8),
    'fdn_conv3d_wgrad_bf16_batch fam=wgrad_bf16_batch op=wgrad dt=bf16 layers=7 splits=24 nseg=2 rounds=several tail=full': ('bf16', 'auto', 3, 32, 32, 32, 11),
    'fdn_conv3d_wgrad_bf16_batch fam=wgrad_bf16_batch op=wgrad dt=bf16 layers=7 splits=24 nseg=2 rounds=several tail=partial': ('bf16', 'auto', 4, 32, 32, 32, 11),
    'fdn_conv3d_wgrad_bf16_batch fam=wgrad_bf16_batch op=wgrad dt=bf16 layers=7 splits=24 nseg=4 rounds=several tail=partial': ('bf16', 'auto', 2, 32, 32, 32, 11),
    'fdn_conv3d_wgrad_bf16_batch fam=wgrad_bf16_batch op=wgrad dt=bf16 layers=7 splits=24 nseg=7 rounds=several tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 11),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_fused_launch op=dgrad dt=bf16 mt=4 nreg=1+6 nsrc=1 rounds=several tail=partial': ('bf16', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_fused_launch op=dgrad dt=bf16 mt=8 nreg=1+6 nsrc=1 rounds=several tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=0 taps=020202 tile=2x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=one tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=0 taps=020202 tile=2x8x8 secondary=0 ymask=0 fmask=1 nsrc=1 rounds=one tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=1 taps=022202 tile=4x1x34 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=1 taps=022202 tile=4x1x34 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=2 taps=020002 tile=4x1x34 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=2 taps=020002 tile=4x1x34 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=3 taps=022202 tile=4x1x34 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=3 taps=022202 tile=4x1x34 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=4 taps=020002 tile=4x1x34 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=4 taps=020002 tile=4x1x34 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=5 taps=020222 tile=4x32x1 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=5 taps=020222 tile=4x32x1 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=6 taps=020200 tile=4x32x1 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=4 box=6 taps=020200 tile=4x32x1 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=1 taps=022202 tile=8x1x44 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=1 taps=022202 tile=8x1x44 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=2 taps=020002 tile=8x1x44 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=2 taps=020002 tile=8x1x44 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=3 taps=022202 tile=8x1x44 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=3 taps=022202 tile=8x1x44 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=4 taps=020002 tile=8x1x44 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=4 taps=020002 tile=8x1x44 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=5 taps=020222 tile=8x64x1 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=5 taps=020222 tile=8x64x1 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=6 taps=020200 tile=8x64x1 secondary=1 ymask=0 fmask=0 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_general op=dgrad dt=bf16 mt=8 box=6 taps=020200 tile=8x64x1 secondary=1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_mode2 op=dgrad dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=one tail=full': ('bf16', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_mode2 op=dgrad dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=several tail=full': ('bf16', 'auto', 4, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_mode2 op=dgrad dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=several tail=partial': ('bf16', 'auto', 3, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_mode2 op=dgrad dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=1 nsrc=1 rounds=one tail=full': ('bf16', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_mode2 op=dgrad dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=1 nsrc=1 rounds=several tail=full': ('bf16', 'auto', 4, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_mode2 op=dgrad dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=0 fmask=1 nsrc=1 rounds=several tail=partial': ('bf16', 'auto', 3, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_mode2 op=dgrad dt=bf16 mt=8 box=0 taps=020202 tile=8x8x8 secondary=0 ymask=0 fmask=0 nsrc=1 rounds=several tail=full': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_mask fam=bf16_mode2 op=dgrad dt=bf16 mt=8 box=0 taps=020202 tile=8x8x8 secondary=0 ymask=0 fmask=1 nsrc=1 rounds=several tail=full': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_multi fam=bf16_fused_launch op=dgrad dt=bf16 mt=8 nreg=1+6 nsrc=3 rounds=several tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_multi fam=bf16_general op=dgrad dt=bf16 mt=8 box=1 taps=022202 tile=8x1x44 secondary=1 ymask=0 fmask=1 nsrc=3 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_multi fam=bf16_general op=dgrad dt=bf16 mt=8 box=2 taps=020002 tile=8x1x44 secondary=1 ymask=0 fmask=1 nsrc=3 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_multi fam=bf16_general op=dgrad dt=bf16 mt=8 box=3 taps=022202 tile=8x1x44 secondary=1 ymask=0 fmask=1 nsrc=3 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_multi fam=bf16_general op=dgrad dt=bf16 mt=8 box=4 taps=020002 tile=8x1x44 secondary=1 ymask=0 fmask=1 nsrc=3 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_multi fam=bf16_general op=dgrad dt=bf16 mt=8 box=5 taps=020222 tile=8x64x1 secondary=1 ymask=0 fmask=1 nsrc=3 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_multi fam=bf16_general op=dgrad dt=bf16 mt=8 box=6 taps=020200 tile=8x64x1 secondary=1 ymask=0 fmask=1 nsrc=3 rounds=one tail=partial': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_bf16_multi fam=bf16_mode2 op=dgrad dt=bf16 mt=8 box=0 taps=020202 tile=8x8x8 secondary=0 ymask=0 fmask=1 nsrc=3 rounds=several tail=full': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=11x1x1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=12x1x1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 3, 24, 24, 24, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=12x1x1 ymask=0 fmask=1 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 5, 24, 24, 24, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=1 nsrc=1 rounds=one tail=full': ('f32', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=1 nsrc=1 rounds=several tail=full': ('f32', 'auto', 4, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=1 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 3, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=4x1x1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=6x1x1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 24, 24, 24, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=8x1x1 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 2, 24, 24, 24, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=8x1x2 ymask=0 fmask=1 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 4, 24, 24, 24, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=8x1x2 ymask=0 fmask=1 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 8, 24, 24, 24, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=2 tile=16x1x2 ymask=0 fmask=1 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 2, 48, 48, 48, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=2 tile=32x1x1 ymask=0 fmask=1 nsrc=1 rounds=several tail=full': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x10x6 r1=1x10x6 r2=16x1x4 r3=16x1x4 r4=6x10x1w nsrc=1 rounds=several tail=partial': ('f32', 'auto', 1, 48, 48, 48, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x18x2 r1=1x18x2 r2=16x1x4 r3=16x1x4 r4=6x9x1w nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x26x2 r1=1x26x2 r2=24x1x2 r3=24x1x2 r4=7x9x1w nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 24, 24, 24, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x26x2 r1=1x26x2 r2=24x1x2 r3=24x1x2 r4=7x9x1w nsrc=1 rounds=several tail=partial': ('f32', 'auto', 2, 24, 24, 24, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x4x16 r1=1x4x16 r2=64x1x1 r3=64x1x1 r4=6x10x1w nsrc=1 rounds=several tail=partial': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x7x8 r1=1x7x8 r2=32x1x2 r3=32x1x2 r4=7x9x1w nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_mask fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x7x8 r1=1x7x8 r2=32x1x2 r3=32x1x2 r4=7x9x1w nsrc=1 rounds=several tail=partial': ('f32', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv64_dgrad_fused_multi fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=0 fmask=1 nsrc=3 rounds=several tail=partial': ('f32', 'auto', 1, 48, 48, 48, 0),
    'fdn_conv64_dgrad_fused_multi fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=1 tile=4x1x1 ymask=0 fmask=1 nsrc=3 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv64_dgrad_fused_multi fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=2 tile=16x1x2 ymask=0 fmask=1 nsrc=3 rounds=several tail=partial': ('f32', 'auto', 2, 48, 48, 48, 0),
    'fdn_conv64_dgrad_fused_multi fam=wino2d op=dgrad dt=f32 hm=4 split=0 mb=2 tile=32x1x1 ymask=0 fmask=1 nsrc=3 rounds=several tail=full': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_dgrad_fused_multi fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x10x6 r1=1x10x6 r2=16x1x4 r3=16x1x4 r4=6x10x1w nsrc=3 rounds=several tail=partial': ('f32', 'auto', 1, 48, 48, 48, 0),
    'fdn_conv64_dgrad_fused_multi fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x18x2 r1=1x18x2 r2=16x1x4 r3=16x1x4 r4=6x9x1w nsrc=3 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv64_dgrad_fused_multi fam=wino2d_shell op=dgrad dt=f32 nreg=5 r0=1x4x16 r1=1x4x16 r2=64x1x1 r3=64x1x1 r4=6x10x1w nsrc=3 rounds=several tail=partial': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_fwd_bf16_mask fam=bf16_general op=fwd dt=bf16 mt=4 box=0 taps=020202 tile=2x8x8 secondary=0 ymask=1 fmask=0 nsrc=1 rounds=one tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_fwd_bf16_mask fam=bf16_mode2 op=fwd dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=1 fmask=0 nsrc=1 rounds=one tail=full': ('bf16', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv64_fwd_bf16_mask fam=bf16_mode2 op=fwd dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=1 fmask=0 nsrc=1 rounds=several tail=full': ('bf16', 'auto', 4, 32, 32, 32, 0),
    'fdn_conv64_fwd_bf16_mask fam=bf16_mode2 op=fwd dt=bf16 mt=4 box=0 taps=020202 tile=4x8x8 secondary=0 ymask=1 fmask=0 nsrc=1 rounds=several tail=partial': ('bf16', 'auto', 3, 32, 32, 32, 0),
    'fdn_conv64_fwd_bf16_mask fam=bf16_mode2 op=fwd dt=bf16 mt=8 box=0 taps=020202 tile=8x8x8 secondary=0 ymask=1 fmask=0 nsrc=1 rounds=several tail=full': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=11x1x1 ymask=1 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 32, 32, 32, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=12x1x1 ymask=1 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 3, 24, 24, 24, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=12x1x1 ymask=1 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 5, 24, 24, 24, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=1 fmask=0 nsrc=1 rounds=one tail=full': ('f32', 'auto', 2, 32, 32, 32, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=1 fmask=0 nsrc=1 rounds=several tail=full': ('f32', 'auto', 4, 32, 32, 32, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=16x1x1 ymask=1 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 3, 32, 32, 32, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=4x1x1 ymask=1 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=6x1x1 ymask=1 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 1, 24, 24, 24, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=8x1x1 ymask=1 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 2, 24, 24, 24, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=8x1x2 ymask=1 fmask=0 nsrc=1 rounds=one tail=partial': ('f32', 'auto', 4, 24, 24, 24, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=1 tile=8x1x2 ymask=1 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 8, 24, 24, 24, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=2 tile=16x1x2 ymask=1 fmask=0 nsrc=1 rounds=several tail=partial': ('f32', 'auto', 2, 48, 48, 48, 0),
    'fdn_conv64_fwd_mask fam=wino2d op=fwd dt=f32 hm=4 split=0 mb=2 tile=32x1x1 ymask=1 fmask=0 nsrc=1 rounds=several tail=full': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv_cout1_dgrad_folded fam=head_dgrad op=dgrad dt=f32 mask=0 walk=1 rounds=one tail=partial': ('f32', 'direct', 1, 16, 16, 16, 0),
    'fdn_conv_cout1_dgrad_folded fam=head_dgrad op=dgrad dt=f32 mask=0 walk=1 rounds=several tail=partial': ('f32', 'direct', 1, 48, 48, 48, 0),
    'fdn_conv_cout1_dgrad_folded fam=head_dgrad op=dgrad dt=f32 mask=0 walk=2 rounds=several tail=partial': ('f32', 'direct', 3, 48, 48, 48, 0),
    'fdn_conv_cout1_dgrad_folded fam=head_dgrad op=dgrad dt=f32 mask=0 walk=3 rounds=several tail=full': ('f32', 'direct', 1, 128, 128, 128, 0),
    'fdn_conv_cout1_dgrad_folded fam=head_dgrad op=dgrad dt=f32 mask=0 walk=3 rounds=several tail=partial': ('f32', 'direct', 5, 48, 48, 48, 0),
    'fdn_conv_cout1_dgrad_folded_bf16_mask fam=head_dgrad op=dgrad dt=bf16 mask=1 walk=3 rounds=several tail=full': ('bf16', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv_cout1_dgrad_folded_mask fam=head_dgrad op=dgrad dt=f32 mask=1 walk=1 rounds=one tail=partial': ('f32', 'auto', 1, 16, 16, 16, 0),
    'fdn_conv_cout1_dgrad_folded_mask fam=head_dgrad op=dgrad dt=f32 mask=1 walk=1 rounds=several tail=partial': ('f32', 'auto', 1, 48, 48, 48, 0),
    'fdn_conv_cout1_dgrad_folded_mask fam=head_dgrad op=dgrad dt=f32 mask=1 walk=2 rounds=several tail=partial': ('f32', 'auto', 3, 48, 48, 48, 0),
    'fdn_conv_cout1_dgrad_folded_mask fam=head_dgrad op=dgrad dt=f32 mask=1 walk=3 rounds=several tail=full': ('f32', 'auto', 1, 128, 128, 128, 0),
    'fdn_conv_cout1_dgrad_folded_mask fam=head_dgrad op=dgrad dt=f32 mask=1 walk=3 rounds=several tail=partial': ('f32', 'auto', 5, 48, 48, 48, 0),
    'fdn_upsample_trilinear_bwd fam=upsample_bwd op=bwd dt=f32 R=2 hb=2 rounds=several tail=full': ('f32', 'auto', 8, 24, 24, 24, 0),
    'fdn_upsample_trilinear_bwd fam=upsample_bwd op=bwd dt=f32 R=2 hb=2 rounds=several tail=partial': ('f32', 'auto', 1, 24, 24, 24, 0),
    'fdn_upsample_trilinear_bwd fam=upsample_bwd op=bwd dt=f32 R=4 hb=2 rounds=several tail=full': ('f32', 'auto', 1, 32, 32, 32, 0),
    'fdn_upsample_trilinear_bwd_bf16 fam=upsample_bwd op=bwd dt=bf16 R=4 hb=2 rounds=several tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
    'fdn_upsample_trilinear_fwd fam=upsample_fwd op=fwd dt=f32 R=2 staged=1 rounds=several tail=full': ('f32', 'auto', 1, 24, 24, 24, 0),
    'fdn_upsample_trilinear_fwd fam=upsample_fwd op=fwd dt=f32 R=4 staged=1 rounds=several tail=full': ('f32', 'auto', 1, 32, 32, 32, 0),
    'fdn_upsample_trilinear_fwd_bf16 fam=upsample_fwd op=fwd dt=bf16 R=4 staged=1 rounds=several tail=full': ('bf16', 'auto', 1, 32, 32, 32, 0),
}


@pytest.fixture(scope="module")
def product_plans():
    plans = collect_product_plans()
    print("\n%d plan keys reached by the product shapes:" % len(plans))
    for k, v in sorted(plans.items()):
        print("  %s\n      case %s\n      reached by %s" % (k, PLAN_CASES.get(k, "NONE"), ", ".join("%s %s%s" % (s[7], s[0], "" if s[1] == "auto" else " direct") for s in v)))
    return plans


def test_every_product_plan_has_a_case(product_plans):
    miss = missing_cases(product_plans, PLAN_CASES)
    assert not miss, "product plans without a float64 case in PLAN_CASES:\n" + "\n".join(
        "  %s\n    reached by %s" % (k, "; ".join("%s N=%d %dx%dx%d" % (s[7], s[2], s[3], s[4], s[5]) for s in v)) for k, v in miss)


@pytest.mark.parametrize("key", sorted(PLAN_CASES))
def test_plan_case_matches_float64(fdn, key):
    reached = run_case(key, PLAN_CASES[key])
    assert key in reached, "case %s no longer reaches its plan %s; it reached:\n  %s" % (PLAN_CASES[key], key, "\n  ".join(sorted(reached)))


@pytest.mark.parametrize("dt,dims,nl,launches", [
    ("f32", (1, 8, 8, 8), 17, ["fam=wgrad_wino_batch layers=16 splits=4", "fam=wgrad_wino dep=1 splits=8"]),
    ("bf16", (5, 16, 16, 16), 15, ["fam=wgrad_bf16_batch layers=7 splits=24", "fam=wgrad_bf16_batch layers=4 splits=40"] + ["fam=wgrad_bf16_batch layers=4 splits=40"])])
def test_batch_steps_reuse_the_workspace_behind_each_other(fdn, dt, dims, nl, launches):
    """A batch no product shape reaches: several steps of one plan (csrc/wgrad64_plan.h), each writing its partial sums over the ones the
    step before has reduced.  fp32, 17 layers: a chunk of 16 and then a lone layer on the single-layer kernel -- bit-equal to the
    single-layer entry point on the same operands.  bf16, 15 layers at the smallest grid with 320 one-plane tiles: 7 + 4 + 4 (no layer
    count leaves a lone bf16 layer behind chunks: tests/test_wgrad64_plan.py).  Every layer of a chunk against float64."""
    bf = dt == "bf16"
    o = bops if bf else ops
    g = torch.Generator(device="cuda").manual_seed(nl)
    xs = [torch.randn(dims + (64,), device="cuda", generator=g).to(torch.bfloat16 if bf else torch.float32) for _ in range(nl)]
    dzs = [torch.randn(dims + (64,), device="cuda", generator=g).to(torch.bfloat16 if bf else torch.float32) for _ in range(nl)]
    dws = [torch.full((3, 3, 3, 64, 64), float("nan"), device="cuda") for _ in range(nl)]
    with _lib.test_build() as lib, PlanTap(lib) as tap:
        tap.take()
        o.conv3d_wgrad_batch(xs, dzs, dws)
        torch.cuda.synchronize()
        recs = [r for _, r in tap.take()]
        lone = o.conv3d_wgrad(xs[-1], dzs[-1], 3, 64, 64)[0] if not bf else None
        torch.cuda.synchronize()
    got = ["fam=%s %s splits=%s" % (r["fam"], "layers=" + r["layers"] if "layers" in r else "dep=" + r["dep"], r["splits"]) for r in recs]
    assert got == launches
    chunked = nl - 1 if not bf else nl
    for i in range(chunked):
        _wgrad_check(xs[i], dzs[i], dws[i], "%s %s layer %d of %d" % (dt, dims, i, nl))
    if not bf:
        assert torch.equal(dws[-1], lone), "the lone layer behind the chunk differs from fdn_conv3d_wgrad on the same operands"


def test_gate_reports_a_forced_tile_without_a_case(fdn):
    """A tile shape outside the table (forced through the test hook) is named by the gate, with the shape that reached it."""
    with _lib.test_build() as lib:
        assert lib.fdn_debug_set_conv64_wino2d_tile(3 | 1 << 8 | 1 << 16) == 0       # td 3 x ch 1 x cw 1: no planner picks it
        try:
            with PlanTap(lib) as tap:
                x = torch.randn((1, 24, 24, 24, 64), device="cuda")
                w = torch.randn((3, 3, 3, 64, 64), device="cuda") * 0.03
                ops.conv3d_fwd(x, w, None, ops.ACT_NONE)
                torch.cuda.synchronize()
                recs = tap.take()
        finally:
            lib.fdn_debug_set_conv64_wino2d_tile(0)
    plans = {}
    for e, r in recs:
        plans.setdefault(plan_key(e, r), []).append(("f32", "auto", 1, 24, 24, 24, 0, "forced"))
    forced = [k for k in plans if "tile=3x1x1" in k]
    assert len(forced) == 1, plans
    assert [k for k, _ in missing_cases(plans, PLAN_CASES)] == forced


def test_empty_shard_launches_no_planned_kernel_and_steps(fdn):
    """Data-parallel ragged tails: 60 patches at batch 8 over 3 ranks end the epoch on shards of 8, 4 and 0 (ShardedIndexSampler keeps
    the ragged batch).  The sizes 1..B are all collected above; a rank with N = 0 launches no conv / wgrad / head kernel and its step
    (zero gradient, Adam) and its evaluation do not fail."""
    parallel = importlib.import_module("4dflownet_amd.parallel")
    last = [list(parallel.ShardedIndexSampler(60, 8, False, rank_=r, world=3))[-1].size for r in range(3)]
    assert last == [8, 4, 0]
    tc = trainer.TrainerController(16, 1, initial_learning_rate=1e-4, quicksave_enable=False, low_resblock=2, hi_resblock=1, seed=0)
    empty = tuple(a[:0] for a in O.synthetic_batch(1, 16, 1, seed=5))
    w0 = tc.model.flat_w.clone()
    with _lib.test_build() as lib, PlanTap(lib) as tap:
        tap.take()
        assert tc.train_step(empty) is None
        assert tc.test_step(empty) is None
        torch.cuda.synchronize()
        recs = tap.take()
    assert recs == [], recs
    assert torch.isfinite(tc.model.flat_w).all() and float(tc.model.flat_g.abs().max()) == 0.0
    assert float((tc.model.flat_w - w0).abs().max()) <= 1.05e-4


if __name__ == "__main__":
    # regenerate PLAN_CASES: collect the product plans, take the cheapest shape of each, check it, print the table
    plans = collect_product_plans()
    cases = derive_cases(plans)
    failed = []
    for k in sorted(cases):
        try:
            reached = run_case(k, cases[k])
            ok = k in reached
        except AssertionError as e:
            ok = False
            print("FAIL %s: %s" % (k, e), file=sys.stderr)
        if not ok:
            failed.append(k)
    print("PLAN_CASES = {")
    for k in sorted(cases):
        print("    %r: %r,%s" % (k, cases[k], "   # FAILED" if k in failed else ""))
    print("}")
    print("%d keys, %d failed" % (len(cases), len(failed)), file=sys.stderr)

"""The 64 -> 1 head kernels past their grid caps, and the thin-layer reductions past theirs, against float64 over the WHOLE tensor.

The head kernels (csrc/heads_mfma.hip) run persistent grids: dgrad min(tiles, 1024) workgroups, wgrad min(tiles, 512) for fp32 storage and
min(tiles, 768) for bf16, forward 3 * ceil(tiles / 1536) tiles per workgroup; a tile is 4 x 8 x 8 voxels.  Below the cap a workgroup does one
tile; above it the second and later tiles take the dz halo through a double buffer whose parity flips per tile, keep the weight-gradient
accumulators and the bias partials live across the walk, and prefetch the next tile's rows.  Every product step runs there (8 x 48^3 is 3456
tiles, 4 x 128^3 is 32768); the other kernel tests stop at 432.  A skipped tile or a stale halo need not touch a sampled voxel, so every
output element is compared here; the reference (tests/_head_ref.py, held to the numpy oracle by tests/test_head_ref.py) runs on the device.

Every head case first reads the launch-plan recorder (the test build) and asserts the grid, tiles and walk class it is named for: a
changed cap fails the case instead of silently moving it off the walk it tests.

    name     (N,D,H,W)         tiles   voxels
    S512     (4,8,64,64)         512   131072   fp32 wgrad: grid = tiles = cap, one tile each
    S513     (1,9,65,148)        513    86580   fp32 wgrad: cap + 1 (workgroup 0 walks 2); 1 plane, 1 row, 4 columns in the ragged last tiles
    S768     (6,8,64,64)         768   196608   bf16 wgrad: grid = cap
    S770     (2,17,49,84)        770   139944   bf16 wgrad: cap + 2
    S1024    (8,8,64,64)        1024   262144   dgrad: grid = cap
    S1025    (1,17,33,324)      1025   181764   dgrad: cap + 1; wgrad walks 2-3 (fp32), 1-2 (bf16)
    S2600    (13,5,33,156)      2600   334620   dgrad walks 2 and 3 (the parity flips twice) across sample boundaries; wgrad walks 5-6 (fp32),
                                                3-4 (bf16); forward iters = 6 with a short last workgroup
    S8448    (1,129,128,128)    8448  2113536   the C = 1 bias gradient past its 512 x 4096 cap; wgrad walks of 16-17

Tolerances: fp32 results 2e-5 of max |ref| (RTOL of test_gpu_kernels.py); bf16 results the one-ulp rule of test_gpu_bf16.py; sums over
voxels 1e-5 of the sum of the terms' magnitudes (the bound any fp32 summation order obeys with room to spare).  Each check prints its worst
error as a fraction of its tolerance before it asserts (pytest -s shows them)."""
import importlib

import pytest
import torch

import _head_ref as R
from test_gpu_bf16 import close_bf16
from test_gpu_kernels import RTOL
from test_gpu_plan_coverage import PlanTap, sign_mask_words

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("4dflownet_amd._lib")
ops = importlib.import_module("4dflownet_amd.ops")
bops = importlib.import_module("4dflownet_amd.ops_bf16")

SHAPES = {"S512": (4, 8, 64, 64), "S513": (1, 9, 65, 148), "S768": (6, 8, 64, 64), "S770": (2, 17, 49, 84), "S1024": (8, 8, 64, 64),
          "S1025": (1, 17, 33, 324), "S2600": (13, 5, 33, 156), "S8448": (1, 129, 128, 128)}
# what the recorder must report: (grid, tiles, walk class = min(ceil(tiles / grid), 3))
DGRAD_PLAN = {"S1024": (1024, 1024, 1), "S1025": (1024, 1025, 2), "S2600": (1024, 2600, 3)}
WGRAD_PLAN = {("f32", "S512"): (512, 512, 1), ("f32", "S513"): (512, 513, 2), ("f32", "S1025"): (512, 1025, 3), ("f32", "S2600"): (512, 2600, 3),
              ("f32", "S8448"): (512, 8448, 3), ("bf16", "S768"): (768, 768, 1), ("bf16", "S770"): (768, 770, 2), ("bf16", "S2600"): (768, 2600, 3)}
FWD_PLAN = {"S1025": (342, 1025, 3, 2), "S2600": (434, 2600, 6, 2)}             # (grid, tiles, iters, tiles of the last workgroup)
SUM_TOL = 1e-5


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(shape, device="cuda", generator=g) * scale


def _report(name, err, tol):
    """Print the worst error as a fraction of its tolerance, then assert.  err, tol: tensors of one shape (or floats)."""
    err, tol = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(tol, dtype=torch.float64)
    frac = float((err / tol.clamp_min(1e-300)).max())
    print("\n  [head_walks] %-72s %.4f of tolerance" % (name, frac))
    assert bool((err <= tol).all()), "%s: %.3f of tolerance" % (name, frac)


def _one_launch(tap, fam):
    recs = [r for _, r in tap.take() if r.get("fam") == fam]
    assert len(recs) == 1, "expected one %s launch in the recorder, got %s" % (fam, recs)
    return recs[0]


def _assert_walk(rec, dt, grid, tiles, walk, name):
    got = (rec["dt"], int(rec["grid"]), int(rec["tiles"]), int(rec["walk"]))
    assert got == (dt, grid, tiles, walk), "%s: launched (dt, grid, tiles, walk) = %s, the case is named for %s" % (name, got, (dt, grid, tiles, walk))


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ (a) head dgrad
_DG = {}             # operands and the linear float64 reference of ONE shape, shared by its dtype x activation cases (never modified)


def _dgrad_operands(sname):
    if _DG.get("name") != sname:
        _DG.clear()
        torch.cuda.empty_cache()
        dims = SHAPES[sname]
        g = _gen(1000 + dims[3])
        dpred, w, y = _randn(g, *dims, 3), _randn(g, 3, 3, 3, 64, 1, scale=0.1), _randn(g, *dims, 64)
        _DG.update(name=sname, dims=dims, dpred=dpred, w=w, y=y, lin=R.head_dgrad_ref(dpred[..., 1], w, dims))
    return _DG


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_reference():
    yield
    _DG.clear()
    torch.cuda.empty_cache()


def _head_dgrad(o, c, y_prev, act, mask=None):
    db = torch.full((64,), float("nan"), device="cuda")
    out = o.conv_cout1_dgrad_folded(c["dpred"], c["w"], c["dims"], y_prev, act, 0.2, lddz=3, dz_coff=1, dbias_prev=db, mask=mask)
    return out, db


@pytest.mark.parametrize("act", ["none", "relu", "leaky"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("sname", ["S1024", "S1025", "S2600"])
def test_head_dgrad_every_voxel(fdn, sname, dt, act):
    """dz_prev of the whole grid and the producer's bias gradient summed over the walks, as the product calls it (channel 1 of the (N,V,3)
    prediction gradient, dbias_prev given)."""
    c = _dgrad_operands(sname)
    bf = dt == "bf16"
    o = bops if bf else ops
    name = "head dgrad %s %s %s" % (sname, dt, act)
    y = c["y"].to(torch.bfloat16) if bf else c["y"]                       # (the rounding keeps every sign: act' is the same in both modes)
    code = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}[act]
    with _lib.test_build() as lib, PlanTap(lib) as tap:
        tap.take()
        out, db = _head_dgrad(o, c, None if act == "none" else y, code)
        torch.cuda.synchronize()
        rec = _one_launch(tap, "head_dgrad")
    _assert_walk(rec, dt, *DGRAD_PLAN[sname], name)
    assert rec["mask"] == "0"
    ref = c["lin"]
    if act != "none":
        slope = 0.0 if act == "relu" else 0.2
        ref = ref * ((c["y"] > 0).double() * (1.0 - slope) + slope)
    assert bool(torch.isfinite(out).all()), name
    if bf:
        err = (out.double() - ref).abs()
        print("\n  [head_walks] %-72s %.4f of tolerance" % (name, float((err / (2.0 ** -8 * ref.abs() + 2e-5 * ref.abs().max())).max())))
        close_bf16(out, ref.cpu().numpy(), name=name)
    else:
        _report(name, (out.double() - ref).abs().max(), RTOL * ref.abs().max())
    r2 = ref.reshape(-1, 64)
    _report(name + ": producer bias gradient", (db.double() - r2.sum(dim=0)).abs(), SUM_TOL * r2.abs().sum(dim=0))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("sname", ["S1025", "S2600"])
def test_head_dgrad_sign_mask_equals_the_y_prev_form(fdn, sname, dt):
    """The sign-mask forms (fp32: planar words built from y; bf16: the mask the 64->64 forward writes beside y) give dz_prev and the producer's
    bias gradient bit for bit on the walked tiles too."""
    c = _dgrad_operands(sname)
    N, D, H, W = c["dims"]
    g = _gen(29)
    if dt == "f32":
        o, y = ops, c["y"]
        mask = sign_mask_words(y, planar=True)
    else:
        o = bops
        x = _randn(g, N, D, H, W, 64).to(torch.bfloat16)
        wf, _ = bops.pack_conv64_weights(_randn(g, 3, 3, 3, 64, 64, scale=0.05))
        mask = bops.new_sign_mask(x)
        y = bops.conv64_fwd(x, wf, None, ops.ACT_RELU, 0.2, None, mask=mask)              # the head's 64->64 conv (ReLU)
    name = "head dgrad sign mask %s %s" % (sname, dt)
    with _lib.test_build() as lib, PlanTap(lib) as tap:
        tap.take()
        a, dba = _head_dgrad(o, c, y, ops.ACT_RELU)
        rec_y = _one_launch(tap, "head_dgrad")
        b, dbb = _head_dgrad(o, c, None, ops.ACT_RELU, mask=mask)
        torch.cuda.synchronize()
        rec_m = _one_launch(tap, "head_dgrad")
    for rec, m in ((rec_y, "0"), (rec_m, "1")):
        _assert_walk(rec, dt, *DGRAD_PLAN[sname], name)
        assert rec["mask"] == m, rec
    assert torch.equal(a, b) and torch.equal(dba, dbb), name
    assert 0.2 < (a == 0).float().mean().item() < 0.8, name                       # (the ReLU mask really bit)


# ------------------------------------------------------------------------------------------------ (b) head wgrad and its C = 1 bias gradient
def _wgrad_operands(sname, dt):
    dims = SHAPES[sname]
    g = _gen(2000 + dims[3])
    x, dpred = _randn(g, *dims, 64), _randn(g, *dims, 3)
    return (x.to(torch.bfloat16) if dt == "bf16" else x), dpred


@pytest.mark.parametrize("dt,sname", sorted(WGRAD_PLAN))
def test_head_wgrad_all_taps(fdn, dt, sname):
    x, dpred = _wgrad_operands(sname, dt)
    o = bops if dt == "bf16" else ops
    name = "head wgrad %s %s" % (sname, dt)
    with _lib.test_build() as lib, PlanTap(lib) as tap:
        tap.take()
        dw, db = o.conv3d_wgrad(x, dpred, 3, 64, 1, want_bias=True, lddz=3, dz_coff=1)
        torch.cuda.synchronize()
        rec = _one_launch(tap, "head_wgrad")
    _assert_walk(rec, dt, *WGRAD_PLAN[(dt, sname)], name)
    dz = dpred[..., 1]
    ref, bound = R.head_wgrad_ref(x, dz), R.head_wgrad_bound(x, dz)
    del x
    assert tuple(dw.shape) == (3, 3, 3, 64, 1) and bool(torch.isfinite(dw).all()), name
    _report(name, (dw.double() - ref).abs(), SUM_TOL * bound)
    _report(name + ": bias gradient", abs(float(db[0]) - float(dz.double().sum())), SUM_TOL * float(dz.double().abs().sum()))


# ------------------------------------------------------------------------------------------------ (c) head forward
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("sname", ["S1025", "S2600"])
def test_head_fwd_every_voxel(fdn, sname, dt):
    """The three-slot ring over several rounds with a predicated tail, written into channel 1 of an (N,V,3) tensor whose other channels stay."""
    dims = SHAPES[sname]
    g = _gen(3000 + dims[3])
    x, w, b = _randn(g, *dims, 64), _randn(g, 3, 3, 3, 64, 1, scale=0.1), _randn(g, 1)
    if dt == "bf16":
        x = x.to(torch.bfloat16)
    name = "head fwd %s %s" % (sname, dt)
    FILL = 7.5
    pred = torch.full(dims + (3,), FILL, device="cuda")
    with _lib.test_build() as lib, PlanTap(lib) as tap:
        tap.take()
        (bops if dt == "bf16" else ops).conv3d_fwd(x, w, b, ops.ACT_NONE, out=pred, ldy=3, y_coff=1)
        torch.cuda.synchronize()
        rec = _one_launch(tap, "head_fwd")
    got = (rec["dt"], int(rec["grid"]), int(rec["tiles"]), int(rec["iters"]), int(rec["last"]))
    assert got == (dt,) + FWD_PLAN[sname], "%s: launched (dt, grid, tiles, iters, last) = %s, the case is named for %s" % (name, got, FWD_PLAN[sname])
    ref = torch.full(dims + (3,), FILL, device="cuda", dtype=torch.float64)
    ref[..., 1] = R.head_fwd_ref(x, w, b)
    _report(name, (pred.double() - ref).abs().max(), RTOL * ref[..., 1].abs().max())
    assert bool((pred[..., 0] == FILL).all()) and bool((pred[..., 2] == FILL).all()), name + ": a neighbouring channel was written"


# ------------------------------------------------------------------------------------------------ (d) run to run
def test_walked_head_gradients_are_bit_identical_run_to_run(fdn):
    """Fixed summation order: the bias partials of a dgrad walk, the wgrad accumulators and both partial reductions."""
    c = _dgrad_operands("S2600")
    x, dpred = _wgrad_operands("S2600", "f32")
    runs = []
    for _ in range(2):
        out, db = _head_dgrad(ops, c, c["y"], ops.ACT_LEAKY)
        dw, dbw = ops.conv3d_wgrad(x, dpred, 3, 64, 1, want_bias=True, lddz=3, dz_coff=1)
        runs.append((out, db, dw, dbw))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ (e) thin-layer reductions past their caps
def _cin3_wgrad_ref(x, dz):
    """dW[a,b,c,ci,co] = sum_o x[clamp(o + (a,b,c) - 1)][ci] dz[o][co] as one float64 matmul over the 81 shifted input columns."""
    N, D, H, W = x.shape[:4]
    xp = R.edge_pad(R.edge_pad(R.edge_pad(x.double(), 1), 2), 3)
    cols = torch.stack([xp[:, a:a + D, b:b + H, c:c + W] for a in range(3) for b in range(3) for c in range(3)], dim=4)      # (N,D,H,W,27,3)
    return torch.matmul(cols.reshape(-1, 81).t(), dz.double().reshape(-1, 64)).reshape(3, 3, 3, 3, 64)


@pytest.mark.parametrize("shape,dt", [((1, 13, 72, 72), "f32"), ((1, 13, 72, 71), "f32"), ((1, 13, 72, 72), "bf16")])
def test_cin3_wgrad_and_bias_grad_past_their_caps(fdn, shape, dt):
    """3 -> 64 weight gradient (min(ceil(nvox / 128), 512) blocks: capped above 65536 voxels; the im2col MFMA kernel for even W, the VALU kernel
    of the product library for odd W) and the C = 64 bias gradient (min(ceil(nvox / 256), 256) blocks: capped above 65536)."""
    N, D, H, W = shape
    assert N * D * H * W > 65536
    g = _gen(4000 + W)
    x, dz = _randn(g, N, D, H, W, 3), _randn(g, N, D, H, W, 64)
    o = ops
    if dt == "bf16":
        o, x, dz = bops, x.to(torch.bfloat16), dz.to(torch.bfloat16)
    dw, db = o.conv3d_wgrad(x, dz, 3, 3, 64, want_bias=True)
    name = "3->64 wgrad %s %s" % (shape, dt)
    _report(name, (dw.double() - _cin3_wgrad_ref(x, dz)).abs(), SUM_TOL * _cin3_wgrad_ref(x.abs(), dz.abs()))
    d2 = dz.double().reshape(-1, 64)
    _report(name + ": bias gradient", (db.double() - d2.sum(dim=0)).abs(), SUM_TOL * d2.abs().sum(dim=0))


@pytest.mark.parametrize("shape,dt", [((4, 32, 32, 32), "f32"), ((1, 33, 64, 63), "f32"), ((4, 32, 32, 32), "bf16")])
def test_conv1x1_wgrad_on_and_past_its_cap(fdn, shape, dt):
    """1x1x1 (64+64) -> 64 weight gradient: clamp(ceil((nvox / 2) / 256), 1, 256) workgroups, 256 exactly at 131072 voxels and capped above."""
    N, D, H, W = shape
    assert N * D * H * W >= 131072
    g = _gen(5000 + W)
    xa, xb, dz = _randn(g, N, D, H, W, 64), _randn(g, N, D, H, W, 64), _randn(g, N, D, H, W, 64)
    o = ops
    if dt == "bf16":
        o, xa, xb, dz = bops, xa.to(torch.bfloat16), xb.to(torch.bfloat16), dz.to(torch.bfloat16)
    dw, _ = o.conv3d_wgrad(xa, dz, 1, 128, 64, x2=xb)
    cat, d2 = torch.cat([xa, xb], dim=-1).double().reshape(-1, 128), dz.double().reshape(-1, 64)
    _report("1x1 wgrad %s %s" % (shape, dt), (dw.double().reshape(128, 64) - torch.matmul(cat.t(), d2)).abs(), SUM_TOL * torch.matmul(cat.abs().t(), d2.abs()))

"""Guard bands: a launch touches nothing outside its operands, and nothing outside them reaches its result.

tests/test_gpu_pow2_scaling.py proves "a kernel's result may depend on nothing but its operands" for scale; this file proves it for the
memory AROUND the operands.  Torch's caching allocator packs tensors next to each other and rounds sizes up, so a stray store into the
slack behind an output, an under-reported fdn_*_workspace_bytes() or a load that overhangs an operand ("times zero", or let through by a
buffer range one row too generous) goes unseen by every other test: the neighbour is finite junk and max |ref| hides it.  In a training
run the neighbour can be a NaN.

One launch under guard (run_guarded): EVERY pointer operand -- activations, weights, bias, packs, masks, flags, device scalars, offset
and descriptor tables, scratch (dxpad), workspace, outputs -- lives in the middle of an allocation of its own (tests/_guarded.py), a band
of at least 4096 elements or one padded slab on either side; a workspace has exactly the advertised byte count.  The launch runs twice:
    run A  every band NaN (int16 all ones, uint8 0xFF), outputs / dxpad / workspace prefilled with NaN;
    run B  every band and prefill the finite sentinel 1234.5 (int16 0x5A5A, uint8 0x00).
Asserted:
    (a) every band of every operand is bit-intact after each run;
    (b) the interior of every const operand is bit-unchanged;
    (c) the outputs of A and B are torch.equal, finite and hold no sentinel; where an entry point writes only part of a tensor the rest
        holds the prefill bit for bit;
    (d) the output equals the plain call with ordinary torch.empty operands, bit for bit;
    (e) the output matches the float64 oracle at the tolerance of the entry point's existing parity test (imported, none invented).
No operand sits at the start or end of an allocation, none has an odd alignment (the bands are multiples of 512 bytes) or extents that
disagree with its storage: this file cannot provoke a fault, it only makes an existing overhang visible.

Grids: the shapes the parity tests chose for their tile overhangs -- (1,1,1,1), (1,2,3,1), (3,4,4,2), (1,5,7,9) direct strips off the
raster, (1,5,7,12) 1-D Winograd with odd H, (2,9,2,24) F(2,3) x F(4,3) with H = 2 and two samples, (1,1,4,4) one F(4,3) x F(4,3) cell,
(1,7,12,20) ragged cell rows and columns, (2,6,6,6); bf16 adds (1,16,16,16), (1,3,20,11), (1,17,9,12).  A two-sample grid is in each
family: the far edge of sample 0 borders sample 1, the far edge of the last sample borders the band."""
import functools
import importlib
import types

import numpy as np
import pytest
import torch

import _guarded as G
import _self_ensemble as se
from _divergence import divergence_loss
from oracle import flownet_oracle as O
from test_gpu_bf16 import close_bf16, close_f32, rb
from test_gpu_divergence_loss import make_case, rel_err
from test_gpu_kernels import RTOL, close, dev
from test_gpu_plan_coverage import sign_mask_words
from test_gpu_pow2_scaling import BF_VARIANTS, bf_variant, hooks

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("4dflownet_amd._lib")
ops = importlib.import_module("4dflownet_amd.ops")
bops = importlib.import_module("4dflownet_amd.ops_bf16")
ddev = importlib.import_module("4dflownet_amd.data_device")

F32, BF16, I16, U8 = torch.float32, torch.bfloat16, torch.int16, torch.uint8
GRIDS = [(1, 1, 1, 1), (1, 2, 3, 1), (3, 4, 4, 2), (1, 5, 7, 9), (1, 5, 7, 12), (2, 9, 2, 24), (1, 1, 4, 4), (1, 7, 12, 20), (2, 6, 6, 6)]
BF_GRIDS = GRIDS + [(1, 16, 16, 16), (1, 3, 20, 11), (1, 17, 9, 12)]
DT_GRIDS = [("f32", d) for d in GRIDS] + [("bf16", d) for d in BF_GRIDS]
ALGOS = {"auto": ops.ALGO_AUTO, "direct": ops.ALGO_DIRECT, "wino_w": ops.ALGO_WINO_W, "wino_h2": ops.ALGO_WINO_H2, "bf16x3": ops.ALGO_WINO_BF16X3}
LEAKY, RELU, NONE = ops.ACT_LEAKY, ops.ACT_RELU, ops.ACT_NONE
HEAD_WS_BYTES = 2048 * 64 * 4                        # include/fdn.h: the workspace of fdn_conv_cout1_dgrad_folded with dbias_prev


# ---------------------------------------------------------------------------------------------------------------- the procedure
def _holds(t, fill):
    t = t.contiguous()
    return bool((G._bits(t) == G._bits(torch.full((1,), fill, dtype=t.dtype, device=t.device))).all())


def _new_out(spec, run):
    if spec[0] == "ws":                                   # ("ws", nbytes): exactly the advertised bytes
        f = G.fill_for(F32, run)
        return G.exact_workspace(spec[1], f, f, "cuda")
    shape, dtype = spec
    return G.guarded(shape, dtype, G.fill_for(dtype, run), "cuda")


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(G._bits(a.contiguous()), G._bits(b.contiguous())))


def run_guarded(name, launch, const=None, inout=None, out=None, oracle=None, sparse=False):
    """launch(T) -> (written, kept): T maps operand names to tensors; `written` are the tensors (or views) the launch must have written in
    full, `kept` views of outputs it must not have touched.  const: read-only operands {name: tensor, or f(T) -> tensor for a table that
    holds addresses of other operands}; inout: operands updated in place; out: {name: (shape, dtype) or ("ws", nbytes)}, prefilled.
    oracle(written) holds assertion (e).  sparse: `written` may hold unwritten elements (a pack with unused slots): what run A left as
    its prefill must be run B's prefill, everything else equal."""
    const, inout, out = const or {}, inout or {}, out or {}
    results = {}
    for run in ("A", "B"):
        H = {}
        for k, v in list(const.items()) + list(inout.items()):
            if not callable(v):
                H[k] = G.guarded_like(v, G.fill_for(v.dtype, run))
        for k, spec in out.items():
            H[k] = _new_out(spec, run)
        T = {k: h.t for k, h in H.items()}
        for k, v in const.items():
            if callable(v):
                val = v(T)
                H[k] = G.guarded_like(val, G.fill_for(val.dtype, run))
                T[k] = H[k].t
        snaps = {k: H[k].t.clone() for k in const}
        written, kept = launch(T)
        torch.cuda.synchronize()
        for k, h in H.items():                                                                        # (a)
            assert G.intact(h), "%s, run %s: the band of %r was written at view-relative flat indices %s" % (name, run, k, h.damaged())
        for k, s in snaps.items():                                                                    # (b)
            assert G.unchanged(H[k], s), "%s, run %s: the const operand %r was modified" % (name, run, k)
        for i, t in enumerate(kept):                                                                  # (c), the part not written
            assert _holds(t, G.fill_for(t.dtype, run)), "%s, run %s: kept view %d lost its prefill" % (name, run, i)
        results[run] = [t.clone() for t in written]
    for i, (a, b) in enumerate(zip(results["A"], results["B"])):                                      # (c)
        if sparse:
            un = G._bits(a) == G._bits(torch.full((1,), G.fill_for(a.dtype, "A"), dtype=a.dtype, device=a.device))
            assert bool((G._bits(b)[un] == G._bits(torch.full((1,), G.fill_for(b.dtype, "B"), dtype=b.dtype, device=b.device))).all()), \
                "%s: output %d has elements written in run B only" % (name, i)
            assert not bool(un.all()), "%s: output %d was not written at all" % (name, i)
            a, b = a[~un], b[~un]
        if not _same_bits(a, b):
            bad = (G._bits(a) != G._bits(b)).reshape(-1)
            j = int(bad.nonzero()[0])
            raise AssertionError("%s: output %d differs between NaN and finite surroundings at %d of %d elements; flat index %d holds %r / %r"
                                 % (name, i, int(bad.sum()), bad.numel(), j, a.reshape(-1)[j].item(), b.reshape(-1)[j].item()))
        if a.is_floating_point():
            assert bool(torch.isfinite(a).all()), "%s: output %d is not finite (%d elements)" % (name, i, int((~torch.isfinite(a)).sum()))
            assert not bool((b == G.SENTINEL).any()), "%s: output %d holds the sentinel" % (name, i)
    T = {}                                                                                            # (d) the plain call
    for k, v in list(const.items()) + list(inout.items()):
        if not callable(v):
            T[k] = v.clone()
    for k, spec in out.items():
        T[k] = torch.empty((spec[1] + 3) // 4, device="cuda") if spec[0] == "ws" else torch.empty(spec[0], dtype=spec[1], device="cuda")
    for k, v in const.items():
        if callable(v):
            T[k] = v(T).clone()
    plain, _ = launch(T)
    torch.cuda.synchronize()
    for i, (a, p) in enumerate(zip(results["A"], plain)):
        if sparse:
            un = G._bits(a) == G._bits(torch.full((1,), G.fill_for(a.dtype, "A"), dtype=a.dtype, device=a.device))
            a, p = a[~un], p[~un]
        assert _same_bits(a, p), "%s: output %d differs from the plain call" % (name, i)
    if oracle is not None:                                                                            # (e)
        try:
            oracle(results["A"])
        except AssertionError as e:
            raise AssertionError("%s, against the oracle: %s" % (name, e)) from e
    return results["A"]


def _f64(a):
    return a.astype(np.float64)


def _st(a, dt):
    """A numpy activation in the storage type on the device (bf16: rounded as the oracle's operand rb(a) is)."""
    return dev(a) if dt == "f32" else dev(rb(a)).to(BF16)


def _ov(a, dt):
    """The oracle's view of an activation operand."""
    return _f64(a) if dt == "f32" else rb(a)


def _o(dt):
    return bops if dt == "bf16" else ops


def _close_act(dt):
    """The parity check of an output in the storage type: tests/test_gpu_kernels.py close (RTOL) / tests/test_gpu_bf16.py close_bf16."""
    return (lambda got, ref, name: close(got, ref, RTOL, name)) if dt == "f32" else (lambda got, ref, name: close_bf16(got, ref, name=name))


def _close_par(dt):
    """... of an fp32 parameter gradient: close (RTOL) / close_f32."""
    return (lambda got, ref, name: close(got, ref, RTOL, name)) if dt == "f32" else (lambda got, ref, name: close_f32(got, ref, name=name))


# ---------------------------------------------------------------------------------------------------------------- operands and oracles, once per grid
@functools.lru_cache(maxsize=None)
def _c64(dims):
    N, D, H, W = dims
    rng = np.random.default_rng(1000 * sum(dims) + W)
    act = lambda c=64: rng.normal(size=(N, D, H, W, c)).astype(np.float32)
    c = types.SimpleNamespace()
    c.x, c.res, c.y, c.skip = act(), act(), act(), act()
    c.dzs = [act() for _ in range(3)]
    c.ws = [(rng.normal(size=(3, 3, 3, 64, 64)) * 0.05).astype(np.float32) for _ in range(3)]
    c.b = rng.normal(size=64).astype(np.float32)
    for a in [c.x, c.res, c.y, c.skip, c.b] + c.dzs + c.ws:
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _fwd_ref(dims, dt, full):
    c = _c64(dims)
    w = _f64(c.ws[0]) if dt == "f32" else rb(c.ws[0])
    if full:
        return O.conv3d_fwd(_ov(c.x, dt), w, _f64(c.b), LEAKY, 0.2, _ov(c.res, dt))
    return O.conv3d_fwd(_ov(c.x, dt), w, None, NONE, 0.2, None)


@functools.lru_cache(maxsize=None)
def _dgrad_lin(dims, dt, s):
    """conv_T(dz_s, W_s) in float64."""
    c = _c64(dims)
    w = _f64(c.ws[s]) if dt == "f32" else rb(c.ws[s])
    return O.conv3d_dgrad(_ov(c.dzs[s], dt), w, tuple(dims) + (64,))


def _dgrad_ref(dims, dt, nsrc=1):
    c = _c64(dims)
    return O.act_bwd_from_output(sum(_dgrad_lin(dims, dt, s) for s in range(nsrc)) + _ov(c.skip, dt), _ov(c.y, dt), LEAKY)


@functools.lru_cache(maxsize=None)
def _wgrad_ref(dims, dt):
    c = _c64(dims)
    return O.conv3d_wgrad(_ov(c.x, dt), _ov(c.dzs[0], dt), 3), O.bias_grad(_ov(c.dzs[0], dt))


# ---------------------------------------------------------------------------------------------------------------- 64 -> 64 forward
def _fwd_case(o, dt, dims, algo_kw, tag):
    N, D, H, W = dims
    c = _c64(dims)
    check = _close_act(dt)
    for full in (True, False):                            # bias + residual + LeakyReLU present / all absent
        const = {"x": _st(c.x, dt), "w": dev(c.ws[0])}
        if full:
            const.update(bias=dev(c.b), res=_st(c.res, dt))
        can_mask = full and o.conv64_mask_ok(N, D, H, W, algo_kw.get("algo", ops.ALGO_AUTO))
        for with_mask in ([False, True] if can_mask else [False]):
            out = {"pack": ((o.PACK_ELEMS,), o.ACT_DTYPE), "y": ((N, D, H, W, 64), o.ACT_DTYPE)}
            if with_mask:
                out["mask"] = (tuple(o.new_sign_mask(const["x"]).shape), I16)

            def launch(T):
                o.pack_conv64_weights(T["w"], wp_fwd=T["pack"], want_dgrad=False)
                o.conv3d_fwd(T["x"], T["w"], T.get("bias"), LEAKY if full else NONE, 0.2, T.get("res"), wpack=T["pack"], out=T["y"],
                             mask=T.get("mask"), **algo_kw)
                return [T["y"]] + ([T["mask"]] if with_mask else []), []

            def oracle(wr):
                check(wr[0], _fwd_ref(dims, dt, full), "conv64 fwd")
                if with_mask:
                    assert torch.equal(wr[1].reshape(-1), sign_mask_words(wr[0], planar=dt == "f32").reshape(-1))
            run_guarded("conv64 fwd %s %s %s full=%d mask=%d" % (dt, dims, tag, full, with_mask), launch, const=const, out=out, oracle=oracle)


@pytest.mark.parametrize("algo", sorted(ALGOS))
@pytest.mark.parametrize("dims", GRIDS)
def test_conv64_fwd_f32(fdn, dims, algo):
    _fwd_case(ops, "f32", dims, {"algo": ALGOS[algo]}, algo)


@pytest.mark.parametrize("mt", BF_VARIANTS)
@pytest.mark.parametrize("dims", BF_GRIDS)
def test_conv64_fwd_bf16(fdn, dims, mt):
    with hooks(**bf_variant(mt)):
        _fwd_case(bops, "bf16", dims, {}, "variant %d" % mt)


# ---------------------------------------------------------------------------------------------------------------- 64 -> 64 input gradient
def _fused_dgrad_case(o, dt, dims, algo_kw, tag, forms):
    """forms: "y" (y_prev), "mask" (the sign mask instead), "parts" (shell and inner box as two calls)."""
    N, D, H, W = dims
    c = _c64(dims)
    y = _st(c.y, dt)
    for form in forms:
        const = {"dz": _st(c.dzs[0], dt), "w": dev(c.ws[0]), "skip": _st(c.skip, dt), "y": y}
        if form == "mask":
            const["mask"] = sign_mask_words(y, planar=dt == "f32")
        out = {"packs": ((2, o.PACK_ELEMS), o.ACT_DTYPE), "pad": ((N, D + 2, H + 2, W + 2, 64), F32), "out": ((N, D, H, W, 64), o.ACT_DTYPE)}

        def launch(T):
            o.pack_conv64_weights(T["w"], T["packs"][0], T["packs"][1])
            kw = dict(skip=T["skip"], y_prev=None if form == "mask" else T["y"], act=LEAKY, **algo_kw)
            if form == "parts":
                o.conv3d_dgrad_fused(T["dz"], T["packs"][1], T["pad"], T["out"], parts=ops.DGRAD_SHELL, **kw)
                o.conv3d_dgrad_fused(T["dz"], T["packs"][1], T["pad"], T["out"], parts=ops.DGRAD_INNER, **kw)
            else:
                o.conv3d_dgrad_fused(T["dz"], T["packs"][1], T["pad"], T["out"], mask=T.get("mask"), **kw)
            o.fold_halo_border([T["pad"]], T["out"], T["skip"], T["y"], LEAKY)
            return [T["out"]], []
        run_guarded("fused dgrad %s %s %s %s" % (dt, dims, tag, form), launch, const=const, out=out,
                    oracle=lambda wr: _close_act(dt)(wr[0], _dgrad_ref(dims, dt), "fused dgrad + border"))


@pytest.mark.parametrize("algo", sorted(ALGOS))
@pytest.mark.parametrize("dims", GRIDS)
def test_conv64_dgrad_fused_f32(fdn, dims, algo):
    A = ALGOS[algo]
    forms = ["y", "parts"] + (["mask"] if ops.conv64_mask_ok(*dims, A) else [])
    _fused_dgrad_case(ops, "f32", dims, {"algo": A}, algo, forms)


@pytest.mark.parametrize("mt", BF_VARIANTS)
@pytest.mark.parametrize("dims", BF_GRIDS)
def test_conv64_dgrad_fused_bf16(fdn, dims, mt):
    with hooks(**bf_variant(mt)):
        _fused_dgrad_case(bops, "bf16", dims, {}, "variant %d" % mt, ["y", "mask"])


def _multi_case(o, dt, dims, nsrc, algo_kw, tag):
    N, D, H, W = dims
    c = _c64(dims)
    y = _st(c.y, dt)
    for form in ("y", "mask"):
        const = {"skip": _st(c.skip, dt), "y": y}
        for s in range(nsrc):
            const["dz%d" % s], const["w%d" % s] = _st(c.dzs[s], dt), dev(c.ws[s])
        if form == "mask":
            const["mask"] = sign_mask_words(y, planar=dt == "f32")
        out = {"packs": ((nsrc, 2, o.PACK_ELEMS), o.ACT_DTYPE), "pad": ((N, D + 2, H + 2, W + 2, 64), F32), "out": ((N, D, H, W, 64), o.ACT_DTYPE)}

        def launch(T):
            for s in range(nsrc):                         # one batched pack buffer: the last dgrad pack ends where the band begins
                o.pack_conv64_weights(T["w%d" % s], T["packs"][s, 0], T["packs"][s, 1])
            o.conv3d_dgrad_fused_multi([T["dz%d" % s] for s in range(nsrc)], [T["packs"][s, 1] for s in range(nsrc)], T["pad"], T["out"],
                                       skip=T["skip"], y_prev=None if form == "mask" else T["y"], act=LEAKY, mask=T.get("mask"), **algo_kw)
            o.fold_halo_border([T["pad"]], T["out"], T["skip"], T["y"], LEAKY)
            return [T["out"]], []
        run_guarded("multi-source fused dgrad %s %s %s n=%d %s" % (dt, dims, tag, nsrc, form), launch, const=const, out=out,
                    oracle=lambda wr: _close_act(dt)(wr[0], _dgrad_ref(dims, dt, nsrc), "multi-source fused dgrad + border"))


@pytest.mark.parametrize("nsrc", [2, 3])
@pytest.mark.parametrize("algo", ["auto", "bf16x3"])
@pytest.mark.parametrize("dims", [d for d in GRIDS if d[2] % 4 == 0 and d[3] % 4 == 0] + [(3, 4, 4, 4)])
def test_conv64_dgrad_fused_multi_f32(fdn, dims, algo, nsrc):
    """Only where conv64_mask_ok: the F(4,3) x F(4,3) grids of the set, (1,1,4,4) and (1,7,12,20), and with them (3,4,4,4) of
    tests/test_gpu_kernels.py, so that this family has a grid whose samples border each other too."""
    assert ops.conv64_mask_ok(*dims, ops.ALGO_AUTO)
    if not ops.conv64_mask_ok(*dims, ALGOS[algo]):        # bf16x3: the inner box is a launch of its own, the call must refuse (test_gpu_pow2_scaling.py)
        c = _c64(dims)
        N, D, H, W = dims
        packs = torch.empty((nsrc, 2, ops.PACK_ELEMS), device="cuda")
        with pytest.raises(_lib.FdnError):
            ops.conv3d_dgrad_fused_multi([dev(c.dzs[s]) for s in range(nsrc)], [packs[s, 1] for s in range(nsrc)],
                                         torch.empty((N, D + 2, H + 2, W + 2, 64), device="cuda"), torch.empty((N, D, H, W, 64), device="cuda"),
                                         skip=dev(c.skip), y_prev=dev(c.y), act=LEAKY, algo=ALGOS[algo])
        return
    _multi_case(ops, "f32", dims, nsrc, {"algo": ALGOS[algo]}, algo)


@pytest.mark.parametrize("nsrc", [2, 3])
@pytest.mark.parametrize("mt", BF_VARIANTS)
@pytest.mark.parametrize("dims", BF_GRIDS)
def test_conv64_dgrad_fused_multi_bf16(fdn, dims, mt, nsrc):
    with hooks(**bf_variant(mt)):
        _multi_case(bops, "bf16", dims, nsrc, {}, "variant %d" % mt)


@pytest.mark.parametrize("nsrc", [1, 3])
@pytest.mark.parametrize("algo", ["auto", "direct"])
@pytest.mark.parametrize("dims", GRIDS)
def test_conv3d_dgrad_then_fold_halo(fdn, dims, algo, nsrc):
    """The older path (fp32 only): the gradient on the padded grid, every element of it written, then the whole-grid fold of 1 or 3 sources."""
    N, D, H, W = dims
    c = _c64(dims)
    const = {"w": dev(c.ws[0]), "skip": dev(c.skip), "y": dev(c.y)}
    out = {"packs": ((2, ops.PACK_ELEMS), F32), "out": ((N, D, H, W, 64), F32)}
    for k in range(nsrc):
        const["dz%d" % k] = dev(c.dzs[k])
        out["pad%d" % k] = ((N, D + 2, H + 2, W + 2, 64), F32)

    def launch(T):
        ops.pack_conv64_weights(T["w"], T["packs"][0], T["packs"][1])
        pads = [ops.conv3d_dgrad(T["dz%d" % k], T["w"], wpack_dgrad=T["packs"][1], out=T["pad%d" % k], algo=ALGOS[algo]) for k in range(nsrc)]
        ops.fold_halo(pads, T["skip"], T["y"], LEAKY, 0.2, out=T["out"])
        return [T["out"]] + pads, []

    def oracle(wr):
        lin = O.conv3d_dgrad(sum(_f64(c.dzs[k]) for k in range(nsrc)), _f64(c.ws[0]), (N, D, H, W, 64)) if nsrc > 1 else _dgrad_lin(dims, "f32", 0)
        close(wr[0], O.act_bwd_from_output(lin + _f64(c.skip), _f64(c.y), LEAKY), name="dgrad + fold_halo")
    run_guarded("dgrad + fold_halo %s %s n=%d" % (dims, algo, nsrc), launch, const=const, out=out, oracle=oracle)


# ---------------------------------------------------------------------------------------------------------------- 64 -> 64 weight gradient
def _wgrad_case(o, dt, dims, tag, algo_kw):
    c = _c64(dims)
    nbytes = o.wgrad_workspace_bytes(*dims, 64, 64, 3)
    assert nbytes > 0
    const = {"x": _st(c.x, dt), "dz": _st(c.dzs[0], dt)}
    for want_bias in (True, False):
        out = {"dw": ((3, 3, 3, 64, 64), F32), "ws": ("ws", nbytes)}
        if want_bias:
            out["db"] = ((64,), F32)

        def launch(T):
            o.conv3d_wgrad(T["x"], T["dz"], 3, 64, 64, want_bias=want_bias, dw=T["dw"], dbias=T.get("db"), workspace=T["ws"], **algo_kw)
            return [T["dw"]] + ([T["db"]] if want_bias else []), []

        def oracle(wr):
            ref_w, ref_b = _wgrad_ref(dims, dt)
            _close_par(dt)(wr[0], ref_w, "wgrad64")
            if want_bias:
                _close_par(dt)(wr[1], ref_b, "bias grad 64")
        run_guarded("wgrad64 %s %s %s bias=%d" % (dt, dims, tag, want_bias), launch, const=const, out=out, oracle=oracle)


@pytest.mark.parametrize("algo", ["auto", "direct", "wino_w"])
@pytest.mark.parametrize("dims", GRIDS)
def test_conv64_wgrad_f32(fdn, dims, algo):
    with hooks(**({"wgrad64_direct": 1} if algo == "direct" else {})):         # the direct kernel is a test-build route (tests/test_gpu_kernels.py)
        _wgrad_case(ops, "f32", dims, algo, {"algo": ops.ALGO_WINO_W if algo == "wino_w" else ops.ALGO_AUTO})


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dims", BF_GRIDS)
def test_conv64_wgrad_bf16(fdn, dims, variant):
    with hooks(**({"wgrad64_bf16_variant": 1} if variant else {})):
        _wgrad_case(bops, "bf16", dims, "variant %d" % variant, {})


@pytest.mark.parametrize("dt,dims,nl", [("f32", (2, 6, 6, 8), 2), ("f32", (2, 6, 6, 8), 3), ("f32", (2, 6, 6, 8), 11), ("f32", (1, 7, 6, 8), 3),
                                        ("bf16", (2, 6, 6, 8), 2), ("bf16", (2, 6, 6, 8), 9)])
def test_conv64_wgrad_batch(fdn, dt, dims, nl):
    """11 fp32 layers go out in chunks, (1,7,6,8) (odd D) layer by layer; bias gradients for every other layer; the workspace has exactly
    fdn_conv3d_wgrad[_bf16]_batch_workspace_bytes bytes."""
    o = _o(dt)
    N, D, H, W = dims
    rng = np.random.default_rng(nl * 1000 + D)
    xs = [rng.normal(size=(N, D, H, W, 64)).astype(np.float32) for _ in range(nl)]
    dzs = [rng.normal(size=(N, D, H, W, 64)).astype(np.float32) for _ in range(nl)]
    nbytes = o.wgrad_batch_workspace_bytes(nl, N, D, H, W)
    assert nbytes > 0
    const, out = {}, {"ws": ("ws", nbytes)}
    for i in range(nl):
        const["x%d" % i], const["dz%d" % i] = _st(xs[i], dt), _st(dzs[i], dt)
        out["dw%d" % i] = ((3, 3, 3, 64, 64), F32)
        if i % 2 == 0:
            out["db%d" % i] = ((64,), F32)

    def launch(T):
        o.conv3d_wgrad_batch([T["x%d" % i] for i in range(nl)], [T["dz%d" % i] for i in range(nl)], [T["dw%d" % i] for i in range(nl)],
                             [T.get("db%d" % i) for i in range(nl)], workspace=T["ws"])
        return [T["dw%d" % i] for i in range(nl)] + [T["db%d" % i] for i in range(0, nl, 2)], []

    def oracle(wr):
        for i in (0, nl - 1):                             # tests/test_gpu_kernels.py test_conv64_wgrad_batch: first and last layer
            _close_par(dt)(wr[i], O.conv3d_wgrad(_ov(xs[i], dt), _ov(dzs[i], dt), 3), "batched wgrad layer %d" % i)
        for j, i in enumerate(range(0, nl, 2)):
            _close_par(dt)(wr[nl + j], O.bias_grad(_ov(dzs[i], dt)), "batched bias grad layer %d" % i)
    run_guarded("batched wgrad64 %s %s %d layers" % (dt, dims, nl), launch, const=const, out=out, oracle=oracle)


# ---------------------------------------------------------------------------------------------------------------- thin layers
@functools.lru_cache(maxsize=None)
def _thin(dims):
    N, D, H, W = dims
    rng = np.random.default_rng(4000 + 100 * sum(dims) + W)
    t = types.SimpleNamespace()
    act = lambda ch: rng.normal(size=(N, D, H, W, ch)).astype(np.float32)
    t.x3, t.x, t.xb, t.dz, t.dpred, t.y = act(3), act(64), act(64), act(64), act(3), act(64)
    t.w3 = (rng.normal(size=(3, 3, 3, 3, 64)) * 0.2).astype(np.float32)
    t.w1 = (rng.normal(size=(3, 3, 3, 64, 1)) * 0.1).astype(np.float32)
    t.wk = (rng.normal(size=(1, 1, 1, 128, 64)) * 0.1).astype(np.float32)
    t.b, t.b1 = rng.normal(size=64).astype(np.float32), rng.normal(size=1).astype(np.float32)
    return t


@functools.lru_cache(maxsize=None)
def _thin_refs(dims, dt):
    t = _thin(dims)
    v = lambda a: _ov(a, dt)
    r = types.SimpleNamespace()
    dzo = _f64(t.dpred[..., 1:2])
    cat = np.concatenate([v(t.x), v(t.xb)], -1)
    r.fwd3 = O.conv3d_fwd(v(t.x3), _f64(t.w3), _f64(t.b), RELU)
    r.dw3, r.db = O.conv3d_wgrad(v(t.x3), v(t.dz), 3), O.bias_grad(v(t.dz))
    r.fwd1 = O.conv3d_fwd(v(t.x), _f64(t.w1), _f64(t.b1))
    r.dw1, r.db1 = O.conv3d_wgrad(v(t.x), dzo, 3), O.bias_grad(dzo)
    r.dx1 = O.act_bwd_from_output(O.conv3d_dgrad(dzo, _f64(t.w1), t.x.shape), v(t.y), LEAKY)
    r.fwdk = O.conv3d_fwd(cat, _f64(t.wk), _f64(t.b), RELU)
    dcat = O.conv3d_dgrad(v(t.dz), _f64(t.wk), cat.shape)
    r.dxa, r.dxb = dcat[..., :64] * (v(t.x) > 0), dcat[..., 64:] * (v(t.xb) > 0)
    r.dwk = O.conv3d_wgrad(cat, v(t.dz), 1)
    return r


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_cin3_layers(fdn, dt, dims, mfma):
    """3 -> 64 forward and weight gradient (workspace of exactly fdn_conv3d_wgrad[_bf16]_workspace_bytes(.., 3, 64, 3))."""
    o, t, r = _o(dt), _thin(dims), _thin_refs(dims, dt)
    N, D, H, W = dims
    with hooks(**({} if mfma else {"cin3_mfma": 0})):
        def fwd(T):
            o.conv3d_fwd(T["x"], T["w"], T["b"], RELU, out=T["y"])
            return [T["y"]], []
        run_guarded("3->64 fwd %s %s mfma=%d" % (dt, dims, mfma), fwd, const={"x": _st(t.x3, dt), "w": dev(t.w3), "b": dev(t.b)},
                    out={"y": ((N, D, H, W, 64), o.ACT_DTYPE)}, oracle=lambda wr: _close_act(dt)(wr[0], r.fwd3, "3->64 fwd"))

        def wgrad(T):
            o.conv3d_wgrad(T["x"], T["dz"], 3, 3, 64, want_bias=True, dw=T["dw"], dbias=T["db"], workspace=T["ws"])
            return [T["dw"], T["db"]], []

        def oracle(wr):
            _close_par(dt)(wr[0], r.dw3, "3->64 wgrad")
            _close_par(dt)(wr[1], r.db, "3->64 bias grad")
        run_guarded("3->64 wgrad %s %s mfma=%d" % (dt, dims, mfma), wgrad, const={"x": _st(t.x3, dt), "dz": _st(t.dz, dt)},
                    out={"dw": ((3, 3, 3, 3, 64), F32), "db": ((64,), F32), "ws": ("ws", o.wgrad_workspace_bytes(N, D, H, W, 3, 64, 3))}, oracle=oracle)


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_head_layers(fdn, dt, dims, mfma):
    """64 -> 1: forward into channel 1 of an (N,V,3) prediction (channels 0 and 2 keep the prefill), weight and bias gradient read through
    lddz = 3 / dz_coff = 1, and conv_cout1_dgrad_folded with dbias_prev and a workspace of exactly 2048 * 64 * 4 bytes, plus its mask form."""
    o, t, r = _o(dt), _thin(dims), _thin_refs(dims, dt)
    N, D, H, W = dims
    with hooks(**({} if mfma else {"heads_mfma": 0})):
        def fwd(T):
            o.conv3d_fwd(T["x"], T["w"], T["b"], NONE, out=T["pred"], ldy=3, y_coff=1)
            return [T["pred"][..., 1]], [T["pred"][..., 0], T["pred"][..., 2]]
        run_guarded("64->1 fwd %s %s mfma=%d" % (dt, dims, mfma), fwd, const={"x": _st(t.x, dt), "w": dev(t.w1), "b": dev(t.b1)},
                    out={"pred": ((N, D, H, W, 3), F32)}, oracle=lambda wr: _close_par(dt)(wr[0], r.fwd1[..., 0], "64->1 fwd"))

        def wgrad(T):
            o.conv3d_wgrad(T["x"], T["dpred"], 3, 64, 1, want_bias=True, dw=T["dw"], dbias=T["db"], workspace=T["ws"], lddz=3, dz_coff=1)
            return [T["dw"], T["db"]], []

        def oracle_w(wr):
            _close_par(dt)(wr[0], r.dw1, "64->1 wgrad")
            _close_par(dt)(wr[1], r.db1, "64->1 bias grad")
        run_guarded("64->1 wgrad %s %s mfma=%d" % (dt, dims, mfma), wgrad, const={"x": _st(t.x, dt), "dpred": dev(t.dpred)},
                    out={"dw": ((3, 3, 3, 64, 1), F32), "db": ((1,), F32), "ws": ("ws", o.wgrad_workspace_bytes(N, D, H, W, 64, 1, 3))}, oracle=oracle_w)

        y = _st(t.y, dt)
        forms = ["y"] + (["mask"] if mfma and (dt == "bf16" or W % 4 == 0) else [])       # tests/test_gpu_pow2_scaling.py: where the mask form exists
        for form in forms:
            const = {"dpred": dev(t.dpred), "w": dev(t.w1)}
            const["mask" if form == "mask" else "y"] = sign_mask_words(y, planar=dt == "f32") if form == "mask" else y

            def dgrad(T):
                o.conv_cout1_dgrad_folded(T["dpred"], T["w"], dims, T.get("y"), LEAKY, 0.2, lddz=3, dz_coff=1, out=T["out"], dbias_prev=T["db"],
                                          workspace=T["ws"], mask=T.get("mask"))
                return [T["out"], T["db"]], []

            def oracle_d(wr):
                _close_act(dt)(wr[0], r.dx1, "64->1 dgrad folded")
                if dt == "f32":
                    close(wr[1], O.bias_grad(r.dx1), name="64->1 dgrad folded: fused bias grad")
                else:                                     # tests/test_gpu_bf16.py: the sum of the unrounded fp32 values
                    close_f32(wr[1], O.bias_grad(r.dx1), tol=3e-3, name="fused bias grad")
            run_guarded("64->1 dgrad folded %s %s mfma=%d %s" % (dt, dims, mfma, form), dgrad, const=const,
                        out={"out": ((N, D, H, W, 64), o.ACT_DTYPE), "db": ((64,), F32), "ws": ("ws", HEAD_WS_BYTES)}, oracle=oracle_d)


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("dt,dims", DT_GRIDS)
def test_conv1x1_layers(fdn, dt, dims, mfma):
    """1x1 (64 + 64) -> 64: forward with x2, conv1x1_dgrad, weight gradient (workspace of exactly ..._workspace_bytes(.., 128, 64, 1))."""
    o, t, r = _o(dt), _thin(dims), _thin_refs(dims, dt)
    N, D, H, W = dims
    act_shape = ((N, D, H, W, 64), o.ACT_DTYPE)
    with hooks(**({} if mfma else {"conv1x1_mfma": 0})):
        def fwd(T):
            o.conv3d_fwd(T["xa"], T["w"], T["b"], RELU, x2=T["xb"], out=T["y"])
            return [T["y"]], []
        run_guarded("1x1 fwd %s %s mfma=%d" % (dt, dims, mfma), fwd, const={"xa": _st(t.x, dt), "xb": _st(t.xb, dt), "w": dev(t.wk), "b": dev(t.b)},
                    out={"y": act_shape}, oracle=lambda wr: _close_act(dt)(wr[0], r.fwdk, "1x1 fwd"))

        def dgrad(T):
            o.conv1x1_dgrad(T["dz"], T["w"], T["ya"], T["yb"], T["dxa"], T["dxb"])
            return [T["dxa"], T["dxb"]], []

        def oracle_d(wr):
            _close_act(dt)(wr[0], r.dxa, "1x1 dgrad a")
            _close_act(dt)(wr[1], r.dxb, "1x1 dgrad b")
        run_guarded("1x1 dgrad %s %s mfma=%d" % (dt, dims, mfma), dgrad, const={"dz": _st(t.dz, dt), "w": dev(t.wk), "ya": _st(t.x, dt), "yb": _st(t.xb, dt)},
                    out={"dxa": act_shape, "dxb": act_shape}, oracle=oracle_d)

        def wgrad(T):
            o.conv3d_wgrad(T["xa"], T["dz"], 1, 128, 64, x2=T["xb"], want_bias=True, dw=T["dw"], dbias=T["db"], workspace=T["ws"])
            return [T["dw"], T["db"]], []

        def oracle_w(wr):
            _close_par(dt)(wr[0], r.dwk, "1x1 wgrad")
            _close_par(dt)(wr[1], r.db, "1x1 bias grad")
        run_guarded("1x1 wgrad %s %s mfma=%d" % (dt, dims, mfma), wgrad, const={"xa": _st(t.x, dt), "xb": _st(t.xb, dt), "dz": _st(t.dz, dt)},
                    out={"dw": ((1, 1, 1, 128, 64), F32), "db": ((64,), F32), "ws": ("ws", o.wgrad_workspace_bytes(N, D, H, W, 128, 64, 1))}, oracle=oracle_w)


# ---------------------------------------------------------------------------------------------------------------- trilinear upsampling
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("dims,R", [((1, 3, 7, 5), 2), ((2, 1, 5, 4), 3), ((1, 4, 1, 3), 2)])
def test_upsample(fdn, dims, R, dt):
    """Forward, and backward with y_prev / LeakyReLU (odd H leaves a one-row block whose tail re-reads a row, an axis of length 1 takes every
    high-res row: tests/test_gpu_kernels.py test_upsample_bwd_row_blocks)."""
    o = _o(dt)
    N, D, H, W = dims
    rng = np.random.default_rng(15 + R + sum(dims))
    x, y = rng.normal(size=(N, D, H, W, 64)).astype(np.float32), rng.normal(size=(N, D, H, W, 64)).astype(np.float32)
    dy = rng.normal(size=(N, D * R, H * R, W * R, 64)).astype(np.float32)

    def fwd(T):
        o.upsample_trilinear_fwd(T["x"], R, out=T["up"])
        return [T["up"]], []
    run_guarded("upsample fwd %s %s R=%d" % (dt, dims, R), fwd, const={"x": _st(x, dt)}, out={"up": (dy.shape, o.ACT_DTYPE)},
                oracle=lambda wr: _close_act(dt)(wr[0], O.upsample_trilinear_fwd(_ov(x, dt), R, f32_coeffs=True), "upsample fwd"))

    def bwd(T):
        o.upsample_trilinear_bwd(T["dy"], R, T["y"], LEAKY, 0.2, out=T["dx"])
        return [T["dx"]], []
    ref = O.act_bwd_from_output(O.upsample_trilinear_bwd(_ov(dy, dt), (D, H, W), R, f32_coeffs=True), _ov(y, dt), LEAKY)
    run_guarded("upsample bwd %s %s R=%d" % (dt, dims, R), bwd, const={"dy": _st(dy, dt), "y": _st(y, dt)}, out={"dx": (x.shape, o.ACT_DTYPE)},
                oracle=lambda wr: _close_act(dt)(wr[0], ref, "upsample bwd+mask"))


# ---------------------------------------------------------------------------------------------------------------- input features
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("nvox", [1, 255, 257])
def test_input_features(fdn, nvox, dt):
    o = _o(dt)
    batch = O.synthetic_batch(2, 6, 2, seed=11)
    ins = [np.ascontiguousarray(a.reshape(-1)[:nvox]) for a in batch[:6]]
    ref = O.input_features(*[_f64(a)[:, None] for a in ins])
    names = ("u", "v", "w", "mu", "mv", "mw")

    def launch(T):
        o.input_features(*[T[n] for n in names], phase=T["phase"], pc=T["pc"])
        return [T["phase"], T["pc"]], []

    def oracle(wr):
        _close_act(dt)(wr[0], ref[0], "phase")
        _close_act(dt)(wr[1], ref[1], "pc")
    run_guarded("input_features %s n=%d" % (dt, nvox), launch, const={n: dev(a) for n, a in zip(names, ins)},
                out={"phase": ((nvox, 3), o.ACT_DTYPE), "pc": ((nvox, 3), o.ACT_DTYPE)}, oracle=oracle)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("orientation", [None, (1, 1), (3, 3)])
@pytest.mark.parametrize("P,R,shape", [(8, 2, (7, 10, 13)), (8, 2, (4, 4, 4))])          # the two smallest CASES of tests/test_gpu_device_tiler.py
def test_input_features_volume(fdn, P, R, shape, orientation, dt):
    """The frames guarded; all patches, and the first and the last patch of the last frame alone: those windows overhang the volume on
    every side (the source coordinate is the patch coordinate - 2, the far patch ends in the pad)."""
    from test_gpu_device_tiler import F, _frames_and_host_patches
    o = _o(dt)
    frames, stacks, counts, _ = _frames_and_host_patches(P, R, shape)
    n = counts[0] * counts[1] * counts[2]
    flat = [s[..., 0] for s in stacks]
    if orientation is not None:
        flat = list(se.forward(flat[:3], orientation, True, lead=1)) + list(se.forward(flat[3:], orientation, False, lead=1))
    ref = O.input_features(*[_f64(np.asarray(a))[..., None] for a in flat])
    for g0, count in ((0, F * n), ((F - 1) * n, 1), (F * n - 1, 1)):
        def launch(T):
            o.input_features_volume(T["frames"], P, counts, g0, count, phase=T["phase"], pc=T["pc"], orientation=orientation)
            return [T["phase"], T["pc"]], []

        def oracle(wr):
            _close_act(dt)(wr[0], ref[0][g0:g0 + count], "phase")
            _close_act(dt)(wr[1], ref[1][g0:g0 + count], "pc")
        spec = ((count, P, P, P, 3), o.ACT_DTYPE)
        run_guarded("input_features_volume %s %s %s %s [%d,+%d)" % (dt, P, shape, orientation, g0, count), launch,
                    const={"frames": torch.tensor(frames, device="cuda")}, out={"phase": spec, "pc": spec}, oracle=oracle)


# ---------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("div_weight", [0.0, 0.8])
@pytest.mark.parametrize("shape", [(1, 1, 4, 5), (2, 3, 2, 7), (3, 5, 7, 9)])
def test_loss_metrics(fdn, shape, div_weight, want_grad):
    """A binary mask: the fp32 atomic mask count of mask_sums_kernel is exact for integer sums only.  Scratch of exactly N (8 + 3 * 256) /
    N (8 + 5 * 256) floats.  Tolerances per column: tests/test_gpu_kernels.py test_input_features_loss_metric (plain) and
    tests/test_gpu_divergence_loss.py test_kernel_matches_float64 (div_weight)."""
    N = shape[0]
    pred, truth, mask = make_case(shape, "binary", seed=sum(shape) + 6)
    cols = 5 if div_weight else 4
    const = {"pred": dev(pred), "uh": dev(truth[0]), "vh": dev(truth[1]), "wh": dev(truth[2]), "mask": dev(mask)}
    out = {"out": ((N, cols), F32), "scratch": ((N * (8 + (5 if div_weight else 3) * 256),), F32)}
    if want_grad:
        out["dpred"] = (pred.shape, F32)

    def launch(T):
        ops.loss_metrics(T["pred"], T["uh"], T["vh"], T["wh"], T["mask"], want_grad=want_grad, out=T["out"], dpred=T.get("dpred"),
                         scratch=T["scratch"], div_weight=div_weight)
        return [T["out"]] + ([T["dpred"]] if want_grad else []), []

    def oracle(wr):
        got = wr[0].cpu().numpy().astype(np.float64)
        hires = np.stack(truth, -1).astype(np.float64)
        mse, dp = O.masked_mse_loss_fwd_bwd(_f64(pred), hires, _f64(mask))
        tol = 1e-5 if div_weight else RTOL                 # sum mask and dpred: 1e-5 in the divergence test, close()'s RTOL in the plain one
        assert rel_err(got[:, 0], mse) <= 1e-5
        assert rel_err(got[:, 1], O.relative_error(pred, hires.astype(np.float32), mask)) <= 2e-3
        assert rel_err(got[:, 2], _f64(mask).sum((1, 2, 3))) <= tol
        if div_weight:
            div_b, dp_div = divergence_loss(pred, hires, mask, div_weight)
            assert rel_err(got[:, 3], (mask < 0.5).sum((1, 2, 3))) <= 1e-5
            assert rel_err(got[:, 4], div_b) <= 1e-5
            dp = dp + dp_div
        if want_grad:
            assert rel_err(wr[1].cpu().numpy(), dp) <= tol
    run_guarded("loss_metrics %s div=%g grad=%d" % (shape, div_weight, want_grad), launch, const=const, out=out, oracle=oracle)


# ---------------------------------------------------------------------------------------------------------------- optimiser kernels
ADAM_N = [1, 255, 257, 100003]
B1, B2, EPS, LR, L2S = 0.9, 0.999, 1e-7, 1e-3, 8 * 2 * O.L2_LAMBDA


@functools.lru_cache(maxsize=None)
def _adam_operands(n):
    rng = np.random.default_rng(13 + n)
    a = types.SimpleNamespace()
    a.w, a.g = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    a.m, a.v = (rng.normal(size=n) * 0.1).astype(np.float32), (rng.uniform(size=n) * 0.1).astype(np.float32)
    a.isk, a.frozen = (rng.uniform(size=n) < 0.8).astype(np.uint8), (rng.uniform(size=n) < 0.3).astype(np.uint8)
    a.ema = rng.normal(size=n).astype(np.float32)
    return a


def _adam_ref(a, t=3, g_scale=None, clip_value=None, frozen=False):
    """One Keras Adam step in float64 on the step's gradient g + l2s w (kernels), scaled or clamped; frozen elements keep w, m, v."""
    w, m, v = _f64(a.w), _f64(a.m), _f64(a.v)
    gp = _f64(a.g) + L2S * w * a.isk
    if g_scale is not None:
        gp = gp * g_scale
    if clip_value is not None:
        gp = np.clip(gp, -clip_value, clip_value)
    w1, m1, v1 = w.copy(), m.copy(), v.copy()
    O.adam_step_tf(w1, gp, m1, v1, t, LR, B1, B2, EPS)
    if frozen:
        live = a.frozen == 0
        w1, m1, v1 = np.where(live, w1, w), np.where(live, m1, m), np.where(live, v1, v)
    return w1, m1, v1


ADAM_FORMS = ["plain", "sumsq", "lr_dev", "frozen", "g_scale", "clip_value", "ema", "ema_init_frozen"]


@pytest.mark.parametrize("form", ADAM_FORMS)
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step(fdn, n, form):
    """Every route of ops.adam_step; the partials buffer has exactly ADAM_PARTIALS floats, device scalars are one guarded float each.
    Against Keras Adam in float64 at the tolerances of tests/test_gpu_kernels.py test_adam_and_l2 (w 5e-5, m 1e-5, v 5e-5: (1 - b2) is
    evaluated in fp32); the average against tests/_ema_ref.py within its bound."""
    import _ema_ref as E
    a = _adam_operands(n)
    t = 3
    lr_t = LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    const = {"g": dev(a.g), "isk": torch.from_numpy(a.isk).cuda()}
    inout = {"w": dev(a.w), "m": dev(a.m), "v": dev(a.v)}
    out, kw, ref_kw = {}, {}, {}
    mom = 0.99
    if form in ("sumsq", "ema"):
        out["part"] = ((ops.ADAM_PARTIALS,), F32)
    if form == "lr_dev":
        const["lr"] = torch.tensor([lr_t], dtype=F32, device="cuda")
    if form in ("frozen", "ema_init_frozen"):
        const["frozen"] = torch.from_numpy(a.frozen).cuda()
        ref_kw["frozen"] = True
    if form == "g_scale":
        const["gs"] = torch.tensor([0.37], dtype=F32, device="cuda")
        ref_kw["g_scale"] = float(np.float32(0.37))
    if form == "clip_value":
        kw["clip_value"], ref_kw["clip_value"] = 0.5, 0.5
    if form.startswith("ema"):
        inout["ema"] = dev(a.ema)
        kw.update(ema_momentum=mom, ema_init=form != "ema")

    def launch(T):
        ops.adam_step(T["w"], T["g"], T["m"], T["v"], T["isk"], lr_t, B1, B2, EPS, L2S, sumsq_partials=T.get("part"), lr_t_dev=T.get("lr"),
                      frozen=T.get("frozen"), g_scale_dev=T.get("gs"), ema=T.get("ema"), **kw)
        return [T["w"], T["m"], T["v"]] + ([T["part"]] if "part" in T else []) + ([T["ema"]] if "ema" in T else []), []

    def oracle(wr):
        w1, m1, v1 = _adam_ref(a, t, **ref_kw)
        close(wr[0], w1, tol=5e-5, name="adam w"); close(wr[1], m1, tol=1e-5, name="adam m"); close(wr[2], v1, tol=5e-5, name="adam v")
        w_after = wr[0].cpu().numpy()
        if "part" in out:                                 # sum of the updated kernel parameters' squares (test_adam_and_l2: 1e-6 against fdn_l2_sumsq)
            close(ops.sum_partials(wr[3]), [float((_f64(w_after)[a.isk != 0] ** 2).sum())], tol=1e-5, name="adam sumsq partials")
        if form.startswith("ema"):
            want = E.ema_step(a.ema, a.w, w_after, mom, init=form != "ema", frozen=a.frozen if form == "ema_init_frozen" else None)
            err = np.abs(wr[-1].cpu().numpy().astype(np.float64) - want)
            assert (err <= E.ema_bound([a.w, w_after] + ([] if form != "ema" else [a.ema]), [want])).all(), err.max()
    run_guarded("adam_step %s n=%d" % (form, n), launch, const=const, inout=inout, out=out, oracle=oracle)


@pytest.mark.parametrize("n", ADAM_N)
def test_sumsq_and_clip_kernels(fdn, n):
    """l2_sumsq, l2_sumsq_partials, grad_sumsq_partials (with l2_scale_dev and frozen), sum_partials and clip_scale; partials of exactly
    ADAM_PARTIALS floats, `out` of exactly 1 / 2 floats.  Float64 sums at the 1e-5 of tests/test_gpu_kernels.py test_adam_and_l2."""
    a = _adam_operands(n)
    w, g, isk, frozen = dev(a.w), dev(a.g), torch.from_numpy(a.isk).cuda(), torch.from_numpy(a.frozen).cuda()
    ksum = float((_f64(a.w)[a.isk != 0] ** 2).sum())

    def l2(T):
        ops.l2_sumsq(T["w"], T["isk"], out=T["out"])
        return [T["out"]], []
    run_guarded("l2_sumsq n=%d" % n, l2, const={"w": w, "isk": isk}, out={"out": ((1,), F32)},
                oracle=lambda wr: close(wr[0], [ksum], tol=1e-5, name="l2 sumsq"))

    def l2p(T):
        ops.l2_sumsq_partials(T["w"], T["isk"], T["part"])
        ops.sum_partials(T["part"], out=T["out"])
        return [T["part"], T["out"]], []
    run_guarded("l2_sumsq_partials + sum_partials n=%d" % n, l2p, const={"w": w, "isk": isk}, out={"part": ((ops.ADAM_PARTIALS,), F32), "out": ((1,), F32)},
                oracle=lambda wr: close(wr[1], [ksum], tol=1e-5, name="l2 sumsq partials"))

    l2g, slot, clip = 2 * O.L2_LAMBDA, 8.0, 0.5
    gp = np.where(a.frozen == 0, _f64(a.g) + float(np.float32(l2g) * np.float32(slot)) * _f64(a.w) * a.isk, 0.0)
    norm = float(np.sqrt((gp ** 2).sum()))

    def gs(T):
        ops.grad_sumsq_partials(T["g"], T["w"], T["isk"], l2g, T["slot"], partials=T["part"], frozen=T["frozen"])
        ops.clip_scale(T["part"], clip, out=T["out"])
        return [T["part"], T["out"]], []

    def oracle(wr):
        close(wr[1][:1], [norm], tol=1e-5, name="global norm")
        close(wr[1][1:], [clip / max(norm, clip)], tol=1e-5, name="clip scale")
    run_guarded("grad_sumsq_partials + clip_scale n=%d" % n, gs,
                const={"g": g, "w": w, "isk": isk, "frozen": frozen, "slot": torch.tensor([slot], dtype=F32, device="cuda")},
                out={"part": ((ops.ADAM_PARTIALS,), F32), "out": ((2,), F32)}, oracle=oracle)


# ---------------------------------------------------------------------------------------------------------------- packs
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pack_conv64_weights(fdn, dt):
    """Both packs of one layer.  A pack may hold slots no kernel reads and the pack kernel does not write (sparse): what is written is the
    same under both fills and equals the plain call.  There is no float64 oracle of a pack; every conv case above reads a guarded one."""
    o = _o(dt)
    w = dev(_c64((1, 1, 4, 4)).ws[0])

    def launch(T):
        o.pack_conv64_weights(T["w"], T["fwd"], T["dgrad"])
        return [T["fwd"], T["dgrad"]], []
    run_guarded("pack_conv64_weights %s" % dt, launch, const={"w": w}, out={"fwd": ((o.PACK_ELEMS,), o.ACT_DTYPE), "dgrad": ((o.PACK_ELEMS,), o.ACT_DTYPE)},
                sparse=True)


@pytest.mark.parametrize("streams", [None, (ops.PACK_STREAM_WINO_H4, ops.PACK_STREAM_DIRECT | ops.PACK_STREAM_WINO_W)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pack_conv64_weights_batch(fdn, dt, streams):
    """Three layers out of a guarded flat parameter buffer whose last layer ends where the band begins; the offsets table guarded too.
    Equal to the per-layer packs where written (tests/test_gpu_kernels.py test_pack_batch_equals_per_layer_pack)."""
    o = _o(dt)
    rng = np.random.default_rng(17)
    nl, sz = 3, 27 * 64 * 64
    offs, pos = [], 7
    for gap in (5, 64, 0):
        offs.append(pos)
        pos += sz + gap
    flat = dev(rng.normal(size=pos).astype(np.float32))
    assert offs[-1] + sz == flat.numel()

    def launch(T):
        o.pack_conv64_weights_batch(T["flat"], T["offs"], T["packs"], streams=streams)
        return [T["packs"]], []

    def oracle(wr):
        for i, off in enumerate(offs):
            wf, wd = o.pack_conv64_weights(flat[off:off + sz].view(3, 3, 3, 64, 64))
            for got, want in ((wr[0][i, 0], wf), (wr[0][i, 1], wd)):
                wrote = ~torch.isnan(got)
                assert bool(wrote.any()) and _same_bits(got[wrote], want[wrote])
    run_guarded("pack_conv64_weights_batch %s %s" % (dt, streams), launch, const={"flat": flat, "offs": torch.tensor(offs, device="cuda", dtype=torch.int64)},
                out={"packs": ((nl, 2, o.PACK_ELEMS), o.ACT_DTYPE)}, oracle=oracle, sparse=True)


# ---------------------------------------------------------------------------------------------------------------- patch gather
@pytest.mark.parametrize("mode", [0, 1])
def test_gather_patches(fdn, mode):
    """fdn_gather_patches through ctypes with a hand-built DESC_DTYPE table (guarded, it holds the address of the guarded volume): a
    (T=2, X=7, Y=6, Z=5) volume, S = 4, patches at the origin and flush against the far corner of the last frame, no rotation and all
    nine (plane, k); bit for bit the numpy slice / rot90 / divide / threshold."""
    lib = _lib.load()
    Tn, X, Y, Z, S = 2, 7, 6, 5, 4
    rng = np.random.default_rng(2024 + mode)
    vol = rng.uniform(-2, 2, (Tn, X, Y, Z)).astype(np.float32)
    rots = [(0, 0)] + [(p, k) for p in (1, 2, 3) for k in (1, 2, 3)]
    rows = []
    for i, (plane, k) in enumerate(rots):
        sign, div = (1.0, 0.25) if mode else ((-1.0, 0.7) if i % 2 else (1.0, 1.5))
        rows.append((0, 0, 0, 0, plane, k, mode, sign, div))                                   # at the origin
        rows.append((Tn - 1, X - S, Y - S, Z - S, plane, k, mode, sign, div))                   # flush against the far corner of the last frame
    B = len(rows)

    def table(T):
        desc = np.zeros(B, ddev.DESC_DTYPE)
        for b, (t, x0, y0, z0, plane, k, md, sign, div) in enumerate(rows):
            desc[b] = (T["vol"].data_ptr(), X, Y, Z, t, x0, y0, z0, plane, k, md, sign, div)
        return torch.from_numpy(desc.view(np.uint8)).cuda()

    def launch(T):
        rc = lib.fdn_gather_patches(T["desc"].data_ptr(), T["out"].data_ptr(), B, S, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.fdn_last_error()
        return [T["out"]], []

    def oracle(wr):
        got = wr[0].cpu().numpy()
        for b, (t, x0, y0, z0, plane, k, md, sign, div) in enumerate(rows):
            p = vol[t, x0:x0 + S, y0:y0 + S, z0:z0 + S]
            if plane:
                p = np.rot90(p, k, axes=se.AXES[plane])
            want = (p >= np.float32(div)).astype(np.float32) if md else np.float32(sign) * (p / np.float32(div))
            assert got[b].tobytes() == np.ascontiguousarray(want, dtype=np.float32).tobytes(), rows[b]
    run_guarded("gather_patches mode %d" % mode, launch, const={"vol": torch.from_numpy(vol).cuda(), "desc": table}, out={"out": ((B, S, S, S), F32)},
                oracle=oracle)

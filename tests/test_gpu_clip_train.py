"""Gradient clipping on the GPU, trainer level: TrainerController(global_clipnorm=, clipvalue=) against a float64 recomputation on the host
of norm, scale and update from the buffers the step left behind, and through every route to the optimiser step -- plain, accumulated,
flushed, fine-tuning, bf16 activations, data parallel, train_network.

Semantics under test (src/Network/TrainerController.py:73,223-225 with tf.keras.optimizers.Adam(global_clipnorm=c) / (clipvalue=c)): the
clipped gradient is tape.gradient's, i.e. flat_g + B 2 lambda w on the trainable kernels, after accumulation and after the all-reduce.

The configuration is tests/test_gpu_grad_accum.py's: P 8, R 2, 1 + 1 blocks, B <= 4."""
import glob
import importlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import flownet_oracle as O
import _clip_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")

P, RES, LB, HB = 8, 2, 1, 1
LR = 1e-4
HUGE = 1e30                          # global_clipnorm that never clips: monitoring only
L2GS = 2 * O.L2_LAMBDA


def _trainer():
    return importlib.import_module("4dflownet_amd.trainer")


def _tc(**kw):
    return _trainer().TrainerController(P, RES, initial_learning_rate=LR, quicksave_enable=False, low_resblock=LB, hi_resblock=HB, seed=0, **kw)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _rows(batch, rows):
    return tuple(a[rows] for a in batch)


def _close(got, ref, tol, name):
    """The measure of tests/test_gpu_kernels.py::close: max |error| over max |reference|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    print("%s: max err %.3e of scale %.3e" % (name, err, np.abs(ref).max()))
    assert err <= tol, (name, err)


@pytest.fixture(scope="module")
def batch4():
    return O.synthetic_batch(4, P, RES, seed=31)


@pytest.fixture(scope="module")
def monitored(batch4):
    """One step of a controller that only watches the norm (huge c): the norm every test below scales its c from, and the unclipped
    weights after one and two steps."""
    tc = _tc(global_clipnorm=HUGE)
    tc.train_step(batch4)
    norm = float(tc.last_grad_norm)
    w1 = _bits(tc.model.flat_w)
    tc.train_step(batch4)
    assert np.isfinite(norm) and norm > 0
    return {"norm": norm, "w1": w1, "w2": _bits(tc.model.flat_w), "mean": tc.grad_norm_metric.result(), "norm2": float(tc.last_grad_norm)}


def _host_recomputation(batch, c_of_norm, monitored_norm, **kw):
    tc = _tc(global_clipnorm=c_of_norm * monitored_norm, **kw)
    m, opt = tc.model, tc.optimizer
    w0 = _np(m.flat_w)
    tc.train_step(batch)
    g, slot, isk = _np(m.flat_g), float(m.batch_slot[0]), _np(m.is_kernel)
    assert slot == batch[0].shape[0]
    l2s = R.l2s_f32(L2GS, slot)
    wr, mr, vr = w0.astype(np.float64), np.zeros(m.n_params), np.zeros(m.n_params)
    norm = R.clipped_adam_step(wr, g, mr, vr, isk, 1, LR, l2s, global_clipnorm=tc.global_clipnorm)
    got = float(tc.last_grad_norm)
    err, bound = R.norm_check(got, g, w0, isk, l2s)
    print("last_grad_norm %.9g, float64 %.9g: |N^2 - S| %.3e, bound %.3e" % (got, norm, err, bound))
    assert err <= bound
    assert norm > 2 * tc.global_clipnorm                             # active, by the host's own norm
    _close(_np(m.flat_w), wr, 5e-5, "w")
    _close(_np(opt.m), mr, 1e-5, "m")                                # (Adam's first update is ~lr sign(g) whatever the scale: the slots
    _close(_np(opt.v), vr, 5e-5, "v")                                # are what shows that the gradient was scaled)
    mu = 0.1 * R.step_gradient(g, w0, isk, l2s)
    assert np.abs(_np(opt.m) - mu).max() > 0.5 * np.abs(mu).max()     # ... far from the unclipped step's
    assert tc.grad_norm_metric.result() == pytest.approx(got, rel=1e-6)
    return tc


# ------------------------------------------------------------------------------------------------ 1. the plain step
def test_clipped_step_against_a_float64_recomputation_on_the_host(batch4, monitored):
    tc = _host_recomputation(batch4, 0.25, monitored["norm"])
    assert float(tc.last_grad_norm) == monitored["norm"]             # the same gradient, the same weights: the same bits
    tc.reset_metrics()
    assert tc.grad_norm_metric.result() == 0.0


def test_bf16_clipped_step_against_a_float64_recomputation_on_the_host(batch4, monitored):
    """Parameter gradients are fp32 in bf16 mode too: the same launches on the same kind of buffers."""
    _host_recomputation(batch4, 0.25, monitored["norm"], dtype="bfloat16")


def test_inactive_clip_changes_no_bit(batch4, monitored):
    plain = _tc()
    clipped = _tc(global_clipnorm=4 * monitored["norm"])
    value = _tc(clipvalue=1e6)
    for tc in (plain, clipped, value):
        tc.train_step(batch4)
    assert np.array_equal(_bits(plain.model.flat_w), monitored["w1"])
    for tc in (plain, clipped, value):
        tc.train_step(batch4)
    for tc in (plain, clipped, value):
        assert np.array_equal(_bits(tc.model.flat_w), monitored["w2"])
        assert np.array_equal(_bits(tc.optimizer.m), _bits(plain.optimizer.m)) and np.array_equal(_bits(tc.optimizer.v), _bits(plain.optimizer.v))
    assert float(clipped.last_grad_norm) == monitored["norm2"]
    assert monitored["mean"] == pytest.approx(0.5 * (monitored["norm"] + monitored["norm2"]), rel=1e-6)
    assert plain.last_grad_norm is None and value.last_grad_norm is None


def test_clipvalue_step_against_a_float64_recomputation_on_the_host(batch4):
    probe = _tc()
    probe.train_step(batch4)
    gp = R.step_gradient(_np(probe.model.flat_g), 0, 0, 0)
    c = float(np.median(np.abs(gp[gp != 0])))                        # half of the non-zero gradient elements are clamped
    tc = _tc(clipvalue=c)
    m, opt = tc.model, tc.optimizer
    w0 = _np(m.flat_w)
    tc.train_step(batch4)
    g, isk = _np(m.flat_g), _np(m.is_kernel)
    wr, mr, vr = w0.astype(np.float64), np.zeros(m.n_params), np.zeros(m.n_params)
    R.clipped_adam_step(wr, g, mr, vr, isk, 1, LR, R.l2s_f32(L2GS, 4.0), clipvalue=c)
    _close(_np(m.flat_w), wr, 5e-5, "w")
    _close(_np(opt.m), mr, 1e-5, "m")
    _close(_np(opt.v), vr, 5e-5, "v")
    assert float(opt.m.abs().max()) <= 0.1 * c * (1 + 1e-6) and bool((opt.m.abs() >= 0.1 * c * (1 - 1e-6)).any())      # m = (1 - b1) g''
    assert tc.last_grad_norm is None and tc._clip_out is None        # no norm pass, no buffers


# ------------------------------------------------------------------------------------------------ 2. the default trainer
def test_default_trainer_issues_no_clipping_launch_and_allocates_nothing(fdn, monkeypatch, batch4, monitored):
    def boom(*a, **k):
        raise AssertionError("a clipping launch without a clipping argument")
    seen = []
    adam = fdn.ops.adam_step

    def watching(*a, **k):
        seen.append(sorted(k))
        return adam(*a, **k)
    monkeypatch.setattr(fdn.ops, "grad_sumsq_partials", boom)
    monkeypatch.setattr(fdn.ops, "clip_scale", boom)
    monkeypatch.setattr(fdn.ops, "adam_step", watching)
    tc = _tc()
    before = set(k for k, v in vars(tc).items() if isinstance(v, torch.Tensor))
    tc.train_step(batch4)
    tc.train_step(batch4)
    assert len(seen) == 2 and all("g_scale_dev" not in k and "clip_value" not in k for k in seen), seen
    assert set(k for k, v in vars(tc).items() if isinstance(v, torch.Tensor)) == before
    assert tc._clip_partials is None and tc._clip_out is None and tc.last_grad_norm is None
    assert np.array_equal(_bits(tc.model.flat_w), monitored["w2"])
    value = _tc(clipvalue=1.0)                                       # clipvalue needs no norm pass either
    value.train_step(batch4)
    assert "clip_value" in seen[-1] and value._clip_out is None


# ------------------------------------------------------------------------------------------------ 3. accumulation
def _check_weights(w, ref_g, ref_w, steps=1):
    """tests/test_gpu_grad_accum.py::_check_weights."""
    dw = np.abs(w.astype(np.float64) - ref_w)
    g = np.abs(ref_g)
    good = g >= 1e-3 * g.max()
    print("weights: max |dw| %.3e (%.2f lr), well-conditioned %.1f %%, max |dw| there %.3e" % (dw.max(), dw.max() / LR, 100.0 * good.mean(), dw[good].max()))
    assert dw.max() <= 2.1 * steps * LR
    assert good.sum() > 0.2 * good.size
    assert dw[good].max() <= 1e-6


def test_accumulated_group_is_clipped_once_and_equals_the_clipped_big_batch(fdn, monkeypatch, batch4, monitored):
    c = 0.25 * monitored["norm"]
    calls = []
    sumsq = fdn.ops.grad_sumsq_partials
    tc = _tc(accum_steps=2, global_clipnorm=c)

    def counting(*a, **k):
        calls.append(tc._accum_count)
        return sumsq(*a, **k)
    monkeypatch.setattr(fdn.ops, "grad_sumsq_partials", counting)
    tc.train_step(_rows(batch4, [0, 1]))
    assert calls == [] and tc.last_grad_norm is None                 # a non-closing micro-step: no norm pass
    tc.train_step(_rows(batch4, [2, 3]))
    assert calls == [2] and tc.optimizer.iterations == 1             # once per group, on the closing micro-step
    big = _tc(global_clipnorm=c)
    big.train_step(batch4)
    assert calls == [2, 0]
    acc, ref = _np(tc.accum_g_ext), _np(big.model.flat_g_ext)
    assert acc[-1] == 4.0 == ref[-1]
    d = acc[:-1].astype(np.float64) - ref[:-1]
    assert np.linalg.norm(d) <= 1e-3 * np.linalg.norm(ref[:-1]) and np.abs(d).max() <= 1e-3 * np.abs(ref[:-1]).max()
    _check_weights(_np(tc.model.flat_w), ref[:-1], _np(big.model.flat_w))
    # the gradients agree to 1e-3 in L2 and the L2 term is the same: so do the norms (triangle inequality), and the slots the scale shaped
    na, nb = float(tc.last_grad_norm), float(big.last_grad_norm)
    assert abs(na - nb) <= 1e-3 * nb and nb == monitored["norm"]
    _close(_np(tc.optimizer.m), _np(big.optimizer.m), 2e-3, "m of the group against m of the big batch")
    # the float64 recomputation from the accumulator
    w0 = _np(_tc().model.flat_w)
    isk = _np(tc.model.is_kernel)
    l2s = R.l2s_f32(L2GS, 4.0)
    err, bound = R.norm_check(na, acc[:-1], w0, isk, l2s)
    assert err <= bound
    wr, mr, vr = w0.astype(np.float64), np.zeros(acc.size - 1), np.zeros(acc.size - 1)
    R.clipped_adam_step(wr, acc[:-1], mr, vr, isk, 1, LR, l2s, global_clipnorm=c)
    _close(_np(tc.optimizer.m), mr, 1e-5, "m")
    _close(_np(tc.model.flat_w), wr, 5e-5, "w")


def test_apply_accumulated_clips_a_ragged_group(fdn, monkeypatch, batch4, monitored):
    calls = []
    sumsq = fdn.ops.grad_sumsq_partials

    def counting(*a, **k):
        calls.append(1)
        return sumsq(*a, **k)
    monkeypatch.setattr(fdn.ops, "grad_sumsq_partials", counting)
    probe = _tc(global_clipnorm=HUGE)
    probe.train_step(_rows(batch4, [0, 1]))
    c = 0.25 * float(probe.last_grad_norm)
    calls.clear()
    tc = _tc(accum_steps=2, global_clipnorm=c)
    w0 = _np(tc.model.flat_w)
    tc.train_step(_rows(batch4, [0, 1]))
    assert not calls and tc.optimizer.iterations == 0
    assert tc.apply_accumulated() is True
    assert calls == [1] and tc.optimizer.iterations == 1
    acc, isk = _np(tc.accum_g_ext), _np(tc.model.is_kernel)
    assert acc[-1] == 2.0
    l2s = R.l2s_f32(L2GS, 2.0)
    err, bound = R.norm_check(float(tc.last_grad_norm), acc[:-1], w0, isk, l2s)
    assert err <= bound
    wr, mr, vr = w0.astype(np.float64), np.zeros(acc.size - 1), np.zeros(acc.size - 1)
    norm = R.clipped_adam_step(wr, acc[:-1], mr, vr, isk, 1, LR, l2s, global_clipnorm=c)
    assert norm > 2 * c
    _close(_np(tc.optimizer.m), mr, 1e-5, "m")
    _close(_np(tc.optimizer.v), vr, 5e-5, "v")
    _close(_np(tc.model.flat_w), wr, 5e-5, "w")
    assert tc.apply_accumulated() is False and calls == [1]


# ------------------------------------------------------------------------------------------------ 4. fine-tuning
def test_frozen_layers_are_outside_the_norm_and_keep_their_bits(batch4):
    probe = _tc(trainable="heads", global_clipnorm=HUGE)
    probe.train_step(batch4)
    c = 0.25 * float(probe.last_grad_norm)
    tc = _tc(trainable="heads", global_clipnorm=c)
    m, opt = tc.model, tc.optimizer
    fz = m.frozen_map.bool()
    live = ~_np(fz)
    assert live.any() and (~live).any()
    opt.m[fz] = 0.125                                                # planted values survive: the slots of frozen parameters are not touched
    opt.v[fz] = 0.375
    w0, m0, v0 = _np(m.flat_w), _bits(opt.m), _bits(opt.v)
    adam = tc._adam

    def poisoned(g, batch_slot):
        g[fz] = float("nan")                                         # what a frozen layer's range holds must not matter
        return adam(g, batch_slot)
    tc._adam = poisoned
    tc.train_step(batch4)
    got = float(tc.last_grad_norm)
    g, isk = _np(m.flat_g), _np(m.is_kernel)
    assert np.isnan(g[~live]).all() and np.isfinite(g[live]).all()
    l2s = R.l2s_f32(L2GS, 4.0)
    g_clean = np.where(live, g, 0.0)
    err, bound = R.norm_check(got, g_clean, w0, isk, l2s, live)
    print("norm over the trainable ranges %.9g: |N^2 - S| %.3e, bound %.3e" % (got, err, bound))
    assert np.isfinite(got) and err <= bound
    assert got == float(probe.last_grad_norm)
    w1 = _np(m.flat_w)
    assert np.array_equal(w1.view(np.int32)[~live], w0.view(np.int32)[~live])
    assert np.array_equal(_bits(opt.m)[~live], m0[~live]) and np.array_equal(_bits(opt.v)[~live], v0[~live])
    assert np.isfinite(w1).all()
    wr, mr, vr = w0.astype(np.float64), np.zeros(m.n_params), np.zeros(m.n_params)
    norm = R.clipped_adam_step(wr, g_clean, mr, vr, isk, 1, LR, l2s, global_clipnorm=c, live=live)
    assert norm > 2 * c
    _close(w1[live], wr[live], 5e-5, "w")
    _close(_np(opt.m)[live], mr[live], 1e-5, "m")
    _close(_np(opt.v)[live], vr[live], 5e-5, "v")


# ------------------------------------------------------------------------------------------------ 5. data parallel
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, q, c):
    """tests/test_gpu_finetune_parallel.py's spawn: one GPU each over nccl with >= 2 GPUs, both ranks on cuda:0 over gloo otherwise."""
    ngpu = torch.cuda.device_count()
    backend = "nccl" if ngpu >= world else "gloo"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank % ngpu), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(rank % ngpu)
    parallel = importlib.import_module("4dflownet_amd.parallel")
    parallel.init_from_env(backend=backend)
    tc = _tc(global_clipnorm=c)
    gb = O.synthetic_batch(2, P, RES, seed=31)
    tc.train_step(tuple(a[rank:rank + 1] for a in gb))
    torch.cuda.synchronize()
    parallel.barrier()
    q.put((rank, _np(tc.model.flat_w), _np(tc.model.flat_g_ext), _np(tc.last_grad_norm.reshape(1)), _np(tc.optimizer.m)))
    torch.distributed.destroy_process_group()


def test_dp2_clipped_step_equals_one_process_and_both_ranks_hold_the_same_bits():
    gb = O.synthetic_batch(2, P, RES, seed=31)
    probe = _tc(global_clipnorm=HUGE)
    probe.train_step(gb)
    c = 0.25 * float(probe.last_grad_norm)
    single = _tc(global_clipnorm=c)
    single.train_step(gb)
    torch.cuda.synchronize()
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, c)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    (_, wa, ga, na, ma), (_, wb, gb_, nb, mb) = res
    assert np.array_equal(wa.view(np.int32), wb.view(np.int32)) and np.array_equal(na.view(np.int32), nb.view(np.int32))
    assert np.array_equal(ma.view(np.int32), mb.view(np.int32))
    assert ga[-1] == 2.0 and gb_[-1] == 2.0                          # the global batch size is in the slot the norm pass reads
    ref = _np(single.model.flat_g).astype(np.float64)
    d = ga[:-1].astype(np.float64) - ref
    print("gradient: rel L2 %.3e, rel max %.3e" % (np.linalg.norm(d) / np.linalg.norm(ref), np.abs(d).max() / np.abs(ref).max()))
    assert np.linalg.norm(d) <= 1e-3 * np.linalg.norm(ref) and np.abs(d).max() <= 1e-3 * np.abs(ref).max()
    _check_weights(wa, ref, _np(single.model.flat_w))
    ns = float(single.last_grad_norm)
    assert abs(float(na[0]) - ns) <= 1e-3 * ns and ns > 2 * c
    _close(ma, _np(single.optimizer.m), 2e-3, "m of the ranks against m of one process")
    w0 = _np(_tc().model.flat_w)
    err, bound = R.norm_check(float(na[0]), ga[:-1], w0, _np(single.model.is_kernel), R.l2s_f32(L2GS, 2.0))
    assert err <= bound                                              # the norm of the all-reduced sum with the global batch in the slot


# ------------------------------------------------------------------------------------------------ 6. train_network
def test_train_network_logs_the_norm_and_leaves_the_columns_alone(tmp_path):
    """cfg1 as in tests/test_gpu_pipeline.py (patch 16, res 1, batch 2, 2 + 1 blocks), two epochs with global_clipnorm set."""
    data = importlib.import_module("4dflownet_amd.data")
    tfevents = importlib.import_module("4dflownet_amd.tfevents")
    trainer = _trainer()
    P1, R1, B, LB1, HB1 = 16, 1, 2, 2, 1
    idx = data.load_indexes(os.path.join(DATA, "train.csv"))[:6]
    val = data.load_indexes(os.path.join(DATA, "validate.csv"))[:4]
    mk = lambda rows, sh: data.PatchHandler3D(DATA, P1, R1, B, 0.6).initialize_dataset(rows, shuffle=sh, shard=(0, 1))
    make = lambda **kw: trainer.TrainerController(P1, R1, initial_learning_rate=2e-4, quicksave_enable=False, network_name="t4d",
                                                  low_resblock=LB1, hi_resblock=HB1, **kw)
    tc = make(global_clipnorm=0.05)
    tc.init_model_dir(base_dir=str(tmp_path / "clipped"))
    tc.train_network(mk(idx, True), mk(val, True), n_epoch=2, verbose=False)
    plain = make()
    plain.init_model_dir(base_dir=str(tmp_path / "plain"))           # (the preamble and the header are written here)
    lines = open(tc.logfile).read().splitlines()
    lines0 = open(plain.logfile).read().splitlines()
    assert "Gradient clipping: global_clipnorm=0.05" in lines and not any(l.startswith("Gradient clipping") for l in lines0)
    header, = [l for l in lines if l.startswith("epoch")]
    header0, = [l for l in lines0 if l.startswith("epoch")]
    assert header.encode() == header0.encode()
    assert lines.index("Gradient clipping: global_clipnorm=0.05") < lines.index(header)
    assert [l for l in lines if not l.startswith("Gradient clipping")][:len(lines0)] == lines0
    rows = [l for l in lines if l[:2] in ("1,", "2,")]
    assert len(rows) == 2
    assert list(tc.loss_metrics) == list(plain.loss_metrics) and "grad_norm" not in tc.loss_metrics
    files = glob.glob(os.path.join(tc.model_dir, "tensorboard", "train", "events.out.tfevents.*"))
    assert len(files) == 1
    by_step = {}
    for e in tfevents.read_events(files[0])[1:]:
        by_step.setdefault(e["step"], {}).update(e["scalars"])
    assert sorted(by_step) == [0, 1]
    for step in (0, 1):
        assert sorted(by_step[step]) == sorted("t4d/" + k for k in ("learning_rate", "grad_norm", "loss", "accuracy", "mse", "div"))
        assert np.isfinite(by_step[step]["t4d/grad_norm"]) and by_step[step]["t4d/grad_norm"] > 0
    assert by_step[1]["t4d/grad_norm"] == pytest.approx(tc.grad_norm_metric.result(), rel=1e-6)      # the mean of the last epoch's three steps
    vfiles = glob.glob(os.path.join(tc.model_dir, "tensorboard", "validate", "events.out.tfevents.*"))
    assert not any("grad_norm" in k for e in tfevents.read_events(vfiles[0])[1:] for k in e["scalars"])
    with pytest.raises(ValueError, match="both set"):
        make(global_clipnorm=1.0, clipvalue=1.0)
    tc.global_clipnorm = -1.0                                        # read again on every optimiser step
    with pytest.raises(ValueError, match="global_clipnorm"):
        tc.train_step(next(iter(mk(idx, False))))

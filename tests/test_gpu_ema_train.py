"""Weight EMA on the GPU, trainer level: TrainerController(use_ema=, ema_momentum=, ema_overwrite_frequency=, ema_validation=) through every
route to the optimiser step -- plain, accumulated, fine-tuning -- and ema_weights(), finalize_ema(), the overwrite, train_network and the
checkpoint files.

The average is compared against the float64 recurrence of tests/_ema_ref.py on the weights read back after every step, at its bound;
everything else -- the weights and slots of a run with an average against a run without, evaluation under the average against a fresh model
holding it, the weights after the context -- bit for bit.

The configuration is tests/test_gpu_clip_train.py's: P 8, R 2, 1 + 1 blocks, B 4."""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import flownet_oracle as O
import _ema_ref as E

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")

P, RES, LB, HB = 8, 2, 1, 1
LR = 1e-4
MOM = 0.9


def _trainer():
    return importlib.import_module("4dflownet_amd.trainer")


def _tc(lr=LR, **kw):
    return _trainer().TrainerController(P, RES, initial_learning_rate=lr, quicksave_enable=False, low_resblock=LB, hi_resblock=HB, seed=0, **kw)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _rows(batch, rows):
    return tuple(a[rows] for a in batch)


def _arrays(model, flat):
    """A flat parameter vector (host) as the list set_weights takes."""
    out = []
    for L in model.layers:
        out.append(flat[L.w_off:L.w_off + L.w.numel()].reshape(tuple(L.w.shape)))
        if L.b is not None:
            out.append(flat[L.b_off:L.b_off + L.b.numel()].reshape(tuple(L.b.shape)))
    return out


def _within(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = int(np.argmax(err))
    print("%s: max |ema - ref| %.3e, bound there %.3e, least slack %.3e" % (what, err[worst], bound[worst], (bound - err).min()))
    assert np.isfinite(err).all() and (err <= bound).all(), what


@pytest.fixture(scope="module")
def batch4():
    return O.synthetic_batch(4, P, RES, seed=31)


@pytest.fixture(scope="module")
def plain3(batch4):
    """Three steps of the default trainer: what a run with an average must reproduce bit for bit."""
    tc = _tc()
    losses = [_bits(tc.train_step(batch4)) for _ in range(3)]
    return {"w": _bits(tc.model.flat_w), "m": _bits(tc.optimizer.m), "v": _bits(tc.optimizer.v), "losses": losses}


# ------------------------------------------------------------------------------------------------ 1. the default trainer
def test_default_trainer_never_calls_the_ema_entry_point_and_allocates_nothing(fdn, monkeypatch, batch4, plain3):
    lib = fdn._lib.load()
    calls = []
    real = lib.fdn_adam_step_ema

    def counting(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, "fdn_adam_step_ema", counting)
    tc = _tc()
    before = set(k for k, v in vars(tc).items() if isinstance(v, torch.Tensor))
    for _ in range(3):
        tc.train_step(batch4)
    assert calls == [] and tc.ema is None and tc._ema_spare is None
    assert set(k for k, v in vars(tc).items() if isinstance(v, torch.Tensor)) == before
    assert np.array_equal(_bits(tc.model.flat_w), plain3["w"])
    with pytest.raises(RuntimeError, match="no weight average yet"):
        with tc.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="no weight average yet"):
        tc.finalize_ema()
    on = _tc(use_ema=True)                                           # ... and the counter does see a run with an average
    assert on.ema is None
    on.train_step(batch4)
    assert calls == [1] and on.ema is not None and on.ema.dtype == torch.float32 and on.ema.shape == on.model.flat_w.shape


# ------------------------------------------------------------------------------------------------ 2. a run with an average
def test_three_steps_with_an_average_equal_the_plain_run_and_follow_the_recurrence(fdn, monkeypatch, batch4, plain3):
    inits = []
    adam = fdn.ops.adam_step

    def watching(*a, **k):
        inits.append(k.get("ema_init"))
        return adam(*a, **k)
    monkeypatch.setattr(fdn.ops, "adam_step", watching)
    tc = _tc(use_ema=True, ema_momentum=MOM)
    weights, losses = [_np(tc.model.flat_w)], []
    for t in range(1, 4):
        losses.append(_bits(tc.train_step(batch4)))
        weights.append(_np(tc.model.flat_w))
        ref = E.ema_chain(weights, MOM)
        _within(_np(tc.ema), ref[-1], E.ema_bound(weights, ref), "step %d" % t)
    assert inits == [True, False, False]
    assert np.array_equal(_bits(tc.model.flat_w), plain3["w"])
    assert np.array_equal(_bits(tc.optimizer.m), plain3["m"]) and np.array_equal(_bits(tc.optimizer.v), plain3["v"])
    assert all(np.array_equal(a, b) for a, b in zip(losses, plain3["losses"]))
    a = _np(tc.ema).astype(np.float64)
    assert np.abs(a - weights[-1]).max() > 0.5 * LR and np.abs(a - weights[0]).max() > 0.05 * LR      # it lags, and it has moved
    # weights changed outside the optimiser: the average restarts from them
    tc.model.set_weights(_arrays(tc.model, weights[0]))
    assert not tc.ema_current
    tc.train_step(batch4)
    assert inits[-1] is True
    restarted = E.ema_chain([weights[0], _np(tc.model.flat_w)], MOM)
    _within(_np(tc.ema), restarted[-1], E.ema_bound([weights[0], _np(tc.model.flat_w)], restarted), "after set_weights")
    # the momentum is read on every step; a bad one stops the step before anything is launched
    tc.ema_momentum = 0.999999999
    it = tc.optimizer.iterations
    with pytest.raises(ValueError, match="ema_momentum"):
        tc.train_step(batch4)
    assert tc.optimizer.iterations == it


def test_accumulation_moves_the_average_once_per_group(fdn, monkeypatch, batch4):
    seen = []
    adam = fdn.ops.adam_step

    def watching(*a, **k):
        seen.append("ema" in k)
        return adam(*a, **k)
    monkeypatch.setattr(fdn.ops, "adam_step", watching)
    tc = _tc(use_ema=True, ema_momentum=MOM, accum_steps=2)
    w0 = _np(tc.model.flat_w)
    tc.train_step(_rows(batch4, [0, 1]))
    assert seen == [] and tc.ema is None and tc.optimizer.iterations == 0      # a non-closing micro-step: no launch, no buffer
    tc.train_step(_rows(batch4, [2, 3]))
    assert seen == [True] and tc.optimizer.iterations == 1
    w1 = _np(tc.model.flat_w)
    ref = E.ema_chain([w0, w1], MOM)
    _within(_np(tc.ema), ref[-1], E.ema_bound([w0, w1], ref), "group 1")
    a1 = _bits(tc.ema)
    tc.train_step(_rows(batch4, [0, 1]))
    assert seen == [True] and np.array_equal(_bits(tc.ema), a1)      # untouched until the group closes
    assert tc.apply_accumulated() is True
    assert seen == [True, True] and tc.optimizer.iterations == 2
    w2 = _np(tc.model.flat_w)
    ref = E.ema_chain([w0, w1, w2], MOM)
    _within(_np(tc.ema), ref[-1], E.ema_bound([w0, w1, w2], ref), "group 2 (flushed)")


def test_frozen_layers_average_is_their_weight(batch4):
    tc = _tc(use_ema=True, ema_momentum=MOM, trainable="heads")
    fz = _np(tc.model.frozen_map) != 0
    assert fz.any() and (~fz).any()
    w0 = _np(tc.model.flat_w)
    weights = [w0]
    for _ in range(2):
        tc.train_step(batch4)
        weights.append(_np(tc.model.flat_w))
    a, w = _bits(tc.ema), _bits(tc.model.flat_w)
    assert np.array_equal(a[fz], w[fz]) and np.array_equal(w[fz], w0.view(np.int32)[fz])
    assert not np.array_equal(a[~fz], w[~fz])
    ref = E.ema_chain(weights, MOM, frozen=fz)
    _within(_np(tc.ema), ref[-1], E.ema_bound(weights, ref), "heads")
    # a layer frozen later: its average becomes its weight, whatever it was while the layer trained
    full = _tc(use_ema=True, ema_momentum=MOM)
    full.train_step(batch4)
    full.train_step(batch4)
    assert not np.array_equal(_bits(full.ema)[fz], _bits(full.model.flat_w)[fz])
    full.model.set_trainable("heads")
    full.train_step(batch4)
    assert np.array_equal(_bits(full.ema)[fz], _bits(full.model.flat_w)[fz])


# ------------------------------------------------------------------------------------------------ 3. evaluating under the average
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_ema_weights_context_evaluates_under_the_average_and_restores_the_exact_bits(batch4, dtype):
    tc = _tc(use_ema=True, ema_momentum=MOM, dtype=dtype)
    for _ in range(2):
        tc.train_step(batch4)
    inputs = [np.asarray(a, np.float32) for a in batch4[:6]]
    w_before, ema_before = _bits(tc.model.flat_w), _bits(tc.ema)
    pred_before = tc.model.predict(inputs)
    l2_version = tc._l2_version
    assert l2_version == tc.model.weights_version
    with tc.ema_weights() as inside:
        assert inside is tc
        assert np.array_equal(_bits(tc.model.flat_w), ema_before)
        pred_ema = tc.model.predict(inputs)
        with pytest.raises(RuntimeError, match="train_step inside"):
            tc.train_step(batch4)
        with pytest.raises(RuntimeError, match="ema_weights inside"):
            with tc.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="finalize_ema inside"):
            tc.finalize_ema()
    assert np.array_equal(_bits(tc.model.flat_w), w_before) and np.array_equal(_bits(tc.ema), ema_before)
    assert np.array_equal(tc.model.predict(inputs).view(np.int32), pred_before.view(np.int32))
    assert tc.ema_current and tc._l2_version == tc.model.weights_version          # neither the average nor Adam's L2 partials went stale
    fresh = _tc(dtype=dtype)
    fresh.model.set_weights(_arrays(fresh.model, _np(tc.ema)))
    pred_fresh = fresh.model.predict(inputs)
    assert np.array_equal(pred_ema.view(np.int32), pred_fresh.view(np.int32))
    assert not np.array_equal(pred_ema, pred_before)
    # an exception inside still restores the weights
    with pytest.raises(KeyError):
        with tc.ema_weights():
            raise KeyError("x")
    assert np.array_equal(_bits(tc.model.flat_w), w_before) and not tc._ema_active
    # the step after the context is the step of a run that never entered it
    twin = _tc(use_ema=True, ema_momentum=MOM, dtype=dtype)
    for _ in range(3):
        twin.train_step(batch4)
    tc.train_step(batch4)
    assert np.array_equal(_bits(tc.model.flat_w), _bits(twin.model.flat_w)) and np.array_equal(_bits(tc.ema), _bits(twin.ema))
    assert tc.loss_metrics["l2_reg_loss"].result() == twin.loss_metrics["l2_reg_loss"].result()
    # an open accumulation group cannot be applied inside
    acc = _tc(use_ema=True, accum_steps=2)
    acc.train_step(_rows(batch4, [0, 1]))
    acc.train_step(_rows(batch4, [2, 3]))
    acc.train_step(_rows(batch4, [0, 1]))
    with acc.ema_weights():
        with pytest.raises(RuntimeError, match="apply_accumulated inside"):
            acc.apply_accumulated()
    assert acc.apply_accumulated() is True


# ------------------------------------------------------------------------------------------------ 4. overwriting the weights
def test_overwrite_frequency_copies_the_average_into_the_weights_and_marks_the_l2_partials_stale(fdn, batch4):
    """A step size of 1e-2 -- a fifth of the largest weight -- so that the sum of squares Adam's launch left behind (the weights before
    the overwrite) is far from that of the averaged weights."""
    tc = _tc(lr=1e-2, use_ema=True, ema_momentum=MOM, ema_overwrite_frequency=2)
    tc.train_step(batch4)
    assert not np.array_equal(_bits(tc.model.flat_w), _bits(tc.ema))
    tc.train_step(batch4)
    assert tc.optimizer.iterations == 2
    assert np.array_equal(_bits(tc.model.flat_w), _bits(tc.ema))
    assert tc._l2_version != tc.model.weights_version
    fresh = float(fdn.ops.l2_sumsq(tc.model.flat_w, tc.model.is_kernel)[0]) * 5e-7
    stale = float(tc._l2_partials.double().sum()) * 5e-7
    tc.reset_metrics()
    w2 = _np(tc.model.flat_w)
    tc.train_step(batch4)
    l2 = tc.loss_metrics["l2_reg_loss"].result()
    # Sums of positive fp32 terms: the relative error is at most (additions on the longest path + 1 for the square) 2^-24.  fdn_l2_sumsq:
    # 4096 chains of ceil(n / 4096) terms, then 2 + 10 levels; the partials: ceil(n / (2048 * 256)) terms per thread, 6 + 2 levels, then
    # fdn_sum_partials with 8 + 6 + 2; one more for the multiply by lambda on either side.
    n = tc.model.n_params
    bound = (-(-n // 4096) + 14 + -(-n // (2048 * 256)) + 26) * 2.0 ** -24 * fresh
    print("l2_reg_loss of the step after the overwrite %.9g, fresh l2_sumsq %.9g, bound %.3e, Adam's stale sum %.9g" % (l2, fresh, bound, stale))
    assert abs(l2 - fresh) <= bound
    assert abs(stale - fresh) > 100 * bound
    assert not np.array_equal(_bits(tc.model.flat_w), _bits(tc.ema))
    # the packs followed the overwrite: the forward of step 3 ran on the averaged weights (a fresh model holding them gives the same loss)
    twin = _tc()
    twin.model.set_weights(_arrays(twin.model, w2))
    twin.train_step(batch4)
    assert tc.loss_metrics["train_mse"].result() == twin.loss_metrics["train_mse"].result()
    # the average went on from the overwritten weights without a restart
    ref = E.ema_step(w2, w2, _np(tc.model.flat_w), MOM)
    _within(_np(tc.ema), ref, E.ema_bound([w2, _np(tc.model.flat_w)], [ref]), "step 3")
    # finalize_ema: the same overwrite on demand
    tc.finalize_ema()
    assert np.array_equal(_bits(tc.model.flat_w), _bits(tc.ema)) and tc.ema_current
    assert tc._l2_version != tc.model.weights_version


# ------------------------------------------------------------------------------------------------ 5. train_network and the files
def test_train_network_validates_and_checkpoints_under_the_average(tmp_path):
    """cfg1 as in tests/test_gpu_pipeline.py (patch 16, res 1, batch 2, 2 + 1 blocks), two epochs."""
    data = importlib.import_module("4dflownet_amd.data")
    trainer = _trainer()
    P1, R1, B, LB1, HB1 = 16, 1, 2, 2, 1
    idx = data.load_indexes(os.path.join(DATA, "train.csv"))[:6]
    val = data.load_indexes(os.path.join(DATA, "validate.csv"))[:4]
    mk = lambda rows: data.PatchHandler3D(DATA, P1, R1, B, 0.6).initialize_dataset(rows, shuffle=False, shard=(0, 1))
    make = lambda **kw: trainer.TrainerController(P1, R1, initial_learning_rate=2e-4, quicksave_enable=False, network_name="t4d",
                                                  low_resblock=LB1, hi_resblock=HB1, **kw)

    def run(name, n_epoch, **kw):
        tc = make(use_ema=True, ema_momentum=MOM, **kw)
        tc.init_model_dir(base_dir=str(tmp_path / name))
        saves = []
        save = tc.save_best_model

        def recording():
            assert not tc._ema_active                                 # train_network has left the context before it saves
            save()
            saves.append((open(tc.model_path + "-best.h5", "rb").read(), open(tc.model_dir + "/optimizer.pkl", "rb").read(), _bits(tc.ema)))
        tc.save_best_model = recording
        val_w = []
        test_step = tc.test_step

        def watching(batch):
            val_w.append(tc._ema_active)
            return test_step(batch)
        tc.test_step = watching
        tc.train_network(mk(idx), mk(val), n_epoch=n_epoch, verbose=False)
        return tc, saves, val_w

    tc, saves, val_w = run("ema_val", 2, ema_validation=True)
    assert len(val_w) == 4 and all(val_w) and not tc._ema_active     # every validation batch saw the averaged weights
    ref, ref_saves, ref_val_w = run("raw_val", 1)
    assert len(ref_val_w) == 2 and not any(ref_val_w)
    assert saves and ref_saves
    assert saves[0][0] == ref_saves[0][0] and saves[0][1] == ref_saves[0][1]      # -best.h5 and optimizer.pkl: what they are without ema_validation
    plain = make()
    plain.init_model_dir(base_dir=str(tmp_path / "plain"))
    plain.save_best_model()
    assert not os.path.exists(plain.model_path + "-best-ema.h5")
    # the header line, and nothing else new in loss.csv
    lines, lines0 = open(tc.logfile).read().splitlines(), open(plain.logfile).read().splitlines()
    extra = [l for l in lines if l.startswith("Weight EMA: momentum=%s" % MOM)]
    assert len(extra) == 1 and not any(l.startswith("Weight EMA") for l in lines0)
    header, = [l for l in lines if l.startswith("epoch")]
    header0, = [l for l in lines0 if l.startswith("epoch")]
    assert header == header0 and lines.index(extra[0]) < lines.index(header)
    assert [l for l in lines if not l.startswith("Weight EMA")][:len(lines0)] == lines0
    # the file of the average: a weights file like any other, holding the average of the moment it was written
    path = tc.model_path + "-best-ema.h5"
    assert os.path.exists(path) and os.path.exists(ref.model_path + "-best-ema.h5")
    fresh = make()
    fresh.model.load_weights(path)
    assert np.array_equal(_bits(fresh.model.flat_w), saves[-1][2])
    if len(saves) == 2:                                              # the last epoch was the best: that moment is now
        assert np.array_equal(saves[-1][2], _bits(tc.ema))
    assert not np.array_equal(_bits(fresh.model.flat_w), _bits(tc.model.flat_w))
    # restore_model brings the average back, and the next step goes on from it
    back = make(use_ema=True, ema_momentum=MOM)
    back.restore_model(tc.model_dir, "t4d-best.h5")
    assert back.ema_current and np.array_equal(_bits(back.ema), saves[-1][2])
    fresh.model.load_weights(tc.model_path + "-best.h5")
    assert np.array_equal(_bits(back.model.flat_w), _bits(fresh.model.flat_w))
    w0, a0 = _np(back.model.flat_w), _np(back.ema)
    batch = next(iter(mk(idx)))
    back.train_step(batch)
    w1 = _np(back.model.flat_w)
    step = E.ema_step(a0, w0, w1, MOM)
    _within(_np(back.ema), step, E.ema_bound([w0, w1, a0], [step]), "the step after restore_model")
    # without use_ema the file is ignored; without the file the average restarts from the loaded weights
    off = make()
    off.restore_model(tc.model_dir, "t4d-best.h5")
    assert off.ema is None
    os.remove(path)
    again = make(use_ema=True, ema_momentum=MOM)
    again.restore_model(tc.model_dir, "t4d-best.h5")
    assert again.ema is None and not again.ema_current
    again.train_step(batch)
    assert np.array_equal(_bits(again.model.flat_w), w1.view(np.int32))
    restart = E.ema_step(None, w0, w1, MOM, init=True)
    _within(_np(again.ema), restart, E.ema_bound([w0, w1], [restart]), "restart after restore_model")

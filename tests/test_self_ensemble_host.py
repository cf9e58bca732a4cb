"""The self-ensemble on the host: the numpy restatement of the orientations (tests/_self_ensemble.py) against data.rotate_vector_field,
inverse o forward as the identity, the fp32 mean, and what the option parser accepts and refuses.  No GPU, no library."""
from importlib import import_module

import numpy as np
import pytest

import _self_ensemble as se

data = import_module("4dflownet_amd.data")
ops = import_module("4dflownet_amd.ops")
ops_bf16 = import_module("4dflownet_amd.ops_bf16")


def _triple(seed=5, shape=(7, 7, 7)):
    rng = np.random.default_rng(seed)
    comps = [rng.standard_normal(shape).astype(np.float32) for _ in range(3)]
    comps[0][0, 1, 2] = 0.0                       # zeros: -0.0 where the sign rule flips them
    comps[1][3, 3, 3] = 0.0
    comps[2][4, 4, 0] = 0.0
    comps[2][6, 0, 5] = -0.0
    return comps


def test_the_ten_orientations_are_the_loaders_in_its_order():
    assert se.ROT90 == ops.ROT90_ORIENTATIONS == ((0, 0),) + tuple((p, k) for p in (1, 2, 3) for k in (1, 2, 3))
    assert set(se.TABLE) == set(se.ROT90) and set(data._ROT) == set(se.ROT90[1:])
    for o in se.ROT90[1:]:
        assert (tuple(se.TABLE[o][0]), tuple(se.TABLE[o][1])) == (tuple(data._ROT[o][0]), tuple(data._ROT[o][1])), o


@pytest.mark.parametrize("orientation", se.ROT90)
def test_forward_equals_rotate_vector_field(orientation):
    plane, k = orientation
    comps = _triple()
    for signed in (True, False):
        want = data.rotate_vector_field(comps, k, plane, signed)
        got = se.forward(comps, orientation, signed=signed)
        for i in range(3):
            assert se.same_bits(got[i], np.ascontiguousarray(want[i])), (orientation, signed, i)
    if orientation != (0, 0):
        neg = [i for i in range(3) if se.TABLE[orientation][1][i] < 0]
        assert neg and any(np.signbit(se.forward(comps, orientation)[i][se.forward(comps, orientation)[i] == 0]).any() for i in neg)


@pytest.mark.parametrize("orientation", se.ROT90)
def test_inverse_of_forward_is_the_identity_bit_for_bit(orientation):
    comps = _triple(seed=6)
    rotated = np.stack(se.forward(comps, orientation), axis=-1)            # the network's output has the layout (S,S,S,3)
    back = se.inverse(rotated, orientation)
    assert se.same_bits(back, np.stack(comps, axis=-1)), orientation
    # with a batch axis in front: the same per patch
    batch = np.stack([rotated, rotated[::-1].copy()])
    got = se.inverse(batch, orientation, lead=1)
    assert se.same_bits(got[0], back) and se.same_bits(got[1], se.inverse(batch[1], orientation))


def test_mean_sums_in_list_order_and_divides_once():
    rng = np.random.default_rng(8)
    preds = [rng.standard_normal((2, 5, 5, 5, 3)).astype(np.float32) for _ in range(3)]
    orientations = [(0, 0), (2, 3), (1, 2)]
    q = [se.inverse(p, o, lead=1) for p, o in zip(preds, orientations)]
    want = (((q[0] + q[1]).astype(np.float32) + q[2]).astype(np.float32) / np.float32(3)).astype(np.float32)
    assert se.same_bits(se.mean(preds, orientations), want)
    assert se.same_bits(se.mean(preds[:1], [(0, 0)]), preds[0])            # one orientation: no divide
    assert not se.same_bits(np.float32([0.0]), np.float32([-0.0])) and se.same_bits(np.float32([np.nan, 1]), -np.float32([np.nan, -1]))


def test_option_parser_accepts_what_the_issue_lists():
    f = ops.self_ensemble_orientations
    assert f is ops_bf16.self_ensemble_orientations
    assert f(None) is None and f(False) is None
    assert f("rot90") == se.ROT90
    assert f([(0, 0), (2, 3), (1, 2)]) == ((0, 0), (2, 3), (1, 2))         # used as given, in its order
    assert f(((3, 1),)) == ((3, 1),) and f([[1, 2], np.array([2, 1])]) == ((1, 2), (2, 1))
    assert f([(0, 0)]) == ((0, 0),)
    assert f(f("rot90")) == se.ROT90


@pytest.mark.parametrize("bad", ["rot", "ROT90", "", [], (), [(0, 1)], [(1, 0)], [(2, 0), (1, 1)], [(4, 1)], [(1, 4)], [(-1, 1)], [(1, 1), (1, 1)],
                                 [(0, 0), (0, 0)], 5, 1.5, True, [None], [(1,)], [(1, 1, 1)], [1, 1], [(1.0, 1)], [(True, 1)], [("1", "1")],
                                 {"rot90": 1}])
def test_option_parser_refuses_everything_else(bad):
    with pytest.raises(ValueError, match="self_ensemble"):
        ops.self_ensemble_orientations(bad)


def test_predictor_signatures_carry_the_option():
    import inspect
    predictor = import_module("4dflownet_amd.predictor")
    for name in ("predict_volume", "predict_cores", "predict_file", "evaluate_file", "main", "evaluate_main"):
        p = inspect.signature(getattr(predictor, name)).parameters
        assert "self_ensemble" in p and p["self_ensemble"].default is None, name
    for m in (ops, ops_bf16):
        p = inspect.signature(m.input_features_volume).parameters
        assert list(p)[-1] == "orientation" and p["orientation"].default is None
        assert m.unrotate_accumulate is ops.unrotate_accumulate
    assert str(inspect.signature(ops.unrotate_accumulate)) == "(pred, acc, orientation, first, divisor=1)"
    assert "device_tiler says" in predictor.predict_file.__doc__            # documented: the option forces the device path

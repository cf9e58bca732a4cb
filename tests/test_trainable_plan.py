"""Fine-tuning without a GPU: network.backward_plan -- which weight gradients and input gradients backward() issues, and what
forward(training=True) retains, for a set of trainable layers --, the set_trainable specs and the Keras-order helpers on a subset.

Layer indices (network.layer_specs, creation order): 0, 1 the pc convs, 2, 3 the phase convs, 4 the 1x1, 5 the conv behind it,
6 .. 6 + 2 (LB + HB) - 1 the ResBlock convs (two per block, low-res blocks first), then three heads of a 64->64 and a 64->1 conv."""
import importlib

import pytest

net = importlib.import_module("4dflownet_amd.network")

CONFIGS = [(2, 1), (0, 1), (2, 0)]


def _names(LB, HB):
    return [s[0] for s in net.layer_specs(LB, HB)]


def _plan(LB, HB, spec):
    return net.backward_plan(LB, HB, net.trainable_flags(spec, LB, HB))


def _is64(LB, HB):
    return [(k, ci, co) == (3, 64, 64) for _, k, ci, co, _ in net.layer_specs(LB, HB)]


@pytest.mark.parametrize("LB,HB", CONFIGS)
def test_all_trainable_is_todays_schedule(LB, HB):
    n = len(_names(LB, HB))
    p = _plan(LB, HB, "all")
    assert p["wgrad"] == [True] * n                              # 12 + 2 (LB + HB) weight gradients
    # every layer but the two that read the network's inputs hands a gradient down: 10 + 2 (LB + HB) input gradients
    assert p["dgrad"] == [i not in (0, 2) for i in range(n)]
    assert p["any_trainable"] and p["all_trainable"] and p["heads_to_trunk"] and p["through_upsample"] and p["conv1x1_dgrad"]
    assert p["branch_phase"] and p["branch_pc"] and p["dbias_prev"] == [True] * 3 and all(p["need_at"])
    k = p["keep"]
    assert all(k[s] for s in ("phase", "pc", "a0", "a1", "p0", "p1", "c0", "up_out")) and all(k["trunk"]) and all(k["h"]) and all(k["heads"])
    m = p["masks"]
    assert all(m["h"]) and all(m["heads"])
    assert m["trunk"] == [j != LB for j in range(LB + HB + 1)]    # the tensor that feeds the upsample: its act' is taken from the tensor


@pytest.mark.parametrize("LB,HB", CONFIGS)
def test_heads_only_needs_no_fused_dgrad_and_six_weight_gradients(LB, HB):
    n = len(_names(LB, HB))
    p = _plan(LB, HB, "heads")
    assert sum(p["wgrad"]) == 6 and p["wgrad"][n - 6:] == [True] * 6
    is64 = _is64(LB, HB)
    assert not any(d for d, f in zip(p["dgrad"], is64) if f)      # the fused dgrad is the input gradient of a 64->64 layer
    assert [p["dgrad"][n - 6 + 2 * h + 1] for h in range(3)] == [True] * 3      # 64->1: its input gradient feeds the head's 64->64 weight gradient
    assert not p["heads_to_trunk"] and not p["through_upsample"] and not p["conv1x1_dgrad"] and not any(p["need_at"])
    assert p["dbias_prev"] == [True] * 3
    k = p["keep"]
    assert not any(k[s] for s in ("phase", "pc", "a0", "a1", "p0", "p1", "c0")) and not any(k["h"]) and k["heads"] == [True] * 3
    # the heads' 64->64 weight gradients read the last trunk tensor (the upsample's output when there is no hi-res block) and nothing else
    if HB:
        assert k["trunk"] == [False] * (LB + HB) + [True] and not k["up_out"]
    else:
        assert k["trunk"] == [False] * (LB + 1) and k["up_out"]
    assert not any(p["masks"]["trunk"]) and not any(p["masks"]["h"]) and p["masks"]["heads"] == [True] * 3


@pytest.mark.parametrize("LB,HB", CONFIGS)
def test_hires_stops_above_the_upsample(LB, HB):
    n = len(_names(LB, HB))
    cut = 6 + 2 * LB
    p = _plan(LB, HB, "hires")
    assert p["wgrad"] == [i >= cut for i in range(n)]
    assert not any(p["dgrad"][:cut + 1])                         # nothing at or below the upsample; the first hi-res conv hands nothing down
    assert not p["through_upsample"] and not p["conv1x1_dgrad"] and not any(p["need_at"][:LB + 1])
    assert p["heads_to_trunk"] == (HB > 0)
    assert all(p["dgrad"][cut + 1:n - 6]) and all(p["need_at"][LB + 1:])
    k = p["keep"]
    assert not any(k[s] for s in ("phase", "pc", "a0", "a1", "p0", "p1", "c0")) and not any(k["trunk"][:LB + 1]) and not any(k["h"][:LB])
    assert k["up_out"] and all(k["h"][LB:]) and all(k["trunk"][LB + 1:])


@pytest.mark.parametrize("LB,HB", CONFIGS)
def test_first_phase_conv_alone_descends_the_phase_branch_only(LB, HB):
    n = len(_names(LB, HB))
    p = _plan(LB, HB, ["conv3d_2"])
    assert p["wgrad"] == [i == 2 for i in range(n)]
    assert p["dgrad"] == [i >= 3 for i in range(n)]             # every layer on the way down to conv3d_2; conv3d, conv3d_1 (pc) and conv3d_2 itself not
    assert p["branch_phase"] and not p["branch_pc"] and p["conv1x1_dgrad"] and p["heads_to_trunk"] and p["through_upsample"]
    assert p["dbias_prev"] == [False] * 3
    k = p["keep"]
    assert k["phase"] and k["p0"] and k["p1"] and k["a1"] and k["c0"] and not k["pc"] and not k["a0"]
    # linear: no act' to form and no weight gradient reads it -- only where the heads sit on it (no hi-res block), their input gradient takes its shape
    assert k["up_out"] == (HB == 0)


@pytest.mark.parametrize("LB,HB", CONFIGS)
def test_a_frozen_layer_between_trainable_ones_hands_the_gradient_down(LB, HB):
    names = _names(LB, HB)
    mid = 5 if LB + HB == 0 else 7                                # conv3d_7: the second conv of the first ResBlock
    p = _plan(LB, HB, [nm for i, nm in enumerate(names) if i != mid])
    assert p["dgrad"][mid] and not p["wgrad"][mid]
    assert sum(p["wgrad"]) == len(names) - 1
    assert p["dgrad"] == _plan(LB, HB, "all")["dgrad"]
    # the reverse, all but one mid conv frozen: its weight gradient, every input gradient above it, none at or below it
    q = _plan(LB, HB, [names[mid]])
    assert q["wgrad"] == [i == mid for i in range(len(names))]
    assert q["dgrad"] == [i > mid for i in range(len(names))]
    assert not q["conv1x1_dgrad"] and not q["branch_phase"] and not q["branch_pc"]


@pytest.mark.parametrize("LB,HB", CONFIGS)
def test_nothing_trainable_is_reported(LB, HB):
    p = _plan(LB, HB, [])
    assert not p["any_trainable"] and not any(p["wgrad"]) and not any(p["dgrad"])
    assert _plan(LB, HB, ["conv3d_1"])["any_trainable"]


def test_plan_refuses_a_flag_list_of_the_wrong_length():
    with pytest.raises(ValueError, match="flags"):
        net.backward_plan(2, 1, [True] * 5)


@pytest.mark.parametrize("LB,HB", CONFIGS)
def test_specs(LB, HB):
    names = _names(LB, HB)
    n = len(names)
    assert net.trainable_flags("all", LB, HB) == [True] * n == net.trainable_flags(None, LB, HB)
    assert net.trainable_flags("heads", LB, HB) == [i >= n - 6 for i in range(n)]
    assert net.trainable_flags("hires", LB, HB) == [i >= 6 + 2 * LB for i in range(n)]
    assert net.trainable_flags((nm for nm in names[1:3]), LB, HB) == [i in (1, 2) for i in range(n)]
    with pytest.raises(ValueError, match="conv3d_%d" % n):
        net.trainable_flags([names[0], "conv3d_%d" % n], LB, HB)
    with pytest.raises(ValueError, match="lowres"):
        net.trainable_flags("lowres", LB, HB)


@pytest.mark.parametrize("LB,HB", CONFIGS)
def test_keras_order_of_a_subset_keeps_the_relative_order_of_all(LB, HB):
    names = _names(LB, HB)
    n = len(names)
    full_names = net.variable_names(LB, HB)
    full = [full_names[i] for i in net.keras_variable_positions(LB, HB)]
    layer_order = [names[i] for i in net.keras_layer_order(LB, HB)]
    assert [v.split("/")[0] for v in full if v.endswith("kernel:0")] == layer_order
    for flags in (net.trainable_flags("heads", LB, HB), net.trainable_flags("hires", LB, HB), [i % 3 != 1 for i in range(n)],
                  net.trainable_flags(["conv3d", "conv3d_2", "conv3d_3"], LB, HB)):
        sub_names = net.variable_names(LB, HB, flags)
        assert sub_names == [v for v in full_names if flags[names.index(v.split("/")[0])]]       # creation order
        pos = net.keras_variable_positions(LB, HB, flags)
        assert sorted(pos) == list(range(len(sub_names)))
        assert [sub_names[i] for i in pos] == [v for v in full if flags[names.index(v.split("/")[0])]]

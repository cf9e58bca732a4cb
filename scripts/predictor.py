"""Counterpart of the reference's src/predictor.py (same hard-coded surface; see 4dflownet_amd/predictor.py:main).
--self-ensemble [rot90]: average every patch's prediction over the training rotations (predict_file(self_ensemble=); ten forwards per
patch, on the device tiler).
--blend B: overlap-add stitching, neighbouring patch cores overlap by B low-res voxels and are cross-faded (predict_file(blend=B);
(E/(E-B))^3 times the forwards with E = patch_size - 4, on the device tiler).
--output-activation {linear,tanh}: the activation the heads of the loaded weights were trained with (prepare_network(output_activation=);
linear = the reference's network as shipped, tanh = its first published weights)."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _self_ensemble(argv):
    """The value behind --self-ensemble ("rot90" when none is given), or None without the switch."""
    if "--self-ensemble" not in argv:
        return None
    nxt = argv[argv.index("--self-ensemble") + 1:][:1]
    return nxt[0] if nxt and not nxt[0].startswith("--") else "rot90"


def _blend(argv):
    """The integer behind --blend, or 0 without the switch; a missing or non-integer value ends the run."""
    if "--blend" not in argv:
        return 0
    nxt = argv[argv.index("--blend") + 1:][:1]
    try:
        return int(nxt[0])
    except (IndexError, ValueError):
        raise SystemExit("--blend needs an integer: the overlap of neighbouring cores in low-res voxels") from None


def _output_activation(argv):
    """The value behind --output-activation, or None without the switch; anything but linear / tanh ends the run."""
    if "--output-activation" not in argv:
        return None
    nxt = argv[argv.index("--output-activation") + 1:][:1]
    if not nxt or nxt[0] not in ("linear", "tanh"):
        raise SystemExit("--output-activation needs linear or tanh")
    return nxt[0]


if __name__ == '__main__':
    importlib.import_module("4dflownet_amd.predictor").main(self_ensemble=_self_ensemble(sys.argv[1:]), blend=_blend(sys.argv[1:]),
                                                            output_activation=_output_activation(sys.argv[1:]))

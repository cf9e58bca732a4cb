"""Scores a checkpoint on a low-resolution file against its high-resolution ground truth (4dflownet_amd/predictor.py:evaluate_main;
the reference has no counterpart: it leaves the comparison to the user).
--self-ensemble [rot90]: average every patch's prediction over the training rotations (predict_file(self_ensemble=); ten forwards per
patch, on the device tiler)."""
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


if __name__ == '__main__':
    importlib.import_module("4dflownet_amd.predictor").evaluate_main(self_ensemble=_self_ensemble(sys.argv[1:]))

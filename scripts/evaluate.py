"""Scores a checkpoint on a low-resolution file against its high-resolution ground truth (4dflownet_amd/predictor.py:evaluate_main;
the reference has no counterpart: it leaves the comparison to the user)."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    importlib.import_module("4dflownet_amd.predictor").evaluate_main()

"""Writes output_activation_none.json: sha256 of the FDN_ACT_NONE output of the 64 -> 1 head forward on the operands of
tests/test_gpu_output_activation.py::test_head_forward, as computed by a library built from the commit BEFORE FDN_ACT_TANH existed --
what "the default path did not change" is pinned against.  Needs a GPU.
   python tests/golden/make_output_activation_none.py path/to/that/lib4dflow_hip.so"""
import hashlib
import importlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import bench_output_activation as B              # noqa: E402  (load_old: a second library through ctypes)
import test_gpu_output_activation as T           # noqa: E402

old = B.load_old(sys.argv[1])
st = torch.cuda.current_stream().cuda_stream
res = {}
for dtype in ("float32", "bfloat16"):
    for shape, ls in T.HEAD_CASES:
        x, w, b = T.head_operands(shape, ls)
        xt = T.dev(x).to(torch.float32 if dtype == "float32" else torch.bfloat16)
        wt, bt = T.dev(w), T.dev(b)
        y = torch.empty(shape + (1,), device="cuda")
        N, D, H, W = shape
        head = (xt.data_ptr(), None, wt.data_ptr(), None, bt.data_ptr(), None, y.data_ptr(), N, D, H, W, 64, 1, 3, 1, 0, 0, 0.2)
        rc = old.fdn_conv3d_fwd(*head, 0, st) if dtype == "float32" else old.fdn_conv3d_fwd_bf16(*head, st)
        assert rc == 0
        torch.cuda.synchronize()
        res["%s %s 2^%d" % (dtype, "x".join(map(str, shape)), ls)] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
with open(os.path.join(HERE, "output_activation_none.json"), "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)

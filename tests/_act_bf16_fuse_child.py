"""Child process of tests/test_gpu_train_act_bf16.py::test_04c_gelu_fusion_off: one LM and one retriever training step (L2 d256 fixture
of tests/_train_bf16_ref.py) under ``precision="bf16"`` with the activation store off and on, under whatever R4D_TRAIN_FUSE_GELU
this process was started with (the library reads it once).  Prints one JSON line
{kind: {"fp32": sha256, "bf16": sha256, "gelu_launches": bf16-output GELU launches of the store-on step}}."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import _train_bf16_ref as R  # noqa: E402
import test_gpu_train_act_bf16 as T  # noqa: E402

dev = torch.device("cuda:0")
out = {}
for kind in ("lm", "enc"):
    c = R.case("L2_d256_T130", kind)
    out[kind] = {}
    for store in ("fp32", "bf16"):
        _tr, step = T.stepper(dev, c, "bf16", store, dropout=(0.1, 0.1, 0.1), seed=5)
        before = T.hits()
        s = T.snapshot(step())
        h = hashlib.sha256()
        for n in sorted(s):
            h.update(s[n].cpu().numpy().tobytes())
        out[kind][store] = h.hexdigest()
        if store == "bf16":
            out[kind]["gelu_launches"] = T.delta(before)["gelu"]
print(json.dumps(out))

"""Child process of tests/test_gpu_conv1d_route.py::test_gelu_fusion_switch: one retriever training step (one layer, d 128, 32 rows,
seeded) under gemm modes bf16x3 and f32, under whatever R4D_TRAIN_FUSE_GELU this process was started with (the library reads it
once).  Prints one JSON line {mode: sha256 over the embeddings and every gradient}."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rag4dyg_amd import ops, training  # noqa: E402
from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG  # noqa: E402

dev = torch.device("cuda:0")
out = {}
for mode in ("bf16x3", "f32"):
    ops.set_gemm_mode(mode)
    torch.manual_seed(128)
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=128, n_positions=16, n_ctx=16, n_embd=128, n_layer=1, n_head=4))
    m.tie_weights()
    tr = training.EncoderTrainer(m.to(dev).eval(), precision="fp32")
    ids = torch.randint(0, 128, (4, 8), generator=torch.Generator().manual_seed(2)).to(dev)
    G = torch.randn(4, 128, generator=torch.Generator().manual_seed(3)).to(dev)
    emb = tr.forward([ids])
    grads = tr.backward(G)
    h = hashlib.sha256(emb.cpu().numpy().tobytes())
    for n in sorted(grads):
        h.update(grads[n].cpu().numpy().tobytes())
    out[mode] = h.hexdigest()
print(json.dumps(out))

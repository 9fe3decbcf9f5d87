#!/usr/bin/env python3
"""SimpleDyG LM-training step (``LMTrainer.step``: forward, LM head, shifted cross entropy, backward) at the reference's script
shapes: ms per step and tokens/s, the per-class breakdown of ``r4d_profile_*``, the CE kernel's bytes / time against the 8 TB/s HBM
spec, the head's share of the step (step minus forward_hidden + backward_hidden timed alone; eval mode, no dropout), the head ALONE
through ``r4d_lm_head_train_f32`` (ms per call and its per-class kernel times), and as a yardstick the same head (h . wte^T, F.cross_entropy, backward) in torch autograd.
``wikiv2_v50k`` is the wikiv2 model on a 50,000-token vocabulary: the chunked head (``csrc/lm_head.hip``, ldV > 15,872).  Its record
adds the chunk rows, the bytes the materialised logits alone would take next to the step's workspace, and the time of ONE sweep of
logits GEMMs over the chunks (the GEMM the chunked head runs twice) with its share of the step.

    python tools/lm_train_bench.py [--steps 10] [--warmup 3] [--shapes uci13,wikiv2] [--attention stored|recompute] [--activations stored|recompute] [--precision fp32|bf16|fp32+attn|bf16+attn] [--head-precision fp32|bf16] [--act-store fp32|bf16] [--attention-kernel products|fused]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"uci13": dict(L=6, H=8, d=768, V=1800, B=32, Ts=(128, 340)),
          "wikiv2": dict(L=2, H=6, d=768, V=8814, B=32, Ts=(128, 512)),
          "wikiv2_v50k": dict(L=2, H=6, d=768, V=50000, B=32, Ts=(128,))}
HBM_BPS = 8e12


def _profile(lib):
    out = {}
    for c in range(lib.r4d_profile_num_classes()):
        ms, n, w = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        lib.r4d_profile_read(c, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
        if n.value:
            out[lib.r4d_profile_class_name(c).decode()] = dict(ms=ms.value, launches=n.value, work=w.value)
    return out


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _logits_sweep(tr, h):
    """One sweep of the chunked head's logits GEMMs (``h . wte_k^T`` per chunk, the arithmetic of the current mode) as a callable."""
    from rag4dyg_amd import _lib, ops
    from rag4dyg_amd.lm_training import head_chunks
    head, d = tr.head, tr.d
    chunks = head_chunks(head.ldV, _lib.load().r4d_lm_head_chunk_rows(head.ldV))
    mode = ops.gemm_mode()
    if mode == "f16x2" and head._h2 is not None:
        parts = [head._h2[c0:c0 + cn] for c0, cn in chunks]
        return lambda: [ops.conv1d_h2(h, p, None) for p in parts]
    if mode != "f32" and head._w3 is not None:
        flat = head._w3.view(-1)
        parts = [flat[3 * c0 * d:3 * (c0 + cn) * d].view(3, cn, d) for c0, cn in chunks]
        return lambda: [ops.conv1d_s3(h, p, None) for p in parts]
    parts = [(head.pad[c0:c0 + cn].t().contiguous(), head.pad[c0:c0 + cn]) for c0, cn in chunks]
    return lambda: [ops.conv1d(h, w, None, "none", None, wt) for w, wt in parts]


def main():
    from oracle import gpt2_ref
    from rag4dyg_amd import _lib, ops, training
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    from rag4dyg_amd.lm_training import LMTrainer
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="uci13,wikiv2")
    ap.add_argument("--one-step", type=int, default=0, metavar="T",
                    help="run one warm-up and ONE timed step at T of the first shape, print nothing else (for a kernel trace)")
    training.add_mode_arguments(ap)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for name in a.shapes.split(","):
        s = SHAPES[name]
        sd = gpt2_ref.make_state_dict(s["L"], s["d"], s["V"], n_positions=1024, seed=1, random_affine=True)
        sd.pop("lm_head.weight", None)
        cfg = GPT2Config(vocab_size=s["V"], n_positions=1024, n_ctx=1024, n_embd=s["d"], n_layer=s["L"], n_head=s["H"])
        m = GPT2LMHeadModel(cfg)
        m.load_state_dict(sd, strict=False)
        m.tie_weights()
        # eval mode: no dropout launches, so that the step and its body (timed alone below) differ by the head only
        m = m.to(dev).eval()
        torch.cuda.reset_peak_memory_stats()
        tr = LMTrainer(m, **training.modes_from_args(a))
        if a.one_step:
            ids = torch.randint(0, s["V"], (s["B"], a.one_step), device=dev)
            tr.step(ids)
            torch.cuda.synchronize()
            tr.step(ids)
            torch.cuda.synchronize()
            return
        for T in s["Ts"]:
            B, V, d = s["B"], s["V"], s["d"]
            ids = torch.randint(0, V, (B, T), device=dev)
            ms = _time(lambda: tr.step(ids), a.steps, a.warmup)
            ws_bytes = int(tr._ws.numel())                         # (the buffer only grows: shapes run in ascending T)
            peak = int(torch.cuda.max_memory_allocated())          # model, trainer and the timed steps up to this T
            lib.r4d_profile_enable(1)
            tr.step(ids)
            torch.cuda.synchronize()
            prof = _profile(lib)
            lib.r4d_profile_enable(0)
            N, ldV = B * T, tr.ldV
            ce = prof.get("lm_ce", {})
            chunked = ldV > 15872                                  # two kernels per chunk: the logits are read twice, written once
            ce_bytes = (3.0 if chunked else 2.0) * N * V * 4
            head_flop = 3 * 2.0 * N * ldV * d
            # the step without its head: forward_hidden + backward_hidden alone (same workspace layout); head = step - body
            c, w, g, keep = tr.enc._structs()
            Bs, Ts = (ctypes.c_int32 * 1)(B), (ctypes.c_int32 * 1)(T)
            ptrs = (ctypes.c_void_p * 1)(ids.data_ptr())
            ws = torch.empty(lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(c), 1, Bs, Ts), dtype=torch.uint8, device=dev)
            h = torch.empty(N, d, device=dev)
            dh = torch.randn(N, d, device=dev) * 1e-4
            stream = torch.cuda.current_stream().cuda_stream

            def body():
                _lib.check(lib.r4d_gpt2_train_forward_hidden_f32(ctypes.byref(c), ctypes.byref(w), 1, ptrs, Bs, Ts, h.data_ptr(), None,
                                                                 ws.data_ptr(), ws.numel(), stream), "fwd")
                _lib.check(lib.r4d_gpt2_train_backward_hidden_f32(ctypes.byref(c), ctypes.byref(w), ctypes.byref(g), 1, ptrs, Bs, Ts,
                                                                  dh.data_ptr(), None, ws.data_ptr(), ws.numel(), stream), "bwd")
            body_ms = _time(body, a.steps, a.warmup)
            del ws
            # the head alone on the ln_f rows the body left in h: the call the step makes, timed and profiled by itself
            from rag4dyg_amd.lm_training import lm_head_train
            tr.select_modes()
            hd_dh, hd_dw = torch.empty(N, d, device=dev), torch.empty(ldV, d, device=dev)
            _loss, hd_ws = lm_head_train(tr.head, h, ids.view(-1), T, 1.0, hd_dh, hd_dw)
            head_alone_ms = _time(lambda: lm_head_train(tr.head, h, ids.view(-1), T, 1.0, hd_dh, hd_dw, hd_ws), a.steps, a.warmup)
            lib.r4d_profile_enable(1)
            lm_head_train(tr.head, h, ids.view(-1), T, 1.0, hd_dh, hd_dw, hd_ws)
            torch.cuda.synchronize()
            head_prof = _profile(lib)
            lib.r4d_profile_enable(0)
            del hd_dh, hd_dw, hd_ws
            hr = h.clone().requires_grad_(True)
            wr = m.transformer.wte.weight.detach().clone().requires_grad_(True)
            lab = ids.view(B, T)[:, 1:].reshape(-1)

            def torch_head():
                lg = (hr @ wr.t()).view(B, T, V)[:, :-1].reshape(-1, V)
                torch.nn.functional.cross_entropy(lg, lab).backward()
            torch_ms = _time(torch_head, a.steps, a.warmup)
            lib.r4d_profile_enable(1)
            tr.step(ids)
            torch.cuda.synchronize()
            prof2 = _profile(lib)
            lib.r4d_profile_enable(0)
            total_prof = sum(v["ms"] for v in prof2.values())
            head_like = {k: v for k, v in prof2.items() if v["work"] > 0}
            rec = dict(shape=name, mode=ops.gemm_mode(), **tr.modes.record(), head_alone_ms=head_alone_ms,
                       head_alone_classes={k: dict(ms=round(v["ms"], 4), launches=v["launches"], work=v["work"]) for k, v in sorted(head_prof.items(), key=lambda kv: -kv[1]["ms"])},
                       launches={k: v["launches"] for k, v in sorted(prof2.items())},
                       workspace_bytes=ws_bytes, max_memory_allocated=peak, L=s["L"], H=s["H"], d=d, V=V,
                       ldV=ldV, B=B, T=T, ms_per_step=ms,
                       tokens_per_s=N / (ms / 1e3), ce_ms=ce.get("ms"), ce_bytes=ce_bytes,
                       ce_hbm_fraction=(ce_bytes / (ce["ms"] / 1e3) / HBM_BPS) if ce else None,
                       head_flop=head_flop, body_ms=body_ms, head_ms=ms - body_ms, head_share=(ms - body_ms) / ms,
                       head_tflops=head_flop / ((ms - body_ms) / 1e3) / 1e12, torch_head_ms=torch_ms, profiled_ms=total_prof,
                       classes={k: dict(ms=round(v["ms"], 4), launches=v["launches"], work=v["work"]) for k, v in sorted(head_like.items(), key=lambda kv: -kv[1]["ms"])})
            if chunked:
                sweep_ms = _time(_logits_sweep(tr, h), a.steps, a.warmup)
                rec.update(chunk_rows=int(lib.r4d_lm_head_chunk_rows(ldV)), materialised_logits_bytes=N * ldV * 4,
                           logits_sweep_ms=sweep_ms, extra_gemm_share=sweep_ms / ms)
            print(json.dumps(rec))
            del h, dh, hr, wr


if __name__ == "__main__":
    main()

"""Beam search against greedy decoding in one run (profiles/beam_search.md).    python tools/beam_bench.py [step] [reorder] [tokens]

step:    the beam step at B0 * n rows against the greedy step at B = B0 * n, UCI_13 (L6 H8 d768) and reddit (L2 H8 d512, V 11,919)
         decode shapes, B0 = 8, n = 2 and 4: graph replay, wall clock around 64 synchronised steps, the arms interleaved; then
         the new kernels' time per launch and the sum of all launches of a step from the library's launch profiler (host loop);
reorder: ``r4d_kv_cache_reorder_f32`` alone with every row moving (a cycle), after 8 and 64 generated positions: bytes read and
         written per second (HBM peak of the MI355X: 8 TB/s);
tokens:  ``generate(num_beams=n)`` against greedy ``generate`` on B0 * n prompts: 11 new tokens each, prefill included.
One JSON line per measurement.
"""
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import gpt2_ref                                                    # noqa: E402  (weights only)
from rag4dyg_amd import _lib, ops, synth                                       # noqa: E402
from rag4dyg_amd.gpt2 import BeamDecoder, GPT2Config, GPT2LMHeadModelRAG, GreedyDecoder   # noqa: E402

dev = torch.device("cuda:0")
SHAPES = (("UCI_13", (6, 8, 768)), ("reddit", (2, 8, 512)))
B0, BEAMS, T_CAP, PROMPT = 8, (2, 4), 384, 100


def model(L, H, d, V):
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=4, random_affine=True)
    sd["transformer.wte.weight"] *= 10.0                                       # logits with some spread
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dev).eval()


def arm(dec):
    """A decoder in the middle of a long generation: PROMPT positions cached, nothing that stops a row."""
    dec.cache.normal_()
    last = torch.randn(dec.B, dec.last.shape[1], device=dev)
    if isinstance(dec, BeamDecoder):
        dec.begin_beams(last, PROMPT, 10 ** 6)
    else:
        dec.begin(last, torch.full((dec.B,), PROMPT), 10 ** 6, 10 ** 6)


def wall_us(dec, n=64):
    arm(dec)
    dec._steps(8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dec._steps(n)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / n


def profile_us(dec, n=32):
    lib = _lib.load()
    was, dec.use_graph = dec.use_graph, False
    for warm in (True, False):
        arm(dec)
        lib.r4d_profile_enable(0 if warm else 1)
        dec._steps(4 if warm else n)
        torch.cuda.synchronize()
    out, total = {}, 0.0
    for c in range(lib.r4d_profile_num_classes()):
        ms, k, wk = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        lib.r4d_profile_read(c, ctypes.byref(ms), ctypes.byref(k), ctypes.byref(wk))
        if k.value:
            out[lib.r4d_profile_class_name(c).decode()] = round(1e3 * ms.value / k.value, 2)
            total += 1e3 * ms.value / n
    lib.r4d_profile_enable(0)
    dec.use_graph = was
    return out, round(total, 1)


def step():
    for shape_name, (L, H, d) in SHAPES:
        V = synth.SHAPES[shape_name].vocab_generator
        tr = model(L, H, d, V).transformer
        for n in BEAMS:
            g, b = GreedyDecoder(tr, B0 * n, T_CAP), BeamDecoder(tr, B0, n, T_CAP)
            ts = {"greedy": [], "beam": []}
            for rep in range(4):                                               # interleaved; the first round is the warm-up
                for name, dec in (("greedy", g), ("beam", b)):
                    us = wall_us(dec)
                    if rep:
                        ts[name].append(round(us, 1))
            us_b, total_b = profile_us(b)
            us_g, total_g = profile_us(g)
            print(json.dumps(dict(measure="step", shape=f"{shape_name} L{L} H{H} d{d} V{V}", B0=B0, n=n, rows=B0 * n,
                                  greedy_step_us=sorted(ts["greedy"]), beam_step_us=sorted(ts["beam"]),
                                  beam_rows_us=us_b.get("beam_rows"), beam_advance_us=us_b.get("beam_advance"), kv_reorder_us=us_b.get("kv_reorder"),
                                  greedy_advance_us=us_g.get("greedy_advance"), beam_step_kernels_us=total_b, greedy_step_kernels_us=total_g)),
                  flush=True)
            g.close()
            b.close()


def reorder():
    for shape_name, (L, H, d) in SHAPES:
        for n in BEAMS:
            R = B0 * n
            cache = torch.randn(L, R, T_CAP, 2 * d, device=dev)
            src = (torch.arange(R).view(B0, n).roll(1, 1)).reshape(-1).to(torch.int32)          # a cycle: every row moves
            for gen in (8, 64):
                lo, hi = torch.full((B0,), PROMPT, dtype=torch.int32), torch.full((B0,), PROMPT + gen, dtype=torch.int32)
                for _ in range(3):
                    ops.kv_cache_reorder(cache, src, n, lo, hi)
                srcd, lod, hid = src.to(dev), lo.to(dev), hi.to(dev)
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
                a.record()
                for _ in range(20):
                    lib.r4d_kv_cache_reorder_f32(cache.data_ptr(), srcd.data_ptr(), lod.data_ptr(), hid.data_ptr(), None, L, B0, n, T_CAP, d, stream)
                z.record()
                torch.cuda.synchronize()
                us = 1e3 * a.elapsed_time(z) / 20
                nbytes = 2 * L * R * gen * 2 * d * 4
                print(json.dumps(dict(measure="reorder", shape=f"{shape_name} L{L} d{d}", B0=B0, n=n, generated=gen, us=round(us, 2),
                                      bytes=nbytes, TB_per_s=round(nbytes / us / 1e6, 3))), flush=True)


def tokens():
    for shape_name, (L, H, d) in SHAPES:
        shape = synth.SHAPES[shape_name]
        V, T = shape.vocab_generator, shape.query_len[0]
        m = model(L, H, d, V)
        for n in BEAMS:
            prompts = [torch.randint(0, shape.v0, (B0 * n, T), generator=torch.Generator().manual_seed(i)).to(dev) for i in range(4)]
            arms = {"greedy B0*n rows": lambda p: m.generate(input_ids=p, max_length=T + 11),
                    "beam": lambda p: m.generate(input_ids=p[:B0], max_length=T + 11, num_beams=n)}
            times = {k: [] for k in arms}
            for rep in range(4):
                for name, fn in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for p in prompts:
                        fn(p)
                    torch.cuda.synchronize()
                    if rep:
                        times[name].append(time.perf_counter() - t0)
            print(json.dumps(dict(measure="tokens/s", shape=f"{shape_name} L{L} H{H} d{d} V{V}", B0=B0, n=n, prompt=T, new_tokens=11,
                                  greedy_row_tokens_per_s=[round(len(prompts) * B0 * n * 11 / t) for t in sorted(times["greedy B0*n rows"])],
                                  beam_returned_tokens_per_s=[round(len(prompts) * B0 * 11 / t) for t in sorted(times["beam"])])), flush=True)


if __name__ == "__main__":
    for part in sys.argv[1:] or ["step", "reorder", "tokens"]:
        {"step": step, "reorder": reorder, "tokens": tokens}[part]()

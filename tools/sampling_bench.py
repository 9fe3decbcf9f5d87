"""Sampled decoding against greedy decoding in one run (profiles/sampling.md).    python tools/sampling_bench.py [kernel] [tokens]

kernel: ``sample_advance_kernel`` against ``greedy_advance_kernel`` per launch, from the library's launch-profiler classes, in the
        host-loop form of the two decoders (B = 32; V = 1,801 / 11,919 / 50,257 on a small L1 d256 model, which only has to feed
        the two kernels logits of that width), and the kernels' share of a whole step at the reddit decode shape;
tokens: ``generate(do_sample=True, ...)`` against greedy ``generate`` at the UCI_13 (L6 H8 d768) and reddit (L2 H8 d512,
        V 11,919) generator shapes: 32 prompts of the shape's median query length, 11 new tokens each (val mode), graph replay,
        wall clock around synchronised calls, prefill included.
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
from rag4dyg_amd import _lib, synth                                            # noqa: E402
from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG, GreedyDecoder, SamplingDecoder   # noqa: E402

dev = torch.device("cuda:0")
SETTINGS = {"k50 p0.95 t0.8": dict(do_sample=True, top_k=50, top_p=0.95, temperature=0.8), "k0 p0.9": dict(do_sample=True, top_k=0, top_p=0.9)}


def model(L, H, d, V):
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=4, random_affine=True)
    sd["transformer.wte.weight"] *= 10.0                                       # logits with some spread
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dev).eval()


def profile_steps(dec, n=50):
    """n host-loop steps under the launch profiler -> {class: us per launch}, us of all launches per step."""
    lib = _lib.load()
    dec.use_graph = False
    dec.cache.normal_()
    dec.last.normal_()
    for warm in (True, False):
        dec.lens.fill_(100); dec.active.fill_(1); dec.gen_len.zero_()
        dec.params.copy_(torch.tensor([10 ** 6, 10 ** 6, 0, 0, 0, 0, 0, 0], dtype=torch.int32))
        lib.r4d_profile_enable(0 if warm else 1)
        dec._steps(5 if warm else n)
        torch.cuda.synchronize()
    out, total = {}, 0.0
    for c in range(lib.r4d_profile_num_classes()):
        ms, k, wk = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        lib.r4d_profile_read(c, ctypes.byref(ms), ctypes.byref(k), ctypes.byref(wk))
        if k.value:
            out[lib.r4d_profile_class_name(c).decode()] = round(1e3 * ms.value / k.value, 2)
            total += 1e3 * ms.value / n
    lib.r4d_profile_enable(0)
    return out, round(total, 1)


def kernel():
    for V in (1801, 11919, 50257):
        tr = model(1, 2, 256, V).transformer
        g = GreedyDecoder(tr, 32, 384)
        us, _ = profile_steps(g)
        rec = dict(measure="kernel", B=32, V=V, greedy_advance_us=us["greedy_advance"])
        g.close()
        s = SamplingDecoder(tr, 32, 384)
        for name, kw in SETTINGS.items():
            s.set_sampling(seed=1, **kw)
            us, _ = profile_steps(s)
            rec["sample_advance_us " + name] = us["sample_advance"]
        s.close()
        print(json.dumps(rec), flush=True)
    tr = model(2, 8, 512, 11919).transformer                                   # the reddit decode shape: the kernels' share of a step
    g = GreedyDecoder(tr, 32, 384)
    us, total = profile_steps(g)
    rec = dict(measure="step share", shape="reddit L2 H8 d512 V11919", B=32, greedy_advance_us=us["greedy_advance"], greedy_step_kernels_us=total)
    g.close()
    s = SamplingDecoder(tr, 32, 384)
    for name, kw in SETTINGS.items():
        s.set_sampling(seed=1, **kw)
        us, total = profile_steps(s)
        rec["sample_advance_us " + name], rec["sampled_step_kernels_us " + name] = us["sample_advance"], total
    s.close()
    print(json.dumps(rec), flush=True)


def tokens():
    for shape_name, (L, H, d) in (("UCI_13", (6, 8, 768)), ("reddit", (2, 8, 512))):
        shape = synth.SHAPES[shape_name]
        V, T = shape.vocab_generator, shape.query_len[0]
        m = model(L, H, d, V)
        prompts = [torch.randint(0, shape.v0, (32, T), generator=torch.Generator().manual_seed(i)).to(dev) for i in range(8)]
        rec = dict(measure="tokens/s", shape=f"{shape_name} L{L} H{H} d{d} V{V}", B=32, prompt=T, new_tokens=11)
        arms = dict({"greedy": dict(do_sample=False)}, **SETTINGS)
        times = {n: [] for n in arms}
        for rep in range(4):                                                   # arms interleaved; the first round is the warm-up
            for name, kw in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i, p in enumerate(prompts):
                    out = m.generate(input_ids=p, max_length=T + 11, seed=i, **kw)
                    assert tuple(out.shape) == (32, T + 11)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
        for name, ts in times.items():
            rec[name + " tokens/s"] = [round(len(prompts) * 32 * 11 / t) for t in sorted(ts)]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    for part in sys.argv[1:] or ["kernel", "tokens"]:
        {"kernel": kernel, "tokens": tokens}[part]()

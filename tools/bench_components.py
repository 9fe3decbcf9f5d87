#!/usr/bin/env python3
"""Secondary measurements (GPU box): the HBM-bound kernels of the path on their own rooflines.

  scan      (S+1)/2 cosine scan at the reference query batch (32) over N pool rows + top-10
  jaccard   f64 Jaccard matrices: real hepth/11 sets (golden fixture) and a synthetic 20k x 20k scale-up
  pool      pool-encode sequences/s (reference batching, fused groups)
  encode_precision   the bench step's encode, val-mode greedy decode and the real-data top-10 lists under
            ops.set_encode_precision("bf16") and ("bf16+attn") beside the f16x2 and bf16x3 arithmetics (alternated in one
            process); the attention kernels of the two words alone at head dims 64 .. 256
  topk_large   top-100 / top-1024 of 256 x 100k, 32 x 100k and 2,048 x 12,512 score rows: the radix-select path, the argsort route
            to the same lists, and the k = 64 launch, alternated in one process
  encode_step_trace WORD [SHAPE]   12 encode steps under one precision word and nothing else: the program of a
            ``rocprofv3 --kernel-trace --stats -- python tools/bench_components.py encode_step_trace bf16+attn`` run
Each line: achieved = algorithmic bytes / HIP-event time of the kernel class (r4d_profile_* hooks), peak 8 TB/s.
CPU baselines: oracle single-thread python-set Jaccard (as retrieval_data_annotation.py:36-41) on a bounded sample.
"""
import ctypes
import functools
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rag4dyg_amd import _lib, ops, synth                                   # noqa: E402
from bench import host_cores                                                # noqa: E402

PEAK = 8000.0
dev = torch.device("cuda:0")
lib = _lib.load()


def profile(fn, reps):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    lib.r4d_profile_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {}
    for c in range(lib.r4d_profile_num_classes()):
        ms, n, w = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        lib.r4d_profile_read(c, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
        if n.value:
            out[lib.r4d_profile_class_name(c).decode()] = dict(us=1e3 * ms.value / n.value, launches=n.value // reps,
                                                              gbs=w.value / (ms.value * 1e-3) / 1e9, work=w.value / n.value)
    lib.r4d_profile_enable(0)
    return wall, out


def emit(**kw):
    print(json.dumps(kw), flush=True)


def graph_wall(fn, iters=20, reps=5):
    """GPU-side time of one `fn()` launch sequence: `iters` back-to-back copies captured into one HIP graph (no Python
    or launch-API time between the kernels, only the GPU's own kernel-to-kernel gaps), replayed `reps` times."""
    fn(); torch.cuda.synchronize()
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        fn()
        st.synchronize()
        with torch.cuda.graph(g, stream=st):
            for _ in range(iters):
                fn()
    g.replay(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / (reps * iters)


def scan():
    s3 = ops.gemm_split3_enabled()                      # R4D_GEMM_SPLIT3=0: the exact-f32 form of the scan
    cases = [(12500, 512), (100000, 512), (12500, 768), (100000, 768)]
    if os.environ.get("R4D_SCAN_CASES"):
        cases = [tuple(int(x) for x in c.split("x")) for c in os.environ["R4D_SCAN_CASES"].split(",")]
    for N, d in cases:
        Q, k = 32, 10
        g = torch.Generator().manual_seed(1)
        q = ops.normalize_rows(torch.randn(Q, d, generator=g).to(dev))
        p = ops.normalize_rows(torch.randn(N, d, generator=g).to(dev))
        wall, pr = profile(lambda: ops.score_topk(q, p, k), 50)
        gw = float("nan") if os.environ.get("R4D_NO_GRAPH") else graph_wall(lambda: ops.score_topk(q, p, k))
        s = pr["pool_scan"]
        emit(component="scan", N=N, d=d, Q=Q, k=k, host_loop_wall_us=round(wall * 1e6, 1), gpu_wall_us=round(gw * 1e6, 2),
             kernel="pool_scan", kernel_us=round(s["us"], 2), algorithmic_bytes=s["work"],
             roofline={"bound": "hbm", "achieved": round(s["gbs"], 1), "peak": PEAK, "unit": "GB/s",
                       "frac": round(s["gbs"] / PEAK, 4)},
             topk_us=round(sum(v["us"] * v["launches"] for n, v in pr.items() if n == "topk"), 2),
             topk_launches=sum(v["launches"] for n, v in pr.items() if n == "topk"),
             operands="bf16x3" if s3 else "f32", env={k_: v for k_, v in os.environ.items() if k_.startswith("R4D_SCAN")},
             queries_per_s_scan_topk=round(Q / gw, 1))
    # full-row ranking (file-compat mode) at the north-star pool size
    S = torch.rand(32, 100000, generator=torch.Generator().manual_seed(2)).to(dev)
    wall, pr = profile(lambda: ops.argsort_desc(S), 5)
    emit(component="argsort", rows=32, n=100000, kernel_us=round(pr["argsort"]["us"], 1), wall_us=round(wall * 1e6, 1))


def topk():
    """Selection alone: per-round cost = slope over k."""
    for n in (12500, 100000):
        S = torch.rand(32, n, generator=torch.Generator().manual_seed(3)).to(dev)
        for k in (1, 10, 64):
            gw = graph_wall(lambda: ops.topk_f32(S, k))
            emit(component="topk", rows=32, n=n, k=k, gpu_wall_us=round(gw * 1e6, 2))


def topk_large():
    """Top-k beyond 64 per row (csrc/topk_large.hip) against the only other route to the same lists -- the full-row ranking
    ``ops.argsort_desc`` sliced to k plus the value gather -- with the k = 64 launch of the same rows as a scale.  HIP events
    around ``reps`` back-to-back calls after a warm-up, the three arms alternated over 5 rounds in one process, medians; the two
    routes' lists are compared before anything is timed."""
    import statistics
    for rows, n in ((256, 100000), (32, 100000), (2048, 12512)):
        S = torch.rand(rows, n, generator=torch.Generator().manual_seed(rows + n)).to(dev)
        for k in (100, 1024):
            def by_argsort():
                perm = ops.argsort_desc(S)[:, :k].long()
                return torch.gather(S, 1, perm), perm
            arms = {"topk_large": (lambda: ops.topk_f32(S, k), 20), "argsort_slice": (by_argsort, 3), "topk_k64": (lambda: ops.topk_f32(S, 64), 20)}
            a, b_ = arms["topk_large"][0](), by_argsort()
            assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]), (rows, n, k)
            us = {name: [] for name in arms}
            for _ in range(5):
                for name, (fn, reps) in arms.items():
                    fn(); torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _r in range(reps):
                        fn()
                    e1.record(); torch.cuda.synchronize()
                    us[name].append(e0.elapsed_time(e1) * 1e3 / reps)
            med = {name: round(statistics.median(v), 1) for name, v in us.items()}
            emit(component="topk_large", rows=rows, n=n, k=k, us=med, spread_us={name: [round(min(v), 1), round(max(v), 1)] for name, v in us.items()},
                 speedup_over_argsort=round(med["argsort_slice"] / med["topk_large"], 1), lists_equal=True)


def jaccard():
    from oracle import jaccard_ref
    g = np.load(os.path.join(REPO, "tests", "golden", "g5_jaccard_hepth.npz"))
    vocab = len(g["vocab_tokens"])
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("tr_out_ptr", "tr_out_idx", "tr_in_ptr", "tr_in_idx", "te_out_ptr", "te_out_idx")}
    cases = [("hepth train_out x train_out", "tr_out", "tr_out", True), ("hepth train_in x train_in", "tr_in", "tr_in", True),
             ("hepth test_out x train_out", "te_out", "tr_out", False)]
    for name, a, b, zd in cases:
        na, nb = t[a + "_ptr"].numel() - 1, t[b + "_ptr"].numel() - 1
        wall, pr = profile(lambda: ops.jaccard(t[a + "_ptr"], t[a + "_idx"], t[b + "_ptr"], t[b + "_idx"], vocab, zd), 20)
        j = pr["jaccard"]
        prep = pr.get("jaccard_prep")
        emit(component="jaccard", case=name, pairs=na * nb, kernel_us=round(j["us"], 2), pairs_per_s=round(na * nb / (j["us"] * 1e-6)),
             prep_us=round(prep["us"], 2) if prep else 0.0, call_wall_us=round(wall * 1e6, 1),
             roofline={"bound": "hbm", "achieved": round(j["gbs"], 1), "peak": PEAK, "unit": "GB/s", "frac": round(j["gbs"] / PEAK, 4)})
    # CPU baseline: the reference's single-thread double loop on a bounded sample of the same sets
    lists = [g["tr_out_idx"][g["tr_out_ptr"][i]:g["tr_out_ptr"][i + 1]].tolist() for i in range(len(g["tr_out_ptr"]) - 1)]
    t0 = time.perf_counter()
    jaccard_ref.occurrence_matrix_naive(lists[:600], lists)
    el = time.perf_counter() - t0
    emit(component="jaccard_cpu_baseline", kind="port", cores=1, sample="600 x 3965 hepth out-set pairs, python sets per pair",
         pairs_per_s=round(600 * len(lists) / el))
    # synthetic scale-up: 20,000 out-sets / in-sets, V0 = 11,901
    sh = synth.Shape("reddit_like", 11901, 11, 2, 8, 512, (8, 133, 512), (8, 133, 512))
    for kind, ins in (("out-sets", False), ("in-sets", True)):
        ptr, idx = synth.output_sets(sh, 20000, in_sets=ins)
        P, I = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
        wall, pr = profile(lambda: ops.jaccard(P, I, P, I, sh.v0, True), 5)
        j = pr["jaccard"]
        prep = pr.get("jaccard_prep")
        emit(component="jaccard", case=f"synthetic 20000 x 20000 {kind} (mean size {idx.size / 20000:.1f})", pairs=4e8,
             kernel_us=round(j["us"], 1), pairs_per_s=round(4e8 / (j["us"] * 1e-6)),
             prep_us=round(prep["us"], 2) if prep else 0.0, call_wall_us=round(wall * 1e6, 1),
             roofline={"bound": "hbm", "achieved": round(j["gbs"], 1), "peak": PEAK, "unit": "GB/s", "frac": round(j["gbs"] / PEAK, 4)})


def pool():
    sys.path.insert(0, REPO)
    from bench import build_model
    from rag4dyg_amd.retrieval import encode_batches, right_pad_batches
    for name in ("UCI_13", "wikiv2"):
        shape = synth.SHAPES[name]
        m = build_model(shape, dev)
        seqs = synth.sequences(shape, 12500, "pool", seed=2026)
        b = right_pad_batches(seqs, 32, shape.pad_id, dev)
        encode_batches(m, b[:40]); torch.cuda.synchronize()
        t0 = time.perf_counter()
        encode_batches(m, b)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        emit(component="pool_encode", shape=name, sequences=12500, padded_tokens=int(sum(x.numel() for x in b)),
             seqs_per_s=round(12500 / el, 1))


def _alternate(arms, run, rounds=5):
    """``arms``: name -> (encode precision, gemm mode[, encode activation store, default "fp32"]); ``run()`` -> (seconds of device
    time, units of work).  Every arm in every round, round after round; -> name -> list of rates."""
    out = {n: [] for n in arms}
    for _ in range(rounds):
        for n, (prec, mode, *store) in arms.items():
            ops.set_encode_precision(prec); ops.set_gemm_mode(mode); ops.set_encode_act_store(store[0] if store else "fp32")
            el, work = run()
            out[n].append(work / el)
    return out


def encode_precision():
    """The opt-in bf16 precision of the encoder forward (ops.set_encode_precision) beside the default f16x2 and bf16x3:
    (a) bench.py's encode step -- ``encode_groups_meanpool`` of 8 query batches of 32 -- on the UCI_13 and wikiv2 shapes, device
    events around 10 steps behind 2 warm-up steps, the arms alternated over 5 rounds; with the per-class launch times of one arm;
    (b) val-mode greedy decode (SimpleDyG loop, 11 tokens per prompt, batches of 32) at the UCI_13 generator model L6 H8 d768:
    tokens/s, wall clock around a synchronised batch loop;
    (c) recorded, not gated: the bf16 top-10 lists on the real UCI_13 (G4) and wikiv2 (G12) fixtures against the golden lists;
    (d) the attention kernels alone (``attention_alone``).
    The "bf16+attn" arm's baseline is the "bf16" arm of the SAME run: the third word touches neither its kernels nor its routing.
    The arms "bf16 | act" and "bf16+attn | act" are those two words with ``ops.set_encode_act_store("bf16")`` (ln1 / ln2 / the GELU
    output stored as bf16: the same bits); THEIR baseline is the same word's store-off arm of the same run, in (a) and (b)."""
    import statistics
    from bench import build_model
    from oracle import gpt2_ref
    from rag4dyg_amd.evaluation import greedy_decode_batch
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel, GPT2LMHeadModelRAG
    from rag4dyg_amd.retrieval import PoolIndex, encode_batches, right_pad_batches
    was = (ops.encode_precision(), ops.gemm_mode(), ops.encode_act_store())
    arms = {"bf16": ("bf16", "f16x2"), "bf16 | act": ("bf16", "f16x2", "bf16"), "bf16+attn": ("bf16+attn", "f16x2"),
            "bf16+attn | act": ("bf16+attn", "f16x2", "bf16"), "f16x2": ("fp32", "f16x2"), "bf16x3": ("fp32", "bf16x3")}
    med = lambda v: statistics.median(v)
    try:
        for name in ("UCI_13", "wikiv2"):
            shape = synth.SHAPES[name]
            m = build_model(shape, dev)
            qb = right_pad_batches(synth.sequences(shape, 32 * 96, "query", seed=9000), 32, shape.pad_id, dev)
            groups = [qb[i:i + 8] for i in range(0, len(qb), 8)]
            rows = sum(b.numel() for g_ in groups[2:] for b in g_) / 10.0

            def run():
                for g_ in groups[:2]:
                    m.encode_groups_meanpool(g_)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for g_ in groups[2:]:
                    m.encode_groups_meanpool(g_)
                b.record(); torch.cuda.synchronize()
                return a.elapsed_time(b) * 1e-3, 10.0
            rates = _alternate(arms, run)
            ms = {n: [1e3 / r for r in v] for n, v in rates.items()}
            ops.set_encode_precision("bf16"); ops.set_gemm_mode("f16x2"); ops.set_encode_act_store("fp32")
            _wall, classes = profile(lambda: m.encode_groups_meanpool(groups[2]), 5)
            ops.set_encode_precision("bf16+attn")
            _wall, classes_attn = profile(lambda: m.encode_groups_meanpool(groups[2]), 5)
            share = lambda cl, k: round(cl[k]["us"] * cl[k]["launches"] / sum(v["us"] * v["launches"] for v in cl.values()), 4) if k in cl else None
            emit(component="encode_step", shape=name, batches_per_step=8, mean_token_rows_per_step=round(rows),
                 ms_per_step={n: round(med(v), 3) for n, v in ms.items()}, ms_min_max={n: [round(min(v), 3), round(max(v), 3)] for n, v in ms.items()},
                 bf16_over_f16x2=round(med(ms["bf16"]) / med(ms["f16x2"]), 3), bf16_over_bf16x3=round(med(ms["bf16"]) / med(ms["bf16x3"]), 3),
                 bf16attn_over_bf16=round(med(ms["bf16+attn"]) / med(ms["bf16"]), 3),
                 act_over_off={n: round(med(ms[n + " | act"]) / med(ms[n]), 3) for n in ("bf16", "bf16+attn")},
                 attention_share_of_kernel_time={"bf16": share(classes, "attn_fused"), "bf16+attn": share(classes_attn, "attn_b1")},
                 bf16_arm_classes={k: dict(us=round(v["us"], 1), launches=v["launches"]) for k, v in classes.items()},
                 bf16attn_arm_classes={k: dict(us=round(v["us"], 1), launches=v["launches"]) for k, v in classes_attn.items()})
        # (b) val-mode decode
        shape = synth.SHAPES["UCI_13"]
        L, H, d, V = 6, 8, 768, shape.vocab
        sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=4, random_affine=True)
        model = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H))
        model.load_state_dict(sd, strict=False); model.tie_weights()
        model = model.to(dev).eval()
        import types
        tok = types.SimpleNamespace(encode=lambda s_: [shape.v0])
        prompts = [s_.tolist() for s_ in synth.sequences(shape, 256, "query", seed=2)]

        def run_decode():
            greedy_decode_batch(model, tok, prompts[:32], "val", 1024, 12, dev); torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
            for b0 in range(0, len(prompts), 32):
                outs = greedy_decode_batch(model, tok, prompts[b0:b0 + 32], "val", 1024, 12, dev)
                n += sum(len(o) - len(p) for o, p in zip(outs, prompts[b0:b0 + 32]))
            torch.cuda.synchronize()
            return time.perf_counter() - t0, float(n)
        tps = _alternate(arms, run_decode, rounds=3)
        emit(component="val_decode", shape="UCI_13", model=f"L{L} H{H} d{d} V{V}", prompts=len(prompts), batch=32,
             mean_prompt_len=round(float(np.mean([len(p) for p in prompts])), 1),
             tokens_per_s={n: round(med(v), 1) for n, v in tps.items()},
             act_over_off={n: round(med(tps[n + " | act"]) / med(tps[n]), 3) for n in ("bf16", "bf16+attn")}, tokens_per_s_min_max={n: [round(min(v), 1), round(max(v), 1)] for n, v in tps.items()})
        # (c) real-data retrieval under bf16 against the golden top-10 lists
        gold = os.path.join(REPO, "tests", "golden")
        unrag = lambda flat, off: [flat[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
        for fixture, tokens in (("g4_uci_retrieval", "g6_uci_tokens"), ("g12_wikiv2_retrieval", "g6_wikiv2_tokens")):
            g, k = np.load(os.path.join(gold, fixture + ".npz")), np.load(os.path.join(gold, tokens + ".npz"))
            if fixture.startswith("g4"):
                L, H, d, V, ref10 = 4, 2, 512, 1801, g["top10_stable"]
            else:
                (L, H, d, V), ref10 = (int(x) for x in g["cfg"]), g["top32_idx"][:, :10]
            sd = gpt2_ref.make_state_dict(L, d, V, seed=int(g["seed"]), random_affine=True)
            m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H))
            m.load_state_dict(sd, strict=False); m.tie_weights()
            m = m.to(dev).eval()
            pad = int(k["pad_id"])
            res = {}
            ops.set_encode_act_store("fp32")
            for n, (prec, mode, *store) in arms.items():
                if store:                                                # the same bits as the store-off arm (tests/test_gpu_encode_bf16_act.py)
                    continue
                ops.set_encode_precision(prec); ops.set_gemm_mode(mode)
                pool = encode_batches(m, right_pad_batches(unrag(k["pool_flat"], k["pool_off"]), 32, pad, dev))
                q = encode_batches(m, right_pad_batches(unrag(k["test_flat"], k["test_off"]), 32, pad, dev))
                idx = PoolIndex(pool).search(q, 10)[1].cpu().numpy()
                inter = [len(set(a.tolist()) & set(b.tolist())) for a, b in zip(idx, ref10)]
                res[n] = dict(mean_overlap_of_10=round(float(np.mean(inter)), 3), min_overlap=int(min(inter)),
                              lists_identical=round(float((idx == ref10).all(axis=1).mean()), 4), top1_identical=round(float((idx[:, 0] == ref10[:, 0]).mean()), 4))
            emit(component="retrieval_top10_vs_golden", fixture=fixture, queries=int(ref10.shape[0]), pool=int(len(k["pool_off"]) - 1), **res)
        attention_alone()
    finally:
        ops.set_encode_precision(was[0]); ops.set_gemm_mode(was[1]); ops.set_encode_act_store(was[2])


def attention_alone():
    """The encoder attention of ONE layer alone: one batch of 256 sequences of T tokens in ONE launch per arm, d = 512 (768 at head
    dim 96) -- the exact-f32 kernel the "bf16" word runs (``ops.attention``: ``launch_attention_fused``, the grouped launch with one
    group) against ``ops.attention_bf16`` on fp32 and on bf16 qkv; device events around 20 calls behind 3 warm-ups, the arms
    alternated over 5 rounds, medians."""
    import statistics
    g = torch.Generator().manual_seed(0)
    for hd in (64, 96, 128, 256):
        d = 768 if hd == 96 else 512
        H = d // hd
        for T in (128, 340):
            B = 256
            qkv = torch.randn(B * T, 3 * d, generator=g).to(dev)
            qbf = qkv.bfloat16()
            q3 = qkv.view(B, T, 3 * d)
            arms = {"exact_f32": lambda: ops.attention(q3, H), "bf16_attn_fp32_qkv": lambda: ops.attention_bf16(qkv, [(B, T)], H, out_bf16=True),
                    "bf16_attn_bf16_qkv": lambda: ops.attention_bf16(qbf, [(B, T)], H)}
            us = {n: [] for n in arms}
            for _ in range(5):
                for n, fn in arms.items():
                    for _w in range(3):
                        fn()
                    torch.cuda.synchronize()
                    a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _r in range(20):
                        fn()
                    b_.record(); torch.cuda.synchronize()
                    us[n].append(a.elapsed_time(b_) * 1e3 / 20)
            med = {n: round(statistics.median(v), 1) for n, v in us.items()}
            emit(component="attention_alone", head_dim=hd, d=d, H=H, T_longest=T, sequences=B, token_rows=B * T, us_per_layer=med,
                 us_min_max={n: [round(min(v), 1), round(max(v), 1)] for n, v in us.items()},
                 bf16_qkv_over_exact=round(med["bf16_attn_bf16_qkv"] / med["exact_f32"], 3),
                 fp32_qkv_over_exact=round(med["bf16_attn_fp32_qkv"] / med["exact_f32"], 3))


def encode_step_trace(word="bf16", shape_name="UCI_13", store="fp32"):
    """12 encode steps of the bench shape under ``word`` (gemm mode f16x2) and the activation ``store``, nothing else on the
    device: for a kernel trace."""
    from bench import build_model
    from rag4dyg_amd.retrieval import right_pad_batches
    shape = synth.SHAPES[shape_name]
    m = build_model(shape, dev)
    qb = right_pad_batches(synth.sequences(shape, 32 * 96, "query", seed=9000), 32, shape.pad_id, dev)
    ops.set_encode_precision(word); ops.set_gemm_mode("f16x2"); ops.set_encode_act_store(store)
    for i in range(0, len(qb), 8):
        m.encode_groups_meanpool(qb[i:i + 8])
    torch.cuda.synchronize()
    emit(component="encode_step_trace", word=word, store=store, shape=shape_name, steps=len(qb) // 8)


def generator(shape_name="UCI_13", L=6, H=8, d=768, topk=7, pool_n=512):
    """RAG generator inference (graph-pooling fusion of top-7 retrieved sequences + greedy decode, val
    mode = 11 tokens per query, batch 1 like the reference) on UCI_13-shaped synthetic data, model L6 H8 d768
    (scripts/train_generator/train_rag_graphpooling_UCI_seed.sh), next to the oracle on the host cores."""
    import types
    from oracle import generator_ref, gpt2_ref
    from rag4dyg_amd import generator as gen
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    shape = synth.SHAPES[shape_name]
    V = shape.vocab_generator if shape_name == "reddit" else shape.vocab
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=4, random_affine=True)
    model = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H))
    model.load_state_dict(sd, strict=False); model.tie_weights()
    gnn = model.get_gnn(d, d // 2, d, 1, 0.2)
    convs = [(gnn.convs[0].lin.weight.detach().clone(), gnn.convs[0].bias.detach().clone())]
    model = model.to(dev).eval()
    pool_seqs = [s.tolist() for s in synth.sequences(shape, pool_n, "pool", seed=1)]
    queries = [s.tolist() for s in synth.sequences(shape, 256, "query", seed=2)]
    rng = np.random.default_rng(0)
    idxs = [rng.permutation(pool_n)[:topk].tolist() for _ in queries]
    ds = types.SimpleNamespace(retrieval_sources=pool_seqs)
    args = types.SimpleNamespace(fusion="graphpooling", m=1, topK=topk)
    tok = types.SimpleNamespace(encode=lambda s: [shape.v0], pad_token_id=shape.pad_id)     # <|endoftext|> = V0
    eos = tok.encode("")[0]

    def run_gpu(qs):
        n = 0
        for q, ix in qs:
            out = gen.greedy_decode_rag(args, model, tok, ds, q, ix, "val", 1024, 12)
            n += len(out) - len(q)
        torch.cuda.synchronize()
        return n
    run_gpu(list(zip(queries[:4], idxs[:4])))
    t0 = time.perf_counter()
    ntok1 = run_gpu(list(zip(queries[:16], idxs[:16])))
    el1 = time.perf_counter() - t0
    batches = [(queries[b0:b0 + 32], idxs[b0:b0 + 32]) for b0 in range(0, len(queries), 32)]     # --per_gpu_eval_batch_size 32
    list(gen.decode_rag_batches(args, model, tok, ds, batches[:3], "val", 1024, 12))                # warm-up (both decoder slots, graphs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ntok = 0
    for (qs, _ix), outs in zip(batches, gen.decode_rag_batches(args, model, tok, ds, batches, "val", 1024, 12)):
        ntok += sum(len(o) - len(q) for o, q in zip(outs, qs))
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    # the same queries at --per_gpu_eval_batch_size 128 (the throughput lever of a latency-bound step: same ids per query)
    big = [(queries[b0:b0 + 128], idxs[b0:b0 + 128]) for b0 in range(0, len(queries), 128)]
    list(gen.decode_rag_batches(args, model, tok, ds, big[:2], "val", 1024, 12)); torch.cuda.synchronize()
    t0 = time.perf_counter()
    ntok128 = 0
    for (qs, _ix), outs in zip(big, gen.decode_rag_batches(args, model, tok, ds, big, "val", 1024, 12)):
        ntok128 += sum(len(o) - len(q) for o, q in zip(outs, qs))
    torch.cuda.synchronize()
    el128 = time.perf_counter() - t0
    t0 = time.perf_counter()
    ncpu = 0
    for q, ix in list(zip(queries, idxs))[:3]:
        fn = lambda t, ix=ix: generator_ref.fusion_graphpooling_embeds(sd, pool_seqs, t, ix, topk, convs)
        out = generator_ref.greedy_decode_rag(sd, H, fn, q, eos, "val", 1024, 12)
        ncpu += len(out) - len(q)
    elc = time.perf_counter() - t0
    emit(component="generator_decode", shape=shape_name, model=f"L{L} H{H} d{d} V{V}", pool=pool_n, fusion="graphpooling", topK=topk,
         queries=len(queries), mean_query_len=round(float(np.mean([len(q) for q in queries])), 1), tokens=ntok,
         tokens_per_s=round(ntok / el, 1), queries_per_s=round(len(queries) / el, 2), batch=32,
         tokens_per_s_batch1=round(ntok1 / el1, 1), tokens_per_s_batch128=round(ntok128 / el128, 1),
         cpu_baseline={"kind": "port", "cores": host_cores(), "tokens_per_s": round(ncpu / elc, 2),
                       "sample": "3 queries, oracle torch-CPU fp32 (fusion + full forward per token, as the reference)"})



def simpledyg_eval():
    """SimpleDyG greedy link-prediction decode (utils/Evaluation_SimpleDyG.py:120-145) at BASELINE config 1's model
    (L6 H8 d768 V1800): test-set histories of the UCI_13 length distribution, val mode (11 tokens per query) and test mode
    (until <|endoftext|> or the context limit; random-init weights rarely emit it, so this is the long-generation case), batch 32,
    next to the oracle's one-at-a-time loop on the host cores."""
    import types
    from oracle import gpt2_ref
    from rag4dyg_amd import evaluation
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    shape = synth.SHAPES["UCI_13"]
    L, H, d, V = 6, 8, 768, shape.vocab - 1                    # SimpleDyG omits [MASK] (main_SimpleDyG.py:91-95)
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=9, random_affine=True)
    model = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H))
    model.load_state_dict(sd, strict=False); model.tie_weights()
    model = model.to(dev).eval()
    queries = [s.tolist() for s in synth.sequences(shape, 256, "query", seed=3)]
    tok = types.SimpleNamespace(encode=lambda s: [shape.v0], pad_token_id=shape.pad_id)
    out = {}
    for mode, budget in (("val", None), ("test", 160)):
        max_len = 1024 if mode == "val" else None
        evaluation.greedy_decode_batch(model, tok, queries[:32], mode, 1024 if mode == "val" else max(len(q) for q in queries[:32]) + budget, 0, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ntok = 0
        for b0 in range(0, len(queries), 32):
            qs = queries[b0:b0 + 32]
            ml = 1024 if mode == "val" else max(len(q) for q in qs) + budget      # test mode: a context limit `budget` tokens past the longest prompt
            outs = evaluation.greedy_decode_batch(model, tok, qs, mode, ml, 0, dev)
            ntok += sum(len(o) - len(q) for o, q in zip(outs, qs))
        torch.cuda.synchronize()
        out[mode] = (ntok, time.perf_counter() - t0)
    t0 = time.perf_counter()
    ncpu = 0
    for q in queries[:2]:
        ncpu += len(gpt2_ref.greedy_decode(sd, H, q, shape.v0, "val")) - len(q)
    elc = time.perf_counter() - t0
    emit(component="simpledyg_greedy_eval", shape="UCI_13", model=f"L{L} H{H} d{d} V{V}", queries=len(queries), batch=32,
         val_tokens_per_s=round(out["val"][0] / out["val"][1], 1), val_queries_per_s=round(len(queries) / out["val"][1], 1),
         test_tokens=out["test"][0], test_tokens_per_s=round(out["test"][0] / out["test"][1], 1),
         cpu_baseline={"kind": "port", "cores": host_cores(), "tokens_per_s": round(ncpu / elc, 2),
                       "sample": "2 queries, val mode, oracle torch-CPU fp32 (full forward per token, as the reference)"})


def generator_reddit():
    """BASELINE config 5 shape: reddit t=11, L2 H8 d512, V = 11,919, pool 10,527, top-7 (the script) and top-5 (BASELINE.json)."""
    generator("reddit", 2, 8, 512, 7, 10527)
    generator("reddit", 2, 8, 512, 5, 10527)


_JAC_CPU = r"""
import json, os, sys, time, multiprocessing as mp
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import jaccard_ref
cores = int(sys.argv[2])
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "g5_jaccard_hepth.npz"))
lists = [g["tr_out_idx"][g["tr_out_ptr"][i]:g["tr_out_ptr"][i + 1]].tolist() for i in range(len(g["tr_out_ptr"]) - 1)]
rows = 150 * cores
blocks = [lists[i:i + 150] for i in range(0, rows, 150)]
t0 = time.perf_counter()
with mp.get_context("fork").Pool(cores) as pool:
    pool.starmap(jaccard_ref.occurrence_matrix_naive, [(b_, lists) for b_ in blocks])
el = time.perf_counter() - t0
print(json.dumps({"rows": rows, "cols": len(lists), "seconds": el}))
"""


TRAINING_MODE_KEYS = ("attention", "activations", "precision", "attention_kernel")      # the axes of training.TRAIN_MODE_AXES this entry takes


def training(**modes):
    """(``--attention stored|recompute``, ``--activations stored|recompute``, ``--precision fp32|bf16|fp32+attn|bf16+attn``,
    ``--attention-kernel products|fused``: the ``EncoderTrainer``'s mode keywords of those names, words and meanings in
    ``rag4dyg_amd.training.TRAIN_MODE_AXES``; the line reports the four words, the trainer's workspace bytes and torch's peak
    allocated bytes.)  SURVEY 8f-4: one retriever training iteration (five forwards with saved activations, losses, encoder backward, clip,
    AdamW) at the UCI_13 script's shape (L4 H2 d512, batch 64: scripts/train_retriever/train_retriever_UCI_13.sh:8-12) on
    synthetic UCI_13-length sequences.  flop = 3 x the forward's algorithmic encoder flop (forward + dX + dW) of the five
    padded batches; wall clock includes the host side of the step (aug, loss autograd over [5, B, d], ~40 optimizer launches)."""
    import random
    import types
    from bench import build_model, f_enc
    from rag4dyg_amd import training as tr
    from rag4dyg_amd.retrieval import right_pad_batches
    shape = synth.SHAPES["UCI_13"]
    B = 64
    m = build_model(shape, dev)
    m.config.eta, m.config.gamma = 0.8, 0.4
    nb = 22
    seqs = synth.sequences(shape, 3 * B * nb, "query", seed=11)
    args = types.SimpleNamespace(device=dev, temperature=0.1, lambda_decay=1e-4, alpha=1.0, per_gpu_train_batch_size=B,
                                 max_grad_norm=1.0, gradient_accumulation_steps=1)
    times = (torch.rand(3 * B * nb) * 1e4).to(dev)
    batches = []
    for i in range(nb):
        trip = [right_pad_batches(seqs[(3 * i + j) * B:(3 * i + j + 1) * B], B, shape.pad_id, "cpu")[0] for j in range(3)]   # as the DataLoader hands them over
        idx = [torch.arange((3 * i + j) * B, (3 * i + j + 1) * B).view(B, 1) for j in range(3)]
        batches.append((*trip, *idx))
    n = nb - 2
    flop = sum(3.0 * (f_enc(shape, B, b[0].shape[1]) * 3 + f_enc(shape, B, b[1].shape[1]) + f_enc(shape, B, b[2].shape[1]))
               for b in batches[2:])
    wall = {}
    torch.cuda.reset_peak_memory_stats()
    for mode in ("warm", "eval", "train"):               # "train": model.train(), dropout 0.1 at the four sites like the reference
        m.train(mode == "train")
        trainer = tr.EncoderTrainer(m, seed=42, **modes)
        opt = tr.AdamW(trainer.params, trainer.grads, lr=1e-5, eps=1e-8, weight_decay=0.0, flat_grads=trainer.flat_grads)
        random.seed(0)
        for b in batches[:2]:
            tr.training_step(args, m, trainer, opt, b, times)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in batches[2:]:
            tr.training_step(args, m, trainer, opt, b, times, sync=False)      # as train_epoch runs it: losses summed on the device
        torch.cuda.synchronize()
        wall[mode] = time.perf_counter() - t0
    el = wall["train"]
    # device-side split of one step (forward / backward / optimizer) with events
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    b = batches[2]
    a1, a2 = tr.aug(b[0], 0.8, 0.4, m.config.vocab_size - 1)
    torch.cuda.synchronize()
    ev[0].record()
    emb = trainer.forward([x.to(dev) for x in (b[0], b[1], b[2], a1, a2)])
    ev[1].record()
    trainer.backward(torch.randn_like(emb))
    ev[2].record()
    opt.step(1.0)
    ev[3].record()
    torch.cuda.synchronize()
    emit(component="retriever_training_step", shape="UCI_13", batch=B, steps=n, dropout=0.1, ms_per_step=round(1e3 * el / n, 3),
         sequences_per_s=round(5 * B * n / el, 1), tflops=round(flop / el / 1e12, 1),
         ms_per_step_dropout_off=round(1e3 * wall["eval"] / n, 3),
         forward_ms=round(ev[0].elapsed_time(ev[1]), 3), backward_ms=round(ev[1].elapsed_time(ev[2]), 3),
         optimizer_ms=round(ev[2].elapsed_time(ev[3]), 3), padded_T=[int(x.shape[1]) for x in b[:3]],
         **{k: getattr(trainer, k) for k in TRAINING_MODE_KEYS}, workspace_bytes=int(trainer._ws.numel()),
         max_memory_allocated=int(torch.cuda.max_memory_allocated()))


def training_cpu():
    """The same training iteration on the host cores: the oracle's grad-enabled forward + torch CPU autograd + the restated
    AdamW (oracle/train_ref.py), ONE step at batch 16 of the same sequence distribution (bounded sample)."""
    import random
    from oracle import gpt2_ref, train_ref
    shape = synth.SHAPES["UCI_13"]
    B = 16
    cores = host_cores()
    torch.set_num_threads(cores)
    sd = gpt2_ref.make_state_dict(shape.n_layer, shape.n_embd, shape.vocab, n_positions=1024, seed=3)
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    seqs = synth.sequences(shape, 3 * B, "query", seed=11)

    def pad(chunk):
        T = max(len(e) for e in chunk)
        b = torch.full((len(chunk), T), int(shape.pad_id), dtype=torch.int64)
        for i, e in enumerate(chunk):
            b[i, :len(e)] = torch.as_tensor(e)
        return b
    a, p_, n_ = pad(seqs[:B]), pad(seqs[B:2 * B]), pad(seqs[2 * B:])
    idx = torch.arange(3 * B).view(3, B).t().contiguous()
    t0 = time.perf_counter()
    r = train_ref.training_step(sd, shape.n_head, a, p_, n_, torch.rand(3 * B) * 1e4, idx, 0.8, 0.4, 1.0, 0.1, 1e-4,
                                shape.vocab - 1, 0, with_grad=True)
    r["loss"].backward()
    names = [k for k in sd if sd[k].grad is not None]
    coef, _ = train_ref.clip_coefficient([sd[k].grad for k in names], 1.0)
    for k in names:
        train_ref.adamw_step(sd[k].detach(), sd[k].grad * coef, torch.zeros_like(sd[k]), torch.zeros_like(sd[k]), 1, 1e-5)
    el = time.perf_counter() - t0
    emit(component="retriever_training_step_cpu", kind="port", cores=cores, shape="UCI_13", batch=B,
         sample=f"one step, batch {B} (5 x {B} sequences), padded T = {[int(a.shape[1]), int(p_.shape[1]), int(n_.shape[1])]}",
         seconds=round(el, 2), sequences_per_s=round(5 * B / el, 2))


def jaccard_cpu_all_cores():
    """the reference's python-set double loop (retrieval_data_annotation.py:36-41) on ALL host cores (row blocks in
    a process pool, started from a fresh interpreter that never touches the GPU) next to the single-thread line of jaccard()."""
    import subprocess
    cores = host_cores()
    out = subprocess.run([sys.executable, "-c", _JAC_CPU, REPO, str(cores)], capture_output=True, text=True, check=True).stdout
    r = json.loads(out.strip().splitlines()[-1])
    emit(component="jaccard_cpu_baseline", kind="port", cores=cores,
         sample=f"{r['rows']} x {r['cols']} hepth out-set pairs, python sets per pair, {cores} processes",
         pairs_per_s=round(r["rows"] * r["cols"] / r["seconds"]))


if __name__ == "__main__":
    from rag4dyg_amd.training import TRAIN_MODE_AXES
    for axis in TRAIN_MODE_AXES:                                                  # training entry only
        flag = "--" + axis.key.replace("_", "-")
        if axis.key in TRAINING_MODE_KEYS and flag in sys.argv:
            i = sys.argv.index(flag)
            if sys.argv[i + 1] not in axis.words:
                sys.exit(f"{flag}: {' or '.join(axis.words)}")
            training = functools.partial(training, **{axis.key: sys.argv[i + 1]})
            del sys.argv[i:i + 2]
    if sys.argv[1:2] == ["encode_step_trace"]:                                    # takes its word (and shape) as arguments
        encode_step_trace(*sys.argv[2:5])
        sys.exit(0)
    for part in (sys.argv[1:] or ["scan", "topk", "jaccard", "jaccard_cpu", "pool", "generator", "generator_reddit", "simpledyg", "training", "training_cpu"]):
        {"scan": scan, "topk": topk, "topk_large": topk_large, "jaccard": jaccard, "jaccard_cpu": jaccard_cpu_all_cores, "pool": pool, "encode_precision": encode_precision, "attention_alone": attention_alone, "encode_step_trace": encode_step_trace, "generator": generator,
         "generator_reddit": generator_reddit, "simpledyg": simpledyg_eval, "training": training, "training_cpu": training_cpu}[part]()

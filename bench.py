#!/usr/bin/env python3
"""Headline benchmark: query-sequences/sec, encode + top-k over the full (sharded) pool.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A STEP is one pass of the hot path over one batch of synthetic input, per rank:
  G (default 4) query batches of 32 UCI_13-shaped sequences (reference batching: each right-padded to its
  own batch max, train_retriever.py:425-432) -> GPT-2 encoder (L4 H2 d512, fp32; the row-wise kernels run
  over the concatenated rows of the G batches) + fused ln_f/mean-pool -> row normalise ->
  [N>1: RCCL all-gather of the query embeddings] -> (S+1)/2 cosine scan of the rank's resident pool shard ->
  canonical top-10 -> [N>1: RCCL all-gather of the per-shard top-k + merge].
Inputs (token ids, the pre-encoded pool shard) are resident in HBM before the timed region.  The pool is the
north-star 100,000-sequence pool at EVERY N: one GPU holds all of it (205 MB of fp32 embeddings), N GPUs hold
contiguous batch-aligned shards of it (12,500 rows each at N = 8).  Weak scaling in the unit of the metric: every
rank encodes its own G x 32 queries per step and scans its shard for the queries of all ranks, so per-GPU work is
fixed as N grows.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the steps and prints the line (``roofline`` and ``cpu_baseline`` null).  ``--full`` adds
everything else after the timed steps: rooflines, the other arithmetics, the CPU baseline and the verification runs.
``--dump-outputs DIR`` writes the last timed step's top-k to DIR as .npy; inputs are seeded, so runs with the same
arguments can be compared output for output.
"""
import hashlib
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from rag4dyg_amd import _lib, ops, synth                      # noqa: E402
from rag4dyg_amd.dist import PipelinedShardedTopK, all_gather_cat, sharded_topk      # noqa: E402
from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG    # noqa: E402
from rag4dyg_amd.retrieval import PoolIndex, encode_batches, right_pad_batches   # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md, dense f32 matrix peak
PEAK_BF16_MFMA_TFLOPS = 2500.0   # same guide: dense bf16 matrix peak (the 2:1-sparsity figure is not used)
# the bf16x3 GEMM spends SIX bf16 products per fp32 product: its ceiling in fp32-equivalent flop is the bf16 peak / 6
PEAK_S3_TFLOPS = round(PEAK_BF16_MFMA_TFLOPS / 6.0, 1)
# the f16x2 GEMM spends THREE fp16 products per fp32 product (same dense peak as bf16): fp16 peak / 3
PEAK_H2_TFLOPS = round(PEAK_BF16_MFMA_TFLOPS / 3.0, 1)
DTYPES = {"f16x2": "f32 (f16x2 operands: two fp16 terms, three products, f32 accumulate)",
          "bf16x3": "f32 (bf16x3 operands, f32 accumulate)", "f32": "f32"}
PEAK_HBM_GBS = 8000.0
QB = 32                          # per_gpu_eval_batch_size, utils/args_parser_retriever.py:225


def build_model(shape, device):
    torch.manual_seed(1234)      # N(0, 0.02) weights, zero biases, LN 1/0 (modeling_gpt2.py:251-262); random-init
    cfg = GPT2Config(vocab_size=shape.vocab, n_positions=1024, n_ctx=1024, n_embd=shape.n_embd,
                     n_layer=shape.n_layer, n_head=shape.n_head)
    return GPT2LMHeadModelRAG(cfg).to(device).eval()


def mfma_peak(kernel):
    return PEAK_H2_TFLOPS if kernel.startswith("gemm_h2") else PEAK_S3_TFLOPS if kernel.startswith("gemm_s3") else PEAK_F32_MFMA_TFLOPS


def f_enc(shape, B, T):
    """Algorithmic encoder flop of a padded [B,T] batch: L*(24*T*d^2 + 2*T^2*d) per sequence."""
    d, L = shape.n_embd, shape.n_layer
    return B * L * (24.0 * T * d * d + 2.0 * T * T * d)


def read_profile():
    import ctypes
    lib = _lib.load()
    out = {}
    for c in range(lib.r4d_profile_num_classes()):
        ms, n, w = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        _lib.check(lib.r4d_profile_read(c, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w)), "profile_read")
        if n.value:
            out[lib.r4d_profile_class_name(c).decode()] = dict(ms=ms.value, launches=n.value, work=w.value)
    return out


def host_cores():
    """Cores this process may actually use: min(affinity mask, cgroup cpu.max quota)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(model, shape, query_seqs, pool_emb, k, first_batches=(), budget_s=12.0):
    """The oracle (CPU port of the reference path) timed on this host's cores on a bounded sample.  Like the reference
    (train_retriever.py:419: ``_, h = model(input_ids)`` computes lm_logits and throws them away) the forward INCLUDES
    the lm_head GEMM; the rate without it is reported beside it.  ``first_batches``: indices of the query batches to take
    first (the LAST timed step's): their oracle scores and stable top-k are returned for the in-run verification."""
    from oracle import gpt2_ref, retrieval_ref
    sd = {k_: v.detach().cpu() for k_, v in model.state_dict().items()}
    pool = pool_emb.cpu()
    torch.set_num_threads(host_cores())
    nqb = len(query_seqs) // QB
    order = list(first_batches) + [b for b in range(nqb) if b not in set(first_batches)]
    done, t0 = 0, time.perf_counter()
    nb, t_head = 0, 0.0
    kept = {}
    for bi in order:
        chunk = query_seqs[bi * QB:(bi + 1) * QB]
        b = retrieval_ref.right_pad_batches(chunk, QB, shape.pad_id)
        embs = []
        for ids in b:                                               # retrieval_ref.encode_batches + the discarded lm_head
            with torch.no_grad():
                out = gpt2_ref.gpt2_forward(sd, ids, shape.n_head, want_logits=False)
                th = time.perf_counter()
                torch.matmul(out["hidden"], sd["transformer.wte.weight"].t())      # modeling_rag.py:675, result unused
                t_head += time.perf_counter() - th
            embs.append(out["hidden"].mean(dim=1))
        S = retrieval_ref.score_batch(torch.cat(embs), pool).numpy()
        top = retrieval_ref.topk_stable(S, k)
        if bi in first_batches:
            kept[bi] = (S, top[1])
        done += len(chunk)
        nb += 1
        if time.perf_counter() - t0 > budget_s and nb >= len(first_batches):
            break
    el = time.perf_counter() - t0
    return {"value": round(done / el, 2), "unit": "query-seqs/s", "cores": torch.get_num_threads(), "kind": "port",
            "value_without_lm_head": round(done / (el - t_head), 2),
            "sample": f"{nb} query batches of {QB} (same synthetic {shape.name}-shape inputs, same resident pool of "
                      f"{pool.shape[0]} rows), oracle torch-CPU fp32 encode INCLUDING the lm_head GEMM the reference computes "
                      f"and discards + score + stable top-{k}, {el:.1f} s"}, kept


def verify_one_gpu(kept, first_batches, last_out, model, q_batches, index, k):
    """N = 1, after the timed region: the LAST timed step's ranked top-k against the oracle's stable top-k of the same
    queries (the CPU baseline computes them anyway): fraction of rows whose whole list is identical and the largest ORACLE
    score gap at any mismatching position (tests/conftest.rank_mismatch_report semantics; pass = gap <= 2e-6); plus the two
    ways of batching the queries into scoring calls against each other (32 per call, all 256 in one call): ONE scoring arithmetic,
    the same bits."""
    S = np.concatenate([kept[b][0] for b in first_batches]).astype(np.float64)
    ref_idx = np.concatenate([np.asarray(kept[b][1]) for b in first_batches]).astype(np.int64)
    got_idx = last_out[1].cpu().numpy()
    got_val = last_out[0].cpu().numpy().astype(np.float64)
    same = ref_idx == got_idx
    gap = 0.0
    for r, c in zip(*np.nonzero(~same)):
        gap = max(gap, abs(S[r, ref_idx[r, c]] - S[r, got_idx[r, c]]))
    ref_val = np.take_along_axis(S, ref_idx, axis=1)
    emb = model.encode_groups_meanpool([q_batches[b] for b in first_batches])
    q_hat = ops.normalize_rows(emb)
    v_gemm, i_gemm, _ = ops.score_topk(q_hat, index.pool_hat, k, index.index_offset)
    parts = [ops.score_topk(q_hat[j:j + QB], index.pool_hat, k, index.index_offset) for j in range(0, q_hat.shape[0], QB)]
    i_scan = torch.cat([p_[1] for p_ in parts])
    v_scan = torch.cat([p_[0] for p_ in parts])
    scan_gap = float((v_scan - v_gemm).abs().max())
    return {"queries": int(ref_idx.shape[0]), "pool_rows": int(S.shape[1]), "topk": k,
            "rows_identical_to_oracle": round(float(same.all(axis=1).mean()), 4),
            "max_oracle_score_gap_at_mismatch": gap, "pass": bool(gap <= 2e-6),
            "max_abs_score_err_vs_oracle": float(np.abs(got_val - ref_val).max()),
            "timed_step_equals_recomputation": bool(torch.equal(i_gemm, last_out[1]) and torch.equal(v_gemm, last_out[0])),
            "rows_identical_across_query_batchings": round(float((i_scan == i_gemm).all(dim=1).float().mean()), 4),
            "max_abs_score_diff_across_query_batchings": scan_gap}


def verify_sharded(world, rank, device, index, last_out, model, q_batches, args, G, k, gather, elapsed_local):
    """N > 1, after the timed region: (1) the process group really has `--gpus` ranks on distinct devices, (2) the merged
    top-k of the LAST timed step equals what ONE GPU computes over the whole pool (rank 0 gathers every shard and rescans:
    bit-exact values and indices), (3) per-rank wall time of the timed region (load spread)."""
    assert dist.get_world_size() == args.gpus == world
    dev_ids = [None] * world
    dist.all_gather_object(dev_ids, (rank, torch.cuda.current_device(), torch.cuda.get_device_properties(device).name))
    times = [None] * world
    dist.all_gather_object(times, elapsed_local)
    # the last timed step's queries, recomputed (deterministic): step index = steps - 1
    i = args.steps - 1
    nqb = len(q_batches)
    emb = model.encode_groups_meanpool([q_batches[(i * G + j) % nqb] for j in range(G)])
    q_all = gather(ops.normalize_rows(emb))
    all_rows = [None] * world
    dist.all_gather_object(all_rows, int(index.pool_hat.shape[0]))
    nmax = max(all_rows)
    pad = torch.zeros(nmax, index.pool_hat.shape[1], dtype=torch.float32, device=device)
    pad[:index.pool_hat.shape[0]] = index.pool_hat
    stacked = gather(pad).view(world, nmax, -1)                      # every rank receives every shard (205 MB at 100k x 512)
    full = torch.cat([stacked[r, :all_rows[r]] for r in range(world)])
    v1, i1, _ = ops.score_topk(q_all, full, k, 0)
    mine = bool(torch.equal(i1, last_out[1]) and torch.equal(v1, last_out[0]))
    oks = [None] * world
    dist.all_gather_object(oks, mine)
    ok = all(oks)
    if not ok and rank == 0:
        print(f"[bench] VERIFY FAILED: sharded top-k differs from the one-GPU recomputation on ranks {[r for r, o in enumerate(oks) if not o]}",
              file=sys.stderr)
    ms = [1e3 * t_ / args.steps for t_ in times]
    # the step's two collectives on their own, HIP-event timed on this rank (embeddings: Q*d*4 B per rank; candidates: Q*k*12 B, values and indices in ONE tensor)
    coll = {}
    try:
        cand_v = torch.zeros(q_all.shape[0], k, dtype=torch.float32, device=device)
        cand_i = torch.zeros(q_all.shape[0], k, dtype=torch.int64, device=device)
        q_loc = q_all[:q_all.shape[0] // world].contiguous()
        from rag4dyg_amd.dist import pack_candidates, unpack_candidates
        for name, fn in (("all_gather_embeddings_us", lambda: gather(q_loc)),
                         ("all_gather_candidates_us", lambda: unpack_candidates(gather(pack_candidates(cand_v, cand_i)), k))):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            coll[name] = round(e0.elapsed_time(e1) * 1e3 / 20, 1)
        coll["rccl_version"] = ".".join(str(x) for x in torch.cuda.nccl.version()) if dist.get_backend() == "nccl" else None
        coll["backend"] = dist.get_backend()
    except Exception as e:                                           # noqa: BLE001
        coll["error"] = f"{type(e).__name__}: {e}"
    return {"world_size": world, "collectives": coll, "devices": sorted({d[1] for d in dev_ids}), "device_names": sorted({d[2] for d in dev_ids}),
            "sharded_topk_equals_one_gpu": ok, "pool_rows_checked": int(sum(all_rows)),
            "per_rank_ms_per_step": [round(x, 3) for x in ms],
            "rank_spread": round((max(ms) - min(ms)) / max(ms), 4)}


def source_sha():
    """sha256 over the kernel sources and the C ABI header: what a PMC traffic figure was profiled on."""
    h = hashlib.sha256()
    csrc = os.path.join(REPO, "rag4dyg_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        h.update(open(os.path.join(csrc, f), "rb").read())
    h.update(open(os.path.join(REPO, "include", "r4d.h"), "rb").read())
    return h.hexdigest()[:16]


def scan_q32(index, shape, k, device, reps=50):
    """The north-star kernel on its own roofline: the (S+1)/2 cosine scan of the rank's RESIDENT pool shard at the
    reference's query batch (32) + top-k, HIP-event timed per launch on the launch stream (r4d_profile hooks)."""
    lib = _lib.load()
    q = ops.normalize_rows(torch.randn(QB, shape.n_embd, generator=torch.Generator().manual_seed(5)).to(device))
    for _ in range(5):
        ops.score_topk(q, index.pool_hat, k, index.index_offset)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ops.score_topk(q, index.pool_hat, k, index.index_offset)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    lib.r4d_profile_enable(1)
    for _ in range(reps):
        ops.score_topk(q, index.pool_hat, k, index.index_offset)
    torch.cuda.synchronize()
    prof = read_profile()
    lib.r4d_profile_enable(0)
    sc, tk = prof["pool_scan"], prof.get("topk", {"ms": 0.0, "launches": 1})
    n_rows = int(index.pool_hat.shape[0])
    scan_s, topk_s = sc["ms"] * 1e-3 / sc["launches"], tk["ms"] * 1e-3 / sc["launches"]
    b_survey = 4.0 * n_rows * shape.n_embd + 4.0 * QB * shape.n_embd + 8.0 * QB * k       # B_score
    b_moved = sc["work"] / sc["launches"]                                                 # + the [Q,N] score rows the kernel writes
    gbs = b_moved / scan_s / 1e9
    traffic = None                                    # PMC bytes of a separate rocprofv3 pass on the same sources and size, else null
    tf = os.path.join(REPO, "profiles", "pmc_scan.json")
    if os.path.exists(tf):
        pmc = json.load(open(tf))
        if pmc.get("_workload", {}).get("source_sha") == source_sha():
            traffic = pmc.get(f"{n_rows}x{shape.n_embd}", {}).get("hbm_bytes_per_launch")
    return {"pool_rows": n_rows, "d": shape.n_embd, "queries": QB, "topk": k,
            "scan_kernel_us": round(scan_s * 1e6, 2), "topk_kernel_us": round(topk_s * 1e6, 2),
            "host_loop_wall_us": round(wall * 1e6, 1), "algorithmic_bytes": b_survey, "bytes_moved": b_moved,
            "roofline": {"kernel": "pool_scan", "bound": "hbm", "achieved": round(b_survey / scan_s / 1e9, 1), "peak": PEAK_HBM_GBS,
                         "unit": "GB/s", "frac": round(b_survey / scan_s / 1e9 / PEAK_HBM_GBS, 4),
                         "frac_survey": round(b_survey / scan_s / 1e9 / PEAK_HBM_GBS, 4),       # SURVEY's B_score / scan kernel time
                         "frac_moved": round(gbs / PEAK_HBM_GBS, 4),                            # incl. the score rows written
                         "frac_scan_plus_topk": round(b_survey / (scan_s + topk_s) / 1e9 / PEAK_HBM_GBS, 4),
                         "traffic": traffic}}


def scan_q32_shard8(index, shape, k, device):
    """N = 1 only: the north-star PARTITION on the one GPU the driver has.  The resident pool cut into the eight batch-aligned
    shards an 8-GPU run would hold (``dist.shard_bounds``): the scan + top-k of shard 0 timed exactly like ``scan_q32`` (the
    12,512-row size the north star's "40 % of the HBM roofline" is quoted for), and the eight per-shard top-k lists (each found
    with its global offset) merged by the HIP merge and compared with the one-GPU top-k -- the data path of N = 8 minus the
    all-gather."""
    import types
    from rag4dyg_amd.dist import shard_bounds
    n = int(index.pool_hat.shape[0])
    bounds = shard_bounds(n, 8)
    s0, e0 = bounds[0]
    out = scan_q32(types.SimpleNamespace(pool_hat=index.pool_hat[s0:e0], index_offset=index.index_offset + s0), shape, k, device)
    q = ops.normalize_rows(torch.randn(QB, shape.n_embd, generator=torch.Generator().manual_seed(6)).to(device))
    v1, i1, _ = ops.score_topk(q, index.pool_hat, k, index.index_offset)
    cv, ci = [], []
    for s_, e_ in bounds:
        v_, i_, _ = ops.score_topk(q, index.pool_hat[s_:e_], k, index.index_offset + s_)
        cv.append(v_); ci.append(i_)
    mv, mi = ops.merge_topk(torch.stack(cv), torch.stack(ci))
    out["shard_rows"] = [e_ - s_ for s_, e_ in bounds]
    out["eight_shard_merge_equals_one_gpu"] = bool(torch.equal(mi, i1) and torch.equal(mv, v1))
    return out


def scan_operating_points(index, shape, k, device, reps=20):
    """N = 1 only: scan + top-k at the sizes the bench's steps REALLY run.  ``step_q256`` -- the 256 queries of a
    step against the whole resident pool (N = 1); ``n8_rank_q2048_shard`` -- what ONE rank of the 8-GPU weak-scaling run does per step:
    the 2,048 gathered queries against its 12,512-row shard.  HIP-event timed per kernel class; reported against the bf16x3 MFMA
    ceiling (2,500 / 6 TFLOP/s of fp32-equivalent flop) AND against one read of the shard at the HBM peak -- not against SURVEY's
    per-32-query ``B_score``, which would credit every 32-query block with its own read of the pool."""
    from rag4dyg_amd.dist import shard_bounds
    lib = _lib.load()
    n, d = int(index.pool_hat.shape[0]), shape.n_embd
    s0, e0 = shard_bounds(n, 8)[0]
    out = {}
    for name, Q, pool in (("step_q256", QB * 8, index.pool_hat), ("n8_rank_q2048_shard", QB * 64, index.pool_hat[s0:e0])):
        q = ops.normalize_rows(torch.randn(Q, d, generator=torch.Generator().manual_seed(7)).to(device))
        rows = int(pool.shape[0])
        for _ in range(3):
            ops.score_topk(q, pool, k, 0)
        torch.cuda.synchronize()
        lib.r4d_profile_enable(1)
        for _ in range(reps):
            ops.score_topk(q, pool, k, 0)
        torch.cuda.synchronize()
        prof = read_profile()
        lib.r4d_profile_enable(0)
        sc, tk = prof["pool_scan"], prof.get("topk", {"ms": 0.0, "launches": 1})
        scan_s, topk_s = sc["ms"] * 1e-3 / reps, tk["ms"] * 1e-3 / reps
        flop = 2.0 * Q * rows * d
        out[name] = {"queries": Q, "pool_rows": rows, "d": d, "scan_kernel_us": round(scan_s * 1e6, 1), "topk_kernel_us": round(topk_s * 1e6, 1),
                     "scan_TFLOPs_fp32_equiv": round(flop / scan_s / 1e12, 1), "frac_of_bf16x3_mfma_ceiling": round(flop / scan_s / 1e12 / 416.7, 3),
                     "one_read_of_the_shard_GBps": round(4.0 * rows * d / scan_s / 1e9, 1),
                     "frac_of_hbm_peak_one_read": round(4.0 * rows * d / scan_s / 1e9 / PEAK_HBM_GBS, 4)}
    return out


def gemm_zero_operand_probe(shape, rows, device, reps=20):
    """Outside the timed region, f16x2 only: the step's c_attn GEMM (rows x d x 3d) on N(0,1) operands and the SAME launch on all-zero
    operands -- identical instructions, addresses and bytes, no switching activity in the multipliers.  The ratio is what the clock
    the chip sustains under fp16 MFMA load on real data costs this kernel."""
    d = shape.n_embd
    out = {"M": rows, "K": d, "N": 3 * d}
    b = torch.zeros(3 * d, device=device)
    for kind in ("normal", "zeros"):
        x = torch.randn(rows, d, device=device) if kind == "normal" else torch.zeros(rows, d, device=device)
        w = torch.randn(d, 3 * d, device=device) * 0.02 if kind == "normal" else torch.zeros(d, 3 * d, device=device)
        planes = ops.split2_planes(w)
        for _ in range(4):
            ops.conv1d_h2(x, planes, b)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.conv1d_h2(x, planes, b)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        out[kind + "_us"] = round(us, 1)
        out[kind + "_TFLOPs"] = round(2.0 * rows * d * 3 * d / us / 1e6, 1)
    out["zeros_over_normal_speed"] = round(out["normal_us"] / out["zeros_us"], 3)
    return out


def dump_outputs(out_dir, out):
    """What a caller of the timed path receives from its last step: the merged top-k of every query of the step (all ranks'
    queries at N > 1).  Indices are global pool rows, exact in float64."""
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "topk_values.npy"), out[0].cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "topk_indices.npy"), out[1].cpu().numpy().astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="UCI_13", choices=sorted(synth.SHAPES))
    ap.add_argument("--pool-total", type=int, default=100000,
                    help="rows of the whole pool (north star: 100k); rank r holds the r-th batch-aligned shard")
    ap.add_argument("--pool-per-gpu", type=int, default=0, help="override: fixed shard rows per rank (pool = N x this)")
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batches-per-step", type=int, default=8,
                    help="reference query batches (32 sequences each, padded independently) handed to the library per step "
                         "as one fused launch sequence")
    ap.add_argument("--query-batches", type=int, default=256,
                    help="distinct synthetic query batches cycled over the steps (256 x 32 = the 8192 queries of SURVEY 8d)")
    ap.add_argument("--gemm", default="f16x2", choices=["f16x2", "split3", "f32"],
                    help="arithmetic of the encoder's Conv1D GEMMs, all at fp32 accuracy (error against float64 no larger than the "
                         "exact-f32 kernel's: profiles/r04_h2_acceptance.md).  f16x2 (default): fp16 matrix cores, two fp16 terms per "
                         "operand, three products; split3: bf16 matrix cores, three bf16 terms, six products; f32: the exact-f32 MFMA "
                         "kernels.  The line of a split mode carries the other modes' runs in extras (exact_f32, bf16x3)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak (the metric's form): every rank encodes --batches-per-step batches per step; strong: the SAME "
                         "64 batches (2048 queries) per step split over the ranks, so total work is fixed as N grows")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--random-pool", action="store_true",
                    help="profiling aid: fill the resident pool shard with N(0,1) embeddings instead of encoding the "
                         "synthetic pool, so that a rocprofv3 trace holds the timed-step kernels only")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-bucketed", action="store_true", help="skip the length-bucketed second run (extras.length_bucketed)")
    ap.add_argument("--no-exact-f32", action="store_true", help="skip the second timed run on the exact-f32 MFMA kernels (extras.exact_f32)")
    ap.add_argument("--headline-only", action="store_true",
                    help="profiling aid: warm-up + timed steps and nothing else, so that a rocprofv3 --kernel-trace --stats of this "
                         "command averages the headline launches only (what a run without --full does anyway)")
    ap.add_argument("--no-verify", action="store_true",
                    help="N > 1: skip the post-run check that the sharded top-k equals a one-GPU recomputation on rank 0")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run everything the headline does not need: the HIP-event roofline pass, the "
                         "other arithmetics, the scan rooflines, the zero-operand probe, the length-bucketed run, the CPU baseline "
                         "and the verification against the oracle (N = 1) or a one-GPU recomputation (N > 1); the --no-* options "
                         "switch parts of it off")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's top-k (topk_values.npy float32, topk_indices.npy float64; [queries, topk]) "
                         "to DIR")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.headline_only or not args.full:
        args.no_roofline = args.no_bucketed = args.no_exact_f32 = args.no_cpu_baseline = args.no_verify = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run for N>1")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    dev_index = local_rank % torch.cuda.device_count()              # == local_rank on a full node
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    backend = os.environ.get("R4D_BENCH_BACKEND", "nccl")           # "nccl" IS RCCL on ROCm; "gloo" = functional
    if world > 1:                                                    # rehearsal of the N>1 path on a 1-GPU box only
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=device)
        else:
            dist.init_process_group(backend=backend)
    _lib.load()
    ops.set_gemm_mode({"f16x2": "f16x2", "split3": "bf16x3", "f32": "f32"}[args.gemm])

    shape = synth.SHAPES[args.shape]
    model = build_model(shape, device)
    k = args.topk

    # --- resident pool shard: this rank's contiguous, batch-aligned run of the global pool, encoded with reference batching
    if args.pool_per_gpu > 0:
        P, p_off, pool_total = args.pool_per_gpu, rank * args.pool_per_gpu, args.pool_per_gpu * world
    else:
        from rag4dyg_amd.dist import shard_bounds
        pool_total = args.pool_total
        p_off, p_end = shard_bounds(pool_total, world)[rank]
        P = p_end - p_off
    if args.random_pool:
        pool_emb = torch.randn(P, shape.n_embd, generator=torch.Generator().manual_seed(2026 + rank)).to(device)
        pool_encode_s = float("nan")
    else:
        # every rank derives the SAME global pool (one seed) and keeps its own rows, so the sharded run scans exactly the
        # pool the one-GPU run scans; with --pool-per-gpu each rank draws its own fixed-size shard instead
        if args.pool_per_gpu > 0:
            pool_seqs = synth.sequences(shape, P, "pool", seed=2026 + rank)
        else:
            pool_seqs = synth.sequences(shape, pool_total, "pool", seed=2026)[p_off:p_off + P]
        pool_batches = right_pad_batches(pool_seqs, QB, shape.pad_id, device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool_emb = encode_batches(model, pool_batches)
        torch.cuda.synchronize()
        pool_encode_s = time.perf_counter() - t0
        del pool_batches
    index = PoolIndex(pool_emb, index_offset=p_off)

    # --- query batches resident in HBM
    q_seqs = synth.sequences(shape, QB * args.query_batches, "query", seed=9000 + rank)
    q_batches = right_pad_batches(q_seqs, QB, shape.pad_id, device)

    G = args.batches_per_step
    if args.scaling == "strong":
        if 64 % world:
            raise SystemExit("--scaling strong splits 64 batches per step over the ranks: N must divide 64")
        G = 64 // world
    nqb = len(q_batches)

    if world > 1 and backend != "nccl":
        import rag4dyg_amd.dist as rdist                            # rehearsal only: stage the two collectives through
        _orig = rdist.all_gather_cat                                # host memory, compute stays on the GPU

        def _host_gather(t, group=None):
            return _orig(t.cpu(), group).to(t.device)
        rdist.all_gather_cat = _host_gather
        gather = _host_gather
    else:
        gather = all_gather_cat

    def local_topk(q, p_, kk, off):
        return ops.score_topk(q, p_, kk, off)[:2]

    # N > 1 over RCCL: the two collectives of a step run asynchronously, each consumed one step later
    # (rag4dyg_amd.dist.PipelinedShardedTopK), so ranks whose batches happen to be longer this step do not stall the
    # others twice per step.  All K steps are still complete inside the timed region (flush before the closing sync).
    # R4D_BENCH_PIPELINE=0 selects the step-synchronous form; a failing self-test falls back to it as well.
    pipe = None
    pipe_env = os.environ.get("R4D_BENCH_PIPELINE", "1")              # "force": also under the gloo rehearsal backend
    if world > 1 and pipe_env != "0" and (backend == "nccl" or pipe_env == "force"):
        try:
            pipe = PipelinedShardedTopK(index.pool_hat, index.index_offset, k, local_topk, ops.merge_topk)
            probe = ops.normalize_rows(torch.randn(QB * G, shape.n_embd, device=device))
            got = [r for r in (pipe.submit(probe), pipe.submit(probe)) if r is not None] + pipe.flush()
            ref = sharded_topk(gather(probe), index.pool_hat, index.index_offset, k, local_topk, ops.merge_topk)
            torch.cuda.synchronize()
            assert len(got) == 2 and got[0][1].shape == (QB * G * world, k)
            assert all(torch.equal(g_[0], ref[0]) and torch.equal(g_[1], ref[1]) for g_ in got), "pipelined != synchronous"
        except Exception as e:                                        # noqa: BLE001 -- never lose the run to the overlap
            if rank == 0:
                print(f"[bench] pipelined collectives unavailable ({type(e).__name__}: {e}); using the synchronous form",
                      file=sys.stderr)
            pipe = None
        agree = torch.tensor([1 if pipe is not None else 0], dtype=torch.int32, device=device)
        dist.all_reduce(agree, op=dist.ReduceOp.MIN)                   # every rank takes the same form, or none does
        if int(agree.item()) == 0:
            pipe = None

    def step(i):
        group = [q_batches[(i * G + j) % nqb] for j in range(G)]
        emb = model.encode_groups_meanpool(group)
        q_hat = ops.normalize_rows(emb)
        if pipe is not None:
            return pipe.submit(q_hat)
        q_all = gather(q_hat) if world > 1 else q_hat
        return sharded_topk(q_all, index.pool_hat, index.index_offset, k, local_topk, ops.merge_topk)

    def drain():
        return pipe.flush() if pipe is not None else []

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_run():
        for i in range(args.warmup):
            step(i)
        drain()
        sync()
        t0 = time.perf_counter()
        for i in range(args.steps):
            out_ = step(i)
        tail = drain()                                               # the last two steps' results: inside the timed region
        if tail:
            out_ = tail[-1]
        sync()
        el = time.perf_counter() - t0
        el_local = el
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        assert out_[1].shape == (QB * G * world, k)
        return out_, el, el_local

    def roofline_run():
        """The same K steps again with per-launch HIP events on the launch stream (r4d_profile hooks)."""
        lib = _lib.load()
        lib.r4d_profile_enable(1)
        for i in range(args.steps):
            step(i)
        drain()
        torch.cuda.synchronize()
        prof = read_profile()
        lib.r4d_profile_enable(0)
        kernels_ = {}
        tot_ms = sum(v["ms"] for v in prof.values())
        for name, v in prof.items():
            is_mfma = name.startswith(("gemm", "attn"))
            rate = v["work"] / (v["ms"] * 1e-3) if v["ms"] > 0 else 0.0
            kernels_[name] = {"share": round(v["ms"] / tot_ms, 4), "launches": v["launches"],
                              "avg_us": round(1e3 * v["ms"] / v["launches"], 2),
                              ("TFLOP/s" if is_mfma else "GB/s"): round(rate / (1e12 if is_mfma else 1e9), 2)}
        dom = max(prof, key=lambda n: prof[n]["ms"])
        v = prof[dom]
        traffic, util = None, None
        sfx = {"f16x2": "_f16x2", "bf16x3": "", "f32": "_f32"}[ops.gemm_mode()]     # every arithmetic has its own PMC pass
        tf = os.path.join(REPO, "profiles", f"pmc_traffic_{args.shape}{sfx}.json")
        if not os.path.exists(tf):
            tf = os.path.join(REPO, "profiles", f"pmc_traffic{sfx}.json")
        if os.path.exists(tf):              # PMC figure of a separate rocprofv3 pass: valid for the workload AND the sources
            pmc = json.load(open(tf))       # it was profiled on only -- otherwise null
            meta = pmc.get("_workload", {})
            if (meta.get("shape") == args.shape and meta.get("batches_per_step") == G and meta.get("n_gpus", 1) == world
                    and meta.get("pool_rows_per_gpu") == P and meta.get("source_sha") == source_sha()
                    and meta.get("gemm", "f32") == {"f16x2": "f16x2", "bf16x3": "split3", "f32": "f32"}[ops.gemm_mode()]):
                traffic = pmc.get(dom, {}).get("hbm_bytes_per_launch")
                util = pmc.get(dom, {}).get("mfma_pipe_util")
        if dom.startswith(("gemm", "attn")):
            ach = v["work"] / (v["ms"] * 1e-3) / 1e12
            peak = mfma_peak(dom)
            roof = {"kernel": dom, "bound": "mfma", "achieved": round(ach, 2), "peak": peak,
                    "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": traffic,
                    "avg_launch_us": round(1e3 * v["ms"] / v["launches"], 2),
                    "flop_per_launch": v["work"] / v["launches"]}
            if dom.startswith("gemm_h2"):
                roof["peak_note"] = ("fp32-equivalent flop; f16x2: three v_mfma_f32_32x32x16_f16 products per fp32 product, so the "
                                     "ceiling is the dense fp16 MFMA peak (2500 TFLOP/s) / 3")
                roof["x_exact_f32_peak"] = round(ach / PEAK_F32_MFMA_TFLOPS, 4)
            if dom.startswith("gemm_s3"):
                roof["peak_note"] = ("fp32-equivalent flop; bf16x3: six v_mfma_f32_32x32x16_bf16 products per fp32 product, "
                                     "so the ceiling is the dense bf16 MFMA peak (2500 TFLOP/s) / 6")
                roof["x_exact_f32_peak"] = round(ach / PEAK_F32_MFMA_TFLOPS, 4)
            if util is not None:
                roof["mfma_pipe_busy_pmc"] = round(util, 4)
        else:
            ach = v["work"] / (v["ms"] * 1e-3) / 1e9
            roof = {"kernel": dom, "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": traffic,
                    "avg_launch_us": round(1e3 * v["ms"] / v["launches"], 2),
                    "bytes_per_launch": v["work"] / v["launches"]}
        return roof, kernels_

    ops.take_range_flag()
    out, elapsed, elapsed_local = timed_run()
    # range guard (include/r4d.h, ABI v6): the device word every encode / normalise of the WHOLE timed region ORs into, read once
    # here (the steps themselves stay asynchronous): non-zero = a non-finite hidden state or an embedding that could not be normalised
    range_word = ops.take_range_flag()
    if range_word:
        raise SystemExit(f"[bench] range guard word {range_word:#x} after the timed region: results are not valid")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)

    roofline, kernels = None, {}
    if not args.no_roofline:
        roofline, kernels = roofline_run()

    # --- N = 1: the same timed region once more on every OTHER arithmetic (the lines the headline is read against): the exact-f32
    # MFMA kernels always, bf16x3 as well when the headline is f16x2
    exact = other_s3 = None
    if world == 1 and args.gemm != "f32" and not args.no_exact_f32:
        head_mode = ops.gemm_mode()
        for mode in (["bf16x3"] if args.gemm == "f16x2" else []) + ["f32"]:
            ops.set_gemm_mode(mode)
            out_f, el_f, _ = timed_run()
            roof_f, kern_f = roofline_run() if not args.no_roofline else (None, {})
            same = (out_f[1] == out[1]).all(dim=1).float().mean()
            rec = {"dtype": DTYPES[mode], "value": round(QB * G * args.steps / el_f, 2), "unit": "query-seqs/s",
                   "ms_per_step": round(1e3 * el_f / args.steps, 4), "roofline": roof_f,
                   "dominant_kernel_share": kern_f.get(roof_f["kernel"], {}).get("share") if roof_f else None,
                   "top10_rows_identical_to_headline": round(float(same), 4),
                   "max_abs_score_diff_vs_headline": float((out_f[0] - out[0]).abs().max())}
            if mode == "f32":
                exact = rec
            else:
                other_s3 = rec
        ops.set_gemm_mode(head_mode)

    # --- N > 1: correctness bit + load spread, outside the timed region (never allowed to lose the run)
    verify = None
    if world > 1 and not args.no_verify:
        try:
            verify = verify_sharded(world, rank, device, index, out, model, q_batches, args, G, k, gather, elapsed_local)
        except Exception as e:                                       # noqa: BLE001
            verify = {"error": f"{type(e).__name__}: {e}"}
    scan = scan8 = scan_ops = None
    if rank == 0 and not args.no_roofline:
        scan = scan_q32(index, shape, k, device)
        if world == 1 and int(index.pool_hat.shape[0]) >= 8 * 64:
            scan8 = scan_q32_shard8(index, shape, k, device)
            try:
                scan_ops = scan_operating_points(index, shape, k, device)
            except Exception as e:                                   # noqa: BLE001
                scan_ops = {"error": f"{type(e).__name__}: {e}"}
    power_probe = None
    if rank == 0 and world == 1 and not args.no_roofline and args.gemm == "f16x2":
        try:
            power_probe = gemm_zero_operand_probe(shape, int(sum(int(b.numel()) for b in q_batches[:G])), device)
        except Exception as e:                                       # noqa: BLE001
            power_probe = {"error": f"{type(e).__name__}: {e}"}
    # --- SURVEY 8d's second, "length-bucketed" run (N = 1): the SAME queries sorted by length before they are cut into
    # batches of 32, so a batch pads to similar lengths.  NOT parity-comparable with the reference (an embedding is a mean
    # over its batch's padded positions) and never the headline value: it shows what the reference's file-order batching costs.
    bucketed = None
    if world == 1 and rank == 0 and not args.no_roofline and not args.no_bucketed:
        order = sorted(range(len(q_seqs)), key=lambda j: len(q_seqs[j]))
        b_batches = right_pad_batches([q_seqs[j] for j in order], QB, shape.pad_id, device)
        nb = len(b_batches)

        def bstep(i):
            emb = model.encode_groups_meanpool([b_batches[(i * G + j) % nb] for j in range(G)])
            return sharded_topk(ops.normalize_rows(emb), index.pool_hat, index.index_offset, k, local_topk, ops.merge_topk)
        for i in range(args.warmup):
            bstep(i)
        torch.cuda.synchronize()
        tb = time.perf_counter()
        for i in range(args.steps):
            bstep(i)
        torch.cuda.synchronize()
        eb = time.perf_counter() - tb
        Tb = [int(b.shape[1]) for b in b_batches]
        Tb_steps = [Tb[(i * G + j) % nb] for i in range(args.steps) for j in range(G)]
        bucketed = {"value": round(QB * G * args.steps / eb, 2), "unit": "query-seqs/s", "ms_per_step": round(1e3 * eb / args.steps, 4),
                    "mean_padded_T": round(float(np.mean(Tb_steps)), 1),
                    "note": "same queries sorted by length before batching: not parity-comparable with the reference's file-order "
                            "batches (mean over padded positions), reported beside the headline value only"}
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        last = [((args.steps - 1) * G + j) % nqb for j in range(G)]     # the query batches of the last timed step
        first = last if not args.no_verify and len(set(last)) == G else []
        cpu, kept = cpu_baseline(model, shape, [s.tolist() for s in q_seqs], pool_emb, k, first_batches=first)
        if first:
            try:
                verify = verify_one_gpu(kept, first, out, model, q_batches, index, k)
                if not verify["pass"]:
                    print(f"[bench] VERIFY FAILED: top-{k} differs from the oracle beyond fp32 noise: {verify}", file=sys.stderr)
            except Exception as e:                                   # noqa: BLE001 -- never lose the run to the check
                verify = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0:
        Ts = [int(b.shape[1]) for b in q_batches]
        steps_T = [Ts[(i * G + j) % len(Ts)] for i in range(args.steps) for j in range(G)]
        enc_flop = sum(f_enc(shape, QB, T) for T in steps_T)
        line = {
            "metric": "query-seqs/sec encode+top-k over full pool",
            "value": round(world * QB * G * args.steps / elapsed, 2),
            "unit": "query-seqs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": DTYPES[ops.gemm_mode()], "data": "synthetic",
            "config": {"workload": f"{shape.name}-shape synthetic sequences, SimpleDyG GPT-2 L{shape.n_layer} H{shape.n_head} "
                                   f"d{shape.n_embd} V{shape.vocab} random-init fp32 weights and activations; per rank and step {G} reference query batches of {QB} "
                                   f"(each padded to its own batch max, mean T={np.mean(Ts):.0f}; one fused launch sequence) "
                                   f"encode+mean-pool+normalise, cosine scan of a "
                                   f"resident {P}-row shard of the {pool_total}-row pool, top-{k}; N>1: RCCL all-gather of embeddings "
                                   f"and per-shard top-k",
                       "query_batch": QB, "query_batches_per_step": G, "queries_per_step_per_gpu": QB * G,
                       "distinct_query_batches": nqb, "pool_rows_per_gpu": P, "pool_rows_total": pool_total, "topk": k,
                       "parallelism": f"pool-shard x{world}",
                       "collectives": ("none" if world == 1 else
                                       "async, consumed one step later (3-stage pipeline)" if pipe is not None else "synchronous")},
            "roofline": roofline,
            "cpu_baseline": cpu,
            "extras": {"source_sha": source_sha(), "gemm": args.gemm,
                       "attention": ("f16x2 (q, k, v as h2 words, two v_mfma_f32_32x32x16_f16 per 8 elements; csrc/attention_h2.hip)"
                                     if args.gemm == "f16x2" and (shape.n_embd // shape.n_head) in (128, 256) else "exact f32 (v_mfma_f32_32x32x2_f32)"),
                       "range_guard_word_after_timed_region": range_word, "exact_f32": exact, "bf16x3": other_s3, "scan_q32": scan, "scan_q32_shard8": scan8, "scan_operating_points": scan_ops, "gemm_zero_operand_probe": power_probe, "verify": verify,
                       "length_bucketed": bucketed,
                       "encoder_algorithmic_TFLOPs_per_gpu": round(enc_flop / elapsed / 1e12, 2),
                       "pool_encode_seqs_per_s_per_gpu": None if args.random_pool else round(P / pool_encode_s, 1),
                       "kernels": kernels},
        }
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

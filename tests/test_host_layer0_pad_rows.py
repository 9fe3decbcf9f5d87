"""Host side of the layer-0 pad-row path (``include/r4d.h``: r4d_set_layer0_pad_rows): what the bench's own batches give the
classification, and the size of the encoder workspaces.  No GPU."""
import ctypes

import numpy as np

from _layer0_pad_rows_ref import classify, plan_words, round_up, workspace_bytes


def _padded(seqs, pad_id, batch=32):
    out = []
    for s in range(0, len(seqs), batch):
        chunk = seqs[s:s + batch]
        b = np.full((len(chunk), max(len(e) for e in chunk)), pad_id, np.int64)
        for i, e in enumerate(chunk):
            b[i, :len(e)] = e
        out.append(b)
    return out


def test_bench_batches_give_the_quoted_pad_block_fractions():
    """256 reference batches of 32 (file order, each padded to its own longest sequence) of the bench's query (seed 9000) and
    pool (seed 2026) sequences, UCI_13: the share of [PAD] rows and of 32-row blocks that hold nothing else -- the work the
    layer-0 c_attn launch drops.  The estimate in DESIGN.md 4.2 rests on these; a change of ``synth`` that moves them shows here."""
    from rag4dyg_amd import synth
    sh = synth.UCI_13
    for kind, seed, rows_want, blocks_want in (("query", 9000, 0.699, 0.584), ("pool", 2026, 0.819, 0.599)):
        batches = _padded(synth.sequences(sh, 32 * 256, kind, seed=seed), sh.pad_id)
        rows = sum(b.size for b in batches)
        pad_rows = sum(int((b == sh.pad_id).sum()) for b in batches) / rows
        dropped = blocks = 0
        for i in range(0, len(batches), 8):                          # the bench hands the library 8 batches per call
            r = classify(batches[i:i + 8])
            assert r["c"] == sh.pad_id                               # 31 of 32 sequences of a batch end in [PAD]
            assert r["M"] % 32 == 0 and r["listed"].size % 4 == 0
            dropped += r["dropped"].size
            blocks += r["Mp"] // 32
        print(kind, "pad rows %.4f" % pad_rows, "pad-only blocks %.4f" % (dropped / blocks), "rows", rows)
        assert abs(pad_rows - rows_want) < 0.005, (kind, pad_rows)
        assert abs(dropped / blocks - blocks_want) < 0.005, (kind, dropped / blocks)
    q = _padded(synth.sequences(sh, 32 * 256, "query", seed=9000), sh.pad_id)
    assert abs(np.mean([b.shape[1] for b in q]) - 250.4) < 0.1


def test_classification_reference_on_small_cases():
    pad = 9
    a = np.full((3, 48), pad)
    a[0, :48] = np.arange(48) % 7                                    # rows 0..47 real; rows 48..50 and 96..98 real, the rest [PAD]
    a[1:, :3] = 1
    r = classify([a])                                                # M = 144: block 2 (rows 64..95) is pad only, block 4 is partial
    assert r["c"] == pad and r["dropped"].tolist() == [2] and r["kept"].tolist() == [0, 1, 3, 4]
    assert r["listed"].tolist() == [0, 1, 3, 4, 5, 6, 6, 6]          # then the table blocks of Tcap = 64 behind M' = 160, padded to 8
    b = np.full((1, 40), 5)                                          # M = 40: block 0 all fives, block 1 partial -> kept
    r = classify([b])
    assert r["c"] == 5 and r["dropped"].tolist() == [0] and r["kept"].tolist() == [1]
    assert r["listed"].tolist() == [1, 2, 3, 3] and r["Mp"] == 64 and r["Tcap"] == 64
    t = np.array([[1, 2, 3, 4], [4, 3, 2, 3]])                       # last tokens 4 and 3, once each: the lower id wins
    assert classify([t])["c"] == 3


def test_workspace_queries_grow_by_the_documented_amount():
    """``r4d_gpt2_workspace_bytes`` / ``r4d_gpt2_groups_workspace_bytes``: x, the LayerNorm rows, qkv and the key-blocked image
    hold round_up(M, 32) + round_up(Tmax, 32) rows, and the plan's words follow (include/r4d.h); everything else is as before."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    H, d, V = 2, 512, 1801
    cfg = _lib.GPT2ConfigC(2, H, d, V, 1024, 1e-5)
    al = lambda n: round_up(n, 256)
    for Bs, Ts in (((1,), (1,)), ((3,), (33,)), ((32,), (128,)), ((3, 4, 5), (33, 70, 96)), ((32,) * 8, (339, 17, 64, 250, 31, 32, 33, 128)),
                   ((7, 1), (100, 1000))):
        n = len(Bs)
        cB, cT = (ctypes.c_int32 * n)(*Bs), (ctypes.c_int32 * n)(*Ts)
        got = lib.r4d_gpt2_groups_workspace_bytes(ctypes.byref(cfg), n, cB, cT)
        assert got == workspace_bytes(H, d, V, Bs, Ts), (Bs, Ts)
        M, Tmax = sum(b * t for b, t in zip(Bs, Ts)), max(Ts)
        Mx = round_up(M, 32) + round_up(Tmax, 32)
        before = sum(al(4 * f) for f in (M * d, M * d, M * 3 * d, M * d, M * 4 * d, max(b * H * t * round_up(t, 128) for b, t in zip(Bs, Ts)),
                                         sum(b * ((t + 15) // 16) * d for b, t in zip(Bs, Ts)), round_up(M, 32) * d))
        grown = sum(al(4 * Mx * d * k) - al(4 * M * d * k) for k in (1, 1, 3)) + al(4 * Mx * d) - al(4 * round_up(M, 32) * d) + \
            al(4 * plan_words(M, Tmax, V))
        assert got - before == grown, (Bs, Ts)
        off = lib.r4d_gpt2_layer0_pad_rows_offset(ctypes.byref(cfg), n, cB, cT)
        assert off == got - al(4 * plan_words(M, Tmax, V)) and off % 256 == 0
        if n == 1:
            assert lib.r4d_gpt2_workspace_bytes(ctypes.byref(cfg), Bs[0], Ts[0]) == got
    assert lib.r4d_gpt2_layer0_pad_rows_offset(ctypes.byref(cfg), 0, None, None) == 0

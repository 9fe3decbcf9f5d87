"""CPU tests of the vocabulary-chunked LM head's host side: the chunk ranges ``HeadOperand`` lays its planes by, the chunk-wise
merge of the online softmax (the formulas of ``lm_ce_stats_kernel`` in numpy float32 against a float64 log-sum-exp) and the
workspace queries of the two training steps (pure host arithmetic: no GPU needed)."""
import ctypes

import numpy as np
import pytest


def _chunk_rows(ldV):
    from rag4dyg_amd import _lib
    return int(_lib.load().r4d_lm_head_chunk_rows(ldV))


def test_chunk_rows_query():
    C = _chunk_rows(1 << 20)
    assert C % 128 == 0 and 128 <= C <= 15872
    assert [_chunk_rows(v) for v in (128, 8832, 15872)] == [128, 8832, 15872]          # one chunk: the row itself
    assert [_chunk_rows(v) for v in (16000, 2 * C + 128, 100096)] == [C, C, C]


@pytest.mark.parametrize("ldV", [128, 8832, 15872, 16000, 16384, 16512, 24704, 100096])
def test_head_chunks_partition_the_padded_rows_in_multiples_of_128(ldV):
    from rag4dyg_amd.lm_training import head_chunks
    C = _chunk_rows(ldV)
    chunks = head_chunks(ldV, C)
    assert chunks[0][0] == 0 and sum(n for _c0, n in chunks) == ldV
    assert all(c0 + n == nxt for (c0, n), (nxt, _n) in zip(chunks, chunks[1:]))       # contiguous, ascending, no overlap
    assert all(n % 128 == 0 and 0 < n <= C for _c0, n in chunks) and all(n == C for _c0, n in chunks[:-1])
    assert len(chunks) == (1 if ldV <= 15872 else -(-ldV // C))
    with pytest.raises(ValueError):
        head_chunks(ldV + 4, C)


def _merged_logsumexp_f32(row, V, chunks):
    """The kernel's fold in float32: per range max mc and sum sc of exp(x - mc) over the columns < V, then
    m' = max(m, mc), s = s exp(m - m') + sc exp(mc - m'); the first range starts the pair."""
    f = np.float32
    m = s = None
    for c0, n in chunks:
        x = row[c0:min(c0 + n, V)].astype(f)
        if x.size == 0:
            continue
        mc = x.max()
        sc = np.exp(x - mc, dtype=f).sum(dtype=f)
        if m is None:
            m, s = mc, sc
        else:
            m2 = max(m, mc)
            s = f(s * np.exp(f(m - m2), dtype=f) + sc * np.exp(f(mc - m2), dtype=f))
            m = m2
    return float(np.log(s, dtype=f)) + float(m)


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_chunkwise_merge_reproduces_float64_logsumexp(where, scale):
    from rag4dyg_amd.lm_training import head_chunks, padded_vocab
    C = _chunk_rows(1 << 20)
    V = 2 * C + 5
    chunks = head_chunks(padded_vocab(V), C)
    assert len(chunks) == 3
    rng = np.random.default_rng(V + len(where))
    row = (rng.standard_normal(V) * scale).astype(np.float32)
    peak = {"first": 17, "middle": C + 3, "last": V - 2}[where]
    row[peak] = 12.0 * scale                                          # the row's maximum sits in that chunk
    x = row.astype(np.float64)
    want = float(np.log(np.exp(x - x.max()).sum()) + x.max())
    got = _merged_logsumexp_f32(row, V, chunks)
    assert abs(got / want - 1) < 1e-6, (got, want)


def test_training_workspace_does_not_grow_with_rows_times_vocabulary():
    """From ldV = C (the one-row kernel) to ldV = padded(2 C + 5) the LM and the RAG workspace grow by less than ldV * d * 4 bytes:
    dwte [ldV, d] is the only slot that follows V (+ three floats per row of softmax state; the weight-gradient scratch is sized
    for a chunk).  The result stays far below the N * ldV * 4 bytes of materialised logits."""
    from rag4dyg_amd import _lib
    from rag4dyg_amd.lm_training import padded_vocab
    lib = _lib.load()
    C = _chunk_rows(1 << 20)
    ldV = padded_vocab(2 * C + 5)
    d, B, T = 64, 32, 128
    N = B * T
    cfg = _lib.GPT2ConfigC(1, 2, d, 2 * C + 5, 1024, 1e-5)            # n_layer, n_head, n_embd, vocab, n_positions, ln_eps
    for fn in (lib.r4d_gpt2_lm_train_workspace_bytes, lib.r4d_rag_train_workspace_bytes):
        small, large = int(fn(ctypes.byref(cfg), B, T, C)), int(fn(ctypes.byref(cfg), B, T, ldV))
        assert (ldV - C) * d * 4 <= large - small < ldV * d * 4, (small, large)
        assert large - small == (ldV - C) * d * 4 + 3 * N * 4         # exactly: dwte's new rows and (m, s, x_label) per row
        assert large < N * ldV * 4, (large, N * ldV * 4)              # the WHOLE step below the materialised logits alone
        ld100k = padded_vocab(100000)
        huge = int(fn(ctypes.byref(cfg), B, T, ld100k))
        assert huge - large == (ld100k - ldV) * d * 4                 # beyond one chunk dwte alone follows V
        assert huge < N * ld100k * 4 // 4                             # a chunk is at most 15,872 of the 100,096 columns (16 %)
    assert lib.r4d_lm_ce_workspace_bytes(N) >= 4 * N * 4              # terms + (m, s, x_label) per row

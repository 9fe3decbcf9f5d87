"""NumPy restatement of the layer-0 pad-row plan (``rag4dyg_amd/csrc/common.h``: PadRowsPlan; ``encoder_ops.hip``:
pad_rows_classify_kernel) for tests/test_gpu_layer0_pad_rows.py and tests/test_host_layer0_pad_rows.py.

A call is a list of right-padded id batches [B_g, T_g]; their rows are concatenated in order.  The candidate token is the most
frequent token among the sequences' last positions (ties: the lowest id); a 32-row block (by global row index) is DROPPED when
all of its 32 rows exist and carry that token; the kept blocks are listed in ascending order, then the table blocks
M'/32 .. M'/32 + Tcap/32 - 1 (M' = round_up(M, 32), Tcap = round_up(Tmax, 32)), then repeats of the last entry up to a multiple
of 4."""
import numpy as np


def round_up(x, m):
    return (x + m - 1) // m * m


def classify(batches):
    """``batches``: a list of 2-D integer arrays.  Returns dict(c, M, Mp, Tcap, kept, dropped, listed) with ``kept`` / ``dropped``
    the ascending block indices and ``listed`` the padded list the GEMM walks."""
    rows = np.concatenate([np.asarray(b).reshape(-1) for b in batches]).astype(np.int64)
    last = np.concatenate([np.asarray(b)[:, -1] for b in batches]).astype(np.int64)
    vals, counts = np.unique(last, return_counts=True)                   # ascending ids: argmax takes the lowest on a tie
    c = int(vals[np.argmax(counts)])
    M = rows.size
    Mp = round_up(M, 32)
    Tcap = round_up(max(np.asarray(b).shape[1] for b in batches), 32)
    full = M // 32
    same = (rows[:full * 32].reshape(full, 32) == c).all(axis=1)
    dropped = np.flatnonzero(same)
    kept = np.setdiff1d(np.arange(Mp // 32), dropped)
    listed = np.concatenate([kept, Mp // 32 + np.arange(Tcap // 32)])
    listed = np.concatenate([listed, np.repeat(listed[-1:], round_up(listed.size, 4) - listed.size)])
    return dict(c=c, M=M, Mp=Mp, Tcap=Tcap, kept=kept, dropped=dropped, listed=listed)


def plan_words(M, Tmax, vocab):
    """32-bit words of the plan region (include/r4d.h)."""
    Mp, Tcap = round_up(M, 32), round_up(Tmax, 32)
    return 8 + 2 * Tcap + 2 * Mp + round_up(Mp // 32 + Tcap // 32, 4) + Mp // 32 + vocab


def workspace_bytes(n_head, d, vocab, Bs, Ts):
    """``r4d_gpt2_groups_workspace_bytes`` restated: every buffer rounded up to 256 bytes; x, the LayerNorm rows, qkv and the
    key-blocked image with round_up(M, 32) + round_up(Tmax, 32) rows, the attention output and the MLP buffer with M rows, the
    score block of the largest batch (T padded to 128), 16-row mean-pool partials, the plan words."""
    al = lambda nbytes: round_up(nbytes, 256)
    M = sum(b * t for b, t in zip(Bs, Ts))
    Mx = round_up(M, 32) + round_up(max(Ts), 32)
    scores = max(b * n_head * t * round_up(t, 128) for b, t in zip(Bs, Ts))
    pool = sum(b * ((t + 15) // 16) * d for b, t in zip(Bs, Ts))
    floats = [Mx * d, Mx * d, Mx * 3 * d, M * d, M * 4 * d, scores, pool, round_up(Mx, 32) * d, plan_words(M, max(Ts), vocab)]
    return sum(al(4 * f) for f in floats)

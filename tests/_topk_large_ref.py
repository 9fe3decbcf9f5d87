"""numpy reference of the library's top-k at any k (tests/test_host_topk_large.py, tests/test_gpu_topk_large.py).

The result definition (include/r4d.h: r4d_topk_f32): every value becomes an order-preserving key -- NaN -> -inf, -0.0 -> +0.0 --
the list is ordered by (key descending, list position ascending), which is ``np.argsort(-x, kind="stable")`` after that mapping,
and the first k (value, index) pairs are the answer; a NaN is reported as -inf.  For a plain row the list position is the column;
in a merge it is the place in the concatenation of the shard lists, and the index is the one the shard list carries.
"""
import numpy as np

PAD_V = np.float32(-np.inf)
PAD_I = np.iinfo(np.int64).max
CHUNK = 16384                      # list positions per workgroup of csrc/topk_large.hip (LG_CHUNK): where its paths change


def canon(x):
    """The value the library ranks and reports: NaN -> -inf, -0.0 -> +0.0 (float32)."""
    x = np.asarray(x, dtype=np.float32)
    y = np.where(np.isnan(x), PAD_V, x).astype(np.float32)
    return (y + np.float32(0.0)).astype(np.float32)


def topk_ref(x, k, index_offset=0):
    """x [rows, n] -> (vals f32 [rows, k], idx int64 [rows, k])."""
    y = canon(x)
    order = np.argsort(-y, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(y, order, axis=1), order.astype(np.int64) + np.int64(index_offset)


def merge_ref(vals, idx):
    """vals / idx [G, Q, k] -> (vals [Q, k], idx [Q, k]): the top-k of the concatenated lists, ties by list position.  A pad
    (-inf, INT64_MAX) is an ordinary candidate at its position."""
    G, Q, k = vals.shape
    lv = canon(np.transpose(vals, (1, 0, 2)).reshape(Q, G * k))
    li = np.transpose(idx, (1, 0, 2)).reshape(Q, G * k)
    order = np.argsort(-lv, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(lv, order, axis=1), np.take_along_axis(li, order, axis=1)


def shard_lists(x, bounds, k):
    """The [G, rows, k] lists that shards [bounds[g], bounds[g + 1]) of the columns of x hand to a merge: each the reference's
    top-min(k, shard length) with global column indices, padded to k with (-inf, INT64_MAX)."""
    rows = x.shape[0]
    G = len(bounds) - 1
    vals = np.full((G, rows, k), PAD_V, dtype=np.float32)
    idx = np.full((G, rows, k), PAD_I, dtype=np.int64)
    for g in range(G):
        a, b = bounds[g], bounds[g + 1]
        kk = min(k, b - a)
        if kk:
            vals[g, :, :kk], idx[g, :, :kk] = topk_ref(x[:, a:b], kk, a)
    return vals, idx


def brute_force(row, k):
    """O(n^2) rank count on one row: the rank of position i is the number of positions that beat it."""
    y = canon(row)
    n = y.shape[0]
    rank = np.zeros(n, dtype=np.int64)
    for i in range(n):
        for j in range(n):
            rank[i] += (y[j] > y[i]) or (y[j] == y[i] and j < i)
    out = np.empty(n, dtype=np.int64)
    out[rank] = np.arange(n)
    return y[out[:k]], out[:k]


# ------------------------------------------------------------------------------------------------ input families (fixed seeds)
FAMILIES = ("gaussian", "five values", "constant", "ascending", "descending", "low mantissa bits", "all negative", "salted")


def family(name, rows, n, seed=0):
    """float32 [rows, n] of one input family."""
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + seed)
    if name == "gaussian":
        x = rng.standard_normal((rows, n))
    elif name == "five values":                  # ties straddle every threshold and every chunk boundary
        x = rng.choice(np.array([-1.5, 0.0, 0.25, 0.5, 3.0]), size=(rows, n))
    elif name == "constant":                     # pure index order
        x = np.full((rows, n), 0.625)
    elif name == "ascending":
        x = np.arange(n, dtype=np.float64)[None, :] * 0.5 - 7.0 + np.arange(rows)[:, None]
    elif name == "descending":
        x = -np.arange(n, dtype=np.float64)[None, :] * 0.5 + 7.0 + np.arange(rows)[:, None]
    elif name == "low mantissa bits":            # equal but for the lowest 6 bits: the last radix digit decides
        bits = np.float32(0.7).view(np.uint32) & np.uint32(0xffffffc0)
        return (bits | rng.integers(0, 64, size=(rows, n)).astype(np.uint32)).view(np.float32)
    elif name == "all negative":
        x = -np.abs(rng.standard_normal((rows, n))) - 0.125
    elif name == "salted":
        x = np.round(rng.standard_normal((rows, n)) * 2) / 2          # zeros among them
        x = x.astype(np.float32)
        salt = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype=np.float32)
        where = rng.random((rows, n)) < 0.3
        x[where] = rng.choice(salt, size=int(where.sum()))
        return x
    else:
        raise ValueError(name)
    return x.astype(np.float32)

"""GPU tests of top-k beyond 64 candidates per row (csrc/topk_large.hip behind r4d_topk_f32, r4d_score_topk_f32 and
r4d_merge_topk_f32): every comparison is ``torch.equal`` on values AND indices against tests/_topk_large_ref.py.

The kernel's own edges: a workgroup owns 16384 list positions (``_topk_large_ref.CHUNK``), so 16384 / 16385 is one level against
two, 32769 three chunks, and 150001 at k = 2048 a third level (10 chunks x 2048 candidates = 20480 > 16384); the survivors are
sorted over the power of two >= k (k = 128 / 129, 1024 / 1025 change it); a chunk shorter than k pads (n = 16385 at any k).
"""
import numpy as np
import pytest
import torch

import _topk_large_ref as R
from _poison import NAN, HUGE, ONE, ZERO, poison, poisoned_allocations

pytestmark = pytest.mark.gpu

NS = (65, 66, 1000, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32769, 50001)
KS = (65, 100, 127, 128, 129, 1000, 1024, 2047, 2048)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _branches():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    return {lib.r4d_dispatch_branch_name(i).decode(): int(lib.r4d_dispatch_branch_hits(i)) for i in range(lib.r4d_dispatch_num_branches())}


def _moved(before, prefix):
    now = _branches()
    return {n: now[n] - c for n, c in before.items() if n.startswith(prefix) and now[n] != c}


def _same(got_v, got_i, want_v, want_i, what):
    wv, wi = torch.from_numpy(np.ascontiguousarray(want_v)), torch.from_numpy(np.ascontiguousarray(want_i))
    gv, gi = got_v.cpu(), got_i.cpu()
    assert gv.dtype == torch.float32 and gi.dtype == torch.int64 and gv.shape == wv.shape and gi.shape == wi.shape, what
    assert torch.equal(gi, wi), (what, "indices", int((gi != wi).sum()), (gi != wi).nonzero()[:4].tolist())
    assert torch.equal(gv.view(torch.int32), wv.view(torch.int32)), (what, "values")      # bits: -0.0 never comes back


def _ties(rows, n, seed):
    """Gaussian values on a grid of 1/64: distinct values and ties side by side."""
    return (np.round(np.random.default_rng(seed).standard_normal((rows, n)) * 64) / 64).astype(np.float32)


# ================================================================================================ 1. topk_f32 against the reference
@pytest.mark.parametrize("n", NS + (150001,))
def test_topk_f32_equals_the_reference(dev, n):
    from rag4dyg_amd import ops
    rows = (1, 3, 33)[NS.index(n) % 3] if n in NS else 2
    x = _ties(rows, n, n)
    xd = torch.from_numpy(x).to(dev)
    ks = sorted({k for k in KS + (n - 1, n) if 64 < k <= min(n, 2048)})
    if n > 100000:
        ks = [65, 2048]                                      # two levels at 65, three at 2048
    assert ks
    for k in ks:
        v, i = ops.topk_f32(xd, k)
        _same(v, i, *R.topk_ref(x, k), what=(rows, n, k))
        if k == n:                                           # the whole row: the ranking kernels' permutation
            assert torch.equal(i.to(torch.int32), ops.argsort_desc(xd))


# ================================================================================================ 2. input families
@pytest.mark.parametrize("n", [R.CHUNK, R.CHUNK + 1, 50001])
@pytest.mark.parametrize("name", R.FAMILIES)
def test_input_families(dev, name, n):
    from rag4dyg_amd import ops
    x = R.family(name, 3, n)
    xd = torch.from_numpy(x).to(dev)
    for k in (65, 1000, 2048):
        v, i = ops.topk_f32(xd, k)
        _same(v, i, *R.topk_ref(x, k), what=(name, n, k))
        assert not torch.isnan(v).any()


# ================================================================================================ 3. consistency with k <= 64
def test_first_64_of_a_top_100_are_the_top_64_and_the_counters_tell_the_paths_apart(dev):
    from rag4dyg_amd import ops
    x = torch.from_numpy(_ties(5, 20000, 3)).to(dev)
    b = _branches()
    v64, i64 = ops.topk_f32(x, 64)
    assert _moved(b, "tuning:topk_large:") == {} and _moved(b, "topk:")
    b = _branches()
    v100, i100 = ops.topk_f32(x, 100)
    assert torch.equal(v100[:, :64], v64) and torch.equal(i100[:, :64], i64)
    b = _branches()
    ops.topk_f32(x, 65)
    assert _moved(b, "tuning:topk_large:") == {"tuning:topk_large:several levels": 1} and _moved(b, "topk:") == {}
    b = _branches()
    ops.topk_f32(x[:, :R.CHUNK].contiguous(), 65)
    assert _moved(b, "tuning:topk_large:") == {"tuning:topk_large:one level": 1} and _moved(b, "topk:") == {}


# ================================================================================================ 4. score_topk
@pytest.fixture(scope="module")
def pools(dev):
    from rag4dyg_amd import ops
    g = torch.Generator().manual_seed(41)
    out = {}
    for N in (1000, 20001):
        p = torch.randn(N, 64, generator=g)
        p[N // 2:N // 2 + 200] = p[:200]                     # equal rows: equal scores at distant indices
        out[N] = ops.normalize_rows(p.to(dev))
    out["q"] = ops.normalize_rows(torch.randn(70, 64, generator=g).to(dev))
    return out


@pytest.mark.parametrize("N,k", [(1000, 100), (20001, 100), (20001, 1024)])          # k <= N
def test_score_topk_equals_the_reference_on_its_own_scores(dev, pools, N, k):
    from rag4dyg_amd import ops
    pool, q = pools[N], pools["q"]
    for off in (0, 12345):
        per_q = {}
        for Q in (1, 33, 70):
            v, i, S = ops.score_topk(q[:Q].contiguous(), pool, k, index_offset=off, want_scores=True)
            _same(v, i, *R.topk_ref(S.cpu().numpy(), k, off), what=(N, k, off, Q))
            v2, i2, none = ops.score_topk(q[:Q].contiguous(), pool, k, index_offset=off, want_scores=False)
            assert none is None and torch.equal(v2, v) and torch.equal(i2, i)
            per_q[Q] = (v, i)
        for Q in (33, 70):                                   # a row does not depend on how the queries are batched
            assert torch.equal(per_q[Q][0][:1], per_q[1][0]) and torch.equal(per_q[Q][1][:1], per_q[1][1])
        assert torch.equal(per_q[70][0][:33], per_q[33][0]) and torch.equal(per_q[70][1][:33], per_q[33][1])


def test_pool_index_search_at_100(dev, pools):
    from rag4dyg_amd import ops
    from rag4dyg_amd.retrieval import PoolIndex
    g = torch.Generator().manual_seed(5)
    emb, qe = torch.randn(3000, 64, generator=g).to(dev), torch.randn(9, 64, generator=g).to(dev)
    index = PoolIndex(emb, index_offset=700)
    v, i, S = index.search(qe, 100, want_scores=True)
    _same(v, i, *R.topk_ref(S.cpu().numpy(), 100, 700), what="PoolIndex.search")
    v2, i2, _ = ops.score_topk(ops.normalize_rows(qe), index.pool_hat, 100, 700)
    assert torch.equal(v, v2) and torch.equal(i, i2)
    hv, hi = index.search_hat(ops.normalize_rows(qe), 100)
    assert torch.equal(v, hv) and torch.equal(i, hi)


# ================================================================================================ 5. merge_topk
@pytest.mark.parametrize("G,k", [(2, 65), (3, 65), (8, 65), (2, 1024), (3, 1024), (8, 1024), (20, 1024)])
def test_merge_topk_equals_the_reference(dev, G, k):
    """Shards of unequal length from one split row, some shorter than k (padded); the five-valued rows put equal values into
    different shards.  20 x 1024 candidates are more than one chunk: the merge's own second level."""
    from rag4dyg_amd import ops
    n = 3 * k + 40 * G
    x = np.concatenate([R.family("five values", 2, n, seed=G), _ties(3, n, G * k)])
    cuts = np.sort(np.random.default_rng(G + k).choice(np.arange(18, n), size=G - 2, replace=False))
    bounds = [0, 17, *[int(c) for c in cuts], n]             # the first shard is far shorter than k
    vals, idx = R.shard_lists(x, bounds, k)
    assert (idx == R.PAD_I).any()
    b = _branches()
    ov, oi = ops.merge_topk(torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev))
    assert _moved(b, "tuning:topk_large:merge") == {"tuning:topk_large:merge route": 1}
    _same(ov, oi, *R.merge_ref(vals, idx), what=("merge", G, k))
    _same(ov, oi, *R.topk_ref(x, k), what=("unsplit", G, k))


def test_eight_shards_in_one_process_equal_the_whole_pool(dev, pools):
    from rag4dyg_amd import ops
    pool, q, k = pools[20001], pools["q"][:33].contiguous(), 100
    bounds = [0, 90, 2500, 5000, 7501, 10000, 12500, 15000, 20001]         # the first shard is shorter than k
    vs, is_ = [], []
    for a, b in zip(bounds, bounds[1:]):
        kk = min(k, b - a)
        v, i, _ = ops.score_topk(q, pool[a:b].contiguous(), kk, index_offset=a)
        pv = torch.full((33, k), float("-inf"), device=dev)
        pi = torch.full((33, k), R.PAD_I, dtype=torch.int64, device=dev)
        pv[:, :kk], pi[:, :kk] = v, i
        vs.append(pv); is_.append(pi)
    mv, mi = ops.merge_topk(torch.stack(vs), torch.stack(is_))
    wv, wi, _ = ops.score_topk(q, pool, k)
    assert torch.equal(mv, wv) and torch.equal(mi, wi)


def test_sharded_topk_at_world_size_one_pads_a_short_shard(dev, pools):
    from rag4dyg_amd import dist, ops
    pool, q = pools[1000][:80].contiguous(), pools["q"][:5].contiguous()
    local = lambda qh, ph, k, off: ops.score_topk(qh, ph, k, off)[:2]
    v, i = dist.sharded_topk(q, pool, 4000, 100, local, ops.merge_topk)
    wv, wi, _ = ops.score_topk(q, pool, 80, 4000)
    assert torch.equal(v[:, :80], wv) and torch.equal(i[:, :80], wi)
    assert bool((v[:, 80:] == float("-inf")).all()) and bool((i[:, 80:] == R.PAD_I).all())
    # the padded lists of two such shards merge to real candidates only: the pads of the first list lose to the second's rows
    gv, gi = torch.stack([v, v]), torch.stack([i, torch.where(i == R.PAD_I, i, i + 80)])
    mv, mi = ops.merge_topk(gv, gi)
    _same(mv, mi, *R.merge_ref(gv.cpu().numpy(), gi.cpu().numpy()), what="padded merge")
    assert bool(torch.isfinite(mv).all())


# ================================================================================================ 6. scratch discipline
def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _run_poisoned(pattern, call):
    """First allocation of every buffer, then its reuse, both filled with ``pattern`` (tests/_poison.py)."""
    from rag4dyg_amd import ops
    ops._WS.clear()
    out = []
    for _ in range(2):
        with poisoned_allocations(pattern):
            out.append({n: t.detach().clone() for n, t in call().items() if t is not None})
        for buf in ops._WS.values():
            poison(buf, pattern)
    return out


@pytest.mark.parametrize("entry", ["topk_f32", "score_topk", "score_topk+scores", "merge_topk"])
def test_poisoned_workspace_and_outputs_are_invisible_at_k_100(dev, pools, entry):
    """Two levels in every entry (50001 columns, 20001 pool rows, 200 x 100 candidates): candidate values and indices of the
    first level pass through the workspace.  Every output byte is written: no output is NaN, +3.4e38 or an index of all ones."""
    from rag4dyg_amd import ops
    k = 100
    if entry == "topk_f32":
        x = torch.from_numpy(_ties(3, 50001, 9)).to(dev)
        call = lambda: dict(zip(("vals", "idx"), ops.topk_f32(x, k)))
    elif entry.startswith("score_topk"):
        q = pools["q"][:5].contiguous()
        call = lambda: dict(zip(("vals", "idx", "scores"), ops.score_topk(q, pools[20001], k, 3, want_scores=entry.endswith("scores"))))
    else:
        x = _ties(4, 40000, 10)
        vals, idx = R.shard_lists(x, [200 * g for g in range(200)] + [40000], k)
        dv, di = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev)
        call = lambda: dict(zip(("vals", "idx"), ops.merge_topk(dv, di)))
    b = _branches()
    base = _run_poisoned(ZERO, call)
    assert _moved(b, "tuning:topk_large:").get("tuning:topk_large:several levels") == 2
    for pattern in (NAN, HUGE, ONE):
        got = _run_poisoned(pattern, call)
        for a, c in zip(base, got):
            assert set(a) == set(c)
            for n in a:
                assert torch.equal(_bits(a[n]), _bits(c[n])), (entry, pattern, n)
    for step in base:
        assert torch.isfinite(step["vals"]).all() and int(step["idx"].min()) >= 0 and int(step["idx"].max()) < (1 << 40)


def test_a_workspace_one_byte_short_is_refused_and_launches_nothing(dev):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows, n, k = 2, 50001, 100
    x = torch.zeros(rows, n, device=dev)
    v, i = torch.empty(rows, k, device=dev), torch.empty(rows, k, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.r4d_topk_f32_workspace_bytes(rows, n, k)), dtype=torch.uint8, device=dev)
    b = _branches()
    rc = lib.r4d_topk_f32(x.data_ptr(), rows, n, k, v.data_ptr(), i.data_ptr(), ws.data_ptr(), ws.numel() - 1, st)
    assert rc != 0 and "workspace too small" in lib.r4d_last_error().decode() and _moved(b, "") == {}
    qh, ph = torch.zeros(rows, 64, device=dev), torch.zeros(n, 64, device=dev)
    ws = torch.empty(int(lib.r4d_score_topk_workspace_bytes(rows, n, k)), dtype=torch.uint8, device=dev)
    rc = lib.r4d_score_topk_f32(qh.data_ptr(), ph.data_ptr(), rows, n, 64, k, 0, v.data_ptr(), i.data_ptr(), None, ws.data_ptr(),
                                ws.numel() - 1, st)
    assert rc != 0 and "workspace too small" in lib.r4d_last_error().decode() and _moved(b, "") == {}
    G = 3
    gv, gi = torch.zeros(G, rows, k, device=dev), torch.zeros(G, rows, k, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.r4d_merge_topk_workspace_bytes(G, rows, k)), dtype=torch.uint8, device=dev)
    rc = lib.r4d_merge_topk_f32(gv.data_ptr(), gi.data_ptr(), G, rows, k, v.data_ptr(), i.data_ptr(), ws.data_ptr(), ws.numel() - 1, st)
    assert rc != 0 and "workspace too small" in lib.r4d_last_error().decode() and _moved(b, "") == {}
    # and with the byte it runs
    rc = lib.r4d_merge_topk_f32(gv.data_ptr(), gi.data_ptr(), G, rows, k, v.data_ptr(), i.data_ptr(), ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    assert rc == 0 and _moved(b, "tuning:topk_large:merge") == {"tuning:topk_large:merge route": 1}


# ================================================================================================ 7. repeatability
def test_the_same_call_twice_gives_the_same_bits(dev, pools):
    from rag4dyg_amd import ops
    x = torch.from_numpy(R.family("five values", 7, 50001)).to(dev)
    for k in (65, 1024, 2048):
        a, b = ops.topk_f32(x, k), ops.topk_f32(x, k)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])
    q = pools["q"][:33].contiguous()
    a, b = ops.score_topk(q, pools[20001], 1024), ops.score_topk(q, pools[20001], 1024)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])

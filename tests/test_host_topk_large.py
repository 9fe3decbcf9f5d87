"""CPU tests of top-k beyond 64 candidates (csrc/topk_large.hip): the numpy reference against a brute-force rank count, the limits
and size queries of the library (host arithmetic only: every refusal below happens before any device call), and the packed
one-collective candidate layout at the largest k."""
import numpy as np
import pytest
import torch

import _topk_large_ref as R

FAKE = 0x1000          # a non-null "device pointer": the calls below are refused before anything dereferences or launches


@pytest.mark.parametrize("name", R.FAMILIES)
def test_reference_equals_brute_force_rank_count(name):
    x = R.family(name, 3, 37)
    for k in (1, 5, 36, 37):
        v, i = R.topk_ref(x, k, index_offset=11)
        for r in range(x.shape[0]):
            bv, bi = R.brute_force(x[r], k)
            assert np.array_equal(v[r].view(np.uint32), bv.view(np.uint32)) and np.array_equal(i[r], bi + 11), (name, k, r)
    assert not np.isnan(R.topk_ref(x, 37)[0]).any() and not np.signbit(R.topk_ref(x, 37)[0][R.topk_ref(x, 37)[0] == 0]).any()


def test_reference_merge_equals_reference_topk_of_the_unsplit_row():
    x = R.family("five values", 4, 300)
    for bounds in ((0, 100, 300), (0, 7, 150, 151, 300)):          # shards shorter than k are padded
        v, i = R.merge_ref(*R.shard_lists(x, bounds, 70))
        wv, wi = R.topk_ref(x, 70)
        assert np.array_equal(v, wv) and np.array_equal(i, wi)


def test_max_k_symbol_and_abi():
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    assert lib.r4d_topk_max_k() == 2048 == ops.TOPK_MAX_K
    assert lib.r4d_abi_version() == 6


@pytest.mark.parametrize("rows,n", [(1, 2048), (32, 12512), (32, 100000), (256, 100000), (3, 1 << 20)])
def test_workspace_queries_do_not_shrink_from_64_to_65(rows, n):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    for fn in (lib.r4d_topk_f32_workspace_bytes, lib.r4d_score_topk_workspace_bytes):
        sizes = [fn(rows, n, k) for k in (63, 64, 65, 66, 100, 1024, 2048)]
        assert all(s > 0 for s in sizes) and sizes[1] <= sizes[2], sizes
        assert all(a <= b for a, b in zip(sizes[2:], sizes[3:])), sizes              # and grow with k on the new path
    G = max(2, n // 4096)
    sizes = [lib.r4d_merge_topk_workspace_bytes(G, rows, k) for k in (64, 65, 1024, 2048)]
    assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    # the candidates of the first level are in it: ceil(n / 16384) chunks of k (value, index) pairs per row
    if n > R.CHUNK:
        assert lib.r4d_topk_f32_workspace_bytes(rows, n, 1024) >= rows * -(-n // R.CHUNK) * 1024 * 12


def _refused(rc, *needles):
    from rag4dyg_amd import _lib
    msg = _lib.load().r4d_last_error().decode()
    assert rc != 0 and all(s in msg for s in needles), (rc, msg)


def test_limits_are_refused_by_name_before_any_device_call():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    big = 1 << 40                                            # a workspace size that passes every size check
    hits = lambda: sum(int(lib.r4d_dispatch_branch_hits(i)) for i in range(lib.r4d_dispatch_num_branches()))
    before = hits()
    _refused(lib.r4d_topk_f32(FAKE, 2, 5000, 2049, FAKE, FAKE, FAKE, big, None), "k=2049", "2048")
    _refused(lib.r4d_topk_f32(FAKE, 2, 100, 101, FAKE, FAKE, FAKE, big, None), "k=101", "n=100")
    _refused(lib.r4d_score_topk_f32(FAKE, FAKE, 2, 5000, 64, 2049, 0, FAKE, FAKE, None, FAKE, big, None), "k=2049", "2048")
    _refused(lib.r4d_score_topk_f32(FAKE, FAKE, 2, 100, 64, 101, 0, FAKE, FAKE, None, FAKE, big, None), "k=101", "N=100")
    _refused(lib.r4d_merge_topk_f32(FAKE, FAKE, 3, 2, 2049, FAKE, FAKE, FAKE, big, None), "k=2049", "2048")
    _refused(lib.r4d_topk_f64(FAKE, 2, 5000, 65, FAKE, FAKE, FAKE, big, None), "k=65", "64")
    assert "2048" not in lib.r4d_last_error().decode()       # the f64 rows keep their own limit and message
    # a workspace one byte short: refused by size, nothing chosen, nothing launched
    for k in (65, 1024):
        need = lib.r4d_topk_f32_workspace_bytes(2, 50001, k)
        _refused(lib.r4d_topk_f32(FAKE, 2, 50001, k, FAKE, FAKE, FAKE, need - 1, None), "workspace too small")
        need = lib.r4d_score_topk_workspace_bytes(2, 50001, k)
        _refused(lib.r4d_score_topk_f32(FAKE, FAKE, 2, 50001, 64, k, 0, FAKE, FAKE, None, FAKE, need - 1, None), "workspace too small")
        need = lib.r4d_merge_topk_workspace_bytes(3, 2, k)
        _refused(lib.r4d_merge_topk_f32(FAKE, FAKE, 3, 2, k, FAKE, FAKE, FAKE, need - 1, None), "workspace too small")
    assert hits() == before


def test_packed_candidates_round_trip_bits_at_the_largest_k():
    from rag4dyg_amd import dist
    k, Q, G = 2048, 3, 2
    x = R.family("salted", G * Q, 5000).reshape(G, Q, 5000)
    packed = []
    for g in range(G):
        v, i = R.topk_ref(x[g], k, index_offset=g * 5000 + (1 << 33))
        v[:, -5:], i[:, -5:] = R.PAD_V, R.PAD_I             # a short shard's padding travels too
        packed.append(dist.pack_candidates(torch.from_numpy(v), torch.from_numpy(i)))
        assert packed[-1].shape == (1, Q, 12 * k) and packed[-1].dtype == torch.uint8
    gv, gi = dist.unpack_candidates(torch.cat(packed), k)
    for g in range(G):
        v, i = R.topk_ref(x[g], k, index_offset=g * 5000 + (1 << 33))
        v[:, -5:], i[:, -5:] = R.PAD_V, R.PAD_I
        assert np.array_equal(gv[g].numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(gi[g].numpy(), i)

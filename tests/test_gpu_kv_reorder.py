"""``ops.kv_cache_reorder`` (``r4d_kv_cache_reorder_f32``: the beam step's in-place reordering of the key/value cache) against
``torch.index_select`` on a copy: bit-exact inside the named groups, positions and layers, every other byte unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_LAYER, T_CAP = 2, 9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def make_cache(dev, B0, n, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(N_LAYER, B0 * n, T_CAP, 2 * d, generator=g)
    c.view(torch.int32)[0, 0, 0, :4] = torch.tensor([0x7fc00001, -1, 0x7f800000, 0x00000001], dtype=torch.int32)   # bit patterns must survive too
    return c.to(dev)


def expected(cache, src, n, lo, hi, active):
    out = cache.clone()
    B0 = cache.shape[1] // n
    for b in range(B0):
        if active is not None and not active[b]:
            continue
        rows = torch.arange(b * n, b * n + n, device=cache.device)
        a, z = max(int(lo[b]), 0), min(int(hi[b]), T_CAP)
        if a < z:
            out[:, rows, a:z] = cache.index_select(1, torch.as_tensor(src[b * n:b * n + n], device=cache.device))[:, :, a:z]
    return out


def perms(n, B0, kind, rng):
    src = np.arange(B0 * n)
    for b in range(B0):
        base = b * n
        if kind == "swap":
            src[base], src[base + n - 1] = base + n - 1, base
        elif kind == "cycle":
            src[base:base + n] = base + (np.arange(n) + 1) % n
        elif kind == "one_source":
            src[base:base + n] = base + (n - 1 if b % 2 else 0)
        elif kind == "random":
            src[base:base + n] = base + rng.integers(0, n, n)
        elif kind == "mixed" and b == 1:
            src[base:base + n] = base + (np.arange(n) + 1) % n            # groups 0 and 2 keep the identity
    return src


def run(dev, B0, n, d, src, lo, hi, active=None, seed=0):
    from rag4dyg_amd import ops
    cache = make_cache(dev, B0, n, d, seed)
    want = expected(cache, src, n, lo, hi, active)
    i32 = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.int32)
    got = ops.kv_cache_reorder(cache, i32(src), n, i32(lo), i32(hi), None if active is None else i32(active))
    torch.cuda.synchronize()
    assert got.data_ptr() == cache.data_ptr()                              # in place
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (B0, n, d)


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("n", [2, 3, 16])
@pytest.mark.parametrize("B0", [1, 3])
def test_permutations_against_index_select(dev, B0, n, d):
    rng = np.random.default_rng(n * 100 + B0)
    for kind in ("identity", "swap", "cycle", "one_source", "random", "mixed"):
        run(dev, B0, n, d, perms(n, B0, kind, rng), [2] * B0, [7] * B0)


@pytest.mark.parametrize("n", [2, 16])
def test_ranges_and_done_groups(dev, n):
    B0, d = 3, 64
    rng = np.random.default_rng(n)
    src = perms(n, B0, "cycle", rng)
    run(dev, B0, n, d, src, [4, 0, 5], [4, T_CAP, 6])                      # lo = hi: nothing; the whole cache; one position
    run(dev, B0, n, d, src, [0, 0, 0], [T_CAP] * 3)
    run(dev, B0, n, d, src, [8, 3, 0], [T_CAP, 2, 1])                      # the last position; hi < lo: nothing; the first position
    run(dev, B0, n, d, src, [-3, 0, 2], [4, T_CAP + 5, 5])                 # ranges are clipped to the cache
    run(dev, B0, n, d, src, [1] * 3, [8] * 3, active=[1, 0, 1])            # a done group is skipped
    run(dev, B0, n, d, src, [1] * 3, [8] * 3, active=[0, 0, 0])


def test_a_source_outside_its_group_is_refused_and_the_cache_left_alone(dev):
    from rag4dyg_amd import ops
    n, B0, d = 2, 2, 64
    cache = make_cache(dev, B0, n, d)
    before = cache.clone()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    for bad in ([0, 2, 2, 3], [1, 0, 3, 1], [-1, 0, 2, 3], [0, 1, 2, 4]):
        with pytest.raises(ValueError, match="outside its own group"):
            ops.kv_cache_reorder(cache, i32(bad), n, i32([0, 0]), i32([T_CAP, T_CAP]))
    with pytest.raises(ValueError):
        ops.kv_cache_reorder(cache, i32([0, 1, 2]), n, i32([0, 0]), i32([T_CAP, T_CAP]))
    torch.cuda.synchronize()
    assert torch.equal(cache.view(torch.int32), before.view(torch.int32))


def test_the_entry_itself_poisons_a_row_whose_source_is_outside_its_group(dev):
    """The decode loop calls the entry with indices it made itself; a wrong one must never become a read outside the group."""
    from rag4dyg_amd import _lib
    n, B0, d = 2, 2, 64
    cache = make_cache(dev, B0, n, d)
    before = cache.clone()
    src = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev)        # group 1 names the rows of group 0
    lo, hi = torch.tensor([2, 2], dtype=torch.int32, device=dev), torch.tensor([5, 5], dtype=torch.int32, device=dev)
    _lib.check(_lib.load().r4d_kv_cache_reorder_f32(cache.data_ptr(), src.data_ptr(), lo.data_ptr(), hi.data_ptr(), None, N_LAYER, B0, n,
                                                    T_CAP, d, torch.cuda.current_stream().cuda_stream), "kv_cache_reorder")
    torch.cuda.synchronize()
    assert torch.isnan(cache[:, 2:4, 2:5]).all()
    keep = torch.ones_like(cache, dtype=torch.bool)
    keep[:, 2:4, 2:5] = False
    assert torch.equal(cache.view(torch.int32)[keep], before.view(torch.int32)[keep])

"""The epilogues of the LDS-DMA f16x2 GEMM (``csrc/gemm_h2p_body.h``) on their column-pair lane mapping.

At the 128 x 256 tile the W rows of a tile are permuted at the DMA source, so that a lane of the accumulator holds two NEIGHBOURING
columns; bias, residual, the row-major stores and the f16x2 lines are all addressed on that mapping (the h2-word output, which
the single-op entry does not reach, keeps one column per lane).  The register-staged ``gemm_h2`` kernels keep the one-column mapping and the same arithmetic: they are the independent
reference, and every comparison here is bit for bit.  The 128 x 128 tile keeps the old mapping and runs beside it.

Shapes: M 1 (one row), 33 and 129 (one row into the next 32-row block / 128-row tile), 128 (one whole tile), 300 (three row
tiles, the last partial); K 32 (ONE k-tile), 96 (the three-stage ring once round), 512 (the bench's); N 256 (one interior column
tile), 320 (an interior and an edge column tile), 512, 1536 (six column tiles).

Which tile width a shape takes is the dispatcher's choice (``pick_tile_128``: the 128 x 256 tile only where the narrower one would
need more rounds of the 256 CUs), and with M <= 300 every shape above takes the 128 x 128 tile -- the mapping that does NOT
change.  So each N runs once more with enough rows for the 128 x 256 tile (``BIG``: between 128 and 256 tiles of that width),
with a partial last row tile, at the smallest K; N = 512 at K = 512 too.  The branch counters say which width ran."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MS, KS, NS = (1, 33, 128, 129, 300), (32, 96, 512), (256, 320, 512, 1536)
BIG = ((16533, 32, 256), (11001, 32, 320), (8333, 512, 512), (8205, 96, 512), (2700, 96, 1536), (4000, 32, 1536))     # (M, K, N)
W256, W128 = "gemm_h2p:128x256x32", "gemm_h2p:128x128x32"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _hits():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    return {lib.r4d_dispatch_branch_name(i).decode(): int(lib.r4d_dispatch_branch_hits(i)) for i in range(lib.r4d_dispatch_num_branches())}


@pytest.fixture(scope="module")
def operands(dev):
    """Per (K, N): weight planes and bias; per (M, K): rows and their lines -- made once, never written."""
    from rag4dyg_amd import ops
    g = torch.Generator().manual_seed(77)
    out = {"w": {}, "x": {}}
    for K in KS:
        for N in NS:
            out["w"][K, N] = (ops.split2_planes((torch.randn(K, N, generator=g) * 0.05).to(dev)), torch.randn(N, generator=g).to(dev))
        for M in MS + tuple(m for m, k, _ in BIG if k == K):
            x = (torch.randn(M, K, generator=g) * 1.7 + 0.3).to(dev)
            out["x"][M, K] = (x, ops.split2_lines(x))
    out["res"] = torch.randn(max(m for m, _, _ in BIG), max(NS), generator=g).to(dev)
    return out


def _compare(ops, operands, M, K, N):
    x, lines = operands["x"][M, K]
    planes, b = operands["w"][K, N]
    res = operands["res"][:M, :N].contiguous()
    for epi, r in (("none", None), ("gelu", None), ("residual", res)):
        want = ops.conv1d_h2(x, planes, b, epi, r)
        got = ops.conv1d_h2p(lines, planes, b, epi, r)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (M, K, N, epi, (got - want).abs().max().item())
    want_l = ops.split2_lines(ops.conv1d_h2(x, planes, b, "gelu"))
    got_l = ops.conv1d_h2p(lines, planes, b, "gelu", out_lines=True)
    assert torch.equal(got_l, want_l), (M, K, N, "lines")
    # no bias: the epilogues' other arm
    assert torch.equal(ops.conv1d_h2p(lines, planes, None, "none"), ops.conv1d_h2(x, planes, None, "none")), (M, K, N, "no bias")


def _ran(before, after):
    return sorted(k[:19] for k in after if after[k] > before.get(k, 0) and k.startswith("gemm_h2p"))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_every_epilogue_equals_the_register_staged_gemm_bit_for_bit(dev, operands, N, K):
    from rag4dyg_amd import ops
    before = _hits()
    for M in MS:
        _compare(ops, operands, M, K, N)
    assert _ran(before, _hits()) == [W128]


@pytest.mark.parametrize("M,K,N", BIG)
def test_the_128x256_tile_with_column_pairs_equals_the_register_staged_gemm_bit_for_bit(dev, operands, M, K, N):
    from rag4dyg_amd import ops
    before = _hits()
    _compare(ops, operands, M, K, N)
    assert _ran(before, _hits()) == [W256]

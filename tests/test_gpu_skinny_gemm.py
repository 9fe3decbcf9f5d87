"""The decode step's weight-stream GEMM (csrc/gemm_skinny.hip) ALONE, through ``ops.conv1d_skinny`` (r4d_conv1d_skinny_f32), against
a float64 reference at the edges of its five kernels: every K class of the dispatcher, the row and column edges of the tiles, the
4096-column boundary of the ticket array, the in-place residual, the self-resetting tickets over 21 unsynchronised launches, both
LayerNorm forms, the fold kernel, and -- in a child process under R4D_SKINNY16=0 -- the 32-column forms.

Error measure and gates: tests/_skinny_ref.py (rho = error in units of 2^-24 x the sum of the magnitudes of the formula's terms;
rho <= chain depth + 16, and rho <= 8 x rho of the float32 in-order reference on the same inputs).  Set-up and after-checks of
every call: tests/_skinny_run.py (NaN-filled y of 32 rows, guards, every poison pattern of tests/_poison.py in the workspace,
dispatch counters exactly those of the intended branch).  tests/test_host_skinny_gemm.py shows on the CPU that the gates hold for
the float32 reference and break for every planted defect at these shapes.  Measured numbers: profiles/skinny_gemm_parity.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _skinny_ref as R
from _poison import NAN, ZERO
from _skinny_run import WS_GUARD, Runner, bits
from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def run(dev):
    return Runner(dev)


@pytest.mark.parametrize("K", R.K_CLASSES)
def test_every_k_class(run, K):
    """M 32, N 90 (five full 16-column tiles and a ragged one; two full 32-column tiles and a ragged one), the three epilogues,
    with and without bias: plain with one slice (256) and five (1280), the fused 16-column kernel (512: ng 2, 768: ng 3), the
    ticketed split-K (1024: ng 2, 1536: ng 3, two slices each; 4096: ng 2, eight slices)."""
    d = R.make(32, K, 90)
    for e in R.EPILOGUES:
        for bias in (True, False):
            c, y = run.case(d, 32, 90, e, bias)
            assert rel_err(y, c.ref) < 1e-5                      # the suite's usual measure, for the record: far coarser than the gates


@pytest.mark.parametrize("K", R.M_EDGE_KS)
def test_m_edges(run, K):
    """A row's bits may not depend on M: rows 0 .. M-1 of each call are those of the M = 32 call on the same data."""
    d = R.make(32, K, R.M_EDGE_N)
    _c, full = run.case(d, 32, R.M_EDGE_N, "residual")
    for M in R.M_EDGES:
        _c, y = run.case(d, M, R.M_EDGE_N, "residual")
        assert np.array_equal(bits(y), bits(full[:M])), f"K {K}: rows 0..{M - 1} of the M = {M} call differ from the M = 32 call's"


@pytest.mark.parametrize("K", R.N_EDGE_KS)
def test_n_edges(run, K):
    """A column's bits may not depend on N (within one kernel form): columns 0 .. N-1 are those of the N = 48 call with the same
    first N weight rows."""
    d = R.make(R.N_EDGE_M, K, R.N_EDGE_FULL)
    assert len({R.form(K, N)[0] for N in R.N_EDGES + (R.N_EDGE_FULL,)}) == 1
    _c, full = run.case(d, R.N_EDGE_M, R.N_EDGE_FULL, "gelu")
    for N in R.N_EDGES:
        _c, y = run.case(d, R.N_EDGE_M, N, "gelu")
        assert np.array_equal(bits(y), bits(full[:, :N])), f"K {K}: columns 0..{N - 1} of the N = {N} call differ from the N = 48 call's"


@pytest.mark.parametrize("K,M,N", R.BOUNDARY)
def test_the_4096_column_boundary(run, K, M, N):
    """K 1024: N = 4096 uses all 256 tickets, N = 4112 (257 tiles) leaves the 16-column kernel for the 32-column split-K plus the
    epilogue launch.  K 512, N = 4112: one slice, the 16-column kernel with 257 tiles and no tickets -- correct whatever the
    workspace holds (Runner.call asserts the branch)."""
    want = {(1024, 4096): ("skinny16", 2, 2), (1024, 4112): ("skinny8", 2, 2), (512, 4112): ("skinny16", 2, 1)}[(K, N)]
    assert R.form(K, N) == want
    run.case(R.make(M, K, N), M, N, "residual")


@pytest.mark.parametrize("K,M,N", R.INPLACE)
def test_in_place_residual(run, K, M, N):
    """y_d == residual_d, as the decode step calls its two residual projections: fused (768) and last arriver (1024).  The same
    bits as with a separate output."""
    d = R.make(M, K, N)
    _c, apart = run.case(d, M, N, "residual", patterns=(ZERO, NAN))
    _c, inplace = run.case(d, M, N, "residual", inplace=True)
    assert np.array_equal(bits(inplace), bits(apart))


def test_ticket_contract(run, dev):
    """One launch with counters_zeroed = 0 on tickets full of 0xFF, then 20 with counters_zeroed = 1 and nothing cleared in
    between: each launch must leave the tickets at zero for the next.  The shapes alternate -- all 256 tickets (K 1024, N 4096),
    three slices' worth of ng 3 (K 1536, N 48), three tickets (K 1024, N 33) -- over ONE workspace, whose partials are therefore
    stale from a different shape or different x each time: per shape the calls alternate between two seeded x, so that a partial
    left over from the previous call of the same shape is a wrong value, and every call is compared bit for bit with the first
    call on the same (shape, x).  One pass, no retry."""
    from _poison import poison
    total = max(R.workspace_bytes(K, N) for K, _M, N in R.TICKET_SHAPES)
    wsbuf = torch.empty(total + WS_GUARD, dtype=torch.uint8, device=dev)
    poison(wsbuf[:total], NAN)
    data = {(s, v): R.make(M, K, N, seed=v) for s, (K, M, N) in enumerate(R.TICKET_SHAPES) for v in (0, 1)}
    first = {}
    for i in range(21):
        s = i % 3
        v = (i // 3) % 2
        K, M, N = R.TICKET_SHAPES[s]
        d = data[(s, v)]
        y = run.call(d, M, N, "residual", zeroed=(i > 0), ws=(wsbuf, total))
        if (s, v) not in first:
            first[(s, v)] = y
            run.gates(f"ticket chain K{K} M{M} N{N} x{v}", run.reference(d, M, N, "residual"), y)
        else:
            assert np.array_equal(bits(y), bits(first[(s, v)])), f"call {i} (K {K}, N {N}, x{v}) differs from the first call on the same inputs"
    assert len(first) == 6
    assert int(wsbuf[:1024].max()) == 0, "the last launch left a ticket behind"


@pytest.mark.parametrize("K", R.LN_KS)
@pytest.mark.parametrize("N", R.LN_NS)
def test_layernorm_forms(run, K, N):
    """LayerNorm formed per launch (ln_w, ln_b), pre-folded into the weight (ops.fold_layernorm), and ops.layernorm followed by the
    entry without LayerNorm: all three against float64 LayerNorm-then-GEMM under the gates with the LayerNorm scale."""
    d = R.make(32, K, N, ln=True)
    for M in R.LN_MS:
        for e in R.LN_EPILOGUES:
            for form in ("launch", "fold", "separate"):
                run.case(d, M, N, e, ln=form, patterns=(ZERO, NAN))


def test_folded_layernorm_takes_a_residual(run):
    """The wrapper accepts the combination; the fused epilogue adds the residual after the LayerNorm constants."""
    run.case(R.make(17, 768, 33, ln=True), 17, 33, "residual", ln="fold", inplace=True)


@pytest.mark.parametrize("K", R.FOLD_KS)
def test_fold_layernorm_alone(dev, K):
    """wTg = fl32(g_k w_nk) bit for bit; lnc against float64 under the hard gate of its chain: K / 64 terms per lane, 6 shuffle
    steps, in units of 2^-24 sum |g w| and 2^-24 sum |beta w|.  N around the four rows of a workgroup; K 100: a ragged last trip."""
    from rag4dyg_amd import ops
    for N in R.FOLD_NS:
        rng = np.random.default_rng([N, K])
        w = (0.05 * rng.standard_normal((N, K))).astype(np.float32)
        g = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        b = (0.1 * rng.standard_normal(K)).astype(np.float32)
        wTg, lnc = ops.fold_layernorm(torch.from_numpy(w).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(b).to(dev))
        want_w, want_c, den = R.fold_ref(w, g, b)
        assert np.array_equal(bits(wTg.cpu().numpy()), bits(want_w)), (N, K)
        r = float((np.abs(lnc.cpu().numpy().astype(np.float64) - want_c) / (R.U * den)).max())
        print(f"[rho] fold_layernorm N{N} K{K} | rho {r:.2f} | hard gate {R.fold_gate(K)}")
        assert r <= R.fold_gate(K), (N, K, r)


# ------------------------------------------------------------------------------------------------ the 32-column forms
@pytest.fixture(scope="module")
def child(dev):
    """tests/_skinny8_child.py in a fresh process with R4D_SKINNY16=0 (the library reads the word once per process)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_skinny8_child.py")
    p = subprocess.Popen([sys.executable, path], env=dict(os.environ, R4D_SKINNY16="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    o, e = p.communicate(timeout=120)
    assert p.returncode == 0, e[-3000:]
    return json.loads(o.strip().splitlines()[-1])


def test_32_column_forms_pass_the_gates(child):
    cases = child["cases"]
    assert len(cases) == 2 * 3 * 3 * 4 + 1
    bad = [c for c in cases if not c["ok"]]
    assert not bad, bad[:5]
    for c in cases:
        print(f"[rho] {c['label']} | {c['form']} | rho {c['rho']:.2f} | rho(seq32) {c['rho_seq32']:.2f} | measured gate {c['measured']:.1f} | "
              f"hard gate {c['hard']}")
        assert c["rho"] <= c["hard"] and c["rho"] <= c["measured"], c


def test_32_column_forms_count_their_branches(child):
    n = 2 * 3 * 3                                               # (K, M, N) combinations
    assert child["counters"] == {"skinny8:ng2": 4 * 4 * (n // 2) + 4, "skinny8:ng3": 4 * 4 * (n // 2),
                                 "tuning:skinny8:+layernorm": 4 * n, "skinny8:split-K + epilogue launch": 4}, child["counters"]


def test_32_column_forms_refuse_a_folded_layernorm(child):
    assert "folded LayerNorm needs the 16-column kernel" in child["fold_refused"], child["fold_refused"]


def test_every_skinny_branch_is_hit_by_this_file(run, child):
    """Every dispatcher branch of gemm_skinny.hip -- each ``skinny*`` counter and ``tuning:skinny8:+layernorm`` -- is reached by
    this file alone: seven small calls here for the 16-column and plain forms, the child's counters for the 32-column ones."""
    lib = run.lib
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    wanted = {n for n in names if n.startswith("skinny")} | {"tuning:skinny8:+layernorm"}
    assert len(wanted) == 11
    here = Runner(run.dev)
    for K, ln in ((256, None), (512, None), (768, None), (1024, None), (512, "launch"), (768, "launch"), (768, "fold")):
        here.call(R.make(2, K, 17, ln=bool(ln)), 2, 17, "none", ln=ln)
    hit = {n for n, c in here.total.items() if c} | {n for n, c in child["counters"].items() if c}
    assert hit >= wanted, sorted(wanted - hit)

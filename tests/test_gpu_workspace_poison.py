"""GPU tests of the buffer contract (include/r4d.h, "What a buffer may hold on entry"): workspace, output and gradient memory may
hold ANYTHING when an entry point is called -- the library writes every byte it later reads.  Every case runs one entry point (or
one trainer step) with all the memory the library allocates or caches filled with a byte pattern (tests/_poison.py): on the first
call through ``poisoned_allocations`` (every ``torch.empty`` of the Python side: workspaces, outputs, plane buffers, the key/value
cache), on a second call through ``poison`` on the buffers that now exist (``ops._WS``, a trainer's ``_ws`` and ``_scratch``,
``flat_grads``, the cache, the greedy decoder's ``ws`` and ``logits``).  The assertion is the same everywhere: the results under
each pattern equal the results under ZERO BIT FOR BIT.  No tolerance: the suite already asserts run-to-run bit determinism of all
these paths, and two runs that differ only in bytes the library must not read have nothing else to differ in.

Classification (read from the layout code of each entry; NAN and HUGE may only go where no word is ever used to form an address,
a loop bound or a length -- a latent bug must show as a failed assertion, never as a memory fault):

  entry point                           regions of its workspace                                            class      patterns
  ------------------------------------  ------------------------------------------------------------------  ---------  ----------
  r4d_gpt2_train_forward/backward_f32   TrainLayout: f32 activations, P / dP / PT, split-K partials,         values     all four
                                        the fixed-point dwte table (u64) + its poison and max words
  r4d_gpt2_lm_train_step_f32            LMLayout = TrainLayout + logits/dlogits [N, ldV] + the CE scratch    values     all four
  r4d_rag_train_step_f32                the RAG layout = LMLayout + the spliced rows                         values     all four
  r4d_retriever_losses_f32              f32 similarity tables and row reductions                             values     all four
  r4d_lm_ce_f32                         f32 row losses; tail: an int count used as a DIVISOR only            values     all four
  r4d_weight_grad_f32                   f32 split-K partials                                                 values     all four
  r4d_layernorm_bwd_f32                 f32 partial column sums                                              values     all four
  r4d_embedding_scatter_f32             u64 fixed-point table + poison and max words (behind a memset)       values     all four
  r4d_weighted_bag_f32                  no workspace (output only)                                           values     all four
  r4d_sumsq_accumulate_f32 (then        sumsq[1:]: one f32 partial per workgroup, min(ceil(n / 256), 1024)    values     all four
    r4d_adamw_step_f32, no workspace)   of them written and read; ([0], m, v: caller STATE, not poisoned)
  r4d_gpt2_encode*_f32                  carve(): f32 x/ln/qkv/att/fc/scores/pool, h2 words, f16x2 lines,     values     all four
                                        the key-blocked K image (u32 words, never an index)
  r4d_attention_f32                     f32 scores                                                           values     all four
  r4d_gpt2_decode_step_f32 / greedy     carve() with the skinny-GEMM pool: split-K ticket counters (compared  values     all four
                                        with ``== KS - 1``, never an index) + f32 partials; the cache rows
                                        at and past ``pos``; the greedy ``logits``
  r4d_score_topk_f32                    f32 scores, top-k tickets (compared only), candidate values and      values     all four
                                        candidate indices (i64 carried as values, never dereferenced)
  r4d_topk_f32 / r4d_topk_f64           tickets, candidates, (f64) the i64 index staging                     values     all four
  r4d_merge_topk_f32                    gathered candidates + the top-k workspace                            values     all four
  r4d_argsort_desc_f32 / _f64           sorted keys and u32 positions of every chunk: rank_scatter COUNTS     values     all four
                                        pairs below its own (<= 2048 per chunk); a position is compared,
                                        never dereferenced, and sort_chunks writes all 2048 slots of a chunk
  r4d_jaccard_prepared_f64              rank[vocab] (a shift count), counts, a_idx2 / b_idx2 (table          INDICES    ZERO, ONE
                                        indices of the main kernel), a_len / b_len (loop bounds), dense
                                        words, order (row indices): lengths and indices the kernel
                                        dereferences -- ONE is a valid token / length / row, NAN / HUGE not

Not poisoned, because they are caller STATE and not scratch (the header lists them): key/value cache rows below ``pos``, the
optimizer's ``m`` / ``v`` / ``sumsq[0]``, a trainer's workspace BETWEEN its forward and its backward, the zero rows of the padded
LM-head operand (``HeadOperand.pad``, ``torch.zeros``), the padding between the views of ``flat_grads`` when the clip norm is taken
over the flat buffer (``torch.zeros``; the library is handed the views as outputs and the flat buffer as an INPUT of the norm).
No entry point that takes a workspace is left out.

Two things the cases below rely on, checked rather than assumed:
  - ``AdamW.step`` clears all of ``sumsq`` before it accumulates, so poison put there through the optimizer never reaches a kernel;
    the scratch partials are therefore poisoned in a test that calls ``r4d_sumsq_accumulate_f32`` itself
    (``test_sumsq_and_adamw_kernels_do_not_read_unwritten_partials``).
  - The key-blocked K image (and the memset of its tail) is used only where the LayerNorms write f16x2 lines: gemm mode f16x2,
    d a multiple of 256, qkv not handed out.  Of the encode cases that is the d = 512 one; at d = 64 the ``h2 + kblk`` variant runs
    the f16x2 attention on row-major K words.  The test asserts on the dispatcher's branch counters which of the two ran.
"""
import types

import numpy as np
import pytest
import torch

import _train_modes
from _poison import ONE, PATTERNS, ZERO, poison, poisoned_allocations
from conftest import load_golden
from test_gpu_train_activation_recompute import TINY, WIDE
from test_gpu_train_attention_recompute import _batches, _demb, _enc_model

pytestmark = pytest.mark.gpu

VALUES, INDICES = PATTERNS, (ZERO, ONE)
BIG = ((3, 140), (4, 65), (2, 129))
DROPS = [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1)]
DROP_IDS = ["dropout off", "dropout 0.1"]
MODES = ["stored", "recompute"]
_WORD = dict(zip(PATTERNS, (0, -1, 0x7F7F7F7F, 1)))           # ZERO, NAN, HUGE, ONE as int32 words


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_switches_restored = _train_modes.switches_restored(force_stored=("attention", "activations"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _snap(d):
    return {k: v.detach().clone() for k, v in d.items() if v is not None}


def _assert_same(base, got, what):
    """Two lists of {name: tensor}: the same names, shapes and BITS."""
    assert len(base) == len(got)
    for k, (a, b) in enumerate(zip(base, got)):
        assert set(a) == set(b), (what, k, set(a) ^ set(b))
        bad = [n for n in a if a[n].shape != b[n].shape or a[n].dtype != b[n].dtype or not torch.equal(_bits(a[n]), _bits(b[n]))]
        report = {n: ("nan" if b[n].is_floating_point() and torch.isnan(b[n]).any() else
                      f"{int((_bits(a[n]) != _bits(b[n])).sum())} bytes differ") for n in bad if a[n].shape == b[n].shape}
        assert not bad, f"{what}, call {k}: {report}"


def _assert_poison_is_invisible(run, patterns=VALUES, finite=True):
    """``run(pattern)`` -> list of {name: tensor} (one dict per call).  ZERO is the baseline; it must be finite and non-trivial."""
    base = run(ZERO)
    for step in base:
        floats = [v for v in step.values() if v.is_floating_point()]
        if finite:
            assert all(torch.isfinite(v).all() for v in floats), "the baseline itself is not finite"
        assert sum(float(v.double().abs().sum()) for v in floats) > 0 or not floats
    for pattern in patterns[1:]:
        _assert_same(base, run(pattern), f"pattern {pattern}")
    return base


def _twice(pattern, call, buffers=lambda: ()):
    """First allocation, then reuse: ``call()`` with an empty workspace cache under poisoned allocations; then every cached
    workspace and every tensor of ``buffers()`` refilled, and ``call()`` again (its outputs are fresh poisoned allocations)."""
    from rag4dyg_amd import ops
    ops._WS.clear()
    out = []
    with poisoned_allocations(pattern):
        out.append(_snap(call()))
    for b in list(ops._WS.values()) + list(buffers()):
        poison(b, pattern)
    with poisoned_allocations(pattern):
        out.append(_snap(call()))
    return out


def _padding_keeps(tr, pattern):
    """Every word of the flat gradient buffer outside the gradient views still holds the pattern (nothing wrote there)."""
    flat = tr.flat_grads
    pad = torch.ones(flat.numel(), dtype=torch.bool, device=flat.device)
    for g in tr.grads.values():
        off = (g.data_ptr() - flat.data_ptr()) // 4
        pad[off:off + g.numel()] = False
    return bool((flat.view(torch.int32)[pad] == _WORD[pattern]).all())


# ================================================================================================ training: the three steps
def _trainer_copies(enc):
    return [t for dct in (enc._wt, enc._w3, enc._w3t, enc._h2) for t in dct.values()]


@pytest.mark.parametrize("activations", MODES, ids=["activations stored", "activations recompute"])
@pytest.mark.parametrize("attention", MODES, ids=["P stored", "P recompute"])
@pytest.mark.parametrize("drop", DROPS, ids=DROP_IDS)
@pytest.mark.parametrize("name,L,H,d,shapes", [TINY, WIDE], ids=[TINY[0], WIDE[0]])
def test_retriever_step_does_not_read_unwritten_memory(dev, name, L, H, d, shapes, drop, attention, activations, gemm_mode):
    """EncoderTrainer: a larger step first (first allocation of everything, under poison), then twice the step under test in the
    same, re-poisoned workspace.  Pooled output and EVERY gradient; ``flat_grads`` is poisoned before each backward (the header:
    gradients are overwritten) and the padding between its views must keep the poison."""
    from rag4dyg_amd import training
    m, _sd = _enc_model(dev, L, H, d)
    sequence = [BIG, shapes, shapes]

    def run(pattern):
        with poisoned_allocations(pattern):                                       # _wt / _w3 / _w3t / _h2 under poison
            tr = training.EncoderTrainer(m, dropout=drop, seed=77, attention=attention, activations=activations)
        out = []
        for k, sh in enumerate(sequence):
            batches = [b.to(dev) for b in _batches(97, sh, seed=len(sh) + k)]
            demb = _demb(sh, d, dev, seed=5 + k)
            if tr._ws is not None:
                ws_ptr = tr._ws.data_ptr()
                poison(tr._ws, pattern)
            with poisoned_allocations(pattern):
                emb = tr.forward(batches).clone()
            poison(tr.flat_grads, pattern)
            grads = _snap(tr.backward(demb))
            assert _padding_keeps(tr, pattern)
            assert k == 0 or tr._ws.data_ptr() == ws_ptr                          # the larger step's buffer, reused
            out.append(dict(grads, pooled=emb))
        return out
    _assert_poison_is_invisible(run)


@pytest.mark.parametrize("activations", MODES, ids=["activations stored", "activations recompute"])
@pytest.mark.parametrize("attention", MODES, ids=["P stored", "P recompute"])
@pytest.mark.parametrize("drop", DROPS, ids=DROP_IDS)
@pytest.mark.parametrize("name,L,H,d,shapes", [TINY, WIDE], ids=[TINY[0], WIDE[0]])
def test_lm_step_does_not_read_unwritten_memory(dev, name, L, H, d, shapes, drop, attention, activations, gemm_mode):
    """LMTrainer at V60 (ldV = 128 > V: the pad columns of dlogits and the pad rows of the planes are contracted over), L3 H2 d64
    and L2 H2 d256: (3,140) first, then the shapes under test -- (2,7), (3,33), (2,129), or (2,40) -- in the same re-poisoned
    workspace.  Loss and every gradient."""
    import test_gpu_lm_training as lm_tests
    from rag4dyg_amd.lm_training import LMTrainer
    m, _sd = lm_tests._model(dev, L, H, d, 60, seed=11)

    def run(pattern):
        with poisoned_allocations(pattern):                                       # the head planes too
            tr = LMTrainer(m, dropout=drop, seed=1234, attention=attention, activations=activations)
        assert tr.ldV > tr.V
        out = []
        for k, (B, T) in enumerate(((3, 140),) + shapes):
            ids = lm_tests._ids(60, B, T, seed=3 + k, pad=59).to(dev)
            poison(tr._ws, pattern)
            poison(tr.flat_grads, pattern)
            with poisoned_allocations(pattern):
                loss = tr.step(ids).clone()
            assert _padding_keeps(tr, pattern)
            out.append(dict(_snap(tr.grads), loss=loss.view(1)))
        return out
    _assert_poison_is_invisible(run)


@pytest.mark.parametrize("activations", MODES, ids=["activations stored", "activations recompute"])
@pytest.mark.parametrize("attention", MODES, ids=["P stored", "P recompute"])
@pytest.mark.parametrize("drop", DROPS, ids=DROP_IDS)
@pytest.mark.parametrize("freeze", [True, False], ids=["frozen", "unfrozen"])
@pytest.mark.parametrize("name,L,H,d,shapes", [TINY, WIDE], ids=[TINY[0], WIDE[0]])
def test_rag_step_does_not_read_unwritten_memory(dev, name, L, H, d, shapes, freeze, drop, attention, activations, gemm_mode):
    """GeneratorTrainer at V60, B = 3 (one bag per sequence), L3 H2 d64 and L2 H2 d256: T + 1 = 141 first, then the lengths of the
    shapes under test -- 7, 33, 129, or 40.  Loss, the ln_f rows, d_fused and every gradient of the trainable set.  Under ``freeze``
    the trainable set is lm_head.weight + gnn_fusion.* and the frozen transformer has no gradient buffer at all
    (``want_grads=False``): what must keep the poison is the rest of the flat buffer."""
    import test_gpu_generator_training as gen_tests
    from rag4dyg_amd.generator_training import GeneratorTrainer
    B = 3
    m, tok, idx, src = gen_tests._setup(dev, L, H, d, 60, B, 140, seed=11, freeze=freeze)
    bags = gen_tests._bags(idx, src, dev)

    def run(pattern):
        with poisoned_allocations(pattern):
            tr = GeneratorTrainer(m, freeze=freeze, dropout=drop, seed=1234, attention=attention, activations=activations)
        if freeze:
            assert set(tr.grads) == {"lm_head.weight", "gnn_fusion.convs.0.lin.weight", "gnn_fusion.convs.0.bias"}
        out = []
        for T in (140,) + tuple(T1 - 1 for _B, T1 in shapes):
            for b in [tr._ws, tr.flat_grads] + list(tr._scratch.values()):
                poison(b, pattern)
            with poisoned_allocations(pattern):
                h = torch.empty(B, T + 1, d, device=dev)
                loss = tr.step(tok[:, :T].contiguous().to(dev), bags, hidden_out=h).clone()
            assert _padding_keeps(tr, pattern)
            out.append(dict(_snap(tr.grads), loss=loss.view(1), hidden=h, d_fused=tr._scratch["d_fused"].clone()))
        return out
    _assert_poison_is_invisible(run)


# ================================================================================================ training: the kernels on their own
@pytest.mark.parametrize("rows,fin,fout", [(31, 64, 192), (1000, 132, 516)])
def test_weight_grad_kernel_does_not_read_unwritten_memory(dev, rows, fin, fout):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows)
    X, DY = torch.randn(rows, fin, generator=g).to(dev), torch.randn(rows, fout, generator=g).to(dev)
    keep = {}

    def call():
        if "ws" not in keep:
            keep["ws"] = torch.empty(max(int(lib.r4d_weight_grad_workspace_bytes(rows, fin, fout)), 256), dtype=torch.uint8, device=dev)
        dw, db = torch.empty(fin, fout, device=dev), torch.empty(fout, device=dev)
        _lib.check(lib.r4d_weight_grad_f32(X.data_ptr(), DY.data_ptr(), rows, fin, fout, dw.data_ptr(), db.data_ptr(), keep["ws"].data_ptr(),
                                           keep["ws"].numel(), _stream()), "weight_grad")
        return dict(dw=dw, db=db)

    def run(pattern):
        keep.clear()
        return _twice(pattern, call, lambda: [keep["ws"]])
    _assert_poison_is_invisible(run)


@pytest.mark.parametrize("rows,d", [(37, 256), (260, 1024)])
def test_layernorm_bwd_kernel_does_not_read_unwritten_memory(dev, rows, d):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows)
    X, W, DY = (torch.randn(*s, generator=g).to(dev) for s in ((rows, d), (d,), (rows, d)))
    keep = {}

    def call():
        if "ws" not in keep:
            keep["ws"] = torch.empty(max(int(lib.r4d_layernorm_bwd_workspace_bytes(rows, d)), 256), dtype=torch.uint8, device=dev)
        dx, dw, db = torch.empty(rows, d, device=dev), torch.empty(d, device=dev), torch.empty(d, device=dev)
        _lib.check(lib.r4d_layernorm_bwd_f32(X.data_ptr(), W.data_ptr(), DY.data_ptr(), None, rows, d, 1e-5, dx.data_ptr(), dw.data_ptr(),
                                             db.data_ptr(), keep["ws"].data_ptr(), keep["ws"].numel(), _stream()), "ln_bwd")
        return dict(dx=dx, dw=dw, db=db)

    def run(pattern):
        keep.clear()
        return _twice(pattern, call, lambda: [keep["ws"]])
    _assert_poison_is_invisible(run)


def test_lm_ce_kernel_does_not_read_unwritten_memory(dev):
    """V = 60 in ldV = 128 columns: the pad columns of the logits arrive holding the pattern and leave as exact zeros."""
    from rag4dyg_amd import _lib, ops
    from rag4dyg_amd.lm_training import padded_vocab
    lib = _lib.load()
    V, B, T = 60, 3, 17
    ldV, N = padded_vocab(V), B * T
    assert ldV > V
    g = torch.Generator().manual_seed(V + T)
    x, ids = torch.randn(N, V, generator=g).to(dev), torch.randint(0, V, (B, T), generator=g).to(dev)

    def call():
        logits = torch.empty(N, ldV, device=dev)                                 # pad columns: whatever the allocation holds
        logits[:, :V] = x
        ws = ops.workspace(lib.r4d_lm_ce_workspace_bytes(N), dev, "lm_ce_poison")
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(lib.r4d_lm_ce_f32(logits.data_ptr(), N, V, ldV, ids.data_ptr(), None, T, 1.0, loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _stream()), "lm_ce")
        assert torch.all(logits[:, V:] == 0)
        return dict(dlogits=logits, loss=loss.view(1))
    _assert_poison_is_invisible(lambda pattern: _twice(pattern, call))


def test_retriever_losses_kernel_does_not_read_unwritten_memory(dev):
    from rag4dyg_amd import training
    B, d = 6, 64
    g = torch.Generator().manual_seed(B)
    emb = torch.randn(5, B, d, generator=g).to(dev)
    ta, tp, tn = (torch.rand(B, generator=g) * 50 for _ in range(3))
    args = types.SimpleNamespace(temperature=0.07, lambda_decay=0.05, alpha=0.3, per_gpu_train_batch_size=B)

    def call():
        losses, demb = training.retriever_losses(args, emb, ta, tp, tn, grad_scale=0.5)
        only, none = training.retriever_losses(args, emb, ta, tp, tn, want_grad=False)
        assert none is None
        return dict(losses=losses, demb=demb, losses_only=only)
    _assert_poison_is_invisible(lambda pattern: _twice(pattern, call))


def test_weighted_bag_and_embedding_scatter_kernels_do_not_read_unwritten_memory(dev):
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    V, d, lens = 300, 192, [17, 1, 40, 9, 120]
    nb, n = len(lens), sum(lens)
    table, ids, w = torch.randn(V, d, generator=g).to(dev), torch.randint(0, V, (n,), generator=g).to(dev), torch.rand(n, generator=g).to(dev)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(dev)
    src = torch.randn(nb, d, generator=g).to(dev)
    row_of = torch.repeat_interleave(torch.arange(nb, dtype=torch.int32), torch.tensor(lens)).to(dev)

    def call():
        bag = torch.empty(nb, d, device=dev)
        _lib.check(lib.r4d_weighted_bag_f32(table.data_ptr(), V, d, ids.data_ptr(), w.data_ptr(), offs.data_ptr(), nb, bag.data_ptr(),
                                            _stream()), "weighted_bag")
        ws = ops.workspace(lib.r4d_embedding_scatter_workspace_bytes(V, d), dev, "scatter_poison")
        out = torch.empty(V, d, device=dev)
        _lib.check(lib.r4d_embedding_scatter_f32(src.data_ptr(), row_of.data_ptr(), w.data_ptr(), ids.data_ptr(), n, d, V, out.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream()), "embedding_scatter")
        return dict(bag=bag, scatter=out)
    _assert_poison_is_invisible(lambda pattern: _twice(pattern, call))


@pytest.mark.parametrize("n", [1000, 70001, 262144 + 77], ids=["4 partials", "274 partials", "all 1024 partials"])
def test_sumsq_and_adamw_kernels_do_not_read_unwritten_partials(dev, n):
    """``r4d_sumsq_accumulate_f32`` on its own (``AdamW.step`` zeroes the whole buffer first, so poison never survives to the kernels
    through the optimizer): ``sumsq[0] = 0`` is the caller's state, ``sumsq[1:]`` holds the pattern.  The launch writes
    min(ceil(n / 256), 1024) partials and must add up exactly those: at n = 1000 and 70001 the other 1020 and 750 slots stay
    unwritten (and must still hold the pattern afterwards).  Two tensors accumulate into the same total, as the optimizer does
    without a flat buffer, then a clipped ``r4d_adamw_step_f32`` reads ``sumsq[0]``: total, p, m and v equal the ZERO run's."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    g0, g1, p0, m0, v0 = (torch.randn(k, generator=g) for k in (n, 300, n, n, n))
    parts = min((n + 255) // 256, 1024)

    def run(pattern):
        grad, other, p, m, v = (t.to(dev) for t in (g0, g1, p0, m0 * 0.1, v0.square() * 0.01))
        sumsq = torch.zeros(1025, dtype=torch.float32, device=dev)
        poison(sumsq[1:], pattern)
        _lib.check(lib.r4d_sumsq_accumulate_f32(other.data_ptr(), other.numel(), sumsq.data_ptr(), _stream()), "sumsq")
        poison(sumsq[1:], pattern)
        _lib.check(lib.r4d_sumsq_accumulate_f32(grad.data_ptr(), n, sumsq.data_ptr(), _stream()), "sumsq")
        assert bool((sumsq[1 + parts:].view(torch.int32) == _WORD[pattern]).all())          # nothing wrote past the launch's partials
        _lib.check(lib.r4d_adamw_step_f32(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3,
                                          sumsq.data_ptr(), 1.0, _stream()), "adamw")
        return [dict(total=sumsq[:1].clone(), p=p, m=m, v=v)]
    base = _assert_poison_is_invisible(run)
    want = float(g0.double().square().sum() + g1.double().square().sum())
    assert abs(float(base[0]["total"]) / want - 1) < 1e-5 and want > 1.0               # the clip (max norm 1) is active


# ================================================================================================ optimizer step, then the derived copies
@pytest.mark.parametrize("kind", ["retriever", "lm"])
def test_optimizer_step_after_a_poisoned_backward_and_the_refreshed_copies(dev, kind, gemm_mode):
    """One clipped AdamW step after a poisoned backward: parameters, m and v equal the clean run's.  The gradient VIEWS are poisoned
    before the backward, the padding between them stays the trainer's zeros (the clip norm reads the flat buffer).  ``AdamW.step``
    clears ``sumsq`` itself, so its scratch partials are poisoned in the kernel test below, not here.  Then the derived copies
    (``_wt``, ``_w3``, ``_w3t``, ``_h2``, the LM head's padded planes) are poisoned and refreshed, and a second step and an inference
    encode run on them."""
    import test_gpu_lm_training as lm_tests
    from rag4dyg_amd import training
    from rag4dyg_amd.lm_training import LMTrainer
    name, L, H, d, shapes = TINY

    def run(pattern):
        from rag4dyg_amd import ops
        ops._WS.clear()
        if kind == "retriever":
            m, _sd = _enc_model(dev, L, H, d)
            batches = [b.to(dev) for b in _batches(97, shapes, seed=3)]
            demb = _demb(shapes, d, dev)
        else:
            m, _sd = lm_tests._model(dev, L, H, d, 60, seed=11)
            ids = lm_tests._ids(60, 3, 33, seed=3, pad=59).to(dev)
        with poisoned_allocations(pattern):
            tr = (training.EncoderTrainer(m, dropout=(0.1, 0.1, 0.1), seed=77) if kind == "retriever" else
                  LMTrainer(m, dropout=(0.1, 0.1, 0.1), seed=77))
        enc = tr if kind == "retriever" else tr.enc
        opt = training.AdamW(tr.params, tr.grads, lr=1e-3, weight_decay=0.01, flat_grads=tr.flat_grads)
        out = []

        def step():
            for gview in tr.grads.values():
                poison(gview, pattern)
            with poisoned_allocations(pattern):
                if kind == "retriever":
                    res = dict(pooled=tr.forward(batches).clone())
                    tr.backward(demb)
                else:
                    res = dict(loss=tr.step(ids).clone().view(1))
            return dict(res, **{"grad:" + n: g.clone() for n, g in tr.grads.items()})
        out.append(step())
        opt.step(1.0)
        out.append(dict({"p:" + n: p.detach().clone() for n, p in tr.params.items()}, **{"m:" + n: v.clone() for n, v in opt.m.items()},
                        **{"v:" + n: v.clone() for n, v in opt.v.items()}, norm=opt.sumsq[:1].clone()))
        for t in _trainer_copies(enc) + ([] if kind == "retriever" else [t for t in (tr.head._w3, tr.head._w3t, tr.head._h2) if t is not None]):
            poison(t, pattern)
        poison(tr._ws, pattern)
        if kind == "retriever":
            tr.refresh_transposed()                                               # (LMTrainer.step refreshes by its stamp)
        out.append(step())
        with poisoned_allocations(pattern):                                       # the inference path's own derived weights, rebuilt
            out.append(dict(encode=m.transformer.encode_groups_meanpool(batches if kind == "retriever" else [ids]).clone()))
        return out
    _assert_poison_is_invisible(run)


# ================================================================================================ inference
def _rag_model(dev, L, H, d, V, P, seed):
    from oracle import gpt2_ref
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=seed, random_affine=True)
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=P, n_ctx=P, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dev).eval()


@pytest.mark.parametrize("variant", ["fused", "h2 + kblk"])
@pytest.mark.parametrize("name,H,d,shapes", [("H2 d64", 2, 64, ((3, 1), (2, 33), (2, 129))), ("H2 d512 head_dim 256", 2, 512, ((2, 33),))],
                         ids=["H2 d64", "H2 d512 head_dim 256"])
def test_encode_and_encode_groups_do_not_read_unwritten_memory(dev, name, H, d, shapes, variant, gemm_mode):
    """``encode`` per batch (hidden + mean pool; then layers + qkv), ``encode_groups`` and ``encode_groups_meanpool`` over all
    batches; rows per call 3, 66, 258 and 327: none a multiple of 32.

    Which attention runs (asserted on the dispatcher's branch counters, so that a variant cannot silently run another one's code):
    ``h2 + kblk`` in gemm mode f16x2, in the calls that do not hand out qkv, takes the f16x2 attention -- at d = 512 (LayerNorm
    rows as f16x2 lines, which needs d % 256 == 0) on the key-blocked K image, whose tail block past row 66 is the memset this
    case is about; at d = 64 on row-major K words, with no key-blocked image.  ``fused``, the other two gemm modes and the
    ``want_qkv`` calls never take either."""
    from rag4dyg_amd import ops
    m = _rag_model(dev, 2, H, d, 97, 256, seed=5)
    tr = m.transformer
    batches = [b.to(dev) for b in _batches(97, shapes, seed=2)]
    assert all((B * T) % 32 for B, T in shapes) and sum(B * T for B, T in shapes) % 32
    hd = d // H
    watched = [f"attention:f16x2 {'key-split ' if hd < 128 else ''}hd{hd}{tail}" for tail in ("", ", key-blocked K")]
    before = [_branch_hits(n) for n in watched]
    # per call(): encode without qkv once per batch, encode_groups without qkv and encode_groups_meanpool once each; two layers;
    # call() runs twice per pattern
    launches = (len(batches) + 2) * 2 * 2 * len(PATTERNS) if variant != "fused" and gemm_mode == "f16x2" else 0
    want = [0, launches] if d % 256 == 0 else [launches, 0]
    was_h2, was_kblk = ops.set_attention_h2(variant != "fused"), ops.set_attention_kblk(variant != "fused")

    def call():
        out = {}
        for i, ids in enumerate(batches):
            r = tr.encode(ids, want_hidden=True, want_meanpool=True)
            out.update({f"hidden{i}": r["hidden"], f"pool{i}": r["meanpool"]})
            r = tr.encode(ids, want_hidden=False, want_meanpool=True, want_layers=True, want_qkv=True)
            out.update({f"layers{i}": r["layers"], f"qkv{i}": r["qkv"], f"pool_q{i}": r["meanpool"]})
        r = tr.encode_groups(batches, want_hidden=True, want_qkv=False, want_meanpool=True)
        out.update(g_hidden=r["hidden"], g_pool=r["meanpool"])
        out.update(g_qkv=tr.encode_groups(batches, want_hidden=False, want_qkv=True, want_meanpool=True)["qkv"])
        out.update(g_meanpool=tr.encode_groups_meanpool(batches))
        return out
    try:
        _assert_poison_is_invisible(lambda pattern: _twice(pattern, call))
    finally:
        ops.set_attention_h2(was_h2)
        ops.set_attention_kblk(was_kblk)
    assert [_branch_hits(n) - b for n, b in zip(watched, before)] == want, (watched, want)


def test_prefill_and_decode_steps_do_not_read_the_cache_past_pos(dev, gemm_mode):
    """L2 H2 d64, B = 5, V = 90: the cache is poisoned before the (ragged) prefill, so every row at and past ``pos`` holds the
    pattern when a decode step runs; five steps, the new hidden rows and the cache rows below ``pos`` are compared."""
    m = _rag_model(dev, 2, 2, 64, 90, 64, seed=12)
    tr = m.transformer
    B, t_cap = 5, 32
    g = torch.Generator().manual_seed(4)
    lens = [9, 3, 7, 1, 9]
    prompt = torch.randint(0, 89, (B, 9), generator=g).to(dev)
    new = torch.randint(0, 89, (5, B), generator=g).to(dev)
    keep = {}

    def call():
        if "cache" not in keep:
            keep["cache"] = tr.new_kv_cache(B, t_cap, dev)
        cache = keep["cache"]
        out = dict(last=tr.prefill_last(cache, lens, input_ids=prompt))
        pos = torch.tensor(lens, dtype=torch.int32, device=dev)
        for k in range(5):
            out[f"hidden{k}"] = tr.decode_step(cache, pos + k, input_ids=new[k])
        for i in range(B):
            out[f"cache{i}"] = cache[:, i, :lens[i] + 5]
        return out

    def run(pattern):
        keep.clear()
        return _twice(pattern, call, lambda: [keep["cache"]])
    _assert_poison_is_invisible(run)


@pytest.mark.parametrize("graph", [False, True], ids=["host loop", "graph"])
def test_greedy_loop_does_not_read_unwritten_memory(dev, graph, gemm_mode):
    """The greedy decoder (its own cache, ``ws`` and ``logits``; allocated under poison, BEFORE the graph is captured): the
    generated ids and the last logits.  Second run: cache, ``ws`` and ``logits`` refilled, prefill and run again."""
    from rag4dyg_amd.gpt2 import GreedyDecoder
    m = _rag_model(dev, 2, 2, 64, 90, 256, seed=12)
    tr = m.transformer
    B, t_cap = 5, 128
    lens = [9, 3, 7, 1, 9]
    prompt = torch.randint(0, 89, (B, 9), generator=torch.Generator().manual_seed(4)).to(dev)

    def run(pattern):
        from rag4dyg_amd import ops
        ops._WS.clear()
        with poisoned_allocations(pattern):
            dec = GreedyDecoder(tr, B, t_cap)
        dec.use_graph = graph
        out = []
        try:
            for _ in range(2):
                for b in (dec.cache, dec.ws, dec.logits):
                    poison(b, pattern)
                with poisoned_allocations(pattern):
                    last = tr.prefill_last(dec.cache, lens, input_ids=prompt)
                toks = dec.run(last, torch.tensor(lens), max_gen=6, len_limit=t_cap, eos=())      # no allocation wrapper while capturing
                assert all(len(t) == 6 for t in toks)
                out.append(dict(tokens=torch.tensor(toks), logits=dec.logits.clone(), last=last.clone()))
            assert dec.graph_builds == (1 if graph else 0)
        finally:
            dec.close()
        return out
    _assert_poison_is_invisible(run)


def test_attention_op_does_not_read_unwritten_memory(dev):
    from rag4dyg_amd import ops
    qkv = torch.randn(2, 129, 3 * 512, generator=torch.Generator().manual_seed(1)).to(dev)          # (B, T, H, head_dim) = (2, 129, 2, 256)
    for fused in (None, False):                                                    # auto, and the three-launch form that uses the scores workspace
        ops.set_attention_fused(fused)
        try:
            _assert_poison_is_invisible(lambda pattern: _twice(pattern, lambda: dict(a=ops.attention(qkv, 2))))
        finally:
            ops.set_attention_fused(None)


def _branch_hits(name):
    from rag4dyg_amd import _lib
    lib = _lib.load()
    for i in range(lib.r4d_dispatch_num_branches()):
        if lib.r4d_dispatch_branch_name(i).decode() == name:
            return int(lib.r4d_dispatch_branch_hits(i))
    raise KeyError(name)


@pytest.mark.parametrize("want_scores", [False, True], ids=["scores in the workspace", "scores handed out"])
def test_score_topk_does_not_read_unwritten_memory(dev, want_scores, gemm_mode):
    """k = 20 > 16 and N = 4097 = four segments + 1: the smallest pool whose rows are cut into two chunks, i.e. that takes the
    cross-workgroup ticket merge (asserted on the dispatcher's own counter)."""
    from rag4dyg_amd import ops
    g = torch.Generator().manual_seed(2)
    q, p = ops.normalize_rows(torch.randn(5, 64, generator=g).to(dev)), ops.normalize_rows(torch.randn(4097, 64, generator=g).to(dev))
    hits = _branch_hits("topk:cross-workgroup ticket merge")

    def call():
        v, i, S = ops.score_topk(q, p, 20, index_offset=3, want_scores=want_scores)
        return dict(vals=v, idx=i, scores=S)
    _assert_poison_is_invisible(lambda pattern: _twice(pattern, call))
    assert _branch_hits("topk:cross-workgroup ticket merge") >= hits + 8


@pytest.mark.parametrize("rows,n,k", [(4, 1025, 64), (3, 16384, 5), (3, 20000, 20), (2, 270000, 64)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_topk_does_not_read_unwritten_memory(dev, dtype, rows, n, k):
    """One workgroup per row (the first two shapes), five chunks merged behind the ticket (20000, k = 20), and 17 chunks x 64
    candidates > 1024: a second level that reads the first level's candidate values AND indices from the workspace."""
    from rag4dyg_amd import ops
    x = (torch.randn(rows, n, generator=torch.Generator().manual_seed(n)).double() * 3).round().div(3).to(dtype).to(dev)      # ties too
    fn = ops.topk_f32 if dtype == torch.float32 else ops.topk_f64

    def call():
        v, i = fn(x, k)
        return dict(vals=v, idx=i)
    _assert_poison_is_invisible(lambda pattern: _twice(pattern, call))


def test_merge_topk_does_not_read_unwritten_memory(dev):
    """G * k = 1280 > 1024: the gather + chunked top-k path (the one with a workspace)."""
    from rag4dyg_amd import ops
    rng = np.random.default_rng(5)
    G, Q, k = 20, 9, 64
    vals = -np.sort(-(np.round(rng.standard_normal((G, Q, k)) * 4).astype(np.float32) / 4), axis=2)
    idx = np.sort(rng.integers(0, 1000, (G, Q, k)), axis=2) + 1000 * np.arange(G)[:, None, None]
    v, i = torch.from_numpy(vals).to(dev), torch.from_numpy(idx.astype(np.int64)).to(dev)

    def call():
        ov, oi = ops.merge_topk(v, i)
        return dict(vals=ov, idx=oi)
    _assert_poison_is_invisible(lambda pattern: _twice(pattern, call))


@pytest.mark.parametrize("rows,n", [(3, 2049), (5, 65537)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_argsort_desc_does_not_read_unwritten_memory(dev, dtype, rows, n):
    from rag4dyg_amd import ops
    x = (torch.randn(rows, n, generator=torch.Generator().manual_seed(n)).double() * 50).round().div(50).to(dtype).to(dev)    # ties too
    _assert_poison_is_invisible(lambda pattern: _twice(pattern, lambda: dict(perm=ops.argsort_desc(x))))


@pytest.mark.parametrize("sort_rows", [False, True], ids=["rows in order", "sort_rows"])
@pytest.mark.parametrize("dense_split", [False, True], ids=["plain lists", "dense_split"])
def test_jaccard_does_not_read_unwritten_memory(dev, dense_split, sort_rows):
    """The UCI_13 fixture rows (test output sets against training input sets, and the training input sets against themselves).
    The prepared workspace holds lengths and indices the main kernel dereferences: ZERO and ONE only."""
    from rag4dyg_amd import ops
    g = load_golden("g5_jaccard_UCI_13")
    vocab = len(g["vocab_tokens"])
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("tr_in_ptr", "tr_in_idx", "te_out_ptr", "te_out_idx")}

    def call():
        return dict(cross=ops.jaccard(t["te_out_ptr"], t["te_out_idx"], t["tr_in_ptr"], t["tr_in_idx"], vocab, dense_split=dense_split,
                                      sort_rows=sort_rows),
                    self_=ops.jaccard(t["tr_in_ptr"], t["tr_in_idx"], t["tr_in_ptr"], t["tr_in_idx"], vocab, zero_diag=True,
                                      dense_split=dense_split, sort_rows=sort_rows))
    _assert_poison_is_invisible(lambda pattern: _twice(pattern, call), patterns=INDICES)

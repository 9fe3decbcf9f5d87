"""GPU tests of RAG generator training (``main_generator.py --do_train``): the spliced training step with one-layer graph pooling
against float64 torch autograd of the reference's calculus (``fusion_graphpooling`` + GPT-2 on ``inputs_embeds`` + shifted CE with
ignore_index -100) under all three arithmetics -- frozen transformer with the untied head (the shipped configuration) and the
unfrozen, tied model --, the frozen step's outputs against the unfrozen step's bit for bit, determinism, dropout given the same
masks, the forward-only loss, the new kernels on their own, and three AdamW steps with the frozen parameters left untouched."""
import numpy as np
import pytest
import torch

from conftest import elementwise_err, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _sources(V, n, seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, V - 2, int(g.integers(5, 16))).tolist() for _ in range(n)]


def _setup(dev, L, H, d, V, B, T, seed, freeze):
    """Model (+ one-layer GCN fusion; under ``freeze`` an untied random head), tokens, index lists, retrieval sources."""
    from oracle import gpt2_ref
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=256, seed=seed, random_affine=True)
    sd.pop("lm_head.weight", None)
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=256, n_ctx=256, n_embd=d, n_layer=L, n_head=H))
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    gnn = m.get_gnn(d, d // 2, d, 1, 0.2)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        gnn.convs[0].lin.weight.copy_(torch.randn(d, d, generator=g) * 0.05)
        gnn.convs[0].bias.copy_(torch.randn(d, generator=g) * 0.05)
    if freeze:
        m.lm_head.weight = torch.nn.Parameter(torch.randn(V, d, generator=g) * 0.05)
    m = m.to(dev).train()
    src = _sources(V, 40, seed)
    rng = np.random.default_rng(seed + 2)
    idx = [rng.choice(40, 7, replace=False).tolist() for _ in range(B)]
    tok = torch.randint(0, V - 2, (B, T), generator=g)
    for i in range(1, B):
        tok[i, int(torch.randint(T // 2, T + 1, (1,), generator=g)):] = V - 1       # right-padded; pad counted, as upstream
    return m, tok, idx, src


def _oracle(m, tok, idx, src, H, freeze, drop=None):
    """float64 autograd of fusion_graphpooling + the spliced forward + CE(ignore_index=-100)."""
    from oracle import generator_ref, gpt2_ref
    sd = {k: v.detach().cpu().double().requires_grad_(not freeze) for k, v in m.named_parameters() if k.startswith("transformer.")}
    conv = m.gnn_fusion.convs[0]
    W = conv.lin.weight.detach().cpu().double().requires_grad_(True)
    b = conv.bias.detach().cpu().double().requires_grad_(True)
    wte = sd["transformer.wte.weight"]
    rows = []
    for ix in idx:
        order, edges = generator_ref.star_union_graph(src, ix[:7])
        a = generator_ref.gcn_norm_dense(len(order), edges).double()
        rows.append(generator_ref.gcn_conv(wte[torch.tensor(order)], a, W, b).mean(dim=0))
    Ht = wte[tok]
    H_aug = torch.cat([Ht[:, :2], torch.stack(rows)[:, None], Ht[:, 2:]], dim=1)
    head = None
    if not freeze:
        sd["lm_head.weight"] = wte
    else:
        head = m.lm_head.weight.detach().cpu().double().requires_grad_(True)
        sd["lm_head.weight"] = head
    if drop is not None:
        drop.next_group(H_aug.shape[0], H_aug.shape[1])
    r = gpt2_ref.gpt2_forward.__wrapped__(sd, None, H, inputs_embeds=H_aug, want_logits=True, drop=drop)
    labels = torch.cat([tok[:, :2], torch.full((tok.shape[0], 1), -100), tok[:, 2:]], dim=1)
    lg = r["logits"][:, :-1].reshape(-1, r["logits"].shape[-1])
    loss = torch.nn.functional.cross_entropy(lg, labels[:, 1:].reshape(-1), ignore_index=-100)
    loss.backward()
    grads = {"gnn_fusion.convs.0.lin.weight": W.grad.float(), "gnn_fusion.convs.0.bias": b.grad.float()}
    if freeze:
        grads["lm_head.weight"] = head.grad.float()
    else:
        grads.update({k: v.grad.float() for k, v in sd.items() if k != "lm_head.weight"})
    return float(loss.detach()), grads, r["hidden"].detach()


def _bags(idx, src, dev):
    from rag4dyg_amd.generator_training import PreparedBags
    return PreparedBags(idx, src, 7).batch(range(len(idx)), dev)


def _check(tr, ref, loss, want):
    assert abs(float(loss) / want - 1) < 1e-5, (float(loss), want)
    assert set(tr.grads) == set(ref), set(tr.grads) ^ set(ref)
    worst = {n: rel_err(tr.grads[n].cpu().numpy(), ref[n].numpy()) for n in ref}
    assert max(worst.values()) < 1e-3, {n: e for n, e in worst.items() if e > 1e-3}
    ew = {n: elementwise_err(tr.grads[n].cpu().numpy(), ref[n].numpy(), rtol=1e-3, atol=1e-4) for n in ref}
    assert max(ew.values()) < 1, {n: e for n, e in ew.items() if e >= 1}


@pytest.mark.parametrize("L,H,d,V,B,T", [(2, 2, 64, 60, 3, 20),            # tiny
                                         (6, 8, 768, 1800, 4, 48),         # UCI_13 script shape
                                         (2, 2, 256, 500, 3, 40),          # hepth-like (head_dim 128)
                                         (2, 8, 512, 900, 3, 40)])         # reddit script shape (head_dim 64)
def test_frozen_graphpooling_step_equals_oracle(dev, L, H, d, V, B, T, gemm_mode):
    """The shipped configuration: --freeze, untied head, one-layer GCN, m = 1.  Loss and the gradients of lm_head.weight and
    gnn_fusion.convs.0.{lin.weight, bias} against float64 autograd; three repeated steps bit-identical."""
    from rag4dyg_amd.generator_training import GeneratorTrainer
    m, tok, idx, src = _setup(dev, L, H, d, V, B, T, seed=L * 100 + d + V, freeze=True)
    tr = GeneratorTrainer(m, freeze=True, dropout=(0.0, 0.0, 0.0))
    assert set(tr.params) == {"lm_head.weight", "gnn_fusion.convs.0.lin.weight", "gnn_fusion.convs.0.bias"}
    bags = _bags(idx, src, dev)
    loss = tr.step(tok.to(dev), bags)
    want, ref, _h = _oracle(m, tok, idx, src, H, freeze=True)
    _check(tr, ref, loss, want)
    first = {n: t.clone() for n, t in tr.grads.items()}
    for _ in range(2):
        assert torch.equal(tr.step(tok.to(dev), bags), loss)
        assert all(torch.equal(tr.grads[n], first[n]) for n in first)


@pytest.mark.parametrize("L,H,d,V,B,T", [(2, 2, 64, 60, 3, 20), (2, 4, 256, 300, 2, 30)])
def test_unfrozen_tied_graphpooling_step_equals_oracle(dev, L, H, d, V, B, T, gemm_mode):
    """Without --freeze: every parameter; wte = token scatter + the tied head's part + the fusion rows' scatter."""
    from rag4dyg_amd.generator_training import GeneratorTrainer
    m, tok, idx, src = _setup(dev, L, H, d, V, B, T, seed=7 + d, freeze=False)
    tr = GeneratorTrainer(m, freeze=False, dropout=(0.0, 0.0, 0.0))
    bags = _bags(idx, src, dev)
    loss = tr.step(tok.to(dev), bags)
    want, ref, _h = _oracle(m, tok, idx, src, H, freeze=False)
    _check(tr, ref, loss, want)
    first = {n: t.clone() for n, t in tr.grads.items()}
    for _ in range(2):
        assert torch.equal(tr.step(tok.to(dev), bags), loss)
        assert all(torch.equal(tr.grads[n], first[n]) for n in first)


def test_frozen_step_equals_unfrozen_step_bit_for_bit(dev):
    """Skipping the parameter gradients of the transformer changes nothing else: same loss, fusion gradients and hidden rows."""
    from rag4dyg_amd.generator_training import GeneratorTrainer
    m, tok, idx, src = _setup(dev, 2, 2, 128, 80, 3, 24, seed=31, freeze=True)
    bags = _bags(idx, src, dev)
    B, Ta = tok.shape[0], tok.shape[1] + 1
    frozen = GeneratorTrainer(m, freeze=True, dropout=(0.1, 0.1, 0.1), seed=5)
    h_f = torch.empty(B, Ta, 128, device=dev)
    loss_f = frozen.step(tok.to(dev), bags, hidden_out=h_f)
    g_f = {n: t.clone() for n, t in frozen.grads.items()}
    free = GeneratorTrainer(m, freeze=False, dropout=(0.1, 0.1, 0.1), seed=5)     # untied head, transformer trainable
    h_u = torch.empty_like(h_f)
    loss_u = free.step(tok.to(dev), bags, hidden_out=h_u)
    assert torch.equal(loss_f, loss_u) and torch.equal(h_f, h_u)
    for n in g_f:
        assert torch.equal(g_f[n], free.grads[n]), n


def test_step_with_dropout_equals_oracle_given_the_same_masks(dev):
    from oracle import train_ref
    from rag4dyg_amd.generator_training import GeneratorTrainer
    m, tok, idx, src = _setup(dev, 2, 2, 64, 60, 3, 20, seed=11, freeze=True)
    p = (0.1, 0.1, 0.1)
    tr = GeneratorTrainer(m, freeze=True, dropout=p, seed=1234)
    loss = tr.step(tok.to(dev), _bags(idx, src, dev))
    drop = train_ref.PhiloxDropout(*p, seed=1234, step=tr.enc.step)
    want, ref, _h = _oracle(m, tok, idx, src, 2, freeze=True, drop=drop)
    _check(tr, ref, loss, want)


def test_forward_only_loss_and_hidden_rows(dev):
    """backward=False (evaluate()): the same loss as the training step without dropout, no gradient written; the hidden rows
    through r4d_lm_logits_f32 reproduce the oracle's last-position logits."""
    from rag4dyg_amd import ops
    from rag4dyg_amd.generator_training import GeneratorTrainer
    m, tok, idx, src = _setup(dev, 2, 2, 64, 60, 2, 16, seed=17, freeze=True)
    tr = GeneratorTrainer(m, freeze=True, dropout=(0.0, 0.0, 0.0))
    bags = _bags(idx, src, dev)
    tr.flat_grads.fill_(7.0)
    h = torch.empty(2, 17, 64, device=dev)
    loss = tr.step(tok.to(dev), bags, backward=False, hidden_out=h)
    assert torch.all(tr.flat_grads == 7.0)
    want, _ref, h_ref = _oracle(m, tok, idx, src, 2, freeze=True)
    assert abs(float(loss) / want - 1) < 1e-5
    assert rel_err(h.cpu().numpy(), h_ref.numpy()) < 1e-4
    lg = ops.lm_logits(h[:, -1].contiguous(), m.lm_head.weight)
    ref_lg = h_ref[:, -1] @ m.lm_head.weight.detach().cpu().double().t()
    assert rel_err(lg.cpu().numpy(), ref_lg.numpy()) < 1e-4


def test_weighted_bag_and_scatter_kernels(dev):
    """r4d_weighted_bag_f32 against float64, r4d_embedding_scatter_f32 against index_add_ in float64 and bit-identical on
    relaunch and under a permutation of the contributions."""
    from rag4dyg_amd import _lib, ops
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(3)
    V, d, nb = 300, 192, 5
    table = torch.randn(V, d, generator=g)
    lens = [17, 1, 40, 9, 120]
    ids = torch.randint(0, V, (sum(lens),), generator=g)
    w = torch.rand(sum(lens), generator=g)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    out = torch.empty(nb, d, device=dev)
    table_d, ids_d, w_d, offs_d = table.to(dev), ids.to(dev), w.to(dev), offs.to(dev)       # alive through the launch
    _lib.check(lib.r4d_weighted_bag_f32(table_d.data_ptr(), V, d, ids_d.data_ptr(), w_d.data_ptr(), offs_d.data_ptr(), nb,
                                        out.data_ptr(), s), "bag")
    ref = torch.stack([(w[a:b, None].double() * table[ids[a:b]].double()).sum(0) for a, b in zip(offs[:-1], offs[1:])])
    assert rel_err(out.cpu().numpy(), ref.numpy()) < 1e-6
    src = torch.randn(nb, d, generator=g)
    row_of = torch.repeat_interleave(torch.arange(nb, dtype=torch.int32), torch.tensor(lens))
    ws = ops.workspace(lib.r4d_embedding_scatter_workspace_bytes(V, d), dev, "scatter_test")

    def scatter(perm):
        o = torch.empty(V, d, device=dev)
        args = [t.contiguous().to(dev) for t in (src, row_of[perm], w[perm], ids[perm])]
        _lib.check(lib.r4d_embedding_scatter_f32(*[t.data_ptr() for t in args], len(perm), d, V, o.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 s), "scatter")
        return o
    a = scatter(torch.arange(len(ids)))
    want = torch.zeros(V, d, dtype=torch.float64).index_add_(0, ids, w[:, None].double() * src[row_of.long()].double())
    assert rel_err(a.cpu().numpy(), want.numpy()) < 1e-6
    assert torch.equal(a, scatter(torch.arange(len(ids))))
    assert torch.equal(a, scatter(torch.randperm(len(ids), generator=g)))


def test_three_adamw_steps_track_the_oracle_and_leave_the_transformer(dev):
    """Under --freeze, --lrdecay 0 (linear warm-up) and 1 (cosine, training.adjust_learning_rate): three clipped AdamW updates of
    the trainable set against oracle.train_ref; every transformer parameter bit-identical afterwards."""
    import argparse
    from oracle import train_ref
    from rag4dyg_amd import training
    from rag4dyg_amd.generator_training import GeneratorTrainer
    from rag4dyg_amd.lm_training import LinearWarmupSchedule, linear_warmup_lambda
    for lrdecay in (0, 1):
        m, tok, idx, src = _setup(dev, 2, 2, 64, 60, 3, 20, seed=41 + lrdecay, freeze=True)
        before = {k: v.detach().clone() for k, v in m.transformer.state_dict().items()}
        tr = GeneratorTrainer(m, freeze=True, dropout=(0.0, 0.0, 0.0))
        bags = _bags(idx, src, dev)
        lr, wd, max_norm = 3e-3, 0.01, 0.5
        opt = training.AdamW(tr.params, tr.grads, lr=lr, eps=1e-8, weight_decay=wd, flat_grads=tr.flat_grads)
        sch = LinearWarmupSchedule(lr, 1, 4)
        args = argparse.Namespace(warmup_steps=1, num_train_epochs=3)
        lam = linear_warmup_lambda(1, 4)
        P = {k: v.detach().cpu().double() for k, v in tr.params.items()}
        M_ = {k: torch.zeros_like(v) for k, v in P.items()}
        V_ = {k: torch.zeros_like(v) for k, v in P.items()}
        for step in range(1, 4):
            if lrdecay == 1:
                training.adjust_learning_rate(args, opt, step - 1, lr, 1, 1)        # epoch step - 1, i = 1, one batch per epoch
                step_lr = opt.lr
            else:
                opt.lr = sch.lr
                step_lr = lr * lam(step - 1)
            tr.step(tok.to(dev), bags)
            _want, ref, _h = _oracle(m, tok, idx, src, 2, freeze=True)
            opt.step(max_norm)
            sch.step()
            coef, _ = train_ref.clip_coefficient(list(ref.values()), max_norm)
            for k in ref:
                decay = 0.0 if "bias" in k else wd
                P[k], M_[k], V_[k] = train_ref.adamw_step(P[k], ref[k].double() * coef, M_[k], V_[k], step, step_lr, (0.9, 0.999), 1e-8,
                                                          decay)
            for k in ref:
                assert rel_err(tr.params[k].detach().cpu().numpy(), P[k].numpy()) < 1e-5, (lrdecay, step, k)
        after = m.transformer.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)

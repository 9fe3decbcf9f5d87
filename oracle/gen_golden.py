#!/usr/bin/env python3
"""Generate tests/golden/*.npz by RUNNING THE REFERENCE'S OWN PYTHON MODULES on CPU.

Build-container only (``/root/reference`` does not exist on the GPU box).  This
script is ours; it imports the reference read-only through ``sys.path`` and
copies none of its source.  What it commits is data: inputs (token ids, CSR
sets, seeds) and the reference's outputs for them.

    cd /root/repo && python oracle/gen_golden.py            # all groups
    python oracle/gen_golden.py g1 g5                         # selected groups

Harness-side shims -- none touches the reference tree:
  * stub modules for uninstalled imports (boto3/botocore, torch_geometric, wandb,
    tensorboardX, ipdb) so ``models/*`` and ``train/*`` import;
  * run from a scratch cwd with ``vocabs``/``resources`` symlinks and a writable
    ``tokenizers/`` (``utils/tokenizer.py:35-38,49`` writes there);
  * ``tokenizer.batch_encode_plus`` no longer exists in transformers 5.x
    (``dataloader/retriever.py:23,53``) -> bound to ``__call__``.
Weights come from ``oracle.gpt2_ref.make_state_dict`` (seeded) and are LOADED
INTO the reference model, so reference and oracle/HIP see identical tensors
without committing them.
"""
import hashlib
import importlib.machinery
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from oracle import gpt2_ref  # noqa: E402


def _install_stubs():
    import transformers.activations  # noqa: F401  (before the boto3 stub)

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m

    class _Missing:
        def __init__(self, *a, **k):
            raise RuntimeError("stubbed dependency")

    stub("boto3"); stub("botocore"); stub("botocore.config", Config=object)
    stub("botocore.exceptions", ClientError=Exception)
    stub("torch_geometric"); stub("torch_geometric.nn", GCNConv=_Missing)
    stub("torch_geometric.utils", from_networkx=None)
    stub("wandb"); stub("tensorboardX", SummaryWriter=object); stub("ipdb")
    sys.path.insert(0, REF)


def _scratch_cwd():
    d = tempfile.mkdtemp(prefix="r4d_gold_")
    os.symlink(os.path.join(REF, "vocabs"), os.path.join(d, "vocabs"))
    os.symlink(os.path.join(REF, "resources"), os.path.join(d, "resources"))
    os.makedirs(os.path.join(d, "tokenizers"))
    os.chdir(d)
    return d


def _ref_model(flavour, n_layer, n_head, n_embd, vocab, n_positions, sd, output_hidden_states=False, output_attentions=False):
    from models import GPT2Config
    import models.modeling_gpt2 as mg
    import models.modeling_rag as mr
    cfg = GPT2Config(vocab_size=vocab, n_positions=n_positions, n_ctx=n_positions, n_embd=n_embd,
                     n_layer=n_layer, n_head=n_head)
    cfg.output_hidden_states = output_hidden_states
    cfg.output_attentions = output_attentions
    cls = {"gpt2": mg.GPT2LMHeadModel, "rag": mr.GPT2LMHeadModel}[flavour]
    m = cls(cfg).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith(".attn.bias") or k.endswith(".attn.masked_bias") for k in missing), missing   # causal buffers only (NOT c_attn.bias)
    return m


def _save(name, **arrs):
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


def _ragged(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]) if len(seqs) else np.zeros(0, np.int32)
    return flat, off


# --------------------------------------------------------------------------- G1
def g1_tiny_forward():
    """Tiny model, every layer's residual stream, ln_f output, logits, LM loss."""
    print("G1 tiny forward")
    L, H, d, V, P = 2, 2, 64, 40, 32
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=11, random_affine=True)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (3, 17), generator=g)
    out = {}
    with torch.no_grad():
        m = _ref_model("gpt2", L, H, d, V, P, sd, output_hidden_states=True)
        res = m(ids, labels=ids)                    # (loss, logits, presents, all_hidden)
        loss, logits, presents, hs = res
        out["loss"] = loss.numpy()
        out["logits"] = logits.numpy()
        out["present0"] = presents[0].numpy()        # [2,B,H,T,hd]
        for i, h in enumerate(hs[:-1]):
            out[f"layer{i}"] = h.numpy()             # residual stream entering block i
        out["hidden"] = hs[-1].numpy()               # ln_f output
        m2 = _ref_model("rag", L, H, d, V, P, sd)
        (logits2, _), hidden2 = m2(input_ids=ids)    # retriever flavour returns (outputs, hidden)
        assert torch.equal(logits2, logits) and torch.equal(hidden2, hs[-1])
        emb = wte_embeds = m2.transformer.wte(ids)
        (logits3, _), hidden3 = m2(inputs_embeds=emb)   # generator-style call
        assert torch.equal(hidden3, hidden2)
    _save("g1_tiny_forward", ids=ids.numpy(), cfg=np.array([L, H, d, V, P, 11]), **out)


# --------------------------------------------------------------------------- G2
def g2_ops():
    """Per-op vectors from the reference modules: LayerNorm, Conv1D, gelu_new MLP, _attn."""
    print("G2 per-op")
    from models import GPT2Config
    import models.modeling_gpt2 as mg
    from models.modeling_utils import Conv1D
    g = torch.Generator().manual_seed(7)
    out = {}
    with torch.no_grad():
        x = torch.randn(5, 9, 96, generator=g) * 3 + 0.5
        ln = torch.nn.LayerNorm(96, eps=1e-5)
        ln.weight.copy_(1 + 0.1 * torch.randn(96, generator=g)); ln.bias.copy_(0.1 * torch.randn(96, generator=g))
        out.update(ln_x=x.numpy(), ln_w=ln.weight.numpy(), ln_b=ln.bias.numpy(), ln_y=ln(x).numpy())
        c = Conv1D(80, 96)
        c.weight.copy_(torch.randn(96, 80, generator=g) * 0.05); c.bias.copy_(torch.randn(80, generator=g) * 0.1)
        out.update(conv_w=c.weight.numpy(), conv_b=c.bias.numpy(), conv_y=c(x).numpy())
        gx = torch.linspace(-6, 6, 257)
        out.update(gelu_x=gx.numpy(), gelu_y=mg.gelu_new(gx).numpy())
        for hd, T, scale in ((32, 40, 1.0), (64, 33, 1.0), (96, 24, 1.0), (128, 24, 1.0), (256, 20, 1.0), (64, 48, 30.0),
                              # (round 5: the head dims attention_h2.hip serves, logits x 900 -- appended, so every earlier vector keeps its draws)
                              (128, 48, 30.0), (256, 40, 30.0), (128, 61, 6.0), (256, 64, 6.0)):
            cfg = GPT2Config(vocab_size=8, n_positions=64, n_ctx=64, n_embd=2 * hd, n_layer=1, n_head=2)
            att = mg.Attention(2 * hd, 64, cfg, scale=True).eval()
            q = torch.randn(2, 2, T, hd, generator=g) * scale
            k = torch.randn(2, 2, hd, T, generator=g) * scale
            v = torch.randn(2, 2, T, hd, generator=g)
            a = att._attn(q, k, v)[0]
            tag = f"attn_hd{hd}_T{T}_s{int(scale)}"
            out.update({tag + "_q": q.numpy(), tag + "_k": k.numpy(), tag + "_v": v.numpy(), tag + "_a": a.numpy()})
    _save("g2_ops", **out)


# --------------------------------------------------------------------------- G3
def g3_config_shapes():
    """Config-shape forwards (cfg1 SimpleDyG B8xT128 incl. logits + loss; retriever shapes)."""
    print("G3 config shapes")
    shapes = {  # name: flavour, L, H, d, V, B, T, seed
        "cfg1_simpledyg": ("gpt2", 6, 8, 768, 1800, 8, 128, 101),
        "cfg2_uci": ("rag", 4, 2, 512, 1801, 32, 128, 102),
        "cfg4_wikiv2": ("rag", 2, 6, 768, 8814, 32, 96, 104),
        "hepth": ("rag", 12, 2, 256, 4756, 16, 80, 103),
    }
    for name, (fl, L, H, d, V, B, T, seed) in shapes.items():
        sd = gpt2_ref.make_state_dict(L, d, V, seed=seed, random_affine=True)
        g = torch.Generator().manual_seed(seed)
        ids = torch.randint(0, V, (B, T), generator=g)
        m = _ref_model(fl, L, H, d, V, 1024, sd)
        with torch.no_grad():
            if fl == "gpt2":
                loss, logits, _ = m(ids, labels=ids)
                hidden = m.transformer(ids)[0]
                extra = dict(loss=loss.numpy(), logits_rows=logits[:, [0, T // 2, T - 1], :].numpy())
            else:
                (logits, _), hidden = m(input_ids=ids)
                extra = dict(logits_rows=logits[:, [0, T - 1], :256].numpy())
        rows = [0, 1, T // 2, T - 1]
        _save("g3_" + name, cfg=np.array([L, H, d, V, B, T, seed]), ids=ids.numpy(),
              hidden_rows=hidden[:, rows, :].numpy(), rows=np.array(rows),
              meanpool=hidden.mean(dim=1).numpy(),
              hidden_abs_sum=np.array(hidden.double().abs().sum().item()), **extra)


# --------------------------------------------------------------------------- G4/G6
def _ref_tokenizer(dataset, timestamp):
    """Tokenizer built by the reference's own ``utils/tokenizer.get_model_tokenizer`` (tiny model).  hepth: the reference
    branches on the dataset NAME to inject node features with ``.cuda()`` (utils/tokenizer.py:56-66, cannot run on this
    CPU-only box); the tokenizer itself depends only on ``vocabs/<name>/<t>/vocab.json``, so the harness points an alias
    directory name at the same vocab file."""
    from models import GPT2Config
    import models.modeling_rag as mr
    from transformers import PreTrainedTokenizerFast
    from utils.tokenizer import get_model_tokenizer
    if dataset == "hepth":
        alias = "hepth_vocab_alias"
        os.makedirs("vocabs_alias/" + alias, exist_ok=True)
        if os.path.islink("vocabs"):                      # scratch cwd: replace the symlink by a directory of symlinks
            target = os.readlink("vocabs")
            os.remove("vocabs"); os.makedirs("vocabs")
            for name in os.listdir(target):
                os.symlink(os.path.join(target, name), os.path.join("vocabs", name))
        if not os.path.exists(os.path.join("vocabs", alias)):
            os.symlink(os.path.join(REF, "vocabs", "hepth"), os.path.join("vocabs", alias))
        dataset = alias
    args = types.SimpleNamespace(model_type="gpt2", config_name=None, model_name_or_path=None, cache_dir=None,
                                 n_head=2, n_layer=1, n_embed=16, eta=0.0, gamma=0.0, beta=0.0,
                                 timestamp=str(timestamp), dataset=dataset, device="cpu", node_feat_file=None)
    classes = {"gpt2": (GPT2Config, mr.GPT2LMHeadModel, PreTrainedTokenizerFast)}
    _, tok, _, _ = get_model_tokenizer(args, classes)
    if not hasattr(tok, "batch_encode_plus"):
        type(tok).batch_encode_plus = lambda self, lines, **kw: self(lines, **kw)
    return tok


def g4_g6_uci_retrieval():
    """UCI_13/12 through the reference tokenizer + datasets + model: ids, embeddings, scores, ranks."""
    print("G4/G6 UCI_13 retrieval")
    import dataloader.retriever as dr
    tok = _ref_tokenizer("UCI_13", 12)
    base = "resources/UCI_13/12/"
    args = types.SimpleNamespace()
    pool_ds = dr.LineByLineTextDatasetHistory(tok, args, base + "train.link_prediction", block_size=512)
    test_ds = dr.LineByLineTextDataset(tok, args, base + "test.link_prediction", block_size=512)
    val_ds = dr.LineByLineTextDataset(tok, args, base + "val.link_prediction", block_size=512)
    full_ds = dr.LineByLineTextDataset(tok, args, base + "train.link_prediction", block_size=512)
    # truncation case: 600-token line keeps the LAST 512
    long_line = "<|endoftext|> <|history|> 3 " + " ".join(str(i % 1700) for i in range(596)) + " <|endofhistory|>"
    trunc = tok.batch_encode_plus([long_line], add_special_tokens=True, max_length=512, truncation="longest_first")["input_ids"][0]
    special = {t: tok.convert_tokens_to_ids(t) for t in
               ["<|endoftext|>", "<|history|>", "<|endofhistory|>", "<|pre|>", "<|endofpre|>", "<|time0|>", "<|time12|>", "[PAD]", "[MASK]"]}
    pf, po = _ragged(pool_ds.examples); tf, to = _ragged(test_ds.examples); vf, vo = _ragged(val_ds.examples)
    ff, fo = _ragged(full_ds.examples[:40])
    _save("g6_uci_tokens", pool_flat=pf, pool_off=po, test_flat=tf, test_off=to, val_flat=vf, val_off=vo,
          full_flat=ff, full_off=fo, trunc_ids=np.asarray(trunc, np.int32),
          special_names=np.array(list(special.keys())), special_ids=np.array(list(special.values())),
          len_tok=np.array(len(tok)), vocab_size=np.array(tok.vocab_size), pad_id=np.array(tok.pad_token_id))

    L, H, d, V = 4, 2, 512, len(tok)
    assert V == 1801
    sd = gpt2_ref.make_state_dict(L, d, V, seed=2026, random_affine=True)
    m = _ref_model("rag", L, H, d, V, 1024, sd)

    def batches(examples):          # restates dataloader/retriever.py:153-166 around the reference model
        for s in range(0, len(examples), 32):
            ch = [torch.tensor(e, dtype=torch.long) for e in examples[s:s + 32]]
            yield torch.nn.utils.rnn.pad_sequence(ch, batch_first=True, padding_value=tok.pad_token_id)

    with torch.no_grad():
        pool = torch.cat([torch.mean(m(input_ids=b)[1], dim=1) for b in batches(pool_ds.examples)], dim=0)
        q = torch.cat([torch.mean(m(input_ids=b)[1], dim=1) for b in batches(test_ds.examples)], dim=0)
        qn = q / q.norm(dim=1, keepdim=True)                      # train_retriever.py:433-438
        pn = pool / pool.norm(dim=1, keepdim=True)
        S = (torch.matmul(qn, pn.t()) + 1) / 2
    S = S.numpy()
    top10 = np.argsort(-S, axis=1, kind="stable")[:, :10]
    _save("g4_uci_retrieval", seed=np.array(2026), pool_emb_head=pool[:64].numpy(), pool_emb_tail=pool[-52:].numpy(),
          pool_emb_norms=pool.norm(dim=1).numpy(), pool_emb_colsum=pool.double().sum(0).numpy(),
          query_emb=q.numpy(), scores=S, top10_stable=top10.astype(np.int32))


# --------------------------------------------------------------------------- G5
def g5_jaccard():
    """Jaccard matrices from the reference's own functions on UCI_13/12 and hepth/11."""
    print("G5 jaccard")
    import retrieval_data_annotation as rda
    for ds, ts in (("UCI_13", "12"), ("hepth", "11")):
        base = f"resources/{ds}/{ts}/"

        def rd(n):
            with open(base + n) as f:
                return [l for l in f.read().splitlines() if (len(l) > 0 and not l.isspace())]
        train, test, test_gt, val, val_gt = (rd(n) for n in ("train.link_prediction", "test.link_prediction",
                                                             "test_gt.link_prediction", "val.link_prediction",
                                                             "val_gt.link_prediction"))
        tr_in, tr_out = rda.get_inout_list(train, train)
        te_in, te_out = rda.get_inout_list(test, test_gt)
        va_in, va_out = rda.get_inout_list(val, val_gt)
        m_test = rda.occurrence_matrix(te_out, tr_out)
        m_val = rda.occurrence_matrix(va_out, tr_out)
        m_out = rda.occurrence_matrix(tr_out, tr_out)
        m_in = rda.occurrence_matrix(tr_in, tr_in)
        np.fill_diagonal(m_out, 0); np.fill_diagonal(m_in, 0)      # :172-173
        # reference train annotation (threshold 0.8, README); RNG column is not pinned
        rda.dataset = ds
        np.random.seed(0)
        rda.save_train_annotation(m_out, m_in, "ann_idx.txt", "ann_score.txt", threshold=0.8, neg_num=5)
        ann = np.loadtxt("ann_idx.txt", dtype=np.int64).reshape(-1, 3)
        from oracle.jaccard_ref import sets_to_csr          # inputs as data: CSR of the reference's token lists
        vocab = {}
        csr = {}
        for nm, seqs in (("tr_out", tr_out), ("tr_in", tr_in), ("te_out", te_out), ("va_out", va_out)):
            ip, ix, vocab = sets_to_csr(seqs, vocab)
            csr[nm + "_ptr"], csr[nm + "_idx"] = ip, ix
        csr["vocab_tokens"] = np.array(sorted(vocab, key=vocab.get))
        csr["tr_out_listlen"] = np.array([len(s) for s in tr_out], np.int32)
        rows = np.arange(0, m_out.shape[0], 97)
        sha = lambda a: np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)
        _save(f"g5_jaccard_{ds}", m_test=m_test, m_val=m_val,
              out_sha256=sha(m_out), in_sha256=sha(m_in), sample_rows=rows,
              out_rows=m_out[rows], in_rows=m_in[rows],
              out_top10=np.argsort(-m_out, axis=1, kind="stable")[:, :10].astype(np.int32),
              out_top10_val=np.take_along_axis(m_out, np.argsort(-m_out, axis=1, kind="stable")[:, :10], axis=1),
              out_rowsum=m_out.sum(1), in_rowsum=m_in.sum(1), ann_triples=ann,
              n=np.array([len(train), len(test), len(val)]), **csr)


def g6_more_tokenizers():
    """G6 for the other two shipped datasets: hepth/11 and dialog/15 ids of the first lines of every split."""
    print("G6 hepth / dialog tokens")
    import dataloader.retriever as dr
    for ds, ts, block in (("hepth", 11, 1024), ("dialog", 15, 1024)):
        tok = _ref_tokenizer(ds, ts)
        base = f"resources/{ds}/{ts}/"
        args = types.SimpleNamespace()
        out = {}
        for split, cls in (("train", dr.LineByLineTextDatasetHistory), ("test", dr.LineByLineTextDataset), ("val", dr.LineByLineTextDataset)):
            with open(base + f"{split}.link_prediction") as f:
                lines = [l for l in f.read().splitlines() if l.strip()][:40]
            with open(f"g6_{ds}_{split}.txt", "w") as f:
                f.write("\n".join(lines) + "\n")
            d_ = cls(tok, args, f"g6_{ds}_{split}.txt", block_size=block)
            out[split + "_flat"], out[split + "_off"] = _ragged(d_.examples)
        names = ["<|endoftext|>", "<|history|>", "<|endofhistory|>", "<|pre|>", "<|endofpre|>", "<|time0|>", f"<|time{ts}|>", "[PAD]", "[MASK]"]
        _save(f"g6_{ds}_tokens", special_names=np.array(names), special_ids=np.array([tok.convert_tokens_to_ids(t_) for t_ in names]),
              len_tok=np.array(len(tok)), vocab_size=np.array(tok.vocab_size), pad_id=np.array(tok.pad_token_id), **out)


# --------------------------------------------------------------------------- G7
def _import_utils_model():
    """``utils/model.py`` imports ``transformers.AdamW`` (gone in transformers 5.x): harness-side alias."""
    import transformers
    if not hasattr(transformers, "AdamW"):
        transformers.AdamW = torch.optim.AdamW
    import utils.model as um
    return um


# fusion_mlp + greedy loop around the reference's own ``utils.model.fusion_mlp`` (used by g7 and g12)
def _run_fusion(out, um, tag, L, H, d, V, pad_id, eos_id, sources, queries, idxs, m, n_layers, topk, seed, n_gen=11):
    from oracle import generator_ref
    sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=seed, random_affine=True)
    model = _ref_model("rag", L, H, d, V, 1024, sd)
    mlp = model.get_mlp(512, m, n_layers)
    mlp.load_state_dict(generator_ref.make_mlp_state(seed + 1, 512, m, n_layers))
    args = types.SimpleNamespace(device="cpu", n_embed=d, m=m)
    tok = types.SimpleNamespace(pad_token_id=pad_id)
    ds = types.SimpleNamespace(retrieval_sources=sources)
    gen, first_logits, step_top = [], [], []
    with torch.no_grad():
        for q, ix in zip(queries, idxs):
            toks = list(q)
            ids_sim = torch.tensor(ix, dtype=torch.long)
            g_, tops = [], []
            while True:                       # Evaluation_generator.py:153-175, val mode, around the reference fusion_mlp
                logits = um.fusion_mlp(args, model, tok, ds, torch.tensor([toks]), ids_sim, m, top_k=topk)
                last = logits[0, -1, :]
                if not g_:
                    first_logits.append(last.numpy().copy())
                nxt = int(torch.argmax(last).item())
                tv, ti = torch.topk(last, 2)
                tops.append([float(tv[0]), float(tv[1])])
                toks.append(nxt); g_.append(nxt)
                if len(g_) > n_gen - 1 or nxt == eos_id:
                    break
            gen.append(g_); step_top.append(tops)
        # batched call (B > 1, equal lengths): the flat `view` reshapes mix the batch dimension exactly as upstream
        same = [q for q in queries if len(q) == len(queries[0])][:2]
        if len(same) == 2:
            bl = um.fusion_mlp(args, model, tok, ds, torch.tensor(same), torch.tensor(idxs[:2], dtype=torch.long), m, top_k=topk)
            out[tag + "_batch2_last"] = bl[:, -1, :64].numpy()
    used = sorted({int(i) for ix in idxs for i in ix[:topk]})
    sf, so = _ragged([sources[i] for i in used])
    qf, qo = _ragged(queries); gf, go = _ragged(gen)
    tt = np.full((len(gen), n_gen, 2), np.nan, np.float32)
    for i, tps in enumerate(step_top):
        tt[i, :len(tps)] = np.asarray(tps, np.float32)
    out.update({tag + "_cfg": np.array([L, H, d, V, pad_id, eos_id, m, n_layers, topk, seed]),
                tag + "_src_ids": np.asarray(used, np.int64), tag + "_src_flat": sf, tag + "_src_off": so,
                tag + "_q_flat": qf, tag + "_q_off": qo, tag + "_idxs": np.asarray(idxs, np.int64),
                tag + "_gen_flat": gf, tag + "_gen_off": go, tag + "_first_logits": np.asarray(first_logits[:2]),
                tag + "_step_top2": tt})


def g7_generator():
    """RAG generator side, from the reference's own code on CPU:
    Evaluation metrics of both ``utils/Evaluation_*.py``, ``MLP_custom`` vectors, ``fusion_mlp`` logits and the greedy
    loop of ``Evaluation_generator.py:153-175`` restated around the reference's ``fusion_mlp`` (tiny and reddit shape),
    the SimpleDyG greedy loop of ``Evaluation_SimpleDyG.py:126-145`` around the reference model, ``TextIndexScoreDataset``.
    NOT pinned: ``fusion_graphpooling`` -- ``GCNConv`` / ``from_networkx`` come from torch_geometric, absent here."""
    print("G7 generator / evaluation")
    import models.modeling_rag as mr
    from oracle import generator_ref
    from rag4dyg_amd import synth
    um = _import_utils_model()
    out = {}

    # ---- (a) metrics: both Evaluation classes, random prediction / target token lists
    import utils.Evaluation_generator as eg
    import utils.Evaluation_SimpleDyG as es
    rng = np.random.default_rng(77)
    preds, tgts, rows = [], [], []
    for _ in range(60):
        tg = [str(x) for x in rng.choice(40, size=int(rng.integers(1, 9)), replace=False)]
        pr = [str(x) for x in rng.choice(40, size=int(rng.integers(0, 12)), replace=True)]
        if rng.random() < 0.5:
            pr = tg[:int(rng.integers(0, len(tg) + 1))] + pr
        preds.append(pr); tgts.append(tg)
        row = []
        for Ev in (eg.Evaluation(), es.Evaluation()):
            row += [Ev.jaccard(pr, tg)] if (pr or tg) else [0.0]
            for k in (1, 3, 5):
                row += [Ev.ndcg_k(pr, tg, k), Ev.recall_k(pr, tg, k), Ev.precision_k(pr, tg, k), Ev.map_k(pr, tg, k)]
        rows.append(row)
    pf, po = _ragged([[int(x) for x in p_] for p_ in preds]); tf, to = _ragged([[int(x) for x in t_] for t_ in tgts])
    out.update(met_pred_flat=pf, met_pred_off=po, met_tgt_flat=tf, met_tgt_off=to, met_values=np.asarray(rows, np.float64))

    # ---- (b) MLP_custom forward
    with torch.no_grad():
        for n_layers, m in ((1, 1), (2, 3), (3, 2)):
            ref = mr.MLP_custom(512, m, n_layers).eval()
            sdm = generator_ref.make_mlp_state(900 + n_layers, 512, m, n_layers)
            ref.load_state_dict(sdm)
            x = torch.randn(24, 512, generator=torch.Generator().manual_seed(n_layers)) * 0.7
            out[f"mlp{n_layers}_x"] = x.numpy(); out[f"mlp{n_layers}_y"] = ref(x).numpy()
            out[f"mlp{n_layers}_cfg"] = np.array([512, m, n_layers, 900 + n_layers])

    # ---- (c) fusion_mlp + greedy loop, tiny and reddit (BASELINE config 5) shapes
    def run_fusion(*a, **k):
        _run_fusion(out, um, *a, **k)

    rng = np.random.default_rng(5)
    V, pad, eos = 79, 78, 60
    srcs = [[eos, 61] + rng.integers(0, 60, int(rng.integers(3, 30))).tolist() + [62] for _ in range(40)]
    qs = [[eos, 61] + rng.integers(0, 60, n).tolist() + [62] for n in (9, 9, 14, 5)]
    run_fusion("fmlp_tiny", 2, 2, 64, V, pad, eos, srcs, qs, [rng.permutation(40)[:7].tolist() for _ in qs], 3, 2, 5, 310)
    sh = synth.SHAPES["reddit"]
    Vr = sh.vocab_generator
    assert Vr == 11919
    pool = [s_.tolist() for s_ in synth.sequences(sh, 10527, "pool", seed=2026)]
    qr = [s_.tolist() for s_ in synth.sequences(sh, 6, "query", seed=31)]
    rng = np.random.default_rng(6)
    run_fusion("fmlp_reddit", 2, 8, 512, Vr, sh.pad_id, sh.v0, pool, qr, [rng.permutation(10527)[:7].tolist() for _ in qr],
               1, 1, 7, 320)

    # ---- (d) SimpleDyG greedy loop (Evaluation_SimpleDyG.py:126-145) around the reference model, val + test stop rules
    def run_simpledyg(tag, L, H, d, V, eos_id, prompts, seed, max_len, n_spl):
        sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=seed, random_affine=True)
        model = _ref_model("gpt2", L, H, d, V, 1024, sd)
        res = {}
        with torch.no_grad():
            for mode in ("val", "test"):
                gens = []
                for pr in prompts:
                    toks, gen_len = list(pr), 0
                    while True:
                        nxt = int(torch.argmax(model(torch.tensor([toks]))[0][0, -1, :]).item())
                        toks.append(nxt); gen_len += 1
                        if mode == "val":
                            if gen_len > 10:
                                break
                        elif len(toks) >= max_len - n_spl:
                            break
                        if nxt == eos_id:
                            break
                    gens.append(toks[len(pr):])
                res[mode] = gens
        pf_, po_ = _ragged(prompts)
        out.update({tag + "_cfg": np.array([L, H, d, V, eos_id, seed, max_len, n_spl]), tag + "_p_flat": pf_, tag + "_p_off": po_})
        for mode in ("val", "test"):
            gf_, go_ = _ragged(res[mode])
            out.update({f"{tag}_{mode}_flat": gf_, f"{tag}_{mode}_off": go_})

    rng = np.random.default_rng(8)
    run_simpledyg("sdg_tiny", 2, 2, 64, 79, 60, [[60, 61] + rng.integers(0, 60, n).tolist() + [62] for n in (4, 11, 7)],
                  330, max_len=40, n_spl=6)
    uci = synth.SHAPES["UCI_13"]
    run_simpledyg("sdg_cfg1", 6, 8, 768, uci.vocab_generator, uci.v0,
                  [s_.tolist() for s_ in synth.sequences(uci, 4, "query", seed=41)], 340, max_len=1024, n_spl=19)

    # ---- (e) TextIndexScoreDataset (dataloader/generator.py:12-80) on the shipped UCI_13 files + a small index/score pair
    import dataloader.generator as dg
    tok = _ref_tokenizer("UCI_13", 12)
    base = "resources/UCI_13/12/"
    with open(base + "test.link_prediction") as f:
        lines = [l for l in f.read().splitlines() if l.strip()][:12]
    rng = np.random.default_rng(9)
    idx_rows = [rng.permutation(1708)[:8].tolist() for _ in lines]
    sc_rows = [np.round(np.sort(rng.random(8))[::-1], 4).tolist() for _ in lines]
    with open("g7_text.txt", "w") as f:
        f.write("\n".join(lines) + "\n\n")
    with open("g7_index.txt", "w") as f:
        f.write("\n".join(" ".join(map(str, r)) for r in idx_rows) + "\n")
    with open("g7_score.txt", "w") as f:
        f.write("\n".join(" ".join(f"{x:.4f}" for x in r) for r in sc_rows) + "\n")
    ds = dg.TextIndexScoreDataset(tok, types.SimpleNamespace(train_data_file=base + "train.link_prediction"),
                                  "g7_text.txt", "g7_index.txt", "g7_score.txt", block_size=512)
    tf_, to_ = _ragged(ds.text); rf_, ro_ = _ragged(ds.retrieval_sources[:25])
    item = ds[3]
    out.update(tis_text_flat=tf_, tis_text_off=to_, tis_src_flat=rf_, tis_src_off=ro_, tis_n_sources=np.array(len(ds.retrieval_sources)),
               tis_index=np.asarray(ds.index, np.int64), tis_score=np.asarray(ds.score, np.float64),
               tis_egolist=np.asarray(ds.egolist, np.int64), tis_lines=np.array(lines),
               tis_item3_text=item[0].numpy(), tis_item3_index=item[1].numpy(), tis_item3_score=item[2].numpy(),
               tis_item3_ego=item[3].numpy(), tis_ego_lookup=ds.get_item_by_egoId(int(ds.egolist[5])).numpy())
    _save("g7_generator", **out)


# --------------------------------------------------------------------------- G8
def g8_training_step():
    """Retriever training step, forward + loss + gradients, from the reference's own code on CPU:
    ``CLtime_loss`` / ``info_nce`` / ``mask_correlated_samples`` (train/train_retriever.py:40-98), ``_aug``
    (models/modeling_rag.py:774-840, python ``random`` seeded), ``PairSequenceDataset`` (dataloader/retriever.py:68-111), and
    one whole step of ``train_epoch`` (:177-196) with autograd -- dropout probabilities set to 0 (the reference trains with
    p = 0.1, whose masks are not reproducible across devices)."""
    print("G8 retriever training step")
    import random
    from models import GPT2Config
    import models.modeling_rag as mr
    _import_utils_model()
    import train.train_retriever as tr
    import dataloader.retriever as dr
    out = {}

    # ---- (a) the two losses on seeded embeddings / times
    g = torch.Generator().manual_seed(21)
    for tag, B, d in (("l4", 4, 16), ("l32", 32, 64)):
        a, p_, n_ = (torch.randn(B, d, generator=g) for _ in range(3))
        ta, tp, tn = (torch.rand(B, 1, generator=g) * 30 for _ in range(3))
        args = types.SimpleNamespace(temperature=0.07, lambda_decay=0.05, per_gpu_train_batch_size=B)
        out[tag + "_emb"] = torch.stack([a, p_, n_]).numpy(); out[tag + "_time"] = torch.stack([ta, tp, tn]).numpy()
        out[tag + "_cltime"] = np.array(tr.CLtime_loss(args, a, p_, n_, ta, tp, tn).item())
        z1 = torch.nn.functional.normalize(a, dim=1); z2 = torch.nn.functional.normalize(p_, dim=1)
        mask = tr.mask_correlated_samples(B)
        out[tag + "_mask"] = mask.numpy()
        out[tag + "_infonce"] = np.array(tr.info_nce(args, z1, z2, 0.07, B, mask).item())
        out[tag + "_infonce_raw"] = np.array(tr.info_nce(args, a, p_, 0.07, B, mask).item())
        args.per_gpu_train_batch_size = B + 1                      # last partial batch: the mask is rebuilt (:92-93)
        out[tag + "_infonce_rebuilt"] = np.array(tr.info_nce(args, a, p_, 0.07, B, None).item())

    # ---- (b) one training step at a tiny and at the cfg2 (UCI retriever) shape
    def step(tag, L, H, d, V, pad, B, lens, seed, eta, gamma, alpha):
        cfg = GPT2Config(vocab_size=V, n_positions=1024, n_ctx=1024, n_embd=d, n_layer=L, n_head=H,
                         resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
        cfg.eta, cfg.gamma, cfg.beta = eta, gamma, 0.0
        model = mr.GPT2LMHeadModel(cfg)
        sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=seed, random_affine=True)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected
        model.train()
        rng = np.random.default_rng(seed)

        def batch():
            rows = [rng.integers(1, V - 2, int(n)).tolist() for n in rng.choice(lens, B)]
            T = max(len(r) for r in rows)
            return torch.tensor([r + [pad] * (T - len(r)) for r in rows], dtype=torch.long)
        anchor, pos, neg = batch(), batch(), batch()
        n_pool = 50
        all_t = torch.tensor(rng.random(n_pool) * 40, dtype=torch.float)
        ai, pi, ni = (torch.tensor(rng.integers(0, n_pool, (B, 1)), dtype=torch.long) for _ in range(3))
        args = types.SimpleNamespace(temperature=0.07, lambda_decay=0.05, per_gpu_train_batch_size=B, alpha=alpha)
        _, h_ego = model(input_ids=anchor); _, h_pos = model(input_ids=pos); _, h_neg = model(input_ids=neg)
        h_egos, h_i, h_j = h_ego.mean(1), h_pos.mean(1), h_neg.mean(1)
        cl = tr.CLtime_loss(args, h_egos, h_i, h_j, all_t[ai], all_t[pi], all_t[ni])
        random.seed(seed)
        aug1, aug2 = model._aug(anchor)
        _, s1 = model(input_ids=aug1); _, s2 = model(input_ids=aug2)
        aug = args.alpha * tr.info_nce(args, s1.mean(1), s2.mean(1), args.temperature, aug1.size(0), tr.mask_correlated_samples(B))
        loss = cl + aug
        loss.backward()
        names = [n for n, p_ in model.named_parameters() if p_.grad is not None]
        gn = np.array([model.get_parameter(n).grad.double().norm().item() for n in names])
        out.update({tag + "_cfg": np.array([L, H, d, V, pad, B, seed]), tag + "_hyper": np.array([eta, gamma, alpha, 0.07, 0.05]),
                    tag + "_anchor": anchor.numpy(), tag + "_pos": pos.numpy(), tag + "_neg": neg.numpy(),
                    tag + "_times": all_t.numpy(), tag + "_idx": torch.cat([ai, pi, ni], 1).numpy(),
                    tag + "_aug1": aug1.numpy(), tag + "_aug2": aug2.numpy(),
                    tag + "_emb": torch.stack([h_egos, h_i, h_j, s1.mean(1), s2.mean(1)]).detach().numpy(),
                    tag + "_losses": np.array([cl.item(), aug.item(), loss.item()]),
                    tag + "_grad_names": np.array(names), tag + "_grad_norms": gn,
                    tag + "_grad_lnf_w": model.transformer.ln_f.weight.grad.numpy().copy(),
                    tag + "_grad_cattn_b0": model.transformer.h[0].attn.c_attn.bias.grad.numpy().copy(),
                    tag + "_grad_wte_rows": model.transformer.wte.weight.grad[:8].numpy().copy()})
        if tag == "ts_tiny":        # EVERY parameter gradient of the small step (wpe: the rows a 64-position batch can touch)
            for n in names:
                gr = model.get_parameter(n).grad
                out[tag + "_grad_all:" + n] = (gr[:64] if n.endswith("wpe.weight") else gr).numpy().copy()

    step("ts_tiny", 2, 2, 64, 80, 78, 4, [9, 12, 17, 23], 410, 0.2, 0.5, 0.1)
    step("ts_cfg2", 4, 2, 512, 1801, 1799, 8, [12, 20, 37, 60], 420, 0.2, 0.5, 0.1)

    # ---- (c) PairSequenceDataset on the shipped UCI_13 train file + a small triples file
    tok = _ref_tokenizer("UCI_13", 12)
    rng = np.random.default_rng(3)
    triples = rng.integers(0, 1708, (10, 3))
    with open("g8_pairs.txt", "w") as f:
        f.write("\n".join(" ".join(map(str, r)) for r in triples.tolist()) + "\n")
    ds = dr.PairSequenceDataset(tok, types.SimpleNamespace(train_data_file="resources/UCI_13/12/train.link_prediction"),
                                "g8_pairs.txt", block_size=512)
    af, ao = _ragged(ds.anchor); pf, po = _ragged(ds.positive); nf, no = _ragged(ds.negative)
    item = ds[2]
    out.update(pair_triples=triples, pair_anchor_flat=af, pair_anchor_off=ao, pair_pos_flat=pf, pair_pos_off=po,
               pair_neg_flat=nf, pair_neg_off=no, pair_item2_anchor=item[0].numpy(), pair_item2_idx=np.array([int(item[3]), int(item[4]), int(item[5])]))
    _save("g8_training_step", **out)


def g14_loss_head_edges():
    """The reference's own ``CLtime_loss`` / ``info_nce`` (with the passed and with the rebuilt mask) / ``mask_correlated_samples``
    (train/train_retriever.py:40-98) in float32 on the edge inputs of ``tests/_loss_head_ref.py``: every regime at B in {2, 3, 17}
    (d <= 65), ``unit`` at B = 65, d = 80; and the record that ``CLtime_loss`` raises at B = 1."""
    print("G14 loss head edges")
    _import_utils_model()
    import train.train_retriever as tr
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _loss_head_ref as lh
    out, tags = {}, []
    for tag, regime, B, d, tau, lam in lh.g14_entries():
        emb, ta, tp, tn = lh.make_inputs(regime, B, d)
        args = types.SimpleNamespace(temperature=tau, lambda_decay=lam, per_gpu_train_batch_size=B)
        mask = tr.mask_correlated_samples(B)
        cl = tr.CLtime_loss(args, emb[0], emb[1], emb[2], ta, tp, tn).item()
        nce = tr.info_nce(args, emb[3], emb[4], tau, B, mask).item()
        args.per_gpu_train_batch_size = B + 1                      # last partial batch: the mask is rebuilt (:92-93)
        rebuilt = tr.info_nce(args, emb[3], emb[4], tau, B, None).item()
        assert np.array_equal(mask.numpy(), lh_mask(B))
        c64, n64 = (x.item() for x in lh.loss_head(tau, lam, 1.0, emb.double(), ta, tp, tn))
        own = lh.loss_err([cl, nce], [c64, n64])                   # a pin at 1e-5 must itself resolve the value
        assert own < 1e-5 / G14_SPARE, f"{tag}: the reference's float32 value is {own:.2e} from float64"
        tags.append(tag)
        out[tag + ":emb"] = emb.numpy(); out[tag + ":time"] = torch.stack([ta, tp, tn]).numpy()
        out[tag + ":hyper"] = np.array([tau, lam], np.float64)
        out[tag + ":losses"] = np.array([cl, nce, rebuilt], np.float64)
        print(f"  {tag}: tau {tau} lam {lam}: CLtime {cl:.6f} info_nce {nce:.6f} (rebuilt mask {rebuilt:.6f})")
    emb, ta, tp, tn = lh.make_inputs("unit", 1, 7)
    try:
        tr.CLtime_loss(types.SimpleNamespace(temperature=0.07, lambda_decay=0.05, per_gpu_train_batch_size=1), emb[0], emb[1], emb[2], ta, tp, tn)
        raised = ""
    except Exception as e:                                         # the 0-d decay "matrix" after .squeeze()
        raised = f"{type(e).__name__}: {e}"
    print(f"  B = 1: CLtime_loss raises {raised!r}")
    _save("g14_loss_head_edges", tags=np.array(tags), b1_raises=np.array(bool(raised)), b1_message=np.array(raised), **out)


G14_SPARE = 4.0                     # the pin's own distance from float64: twice it (as much again on the other side) in half of 1e-5


def lh_mask(B):
    """``mask_correlated_samples`` as a plain statement: every pair but the diagonal and the two partner diagonals."""
    m = ~np.eye(2 * B, dtype=bool)
    i = np.arange(B)
    m[i, B + i] = False
    m[B + i, i] = False
    return m


def g8b_lr_schedule():
    """``adjust_learning_rate`` (train/train_retriever.py:120-130) sampled over warm-up and cosine epochs."""
    _import_utils_model()
    import train.train_retriever as tr
    rows = []
    for warm, epochs, ipe, base in ((0, 50, 150, 1e-5), (2, 10, 37, 3e-4), (1, 3, 5, 1.0)):
        args = types.SimpleNamespace(warmup_steps=warm, num_train_epochs=epochs)
        opt = types.SimpleNamespace(param_groups=[{"lr": None}])
        for ep in range(epochs):
            for i in sorted({0, 1, ipe // 2, ipe - 1}):
                tr.adjust_learning_rate(args, opt, ep, base, i, ipe)
                rows.append((warm, epochs, ipe, base, ep, i, opt.param_groups[0]["lr"]))
    _save("g8b_lr_schedule", rows=np.array(rows, np.float64))


def g9_query_times():
    """get_train_query_time.py (the training loop's ``resources/<ds>_train_query_time.pt``): the reference's own ``load_data`` /
    ``get_query_time`` run on the shipped event tables of all three datasets; committed: the event columns the functions
    read (u, i, ts, timestamp), the ego id of every training line and the resulting times (float32 after the scale)."""
    import importlib.util
    import pandas as pd
    spec = importlib.util.spec_from_file_location("ref_get_train_query_time", os.path.join(REF, "get_train_query_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                   # the __main__ block is guarded
    scales = {"UCI_13": 3600 * 24, "hepth": 3600 * 24 * 30, "dialog": 1}
    out = {}
    for ds, ts in (("UCI_13", "12"), ("hepth", "11"), ("dialog", "15")):
        ml = mod.load_data(ds, ts)
        with open(os.path.join("resources", ds, ts, "train.link_prediction")) as f:
            lines = [ln for ln in f.read().splitlines() if len(ln) > 0 and not ln.isspace()]
        egos = [int(ln.split('<|history|>')[1].split(' ')[1]) for ln in lines]
        times = [mod.get_query_time(ml, q, ts) / scales[ds] for q in egos]
        raw = pd.read_csv(os.path.join("resources", ds, ts, f"ml_{ds}.csv"))
        out[f"{ds}_u"] = raw["u"].to_numpy(np.int64); out[f"{ds}_i"] = raw["i"].to_numpy(np.int64)
        out[f"{ds}_ts"] = raw["ts"].to_numpy(np.float64); out[f"{ds}_snapshot"] = raw["timestamp"].to_numpy(np.int64)
        out[f"{ds}_egos"] = np.array(egos, np.int64)
        out[f"{ds}_times"] = torch.tensor(times, dtype=torch.float).numpy()
        out[f"{ds}_cfg"] = np.array([int(ts), scales[ds]], np.int64)
    _save("g9_query_times", **out)


# --------------------------------------------------------------------------- G10
def g10_trained(tag="small", weights=None, device_npz=None):
    """TRAINED weights (every other vector uses N(0, 0.02) + random affine).  The checkpoint comes from THIS build's
    own trainer on the real UCI_13/12 data (GPU box: ``python tools/g10_trained.py <tag> L H d epochs lr`` -> gpurun_out/g10/
    <tag>_weights.npz, the reference script's recipe for the full-size run); here the SAME tensors are loaded into the
    reference model on CPU and the hot path is run with the reference's own modules (as g4 does).
      tag == "small" (L2 H2 d128, 2.8 MB, ALL 28 tensors of the L2 model -- round 3's file had lost both c_attn.bias): weights +
        reference outputs are committed as tests/golden/g10_trained_small.npz.  With no ``weights`` argument the weights are
        read back from that committed file, so ``python oracle/gen_golden.py g10`` regenerates it bit for bit like every other
        group; pass gpurun_out/g10/small_weights.npz to commit a NEW checkpoint.  The same call writes G11
        (tests/golden/g11_stress_small.npz): the reference's outputs for ``gpt2_ref.stress_transform`` of those weights --
        trained-GPT-2 statistics (outlier LayerNorm gains, offset residual rows, massive-activation channels);
      any other tag (the full-size L4 H2 d512 checkpoint, 56 MB: not committed): the reference outputs are compared with the
      device outputs the GPU run dumped next to the weights and a report goes to profiles/r03_trained_parity_<tag>.json."""
    print(f"G10 trained weights [{tag}]")
    import json
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if weights is None and tag == "small":
        w = np.load(os.path.join(GOLD, "g10_trained_small.npz"))
        sd = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("w:")}
    else:
        weights = weights or os.path.join(here, "gpurun_out", "g10", f"{tag}_weights.npz")
        w = np.load(weights)
        sd = {k: torch.from_numpy(w[k]) for k in w.files}
    device_npz = device_npz or os.path.join(here, "gpurun_out", "g10", f"{tag}_device.npz")
    d = sd["transformer.wte.weight"].shape[1]
    V = sd["transformer.wte.weight"].shape[0]
    L = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.h."))
    H = 2
    n_pos = sd["transformer.wpe.weight"].shape[0]
    assert len(sd) == 12 * L + 4, f"{len(sd)} tensors for an L{L} model: expected {12 * L + 4} (wte, wpe, ln_f x2, 12 per block)"
    if "lm_head.weight" not in sd:
        sd["lm_head.weight"] = sd["transformer.wte.weight"]
    g6 = np.load(os.path.join(GOLD, "g6_uci_tokens.npz"))
    pad = int(g6["pad_id"])

    def seqs(flat, off):
        return [flat[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    pool, test = seqs(g6["pool_flat"], g6["pool_off"]), seqs(g6["test_flat"], g6["test_off"])
    NP = 256                                                         # pool rows used: the first 8 reference batches

    def batches(examples):          # dataloader/retriever.py:153-166 around the reference model (as g4)
        for s in range(0, len(examples), 32):
            ch = [torch.tensor(e, dtype=torch.long) for e in examples[s:s + 32]]
            yield torch.nn.utils.rnn.pad_sequence(ch, batch_first=True, padding_value=pad)

    def hot_path(state):
        m = _ref_model("rag", L, H, d, V, n_pos, state)
        with torch.no_grad():
            pe = torch.cat([torch.mean(m(input_ids=b)[1], dim=1) for b in batches(pool[:NP])], dim=0)
            qe = torch.cat([torch.mean(m(input_ids=b)[1], dim=1) for b in batches(test)], dim=0)
            qn = qe / qe.norm(dim=1, keepdim=True)                      # train_retriever.py:433-438
            pn = pe / pe.norm(dim=1, keepdim=True)
            S = ((torch.matmul(qn, pn.t()) + 1) / 2).numpy()
        return pe, qe, S, np.argsort(-S, axis=1, kind="stable")[:, :10].astype(np.int32)
    pe, qe, S, top10 = hot_path(sd)
    stats = {"max_abs_weight": float(max(v.abs().max() for v in sd.values())),
             "ln_gain_range": [float(min(v.min() for k, v in sd.items() if "ln_" in k and k.endswith("weight"))),
                               float(max(v.max() for k, v in sd.items() if "ln_" in k and k.endswith("weight")))],
             "query_emb_absmax": float(qe.abs().max())}
    if tag == "small":
        _save("g10_trained_small", n_layer=np.array(L), n_head=np.array(H), pool_rows=np.array(NP),
              pool_emb=pe.numpy(), query_emb=qe.numpy(), scores=S, top10_stable=top10,
              **{"w:" + k: v.numpy() for k, v in sd.items() if k != "lm_head.weight"})
        print("   ", stats)
        # ---- G11: the same checkpoint with trained-GPT-2 statistics (oracle/gpt2_ref.py:stress_transform), reference outputs only
        st = gpt2_ref.stress_transform(sd)
        pe2, qe2, S2, top2 = hot_path(st)
        ids0 = next(batches(test))
        with torch.no_grad():
            m2 = _ref_model("gpt2", L, H, d, V, n_pos, st, output_hidden_states=True)
            hs = m2(ids0)[2]
        ratio = [float((h.mean(-1).abs() / h.std(-1)).median()) for h in hs[:-1]]
        sig = np.array([float(st[k].double().abs().sum()) for k in sorted(st) if k != "lm_head.weight"])
        _save("g11_stress_small", n_layer=np.array(L), n_head=np.array(H), pool_rows=np.array(NP), pool_emb=pe2.numpy(),
              query_emb=qe2.numpy(), scores=S2, top10_stable=top2, weight_abs_sums=sig,
              residual_mean_over_std=np.array(ratio), residual_absmax=np.array([float(h.abs().max()) for h in hs[:-1]]))
        print("    G11 stress: residual |row mean| / std per layer", [round(r, 2) for r in ratio], "query emb absmax",
              float(qe2.abs().max()), "score range", float(S2.min()), float(S2.max()))
        return
    dv = np.load(device_npz)
    rep = {"checkpoint": f"tools/g10_trained.py {tag}: {L} layers, {H} heads, d {d}, vocab {V}; the reference recipe "
                         "(scripts/train_retriever/train_retriever_UCI_13.sh) on UCI_13/12 with this build's trainer", "weights": stats,
           "compared": f"{qe.shape[0]} test queries x first {NP} pool rows, reference modules on CPU vs the HIP path on MI355X"}
    for mode in ("split3", "f32"):
        q_d, p_d, S_d = dv[f"{mode}_query_emb"], dv[f"{mode}_pool_emb_head"][:NP], dv[f"{mode}_scores"][:, :NP]
        # device top-10 restricted to the first NP pool rows, canonical order, from the DEVICE scores
        top_d = np.argsort(-S_d.astype(np.float64), axis=1, kind="stable")[:, :10]
        same = top_d == top10
        gap = 0.0
        for r, c in zip(*np.nonzero(~same)):
            gap = max(gap, abs(float(S[r, top10[r, c]]) - float(S[r, top_d[r, c]])))

        def ew(got, ref):
            got, ref = got.astype(np.float64), ref.astype(np.float64)
            return float((np.abs(got - ref) / (1e-4 * np.abs(ref) + 1e-5 * np.abs(ref).max())).max())
        rep[mode] = {"query_emb_maxnorm_err": float(np.abs(q_d - qe.numpy()).max() / np.abs(qe.numpy()).max()),
                     "query_emb_elementwise_ratio": ew(q_d, qe.numpy()), "pool_emb_elementwise_ratio": ew(p_d, pe.numpy()),
                     "scores_max_abs_err": float(np.abs(S_d - S).max()), "top10_rows_identical": float(same.all(axis=1).mean()),
                     "max_reference_score_gap_at_mismatch": gap}
    out = os.path.join(here, "profiles", f"r03_trained_parity_{tag}.json")
    json.dump(rep, open(out, "w"), indent=1)
    print(json.dumps(rep, indent=1))


# --------------------------------------------------------------------------- G12
def _regenerated_dataset_cwd(pairs):
    """A scratch cwd holding ``resources/<ds>/<t>/*.link_prediction`` + ``vocabs/<ds>/<t>/vocab.json`` REGENERATED by the
    reference's own ``csv2resources.py`` (run unmodified as a child process, cwd-relative ``../all_data`` -> a symlink to the
    reference's ``all_data``) from ``all_data/<ds>/<t>/ml_<ds>.csv`` -- the reference ships no ``resources/`` for wikiv2 /
    reddit (SURVEY ground facts).  Row order inside one second depends on the installed pandas' ``sort_values``,
    so the ids committed by g12 ARE the fixture; the csv is not re-read on the GPU box."""
    import subprocess
    root = tempfile.mkdtemp(prefix="r4d_g12_")
    os.symlink(os.path.join(REF, "all_data"), os.path.join(root, "all_data"))
    work = os.path.join(root, "work")
    os.makedirs(os.path.join(work, "tokenizers"))
    for ds, ts in pairs:
        r = subprocess.run([sys.executable, os.path.join(REF, "csv2resources.py"), ds, str(ts)], cwd=work, capture_output=True, text=True,
                           env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
        if r.returncode != 0:
            # reddit/11: the reference's own script raises at csv2resources.py:186 (`int(NaN)`: a validation user without any
            # history row) AFTER writing the complete train file (10,527 lines, :117-164) and the first 1,285 val lines, and BEFORE
            # the test files and vocab.json (:211-231).  Nothing is patched: the train file and the val lines it did write are
            # used as they are, and the vocabulary of :211-231 ({str(id): rank among the sorted ids of u and i}) is written by
            # the harness from the same csv.
            assert ds == "reddit" and "cannot convert float NaN to integer" in r.stderr, r.stderr[-2000:]
            import json
            import pandas as pd
            data = pd.read_csv(os.path.join(REF, "all_data", ds, str(ts), f"ml_{ds}.csv"), index_col=0)
            ids = sorted(set(list(data["u"]) + list(data["i"])))
            with open(os.path.join(work, "vocabs", ds, str(ts), "vocab.json"), "w") as f:
                json.dump({str(i): ind for ind, i in enumerate(ids)}, f, indent=4)
    os.chdir(work)
    return work


def g12_real_wikiv2_reddit():
    """REAL-DATA fixtures for BASELINE configs 4 and 5.
    wikiv2/15 (config 4: L2 H6 d768, block 512): the reference tokenizer + dataset classes on the regenerated files -> ids of the
    8,556 pool histories, the 593 test and 868 val queries (two pool sequences exceed 512 tokens: the left-truncation case);
    the reference model (seeded weights loaded into it, as g4) over the WHOLE pool and all test queries -> first / last two pool
    batches, every pool norm, the float64 column sum, 64 full query rows + every query norm, the scores against the first 512
    pool rows, and the stable top-32 (index, score) of every query over the full pool (a full [593, 8556] score matrix would be
    20 MB; the top-32 lets the test price any mismatching rank in REFERENCE scores).
    reddit/11 (config 5 inputs: L2 H8 d512, generator tokenizer without [MASK]): ids of the 10,527 training lines (the
    generator's ``retrieval_sources``) and of the 1,285 validation queries the reference's script writes before it raises on
    this csv (``_regenerated_dataset_cwd``; the test files are never written) via ``TextIndexScoreDataset``'s own encode calls;
    ``fusion_mlp`` + the greedy loop on six REAL queries with seven real demonstrations each (``fmlp_reddit_real``, g7's recipe)."""
    print("G12 real wikiv2 / reddit")
    import time
    _regenerated_dataset_cwd([("wikiv2", 15), ("reddit", 11)])
    import dataloader.retriever as dr
    tok = _ref_tokenizer("wikiv2", 15)
    base = "resources/wikiv2/15/"
    args = types.SimpleNamespace()
    pool_ds = dr.LineByLineTextDatasetHistory(tok, args, base + "train.link_prediction", block_size=512)
    test_ds = dr.LineByLineTextDataset(tok, args, base + "test.link_prediction", block_size=512)
    val_ds = dr.LineByLineTextDataset(tok, args, base + "val.link_prediction", block_size=512)
    with open(base + "train.link_prediction") as f:
        raw_len = [len(ln.split("<|pre|>")[0].split()) for ln in f.read().splitlines() if ln.strip()]
    long_rows = [i for i, n in enumerate(raw_len) if n > 512]
    assert len(pool_ds.examples) == 8556 and len(test_ds.examples) == 593 and len(val_ds.examples) == 868 and len(tok) == 8814
    assert len(long_rows) >= 1 and all(len(pool_ds.examples[i]) == 512 for i in long_rows)
    pf, po = _ragged(pool_ds.examples); tf, to = _ragged(test_ds.examples); vf, vo = _ragged(val_ds.examples)
    names = ["<|endoftext|>", "<|history|>", "<|endofhistory|>", "<|pre|>", "<|endofpre|>", "<|time0|>", "<|time15|>", "[PAD]", "[MASK]"]
    with open(base + "train.link_prediction") as f:
        hist = [ln.split("<|pre|>")[0] for ln in f.read().splitlines() if ln.strip()]
    full = [tok(hist[i])["input_ids"] for i in long_rows]           # the same tokenizer WITHOUT max_length: what truncation cut from
    assert all(full[j][-512:] == pool_ds.examples[i] for j, i in enumerate(long_rows))
    lf, lo = _ragged(full)
    import json
    vocab = json.load(open("vocabs/wikiv2/15/vocab.json"))
    vk = np.asarray([int(k_) for k_, _v in sorted(vocab.items(), key=lambda kv: kv[1])], np.int64)
    assert sorted(vocab.values()) == list(range(len(vocab)))
    _save("g6_wikiv2_tokens", pool_flat=pf, pool_off=po, test_flat=tf, test_off=to, val_flat=vf, val_off=vo,
          vocab_keys=vk, truncated_full_flat=lf, truncated_full_off=lo,
          truncated_rows=np.asarray(long_rows, np.int64), truncated_raw_len=np.asarray([raw_len[i] for i in long_rows], np.int64),
          special_names=np.array(names), special_ids=np.array([tok.convert_tokens_to_ids(t_) for t_ in names]),
          len_tok=np.array(len(tok)), vocab_size=np.array(tok.vocab_size), pad_id=np.array(tok.pad_token_id))
    L, H, d, V = 2, 6, 768, len(tok)
    sd = gpt2_ref.make_state_dict(L, d, V, seed=2027, random_affine=True)
    m = _ref_model("rag", L, H, d, V, 1024, sd)

    def batches(examples):          # dataloader/retriever.py:153-166 around the reference model (as g4)
        for s_ in range(0, len(examples), 32):
            ch = [torch.tensor(e, dtype=torch.long) for e in examples[s_:s_ + 32]]
            yield torch.nn.utils.rnn.pad_sequence(ch, batch_first=True, padding_value=tok.pad_token_id)
    t0 = time.time()
    with torch.no_grad():
        pool = torch.cat([torch.mean(m(input_ids=b)[1], dim=1) for b in batches(pool_ds.examples)], dim=0)
        q = torch.cat([torch.mean(m(input_ids=b)[1], dim=1) for b in batches(test_ds.examples)], dim=0)
        qn = q / q.norm(dim=1, keepdim=True)                      # train_retriever.py:433-438
        pn = pool / pool.norm(dim=1, keepdim=True)
        S = ((torch.matmul(qn, pn.t()) + 1) / 2).numpy()
    print(f"    reference encode + score of 8,556 + 593 sequences: {time.time() - t0:.0f} s")
    order = np.argsort(-S, axis=1, kind="stable")[:, :32]
    lb = [i // 32 for i in long_rows]                               # the batches holding a truncated sequence
    _save("g12_wikiv2_retrieval", seed=np.array(2027), cfg=np.array([L, H, d, V]), pool_emb_head=pool[:64].numpy(),
          pool_emb_tail=pool[-(len(pool) - (len(pool) - 1) // 32 * 32 + 32):].numpy(),
          pool_emb_norms=pool.norm(dim=1).numpy(), pool_emb_colsum=pool.double().sum(0).numpy(),
          pool_emb_truncated_batches=np.concatenate([pool[b * 32:b * 32 + 32].numpy() for b in lb]),
          truncated_batches=np.asarray(lb, np.int64), query_emb_head=q[:64].numpy(), query_emb_norms=q.norm(dim=1).numpy(),
          scores_first512=S[:, :512].copy(), top32_idx=order.astype(np.int32), top32_scores=np.take_along_axis(S, order, axis=1),
          score_row_sums=S.astype(np.float64).sum(1))

    # ---- reddit / 11 (BASELINE config 5 inputs), generator flavour
    from models import GPT2Config
    import models.modeling_rag as mr
    from transformers import PreTrainedTokenizerFast
    from utils.tokenizer_generator import get_model_tokenizer as get_gen
    import dataloader.generator as dg
    um = _import_utils_model()
    a = types.SimpleNamespace(model_type="gpt2", config_name=None, model_name_or_path=None, cache_dir=None, n_head=2, n_layer=1,
                              n_embed=16, timestamp="11", dataset="reddit", device="cpu", node_feat_file=None)
    _, rtok, _, _ = get_gen(a, {"gpt2": (GPT2Config, mr.GPT2LMHeadModel, PreTrainedTokenizerFast)})
    if not hasattr(rtok, "batch_encode_plus"):
        type(rtok).batch_encode_plus = lambda self, lines, **kw: self(lines, **kw)
    assert len(rtok) == 11919
    rbase = "resources/reddit/11/"
    rng = np.random.default_rng(12)
    n_test = sum(1 for ln in open(rbase + "val.link_prediction") if ln.strip())   # the val lines the script wrote before it raised
    assert n_test == 1285 and sum(1 for ln in open(rbase + "train.link_prediction") if ln.strip()) == 10527
    idx_rows = [rng.permutation(10527)[:20].tolist() for _ in range(n_test)]     # a stand-in retrieval ranking (no retriever output is shipped)
    with open("g12_idx.txt", "w") as f:
        f.write("\n".join(" ".join(map(str, r)) for r in idx_rows) + "\n")
    with open("g12_score.txt", "w") as f:
        f.write("\n".join(" ".join("%.4f" % (1 - 0.01 * j) for j in range(20)) for _ in idx_rows) + "\n")
    ds = dg.TextIndexScoreDataset(rtok, types.SimpleNamespace(train_data_file=rbase + "train.link_prediction"),
                                  rbase + "val.link_prediction", "g12_idx.txt", "g12_score.txt", block_size=1024)
    assert len(ds.retrieval_sources) == 10527
    sf, so = _ragged(ds.retrieval_sources); qf, qo = _ragged(ds.text)
    rnames = ["<|endoftext|>", "<|history|>", "<|endofhistory|>", "<|pre|>", "<|endofpre|>", "<|time0|>", "<|time11|>", "[PAD]"]
    rvocab = json.load(open("vocabs/reddit/11/vocab.json"))
    rvk = np.asarray([int(k_) for k_, _v in sorted(rvocab.items(), key=lambda kv: kv[1])], np.int64)
    _save("g6_reddit_tokens", vocab_keys=rvk, source_flat=sf, source_off=so, val_flat=qf, val_off=qo, egos=np.asarray(ds.egolist, np.int64),
          special_names=np.array(rnames), special_ids=np.array([rtok.convert_tokens_to_ids(t_) for t_ in rnames]),
          len_tok=np.array(len(rtok)), vocab_size=np.array(rtok.vocab_size), pad_id=np.array(rtok.pad_token_id))
    out = {}
    lens = np.array([len(t_) for t_ in ds.text])
    pick = [int(i) for i in np.argsort(lens, kind="stable")[[len(lens) // 10, len(lens) // 4, len(lens) // 2, len(lens) // 2 + 1,
                                                              3 * len(lens) // 4, 9 * len(lens) // 10]]]
    # demonstrations short enough that query + 7 demos stay inside n_positions (utils/model.py pads demos to the longest of the 7)
    short = [i for i, s_ in enumerate(ds.retrieval_sources) if len(s_) <= 120]
    idxs = [[short[j] for j in rng.permutation(len(short))[:7]] for _ in pick]
    _run_fusion(out, um, "fmlp_reddit_real", 2, 8, 512, len(rtok), rtok.pad_token_id, rtok.convert_tokens_to_ids("<|endoftext|>"),
                ds.retrieval_sources, [ds.text[i] for i in pick], idxs, 1, 1, 7, 330)
    out["fmlp_reddit_real_query_rows"] = np.asarray(pick, np.int64)
    _save("g12_reddit_generator", **out)


# --------------------------------------------------------------------------- G13
def g13_h2_attention_stress():
    """Reference-held vectors with HARD statistics at the head dims ``csrc/attention_h2.hip`` serves (G11 is
    head_dim 64 and routed to the exact-f32 kernel then).  Seven cases (the last three for the key-split kernel of head_dim 32 / 64 / 96), each the reference model on the real UCI_13/12 ids (first 256
    pool histories = 8 reference batches, all 110 test queries), as g10 does:
      hd128_plain    the TRAINED G10 tensors loaded with n_head = 1 (one head of 128);
      hd128_stress   the same after ``gpt2_ref.stress_transform`` (G11's transform);
      hd128_peaked   the same after ``stress_transform`` and ``sharpen_attention(4)`` (every logit x 16);
      hd256_peaked   a seeded L2 H2 d512 model (-> head_dim 256; weights by ``make_state_dict``, not committed) after
                     ``stress_transform`` and ``sharpen_attention(6)`` (every logit x 36).
    Stored per case: embeddings, scores, stable top-10, three token rows of the ln_f hidden states of the first query batch (the
    mean-pool hides per-token error), the per-tensor weight checksum (sum of the fp32 BIT PATTERNS: exact, independent of
    summation order and thread count), and HOW peaked the reference's own softmax was (median /
    90th percentile of the row maximum of its attention probabilities per layer, from ``config.output_attentions``)."""
    print("G13 attention_h2 head dims under stress")
    gw = np.load(os.path.join(GOLD, "g10_trained_small.npz"))
    trained = {k[2:]: torch.from_numpy(gw[k]) for k in gw.files if k.startswith("w:")}
    trained["lm_head.weight"] = trained["transformer.wte.weight"]
    g6 = np.load(os.path.join(GOLD, "g6_uci_tokens.npz"))
    pad = int(g6["pad_id"])

    def seqs(flat, off):
        return [flat[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    pool, test = seqs(g6["pool_flat"], g6["pool_off"])[:256], seqs(g6["test_flat"], g6["test_off"])

    def batches(examples):          # dataloader/retriever.py:153-166 around the reference model (as g4)
        for s in range(0, len(examples), 32):
            ch = [torch.tensor(e, dtype=torch.long) for e in examples[s:s + 32]]
            yield torch.nn.utils.rnn.pad_sequence(ch, batch_first=True, padding_value=pad)
    seeded = gpt2_ref.make_state_dict(2, 512, 1801, seed=2031, random_affine=True)
    seeded96 = gpt2_ref.make_state_dict(2, 768, 1801, seed=2032, random_affine=True)
    cases = {"hd128_plain": (trained, 1), "hd128_stress": (gpt2_ref.stress_transform(trained), 1),
             "hd128_peaked": (gpt2_ref.sharpen_attention(gpt2_ref.stress_transform(trained), 4.0), 1),
             "hd256_peaked": (gpt2_ref.sharpen_attention(gpt2_ref.stress_transform(seeded), 6.0), 2),
             # (later in round 5: the key-split f16x2 kernel's head dims -- the trained tensors as 2 heads of 64 and 4 heads of 32, and a
             #  seeded L2 H8 d768 model = head_dim 96, the SimpleDyG UCI_13 shape -- appended: the earlier cases keep their values)
             "hd64_peaked": (gpt2_ref.sharpen_attention(gpt2_ref.stress_transform(trained), 4.0), 2),
             "hd32_peaked": (gpt2_ref.sharpen_attention(gpt2_ref.stress_transform(trained), 4.0), 4),
             "hd96_peaked": (gpt2_ref.sharpen_attention(gpt2_ref.stress_transform(seeded96), 6.0), 8)}
    out = {}
    for tag, (sd, H) in cases.items():
        V, d = sd["transformer.wte.weight"].shape
        n_pos = sd["transformer.wpe.weight"].shape[0]
        L = gpt2_ref.n_layers_of(sd)
        m = _ref_model("rag", L, H, d, V, n_pos, sd)
        with torch.no_grad():
            pe = torch.cat([torch.mean(m(input_ids=b)[1], dim=1) for b in batches(pool)], dim=0)
            hid0 = None
            qs = []
            for b in batches(test):
                h = m(input_ids=b)[1]
                if hid0 is None:
                    T0 = h.shape[1]
                    rows = [0, T0 // 2, T0 - 1]
                    hid0 = h[:, rows, :].numpy().copy()
                qs.append(torch.mean(h, dim=1))
            qe = torch.cat(qs, dim=0)
            qn = qe / qe.norm(dim=1, keepdim=True)                      # train_retriever.py:433-438
            pn = pe / pe.norm(dim=1, keepdim=True)
            S = ((torch.matmul(qn, pn.t()) + 1) / 2).numpy()
            ma = _ref_model("gpt2", L, H, d, V, n_pos, sd, output_attentions=True)
            att = ma(next(batches(test)))[-1]                             # tuple over layers of [B,H,T,T] probabilities
            peak = np.array([[float(a.max(-1).values.median()), float(a.max(-1).values.quantile(0.9))] for a in att])
        top10 = np.argsort(-S, axis=1, kind="stable")[:, :10].astype(np.int32)
        sig = gpt2_ref.weight_bit_checksums(sd)
        out.update({f"{tag}:cfg": np.array([L, H, d, V, n_pos]), f"{tag}:pool_emb": pe.numpy(), f"{tag}:query_emb": qe.numpy(),
                    f"{tag}:scores": S, f"{tag}:top10_stable": top10, f"{tag}:hidden_rows": hid0, f"{tag}:rows": np.array(rows),
                    f"{tag}:weight_checksums": sig, f"{tag}:attn_rowmax_median_p90": peak})
        print(f"    {tag}: L{L} H{H} d{d} -> head_dim {d // H}; attention row-max median / p90 per layer {peak.round(3).tolist()}; "
              f"query emb absmax {float(qe.abs().max()):.3f}; score range {float(S.min()):.4f} .. {float(S.max()):.4f}")
    _save("g13_h2_attention_stress", seed_hd256=np.array(2031), seed_hd96=np.array(2032), pool_rows=np.array(256), **out)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "g10":                   # g10 <tag> [weights.npz] [device.npz]
        torch.set_num_threads(os.cpu_count() or 1)
        _install_stubs()
        _scratch_cwd()
        g10_trained(*sys.argv[2:5])
        return
    groups = {"g1": g1_tiny_forward, "g2": g2_ops, "g3": g3_config_shapes, "g4": g4_g6_uci_retrieval, "g5": g5_jaccard,
              "g6b": g6_more_tokenizers, "g7": g7_generator, "g8": g8_training_step, "g8b": g8b_lr_schedule, "g9": g9_query_times,
              "g10": g10_trained, "g12": g12_real_wikiv2_reddit, "g13": g13_h2_attention_stress, "g14": g14_loss_head_edges}
    want = [a for a in sys.argv[1:] if a in groups] or list(groups)
    torch.set_num_threads(os.cpu_count() or 1)
    _install_stubs()
    _scratch_cwd()
    for k in want:
        groups[k]()


if __name__ == "__main__":
    main()

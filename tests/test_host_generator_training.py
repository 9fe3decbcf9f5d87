"""Host-side tests of RAG generator training (no GPU): the trainable set and AdamW groups with and without --freeze, the augmented
ids / labels, the cosine schedule against the reference's formula, the bag weights against a dense A_norm, and the refusals."""
import argparse
import math

import numpy as np
import pytest
import torch


def _model(untie):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=50, n_positions=64, n_ctx=64, n_embd=64, n_layer=2, n_head=2))
    m.get_gnn(64, 32, 64, 1, 0.2)
    if untie:
        m.lm_head.weight = torch.nn.Parameter(m.transformer.wte.weight.detach().clone())
    return m


def test_trainable_set_and_adamw_groups():
    from rag4dyg_amd.generator_training import trainable_names
    frozen = trainable_names(_model(True), freeze=True)
    assert frozen == ["lm_head.weight", "gnn_fusion.convs.0.bias", "gnn_fusion.convs.0.lin.weight"]
    full = trainable_names(_model(False), freeze=False)
    assert "lm_head.weight" not in full and "transformer.wte.weight" in full and full[-2:] == frozen[1:]
    assert len(full) == 4 + 12 * 2 + 2
    no_decay = ("bias", "LayerNorm.weight")                            # utils/model.py:80-88
    decayed = [n for n in frozen if not any(nd in n for nd in no_decay)]
    assert decayed == ["lm_head.weight", "gnn_fusion.convs.0.lin.weight"]


def test_augmented_ids_are_splice_labels_and_scatter_ids():
    from rag4dyg_amd.generator_training import augmented_ids
    tok = torch.tensor([[5, 6, 7, 8], [1, 2, 3, 4]])
    aug = augmented_ids(tok, 1)
    want = torch.cat([tok[:, :2], torch.full((2, 1), -100), tok[:, 2:]], dim=1)       # train_generator.py:92-95
    assert torch.equal(aug, want) and aug.dtype == torch.int64


def test_cosine_schedule_matches_the_reference_formula():
    from rag4dyg_amd import training

    class Opt:
        lr = None
    args = argparse.Namespace(warmup_steps=2, num_train_epochs=7)
    for epoch in range(7):
        for i in range(5):
            training.adjust_learning_rate(args, Opt, epoch, 1e-3, i, 5)
            T = epoch * 5 + i                                         # train/train_generator.py:33-44
            if epoch < 2:
                want = 1e-3 * T / (2 * 5)
            else:
                want = 0.5 * 1e-3 * (1 + math.cos((T - 10) / ((7 - 2) * 5) * math.pi))
            assert abs(Opt.lr - want) < 1e-15


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_bag_weights_equal_the_mean_over_nodes_of_dense_a_norm(seed):
    from oracle import generator_ref
    from rag4dyg_amd.generator_training import bag_weights
    g = np.random.default_rng(seed)
    src = [g.integers(0, 30, int(g.integers(3, 12))).tolist() for _ in range(20)]
    idx = g.choice(20, 7, replace=False).tolist()
    nodes, c = bag_weights(src, idx)
    order, edges = generator_ref.star_union_graph(src, idx)
    assert nodes.tolist() == order
    a = generator_ref.gcn_norm_dense(len(order), edges).double()
    assert np.allclose(c, a.mean(dim=0).numpy(), rtol=1e-6, atol=1e-7)


def test_prepared_bags_concatenate_in_batch_order():
    from rag4dyg_amd.generator_training import PreparedBags
    src = [[1, 2, 3, 4], [5, 6, 7], [8, 9, 10, 11, 12]]
    pb = PreparedBags([[0], [1, 2], [2]], src, 7)
    nodes, c, offs, row_of = pb.batch([2, 0], "cpu")
    assert offs.tolist() == [0, len(pb.items[2][0]), len(pb.items[2][0]) + len(pb.items[0][0])]
    assert nodes.tolist() == pb.items[2][0].tolist() + pb.items[0][0].tolist()
    assert row_of.tolist() == [0] * len(pb.items[2][0]) + [1] * len(pb.items[0][0])


@pytest.mark.parametrize("change,exc", [({"fp16": True}, NotImplementedError), ({"should_continue": True}, NotImplementedError),
                                        ({"fusion": "mlp"}, NotImplementedError), ({"gnn_layers": 2}, NotImplementedError),
                                        ({"m": 3}, ValueError)])
def test_unsupported_configurations_are_refused(change, exc):
    from rag4dyg_amd.generator_training import check_supported
    base = dict(fp16=False, should_continue=False, fusion="graphpooling", gnn_layers=1, m=1)
    check_supported(argparse.Namespace(**base))
    with pytest.raises(exc):
        check_supported(argparse.Namespace(**{**base, **change}))

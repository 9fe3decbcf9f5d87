"""The backward's guard over the training modes (csrc/train.hip: the ``guarded`` column of kTrainModes): on the workspace of the
most recent forward it refuses every switch that moved since -- by name, on the host, before any launch -- except the LM head's,
which no saved block depends on.  One tiny shape (L1 H1 d64, one sequence of 5 tokens, no dropout), one case per switch."""
import pytest
import torch

import _train_modes
from test_gpu_train_attention_recompute import _bits_equal, _enc_model

pytestmark = pytest.mark.gpu

restore = _train_modes.switches_restored()

# (switch, the name in the refusal, the forward's words, the one word that moves that switch to another state the trainers accept)
GUARDED = [("attention", "train-attention mode", {}, {"attention": "recompute"}),
           ("activations", "train-activations mode", {}, {"activations": "recompute"}),
           ("bf16", "train-bf16", {}, {"precision": "bf16"}),
           ("attention_bf16", "train-attention-bf16", {}, {"precision": "fp32+attn"}),
           ("act_bf16", "train-act-bf16", {"precision": "bf16"}, {"act_store": "bf16"}),
           ("attention_fused", "train-attention-fused", {"precision": "fp32+attn", "attention_kernel": "fused"}, {"attention_kernel": "products"})]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _forward(dev, words):
    from rag4dyg_amd import training
    m, _sd = _enc_model(dev, 1, 1, 64)
    tr = training.EncoderTrainer(m, dropout=(0.0, 0.0, 0.0), seed=5, **words)
    ids = torch.randint(0, 95, (1, 5), generator=torch.Generator().manual_seed(2)).to(dev)
    tr.forward([ids])
    return tr, torch.randn(1, 64, generator=torch.Generator().manual_seed(3)).to(dev)


@pytest.mark.parametrize("switch,name,words,flip", GUARDED, ids=[g[0] for g in GUARDED])
def test_backward_refuses_a_guarded_switch_that_moved_and_runs_once_it_is_back(dev, switch, name, words, flip):
    from rag4dyg_amd import _lib, training
    clean, demb = _forward(dev, words)
    want = {n: g.clone() for n, g in clean.backward(demb).items()}
    tr, _ = _forward(dev, words)
    was = training.library_modes()
    (key, word), = flip.items()
    first = getattr(tr, key)
    setattr(tr, key, word)                                                     # the trainer selects the other state before its backward
    with pytest.raises(_lib.R4DError, match=f"{name} {was[switch]}, the current value is {1 - was[switch]}"):
        tr.backward(demb)
    moved = training.library_modes()
    assert moved[switch] == 1 - was[switch] and {s: v for s, v in moved.items() if s != switch} == {s: v for s, v in was.items() if s != switch}
    setattr(tr, key, first)
    got = tr.backward(demb)                                                    # the refusal launched nothing: the saved blocks still give the gradients
    assert training.library_modes() == was
    for n in want:
        assert _bits_equal(want[n], got[n]), n


def test_backward_does_not_mind_the_head_switch(dev):
    from rag4dyg_amd import _lib, training
    lib = _lib.load()
    clean, demb = _forward(dev, {})
    want = {n: g.clone() for n, g in clean.backward(demb).items()}
    tr, _ = _forward(dev, {})
    head_was = lib.r4d_get_train_head_bf16()
    lib.r4d_set_train_head_bf16(1 - head_was)                                  # (an EncoderTrainer without a head leaves it where it is)
    got = tr.backward(demb)
    assert training.library_modes()["head_bf16"] == 1 - head_was
    for n in want:
        assert _bits_equal(want[n], got[n]), n

"""The DEVICE's statement of the hypothesis rule (csrc/beam.hip: beam_advance_kernel) on planted steps with bit-equal scores, which
the fixture's wide margins never reach: two eos candidates of one step with the same score fill the list in flat-index order, and
when a better hypothesis arrives at the next step the EARLIEST of the two equal lowest leaves (tests/_beam_ref.Hyps, ``gpt2.BeamHyps``
and the reference's ``sorted([(s, idx)])`` say the same).

The logits of a step are ``last . wte^T`` and ``last`` is caller state, so a step is planted by writing ``dec.last`` before it: the
least-norm solution of ``wte . last = target`` for a tiny model whose head rows 5 and 17 are one and the same row -- whatever
``last`` holds, the two ids get the same logit bit for bit (asserted on the step's own logits)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import _beam_ref as br

pytestmark = pytest.mark.gpu

A, B, E3 = 5, 17, 29                 # the two ids with one row, a third eos
C1, C2, C3 = 8, 11, 20               # plain ids
T, LP, MAX_GEN = 3, 3.0, 10


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def planted(wte64, **logit):
    """``last`` [d] with wte . last = the target row: 0 everywhere but the named ids."""
    t = np.zeros(wte64.shape[0])
    for k, v in logit.items():
        t[int(k[1:])] = v
    assert t[A] == t[B]
    return t, torch.from_numpy(np.linalg.lstsq(wte64, t, rcond=None)[0].astype(np.float32))


@pytest.mark.parametrize("graph", [False, True], ids=["host loop", "graph"])
def test_equal_scores_fill_in_flat_order_and_the_earliest_of_two_equal_lowest_leaves(dev, graph):
    from rag4dyg_amd.gpt2 import BeamDecoder, GPT2Config, GPT2LMHeadModel
    sd = br.weights_from(load_golden(br.FIXTURE))
    sd["transformer.wte.weight"][B] = sd["transformer.wte.weight"][A]           # (tied: the head's rows too)
    m = GPT2LMHeadModel(GPT2Config(vocab_size=br.VOCAB, n_positions=br.N_POSITIONS, n_ctx=br.N_POSITIONS, n_embd=br.N_EMBD, n_layer=br.N_LAYER,
                                   n_head=br.N_HEAD))
    m.load_state_dict(sd, strict=False)
    m = m.to(dev).eval()
    tr = m.transformer
    wte64 = sd["transformer.wte.weight"].double().numpy()
    prompt = torch.tensor([[1, 2, 3]], device=dev)
    n = 2
    dec = BeamDecoder(tr, 1, n, 128)
    dec.use_graph = graph
    try:
        tr.prefill_last(dec.cache, [T] * n, input_ids=prompt.repeat_interleave(n, 0))
        # step 1: the two equal eos ids lead, then two plain ids; the third eos is far below
        kw1 = {f"i{A}": 5.0, f"i{B}": 5.0, f"i{C1}": 4.0, f"i{C2}": 3.5, f"i{E3}": -5.0}
        t1, last1 = planted(wte64, **kw1)
        dec.begin_beams(last1.to(dev).expand(n, -1), T, MAX_GEN, [A, B, E3], length_penalty=LP)
        dec._steps(1)
        torch.cuda.synchronize()
        lg = dec.logits.cpu()
        assert lg[0, A].view(torch.int32) == lg[0, B].view(torch.int32) and abs(float(lg[0, C1]) - 4.0) < 1e-3
        assert dec.hyp_count.tolist() == [2] and dec.hyp_added.tolist() == [2] and dec.done.tolist() == [0] and dec.status.tolist() == [0]
        assert dec.hyp_seq.cpu()[0].tolist() == [0, 1] and dec.hyp_len.cpu()[0].tolist() == [0, 0]
        hs = dec.hyp_score.cpu()[0]
        assert hs[0].view(torch.int64) == hs[1].view(torch.int64)               # one score, twice
        assert float(dec.hyp_worst.cpu()[0]) == float(hs[0])
        assert dec.next.tolist() == [C1, C2] and dec.beam_idx.tolist() == [0, 0] and dec.gen_len.tolist() == [1, 1]
        s1 = br.row_scores(t1, 0.0)
        ref = br.Hyps(n, T + MAX_GEN, LP)
        ref.add([1, 2, 3], s1[A])
        ref.add([1, 2, 3], s1[B])
        assert abs(float(hs[0]) - ref.worst) < 1e-5
        # step 2: the third eos leads beam 0 and beats the two that wait; beam 1 offers no eos
        t2, last2 = planted(wte64, **{f"i{A}": -5.0, f"i{B}": -5.0, f"i{E3}": 6.0, f"i{C2}": 4.0, f"i{C3}": 3.75})
        _, last2b = planted(wte64, **{f"i{A}": -5.0, f"i{B}": -5.0, f"i{E3}": -5.0, f"i{C1}": 1.0, f"i{C3}": 0.5})
        dec.last.copy_(torch.stack([last2, last2b]).to(dev))
        dec._steps(1)
        torch.cuda.synchronize()
        better = (s1[C1] + br.row_scores(t2, 0.0)[E3]) / (T + 1) ** LP
        assert better > ref.worst + 1e-3                                        # the scenario: a third, better hypothesis
        ref.add([1, 2, 3, C1], s1[C1] + br.row_scores(t2, 0.0)[E3])
        assert [ids for _, ids in ref.beams] == [[1, 2, 3], [1, 2, 3, C1]] and ref.displaced == 1
        # the device: the slot of the EARLIEST arrival (seq 0) holds the newcomer, the other equal one stays
        assert dec.hyp_count.tolist() == [2] and dec.hyp_added.tolist() == [3] and dec.done.tolist() == [0]
        assert dec.hyp_seq.cpu()[0].tolist() == [2, 1] and dec.hyp_len.cpu()[0].tolist() == [1, 0]
        assert dec.hyp_ids.cpu()[0, 0, 0].item() == C1
        hs2 = dec.hyp_score.cpu()[0]
        assert hs2[1].view(torch.int64) == hs[1].view(torch.int64) and abs(float(hs2[0]) - better) < 1e-5
        assert float(dec.hyp_worst.cpu()[0]) == float(hs2[1]) and abs(float(hs2[1]) - ref.worst) < 1e-5
        assert dec.next.tolist() == [C2, C3] and dec.beam_idx.tolist() == [0, 0] and dec.gen_len.tolist() == [2, 2]
        assert dec.out.cpu()[:, :2].tolist() == [[C1, C2], [C1, C3]]
    finally:
        dec.close()

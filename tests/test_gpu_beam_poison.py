"""The beam entries never read memory they have not written (include/r4d.h, "What a buffer may hold on entry"): the outputs and the
candidate lists of ``r4d_beam_select_f32``, and the beam decoder's cache, workspace, logits, candidate lists, reorder arguments and
hypothesis buffers -- all ``torch.empty`` on the Python side -- filled with each pattern of tests/_poison.py, against a run on
zeroed memory, bit for bit.  None of these buffers forms an address, a loop bound or a length before the step has written it
(hypothesis slots are read up to ``hyp_count`` only, which is caller state and starts at 0), so every pattern may go everywhere."""
import json

import numpy as np
import pytest
import torch

from _poison import PATTERNS, ZERO, poison, poisoned_allocations
from conftest import load_golden

import _beam_ref as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _assert_same_runs(run):
    base = run(ZERO)
    for pattern in PATTERNS[1:]:
        got = run(pattern)
        assert len(got) == len(base)
        for k, (a, b) in enumerate(zip(base, got)):
            assert set(a) == set(b)
            for n in a:
                assert a[n].shape == b[n].shape and torch.equal(_bits(a[n]), _bits(b[n])), (pattern, k, n)


def test_beam_select_does_not_read_its_outputs_or_its_candidate_lists(dev):
    from rag4dyg_amd import ops
    cases = [(3, 2, 300), (1, 16, 16385), (2, 3, 3)]

    def run(pattern):
        out = []
        for B0, n, V in cases:
            rng = np.random.default_rng(V)
            x = torch.from_numpy((rng.standard_normal((B0 * n, V)) * 4).astype(np.float32)).to(dev)
            bs = torch.from_numpy((-rng.random(B0 * n)).astype(np.float32)).to(dev)
            with poisoned_allocations(pattern):
                s, i, cs, ci = ops.beam_select(x, bs, n, want_rows=True)
            out.append(dict(s=s.clone(), i=i.clone(), cs=cs.clone(), ci=ci.clone()))
        return out
    _assert_same_runs(run)


@pytest.mark.parametrize("graph", [False, True], ids=["host loop", "graph"])
def test_beam_loop_does_not_read_unwritten_memory(dev, graph):
    from rag4dyg_amd import ops
    from rag4dyg_amd.gpt2 import BeamDecoder, GPT2Config, GPT2LMHeadModel
    g = load_golden(br.FIXTURE)
    m = GPT2LMHeadModel(GPT2Config(vocab_size=br.VOCAB, n_positions=br.N_POSITIONS, n_ctx=br.N_POSITIONS, n_embd=br.N_EMBD, n_layer=br.N_LAYER,
                                   n_head=br.N_HEAD))
    m.load_state_dict(br.weights_from(g), strict=False)
    m = m.to(dev).eval()
    tr = m.transformer
    name = "n4_penalty_13"
    prompts, kw, want = torch.from_numpy(g[f"{name}/prompts"]).to(dev), json.loads(str(g[f"{name}/args"])), g[f"{name}/ids"]
    B0, T = prompts.shape
    n = kw["num_beams"]

    def run(pattern):
        ops._WS.clear()
        with poisoned_allocations(pattern):
            dec = BeamDecoder(tr, B0, n, 128)
        dec.use_graph = graph
        tr.__dict__.setdefault("_beam_decoders", {}).clear()
        tr.__dict__["_beam_decoders"][((B0, n), 128, 0)] = dec                 # generate finds this decoder
        out = []
        try:
            for _ in range(2):
                for b in (dec.cache, dec.ws, dec.logits, dec.cand_scores, dec.cand_ids, dec.beam_idx, dec.lo, dec.hi, dec.group_active,
                          dec.hyp_score, dec.hyp_len, dec.hyp_seq, dec.hyp_ids):
                    poison(b, pattern)
                with poisoned_allocations(pattern):
                    ids = m.generate(input_ids=prompts, do_sample=False, **kw)
                assert np.array_equal(ids.cpu().numpy(), want)
                out.append(dict(ids=ids.clone(), scores=dec.beam_scores.clone(), count=dec.hyp_count.clone(), worst=dec.hyp_worst.clone(),
                                seen=dec.seen.clone()))
            assert dec.graph_builds == (1 if graph else 0)
        finally:
            tr.__dict__["_beam_decoders"].clear()
            dec.close()
        return out
    _assert_same_runs(run)

"""``generate(num_beams > 1)`` on the device against the reference's own output ids (tests/golden/g16_beam_search.npz, written by
tools/gen_beam_fixture.py) and against the float64 restatement tests/_beam_ref.py driven by this project's own uncached forward.

The fixture's decisions all have a margin of 1e-3 in log-probability (asserted when it is written and in tests/test_host_beam.py),
some hundred times fp32's error on such scores: the ids must be the reference's exactly."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

import _beam_ref as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    return load_golden(br.FIXTURE)


def model_from(sd, dev, rag, n_layer, n_head, d, V, n_positions):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel, GPT2LMHeadModelRAG
    cls = GPT2LMHeadModelRAG if rag else GPT2LMHeadModel
    m = cls(GPT2Config(vocab_size=V, n_positions=n_positions, n_ctx=n_positions, n_embd=d, n_layer=n_layer, n_head=n_head))
    m.load_state_dict(sd, strict=False)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def models(dev, fixture):
    sd = br.weights_from(fixture)
    return {rag: model_from(sd, dev, rag, br.N_LAYER, br.N_HEAD, br.N_EMBD, br.VOCAB, br.N_POSITIONS) for rag in (False, True)}


def case(fixture, name):
    return torch.from_numpy(fixture[f"{name}/prompts"]), json.loads(str(fixture[f"{name}/args"])), fixture[f"{name}/ids"]


@pytest.mark.parametrize("rag", [False, True])
@pytest.mark.parametrize("name", list(br.CASES))
def test_every_fixture_case_gives_the_reference_ids(dev, fixture, models, name, rag):
    prompts, kw, want = case(fixture, name)
    got = models[rag].generate(input_ids=prompts.to(dev), do_sample=False, **kw)
    assert got.dtype == torch.long and got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), want), (name, got.cpu().numpy(), want)


@pytest.mark.parametrize("name", ["n2_one_eos", "n4_penalty_13", "n16_single_prompt"])
def test_graph_and_kernel_by_kernel_steps_and_a_second_call_give_the_same_ids(dev, fixture, models, name):
    prompts, kw, want = case(fixture, name)
    m = models[False]
    dec = m.transformer.beam_decoder(prompts.shape[0], kw["num_beams"], kw["max_length"])
    was = dec.use_graph
    try:
        for use_graph in (True, False, True):                                  # (the third call: hypotheses of the second are stale state)
            dec.use_graph = use_graph
            got = m.generate(input_ids=prompts.to(dev), do_sample=False, **kw)
            assert m.transformer.beam_decoder(prompts.shape[0], kw["num_beams"], kw["max_length"]) is dec
            assert np.array_equal(got.cpu().numpy(), want), (name, use_graph)
        assert dec.graph_builds >= 1
    finally:
        dec.use_graph = was


def test_another_call_with_other_arguments_reuses_the_graph(dev, fixture, models):
    """max_gen, the eos ids, both penalties and the prompt length are device words: one captured graph serves every call."""
    m = models[False]
    p1, kw1, want1 = case(fixture, "n2_one_eos")
    dec = m.transformer.beam_decoder(3, 2, 14)
    m.generate(input_ids=p1.to(dev), do_sample=False, **kw1)
    builds = dec.graph_builds
    kw2 = dict(kw1, max_length=11, eos_token_ids=[17, 29], length_penalty=0.6, repetition_penalty=1.3)
    p2 = p1[:, :4].contiguous()
    got2 = m.generate(input_ids=p2.to(dev), do_sample=False, **kw2)
    assert dec.graph_builds == builds and m.transformer.beam_decoder(3, 2, 11) is dec
    ref = br.beam_search(br.logits_fn(br.weights_from(fixture)), p2.tolist(), 2, 11, [17, 29], 0.6, 1.3, None, 1)
    assert ref["margin"] >= br.MARGIN                                           # (4.1e-3, looked up on the CPU)
    assert np.array_equal(got2.cpu().numpy(), ref["ids"])
    got1 = m.generate(input_ids=p1.to(dev), do_sample=False, **kw1)
    assert np.array_equal(got1.cpu().numpy(), want1)


def test_a_batch_of_three_equals_the_three_prompts_alone(dev, fixture, models):
    prompts, kw, want = case(fixture, "n2_one_eos")
    kw = dict(kw, pad_token_id=0)
    m = models[True]
    together = m.generate(input_ids=prompts.to(dev), do_sample=False, **kw).cpu()
    assert together.shape[1] < kw["max_length"] or bool((together == 0).any())     # the case pads: the rows differ in length
    for b in range(prompts.shape[0]):
        hyp = m.generate(input_ids=prompts[b:b + 1].to(dev), do_sample=False, **kw).cpu()[0].tolist()   # alone: neither closed nor padded
        row = together[b].tolist()
        tail = row[len(hyp):]
        assert row[:len(hyp)] == hyp, b
        assert tail == ([kw["eos_token_ids"][0]] + [0] * (len(tail) - 1) if tail else []), (b, tail)


def test_inputs_embeds_of_the_prompts_own_rows_equal_input_ids(dev, fixture, models):
    for name in ("n3_three_eos_lp06", "n4_penalty_13"):
        prompts, kw, want = case(fixture, name)
        m = models[True]
        emb = m.transformer.wte.weight.detach()[prompts.to(dev)]
        both = m.generate(input_ids=prompts.to(dev), inputs_embeds=emb, do_sample=False, **kw)
        assert np.array_equal(both.cpu().numpy(), want), name
        if kw.get("repetition_penalty", 1.0) == 1.0:
            only = m.generate(inputs_embeds=emb, do_sample=False, **kw)      # no ids for the prompt: the generated columns
            assert np.array_equal(only.cpu().numpy(), want[:, prompts.shape[1]:]), name


def test_the_prefilled_cache_rows_of_a_group_hold_identical_bits(dev, fixture, models):
    """The premise of reordering positions [T, cached) only: the n rows of a group are prefilled from one prompt."""
    for name in ("n4_lp2_return_all", "n16_single_prompt", "n2_one_token"):
        prompts, kw, _ = case(fixture, name)
        B0, T = prompts.shape
        n = kw["num_beams"]
        tr = models[False].transformer
        dec = tr.beam_decoder(B0, n, kw["max_length"])
        last = tr.prefill_last(dec.cache, [T] * (B0 * n), input_ids=prompts.to(dev).repeat_interleave(n, 0))
        torch.cuda.synchronize()
        rows = dec.cache[:, :, :T].view(torch.int32).view(br.N_LAYER, B0, n, T, -1)
        assert torch.equal(rows, rows[:, :, :1].expand_as(rows)), name
        lastv = last.view(torch.int32).view(B0, n, -1)
        assert torch.equal(lastv, lastv[:, :1].expand_as(lastv)), name


# ------------------------------------------------------------------------------------------------ beyond the fixture's shape
def test_the_restatement_on_the_projects_own_forward_at_another_shape(dev):
    """d 256, 4 heads, V 1000, T 5, max_length 24, n 4: ``_beam_ref.beam_search`` walks with the logits of this project's own
    uncached full forward at every step; the device search must give its ids wherever the restated margin is at least 1e-3."""
    I = br.INDEPENDENT
    sd = br.independent_weights()
    m = model_from(sd, dev, False, I["n_layer"], I["n_head"], I["d"], I["V"], I["n_positions"])

    def step(rows):
        with torch.no_grad():
            return m(torch.tensor(rows, dtype=torch.long, device=dev))[0][:, -1].double().cpu().numpy()
    skipped = 0
    for seed in I["seeds"]:
        prompts = br.independent_prompts(seed)
        kw = dict(num_beams=I["n"], max_length=I["max_length"], eos_token_ids=I["eos"], length_penalty=I["length_penalty"],
                  num_return_sequences=2)
        ref = br.beam_search(step, prompts, I["n"], I["max_length"], I["eos"], I["length_penalty"], 1.0, None, 2)
        if ref["margin"] < br.MARGIN:
            skipped += 1
            continue
        got = m.generate(input_ids=torch.tensor(prompts, device=dev), do_sample=False, **kw)
        assert np.array_equal(got.cpu().numpy(), ref["ids"]), (seed, ref["margin"])
    assert skipped * 10 <= len(I["seeds"]), skipped

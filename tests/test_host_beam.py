"""Beam search without a GPU: the ABI surface, the float64 restatement (tests/_beam_ref.py) against the ids that the reference's
own ``generate(num_beams > 1)`` gave (tests/golden/g16_beam_search.npz), the hypothesis rule and the last step of the host side
(``gpt2.BeamHyps``, ``gpt2.beam_finalize``) against the same restatement, and ``generate``'s new argument checks."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

import _beam_ref as br

REF = "/root/reference"
has_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
NEW_SYMBOLS = ("r4d_beam_select_f32", "r4d_kv_cache_reorder_f32", "r4d_gpt2_beam_workspace_bytes", "r4d_gpt2_beam_step_f32",
               "r4d_gpt2_beam_graph_create")


def test_beam_symbols_are_declared_bound_and_exported():
    import ctypes
    from rag4dyg_amd import _lib, ops
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    declared = set(re.findall(r"\b(r4d_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert "#define R4D_BEAM_MAX 16" in hdr and ops.BEAM_MAX == 16
    # the binding's struct is the header's, field by field
    body = hdr[hdr.index("typedef struct r4d_beam_state {"):hdr.index("} r4d_beam_state;")]
    assert re.findall(r"\b(\w+_d|out_cap|n_beams);", body) == [n for n, _ in _lib.BeamStateC._fields_]
    assert [n for n, _ in _lib.BeamStateC._fields_][:len(_lib.GreedyStateC._fields_)] == [n for n, _ in _lib.GreedyStateC._fields_]
    cfg = _lib.GPT2ConfigC(2, 2, 256, 1801, 512, 1e-5)
    assert lib.r4d_gpt2_beam_workspace_bytes(ctypes.byref(cfg), 3, 4) == lib.r4d_gpt2_greedy_workspace_bytes(ctypes.byref(cfg), 12) > 0
    assert lib.r4d_gpt2_beam_workspace_bytes(ctypes.byref(cfg), 3, 17) == 0 == lib.r4d_gpt2_beam_workspace_bytes(ctypes.byref(cfg), 3, 1)
    classes = [lib.r4d_profile_class_name(c).decode() for c in range(lib.r4d_profile_num_classes())]
    assert {"beam_rows", "beam_advance", "kv_reorder"} <= set(classes)


def test_both_head_models_have_the_beam_decoder():
    from rag4dyg_amd.gpt2 import BeamDecoder, GPT2Model, GreedyDecoder
    assert issubclass(BeamDecoder, GreedyDecoder) and hasattr(GPT2Model, "beam_decoder")


# ------------------------------------------------------------------------------------------------ the restatement and the fixture
def run_case(step, prompts, kw):
    return br.beam_search(step, prompts, kw["num_beams"], kw["max_length"], kw.get("eos_token_ids"), kw.get("length_penalty", 1.0),
                          kw.get("repetition_penalty", 1.0), kw.get("pad_token_id"), kw.get("num_return_sequences", 1))


def test_restatement_gives_the_reference_ids_of_the_fixture_with_wide_margins():
    g = load_golden(br.FIXTURE)
    sd, made = br.weights_from(g), br.make_weights()
    assert sorted(sd) == sorted(made) and all(torch.equal(sd[k], made[k]) for k in sd)
    step = br.logits_fn(sd)
    total = dict(done_early=0, displaced=0, pads=0, unfinished=0)
    for name, case in br.CASES.items():
        prompts, kw = br.case_inputs(case)
        assert np.array_equal(g[f"{name}/prompts"], np.asarray(prompts)) and json.loads(str(g[f"{name}/args"])) == kw
        res = run_case(step, prompts, kw)
        assert np.array_equal(res["ids"], g[f"{name}/ids"]), name
        assert res["margin"] >= br.MARGIN, (name, res["margin"])
        for k in total:
            total[k] += int(res["stats"][k])
    assert all(v > 0 for v in total.values()), total          # every branch of the rule is taken somewhere in the fixture


def test_fixture_covers_the_case_list():
    kws = [c[3] for c in br.CASES.values()]
    assert {2, 3, 4, 16} <= {k["num_beams"] for k in kws}
    assert any(k["num_beams"] == 16 and c[1] == 1 for c, k in zip(br.CASES.values(), kws))
    assert any("eos_token_ids" not in k for k in kws) and {1, 3} <= {len(k.get("eos_token_ids", ())) for k in kws}
    assert {0.6, 1.0, 2.0} <= {k.get("length_penalty", 1.0) for k in kws}
    assert any(k.get("repetition_penalty") == 1.3 for k in kws)
    assert any(k.get("num_return_sequences") == k["num_beams"] for k in kws)
    assert any(c[2] == 1 for c in br.CASES.values()) and any(k["max_length"] == c[2] + 1 for c, k in zip(br.CASES.values(), kws))


# ------------------------------------------------------------------------------------------------ the hypothesis rule, both statements
def both_lists(n, max_length, lp):
    from rag4dyg_amd.gpt2 import BeamHyps
    return br.Hyps(n, max_length, lp), BeamHyps(n, max_length, lp)


@pytest.mark.parametrize("which", [0, 1])
def test_hypothesis_rule_fill_displace_equal_scores_and_is_done(which):
    h = both_lists(2, 11, 1.0)[which]
    assert not h.is_done(0.0)                                 # not full: never done
    h.add([1, 2, 3, 4], -4.0)                                 # score -1
    assert h.worst == -1.0 and len(h.beams) == 1
    h.add([1, 2], -6.0)                                       # score -3: the list is full
    assert h.worst == -3.0 and [b[1] for b in h.beams] == [[1, 2, 3, 4], [1, 2]]
    h.add([7, 7], -6.0)                                       # equal to worst: not better, refused
    assert [b[1] for b in h.beams] == [[1, 2, 3, 4], [1, 2]] and h.worst == -3.0
    h.add([9, 9, 9, 9], -8.0)                                 # score -2 displaces -3; worst = the lowest that stays
    assert [b[1] for b in h.beams] == [[1, 2, 3, 4], [9, 9, 9, 9]] and h.worst == -2.0
    h.add([8, 8], -2.0)                                       # score -1 == the best's: -2 leaves, both -1 stay
    assert [b[1] for b in h.beams] == [[1, 2, 3, 4], [8, 8]] and h.worst == -1.0
    h.add([6], -0.5)                                          # two equal lowest scores: the earliest arrival leaves
    assert [b[1] for b in h.beams] == [[8, 8], [6]] and h.worst == -1.0
    # is_done divides by (max_length - 1) ** lp = 10: both sides of worst = -1
    assert h.is_done(-10.0) and h.is_done(-10.5) and not h.is_done(-9.5)
    assert h.best(2) == [[6], [8, 8]]
    e = both_lists(2, 11, 1.0)[which]
    e.add([1], -1.0)
    e.add([2], -1.0)
    assert e.best(2) == [[2], [1]]                            # equal scores: the latest arrival is returned first


@pytest.mark.parametrize("lp", [0.6, 2.0])
def test_both_statements_agree_on_a_random_stream_of_hypotheses(lp):
    rng = np.random.default_rng(3)
    a, b = both_lists(3, 20, lp)
    for _ in range(200):
        ids = list(range(int(rng.integers(1, 19))))
        s = -float(rng.integers(1, 40)) / 4                   # a coarse grid: equal scores occur
        a.add(ids, s)
        b.add(ids, s)
        assert [(x[0], list(x[1])) for x in a.beams] == [(y[0], list(y[1])) for y in b.beams] and a.worst == b.worst
        q = -float(rng.integers(1, 400)) / 4
        assert a.is_done(q) == b.is_done(q)
    assert a.best(3) == b.best(3)


# ------------------------------------------------------------------------------------------------ the last step on the host
def filled(n, max_length, rows):
    out = both_lists(n, max_length, 1.0)
    for h in out:
        for ids, s in rows:
            h.add(ids, s)
    return out


def test_finalisation_pads_appends_the_eos_and_orders_the_rows():
    from rag4dyg_amd.gpt2 import beam_finalize
    # prompt 0: a short finished hypothesis beats a full-length one; prompt 1: two of full length
    r0 = [([3, 4, 9], -0.3), ([3, 4, 1, 2, 6, 7], -6.0)]
    r1 = [([5, 5, 1, 1, 1, 1], -1.2), ([5, 5, 2, 2, 2, 2], -0.6)]
    for n_ret in (1, 2):
        ref = br.finalize([filled(2, 6, r0)[0], filled(2, 6, r1)[0]], n_ret, 6, 0, [9, 8])
        got = beam_finalize([filled(2, 6, r0)[1], filled(2, 6, r1)[1]], n_ret, 6, 0, [9, 8])
        assert got.dtype == torch.long and np.array_equal(got.numpy(), ref)
    assert ref.tolist() == [[3, 4, 9, 9, 0, 0], [3, 4, 1, 2, 6, 7],            # row i * n_ret + j: prompt i's j-th best; the short row gets
                            [5, 5, 2, 2, 2, 2], [5, 5, 1, 1, 1, 1]]            # eos_token_ids[0] behind it, then the pad id
    # the width is one past the longest row, at most max_length
    ref = br.finalize([filled(2, 9, [([1, 2], -0.2), ([1, 2, 3, 4], -0.8)])[0]], 2, 9, 7, [6])
    got = beam_finalize([filled(2, 9, [([1, 2], -0.2), ([1, 2, 3, 4], -0.8)])[1]], 2, 9, 7, [6])
    assert np.array_equal(got.numpy(), ref) and ref.tolist() == [[1, 2, 6, 7, 7], [1, 2, 3, 4, 6]]
    # rows of one length are returned as they are: nothing appended
    got = beam_finalize([filled(2, 9, [([1, 2, 3], -0.3), ([4, 5, 6], -0.6)])[1]], 2, 9, None, None)
    assert got.tolist() == [[1, 2, 3], [4, 5, 6]]
    with pytest.raises(AssertionError):
        beam_finalize([filled(2, 9, [([1, 2], -0.2), ([1, 2, 3, 4], -0.8)])[1]], 2, 9, None, None)


# ------------------------------------------------------------------------------------------------ generate's argument checks
def tiny_cpu_model(vocab=40):
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    return GPT2LMHeadModel(GPT2Config(vocab_size=vocab, n_positions=32, n_ctx=32, n_embd=64, n_layer=1, n_head=2))


def test_generate_checks_the_beam_arguments():
    m = tiny_cpu_model()
    ids = torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(AssertionError, match="cannot return more sequences than it has beams"):
        m.generate(input_ids=ids, max_length=8, num_beams=2, num_return_sequences=3)
    with pytest.raises(AssertionError, match="Greedy decoding will always produce the same output"):
        m.generate(input_ids=ids, max_length=8, num_beams=1, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        m.generate(input_ids=ids, max_length=8, num_beams=2)                     # a model whose weights are not on a GPU
    with pytest.raises(NotImplementedError):
        m.generate(input_ids=ids, max_length=8, num_beams=2, do_sample=True)
    with pytest.raises(NotImplementedError):
        m.generate(input_ids=ids, max_length=8, num_beams=17)


def test_sampled_beams_too_many_beams_and_a_one_id_vocabulary_are_refused_before_the_device_is_looked_at():
    from rag4dyg_amd import gpt2
    m = tiny_cpu_model()
    ids = torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="sampled beam search"):
        m.generate(input_ids=ids, max_length=8, num_beams=2, do_sample=True)
    with pytest.raises(NotImplementedError, match="at most 16 beams"):
        m.generate(input_ids=ids, max_length=8, num_beams=17)
    one = tiny_cpu_model(vocab=1)
    with pytest.raises(ValueError, match="at least 2 ids"):
        one.generate(input_ids=ids, max_length=8, num_beams=2)
    assert gpt2._GENERATE_DEFAULTS["num_beams"] == 1


@has_ref
def test_fixture_regenerates_from_the_reference(tmp_path):
    env = dict(os.environ, R4D_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_beam_fixture.py")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    new, old = np.load(tmp_path / (br.FIXTURE + ".npz")), load_golden(br.FIXTURE)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k

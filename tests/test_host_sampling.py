"""Sampled decoding without a GPU: the ABI surface, ``generate``'s argument checks, and the float64 restatement of the sampler
(tests/_sampling_ref.py) against the kept sets the reference's own functions gave (tests/golden/g15_sampling_filter.npz)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

import _sampling_ref as sr

REF = "/root/reference"
has_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
NEW_SYMBOLS = ("r4d_sample_logits_f32", "r4d_gpt2_sample_workspace_bytes", "r4d_gpt2_sample_step_f32", "r4d_gpt2_sample_graph_create")


def test_sampling_symbols_are_declared_bound_and_exported_at_abi_6():
    from rag4dyg_amd import _lib
    hdr = open(os.path.join(REPO, "include", "r4d.h")).read()
    declared = set(re.findall(r"\b(r4d_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.r4d_abi_version() == _lib.R4D_ABI_VERSION == 6
    assert "R4D_ABI_VERSION 6" in hdr
    # the sampled state is the greedy state's fields, in order, then the sampler's four pointers
    names = [n for n, _ in _lib.SampleStateC._fields_]
    assert names[:len(_lib.GreedyStateC._fields_)] == [n for n, _ in _lib.GreedyStateC._fields_]
    assert names[len(_lib.GreedyStateC._fields_):] == ["seen_d", "stream_d", "fparams_d", "iparams_d"]
    body = hdr[hdr.index("typedef struct r4d_sample_state {"):hdr.index("} r4d_sample_state;")]
    assert re.findall(r"\b(\w+_d|out_cap);", body) == names
    cfg = _lib.GPT2ConfigC(2, 2, 256, 1801, 512, 1e-5)
    import ctypes
    assert lib.r4d_gpt2_sample_workspace_bytes(ctypes.byref(cfg), 5) == lib.r4d_gpt2_greedy_workspace_bytes(ctypes.byref(cfg), 5) > 0


def test_new_dispatcher_branches_are_tuning_branches_and_the_profile_class_exists():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    mine = [n for n in names if "sample" in n]
    assert len(mine) == 2 and all(n.startswith("tuning:sample:") for n in mine), mine
    classes = [lib.r4d_profile_class_name(c).decode() for c in range(lib.r4d_profile_num_classes())]
    assert "sample_advance" in classes and "greedy_advance" in classes


def test_both_head_models_have_generate():
    from rag4dyg_amd.gpt2 import GPT2LMHeadModel, GPT2LMHeadModelRAG, GreedyDecoder, SamplingDecoder
    assert hasattr(GPT2LMHeadModel, "generate") and hasattr(GPT2LMHeadModelRAG, "generate")
    assert GPT2LMHeadModel.generate is GPT2LMHeadModelRAG.generate
    assert issubclass(SamplingDecoder, GreedyDecoder)


def tiny_cpu_model():
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModel
    return GPT2LMHeadModel(GPT2Config(vocab_size=40, n_positions=32, n_ctx=32, n_embd=64, n_layer=1, n_head=2))


@pytest.mark.parametrize("kw", [dict(max_length=0), dict(max_length=2.5), dict(do_sample=1), dict(num_beams=0), dict(temperature=0.0),
                                dict(temperature=-1.0), dict(top_k=-1), dict(top_k=2.0), dict(top_p=1.5), dict(top_p=-0.1),
                                dict(repetition_penalty=0.9), dict(pad_token_id=-1), dict(eos_token_ids="x"), dict(length_penalty=0.0),
                                dict(num_return_sequences=0), dict(do_sample=False, num_return_sequences=2),
                                dict(input_ids=torch.zeros(3, dtype=torch.long))])
def test_generate_refuses_what_the_reference_asserts(kw):
    m = tiny_cpu_model()
    args = dict(input_ids=torch.zeros(1, 3, dtype=torch.long), max_length=8)
    args.update(kw)
    with pytest.raises(AssertionError):
        m.generate(**args)


def test_generate_without_prompt_needs_a_bos_id_and_beam_search_is_not_built():
    m = tiny_cpu_model()
    with pytest.raises(AssertionError):
        m.generate(max_length=4)                                                  # no input_ids, no bos_token_id
    with pytest.raises(NotImplementedError):
        m.generate(input_ids=torch.zeros(1, 3, dtype=torch.long), max_length=8, num_beams=2)
    with pytest.raises(NotImplementedError):
        m.generate(input_ids=torch.zeros(1, 3, dtype=torch.long), max_length=8, eos_token_ids=[1, 2, 3, 4, 5])
    with pytest.raises(ValueError):                                               # a penalty over a prompt nobody named
        m.generate(inputs_embeds=torch.zeros(1, 3, 64), max_length=8, repetition_penalty=1.2)
    with pytest.raises(ValueError):
        m.generate(input_ids=torch.zeros(1, 3, dtype=torch.long), max_length=33)  # beyond n_positions


def test_generate_defaults_come_from_the_config_then_from_the_reference():
    from rag4dyg_amd import gpt2
    assert gpt2._GENERATE_DEFAULTS == dict(max_length=20, do_sample=False, num_beams=1, temperature=1.0, top_k=50, top_p=1.0,
                                           repetition_penalty=1.0, bos_token_id=None, pad_token_id=None, eos_token_ids=None,
                                           length_penalty=1.0, num_return_sequences=1)
    m = tiny_cpu_model()
    m.config.num_beams = 3                                                        # a config that carries a value wins over the default
    with pytest.raises(NotImplementedError):
        m.generate(input_ids=torch.zeros(1, 3, dtype=torch.long), max_length=8)
    ids = torch.arange(6).view(2, 3)
    assert torch.equal(m.generate(input_ids=ids, max_length=3, num_beams=1), ids)   # nothing to generate: the prompt, no GPU touched


def test_philox_restatement_known_answers():
    # the test vectors of the Random123 distribution (kat_vectors: philox4x32 10)
    assert [int(v) for v in sr.philox4x32_10([0] * 4, [0] * 2)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v) for v in sr.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    u, w = sr.philox_u(123, np.arange(4096), 0)
    assert np.all((0 <= u) & (u < 1)) and np.array_equal((w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24, u)
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * 4096)


def test_restatement_gives_the_reference_kept_sets_of_the_fixture():
    g = load_golden("g15_sampling_filter")
    assert np.array_equal(g["grid"], np.asarray(sr.GRID, dtype=np.float64)) and tuple(g["sizes"]) == sr.FIXTURE_SIZES
    for V in sr.FIXTURE_SIZES:
        x, seen = sr.make_logits(V, sr.SEEDS[V])
        assert np.array_equal(x, g[f"x_{V}"]) and np.array_equal(sr.pack_bits(seen), g[f"seen_{V}"])
        assert np.unique(x).size == V
        keeps = sr.unpack_bits(g[f"keep_{V}"], V)
        for i, (k, p, t, r) in enumerate(sr.GRID):
            res = sr.sample_row(x, seen, True, t, k, p, r)
            assert res["p_margin"] > sr.P_MARGIN and res["k_margin"] > sr.K_MARGIN, (V, k, p, t, r)
            assert np.array_equal(res["keep"], keeps[i]), (V, k, p, t, r)
            assert res["keep"][res["token"]] and sr.draw_ok(res["token"], res)


def test_rows_beyond_the_fixture_have_the_same_margins():
    for V in (16385, 50257):
        x, seen = sr.make_logits(V, sr.SEEDS[V])
        assert np.unique(x).size == V and sr.grid_margins_ok(x, seen)


def test_restatement_edge_rules_and_ties():
    nan, inf = float("nan"), float("inf")
    assert sr.sample_row(np.array([nan, -inf, nan], np.float32))["token"] == 0                      # nothing above -inf: id 0
    assert sr.sample_row(np.array([nan, 1.0, inf, inf], np.float32))["token"] == 2                  # lowest-indexed +inf
    r = sr.sample_row(np.array([nan, 0.5, nan], np.float32), seed=3)
    assert r["token"] == 1 and list(r["keep"]) == [True, True, True] and r["w"][0] == 0             # NaN: weight 0, never drawn
    # several equal values on the top-k threshold are all kept
    x = np.array([3, 1, 2, 2, 0, 2, 5], np.float32)
    assert list(np.nonzero(sr.sample_row(x, top_k=3)["keep"])[0]) == [0, 2, 3, 5, 6]
    # equal values across the top-p cut: index ascending
    x = np.array([0, 1, 0, 0, 0, 0], np.float32)                                                    # weights 1 : e : 1 : 1 : 1 : 1
    z = np.e + 5
    r = sr.sample_row(x, top_p=(np.e + 1.5) / z)                                                    # mass in front: 0, e, e+1 kept; e+2 not
    assert list(np.nonzero(r["keep"])[0]) == [0, 1, 2]
    # the penalty multiplies negative logits and divides positive ones
    y = sr.transform(np.array([2.0, -2.0, 2.0, -2.0], np.float32), np.array([1, 1, 0, 0], bool), True, 1.0, 2.0)
    assert list(y) == [1.0, -4.0, 2.0, -2.0]


def test_frequency_case_is_sound_on_the_cpu():
    x, p, n, seed, tok, near, q = sr.frequency_case()
    assert near.mean() <= 1e-3                                         # draws the restatement itself cannot place
    counts = np.bincount(tok, minlength=8)
    sigma = np.sqrt(n * q * (1 - q))
    assert np.all(np.abs(counts - n * q) <= 5 * sigma), (counts, n * q)
    assert np.max(np.abs(q - p)) < 1e-6


@has_ref
def test_fixture_regenerates_from_the_reference(tmp_path):
    env = dict(os.environ, R4D_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_sampling_fixture.py")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    new, old = np.load(tmp_path / "g15_sampling_filter.npz"), load_golden("g15_sampling_filter")
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k

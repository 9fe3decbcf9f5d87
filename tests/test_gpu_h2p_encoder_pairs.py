"""The encoder with the LDS-DMA f16x2 GEMMs (``r4d_set_gemm_h2p`` on: at the 128 x 256 tile the c_fc line output and the
row-major / residual outputs on the column-pair mapping, the h2-word c_attn and layer 0's row-block map on one column per lane)
against the register-staged kernels (off): per-layer hidden rows, the last hidden state and the mean-pool bit for bit.
Key-blocked K and layer 0's pad rows are on.

Small batches (B 2, T 5 / 33 / 70: rows off the multiples of 32) keep every launch on the 128 x 128 tile; the large call of each
model has the rows at which the dispatcher takes the 128 x 256 tile for c_attn (N = 3 d) and c_fc (N = 4 d) -- 3,200 rows at
d 512, 2,240 at d 768, 5,760 at d 256 (``pick_tile_128``) -- so that the two mappings of that tile run side by side inside the
encoder, the key-blocked K image at head_dim 32 / 96 / 128 / 256 included."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, P, PAD = 64, 128, 63
MODELS = {"d512_H2_hd256": (2, 2, 512, (32, 100)), "d256_H2_hd128": (2, 2, 256, (64, 90)), "d256_H8_hd32": (2, 8, 256, (64, 90)),
          "d768_H8_hd96": (2, 8, 768, (32, 70))}
W256 = "gemm_h2p:128x256x32"
ROWMAP = "gemm_h2p:row-block map"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _hits():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    return {lib.r4d_dispatch_branch_name(i).decode(): int(lib.r4d_dispatch_branch_hits(i)) for i in range(lib.r4d_dispatch_num_branches())}


def _takes_256(M, N):
    """``pick_tile_128`` (csrc/gemm_common.h) restated: the 128 x 256 tile unless the 128 x 128 one needs fewer rounds of the 256 CUs."""
    mt, c = -(-M // 128), lambda n: -(-n // 256)
    return not (c(mt * -(-N // 128)) * 128 * 128 / 0.9 < c(mt * -(-N // 256)) * 128 * 256)


def _ragged(rng, B, T):
    """Right-padded rows: two full sequences, the rest short (long runs of the pad token for layer 0's plan)."""
    b = np.full((B, T), PAD, np.int64)
    for i in range(B):
        n = T if i < 2 else int(rng.integers(1, max(2, T // 3)))
        b[i, :n] = rng.integers(0, PAD, n)
    return b


@pytest.mark.parametrize("name", sorted(MODELS))
def test_encoder_h2p_on_equals_off_bit_for_bit(dev, name):
    from oracle import gpt2_ref
    from rag4dyg_amd import ops
    from rag4dyg_amd.gpt2 import GPT2Config, GPT2LMHeadModelRAG
    L, H, d, (Bbig, Tbig) = MODELS[name]
    mode = ops.gemm_mode()
    ops.set_gemm_mode("f16x2")
    kb, pr = ops.set_attention_kblk(True), ops.set_layer0_pad_rows(True)
    try:
        m = GPT2LMHeadModelRAG(GPT2Config(vocab_size=V, n_positions=P, n_ctx=P, n_embd=d, n_layer=L, n_head=H))
        m.load_state_dict(gpt2_ref.make_state_dict(L, d, V, n_positions=P, seed=d + H, random_affine=True), strict=False)
        m.tie_weights()
        enc = m.to(dev).eval().transformer
        rng = np.random.default_rng(d + H)
        small = [torch.from_numpy(_ragged(rng, 2, T)).to(dev) for T in (5, 33, 70)]
        big = torch.from_numpy(_ragged(rng, Bbig, Tbig)).to(dev)
        outs = {}
        for on in (True, False):
            prev = ops.set_gemm_h2p(on)
            try:
                before = _hits()
                o = [enc.encode(t, want_hidden=False, want_meanpool=True, want_layers=True) for t in small]
                mid = _hits()
                o.append(enc.encode(big, want_hidden=False, want_meanpool=True, want_layers=True))
                if on:
                    # the large call alone: c_attn of layer 1 (layer 0's goes through the row map) and c_fc of both layers are the launches
                    # at the 128 x 256 tile -- pinned by their count
                    M = Bbig * Tbig
                    assert _takes_256(M, 3 * d), (M, d)
                    want = (L - 1) * _takes_256(M, 3 * d) + L * (_takes_256(M, 4 * d) + 2 * _takes_256(M, d))
                    now = _hits()
                    got = sum(now[k] - mid.get(k, 0) for k in now if k.startswith(W256))
                    assert got == want, (name, got, want)
                grp = enc.encode_groups(small + [big], want_hidden=True, want_meanpool=True)
                torch.cuda.synchronize()
                after = _hits()
                outs[on] = ([(x["meanpool"].clone(), [y.clone() for y in x["layers"]]) for x in o],
                            grp["hidden"].clone(), grp["meanpool"].clone())
                ran = {k for k in after if after[k] > before.get(k, 0)}
                if on:
                    assert any(k.startswith(W256) for k in ran) and any(k.startswith(ROWMAP) for k in ran), sorted(ran)
                    assert any("key-blocked K" in k for k in ran), sorted(ran)
                else:
                    assert not any(k.startswith("gemm_h2p") for k in ran), sorted(ran)
            finally:
                ops.set_gemm_h2p(prev)
        def same(a, b):
            return torch.equal(a.view(torch.int32), b.view(torch.int32))
        for i, ((p1, l1), (p0, l0)) in enumerate(zip(outs[True][0], outs[False][0])):
            assert len(l1) == len(l0) == L
            for k, (a, b) in enumerate(zip(l1, l0)):
                assert same(a, b), (name, "batch", i, "layer", k, float((a - b).abs().max()))
            assert same(p1, p0), (name, "batch", i, "meanpool", float((p1 - p0).abs().max()))
            assert torch.isfinite(p1).all()
        assert same(outs[True][1], outs[False][1]), (name, "groups hidden", float((outs[True][1] - outs[False][1]).abs().max()))
        assert same(outs[True][2], outs[False][2]), (name, "groups meanpool")
    finally:
        ops.set_layer0_pad_rows(pr)
        ops.set_attention_kblk(kb)
        ops.set_gemm_mode(mode)

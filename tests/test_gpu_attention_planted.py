"""The encoder attention kernels on planted logits (tests/_attention_ref.py), per (sequence, head) slice against float64.

Seven forms: the fused exact-f32 kernels as the dispatcher picks them (key-split at head_dim 32 / 64, column-split at 96 / 128 /
256), the key-split kernel forced at the wide heads, the three-launch GEMM form, and the f16x2 kernels (``attn_h2ks_kernel`` up to
head_dim 96, ``attn_h2_kernel`` beyond) reading K row-major or from the key-blocked image.  Each is selected through the existing
switches, and the dispatcher's branch counters say that it -- and no other -- ran.

  a. values: eight logit patterns x ten lengths (1 .. 1024: each side of the 32-key tile and of the 128-key super-tile) at B = 3,
     H = 2 -- sequences 1 and 2 start mid-block whenever T is no multiple of 32, and 6 (sequence, head) pairs leave two of the
     eight XCD slots of the 1-D mapping empty -- plus B = 5, H = 3 at head_dim 64 / 128.  Bound: the project's numbers for this
     operation or 4 x the float32 CPU yardstick of the same case (``_attention_ref.device_bound``); ``flat`` must be the plain
     mean it is, without any reference; a second launch gives the same bits; key-blocked = row-major bit for bit.
  b. isolation: a sequence's output does not depend on its neighbours in the launch (NaN words there), is bit-identical to the
     same sequence run alone, and no row outside [B, T, d] is written.
  c. refusals: bad shapes and a short workspace are refused with a message before any dispatch or launch.

tests/test_host_attention_planted.py shows, without a GPU, that a lost or doubled tile-boundary key, a missing rescale, an
off-by-one mask, an unweighted merge or a neighbour's keys move a planted case by 10x or more of the bound of (a).  The measured
errors are recorded in profiles/attention_planted.md."""
import contextlib

import pytest
import torch

from _attention_ref import case, device_bound, forget_cases, patterns_for, slice_errs

pytestmark = pytest.mark.gpu

TS = (1, 31, 32, 33, 127, 128, 129, 160, 257, 1024)
B, H = 3, 2
EXTRA_LAYOUT = dict(B=5, H=3, hds=(64, 128), Ts=(33, 129, 257))
NAN_F32, NAN_H2 = 0x7FC0BEEF, 0x7e007e00      # a quiet fp32 NaN with a payload; fp16 NaN in both halves of an h2 word
GUARD_ROWS = 64

FORM_HDS = {"fused": (32, 64, 96, 128, 256), "keysplit_forced": (96, 128, 256), "three_launch": (32, 48, 64, 96, 128, 256),
            "h2": (32, 64, 96, 128, 256), "h2_kblk": (32, 64, 96, 128, 256)}
FUSED_MODE = {"fused": True, "keysplit_forced": 2, "three_launch": False}
# by head_dim, so that the forms of one head_dim share the cached references (``_attention_ref.case`` keeps one head_dim)
VALUE_CASES = sorted(((f, hd) for f, hds in FORM_HDS.items() for hd in hds), key=lambda c: (c[1], list(FORM_HDS).index(c[0])))
ISOLATION_CASES = [("fused", 64), ("fused", 256), ("keysplit_forced", 256), ("three_launch", 48), ("h2", 96), ("h2", 256),
                   ("h2_kblk", 96), ("h2_kblk", 256)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _cases_forgotten():
    yield
    forget_cases()


def fused_branch(hd):
    return f"attention:{'key-split' if hd <= 64 else 'column-split'} hd{hd}"


def branch_of(form, hd):
    if form == "fused":
        return fused_branch(hd)
    if form == "keysplit_forced":
        return "tuning:attention:key-split at hd96/128/256"
    if form == "three_launch":
        return "attention:three-launch GEMM form"
    return f"attention:f16x2 {'key-split ' if hd < 128 else ''}hd{hd}" + (", key-blocked K" if form == "h2_kblk" else "")


def attention_hits():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    names = [lib.r4d_dispatch_branch_name(i).decode() for i in range(lib.r4d_dispatch_num_branches())]
    return {n: int(lib.r4d_dispatch_branch_hits(i)) for i, n in enumerate(names) if "attention:" in n and "decode" not in n}


def all_hits():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    return [int(lib.r4d_dispatch_branch_hits(i)) for i in range(lib.r4d_dispatch_num_branches())]


@contextlib.contextmanager
def fused_mode(mode):
    from rag4dyg_amd import ops
    ops.set_attention_fused(mode)
    try:
        yield
    finally:
        ops.set_attention_fused(None)


def bits(t):
    return t.view(torch.int32)


def layouts_of(hd):
    extra = [(EXTRA_LAYOUT["B"], EXTRA_LAYOUT["H"], EXTRA_LAYOUT["Ts"])] if hd in EXTRA_LAYOUT["hds"] else []
    return [(B, H, TS)] + extra


def launcher(form, x, nh):
    """-> (a function that launches ``form`` on the device tensor ``x`` [B, T, 3d] and returns its output, the h2 words or None)."""
    from rag4dyg_amd import ops
    if form == "h2":
        words = ops.pack_h2_words(x)
        return (lambda: ops.attention_h2(words, nh)), words
    if form == "h2_kblk":
        words = ops.pack_h2_words(x)
        kblk = ops.pack_kblk_words(words, nh)
        return (lambda: ops.attention_h2_kblk(words, kblk, nh)), words

    def run():
        with fused_mode(FUSED_MODE[form]):
            return ops.attention(x, nh)
    return run, None


@pytest.mark.parametrize("form,hd", VALUE_CASES, ids=[f"{f}-hd{hd}" for f, hd in VALUE_CASES])
def test_planted_values_per_sequence_and_head(dev, form, hd):
    """Every pattern x T of every layout: the (sequence, head) slices against float64 inside ``device_bound`` of the case's own
    float32 CPU yardstick, a second launch the same bits, key-blocked = row-major bit for bit; the f16x2 forms beside the exact-f32
    fused kernel on the same input (printed).  Every case runs and prints its figures; the failures are asserted at the end."""
    from rag4dyg_amd import ops
    is_h2 = form.startswith("h2")
    before = attention_hits()
    calls = 0
    worst, bad = {}, []
    for nb, nh, Ts in layouts_of(hd):
        for T in Ts:
            for pattern in patterns_for(T):
                qkv, want, f32 = case(nb, T, nh, hd, pattern)
                x = qkv.to(dev)
                calls += 1
                run, words = launcher(form, x, nh)
                got, again = run(), run()
                if not torch.equal(bits(got), bits(again)):
                    bad.append((pattern, nb, T, "a second launch gives other bits"))
                if form == "h2_kblk" and not torch.equal(bits(got), bits(ops.attention_h2(words, nh))):
                    bad.append((pattern, nb, T, "key-blocked != row-major"))
                ratio = 0.0
                got = got.cpu()
                if not bool(torch.isfinite(got).all()):
                    bad.append((pattern, nb, T, "not finite"))
                e, w = slice_errs(got.numpy(), want.numpy(), nh)
                e_max, w_max = device_bound(*f32)
                if is_h2:
                    with fused_mode(True):
                        exact = ops.attention(x, nh).cpu()
                    ratio = e / max(slice_errs(exact.numpy(), want.numpy(), nh)[0], 2.0 ** -24)     # (T = 1: the exact-f32 kernels return v itself)
                print(f"[attn-planted case] {form} hd {hd} B {nb} H {nh} {pattern} T {T}: device {e:.2e} {w:.3f}  float32 {f32[0]:.2e} "
                      f"{f32[1]:.3f}  bound {e_max:.1e} {w_max:.2f}" + (f"  h2 / exact-f32 kernel {ratio:.2f}" if is_h2 else ""))
                ww = worst.setdefault(pattern, [0.0, 0.0, 0.0, 0.0, 0.0])
                worst[pattern] = [max(a, b_) for a, b_ in zip(ww, (e, w, f32[0], f32[1], ratio))]
                if not (e < e_max and w < w_max):
                    bad.append((pattern, nb, T, "device", e, w, "bound", e_max, w_max))
    for pattern, (e, w, fe, fw, r) in worst.items():
        print(f"[attn-planted] {form} hd {hd} {pattern}: device {e:.2e} {w:.3f}  float32 {fe:.2e} {fw:.3f}"
              + (f"  h2 / exact-f32 kernel {r:.2f}" if is_h2 else ""))
    # the form under test ran, and nothing else did: 2 launches per case, plus the comparison launches of the f16x2 forms
    want_hits = {branch_of(form, hd): 2 * calls}
    if is_h2:
        want_hits[fused_branch(hd)] = calls
    if form == "h2_kblk":
        want_hits[branch_of("h2", hd)] = calls
    hits = {n: v - before[n] for n, v in attention_hits().items() if v != before[n]}
    assert hits == want_hits, (hits, want_hits)
    assert not bad, (form, hd, bad)


@pytest.mark.parametrize("form,hd", VALUE_CASES, ids=[f"{f}-hd{hd}" for f, hd in VALUE_CASES])
def test_flat_logits_give_the_plain_mean(dev, form, hd):
    """``flat`` (q = 0, v[..., 0] = 1, v[..., 1] = j) needs no reference: output row i is the mean over keys 0 .. i, so column 0
    is 1 and column 1 is i / 2, each to 1e-5 relative -- a key lost or doubled moves them by 1 / (i + 1).

    This test found the three-launch form 1.407e-05 off at T = 1024 (row 993): it normalised P BEFORE the P.V GEMM, whose k-loop
    then added 994 copies of fl(1 / 994) one after the other in fp32.  It now divides after P.V, like the fused kernels
    (profiles/attention_planted.md)."""
    bad = []
    for nb, nh, Ts in layouts_of(hd):
        for T in Ts:
            x = case(nb, T, nh, hd, "flat")[0].to(dev)
            o = launcher(form, x, nh)[0]().cpu().view(nb, T, nh, hd).double()
            half_i = (torch.arange(T, dtype=torch.float64) / 2).view(1, T, 1)
            e0 = (o[..., 0] - 1.0).abs()
            e1 = (o[..., 1] - half_i).abs()
            print(f"[attn-planted flat] {form} hd {hd} B {nb} H {nh} T {T}: column 0 off 1 by {float(e0.max()):.3e} (row "
                  f"{int(e0.amax(dim=(0, 2)).argmax())}), column 1 off i / 2 by {float((e1 / half_i.clamp(min=0.5)).max()):.3e} relative")
            if not bool((e0 <= 1e-5).all()):
                bad.append((nb, T, "column 0 is not 1", float(e0.max())))
            if not bool((e1 <= 1e-5 * half_i).all()):
                bad.append((nb, T, "column 1 is not i / 2", float((e1 / half_i.clamp(min=0.5)).max())))
    assert not bad, (form, hd, bad)


# ------------------------------------------------------------------------------------------------------------ b. isolation
def _raw_attention(form, x_ptr, nb, T, nh, d, out_ptr, dev):
    """One call of the raw entry point of ``form`` on device pointers (the caller keeps the allocations alive)."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    if not form.startswith("h2"):
        ws = torch.empty(max(int(lib.r4d_attention_workspace_bytes(nb, nh, T)), 256), dtype=torch.uint8, device=dev)
        _lib.check(lib.r4d_attention_f32(x_ptr, nb, T, nh, d, out_ptr, ws.data_ptr(), ws.numel(), s), "attention")
        torch.cuda.synchronize()
        return
    if form == "h2":
        _lib.check(lib.r4d_attention_h2_f32(x_ptr, nb, T, nh, d, out_ptr, s), "attention_h2")
        torch.cuda.synchronize()
        return
    blocks = (nb * T + 31) // 32                  # the image of the call's rows, one NaN block before and one after it
    img = torch.full(((blocks + 2) * 32 * d,), NAN_H2, dtype=torch.int32, device=dev)
    img_ptr = img.data_ptr() + 32 * d * 4
    _lib.check(lib.r4d_pack_kblk_words(x_ptr, nb * T, nh, d, img_ptr, s), "pack_kblk_words")
    _lib.check(lib.r4d_attention_h2_kblk_f32(x_ptr, img_ptr, nb, T, nh, d, out_ptr, s), "attention_h2_kblk")
    torch.cuda.synchronize()
    assert bool((img[:32 * d] == NAN_H2).all()) and bool((img[(blocks + 1) * 32 * d:] == NAN_H2).all()), "the image's guard blocks were written"


def _guarded_call(form, seqs, nan_word, T, nh, d, dev):
    """``seqs`` (a list of [T, 3d] int32 bit patterns, None = a NaN sequence) between one NaN sequence before and one after, the
    output between ``GUARD_ROWS`` NaN rows on each side.  Returns the output rows [len(seqs) * T, d] as int32 bits."""
    nb = len(seqs)
    x = torch.full((nb + 2, T, 3 * d), nan_word, dtype=torch.int32, device=dev)
    for i, sq in enumerate(seqs):
        if sq is not None:
            x[i + 1] = sq
    out = torch.full((2 * GUARD_ROWS + nb * T, d), nan_word, dtype=torch.int32, device=dev)
    _raw_attention(form, x.data_ptr() + T * 3 * d * 4, nb, T, nh, d, out.data_ptr() + GUARD_ROWS * d * 4, dev)
    assert bool((out[:GUARD_ROWS] == nan_word).all()) and bool((out[GUARD_ROWS + nb * T:] == nan_word).all()), \
        (form, T, "a row outside [B, T, d] was written")
    return out[GUARD_ROWS:GUARD_ROWS + nb * T]


@pytest.mark.parametrize("form,hd", ISOLATION_CASES, ids=[f"{f}-hd{hd}" for f, hd in ISOLATION_CASES])
def test_a_sequence_is_independent_of_its_neighbours(dev, form, hd):
    """``spike`` at T = 33 and 129, B = 3: the call sits inside larger allocations whose other sequences, and then also the call's
    own sequences 0 and 2, hold NaN words; the output has NaN guard rows.  Sequence 1 is finite and equal, bit for bit, to the same
    sequence run alone; the guards keep their pattern.  Every address a kernel forms stays inside these allocations."""
    from rag4dyg_amd import ops
    is_h2 = form.startswith("h2")
    nan_word = NAN_H2 if is_h2 else NAN_F32
    d = H * hd
    with fused_mode(FUSED_MODE.get(form)):
        for T in (33, 129):
            qkv = case(B, T, H, hd, "spike")[0].to(dev)
            x = bits(ops.pack_h2_words(qkv) if is_h2 else qkv)
            alone = _guarded_call(form, [x[1]], nan_word, T, H, d, dev)
            assert bool(torch.isfinite(alone.view(torch.float32)).all()), (form, T)
            in_batch = _guarded_call(form, [x[0], x[1], x[2]], nan_word, T, H, d, dev)
            assert bool(torch.isfinite(in_batch.view(torch.float32)).all()), (form, T, "a sequence of the call saw the NaN rows around it")
            among_nan = _guarded_call(form, [None, x[1], None], nan_word, T, H, d, dev)
            for what, out in (("in a batch", in_batch), ("between NaN sequences", among_nan)):
                mine = out[T:2 * T]
                assert bool(torch.isfinite(mine.view(torch.float32)).all()), (form, T, what)
                diff = (mine.view(torch.float32).double() - alone.view(torch.float32).double()).abs().max().item()
                print(f"[attn-planted isolation] {form} hd {hd} T {T} {what}: max |difference| from the sequence alone {diff:.2e}")
                assert torch.equal(mine, alone), (form, T, what, diff)


# ------------------------------------------------------------------------------------------------------------ c. refusals
def test_bad_shapes_and_a_short_workspace_are_refused_before_any_launch(dev):
    """``r4d_attention_f32`` at B = 0, T = 0, T = 1025, a head_dim that is no multiple of 16 and a short workspace, the two f16x2
    entries at head_dim 48: nonzero with a message, no dispatcher count moves, the NaN-filled output keeps its bits."""
    from rag4dyg_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    qkv = torch.zeros(2 * 1025 * 3 * 64, dtype=torch.int32, device=dev)          # every refused shape would fit
    kblk = torch.zeros(2 * 1056 * 64, dtype=torch.int32, device=dev)
    out = torch.full((2 * 1025 * 64,), NAN_F32, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.r4d_attention_workspace_bytes(2, 2, 1024)), dtype=torch.uint8, device=dev)
    f32 = lambda nb, T, nh, d, ws_bytes: lib.r4d_attention_f32(qkv.data_ptr(), nb, T, nh, d, out.data_ptr(), ws.data_ptr(), ws_bytes, s)
    calls = {                                                                    # what: (call, a word of its own message)
        "B = 0": (lambda: f32(0, 33, 2, 64, ws.numel()), "B=0"),
        "B = -1": (lambda: f32(-1, 33, 2, 64, ws.numel()), "B=-1"),
        "T = 0": (lambda: f32(2, 0, 2, 64, ws.numel()), "T=0"),
        "T = 1025": (lambda: f32(2, 1025, 2, 64, ws.numel()), "T=1025"),
        "head_dim 24": (lambda: f32(2, 33, 2, 48, ws.numel()), "multiple of 16"),
        "short workspace": (lambda: f32(2, 33, 2, 96, int(lib.r4d_attention_workspace_bytes(2, 2, 33)) - 256), "workspace"),
        "h2 at head_dim 48": (lambda: lib.r4d_attention_h2_f32(qkv.data_ptr(), 2, 33, 2, 96, out.data_ptr(), s), "head_dim 48"),
        "h2 key-blocked at head_dim 48": (lambda: lib.r4d_attention_h2_kblk_f32(qkv.data_ptr(), kblk.data_ptr(), 2, 33, 2, 96,
                                                                                 out.data_ptr(), s), "head_dim 48"),
    }
    assert int(lib.r4d_attention_workspace_bytes(2, 2, 33)) > 256
    for what, (call, word) in calls.items():
        before = all_hits()
        rc = call()
        msg = lib.r4d_last_error().decode("utf-8", "replace")
        print(f"[attn-planted refusal] {what}: rc {rc}, '{msg}'")
        assert rc != 0 and word in msg, (what, rc, msg)
        assert all_hits() == before, (what, "a dispatcher branch was counted")
        torch.cuda.synchronize()
        assert bool((out == NAN_F32).all()), (what, "the output was written")

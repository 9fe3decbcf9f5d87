"""The cached decode step's reference (tests/_decode_ref.py) pinned to the oracle, and the proof that the GPU test built on it
(tests/test_gpu_decode_long_context.py) has teeth: no GPU needed.

  * ``decode_step_ref`` in float64 == the last row of a float64 ``gpt2_ref.gpt2_forward`` when given that forward's K / V rows;
  * its float32 evaluation stays well inside the bound the device is held to, on the planted caches the device test uses;
  * dropping ONE boundary key of a planted cache moves the float64 output by 10x or more of that bound, so a kernel that loses,
    doubles or mis-weights such a key cannot pass."""
import pytest
import torch

from _decode_ref import PATTERNS, cast_sd, decode_layers_ref, decode_step_ref, plant_cache, spike_keys, trip_of
from conftest import elementwise_err, rel_err
from oracle import gpt2_ref

H, V = 2, 40
WIDTHS = (64, 512)


def positions(d):
    trip = trip_of(d // H)
    return (1, trip, trip + 1, 1023)


_MODELS = {}


def model(d, L=1):
    if (d, L) not in _MODELS:
        sd = gpt2_ref.make_state_dict(L, d, V, n_positions=1024, seed=d + L, random_affine=True)
        _MODELS[(d, L)] = (sd, cast_sd(sd, torch.float64))
    return _MODELS[(d, L)]


_CASES = {}


def case(d, p, pattern):
    """(x_new, K, V) float32, float64 hidden row: built once, shared by the tests below, never modified."""
    key = (d, p, pattern)
    if key not in _CASES:
        sd, sd64 = model(d)
        g = torch.Generator().manual_seed(1000 * d + 7 * p + PATTERNS.index(pattern))
        tok = int(torch.randint(0, V, (1,), generator=g))
        x = sd["transformer.wte.weight"][tok] + sd["transformer.wpe.weight"][p]
        K, Vv = plant_cache(sd, H, x, p, pattern, g)
        _CASES[key] = (x, K, Vv, decode_step_ref(sd64, H, x, K, Vv, torch.float64)[0])
    return _CASES[key]


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("d", WIDTHS)
def test_decode_ref_equals_the_oracle_forward(d, L):
    """float64: the K / V columns of c_attn(ln_1(residual stream)) of a full forward, layer by layer, are the cache; the new row's
    step over them is the forward's last hidden row (and its K / V are the forward's last K / V row)."""
    sd, sd64 = model(d, L)
    T = 131
    ids = torch.randint(0, V, (1, T), generator=torch.Generator().manual_seed(d + L))
    out = gpt2_ref.gpt2_forward(sd64, ids, H, want_logits=False, want_layers=True)
    Ks, Vs = [], []
    for i in range(L):
        p = f"transformer.h.{i}."
        qkv = gpt2_ref.conv1d(gpt2_ref.layer_norm(out["layers"][i][0], sd64[p + "ln_1.weight"], sd64[p + "ln_1.bias"]),
                              sd64[p + "attn.c_attn.weight"], sd64[p + "attn.c_attn.bias"])
        Ks.append(qkv[:, d:2 * d])
        Vs.append(qkv[:, 2 * d:])
    h, k_new, v_new = decode_layers_ref(sd64, H, out["layers"][0][0, -1], [k[:T - 1] for k in Ks], [v[:T - 1] for v in Vs],
                                        torch.float64)
    assert rel_err(h.numpy(), out["hidden"][0, -1].numpy()) < 1e-12
    assert rel_err(k_new.numpy(), torch.stack(Ks)[:, -1].numpy()) < 1e-12
    assert rel_err(v_new.numpy(), torch.stack(Vs)[:, -1].numpy()) < 1e-12


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("d", WIDTHS)
def test_float32_reference_is_inside_the_device_bounds(d, pattern):
    """What plain fp32 costs on these inputs: 10x below the device's rel_err bound (2e-5), 5x below its element-wise one (1)."""
    sd, _ = model(d)
    for p in positions(d):
        x, K, Vv, want = case(d, p, pattern)
        got = decode_step_ref(sd, H, x, K, Vv, torch.float32)[0]
        e, ew = rel_err(got.numpy(), want.numpy()), elementwise_err(got.numpy(), want.numpy())
        print(f"[decode-ref f32] d {d} p {p} {pattern}: rel_err {e:.2e} elementwise_err {ew:.3f}")
        assert e <= 2e-6 and ew <= 0.2, (d, p, pattern, e, ew)


@pytest.mark.parametrize("pattern,floor", [("spike", 0.25), ("flat", 2e-4), ("up", 5e-3), ("down", 5e-3)])
@pytest.mark.parametrize("d", WIDTHS)
def test_dropping_one_boundary_key_moves_the_output(d, pattern, floor):
    """float64: without one key of {0, trip - 1, trip, p - 1, p} (p = the new key) the hidden row moves by at least ``floor`` --
    the planted key of either head of a ``spike`` cache, every such key of a ``flat`` one, the key that holds the maximum of
    ``up`` (p - 1; at p = 1, where that key's logit is -30, the new key p instead: floor 0.25) and ``down`` (0).  The device's pass bound is 2e-5."""
    _, sd64 = model(d)
    trip = trip_of(d // H)
    for p in positions(d):
        x, K, Vv, want = case(d, p, pattern)
        edge = sorted({t for t in (0, trip - 1, trip, p - 1, p) if 0 <= t <= p})
        drop = {"spike": sorted(set(spike_keys(H, p, trip))), "flat": edge, "up": [p - 1], "down": [0]}[pattern]
        need = floor
        if pattern == "up" and p == 1:      # l_0 = -30 + 30 * 0 / 1: the one cached key weighs e^-30 against the new key and holds
            drop, need = [p], 0.25          # no maximum (from p = trip on, l_(p-1) = -30 / p > -0.5 does).  The NEW key holds it, with
        for t in drop:                      # all of the weight: without it the attention output is another row altogether, order 1
            got = decode_step_ref(sd64, H, x, K, Vv, torch.float64, drop_key=t)[0]
            e = rel_err(got.numpy(), want.numpy())
            print(f"[decode-ref drop] d {d} p {p} {pattern}: without key {t} rel_err {e:.2e}")
            assert e >= need, (d, p, pattern, t, e)

"""Plain-torch CPU reference of ONE cached decode step, and planted key/value caches for it (test infra only).

``decode_step_ref`` restates what ``r4d_gpt2_decode_step_f32`` computes for one sequence -- one new row against given cached
K / V rows -- from the oracle's own pieces (``oracle/gpt2_ref.py``: ``layer_norm``, ``conv1d``, ``gelu_new``, ``mlp``), with the
number format a parameter: float64 is the reference the device is held to, float32 the yardstick for what fp32 itself costs.

``plant_cache`` builds cache rows whose attention LOGITS are chosen, not drawn: with ``q_h`` the new row's float64 query of head
``h`` and ``u_h = q_h * sqrt(hd) / (q_h . q_h)``, a cached key ``l * u_h`` has the logit ``l`` exactly, so a pattern can put the
running maximum, an underflowing group or a dominating key on any row -- on the last key of a trip of ``decode_attn_kernel``, on
the first of the next -- and a kernel that drops, doubles or mis-scales that key moves the output by order 1."""
import math

import torch

from oracle import gpt2_ref

PATTERNS = ("spike", "up", "down", "wide", "flat")


def trip_of(head_dim):
    """Keys per trip of ``decode_attn_kernel``: 16 groups of 32 lanes x 8 keys up to head_dim 128, 8 groups of 64 lanes x 8 beyond."""
    return 64 if head_dim > 128 else 128


def cast_sd(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


@torch.no_grad()
def decode_step_ref(sd, n_head, x_new, K, V, dtype, drop_key=None, layer=0, final=True):
    """One block of the reference (``gpt2_ref.block``) for the one new residual row ``x_new`` [d] against the cached rows
    ``K, V`` [p, d] of that layer: ln_1, c_attn, a softmax over the p cached keys and the new key (logits divided by
    sqrt(head_dim), ``modeling_gpt2.py:143``; no mask: only positions <= p exist), c_proj + residual, ln_2, MLP + residual, then
    ``ln_f`` (``final``; a model of several layers loops this with ``final=False`` up to the last, see ``decode_layers_ref``).
    Everything is evaluated in ``dtype`` (weights that already have it are not copied: pass ``cast_sd(sd, dtype)`` when calling
    this often).  ``drop_key`` in [0, p] removes that key and its value from the softmax (p = the new key).
    Returns (hidden row [d], query [d], new K row [d], new V row [d])."""
    pfx = f"transformer.h.{layer}."
    w = lambda name: sd[name].to(dtype)
    x = x_new.to(dtype).view(1, -1)
    d = x.shape[1]
    hd = d // n_head
    qkv = gpt2_ref.conv1d(gpt2_ref.layer_norm(x, w(pfx + "ln_1.weight"), w(pfx + "ln_1.bias")),
                          w(pfx + "attn.c_attn.weight"), w(pfx + "attn.c_attn.bias"))
    q, k_new, v_new = qkv[0].split(d)
    keys = torch.cat([K.to(dtype).view(-1, d), k_new.view(1, d)])
    vals = torch.cat([V.to(dtype).view(-1, d), v_new.view(1, d)])
    if drop_key is not None:
        keep = [t for t in range(keys.shape[0]) if t != drop_key]
        keys, vals = keys[keep], vals[keep]
    n = keys.shape[0]
    logits = torch.einsum("hc,thc->ht", q.view(n_head, hd), keys.view(n, n_head, hd)) / math.sqrt(hd)
    a = torch.einsum("ht,thc->hc", torch.softmax(logits, dim=-1), vals.view(n, n_head, hd)).reshape(1, d)
    x = x + gpt2_ref.conv1d(a, w(pfx + "attn.c_proj.weight"), w(pfx + "attn.c_proj.bias"))
    sdt = {k_: w(k_) for k_ in sd if k_.startswith(pfx + "mlp.")}
    x = x + gpt2_ref.mlp(gpt2_ref.layer_norm(x, w(pfx + "ln_2.weight"), w(pfx + "ln_2.bias")), sdt, pfx + "mlp.")
    if final:
        x = gpt2_ref.layer_norm(x, w("transformer.ln_f.weight"), w("transformer.ln_f.bias"))
    return x[0], q, k_new, v_new


@torch.no_grad()
def decode_layers_ref(sd, n_head, x_new, Ks, Vs, dtype):
    """``decode_step_ref`` looped over the layers of ``sd`` with per-layer caches ``Ks[i], Vs[i]`` [p, d].
    Returns (ln_f hidden row [d], new K rows [n_layer, d], new V rows [n_layer, d])."""
    L = gpt2_ref.n_layers_of(sd)
    x, ks, vs = x_new, [], []
    for i in range(L):
        x, _, k, v = decode_step_ref(sd, n_head, x, Ks[i], Vs[i], dtype, layer=i, final=i == L - 1)
        ks.append(k)
        vs.append(v)
    return x, torch.stack(ks), torch.stack(vs)


def spike_keys(n_head, p, trip):
    """The key ``t*`` of every head that the ``spike`` pattern gives the logit 12: the first key of the second trip (or the last
    cached key before that), the last cached key, key 0."""
    return [min(trip, p - 1) if h == 0 else p - 1 if h == 1 else 0 for h in range(n_head)]


@torch.no_grad()
def plant_cache(sd, n_head, x_new, p, pattern, generator):
    """Cached rows ``K, V`` [p, d] (float32) for layer 0 and the new row ``x_new`` with the logits ``l_t`` of ``pattern``:
    ``K[t, head h] = l_t * u_h + 0.01 * randn``, ``V = randn``, generated in float64 and rounded to float32 once (every
    reference reads the rounded values).

        spike   0.5 * randn, but 12 at one key t* per head (``spike_keys``) whose V slice is multiplied by 4
        up      -30 + 30 t / p    every trip raises the running maximum
        down    -30 t / p         the maximum is the first key, later trips rescale by almost 1
        wide    -100 * rand       whole groups underflow to weight 0
        flat    0                 the output is a plain mean: any miscount of the denominator shows"""
    assert pattern in PATTERNS, pattern
    d = x_new.numel()
    hd = d // n_head
    f64 = dict(dtype=torch.float64, generator=generator)
    if p == 0:
        return torch.zeros(0, d), torch.zeros(0, d)
    q = decode_step_ref(sd, n_head, x_new, torch.zeros(0, d), torch.zeros(0, d), torch.float64)[1].view(n_head, hd)
    u = q * math.sqrt(hd) / (q * q).sum(dim=1, keepdim=True)                       # [H, hd]: (l * u_h) . q_h / sqrt(hd) == l
    t = torch.arange(p, dtype=torch.float64)
    V = torch.randn(p, n_head, hd, **f64)
    if pattern == "spike":
        l = 0.5 * torch.randn(p, n_head, **f64)
        for h, ts in enumerate(spike_keys(n_head, p, trip_of(hd))):
            l[ts, h] = 12.0
            V[ts, h] *= 4.0
    elif pattern == "up":
        l = (-30.0 + 30.0 * t / p).view(p, 1).expand(p, n_head)
    elif pattern == "down":
        l = (-30.0 * t / p).view(p, 1).expand(p, n_head)
    elif pattern == "wide":
        l = -100.0 * torch.rand(p, n_head, **f64)
    else:
        l = torch.zeros(p, n_head, dtype=torch.float64)
    K = l.unsqueeze(-1) * u.unsqueeze(0) + 0.01 * torch.randn(p, n_head, hd, **f64)
    return K.reshape(p, d).float(), V.reshape(p, d).float()

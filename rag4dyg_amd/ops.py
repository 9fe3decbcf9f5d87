"""torch-tensor front end of the C ABI: pointer/shape checks, workspace and stream plumbing only.

Every function requires CUDA(HIP) tensors and raises otherwise -- there is no CPU path here.
"""
import ctypes

import torch

from . import _lib
from ._lib import check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.R4DError(f"{name}: expected a tensor on the GPU (no CPU fallback in rag4dyg_amd)")
    if t.dtype != dtype:
        raise _lib.R4DError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.R4DError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


_WS = {}


def workspace(nbytes, device, tag="default"):
    """Grow-only scratch buffer per (device, tag); the library itself never allocates."""
    key = (str(device), tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def layernorm(x, w, b, eps=1e-5):
    d = x.shape[-1]
    y = torch.empty_like(x)
    rows = x.numel() // d
    check(_lib.load().r4d_layernorm_f32(_dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"),
                                        _dev(b, torch.float32, "b"), rows, d, eps, y.data_ptr(), _stream()), "layernorm")
    return y


def conv1d(x, w, bias, epilogue="none", residual=None, w_t=None):
    """y = epilogue(x @ W[K,N] + bias); epilogue in {'none','gelu','residual'} (Conv1D, modeling_utils.py:1267-1271).
    ``w_t``: optional contiguous transposed copy W^T [N,K] of the (static) weight -> the k-contiguous GEMM kernel."""
    K, N = w.shape
    M = x.numel() // K
    y = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    epi = {"none": 0, "gelu": 1, "residual": 2}[epilogue]
    rp = _dev(residual, torch.float32, "residual") if residual is not None else None
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    tp = _dev(w_t, torch.float32, "w_t") if w_t is not None else None
    check(_lib.load().r4d_conv1d_f32(_dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"), tp, bp, rp, M, K, N, epi,
                                     y.data_ptr(), _stream()), "conv1d")
    return y


_GEMM_MODES = {"f32": 0, "bf16x3": 1, "f16x2": 2}
_GEMM_MODE = None
DEFAULT_GEMM_MODE = "f16x2"


def gemm_mode():
    """Arithmetic of the encoder's Conv1D GEMMs: ``"f16x2"`` -- fp16 matrix cores, two fp16 terms per operand,
    three products per fp32 product; ``"bf16x3"`` -- bf16 matrix cores, three bf16 terms, six products; ``"f32"`` -- the
    exact-f32 MFMA kernels.  All three at fp32 accuracy (error against float64 no larger than the exact-f32 kernel's).
    Default ``DEFAULT_GEMM_MODE``; ``R4D_GEMM_MODE=f32|bf16x3|f16x2`` (or the older ``R4D_GEMM_SPLIT3=0`` for f32) and
    :func:`set_gemm_mode` select another.  Process-wide: the ranks of a sharded job must agree."""
    global _GEMM_MODE
    if _GEMM_MODE is None:
        import os
        m = os.environ.get("R4D_GEMM_MODE")
        if m is None:
            m = "f32" if os.environ.get("R4D_GEMM_SPLIT3", "1") == "0" else DEFAULT_GEMM_MODE
        set_gemm_mode(m)
    return _GEMM_MODE


_LAST_SPLIT_MODE = None


def set_gemm_mode(mode):
    global _GEMM_MODE, _LAST_SPLIT_MODE
    if mode not in _GEMM_MODES:
        raise ValueError(f"gemm mode {mode!r}: one of {sorted(_GEMM_MODES)}")
    _GEMM_MODE = mode
    if mode != "f32":
        _LAST_SPLIT_MODE = mode
    check(_lib.load().r4d_set_gemm_split3(_GEMM_MODES[mode]), "set_gemm_split3")


def gemm_split3_enabled():
    """True unless the exact-f32 MFMA kernels are selected (``gemm_mode() != "f32"``): the bf16x3 planes are in use (also in
    "f16x2" mode, for the training GEMMs and for layers without fp16 planes)."""
    return gemm_mode() != "f32"


def set_gemm_split3(on):
    """Older on / off switch.  False -> "f32".  True -> the split mode that was selected LAST in this process ("f16x2" or
    "bf16x3": off-then-on returns to where it was), else ``R4D_GEMM_MODE`` if that names a split mode, else
    ``DEFAULT_GEMM_MODE``; a no-op while a split mode is already selected."""
    if not on:
        set_gemm_mode("f32")
    elif gemm_mode() == "f32":
        import os
        m = _LAST_SPLIT_MODE or os.environ.get("R4D_GEMM_MODE", DEFAULT_GEMM_MODE)
        set_gemm_mode(m if m != "f32" else DEFAULT_GEMM_MODE)


H2_MAX_WEIGHT = 6.0e4          # fp16 tops out at 65504: a weight beyond this keeps the bf16x3 planes


def split2_planes(w, transposed=False):
    """Static Conv1D weight [K,N] (``transposed``: an [N,K] copy) -> its two fp16 terms (hi, 2^11-scaled lo) as 128-byte lines,
    a uint16 tensor [N, K/32, 2, 32] (fp16 bit patterns; ``[:, :, 0]`` = hi, ``[:, :, 1]`` = lo of 32 consecutive k): the operand
    format of :func:`conv1d_h2`.  K must be a multiple of 32.  None when the weight exceeds the fp16 range (one host read of the
    tensor's maximum, once per checkpoint)."""
    if transposed:
        N, K = w.shape
    else:
        K, N = w.shape
    amax = float(w.detach().abs().max())
    if not (amax < H2_MAX_WEIGHT):
        return None
    if K % 32:
        raise ValueError(f"split2_planes: K = {K} is not a multiple of 32")
    planes = torch.empty(N, K // 32, 2, 32, dtype=torch.int16, device=w.device)
    check(_lib.load().r4d_split2_planes_f16(_dev(w, torch.float32, "w"), K, N, int(bool(transposed)), planes.data_ptr(),
                                            _stream()), "split2_planes")
    return planes


def set_gemm_h2p(on):
    """f16x2 mode: True (default) -- LayerNorm / GELU write their rows as f16x2 lines and the GEMMs stage both operands by LDS-DMA
    (``csrc/gemm_h2p.hip``); False -- the register-staged ``gemm_h2`` kernels on fp32 activations.  Same bits either way.
    Returns the previous setting."""
    return bool(_lib.load().r4d_set_gemm_h2p(1 if on else 0))


def split2_lines(x):
    """fp32 rows [..., K] -> their f16x2 lines, int16 [rows, K/32, 2, 32] (fp16 bit patterns of x/4: ``[:, :, 0]`` hi, ``[:, :, 1]`` lo'):
    the A operand of :func:`conv1d_h2p` (what the LayerNorm kernels and the c_fc epilogue write in f16x2 mode)."""
    K = x.shape[-1]
    rows = x.numel() // K
    out = torch.empty(rows, K // 32, 2, 32, dtype=torch.int16, device=x.device)
    check(_lib.load().r4d_split2_lines_f16(_dev(x, torch.float32, "x"), rows, K, out.data_ptr(), _stream()), "split2_lines")
    return out


def layernorm_lines(x, w, b, eps=1e-5):
    """:func:`layernorm` whose output rows are f16x2 lines [rows, d/32, 2, 32] (d % 256 == 0)."""
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty(rows, d // 32, 2, 32, dtype=torch.int16, device=x.device)
    check(_lib.load().r4d_layernorm_lines_f32(_dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"), _dev(b, torch.float32, "b"),
                                              rows, d, eps, y.data_ptr(), _stream()), "layernorm_lines")
    return y


def conv1d_h2p(x_lines, planes, bias, epilogue="none", residual=None, out_lines=False):
    """:func:`conv1d_h2` with the input given as f16x2 lines (:func:`split2_lines`), both operands staged by LDS-DMA; bit-identical
    results.  ``out_lines`` (gelu only): the result as lines [M, N/32, 2, 32] instead of fp32 [M, N]."""
    N, K = planes.shape[0], planes.shape[1] * 32
    M = x_lines.shape[0]
    epi = {"none": 0, "gelu": 1, "residual": 2}[epilogue]
    y = (torch.empty(M, N // 32, 2, 32, dtype=torch.int16, device=x_lines.device) if out_lines
         else torch.empty(M, N, dtype=torch.float32, device=x_lines.device))
    rp = _dev(residual, torch.float32, "residual") if residual is not None else None
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    check(_lib.load().r4d_conv1d_h2p_f32(_dev(x_lines, torch.int16, "x_lines"), _dev(planes, torch.int16, "planes"), bp, rp, M, K, N, epi,
                                         int(bool(out_lines)), y.data_ptr(), _stream()), "conv1d_h2p")
    return y


def conv1d_h2(x, planes, bias, epilogue="none", residual=None):
    """:func:`conv1d` on the fp16 matrix cores at fp32 accuracy (two fp16 terms per operand, three partial products, two fp32
    accumulator sets); ``planes`` from :func:`split2_planes`.  |x| < 2^18."""
    N, K = planes.shape[0], planes.shape[1] * 32
    M = x.numel() // K
    y = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    epi = {"none": 0, "gelu": 1, "residual": 2}[epilogue]
    rp = _dev(residual, torch.float32, "residual") if residual is not None else None
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    check(_lib.load().r4d_conv1d_h2_f32(_dev(x, torch.float32, "x"), _dev(planes, torch.int16, "planes"), bp, rp, M, K, N, epi,
                                        y.data_ptr(), _stream()), "conv1d_h2")
    return y


def split3_planes(w, transposed=False):
    """Static Conv1D weight [K,N] (``transposed``: an [N,K] copy) -> its three k-contiguous bf16 planes (hi, mid, lo),
    a uint16 tensor [3,N,K] (torch's bfloat16 bit patterns): the operand format of :func:`conv1d_s3`."""
    if transposed:
        N, K = w.shape
    else:
        K, N = w.shape
    planes = torch.empty(3, N, K, dtype=torch.int16, device=w.device)
    check(_lib.load().r4d_split3_planes_bf16(_dev(w, torch.float32, "w"), K, N, int(bool(transposed)), planes.data_ptr(),
                                             _stream()), "split3_planes")
    return planes


def fold_layernorm(wT, ln_w, ln_b):
    """Decode-only copy of a projection that reads a LayerNorm: ``wT`` [N,K] (k-contiguous weight), LayerNorm gain / shift [K]
    -> (``wTg`` [N,K] = gain * wT, ``lnc`` [2,N] = (sum_k gain W, sum_k shift W)): LN(x) W = rstd (x wTg^T - mean c1) + c2."""
    N, K = wT.shape
    wTg = torch.empty_like(wT)
    lnc = torch.empty(2, N, dtype=torch.float32, device=wT.device)
    check(_lib.load().r4d_fold_layernorm_f32(_dev(wT, torch.float32, "wT"), _dev(ln_w, torch.float32, "ln_w"),
                                             _dev(ln_b, torch.float32, "ln_b"), N, K, wTg.data_ptr(), lnc.data_ptr(), _stream()),
          "fold_layernorm")
    return wTg, lnc


def conv1d_skinny_workspace(K, N):
    """Bytes of the workspace :func:`conv1d_skinny` needs for a [N,K] weight (0 where the kernels do not serve K or N)."""
    return int(_lib.load().r4d_conv1d_skinny_workspace_bytes(int(K), int(N)))


def conv1d_skinny(x, wT, bias=None, epilogue="none", residual=None, ln=None, ln_fold=None, eps=1e-5, counters_zeroed=False,
                  out=None, ws=None):
    """The decode step's weight-stream GEMM alone (``csrc/gemm_skinny.hip``): y = epilogue(x' @ wT^T + bias) for 1 .. 32 rows ``x``
    [M,K], ``wT`` [N,K], K a multiple of 256.  ``ln`` = (gain, shift): x' = LayerNorm(x), formed in the launch; ``ln_fold`` = the
    ``lnc`` of :func:`fold_layernorm`, ``wT`` then being its ``wTg`` (both K = 512 or 768 only).  ``out``: a float32 tensor whose first
    M * N elements receive y (it may be ``residual``); ``ws``: a uint8 workspace of :func:`conv1d_skinny_workspace` bytes whose first
    1024 bytes the caller has zeroed if ``counters_zeroed``.  Both are allocated here when None."""
    N, K = wT.shape
    M = x.numel() // K
    epi = {"none": 0, "gelu": 1, "residual": 2}[epilogue]
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    elif out.numel() < M * N:
        raise _lib.R4DError(f"conv1d_skinny: out holds {out.numel()} elements, fewer than M * N = {M * N}")
    if ws is None:
        ws = workspace(conv1d_skinny_workspace(K, N), x.device, "conv1d_skinny")
        counters_zeroed = False
    rp = _dev(residual, torch.float32, "residual") if residual is not None else None
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    gp, sp = (_dev(ln[0], torch.float32, "ln gain"), _dev(ln[1], torch.float32, "ln shift")) if ln is not None else (None, None)
    fp = _dev(ln_fold, torch.float32, "ln_fold") if ln_fold is not None else None
    check(_lib.load().r4d_conv1d_skinny_f32(_dev(x, torch.float32, "x"), _dev(wT, torch.float32, "wT"), bp, rp, M, K, N, epi, gp, sp,
                                            eps, fp, int(bool(counters_zeroed)), _dev(out, torch.float32, "out"),
                                            _dev(ws, torch.uint8, "ws"), ws.numel(), _stream()), "conv1d_skinny")
    return out


def conv1d_s3(x, planes, bias, epilogue="none", residual=None):
    """:func:`conv1d` on the bf16 matrix cores at fp32 accuracy (three-way bf16 split of both operands, six partial
    products, fp32 accumulation); ``planes`` from :func:`split3_planes`."""
    _, N, K = planes.shape
    M = x.numel() // K
    y = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    epi = {"none": 0, "gelu": 1, "residual": 2}[epilogue]
    rp = _dev(residual, torch.float32, "residual") if residual is not None else None
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    check(_lib.load().r4d_conv1d_s3_f32(_dev(x, torch.float32, "x"), _dev(planes, torch.int16, "planes"), bp, rp, M, K, N, epi,
                                        y.data_ptr(), _stream()), "conv1d_s3")
    return y


_ENCODE_PRECISIONS = {"fp32": (0, 0), "bf16": (1, 0), "bf16+attn": (1, 1)}     # word -> (r4d_set_encode_bf16, r4d_set_encode_attention_bf16)
_ENCODE_PRECISION = None


def resolve_encode_precision(precision=None):
    """``"fp32"``, ``"bf16"`` or ``"bf16+attn"``.  None -> the environment variable ``R4D_ENCODE_PRECISION``, ``fp32`` when it is unset or empty.
    Anything else raises."""
    if precision is None:
        import os
        precision = os.environ.get("R4D_ENCODE_PRECISION") or "fp32"
    if precision not in _ENCODE_PRECISIONS:
        raise ValueError(f"encode precision {precision!r}: expected one of {sorted(_ENCODE_PRECISIONS)}")
    return precision


def encode_precision():
    """Arithmetic of the encoder FORWARD GEMMs (``encode``, ``encode_groups*``, ``prefill``, ``prefill_last``, ``forward()``,
    ``retrieval.encode_batches``): ``"fp32"`` (default) -- the fp32-accurate arithmetic :func:`gemm_mode` names; ``"bf16"`` -- both
    operands rounded to bf16, one matrix-core product per fp32 product (``csrc/gemm_b1.hip``).  "bf16" is NOT fp32-accurate
    (DESIGN.md 7): retrieval under it is approximate, and greedy decoding prefills in bf16 while the cached step stays fp32.
    ``"bf16+attn"`` -- the "bf16" arithmetic with the encoder's attention on bf16 operands as well (``csrc/attention_b1.hip``: q, k,
    v and the unnormalised probabilities rounded to bf16, one matrix-core product per product, fp32 softmax and accumulation;
    q | k | v and the attention output travel as bf16 between their producers and consumers); where that kernel does not serve a
    shape the block takes the "bf16" route.
    ``R4D_ENCODE_PRECISION=bf16`` (read once, at the first call) or :func:`set_encode_precision` select it.  Process-wide: the
    ranks of a sharded job must agree.  (The first call also resolves :func:`encode_act_store`, which applies to the same entries.)"""
    if _ENCODE_PRECISION is None:
        set_encode_precision(resolve_encode_precision())
    if _ENCODE_ACT_STORE is None:
        encode_act_store()
    return _ENCODE_PRECISION


def set_encode_precision(precision):
    """Select :func:`encode_precision` ("fp32" | "bf16" | "bf16+attn"; anything else raises ValueError and changes nothing).
    Returns the previous setting."""
    global _ENCODE_PRECISION
    if precision not in _ENCODE_PRECISIONS:
        raise ValueError(f"encode precision {precision!r}: expected one of {sorted(_ENCODE_PRECISIONS)}")
    prev = _ENCODE_PRECISION if _ENCODE_PRECISION is not None else resolve_encode_precision()
    gemms, attn = _ENCODE_PRECISIONS[precision]
    _lib.load().r4d_set_encode_bf16(gemms)
    _lib.load().r4d_set_encode_attention_bf16(attn)
    _ENCODE_PRECISION = precision
    return prev


_ENCODE_ACT_STORES = {"fp32": 0, "bf16": 1}                                     # word -> r4d_set_encode_act_bf16
_ENCODE_ACT_STORE = None


def resolve_encode_act_store(store=None):
    """``"fp32"`` or ``"bf16"``.  None -> the environment variable ``R4D_ENCODE_ACT_STORE``, ``fp32`` when it is unset or empty.
    Anything else raises."""
    if store is None:
        import os
        store = os.environ.get("R4D_ENCODE_ACT_STORE") or "fp32"
    if store not in _ENCODE_ACT_STORES:
        raise ValueError(f"encode activation store {store!r}: expected one of {sorted(_ENCODE_ACT_STORES)}")
    return store


def encode_act_store():
    """How the encoder FORWARD under ``encode_precision()`` "bf16" / "bf16+attn" keeps a block's ln1, ln2 and GELU output between
    producer and consumer: ``"fp32"`` (default) -- fp32 rows that the bf16 GEMM rounds while staging; ``"bf16"`` -- rounded once where
    they are produced and stored as bf16 rows the GEMM reads as they are (``r4d_set_encode_act_bf16``): half the bytes, the SAME
    output bits.  Per buffer, where its GEMMs run on the bf16 kernel and n_embd % 256 == 0; elsewhere that buffer stays fp32.
    Applies exactly where the precision word applies and does nothing under ``"fp32"`` precision.
    ``R4D_ENCODE_ACT_STORE=bf16`` (read once, at the first call) or :func:`set_encode_act_store` select it.  Process-wide."""
    if _ENCODE_ACT_STORE is None:
        set_encode_act_store(resolve_encode_act_store())
    return _ENCODE_ACT_STORE


def set_encode_act_store(store):
    """Select :func:`encode_act_store` ("fp32" | "bf16"; anything else raises ValueError and changes nothing).  Returns the
    previous setting."""
    global _ENCODE_ACT_STORE
    if store not in _ENCODE_ACT_STORES:
        raise ValueError(f"encode activation store {store!r}: expected one of {sorted(_ENCODE_ACT_STORES)}")
    prev = _ENCODE_ACT_STORE if _ENCODE_ACT_STORE is not None else resolve_encode_act_store()
    _lib.load().r4d_set_encode_act_bf16(_ENCODE_ACT_STORES[store])
    _ENCODE_ACT_STORE = store
    return prev


def bf16_plane(w, transposed=False):
    """Static Conv1D weight [K,N] (``transposed``: an [N,K] copy) -> its round-to-nearest-even bf16 image as ONE k-contiguous
    plane, an int16 tensor [N,K] (torch's bfloat16 bit patterns of ``w.t()``): plane 0 of :func:`split3_planes`, the weight
    operand of :func:`conv1d_bf16`."""
    return split3_planes(w, transposed)[0].clone()


def conv1d_bf16(x, w_bf16, bias, epilogue="none", residual=None):
    """y = epilogue(bf16(x) @ bf16(W) + bias) with ONE bf16 matrix-core product per fp32 product and fp32 accumulation: NOT
    fp32-accurate (8 significant bits per operand).  ``w_bf16`` from :func:`bf16_plane`; K % 32 == 0.  The kernel the encoder
    runs under ``encode_precision() == "bf16"``."""
    N, K = w_bf16.shape
    M = x.numel() // K
    y = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    epi = {"none": 0, "gelu": 1, "residual": 2}[epilogue]
    rp = _dev(residual, torch.float32, "residual") if residual is not None else None
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    check(_lib.load().r4d_conv1d_bf16_f32(_dev(x, torch.float32, "x"), _dev(w_bf16, torch.int16, "w_bf16"), bp, rp, M, K, N, epi,
                                          y.data_ptr(), _stream()), "conv1d_bf16")
    return y


def attention_bf16(qkv, groups, n_head, out_bf16=None):
    """The encoder attention of ``encode_precision() == "bf16+attn"`` alone (``r4d_attention_bf16_groups``; NOT fp32-accurate) over
    ``groups`` = [(B, T), ...] (at most 16) in ONE launch: batch g's B * T token rows follow batch g - 1's in ``qkv`` [rows, 3d]
    (torch.float32, or torch.bfloat16 as c_attn writes it under the word) -> [rows, d] merged heads, torch.bfloat16 when
    ``out_bf16`` (default: as ``qkv``), else torch.float32.  head_dim = d / n_head a multiple of 16 in 16 .. 256, T <= 1024."""
    if not qkv.is_cuda or qkv.dtype not in (torch.float32, torch.bfloat16) or not qkv.is_contiguous() or qkv.dim() != 2:
        raise _lib.R4DError("attention_bf16: qkv must be a contiguous 2-D fp32 or bf16 device tensor [rows, 3d]")
    in_bf16 = qkv.dtype == torch.bfloat16
    out_bf16 = in_bf16 if out_bf16 is None else bool(out_bf16)
    rows, d3 = qkv.shape
    d = d3 // 3
    n = len(groups)
    if n < 1 or d3 % 3 or sum(int(B) * int(T) for B, T in groups) != rows or any(int(B) < 1 or int(T) < 1 for B, T in groups):
        raise _lib.R4DError(f"attention_bf16: groups {list(groups)} do not tile the {rows} rows of qkv [rows, 3d]")
    Bs = (ctypes.c_int32 * n)(*[int(B) for B, _ in groups])
    Ts = (ctypes.c_int32 * n)(*[int(T) for _, T in groups])
    r0, acc = [], 0
    for B, T in groups:
        r0.append(acc)
        acc += int(B) * int(T)
    row0s = (ctypes.c_int64 * n)(*r0)
    out = torch.empty(rows, d, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=qkv.device)
    check(_lib.load().r4d_attention_bf16_groups(qkv.data_ptr(), int(in_bf16), n, Bs, Ts, row0s, int(n_head), d, out.data_ptr(), int(out_bf16),
                                                _stream()), "attention_bf16")
    return out


def conv1d_bf16_keep(x, w_bf16, bias):
    """The c_fc forward of the training steps' "bf16" precision (``training.resolve_train_precision``): -> (pre, y) with pre =
    bf16(x) @ bf16(W) + bias (the pre-activation the backward keeps) and y = gelu_new(pre), one launch.  NOT fp32-accurate."""
    N, K = w_bf16.shape
    M = x.numel() // K
    pre = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    y = torch.empty_like(pre)
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    check(_lib.load().r4d_conv1d_bf16_keep_f32(_dev(x, torch.float32, "x"), _dev(w_bf16, torch.int16, "w_bf16"), bp, M, K, N,
                                               pre.data_ptr(), y.data_ptr(), _stream()), "conv1d_bf16_keep")
    return pre, y


def conv1d_bf16_dgrad(dy, wt_bf16, kind="none", second=None):
    """The Conv1D data gradient of the "bf16" training precision: dx = bf16(dy) @ bf16(W)^T for a weight W [in, out] given as
    ``wt_bf16`` = ``bf16_plane(W.t().contiguous())`` ([in, out], out contiguous: plane 0 of the trainers' ``_w3t`` sets).
    ``kind``: "none"; "residual" (dx = second + ...); "gelu_grad" (dx = (...) * gelu_new'(second)); ``second`` [M, in]."""
    n_in, n_out = wt_bf16.shape
    M = dy.numel() // n_out
    dx = torch.empty(dy.shape[:-1] + (n_in,), dtype=torch.float32, device=dy.device)
    k = {"none": 0, "residual": 1, "gelu_grad": 2}[kind]
    sp = _dev(second, torch.float32, "second") if second is not None else None
    check(_lib.load().r4d_conv1d_bf16_dgrad_f32(_dev(dy, torch.float32, "dy"), _dev(wt_bf16, torch.int16, "wt_bf16"), M, n_in, n_out, k,
                                                sp, dx.data_ptr(), _stream()), "conv1d_bf16_dgrad")
    return dx


def weight_grad_bf16(x, dy, want_db=True, workspace=None):
    """The Conv1D weight gradient of the "bf16" training precision: -> (dW [in, out] = bf16(x)^T @ bf16(dy), db [out] = the fp32
    column sums of the unrounded dy, or None).  ``x`` [rows, in] and ``dy`` [rows, out] may be column blocks of wider buffers
    (row stride >= width, element stride 1).  in % 128 == 0, out % 256 == 0, rows >= 32, else R4DError.  ``workspace``: a uint8
    tensor of at least ``r4d_weight_grad_bf16_workspace_bytes`` (default: a fresh one)."""
    lib = _lib.load()
    for t, n in ((x, "x"), (dy, "dy")):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise R4DError(f"weight_grad_bf16: {n} must be a 2-D fp32 device tensor with contiguous rows")
    rows, n_in = x.shape
    n_out = dy.shape[1]
    if dy.shape[0] != rows:
        raise R4DError("weight_grad_bf16: x and dy differ in rows")
    nbytes = lib.r4d_weight_grad_bf16_workspace_bytes(rows, n_in, n_out)
    if workspace is None:
        workspace = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=x.device)
    dw = torch.empty(n_in, n_out, dtype=torch.float32, device=x.device)
    db = torch.empty(n_out, dtype=torch.float32, device=x.device) if want_db else None
    check(lib.r4d_weight_grad_bf16_f32(x.data_ptr(), int(x.stride(0)), dy.data_ptr(), int(dy.stride(0)), rows, n_in, n_out, dw.data_ptr(),
                                       db.data_ptr() if want_db else None, workspace.data_ptr(), workspace.numel(), _stream()),
          "weight_grad_bf16")
    return dw, db


# ---- the single ops of the bf16 activation store (``training.resolve_train_act_store``, ``r4d_set_train_act_bf16``): the kernels the
# step launches where a saved activation is bf16 in memory.  bf16 tensors are torch.bfloat16 [rows, width], contiguous.
def layernorm_bf16(x, w, b, eps=1e-5):
    """:func:`layernorm` whose output is torch.bfloat16 [..., d]: the same statistics and arithmetic, rounded to nearest even at
    the store (d % 256 == 0)."""
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(_lib.load().r4d_layernorm_bf16_f32(_dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"), _dev(b, torch.float32, "b"),
                                             rows, d, eps, y.data_ptr(), _stream()), "layernorm_bf16")
    return y


def conv1d_bf16_act(x_bf16, w_bf16, bias, epilogue="none", residual=None):
    """:func:`conv1d_bf16` / :func:`conv1d_bf16_keep` on an activation that is ALREADY bf16 in memory (``x_bf16`` torch.bfloat16
    [M, K]): the same operand bits, so the same result bits as on the fp32 activation it was rounded from.  ``epilogue``: "none" ->
    y fp32; "residual" -> y = residual + ...; "gelu_keep" -> (pre fp32, y torch.bfloat16 = RN(gelu_new(pre))); the encoder's
    (:func:`encode_act_store`) "gelu" -> y torch.bfloat16 = RN(gelu_new(v)), no pre-activation kept; "none_bf16" -> y torch.bfloat16 = RN(v)."""
    N, K = w_bf16.shape
    M = x_bf16.numel() // K
    kind = {"none": 0, "residual": 1, "gelu_keep": 2, "gelu": 3, "none_bf16": 4}[epilogue]
    dev = x_bf16.device
    y = torch.empty(x_bf16.shape[:-1] + (N,), dtype=torch.bfloat16 if kind >= 2 else torch.float32, device=dev)
    second = None
    if kind == 1:
        second = residual
        _dev(residual, torch.float32, "residual")
    elif kind == 2:
        second = torch.empty(x_bf16.shape[:-1] + (N,), dtype=torch.float32, device=dev)
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    check(_lib.load().r4d_conv1d_bf16_act_f32(_dev(x_bf16, torch.bfloat16, "x_bf16"), _dev(w_bf16, torch.int16, "w_bf16"), bp, M, K, N, kind,
                                              second.data_ptr() if second is not None else None, y.data_ptr(), _stream()),
          "conv1d_bf16_act")
    return (second, y) if kind == 2 else y


def weight_grad_bf16_act(x_bf16, dy, want_db=True, workspace=None):
    """:func:`weight_grad_bf16` on an ``x_bf16`` that is ALREADY bf16 in memory (torch.bfloat16 [rows, in], or a column block of a
    wider bf16 buffer with a row stride that is a multiple of 8); ``dy`` stays fp32.  The same bits as on the fp32 x it was
    rounded from."""
    lib = _lib.load()
    if not x_bf16.is_cuda or x_bf16.dtype != torch.bfloat16 or x_bf16.dim() != 2 or x_bf16.stride(1) != 1:
        raise R4DError("weight_grad_bf16_act: x must be a 2-D bfloat16 device tensor with contiguous rows")
    if not dy.is_cuda or dy.dtype != torch.float32 or dy.dim() != 2 or dy.stride(1) != 1:
        raise R4DError("weight_grad_bf16_act: dy must be a 2-D fp32 device tensor with contiguous rows")
    rows, n_in = x_bf16.shape
    n_out = dy.shape[1]
    if dy.shape[0] != rows:
        raise R4DError("weight_grad_bf16_act: x and dy differ in rows")
    nbytes = lib.r4d_weight_grad_bf16_workspace_bytes(rows, n_in, n_out)
    if workspace is None:
        workspace = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dy.device)
    dw = torch.empty(n_in, n_out, dtype=torch.float32, device=dy.device)
    db = torch.empty(n_out, dtype=torch.float32, device=dy.device) if want_db else None
    check(lib.r4d_weight_grad_bf16_act_f32(x_bf16.data_ptr(), int(x_bf16.stride(0)), dy.data_ptr(), int(dy.stride(0)), rows, n_in, n_out,
                                           dw.data_ptr(), db.data_ptr() if want_db else None, workspace.data_ptr(), workspace.numel(),
                                           _stream()), "weight_grad_bf16_act")
    return dw, db


TRAIN_ATTN_PRODUCTS =("s", "pv", "dp", "dq", "dk", "dv")


def train_attn_probs_ld(T):
    """Row stride (floats) of a P-shaped block [B*H, T, ld] of the training steps: T rounded up to 128."""
    return int(_lib.load().r4d_train_attn_probs_ld(int(T)))


def train_attn_product_bf16(which, a, b, c, B, T, H, d):
    """ONE of the six per-head attention products of the ``+attn`` training precisions (``r4d_train_attn_product_bf16_f32``;
    ``which``: a name of ``TRAIN_ATTN_PRODUCTS`` or its index) over a [B, T] batch with H heads of d / H columns.  ``a`` / ``b`` /
    ``c``: fp32 device tensors whose FIRST element is the (sequence 0, head 0) element of the operand in the step's layout (a Q / K / V
    slice view of [B, T, 3d], merged heads [B, T, d], or a P-shaped block [B*H, T, ``train_attn_probs_ld(T)``]); ``c`` is written in
    place (its [T, N] block per (sequence, head) only) and returned."""
    idx = TRAIN_ATTN_PRODUCTS.index(which) if isinstance(which, str) else int(which)
    for t, n in ((a, "a"), (b, "b"), (c, "c")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise R4DError(f"train_attn_product_bf16: {n} must be an fp32 device tensor")
    check(_lib.load().r4d_train_attn_product_bf16_f32(idx, a.data_ptr(), b.data_ptr(), c.data_ptr(), int(B), int(T), int(H), int(d),
                                                      _stream()), "train_attn_product_bf16")
    return c


def _attn_dropout_struct(dropout):
    """None, or (attn_p, seed, step) -> the r4d_train_dropout the fused single ops read (attn_p, seed and step only)"""
    if dropout is None:
        return None
    p, seed, step = dropout
    return _lib.TrainDropoutC(0.0, float(p), 0.0, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1))


def train_attn_fused_fwd(qkv, B, T, H, d, att=None, lse=None, dropout=None, site=0, index_base=0):
    """The fused attention forward of ``attention_kernel="fused"`` (``r4d_train_attn_fused_fwd_f32``) over ONE [B, T] batch with H heads:
    ``qkv`` [B, T, 3d] fp32 -> (``att`` [B, T, d] merged heads, ``lse`` [B*H, T]: one log-sum-exp per (sequence, head, query)); no
    [T, T] block is formed in memory.  ``att`` / ``lse``: optional fp32 device tensors written in place from their FIRST element on
    (only the T rows' own-head columns); ``dropout``: None or (attn_p, seed, step) -- the mask of element (bh, i, j) is
    ``r4d_dropout_f32``'s at ``site`` and ``index_base + (bh * T + i) * train_attn_probs_ld(T) + j``."""
    if att is None:
        att = torch.empty(B, T, d, dtype=torch.float32, device=qkv.device)
    if lse is None:
        lse = torch.empty(B * H, T, dtype=torch.float32, device=qkv.device)
    for t, n in ((qkv, "qkv"), (att, "att"), (lse, "lse")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.R4DError(f"train_attn_fused_fwd: {n} must be an fp32 device tensor")
    ds = _attn_dropout_struct(dropout)
    check(_lib.load().r4d_train_attn_fused_fwd_f32(qkv.data_ptr(), int(B), int(T), int(H), int(d), att.data_ptr(), lse.data_ptr(),
                                                   ctypes.byref(ds) if ds is not None else None, int(site), int(index_base), _stream()),
          "train_attn_fused_fwd")
    return att, lse


def train_attn_fused_bwd(qkv, att, lse, dao, B, T, H, d, dqkv=None, dropout=None, site=0, index_base=0, workspace=None):
    """The fused attention backward (``r4d_train_attn_fused_bwd_f32``): ``dao`` [B, T, d] (gradient of ``att``) -> ``dqkv`` [B, T, 3d],
    from ``qkv``, the forward's ``att`` and ``lse``; three launches (row sums, dK / dV, dQ), P formed again in registers.  ``dqkv``:
    optional fp32 device tensor written in place (only the T rows' own-head columns); ``workspace``: optional uint8 device tensor of
    at least ``r4d_train_attn_fused_bwd_workspace_bytes`` bytes (written before it is read); ``dropout`` as in the forward."""
    lib = _lib.load()
    if dqkv is None:
        dqkv = torch.empty(B, T, 3 * d, dtype=torch.float32, device=qkv.device)
    for t, n in ((qkv, "qkv"), (att, "att"), (lse, "lse"), (dao, "dao"), (dqkv, "dqkv")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.R4DError(f"train_attn_fused_bwd: {n} must be an fp32 device tensor")
    if workspace is None:
        workspace = torch.empty(max(int(lib.r4d_train_attn_fused_bwd_workspace_bytes(int(B), int(T), int(H), int(d))), 256),
                                dtype=torch.uint8, device=qkv.device)
    ds = _attn_dropout_struct(dropout)
    check(lib.r4d_train_attn_fused_bwd_f32(qkv.data_ptr(), att.data_ptr(), lse.data_ptr(), dao.data_ptr(), int(B), int(T), int(H), int(d),
                                           dqkv.data_ptr(), ctypes.byref(ds) if ds is not None else None, int(site), int(index_base),
                                           workspace.data_ptr(), workspace.numel(), _stream()), "train_attn_fused_bwd")
    return dqkv


def set_attention_fused(mode):
    """-1 / None: auto by head_dim (default); True: fused flash-style kernel; False: three-launch GEMM form."""
    _lib.load().r4d_set_attention_fused(-1 if mode is None or mode == -1 else (2 if mode == 2 else int(bool(mode))))


def set_attention_h2(on):
    """In gemm mode "f16x2": head_dim 32 / 64 / 96 / 128 / 256 attention of the encoder on the fp16 matrix cores (csrc/attention_h2.hip; default
    on).  Off: the exact-f32 attention kernels in every mode.  Returns the previous setting.  Process-wide: ranks must agree."""
    return bool(_lib.load().r4d_set_attention_h2(int(bool(on))))


def set_attention_kblk(on):
    """f16x2 attention: K read from the key-blocked image the c_attn GEMM writes (whole cache lines per load
    instruction; default on) or from row-major K words.  Same bits either way.  Returns the previous setting."""
    return bool(_lib.load().r4d_set_attention_kblk(int(bool(on))))


def set_layer0_pad_rows(on):
    """f16x2 encoder: the layer-0 c_attn GEMM skips the 32-row blocks that hold one repeated token (the right padding) and a
    copy fills them from a per-call table of (token, position) rows (default on; ``R4D_LAYER0_PAD_ROWS=0`` in the environment
    switches it off).  Same bits either way.  Returns the previous setting.  Process-wide."""
    return bool(_lib.load().r4d_set_layer0_pad_rows(int(bool(on))))


def pack_kblk_words(qkv_words, n_head):
    """Row-major qkv words [B, T, 3d] -> the key-blocked K image (``include/r4d.h``) as a flat int32 tensor."""
    B, T, d3 = qkv_words.shape
    d = d3 // 3
    rows = B * T
    out = torch.empty((rows + 31) // 32 * 32 * d, dtype=torch.int32, device=qkv_words.device)
    check(_lib.load().r4d_pack_kblk_words(_dev(qkv_words, torch.int32, "qkv_words"), rows, n_head, d, out.data_ptr(), _stream()), "pack_kblk_words")
    return out


def attention_h2_kblk(qkv_words, kblk, n_head):
    """:func:`attention_h2` with K taken from ``kblk`` = :func:`pack_kblk_words`."""
    B, T, d3 = qkv_words.shape
    d = d3 // 3
    a = torch.empty(B, T, d, dtype=torch.float32, device=qkv_words.device)
    check(_lib.load().r4d_attention_h2_kblk_f32(_dev(qkv_words, torch.int32, "qkv_words"), _dev(kblk, torch.int32, "kblk"), B, T, n_head, d,
                                                a.data_ptr(), _stream()), "attention_h2_kblk")
    return a


def pack_h2_words(x):
    """fp32 tensor -> its "h2 words" (int32 tensor of the same shape: fp16 hi | fp16 lo' << 16 of value / 4), the operand format of
    :func:`attention_h2` -- what the f16x2 c_attn GEMM writes inside the encoder."""
    x = x.contiguous()
    w = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    check(_lib.load().r4d_pack_h2_words_f32(_dev(x, torch.float32, "x"), x.numel(), w.data_ptr(), _stream()), "pack_h2_words")
    return w


def attention_h2(qkv_words, n_head):
    """:func:`attention` on the fp16 matrix cores at fp32 accuracy: ``qkv_words`` = :func:`pack_h2_words` of the packed c_attn
    output [B,T,3d]; head_dim 32 / 64 / 96 / 128 / 256."""
    B, T, d3 = qkv_words.shape
    d = d3 // 3
    a = torch.empty(B, T, d, dtype=torch.float32, device=qkv_words.device)
    check(_lib.load().r4d_attention_h2_f32(_dev(qkv_words, torch.int32, "qkv_words"), B, T, n_head, d, a.data_ptr(), _stream()),
          "attention_h2")
    return a


def attention(qkv, n_head):
    """Causal MHA over packed c_attn output [B,T,3d] -> [B,T,d] (modeling_gpt2.py:140-175)."""
    B, T, d3 = qkv.shape
    d = d3 // 3
    lib = _lib.load()
    nbytes = lib.r4d_attention_workspace_bytes(B, n_head, T)
    ws = workspace(nbytes, qkv.device, "attn")
    a = torch.empty(B, T, d, dtype=torch.float32, device=qkv.device)
    check(lib.r4d_attention_f32(_dev(qkv, torch.float32, "qkv"), B, T, n_head, d, a.data_ptr(), ws.data_ptr(),
                                ws.numel(), _stream()), "attention")
    return a


def lm_logits(hidden, wte):
    V, d = wte.shape
    M = hidden.numel() // d
    out = torch.empty(hidden.shape[:-1] + (V,), dtype=torch.float32, device=hidden.device)
    check(_lib.load().r4d_lm_logits_f32(_dev(hidden, torch.float32, "hidden"), _dev(wte, torch.float32, "wte"), M, V, d,
                                        out.data_ptr(), _stream()), "lm_logits")
    return out


def sample_params(device, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=0):
    """The two parameter words of the sampler (``r4d.h``: fparams_d float[4], iparams_d int32[4]) as device tensors."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    i32 = lambda v: v - (1 << 32) if v >= (1 << 31) else v
    f = torch.tensor([float(temperature), float(top_p), float(repetition_penalty), 0.0], dtype=torch.float32).to(device)
    i = torch.tensor([1 if do_sample else 0, int(top_k), i32(lo), i32(hi)], dtype=torch.int32).to(device)
    return f, i


def sample_logits(logits, step, stream, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=0,
                  seen=None, want_keep=False, want_u=False):
    """One sampled (or, ``do_sample=False``, arg-max) token per row of ``logits`` [B, V] (``r4d_sample_logits_f32``): repetition
    penalty over the ids whose bit is set in ``seen`` (int32 [B, ceil(V/32)], updated with the chosen id), temperature, top-k,
    top-p, and the Philox draw of (``seed``, ``stream[b]``, ``step[b]``).  Returns the ids, int64 [B]; with ``want_keep`` /
    ``want_u`` a tuple that also holds the kept-set bitmap (int32 [B, ceil(V/32)]) and the uniforms (float32 [B])."""
    B, V = logits.shape
    dev = logits.device
    if not (temperature > 0 and 0 <= top_p <= 1 and repetition_penalty >= 1 and int(top_k) >= 0):
        raise ValueError("sample_logits: temperature > 0, 0 <= top_p <= 1, repetition_penalty >= 1, top_k >= 0")
    nw = (V + 31) // 32
    if seen is not None and tuple(seen.shape) != (B, nw):
        raise ValueError(f"sample_logits: seen must be int32 [{B}, {nw}]")
    step = step.to(device=dev, dtype=torch.int32).contiguous()
    stream = stream.to(device=dev, dtype=torch.int32).contiguous()
    if step.numel() != B or stream.numel() != B:
        raise ValueError("sample_logits: step and stream hold one value per row")
    fpar, ipar = sample_params(dev, do_sample, temperature, top_k, top_p, repetition_penalty, seed)
    tok = torch.empty(B, dtype=torch.int64, device=dev)
    keep = torch.empty(B, nw, dtype=torch.int32, device=dev) if want_keep else None
    u = torch.empty(B, dtype=torch.float32, device=dev) if want_u else None
    check(_lib.load().r4d_sample_logits_f32(_dev(logits, torch.float32, "logits"), B, V,
                                            _dev(seen, torch.int32, "seen") if seen is not None else None, step.data_ptr(),
                                            stream.data_ptr(), fpar.data_ptr(), ipar.data_ptr(), tok.data_ptr(),
                                            keep.data_ptr() if want_keep else None, u.data_ptr() if want_u else None, _stream()),
          "sample_logits")
    if not (want_keep or want_u):
        return tok
    return (tok,) + ((keep,) if want_keep else ()) + ((u,) if want_u else ())


BEAM_MAX = 16


def beam_params(device, length_penalty=1.0, repetition_penalty=1.0):
    """The parameter word of the beam step (``r4d.h``: fparams_d float[4]) as a device tensor."""
    return torch.tensor([float(length_penalty), float(repetition_penalty), 0.0, 0.0], dtype=torch.float32).to(device)


def beam_select(logits, beam_scores, num_beams, repetition_penalty=1.0, seen=None, want_rows=False):
    """The 2n best continuations of every prompt (``r4d_beam_select_f32``): ``logits`` [B0 * n, V] (rows ``b n .. b n + n - 1`` the
    beams of prompt ``b``), ``beam_scores`` [B0 * n]; score = log_softmax(penalised row) + beam score in fp32, order (score descending,
    flat index ``beam * V + id`` ascending).  Returns (scores float32 [B0, 2n], flat indices int32 [B0, 2n]); with ``want_rows`` also
    the rows' own lists (float32 / int32 [B0 * n, 2n], entries past min(2n, V): -inf / -1).  ``seen`` is read, not updated."""
    R, V = logits.shape
    n = int(num_beams)
    dev = logits.device
    if not 2 <= n <= BEAM_MAX or R % n:
        raise ValueError(f"beam_select: 2 <= num_beams <= {BEAM_MAX} and rows in groups of num_beams")
    if V < 2 or n * V >= 1 << 31:
        raise ValueError("beam_select: 2 <= V and num_beams * V < 2^31")
    if repetition_penalty < 1:
        raise ValueError("beam_select: repetition_penalty >= 1")
    nw = (V + 31) // 32
    if seen is not None and tuple(seen.shape) != (R, nw):
        raise ValueError(f"beam_select: seen must be int32 [{R}, {nw}]")
    B0 = R // n
    fpar = beam_params(dev, 1.0, repetition_penalty)
    cs = torch.empty(R, 2 * n, dtype=torch.float32, device=dev)
    ci = torch.empty(R, 2 * n, dtype=torch.int32, device=dev)
    out_s = torch.empty(B0, 2 * n, dtype=torch.float32, device=dev)
    out_i = torch.empty(B0, 2 * n, dtype=torch.int32, device=dev)
    check(_lib.load().r4d_beam_select_f32(_dev(logits, torch.float32, "logits"), _dev(beam_scores, torch.float32, "beam_scores"),
                                          _dev(seen, torch.int32, "seen") if seen is not None else None, fpar.data_ptr(), B0, n, V,
                                          cs.data_ptr(), ci.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), _stream()), "beam_select")
    return (out_s, out_i, cs, ci) if want_rows else (out_s, out_i)


def kv_cache_reorder(kv_cache, src_row, num_beams, lo, hi, active=None):
    """Reorder ``kv_cache`` [n_layer, B0 * n, t_cap, 2d] IN PLACE (``r4d_kv_cache_reorder_f32``): for every group ``b`` (``active[b]``
    != 0) and position in ``[lo[b], hi[b])``, row ``b n + i`` receives the K | V line of row ``src_row[b n + i]``.  This front end
    reads ``src_row`` on the host (one synchronisation) and refuses a source outside its own group; the decode loop calls the entry
    itself, where such a row is poisoned instead."""
    if kv_cache.dim() != 4 or kv_cache.shape[3] % 4:
        raise ValueError("kv_cache_reorder: kv_cache must be [n_layer, rows, t_cap, 2d] with d even")
    L, R, t_cap, d2 = kv_cache.shape
    n = int(num_beams)
    if not 1 <= n <= BEAM_MAX or R % n:
        raise ValueError(f"kv_cache_reorder: 1 <= num_beams <= {BEAM_MAX} and rows in groups of num_beams")
    B0 = R // n
    dev = kv_cache.device
    i32 = lambda t, m, name: _check_len(t.to(device=dev, dtype=torch.int32).contiguous(), m, name)
    src_row, lo, hi = i32(src_row, R, "src_row"), i32(lo, B0, "lo"), i32(hi, B0, "hi")
    active = i32(active, B0, "active") if active is not None else None
    group = torch.arange(R, device=dev, dtype=torch.int32) // n
    if bool(((src_row // n != group) | (src_row < 0)).any()):
        raise ValueError("kv_cache_reorder: a src_row outside its own group")
    check(_lib.load().r4d_kv_cache_reorder_f32(_dev(kv_cache, torch.float32, "kv_cache"), src_row.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                               active.data_ptr() if active is not None else None, L, B0, n, t_cap, d2 // 2, _stream()),
          "kv_cache_reorder")
    return kv_cache


def _check_len(t, m, name):
    if t.numel() != m:
        raise ValueError(f"{name}: expected {m} values, got {t.numel()}")
    return t


# ------------------------------------------------------------------------------------------- range guard (include/r4d.h, ABI v6)
RANGE_NONFINITE_HIDDEN, RANGE_BAD_NORM, RANGE_BAD_LABEL = 1, 2, 4
_RANGE_FLAG = None


def range_flag(device=None):
    """The process's range-guard word (int32 [1] on the GPU), registered with the library on first use (``r4d_set_range_flag``):
    bit 0 = a non-finite row reached ln_f in an ``encode_*`` call (in f16x2 mode: an activation beyond the fp16 range), bit 1 = a
    row that could not be normalised (NaN / inf / zero norm).  Sticky: the library only ORs bits in."""
    global _RANGE_FLAG
    if _RANGE_FLAG is None:
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        _RANGE_FLAG = torch.zeros(1, dtype=torch.int32, device=dev)
        check(_lib.load().r4d_set_range_flag(_RANGE_FLAG.data_ptr()), "set_range_flag")
    return _RANGE_FLAG


def take_range_flag():
    """Read AND clear the range-guard word (one device synchronisation).  0 = every encode / normalise since the last call stayed
    in range."""
    f = range_flag()
    v = int(f.item())
    if v:
        f.zero_()
    return v


def check_range(what):
    """Raise ``R4DError`` if the range-guard word is set (and clear it): the point where results are about to leave the device."""
    v = take_range_flag()
    if v:
        why = []
        if v & RANGE_NONFINITE_HIDDEN:
            why.append("a non-finite hidden state reached ln_f (an activation, q, k or v beyond the arithmetic's range: "
                       "|x| >= 2^18 in gemm mode 'f16x2'; 'bf16x3' and 'f32' have fp32's exponent range)")
        if v & RANGE_BAD_NORM:
            why.append("an embedding row could not be normalised (NaN, inf or zero norm)")
        if v & RANGE_BAD_LABEL:
            why.append("a token id outside [0, vocab) reached the LM cross entropy")
        raise _lib.R4DError(f"{what}: " + "; ".join(why) + " -- no ranking was produced from it")


def normalize_rows(x):
    n, d = x.shape
    range_flag(x.device)
    out = torch.empty_like(x)
    check(_lib.load().r4d_normalize_rows_f32(_dev(x, torch.float32, "x"), n, d, out.data_ptr(), _stream()),
          "normalize_rows")
    return out


SCORE_TOPK_MAX_QUERIES = 65535      # queries per library call (a grid dimension); more are handed over in chunks


def score_topk(q_hat, pool_hat, k, index_offset=0, want_scores=False):
    """(S+1)/2 cosine scan of one pool shard + canonical top-k.  Returns (vals [Q,k], idx int64 [Q,k], scores|None).
    Any number of queries: beyond ``SCORE_TOPK_MAX_QUERIES`` the call is made in chunks (a score does not depend on how the queries
    are batched into calls, so the result is the one call's)."""
    Q, d = q_hat.shape
    if Q > SCORE_TOPK_MAX_QUERIES:
        parts = [score_topk(q_hat[s:s + SCORE_TOPK_MAX_QUERIES].contiguous(), pool_hat, k, index_offset, want_scores)
                 for s in range(0, Q, SCORE_TOPK_MAX_QUERIES)]
        return (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]),
                torch.cat([p[2] for p in parts]) if want_scores else None)
    N = pool_hat.shape[0]
    lib = _lib.load()
    ws = workspace(lib.r4d_score_topk_workspace_bytes(Q, N, k), q_hat.device, "score")
    vals = torch.empty(Q, k, dtype=torch.float32, device=q_hat.device)
    idx = torch.empty(Q, k, dtype=torch.int64, device=q_hat.device)
    scores = torch.empty(Q, N, dtype=torch.float32, device=q_hat.device) if want_scores else None
    check(lib.r4d_score_topk_f32(_dev(q_hat, torch.float32, "q_hat"), _dev(pool_hat, torch.float32, "pool_hat"), Q, N, d,
                                 k, int(index_offset), vals.data_ptr(), idx.data_ptr(),
                                 scores.data_ptr() if want_scores else None, ws.data_ptr(), ws.numel(), _stream()),
          "score_topk")
    return vals, idx, scores


def __getattr__(name):
    # ops.TOPK_MAX_K: the largest k of topk_f32 / score_topk / merge_topk (2048; topk_f64: 64).  Read from the library on first
    # use, so that importing this module does not need the library.
    if name == "TOPK_MAX_K":
        globals()["TOPK_MAX_K"] = int(_lib.load().r4d_topk_max_k())
        return globals()["TOPK_MAX_K"]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def topk_f32(m, k):
    """Canonical per-row top-k of an f32 matrix -> (vals [rows,k], idx int64 [rows,k]); k <= min(TOPK_MAX_K, n).  Values are
    ordered as keys (NaN -> -inf, -0.0 -> +0.0), ties by ascending column; beyond k = 64 the library selects by radix select."""
    rows, n = m.shape
    lib = _lib.load()
    ws = workspace(lib.r4d_topk_f32_workspace_bytes(rows, n, k), m.device, "topk32")
    vals = torch.empty(rows, k, dtype=torch.float32, device=m.device)
    idx = torch.empty(rows, k, dtype=torch.int64, device=m.device)
    check(lib.r4d_topk_f32(_dev(m, torch.float32, "m"), rows, n, k, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                           ws.numel(), _stream()), "topk_f32")
    return vals, idx


def merge_topk(vals, idx):
    """[G,Q,k] per-shard candidates -> [Q,k] global top-k (same canonical order)."""
    G, Q, k = vals.shape
    ov = torch.empty(Q, k, dtype=torch.float32, device=vals.device)
    oi = torch.empty(Q, k, dtype=torch.int64, device=vals.device)
    lib = _lib.load()
    ws = workspace(lib.r4d_merge_topk_workspace_bytes(G, Q, k), vals.device, "merge")
    check(lib.r4d_merge_topk_f32(_dev(vals, torch.float32, "vals"), _dev(idx, torch.int64, "idx"), G, Q, k,
                                 ov.data_ptr(), oi.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "merge_topk")
    return ov, oi


def argsort_desc(scores):
    """Stable argsort of -scores per row (== np.argsort(-S, axis=1, kind='stable')), int32 [rows,n]."""
    rows, n = scores.shape
    perm = torch.empty(rows, n, dtype=torch.int32, device=scores.device)
    lib = _lib.load()
    f64 = scores.dtype == torch.float64
    fn = lib.r4d_argsort_desc_f64 if f64 else lib.r4d_argsort_desc_f32
    ptr = _dev(scores, torch.float64 if f64 else torch.float32, "scores")
    step = 65535                                            # grid.y limit of one launch
    for r0 in range(0, rows, step):
        nr = min(step, rows - r0)
        ws = workspace(lib.r4d_argsort_workspace_bytes(nr, n, 8 if f64 else 4), scores.device, "argsort")
        check(fn(ptr + r0 * n * scores.element_size(), nr, n, perm.data_ptr() + r0 * n * 4, ws.data_ptr(), ws.numel(),
                 _stream()), "argsort_desc")
    return perm


def jaccard(a_ptr, a_idx, b_ptr, b_idx, vocab, zero_diag=False, sort_rows=None, dense_split=None):
    """f64 [na,nb] Jaccard matrix of CSR sets (occurrence_matrix, retrieval_data_annotation.py:36-41).
    ``dense_split``: the 32 most frequent tokens leave the lists for a per-set membership word -- same values, 2-3x fewer token
    steps on the input sets (ego + <|timeK|> + neighbours).  ``sort_rows``: the kernel visits the A rows longest set first --
    same values, fewer padded token steps.  Both are prepared ON THE DEVICE by ``r4d_jaccard_prepared_f64`` (three small HIP
    launches; until round 5 a dozen torch index ops that cost more GPU time than the kernel).
    Defaults: both only where they pay (sets averaging more than 4 tokens and >= 5*10^6 / 5*10^7 pairs; the 1.8-token output
    sets are bound by the division and the store: the extra lookups cost more than they save)."""
    na, nb = a_ptr.numel() - 1, b_ptr.numel() - 1
    out = torch.empty(na, nb, dtype=torch.float64, device=a_ptr.device)
    if a_idx.numel() == 0:                     # contract: idx buffers hold at least one element
        a_idx = torch.zeros(1, dtype=torch.int32, device=a_ptr.device)
    if b_idx.numel() == 0:
        b_idx = torch.zeros(1, dtype=torch.int32, device=b_ptr.device)
    long_sets = a_idx.numel() > 4 * na
    if dense_split is None:
        dense_split = long_sets and na * nb >= 5_000_000
    if sort_rows is None:
        sort_rows = long_sets and na * nb >= 50_000_000      # small problems: the ordering costs what it saves
    lib = _lib.load()
    ws = None
    if dense_split or sort_rows:
        ws = workspace(lib.r4d_jaccard_prepared_workspace_bytes(na, a_idx.numel(), nb, b_idx.numel(), int(vocab)), a_ptr.device,
                       "jaccard")
    check(lib.r4d_jaccard_prepared_f64(_dev(a_ptr, torch.int32, "a_ptr"), _dev(a_idx, torch.int32, "a_idx"), na, a_idx.numel(),
                                       _dev(b_ptr, torch.int32, "b_ptr"), _dev(b_idx, torch.int32, "b_idx"), nb, b_idx.numel(),
                                       int(vocab), int(bool(zero_diag)), int(bool(dense_split)), int(bool(sort_rows)),
                                       out.data_ptr(), ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                       _stream()), "jaccard")
    return out


def topk_f64(m, k):
    rows, n = m.shape
    lib = _lib.load()
    ws = workspace(lib.r4d_topk_f64_workspace_bytes(rows, n, k), m.device, "topk64")
    vals = torch.empty(rows, k, dtype=torch.float64, device=m.device)
    idx = torch.empty(rows, k, dtype=torch.int32, device=m.device)
    check(lib.r4d_topk_f64(_dev(m, torch.float64, "m"), rows, n, k, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                           ws.numel(), _stream()), "topk_f64")
    return vals, idx

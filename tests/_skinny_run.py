"""How tests/test_gpu_skinny_gemm.py and its child tests/_skinny8_child.py call ``ops.conv1d_skinny``: the set-up before every
call (y of 32 rows filled with NaN, a guard behind y and behind the workspace, the workspace poisoned), the checks after it (rows
>= M still NaN, guards unchanged, the dispatch counters exactly those of the intended branch) and the two gates of
tests/_skinny_ref.py.  Needs a GPU; imported by GPU tests only."""
import numpy as np
import torch

import _skinny_ref as R
from _poison import PATTERNS, ZERO, poison

Y_GUARD, WS_GUARD = 1024, 4096              # floats behind y, bytes behind the workspace
Y_MARK, WS_MARK = 12345.0, 0xA5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Runner:
    def __init__(self, dev, skinny16=True):
        from rag4dyg_amd import _lib
        self.dev, self.skinny16, self.lib = dev, skinny16, _lib.load()
        self.total = {}                      # dispatch counter name -> launches, over every call made through this object
        self.records = []                    # (label, kernel form, rho, rho_seq32, hard gate)
        self._cases, self._dev_data, self._folds = {}, {}, {}

    def counters(self):
        lib = self.lib
        return {lib.r4d_dispatch_branch_name(i).decode(): int(lib.r4d_dispatch_branch_hits(i))
                for i in range(lib.r4d_dispatch_num_branches()) if lib.r4d_dispatch_branch_hits(i)}

    def tensors(self, d):
        t = self._dev_data.get(id(d))
        if t is None:
            t = self._dev_data[id(d)] = (d, {k: torch.from_numpy(v).to(self.dev) for k, v in d.items()})
        return t[1]

    def fold(self, d, N):
        from rag4dyg_amd import ops
        key = (id(d), N)
        if key not in self._folds:
            t = self.tensors(d)
            self._folds[key] = ops.fold_layernorm(t["wT"][:N].contiguous(), t["g"], t["beta"])
        return self._folds[key]

    def call(self, d, M, N, epilogue, bias=True, ln=None, inplace=False, pattern=ZERO, zeroed=None, ws=None):
        """One launch.  ``ln``: None, "launch" (ln_w / ln_b), "fold" (pre-folded weight) or "separate" (ops.layernorm, then the entry
        without LayerNorm).  ``ws``: (buffer, bytes) of a workspace that is used as it is; otherwise a fresh one of exactly the
        queried size is poisoned with ``pattern``, its tickets zeroed only if ``zeroed``.  Returns y [M,N] as numpy."""
        from rag4dyg_amd import ops
        t = self.tensors(d)
        K = d["x"].shape[1]
        x, wT = t["x"][:M].contiguous(), t["wT"][:N].contiguous()
        kw = {}
        if ln == "launch":
            kw["ln"] = (t["g"], t["beta"])
        elif ln == "fold":
            wT, kw["ln_fold"] = self.fold(d, N)
        elif ln == "separate":
            x = ops.layernorm(x, t["g"], t["beta"], R.LN_EPS)
        nb = R.workspace_bytes(K, N)
        assert ops.conv1d_skinny_workspace(K, N) == nb
        if ws is None:
            nb_guard = nb
            wsbuf = torch.empty(nb + WS_GUARD, dtype=torch.uint8, device=self.dev)
            poison(wsbuf[:nb], pattern)
            if zeroed:
                wsbuf[:1024] = 0
        else:
            wsbuf, nb_guard = ws
            assert nb_guard >= nb and wsbuf.numel() == nb_guard + WS_GUARD
        wsbuf[nb_guard:] = WS_MARK
        ybuf = torch.full((32 * N + Y_GUARD,), float("nan"), dtype=torch.float32, device=self.dev)
        ybuf[32 * N:] = Y_MARK
        resid = None
        if epilogue == "residual":
            resid = t["resid"][:M, :N].contiguous()
            if inplace:
                ybuf[:M * N] = resid.reshape(-1)
                resid = ybuf[:M * N].view(M, N)
        torch.cuda.synchronize()
        self.lib.r4d_dispatch_reset()
        ops.conv1d_skinny(x, wT, t["bias"][:N].contiguous() if bias else None, epilogue, residual=resid, eps=R.LN_EPS,
                          counters_zeroed=bool(zeroed), out=ybuf[:32 * N], ws=wsbuf[:nb], **kw)
        torch.cuda.synchronize()
        got = self.counters()
        want = R.expected_branches(K, N, ln if ln in ("launch", "fold") else None, self.skinny16)
        assert got == want, f"dispatch counters {got}, meant {want}"
        for n, c in got.items():
            self.total[n] = self.total.get(n, 0) + c
        y = ybuf.cpu().numpy()
        assert np.isnan(y[M * N:32 * N]).all(), "rows >= M of y were written"
        assert (y[32 * N:] == Y_MARK).all(), "the guard behind y was written"
        assert bool((wsbuf[nb_guard:] == WS_MARK).all()), "the guard behind the workspace was written"
        return y[:M * N].reshape(M, N).copy()

    def reference(self, d, M, N, epilogue, bias=True, ln=None):
        """The Case of these inputs: built once, shared by every call that needs it, never changed."""
        key = (id(d), M, N, epilogue, bias, ln is not None)
        if key not in self._cases:
            self._cases[key] = R.Case(d["x"][:M], d["wT"][:N], d["bias"][:N] if bias else None,
                                      np.ascontiguousarray(d["resid"][:M, :N]), epilogue, R.ln_of(d) if ln else None, self.skinny16)
        return self._cases[key]

    def gates(self, label, c, y, ln=None):
        r = c.rho(y)
        kind, ng, KS = R.form(c.K, c.N, self.skinny16)
        formname = kind + (f" ng{ng}" if ng else "") + (f" KS{KS}" if KS > 1 else "") + (f" LayerNorm:{ln}" if ln else "")
        self.records.append((label, formname, r, c.rho_seq32, c.hard))
        print(f"[rho] {label} | {formname} | rho {r:.2f} | rho(seq32) {c.rho_seq32:.2f} | measured gate {c.measured:.1f} | hard gate {c.hard}")
        c.last_rho = r
        assert r <= c.hard, f"{label}: rho {r:.2f} above the derived bound {c.hard}"
        assert r <= c.measured, f"{label}: rho {r:.2f} above 8 x rho(seq32) = {c.measured:.2f}"

    def case(self, d, M, N, epilogue, bias=True, ln=None, inplace=False, patterns=PATTERNS, label=None):
        """The call under every poison pattern (tickets zeroed and promised under ZERO, left poisoned otherwise): the same bits
        each time, and inside both gates.  Returns (Case, y)."""
        K = d["x"].shape[1]
        label = label or f"K{K} M{M} N{N} {epilogue} bias{int(bias)}" + (f" ln:{ln}" if ln else "") + (" in-place" if inplace else "")
        ys = [self.call(d, M, N, epilogue, bias, ln, inplace, p, zeroed=(p == ZERO)) for p in patterns]
        for p, y in zip(patterns[1:], ys[1:]):
            assert np.array_equal(bits(y), bits(ys[0])), f"{label}: the result depends on what the workspace held ({p} vs {patterns[0]})"
        c = self.reference(d, M, N, epilogue, bias, ln)
        self.gates(label, c, ys[0], ln)
        return c, ys[0]

"""Shared reference and metrics of the attention operator tests (plain module, imported by the GPU test files; nothing here needs a GPU to import).

Reference: softmax attention written out in float64 on the SAME bf16-rounded operands the kernel reads -- scores, key mask, softmax, P @ V --
so that torch autograd gives dq / dk / dv of exactly the function the kernels implement.  All kernels work in the log2 domain on a q that
already carries log2(e) / sqrt(head_dim): P = 2^(s - L), L = log2 sum_j 2^(s_j).

Metrics: a global rel-L2 hides one wrong row among thousands (one bad (query, head) row in 4429 x 24 moves it by ~3e-3 in quadrature), so every
tensor is ALSO checked row by row: |got_row - ref_row|_2 <= c * 2^-8 * (|ref_row|_2 + floor), with 2^-8 = one bf16 ulp of a value in [1, 2).
"""
import math

import torch

LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
EPS_BF16 = 2.0 ** -8
SENTINEL = -23.625          # exactly representable in bf16 (0xC1BD) and not a value any of these kernels computes from the test operands
SENTINEL_F32 = -12345.5


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def reference(q, k, v, kv_len=None, d_o=None):
    """q [B, H, S, d] (pre-scaled: scores are in the log2 domain), k, v [B, H, Sk, d]; kv_len int [B] (sample b sees keys < max(1, kv_len[b])).
    d_o [B, H, S, d] or None.  Returns a dict of float64 tensors: o, lse (log2 domain), and with d_o: dq, dk, dv, delta, plus max_abs_score."""
    q64 = q.double().detach().requires_grad_(d_o is not None)
    k64 = k.double().detach().requires_grad_(d_o is not None)
    v64 = v.double().detach().requires_grad_(d_o is not None)
    s = q64 @ k64.transpose(2, 3)                                   # log2 domain
    Sk = k.shape[2]
    if kv_len is not None:
        n = kv_len.to(s.device).clamp(min=1).view(-1, 1, 1, 1)
        dead = torch.arange(Sk, device=s.device).view(1, 1, 1, Sk) >= n
        s = s.masked_fill(dead, float("-inf"))
    p = torch.softmax(s * LN2, dim=-1)                              # 2^(s - L)
    o = p @ v64
    out = {"o": o.detach(), "lse": (torch.logsumexp(s.detach() * LN2, dim=-1) * LOG2E),
           "max_abs_score": float(s.detach()[torch.isfinite(s.detach())].abs().max())}
    if d_o is not None:
        o.backward(d_o.double())
        out.update(dq=q64.grad, dk=k64.grad, dv=v64.grad, delta=(d_o.double() * o.detach()).sum(-1))
        # The flash backward forms Delta_i = rowsum(dO_i * O_i) from the bf16-ROUNDED O: an error e_i ~ 2^-9 |dO_i * O_i|_2 that enters every
        # dZ_ij as P_ij * e_i, so dq_i moves by e_i * sum_j P_ij k_j and dk_j by sum_i e_i P_ij q_i.  Next to a row whose own norm is small
        # (a nearly one-hot softmax: dq_i ~ p (1 - p)) this term dominates; it belongs to the algorithm, not to a kernel, and is added to the
        # row norm the per-row bound is relative to.
        with torch.no_grad():
            pd, e = p.detach(), (d_o.double() * o.detach()).norm(dim=-1)
            out["dq_slack"] = e * (pd @ k64.detach()).norm(dim=-1)
            out["dk_slack"] = ((e * q64.detach().norm(dim=-1)).unsqueeze(-1) * pd).pow(2).sum(dim=2).sqrt()
    return out


def rel_l2(got, ref) -> float:
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def worst_row(got, ref, floor_frac: float = 0.02, slack=None):
    """Largest per-row error in units of 2^-8 * (|ref row|_2 + slack + floor), floor = floor_frac * mean row norm of ref; rows = all but the last
    dim; `slack` = an optional per-row term of the error model (see `reference`).  Returns (worst ratio, flat index of that row).  Non-finite
    values in `got` give inf."""
    got, ref = got.detach().double(), ref.detach().double()
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    if not bool(torch.isfinite(got).all()):
        bad = (~torch.isfinite(got)).any(-1).nonzero()[0]
        return float("inf"), int(bad)
    rn = ref.norm(dim=-1)
    floor = floor_frac * float(rn.mean())
    if slack is not None:
        rn = rn + slack.detach().double().reshape(-1)
    ratio = (got - ref).norm(dim=-1) / (EPS_BF16 * (rn + floor) + 1e-300)
    i = int(ratio.argmax())
    return float(ratio[i]), i


def check_rows(name, got, ref, c: float, rel_bound: float, record=None, floor_frac: float = 0.02, slack=None):
    """Per-row bound (c, in bf16 ulps of the row norm) AND global rel-L2; `record` (a list) collects (name, worst ratio, rel-L2) for the report."""
    w, i = worst_row(got, ref, floor_frac, slack)
    r = rel_l2(got, ref) if math.isfinite(w) else float("inf")
    if slack is not None and math.isfinite(w):      # (a reference that is exactly zero -- one live key: dq = dk = 0 -- leaves only the slack to compare with)
        rn = ref.detach().double().norm(dim=-1).reshape(-1) + slack.detach().double().reshape(-1)
        r = float((got.detach().double() - ref.detach().double()).norm() / (rn.norm() + 1e-300))
    if record is not None:
        record.append((name, w, r))
    assert w <= c, f"{name}: row {i} is off by {w:.2f} x 2^-8 of its norm (bound {c}); global rel-L2 {r:.2e}"
    assert r <= rel_bound, f"{name}: global rel-L2 {r:.3e} > {rel_bound}"
    return w, r


def filled(shape, device, dtype=torch.bfloat16):
    """An output buffer pre-filled with the sentinel: whatever the kernel does not write still holds it afterwards."""
    return torch.full(shape, SENTINEL if dtype == torch.bfloat16 else SENTINEL_F32, device=device, dtype=dtype)


def assert_written(name, t):
    """Every element was overwritten (none still equals the sentinel)."""
    s = SENTINEL if t.dtype == torch.bfloat16 else SENTINEL_F32
    n = int((t == s).sum())
    assert n == 0, f"{name}: {n} of {t.numel()} elements were never written"


def assert_untouched(name, t):
    """No element was written (all still equal the sentinel)."""
    s = SENTINEL if t.dtype == torch.bfloat16 else SENTINEL_F32
    n = int((t != s).sum())
    assert n == 0, f"{name}: {n} of {t.numel()} elements outside the output were written"

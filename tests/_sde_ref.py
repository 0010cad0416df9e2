"""TEST INFRASTRUCTURE ONLY: the reference the fused scheduler step (csrc/sde_step.hip) and its adjoint (sde_step_bwd_kernel, csrc/backward.hip)
are judged by in tests/test_gpu_sde_step_ops.py.

`sde_step` restates the published formulas of the reference's FlowMatchEulerDiscreteSDEScheduler.step (flow_match_euler_discrete.py:305-426)
in plain torch, in the operation order of `oracle/scheduler_ref.py::sde_step`, with these differences:

  * the arithmetic runs in `dtype` (torch.float32: the reference's own precision; torch.float64: the yardstick of the adjoint test).  The
    scalars are taken as the fp32 VALUES the kernel reads and widened, never re-derived in fp64;
  * `sigma`, `sigma_next`, `eta` are per-sample tensors [B] (a number or a one-element tensor broadcasts);
  * it returns next_latents_mean, next_latents, std_dev_t [B], dt [B], log_prob [B] and noise_pred;
  * every operation is differentiable in `v`: `sde_step_bwd` is autograd through it.

`sde_step_bwd` differentiates at the value the kernel consumed: with a CFG pair the leaf is the bf16 op-by-op combine
`oracle.rollout_ref.cfg_combine_bf16(vu, vt, g)`, and d vu = (1 - g) dv, d vt = g dv (the combine's roundings are treated as identity, as
csrc/backward.hip documents).  Output order [uncond | text].

tests/test_sde_ref.py pins this file against `oracle.scheduler_ref.sde_step`, the fixtures of tests/golden/scheduler_steps.npz (written by
the reference's own code) and `_plugin_fakes.oracle_sde_step_bwd` before any kernel is compared with it.
"""
import math

import torch

from oracle import rollout_ref, scheduler_ref

DYNAMICS = scheduler_ref.DYNAMICS


def _per_sample(value, ref: torch.Tensor, dtype) -> torch.Tensor:
    """a number / [1] / [B] fp32 scalar -> (B, 1, ..., 1) in `dtype`, through its fp32 value"""
    t = torch.as_tensor(value, dtype=torch.float32).reshape(-1)
    if t.numel() == 1:
        t = t.expand(ref.shape[0])
    assert t.numel() == ref.shape[0], "per-sample scalars must have one value per sample"
    return t.to(dtype).reshape(-1, *([1] * (ref.dim() - 1)))


def sde_step(v, latents, sigma, sigma_next, eta, dynamics: str, sigma_max: float, noise=None, next_latents=None, compute_log_prob=True,
             dtype=torch.float32):
    """One scheduler step.  `v`: the (CFG-combined) prediction, any float dtype, widened exactly; `latents`: storage dtype; `noise`: eps of a
    rollout step; `next_latents`: the stored x' of a replay (never re-rounded)."""
    assert dynamics in DYNAMICS and dtype in (torch.float32, torch.float64)
    in_dtype = latents.dtype
    v = v.to(dtype)
    x = latents.to(dtype)
    nxt = next_latents.to(dtype) if next_latents is not None else None
    s = _per_sample(sigma, x, dtype)
    sp = _per_sample(sigma_next, x, dtype)
    eta = torch.zeros_like(s) if dynamics == "ODE" else _per_sample(eta, x, dtype)
    dt = sp - s
    log_prob = None
    red = tuple(range(1, x.dim()))
    log_sqrt_2pi = torch.log(torch.sqrt(2 * torch.as_tensor(math.pi, dtype=dtype)))
    if dynamics == "ODE":  # :329-340
        mean = x + v * dt
        std = torch.zeros_like(s)
        if nxt is None:
            nxt = mean          # unrounded: cast_latents rounds it on store
        if compute_log_prob:
            log_prob = torch.zeros(x.shape[0], dtype=dtype)
    elif dynamics == "Flow-SDE":  # :342-371
        smax = _per_sample(sigma_max, x, dtype)
        std = torch.sqrt(s / (1 - torch.where(s == 1.0, smax, s))) * eta
        mean = x * (1 + std**2 / (2 * s) * dt) + v * (1 + std**2 * (1 - s) / (2 * s)) * dt
        if nxt is None:
            nxt = (mean + std * torch.sqrt(-1 * dt) * noise.to(dtype)).to(in_dtype).to(dtype)
        if compute_log_prob:
            sv = std * torch.sqrt(-1 * dt)
            lp = -((nxt - mean) ** 2) / (2 * sv**2) - torch.log(sv) - log_sqrt_2pi
            log_prob = lp.mean(dim=red)
    elif dynamics == "Dance-SDE":  # :373-398
        x0 = x - s * v
        std = eta
        log_term = 0.5 * eta**2 * (x - x0 * (1 - s)) / s**2
        mean = x + (v + log_term) * dt
        if nxt is None:
            nxt = (mean + std * torch.sqrt(-1 * dt) * noise.to(dtype)).to(in_dtype).to(dtype)
        if compute_log_prob:
            sv = std * torch.sqrt(-1 * dt)
            lp = -((nxt - mean) ** 2) / (2 * sv**2) - torch.log(sv) - log_sqrt_2pi
            log_prob = lp.mean(dim=red)
    else:  # CPS :400-420
        std = sp * torch.sin(eta * torch.pi / 2)
        x0 = x - s * v
        x1 = x + v * (1 - s)
        mean = x0 * (1 - sp) + x1 * torch.sqrt(sp**2 - std**2)
        if nxt is None:
            nxt = (mean + std * noise.to(dtype)).to(in_dtype).to(dtype)
        if compute_log_prob:
            lp = -((nxt - mean) ** 2)
            log_prob = lp.mean(dim=red)
    return dict(next_latents=nxt, next_latents_mean=mean, std_dev_t=std.reshape(-1), dt=dt.reshape(-1), log_prob=log_prob, noise_pred=v)


def consumed_prediction(v_text, v_uncond, guidance):
    """the value the step consumes: the prediction itself, or the CFG combine evaluated op by op in bf16"""
    return v_text if v_uncond is None else rollout_ref.cfg_combine_bf16(v_uncond, v_text, guidance)


def sde_step_bwd(v_text, v_uncond, guidance, latents, next_latents, sigma, sigma_next, eta, sigma_max, dynamics: str, compute_log_prob,
                 g_log_prob=None, g_noise_pred=None, g_mean=None, dtype=torch.float64):
    """d loss / d v for loss = <g_log_prob, log_prob> + <g_noise_pred, noise_pred> + <g_mean, next_latents_mean>, by autograd through
    `sde_step` in `dtype`; [B, ...], or [2B, ...] = [uncond | text] with a CFG pair."""
    with torch.enable_grad():
        v = consumed_prediction(v_text, v_uncond, guidance).detach().to(dtype).requires_grad_(True)
        out = sde_step(v, latents, sigma, sigma_next, eta, dynamics, sigma_max, next_latents=next_latents,
                       compute_log_prob=bool(compute_log_prob), dtype=dtype)
        loss = v.sum() * 0.0
        if g_log_prob is not None and out["log_prob"] is not None:
            loss = loss + (g_log_prob.to(dtype) * out["log_prob"]).sum()
        if g_noise_pred is not None:
            loss = loss + (g_noise_pred.to(dtype) * out["noise_pred"]).sum()
        if g_mean is not None:
            loss = loss + (g_mean.to(dtype) * out["next_latents_mean"]).sum()
        (dv,) = torch.autograd.grad(loss, v)
    if v_uncond is None:
        return dv
    g = torch.as_tensor(float(guidance), dtype=torch.float32).to(dtype)
    return torch.cat([(1 - g) * dv, g * dv])

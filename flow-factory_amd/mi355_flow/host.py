"""What the four families' host mirrors share above the engine (`adapter.py`, `flux.py`, `qwen.py`, `wan.py`).

`RolloutMixinBase` is the common part of the rollout mixins: bodies only.  `inference()` / `forward()` stay written out per family, because
their parameter lists are the ABI (the trainer filters kwargs by signature), and because the Flow-Factory plugin mixes these classes in
FRONT of the reference's adapters: nothing here may shadow an attribute of theirs (no `__init__`, `device`, mode switches, encode / decode).
`StandaloneAdapterBase` holds what only the four standalone adapters share; it is never part of a plugin class.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, Optional

import torch

from .scheduler import SDESchedulerOutput, host_noise_levels, randn_tensor
from .trajectory import _resolve, collect_rollout

logger = logging.getLogger(__name__)

_DTYPE_MAP = {"fp16": torch.float16, "float16": torch.float16, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16,
              "fp32": torch.float32, "float32": torch.float32}
VAE_SCALE_FACTOR = 8  # SD3 / FLUX / Qwen-Image VAE: latent = image / 8

_STEP_FIELDS = ("next_latents", "next_latents_mean", "noise_pred", "std_dev_t", "dt")


class RolloutMixinBase:
    """Shared bodies of `inference()` / `forward()` on the engine.  FLUX.1, Qwen-Image and Wan step as an engine forward followed by the
    fused scheduler step: their mixins provide `_FAMILY`, `_forward_impl(..., grad, host)`, `_rollout_stepwise` and `_sde_step` (two lines
    that call THEIR module's `sde_step`, so that the name stays patchable per module) and use everything below.  SD3.5 steps through its
    plan's fused `denoise_step`: it has its own `forward()` body and step-wise loop on `_native_grad_refusal`, `_step_schedule` and
    `_step_output`."""

    _FAMILY = ""
    _output_cls = SDESchedulerOutput      # hook: the Flow-Factory plugin puts the reference's own container here

    def _before_engine_call(self) -> None:
        """Hook run at the top of inference() / forward(): the Flow-Factory plugin re-binds changed weights here."""

    def _grad_fallback(self, why: str, kwargs: Dict[str, Any]):
        """Grad-mode forward() the native backward cannot serve.  Standalone: there is no other implementation -- raise (the Flow-Factory
        plugin overrides this with the reference's autograd path)."""
        raise NotImplementedError(f"mi355_flow: {self._FAMILY} forward() with autograd is not available natively: {why}")

    def _check_joint_attention_kwargs(self, jak: Optional[Dict[str, Any]], name: str = "joint_attention_kwargs") -> None:
        """`joint_attention_kwargs` / `attention_kwargs` (the reference forwards them to the transformer, sd3_5.py:421-428): diffusers
        consumes `scale` (LoRA scale of the peft backend: `scale_lora_layers`) and IP-adapter inputs.  The engine honours `scale` through the
        weight binding (LoRA deltas are merged with that extra factor; no effect without LoRA layers, as in diffusers); anything else raises."""
        jak = dict(jak or {})
        scale = float(jak.pop("scale", 1.0))
        if jak:
            raise NotImplementedError(f"mi355_flow: {name} {sorted(jak)} are not supported by the native engine (only the LoRA `scale` is)")
        live = getattr(self, "_live_weights", None)
        if live is not None:
            live.set_lora_scale(scale)
        elif scale != 1.0:
            logger.warning("%s['scale'] has no effect: no LoRA layers are bound to the native engine", name)

    # -------------------------------------------------------------- latent casting (models/abc.py:172-182)
    def cast_latents(self, latents: torch.Tensor, default_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        target = self.latent_storage_dtype or default_dtype
        if target is None or latents.dtype == target:
            return latents
        if target == torch.float16:
            latents = latents.clamp(-65504.0, 65504.0)  # unconditional: no abs().max().item() host sync
        return latents.to(target)

    # -------------------------------------------------------------- inference(): from the schedule to the collectors
    def _rollout_and_collect(self, plan, timesteps, N, guidance, latents, storage, step_noise, cond: tuple, compute_log_prob,
                             extra_call_back_kwargs, trajectory_indices, sampler=None, rollout_kw=None, **sampler_kw):
        """The tail of every `inference()`: the schedule as host lists (one D2H before the loop, none inside), the fused rollout (one C call)
        or -- when per-step callback tensors are asked for, or the family forces a `sampler` of `_rollout_stepwise`'s signature -- per-step
        engine calls (still all-HIP), then exactly the reference's collector bookkeeping (sd3_5.py:265-304) over the engine outputs.
        `cond`: the family's conditioning arguments, as its `plan.rollout` and `_rollout_stepwise` take them; `rollout_kw`: further keywords
        of the fused `plan.rollout` alone.  Returns (trajectory, final)."""
        sched = self.scheduler
        ts_host = [float(t) for t in timesteps.tolist()]
        sig_host = [float(s) for s in sched.sigmas.tolist()]
        eta_host = host_noise_levels(sched, N)
        dyn = sched.dynamics_type
        if sampler is None and any(k != "noise_level" for k in extra_call_back_kwargs):
            sampler = self._rollout_stepwise
        kept = _resolve(trajectory_indices, N + 1)
        keep_positions = list(range(N + 1)) if kept is None else sorted(kept)
        step_outputs = None
        if sampler is None:
            lat_kept, log_probs, final = plan.rollout(ts_host, sig_host, eta_host, dyn, guidance, latents, storage, step_noise, *cond,
                                                      keep_positions=keep_positions, compute_log_prob=compute_log_prob, **(rollout_kw or {}))
            pos_to_slot = {p: s for s, p in enumerate(keep_positions)}
        else:
            lat_kept, log_probs, step_outputs = sampler(plan, ts_host, sig_host, eta_host, guidance, latents, storage, step_noise, *cond,
                                                        compute_log_prob, extra_call_back_kwargs, **sampler_kw)
            final = lat_kept[N]
            pos_to_slot = {p: p for p in range(N + 1)}
        traj = collect_rollout(trajectory_indices, N, lambda pos: lat_kept[pos_to_slot[pos]], log_probs, eta_host, compute_log_prob,
                               step_outputs, extra_call_back_kwargs,
                               captured_noise_levels=host_noise_levels(sched, N, effective=False), dynamics=dyn)
        return traj, final

    def _stepwise(self, ts, sig, eta, latents, storage, step_noise, compute_log_prob, extra_keys, predict):
        """Common body of `_rollout_stepwise`: `predict(i, latents_i)` -> (v_text, v_uncond, guidance) is the family's engine forward, the
        fused scheduler step follows with the host arithmetic of the fused rollout (fp32 quotients)."""
        N, B = len(ts), latents.shape[0]
        cur = self.cast_latents(latents, storage)
        all_lat = [cur]
        log_probs = torch.full((N, B), float("nan"), device=latents.device)
        outs = []
        want = tuple(k for k in extra_keys if k in _STEP_FIELDS)
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)          # noqa: E731
        for i in range(N):
            t_next = ts[i + 1] if i + 1 < N else 0.0
            clp = compute_log_prob and eta[i] > 0
            vt, vu, gd = predict(i, cur)
            o = self._sde_step(vt, vu, gd, cur, f32(ts[i]) / f32(1000.0), f32(t_next) / f32(1000.0), eta[i], sig[1], self.scheduler.dynamics_type,
                               noise=step_noise[i] if step_noise is not None else None, compute_log_prob=clp, want=want)
            if clp:
                log_probs[i] = o.log_prob
            cur = o.next_storage
            all_lat.append(cur)
            outs.append(o)
        return all_lat, log_probs, outs

    # -------------------------------------------------------------- forward(): grad-mode dispatch
    def _native_grad_refusal(self, host, next_latents, compute_log_prob, return_kwargs) -> Optional[str]:
        """None when this grad-mode forward() can run on the engine's differentiable step for `host` (mi355_flow/autograd.py); else why not.
        (1) `optimize()` replay of a stored transition (trainers/grpo.py:263): log-prob of `next_latents`.  (2) The matching-loss trainers --
        AWM (trainers/awm.py:357-370), NFT (nft.py:297-304), DPO (dpo.py:468-469), DGPO (dgpo.py:352-364), CRD (crd.py:497-509) -- call
        forward() WITH autograd at an arbitrary `t`, no stored transition, `compute_log_prob=False`, and read `noise_pred`: the same step,
        whose network output, mean, std and dt do not depend on the next state (a placeholder transition is passed; its log-prob is
        switched off).  A freshly SAMPLED next state (or its log-prob) with autograd is not a native output: reference path."""
        from . import autograd as AG
        why = AG.unsupported_reason(host)
        sampled = next_latents is None and ("next_latents" in return_kwargs or (compute_log_prob and "log_prob" in return_kwargs))
        if why is None and sampled:
            why = "a sampled next state (or its log-prob) was requested with autograd"
        return why

    def _forward_dispatch(self, kw: Dict[str, Any], replay_host=None) -> SDESchedulerOutput:
        """Body of `forward(**kw)`: with autograd and a live module, the engine's differentiable forward + native backward when that backward
        covers the trainable set of `replay_host()` (default: this adapter), `_grad_fallback` when it does not; the no-grad step otherwise
        (also for a module with nothing trainable)."""
        if torch.is_grad_enabled() and getattr(self, "_live_weights", None) is not None:
            self._before_engine_call()
            host = self if replay_host is None else replay_host()
            why = self._native_grad_refusal(host, kw["next_latents"], kw["compute_log_prob"], kw["return_kwargs"])
            if why is None:
                return self._forward_impl(grad=True, host=host, **kw)
            if not why.startswith("the bound module has no trainable"):
                return self._grad_fallback(why, kw)
        return self._forward_nograd(**kw)

    def _forward_nograd(self, **kw) -> SDESchedulerOutput:
        with torch.no_grad():
            return self._forward_impl(grad=False, **kw)

    # -------------------------------------------------------------- forward(): the scheduler half of one step
    def _step_schedule(self, t: torch.Tensor, t_next, noise_level, latents: torch.Tensor, next_latents):
        """`t`: fp32 on the latents' device, 0-d or (B,).  Resolves `t_next` from the scheduler, sigma = t / 1000, the noise level and the
        noise draw of flow_match_euler_discrete.py:352-357 (none for a stored transition or under ODE dynamics).
        Returns (t_next, sigma, sigma_next, noise_level, noise, dynamics)."""
        sched, dev = self.scheduler, latents.device
        if t_next is None:
            idx = [sched.index_for_timestep(x) for x in t.reshape(-1)]
            t_next = torch.stack([sched.timesteps[i + 1] if i + 1 < len(sched.timesteps) else torch.zeros(()) for i in idx]).to(dev)
            if t.ndim == 0:
                t_next = t_next[0]
        t_next = torch.as_tensor(t_next, dtype=torch.float32, device=dev)
        dyn = sched.dynamics_type
        # exact fp32 quotient (torch's GPU tensor/scalar division multiplies by a rounded reciprocal: 1 ulp off
        # the host-side t/1000 the fused rollout uses, which would break the bit-exact ratio == 1 invariant)
        sigma, sigma_next = (t.double() / 1000).float(), (t_next.double() / 1000).float()
        if sched.is_eval or dyn == "ODE":
            noise_level = 0.0
        elif noise_level is None:
            noise_level = sched.get_noise_level_for_sigma(sigma.reshape(-1)) if sigma.ndim else sched.get_noise_level_for_sigma(float(sigma))
        noise = None
        if next_latents is None and dyn != "ODE":
            noise = randn_tensor(latents.shape, device=dev, dtype=torch.float32)
        return t_next, sigma, sigma_next, noise_level, noise, dyn

    def _step_output(self, return_kwargs, rank: int, next_latents, log_prob: bool, o=None, replay=None) -> SDESchedulerOutput:
        """The scheduler output of one step from `o` (an `sde_step` / `denoise_step` result) or `replay` (the autograd node's tuple, which
        never samples a next state).  std_dev_t / dt broadcast against latents of `rank` dimensions: (B, 1, ...)."""
        if replay is not None:
            lp, npred, mean, std, dt = replay
            sampled = None
        else:
            lp, npred, mean, std, dt, sampled = o.log_prob, o.noise_pred, o.next_latents_mean, o.std_dev_t, o.dt, o.next_latents
        view = (-1,) + (1,) * (rank - 1)
        res = dict(noise_pred=npred, next_latents=sampled if next_latents is None else next_latents.float(), next_latents_mean=mean,
                   std_dev_t=std.view(view) if std is not None else None, dt=dt.view(view) if dt is not None else None,
                   log_prob=lp if log_prob else None)
        return self._output_cls.from_dict({k: res[k] for k in return_kwargs if k in res})

    def _scheduler_step(self, t, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs, v=None, replay=None):
        """Second half of a family's `_forward_impl`.  No-grad: `v` = (v_text, v_uncond, guidance), the prediction(s) of the engine forward
        that already ran.  Grad: `replay` = (autograd entry point, host, plan, the family's entries of the call record); the stored
        transition's log-prob when there is one, else a placeholder transition with the log-prob switched off."""
        _, sigma, sigma_next, noise_level, noise, dyn = self._step_schedule(t, t_next, noise_level, latents, next_latents)
        sigma_max = float(self.scheduler.sigmas[1])
        if replay is not None:
            fn, host, plan, call = replay
            clp = bool(compute_log_prob) and next_latents is not None
            call = dict(call, latents=latents, sigma=sigma, sigma_next=sigma_next, eta=noise_level, sigma_max=sigma_max, dynamics=dyn,
                        next_latents=latents if next_latents is None else next_latents, compute_log_prob=clp)
            return self._step_output(return_kwargs, latents.ndim, next_latents, clp, replay=fn(host, plan, call))
        o = self._sde_step(*v, latents, sigma, sigma_next, noise_level, sigma_max, dyn, noise=noise, next_latents=next_latents,
                           compute_log_prob=compute_log_prob, want=tuple(k for k in return_kwargs if k in _STEP_FIELDS))
        return self._step_output(return_kwargs, latents.ndim, next_latents, compute_log_prob, o=o)


class StandaloneAdapterBase:
    """What the four standalone adapters (no Flow-Factory import) share: the engine bound from a state dict or from a live torch module,
    the scheduler's mode switches, the latent storage dtype and the numpy tail of `decode_latents`."""

    def _init_engine(self, engine_cls, config, scheduler, latent_storage_dtype, transformer_dtype, device) -> None:
        if not torch.cuda.is_available():
            raise RuntimeError("mi355_flow: no GPU visible; the native rollout engine has no CPU path")
        self.device = torch.device(device)
        self.transformer_dtype = transformer_dtype
        self._latent_storage = latent_storage_dtype
        self.scheduler = scheduler
        self.engine = engine_cls(config)
        self._live_weights = None

    def _bind(self, source) -> None:
        """`source`: a state dict (bound once; `refresh_weights` re-binds) or an `nn.Module` (bound live)."""
        if isinstance(source, torch.nn.Module):
            # a torch module with HF parameter names (possibly DDP / FSDP2 / peft wrapped): its CURRENT parameters are re-bound before every
            # engine call, and grad-mode forward() differentiates w.r.t. its trainable parameters (mi355_flow/autograd.py)
            from .binding import LiveWeights
            self._live_weights = LiveWeights(self.engine, lambda: source)
            self._sync_weights()
        else:
            self.refresh_weights(source)

    def _init_vae(self, decoder_cls, config, state_dict, max_batch: int) -> None:
        self.vae_decoder = None
        self.vae_max_batch = max_batch
        if state_dict is not None:
            self.vae_decoder = decoder_cls(config)
            self.vae_decoder.bind_state_dict(state_dict)
            self.vae_decoder.ready()

    @property
    def latent_storage_dtype(self) -> Optional[torch.dtype]:
        return _DTYPE_MAP.get(self._latent_storage) if self._latent_storage else None

    def _sync_weights(self) -> int:
        if self._live_weights is None:
            return 0
        n = self._live_weights.sync()
        if n:
            self.engine.ready()
        return n

    def _before_engine_call(self) -> None:
        self._sync_weights()

    def refresh_weights(self, state_dict: Dict[str, torch.Tensor]) -> None:
        """Re-pack the (live) torch parameters: call after optimizer steps / EMA swaps / LoRA merges."""
        self.engine.bind_state_dict(state_dict)
        self.engine.ready()

    # mode switches the trainer calls (models/abc.py:351-378)
    def rollout(self):
        self.scheduler.rollout()

    def eval(self):
        self.scheduler.eval()

    def train(self, mode: bool = True):
        self.scheduler.train(mode)

    @staticmethod
    def _images_as(img: torch.Tensor, output_type: str):
        """(B, 3, H, W) images as 'pt' (unchanged) or 'np' (B, H, W, 3) fp32 on the host."""
        return img if output_type == "pt" else img.float().permute(0, 2, 3, 1).cpu().numpy()

"""`SD3_5NativeAdapter`: the rollout hot path of Flow-Factory's `SD3_5Adapter` on the MI355X engine.

Mirrors `SD3_5Adapter.inference` / `SD3_5Adapter.forward` (reference
src/flow_factory/models/stable_diffusion/sd3_5.py:176-349, :352-448): the parameter names and
defaults are the ABI (the trainer filters kwargs by signature, trainers/grpo.py:165,252), the RNG
draw order, latent storage dtype, CFG batch order and collector semantics are the reference's.
The N-step loop itself runs inside libmi355flow.so (`mi355_rollout`) with no host sync.

This class is self-contained (no `flow_factory` / `diffusers` import) so it runs and is tested
here; `mi355_flow.flow_factory_plugin` subclasses the reference's own `SD3_5Adapter` with it when
Flow-Factory is installed.
"""
from __future__ import annotations

import logging
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from .engine import Engine, TransformerConfig
from .host import _DTYPE_MAP, _STEP_FIELDS, VAE_SCALE_FACTOR, RolloutMixinBase, StandaloneAdapterBase  # noqa: F401  (re-exported)
from .samples import SD3_5Sample
from .scheduler import FlowMatchEulerDiscreteSDEScheduler, SDESchedulerOutput, randn_tensor, set_scheduler_timesteps
from .trajectory import TrajectoryIndicesType

logger = logging.getLogger(__name__)


class NativeRolloutMixin(RolloutMixinBase):
    """inference()/forward() on the engine.  Host classes provide: `engine` (Engine), `scheduler`
    (FlowMatchEulerDiscreteSDEScheduler-like), `device`, `transformer_dtype`,
    `latent_storage_dtype`, `decode_latents(latents, output_type)`."""

    engine: Engine
    scheduler: FlowMatchEulerDiscreteSDEScheduler
    # hooks the Flow-Factory plugin overrides with the reference's own objects (flow_factory_plugin.py): the sample class the
    # trainer stacks (`BaseSample.stack`, trainers/grpo.py:215), the schedule setter and the scheduler-output container
    _sample_cls = SD3_5Sample
    _set_timesteps = staticmethod(set_scheduler_timesteps)

    def _grad_fallback(self, why: str, kwargs: Dict[str, Any]):
        """Grad-mode forward() with trainable parameters the native backward does not cover.  The Flow-Factory plugin overrides this
        with the reference's autograd path; standalone there is no other implementation to fall back to."""
        raise NotImplementedError(f"mi355_flow: grad-mode forward() is not available: {why}")

    # -------------------------------------------------------------- rollout
    @torch.no_grad()
    def inference(
        self,
        prompt: Union[str, List[str], None] = None,
        negative_prompt: Optional[Union[str, List[str]]] = None,
        height: Optional[int] = 1024,
        width: Optional[int] = 1024,
        num_inference_steps: Optional[int] = 50,
        guidance_scale: float = 7.5,
        generator: Optional[torch.Generator] = None,
        joint_attention_kwargs: Optional[Dict[str, Any]] = None,
        prompt_ids: Optional[torch.Tensor] = None,
        prompt_embeds: Optional[torch.Tensor] = None,
        pooled_prompt_embeds: Optional[torch.Tensor] = None,
        negative_prompt_ids: Optional[torch.Tensor] = None,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        negative_pooled_prompt_embeds: Optional[torch.Tensor] = None,
        compute_log_prob: bool = True,
        extra_call_back_kwargs: List[str] = [],
        trajectory_indices: TrajectoryIndicesType = "all",
    ) -> List[SD3_5Sample]:
        self._before_engine_call()
        device = self.device
        dtype = self.transformer_dtype
        self._check_joint_attention_kwargs(joint_attention_kwargs)
        do_cfg = guidance_scale > 1.0
        has_neg = negative_prompt is not None or (negative_prompt_embeds is not None and negative_pooled_prompt_embeds is not None)
        if do_cfg and not has_neg:
            logger.warning("No negative prompt/embeds provided, classifier-free-guidance will be disabled.")
            do_cfg = False
        if prompt_embeds is None or pooled_prompt_embeds is None:
            enc = self.encode_prompt(prompt, negative_prompt, guidance_scale=guidance_scale, device=device)
            prompt_embeds, pooled_prompt_embeds, prompt_ids = enc["prompt_embeds"], enc["pooled_prompt_embeds"], enc["prompt_ids"]
            if do_cfg:
                negative_prompt_embeds = enc["negative_prompt_embeds"]
                negative_prompt_ids = enc["negative_prompt_ids"]
                negative_pooled_prompt_embeds = enc["negative_pooled_prompt_embeds"]
        else:
            prompt_embeds, pooled_prompt_embeds = prompt_embeds.to(device), pooled_prompt_embeds.to(device)
            if do_cfg:
                if negative_prompt_embeds is None or negative_pooled_prompt_embeds is None:
                    raise ValueError("classifier-free guidance with pre-encoded prompts needs negative_prompt_embeds "
                                     "and negative_pooled_prompt_embeds")
                negative_prompt_embeds = negative_prompt_embeds.to(device)
                negative_pooled_prompt_embeds = negative_pooled_prompt_embeds.to(device)
        B = len(prompt_embeds)
        C = self.engine.cfg.in_channels
        h, w = int(height) // VAE_SCALE_FACTOR, int(width) // VAE_SCALE_FACTOR
        N = int(num_inference_steps)

        # RNG, in the reference's order: prepare_latents on `generator` (transformer dtype; None = the global device generator, a CPU
        # generator draws on the host like diffusers' randn_tensor), then one fp32 draw per step -- also when noise_level == 0, but none
        # at all under ODE dynamics (flow_match_euler_discrete.py:329-340 draws nothing).  The step draws ALWAYS come from the global
        # generator: the reference hands `generator` to `prepare_latents` only (sd3_5.py:242-250), never to `scheduler.step` (:436-446)
        # (found by tests/test_rollout_control_flow_pin.py::test_differential_sweep_plugin_vs_reference_adapter)
        dyn = self.scheduler.dynamics_type
        latents = randn_tensor((B, C, h, w), generator=generator, device=device, dtype=dtype)
        step_noise = None
        if dyn != "ODE":
            step_noise = torch.empty((N, B, C, h, w), device=device, dtype=torch.float32)
            for i in range(N):
                step_noise[i] = randn_tensor((B, C, h, w), generator=None, device=device, dtype=torch.float32)

        ps = self.engine.cfg.patch_size
        timesteps = self._set_timesteps(self.scheduler, N, seq_len=(h // ps) * (w // ps), device=device)
        storage = self.latent_storage_dtype or dtype

        plan = self.engine.plan(B, 2 if do_cfg else 1, h, w, prompt_embeds.shape[1], N)
        cond = (prompt_embeds, pooled_prompt_embeds, negative_prompt_embeds if do_cfg else None, negative_pooled_prompt_embeds if do_cfg else None)
        traj, final = self._rollout_and_collect(plan, timesteps, N, guidance_scale, latents, storage, step_noise, cond, compute_log_prob,
                                                extra_call_back_kwargs, trajectory_indices)
        images = self.decode_latents(latents=final, output_type="pt")
        samples = []
        for b in range(B):
            samples.append(self._sample_cls(
                timesteps=timesteps,
                **traj.per_sample(b),
                prompt=prompt[b] if isinstance(prompt, list) else prompt,
                prompt_ids=prompt_ids[b] if prompt_ids is not None else None,
                prompt_embeds=prompt_embeds[b],
                pooled_prompt_embeds=pooled_prompt_embeds[b],
                negative_prompt=(negative_prompt[b] if isinstance(negative_prompt, list) else negative_prompt),
                negative_prompt_ids=negative_prompt_ids[b] if negative_prompt_ids is not None else None,
                negative_prompt_embeds=negative_prompt_embeds[b] if negative_prompt_embeds is not None else None,
                negative_pooled_prompt_embeds=negative_pooled_prompt_embeds[b] if negative_pooled_prompt_embeds is not None else None,
                height=height, width=width,
                image=images[b] if images is not None else None,
            ))
        return samples

    def _rollout_stepwise(self, plan, ts, sig, eta, guidance, latents, storage, step_noise, pe, pp, ne, npl, compute_log_prob,
                          extra_keys):
        """Per-step engine calls (still all-HIP) for rollouts that ask for per-step callback tensors."""
        N, B = len(ts), latents.shape[0]
        cur = self.cast_latents(latents, storage)
        all_lat = [cur]
        log_probs = torch.full((N, B), float("nan"), device=latents.device)
        outs = []
        want = tuple(k for k in extra_keys if k in _STEP_FIELDS)
        for i in range(N):
            t_next = ts[i + 1] if i + 1 < N else 0.0
            clp = compute_log_prob and eta[i] > 0
            enc_a, pool_a, enc_b, pool_b = (ne, npl, pe, pp) if ne is not None else (pe, pp, None, None)
            o = plan.denoise_step(cur, torch.tensor(ts[i]), enc_a, pool_a, enc_b, pool_b, guidance,
                                  torch.tensor(ts[i]) / 1000, torch.tensor(t_next) / 1000, eta[i], sig[1],
                                  self.scheduler.dynamics_type, noise=step_noise[i] if step_noise is not None else None,
                                  compute_log_prob=clp, want=want)
            if clp:
                log_probs[i] = o.log_prob
            cur = o.next_storage
            all_lat.append(cur)
            outs.append(o)
        return all_lat, log_probs, outs

    # -------------------------------------------------------------- one step (rollout or replay)
    def forward(
        self,
        t: torch.Tensor,
        latents: torch.Tensor,
        prompt_embeds: torch.Tensor,
        pooled_prompt_embeds: torch.Tensor,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        negative_pooled_prompt_embeds: Optional[torch.Tensor] = None,
        guidance_scale: float = 7.5,
        t_next: Optional[torch.Tensor] = None,
        next_latents: Optional[torch.Tensor] = None,
        noise_level: Optional[float] = None,
        joint_attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        return_kwargs: List[str] = ["noise_pred", "next_latents", "next_latents_mean", "std_dev_t", "dt", "log_prob"],
    ) -> SDESchedulerOutput:
        self._before_engine_call()
        self._check_joint_attention_kwargs(joint_attention_kwargs)
        B = latents.shape[0]
        dev = latents.device
        if guidance_scale > 1.0 and (negative_prompt_embeds is None or negative_pooled_prompt_embeds is None):
            logger.warning("Passed `guidance_scale` > 1.0, but no `negative_prompt_embeds` or `negative_pooled_prompt_embeds` "
                           "provided. Classifier-free guidance will be disabled.")
        do_cfg = negative_prompt_embeds is not None and negative_pooled_prompt_embeds is not None and guidance_scale > 1.0
        sched = self.scheduler
        t = torch.as_tensor(t, dtype=torch.float32, device=dev)
        t_next, sigma, sigma_next, noise_level, noise, dyn = self._step_schedule(t, t_next, noise_level, latents, next_latents)
        plan = self.engine.plan(B, 2 if do_cfg else 1, latents.shape[2], latents.shape[3], prompt_embeds.shape[1], 1)
        enc = (negative_prompt_embeds, negative_pooled_prompt_embeds, prompt_embeds, pooled_prompt_embeds) if do_cfg else \
              (prompt_embeds, pooled_prompt_embeds, None, None)
        sigma_max = float(sched.sigmas[1])
        if torch.is_grad_enabled() and getattr(self, "_live_weights", None) is not None:
            # grad-mode forward on the engine's differentiable step (mi355_flow/autograd.py: denoise_replay) -- see `_native_grad_refusal`
            from . import autograd as AG
            why = self._native_grad_refusal(self, next_latents, compute_log_prob, return_kwargs)
            if why is None:
                clp = bool(compute_log_prob) and next_latents is not None
                call = dict(latents=latents, timestep=t, enc_a=enc[0], pooled_a=enc[1], enc_b=enc[2], pooled_b=enc[3], guidance=guidance_scale,
                            sigma=sigma, sigma_next=sigma_next, eta=noise_level, sigma_max=sigma_max, dynamics=dyn,
                            next_latents=latents if next_latents is None else next_latents, compute_log_prob=clp)
                return self._step_output(return_kwargs, 4, next_latents, clp, replay=AG.denoise_replay(self, plan, call))
            if not why.startswith("the bound module has no trainable"):
                return self._grad_fallback(why, dict(
                    t=t, latents=latents, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                    negative_prompt_embeds=negative_prompt_embeds, negative_pooled_prompt_embeds=negative_pooled_prompt_embeds,
                    guidance_scale=guidance_scale, t_next=t_next, next_latents=next_latents, noise_level=noise_level,
                    joint_attention_kwargs=joint_attention_kwargs, compute_log_prob=compute_log_prob, return_kwargs=return_kwargs))
        o = plan.denoise_step(latents, t, enc[0], enc[1], enc[2], enc[3], guidance_scale, sigma, sigma_next, noise_level,
                              sigma_max, dyn, noise=noise, next_latents=next_latents, compute_log_prob=compute_log_prob,
                              want=tuple(k for k in return_kwargs if k in _STEP_FIELDS))
        return self._step_output(return_kwargs, 4, next_latents, compute_log_prob, o=o)


class SD3_5NativeAdapter(StandaloneAdapterBase, NativeRolloutMixin):
    """Standalone adapter (no Flow-Factory import): engine + scheduler + optional VAE decoder."""

    def __init__(self, state_dict: Union[Dict[str, torch.Tensor], torch.nn.Module], config: Optional[TransformerConfig] = None,
                 scheduler: Optional[FlowMatchEulerDiscreteSDEScheduler] = None, latent_storage_dtype: Optional[str] = "fp16",
                 transformer_dtype: torch.dtype = torch.bfloat16, device: Union[str, torch.device] = "cuda",
                 vae_decode: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                 vae_state_dict: Optional[Dict[str, torch.Tensor]] = None, vae_config=None, vae_max_batch: int = 4):
        from .vae import VAEConfig, VAEDecoder
        self._init_engine(Engine, config or TransformerConfig(),
                          scheduler or FlowMatchEulerDiscreteSDEScheduler(shift=3.0, sde_steps=[1, 2, 3], num_sde_steps=1),
                          latent_storage_dtype, transformer_dtype, device)
        self._bind(state_dict)
        self._vae_decode = vae_decode
        self._init_vae(VAEDecoder, vae_config or VAEConfig(), vae_state_dict, vae_max_batch)

    def encode_prompt(self, *a, **k):
        raise RuntimeError("mi355_flow standalone adapter has no text encoders: pass prompt_embeds / pooled_prompt_embeds "
                           "(the Flow-Factory plugin inherits encode_prompt from SD3_5Adapter)")

    def decode_latents(self, latents: torch.Tensor, output_type: str = "pt"):
        """sd3_5.py:161-172.  With `vae_state_dict` the native decoder (mi355_vae_*) produces the 'pt' images; a custom
        `vae_decode` callable takes precedence; with neither the samples carry no image."""
        if self._vae_decode is not None:
            return self._vae_decode(latents)
        if self.vae_decoder is None:
            return None
        if output_type not in ("pt", "np"):
            raise ValueError("mi355_flow standalone adapter decodes to 'pt' or 'np' (PIL conversion lives in the pipeline's image_processor)")
        return self._images_as(self.vae_decoder.decode(latents, postprocess=True, out_dtype=torch.bfloat16, max_batch=self.vae_max_batch), output_type)

"""Wan2.1 text-to-video rollout on the native engine (mi355_wan_*): host mirror of `Wan2_T2V_Adapter.inference` / `.forward`
(reference src/flow_factory/models/wan/wan2_t2v.py:234-421, :426-543) -- SURVEY.md 8(f) row N4, single-transformer Wan2.1.

Kept from the reference: latents `(B, 16, T, h, w)` drawn in fp32 (`prepare_latents(dtype=float32)`), `timestep = t.expand(B)` with
the scheduler's integer timesteps, classifier-free guidance as `u + g (c - u)` (here one forward over the batch [negative, positive]
instead of two passes), `UniPCMultistepSDEScheduler.step` in rollout mode = the four SDE / ODE dynamics with sigma = t / 1000.
Not covered (raise): `attention_kwargs`; image-conditioned TI2V (per-token timesteps that DIFFER: the text-to-video use of Wan2.2-TI2V-5B, whose
`expand_timesteps` mask is all ones, runs as the scalar-timestep forward).  The causal 3-D video VAE decode is native too
(`mi355_flow.vae.WanVAEDecoder`, csrc/wan_vae_engine.hip): pass `vae_state_dict` to the standalone adapter (or a `video_decode` callable).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._lib import WanCfg
from .engine import EngineBase, PlanBase, _bf16c, _ptr, _stream, dtype_code, sde_step
from .host import RolloutMixinBase, StandaloneAdapterBase
from .samples import WanT2VSample
from .scheduler import FlowMatchEulerDiscreteSDEScheduler, SDESchedulerOutput, randn_tensor
from .trajectory import TrajectoryIndicesType

VAE_SCALE_SPATIAL, VAE_SCALE_TEMPORAL = 8, 4


@dataclass
class WanConfig:
    """diffusers WanTransformer3DModel config fields the engine needs (Wan2.1-T2V-1.3B defaults)."""
    in_channels: int = 16
    out_channels: int = 16
    num_layers: int = 30
    num_attention_heads: int = 12
    attention_head_dim: int = 128
    ffn_dim: int = 8960
    text_dim: int = 4096
    freq_dim: int = 256
    patch_size: Tuple[int, int, int] = (1, 2, 2)
    eps: float = 1e-6

    @property
    def dim(self) -> int:
        return self.num_attention_heads * self.attention_head_dim

    def to_c(self) -> WanCfg:
        return WanCfg(self.in_channels, self.out_channels, self.num_layers, self.num_attention_heads, self.attention_head_dim, self.ffn_dim,
                      self.text_dim, self.freq_dim, self.patch_size[0], self.patch_size[1], self.patch_size[2], self.eps)


class UniPCMultistepSDEScheduler(FlowMatchEulerDiscreteSDEScheduler):
    """Rollout-mode mirror of the reference's `UniPCMultistepSDEScheduler` (scheduler/unipc_multistep.py): the SDE-step selection
    mixin and `step()` are shared with the flow-match scheduler (its train / rollout branch is the same four dynamics,
    :296-421); the schedule is diffusers' UniPC flow schedule (`use_flow_sigmas`, `flow_shift`): integer timesteps."""

    def __init__(self, flow_shift: float = 3.0, **kw):
        kw.setdefault("shift", flow_shift)
        super().__init__(**kw)
        self.config["flow_shift"] = flow_shift

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, **_ignored) -> None:
        n_train = self.config.num_train_timesteps
        shift = self.config["flow_shift"]
        alphas = np.linspace(1, 1 / n_train, num_inference_steps + 1)
        sig = 1.0 - alphas
        sig = np.flip(shift * sig / (1 + (shift - 1) * sig))[:-1].copy()
        ts = (sig * n_train).copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts).to(device=device)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32)).to(device=device)
        self.num_inference_steps = len(ts)
        self._host_timesteps = [float(x) for x in ts.tolist()]


class WanPlan(PlanBase):
    _PRE = "wan_"

    def __init__(self, engine: WanEngine, batch: int, n_cfg: int, T: int, h: int, w: int, n_text: int, max_steps: int):
        self.batch, self.n_cfg, self.T, self.h, self.w, self.n_text = batch, n_cfg, T, h, w, n_text
        super().__init__(engine, (batch, n_cfg, T, h, w, n_text), max_steps)
        # d loss / d v arrives as [uncond | text], as `engine.sde_step_bwd` returns it
        self.dv_shape = (batch * n_cfg, engine.cfg.out_channels, T, h, w)

    def _forward(self, symbol: str, latents, t, enc_a, enc_b) -> torch.Tensor:
        B, Bp = self.batch, self.batch * self.n_cfg
        assert tuple(latents.shape) == (B, self.C, self.T, self.h, self.w), latents.shape
        dev = latents.device
        t = t.to(device=dev, dtype=torch.float32).reshape(-1)
        t = (t.expand(Bp) if t.numel() == 1 else (t.repeat(self.n_cfg) if t.numel() == B and self.n_cfg == 2 else t)).contiguous()
        assert t.numel() == Bp
        out = torch.empty(self.dv_shape, device=dev, dtype=torch.bfloat16)
        latents = latents.contiguous()
        ea = _bf16c(enc_a)
        eb = _bf16c(enc_b) if enc_b is not None else None
        self._call(symbol, self._h, _stream(), _ptr(latents), dtype_code(latents.dtype), _ptr(t), _ptr(ea), _ptr(eb), _ptr(out))
        return out

    def transformer_forward(self, latents: torch.Tensor, t: torch.Tensor, enc_a: torch.Tensor, enc_b: Optional[torch.Tensor] = None):
        """latents (B, 16, T, h, w); t (B*n_cfg,) or scalar; n_cfg == 2: enc_a = negative, enc_b = positive, output (2B, ...)."""
        return self._forward("forward", latents, t, enc_a, enc_b)

    # ---------------------------------------------------------------- differentiable forward (optimize() replay)
    def forward_train(self, latents: torch.Tensor, t: torch.Tensor, enc_a: torch.Tensor, enc_b: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mi355_wan_forward_train: `transformer_forward` on per-block activation buffers -- the same kernel binaries, so the prediction is
        bit-identical -- keeping what `backward` needs in the plan's training stash (ONE per plan; every call takes a serial number)."""
        out = self._forward("forward_train", latents, t, enc_a, enc_b)
        self._train_serial += 1
        return out

    def rollout(self, timesteps: Sequence[float], sigmas: Sequence[float], noise_levels: Sequence[float], dynamics: str, guidance: float,
                init_latents: torch.Tensor, storage_dtype: torch.dtype, step_noise: Optional[torch.Tensor], prompt_embeds: torch.Tensor,
                neg_embeds: Optional[torch.Tensor] = None, keep_positions: Optional[Sequence[int]] = None, compute_log_prob: bool = True):
        shape = (self.batch, self.C, self.T, self.h, self.w)
        assert tuple(init_latents.shape) == shape, init_latents.shape
        pe = _bf16c(prompt_embeds)
        ne = _bf16c(neg_embeds) if neg_embeds is not None else None
        return self._rollout(shape, timesteps, sigmas, noise_levels, dynamics, guidance, init_latents, storage_dtype, step_noise,
                             (_ptr(pe), _ptr(ne)), keep_positions, compute_log_prob)


class WanEngine(EngineBase):
    """Owns the packed bf16 copy of one Wan transformer (mi355_wan).  `plan(batch, n_cfg, T, h, w, n_text, max_steps)`."""

    _ABI, _WHAT, _PLAN = "wan", "Wan transformer", WanPlan

    #: the native backward (end of round 4; its seven GPU tests are green on MI355X: profiles/r04u_*, r04v_*).  MI355_WAN_NATIVE_BACKWARD=0 keeps
    #: grad-mode forward() on the engine-valued replay (value = engine, gradient = the reference's torch path)
    native_backward_enabled = os.environ.get("MI355_WAN_NATIVE_BACKWARD", "1") != "0"

    def __init__(self, cfg: WanConfig = WanConfig()):
        super().__init__(cfg)

    def grad_supported(self, name: str) -> int:
        return super().grad_supported(name) if type(self).native_backward_enabled else 0


class WanRolloutMixin(RolloutMixinBase):
    """`inference()` / `forward()` of `Wan2_T2V_Adapter` (reference models/wan/wan2_t2v.py:234-421, :426-543) on the engine, for the
    single-transformer Wan2.1 configuration.  Host classes provide `engine` (WanEngine), `scheduler`, `device`, `transformer_dtype`,
    `latent_storage_dtype`, `encode_prompt`, `decode_latents(latents, output_type)`.

    Evaluation mode: the reference's `UniPCMultistepSDEScheduler.step` delegates to diffusers' UniPC multistep predictor-corrector when
    `is_eval` (scheduler/unipc_multistep.py:282-285).  Since round 5 `inference()` samples it natively (`_rollout_eval`: per-step engine
    forwards + the solver as two streaming HIP kernels, mi355_flow/unipc.py; the solver body is third-party code restated from its published
    algorithm -- oracle/unipc_ref.py, parity unpinned).  `MI355_WAN_EVAL_REFERENCE=1` routes evaluation to `_eval_inference` instead (the
    Flow-Factory plugin: the reference's own loop; standalone it raises) -- never a silent first-order Euler step."""

    _FAMILY = "Wan"
    _sample_cls = WanT2VSample
    # Wan2.2 two-expert pipelines (wan2_t2v.py:476-487): `engine` holds the high-noise expert (`pipeline.transformer`, used while
    # t >= boundary_ratio * num_train_timesteps with `guidance_scale`), `engine_2` the low-noise one (`pipeline.transformer_2`, with
    # `guidance_scale_2`).  None = single-transformer Wan2.1.  Per-token timesteps (`expand_timesteps`, TI2V-5B) are not supported.
    engine_2 = None
    boundary_ratio: Optional[float] = None
    low_noise_only = False      # a Wan2.2 pipeline whose boundary lies above every timestep: `engine` holds transformer_2, guidance_scale_2 applies

    def _boundary_timestep(self, boundary_timestep: Optional[float] = None) -> Optional[float]:
        if boundary_timestep is None and self.boundary_ratio is not None:
            boundary_timestep = float(self.boundary_ratio) * float(self.scheduler.config.get("num_train_timesteps", 1000))
        return boundary_timestep

    def _expert(self, t: float, guidance_scale: float, guidance_scale_2: Optional[float], boundary_timestep: Optional[float]):
        """(engine, guidance) for a step at timestep t: the reference's selection rule."""
        if self.low_noise_only:
            return self.engine, (guidance_scale_2 if guidance_scale_2 is not None else guidance_scale)
        bt = self._boundary_timestep(boundary_timestep)
        if self.engine_2 is None or bt is None or t >= bt:
            return self.engine, guidance_scale
        return self.engine_2, (guidance_scale_2 if guidance_scale_2 is not None else guidance_scale)

    def _sde_step(self, *a, **k):
        return sde_step(*a, **k)          # this module's name, looked up per call

    def _eval_inference(self, **kwargs):
        raise NotImplementedError("mi355_flow: evaluation-mode sampling for Wan uses diffusers' UniPC multistep solver in the reference "
                                  "(unipc_multistep.py:282-285); the native engine implements the rollout (SDE / Euler) branch only")

    # ------------------------------------------------------------------ rollout (wan2_t2v.py:234-421)
    @torch.no_grad()
    def inference(
        self,
        prompt: Optional[Union[str, List[str]]] = None,
        negative_prompt: Optional[Union[str, List[str]]] = None,
        height: int = 480,
        width: int = 832,
        num_frames: int = 81,
        num_inference_steps: int = 50,
        guidance_scale: float = 5.0,
        guidance_scale_2: Optional[float] = None,
        generator: Optional[torch.Generator] = None,
        prompt_ids: Optional[torch.Tensor] = None,
        prompt_embeds: Optional[torch.Tensor] = None,
        negative_prompt_ids: Optional[torch.Tensor] = None,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        compute_log_prob: bool = False,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        max_sequence_length: int = 512,
        extra_call_back_kwargs: List[str] = [],
        trajectory_indices: TrajectoryIndicesType = "all",
    ) -> List[WanT2VSample]:
        device = self.device
        eval_mode = bool(getattr(self.scheduler, "is_eval", False))
        if eval_mode and os.environ.get("MI355_WAN_EVAL_REFERENCE") == "1":
            return self._eval_inference(
                prompt=prompt, negative_prompt=negative_prompt, height=height, width=width, num_frames=num_frames,
                num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, guidance_scale_2=guidance_scale_2,
                generator=generator, prompt_ids=prompt_ids, prompt_embeds=prompt_embeds, negative_prompt_ids=negative_prompt_ids,
                negative_prompt_embeds=negative_prompt_embeds, compute_log_prob=compute_log_prob, attention_kwargs=attention_kwargs,
                max_sequence_length=max_sequence_length, extra_call_back_kwargs=extra_call_back_kwargs,
                trajectory_indices=trajectory_indices)
        self._before_engine_call()
        if attention_kwargs:
            raise NotImplementedError("mi355_flow: attention_kwargs are not supported by the native engine")
        if self.low_noise_only:
            if guidance_scale_2 is not None:
                guidance_scale = guidance_scale_2          # every step runs the low-noise expert with its own scale
            guidance_scale_2 = None
        if guidance_scale_2 is not None and guidance_scale_2 != guidance_scale and self.engine_2 is None:
            raise ValueError("mi355_flow: guidance_scale_2 needs a two-expert (Wan2.2) adapter: no second transformer is bound")
        # (the pipeline's VAE compression: 4 x 8 x 8 for Wan2.1 / Wan2.2-A14B, 4 x 16 x 16 for the Wan2.2-TI2V-5B VAE; the plugin reads them
        # from the pipeline, wan2_t2v.py:267-279)
        vst, vss = int(getattr(self, "vae_scale_temporal", VAE_SCALE_TEMPORAL)), int(getattr(self, "vae_scale_spatial", VAE_SCALE_SPATIAL))
        if (num_frames - 1) % vst != 0:
            num_frames = num_frames // vst * vst + 1
        num_frames = max(num_frames, 1)
        ps = self.engine.cfg.patch_size
        hm, wm = vss * ps[1], vss * ps[2]
        height, width = height // hm * hm, width // wm * wm
        if prompt_embeds is None:
            enc = self.encode_prompt(prompt=prompt, negative_prompt=negative_prompt, guidance_scale=guidance_scale)
            prompt_embeds, prompt_ids = enc["prompt_embeds"], enc["prompt_ids"]
            negative_prompt_embeds, negative_prompt_ids = enc.get("negative_prompt_embeds"), enc.get("negative_prompt_ids")
        prompt_embeds = prompt_embeds.to(device).to(self.transformer_dtype)
        if negative_prompt_embeds is not None:
            negative_prompt_embeds = negative_prompt_embeds.to(device).to(self.transformer_dtype)
        two = self.engine_2 is not None
        g2 = guidance_scale_2 if guidance_scale_2 is not None else guidance_scale
        do_cfg = (guidance_scale > 1.0 or (two and g2 > 1.0)) and negative_prompt_embeds is not None
        B = prompt_embeds.shape[0]
        N = int(num_inference_steps)
        self.scheduler.set_timesteps(N, device=device)
        timesteps = self.scheduler.timesteps
        Cl = self.engine.cfg.in_channels
        T, h, w = (num_frames - 1) // vst + 1, height // vss, width // vss
        # RNG in the reference's order: prepare_latents in fp32, then one fp32 draw per step
        # (none of the step draws under ODE dynamics: the reference's ODE branch draws nothing)
        latents = randn_tensor((B, Cl, T, h, w), generator=generator, device=device, dtype=torch.float32)
        step_noise = None
        if self.scheduler.dynamics_type != "ODE" and not eval_mode:      # (the evaluation-mode solver is deterministic: the reference draws nothing)
            step_noise = torch.empty((N, B, Cl, T, h, w), device=device, dtype=torch.float32)
            for i in range(N):
                step_noise[i] = randn_tensor((B, Cl, T, h, w), generator=None, device=device, dtype=torch.float32)
        storage = self.latent_storage_dtype or torch.float32       # cast_latents(latents) with no default: fp32 stays fp32
        plan = self.engine.plan(B, 2 if do_cfg else 1, T, h, w, prompt_embeds.shape[1], N)
        plan_2 = self.engine_2.plan(B, 2 if do_cfg else 1, T, h, w, prompt_embeds.shape[1], N) if two else None
        sampler = None
        if eval_mode:
            if compute_log_prob or any(k != "noise_level" for k in extra_call_back_kwargs):
                raise NotImplementedError("mi355_flow: evaluation-mode Wan sampling returns latents only (the reference's UniPC step yields neither "
                                          "a log-prob nor per-step callback tensors: unipc_multistep.py:282-285)")
            sampler = self._rollout_eval_stepwise
        elif two:
            # two experts: per-step engine calls (each step picks its expert and guidance by the boundary rule; still all-HIP)
            sampler = self._rollout_stepwise
        traj, final = self._rollout_and_collect(plan, timesteps, N, guidance_scale, latents, storage, step_noise,
                                                (prompt_embeds, negative_prompt_embeds if do_cfg else None), compute_log_prob,
                                                extra_call_back_kwargs, trajectory_indices, sampler=sampler, plan_2=plan_2, guidance_2=g2)
        videos = self.decode_latents(final, output_type="pt")
        return [
            self._sample_cls(
                timesteps=timesteps,
                **traj.per_sample(b),
                video=videos[b] if videos is not None else None,
                height=height, width=width,
                prompt=prompt[b] if isinstance(prompt, list) else prompt,
                prompt_ids=prompt_ids[b] if prompt_ids is not None else None,
                prompt_embeds=prompt_embeds[b],
                negative_prompt=negative_prompt[b] if isinstance(negative_prompt, list) else negative_prompt,
                negative_prompt_ids=negative_prompt_ids[b] if negative_prompt_ids is not None else None,
                negative_prompt_embeds=negative_prompt_embeds[b] if negative_prompt_embeds is not None else None,
            )
            for b in range(B)
        ]

    def _rollout_eval_stepwise(self, plan, ts, sig, eta, guidance, latents, storage, step_noise, pe, ne, compute_log_prob, extra_keys,
                               plan_2=None, guidance_2=None):
        """`_rollout_eval` as a sampler of `_rollout_stepwise`'s signature: no log-probs, no per-step outputs."""
        all_lat = self._rollout_eval(plan, ts, sig, guidance, latents, storage, pe, ne, plan_2=plan_2, guidance_2=guidance_2)
        return all_lat, torch.full((len(ts), latents.shape[0]), float("nan"), device=latents.device), None

    def _rollout_eval(self, plan, ts, sig, guidance, latents, storage, pe, ne, plan_2=None, guidance_2=None):
        """Evaluation-mode sampling (reference: the loop of wan2_t2v.py:346-375 with `scheduler.step` in its `is_eval` branch,
        unipc_multistep.py:282-285 = diffusers' UniPC multistep predictor-corrector): one engine forward per step (per expert and guidance by
        the boundary rule, like the rollout), then the solver step on the GPU -- `mi355_unipc_convert` + `mi355_op_lincomb` with host-side
        coefficients (mi355_flow/unipc.py).  Deterministic: no noise is drawn."""
        from .unipc import UniPCSampler
        cfg = self.scheduler.config
        get = (lambda k, d: cfg.get(k, d)) if hasattr(cfg, "get") else (lambda k, d: getattr(cfg, k, d))
        if get("prediction_type", "flow_prediction") != "flow_prediction" or not get("predict_x0", True):
            raise NotImplementedError("mi355_flow: the native UniPC sampler implements flow prediction with predict_x0 (the Wan pipelines' setting)")
        if get("thresholding", False) or get("solver_p", None) is not None:
            raise NotImplementedError("mi355_flow: UniPC thresholding / a custom predictor solver are not implemented")
        solver = UniPCSampler(sig, solver_order=int(get("solver_order", 2)), solver_type=str(get("solver_type", "bh2")),
                              lower_order_final=bool(get("lower_order_final", True)), disable_corrector=tuple(get("disable_corrector", ()) or ()),
                              sample_dtype=self.cast_latents(latents[:0], storage).dtype)
        N, B = len(ts), latents.shape[0]
        cur = self.cast_latents(latents, storage)
        all_lat = [cur]
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)          # noqa: E731
        bt = self._boundary_timestep()
        for i in range(N):
            low = plan_2 is not None and bt is not None and ts[i] < bt
            pl, gd = (plan_2, guidance_2) if low else (plan, guidance)
            cfg_i = ne is not None and gd > 1.0
            if not cfg_i and pl.n_cfg == 2:
                pl = pl.engine.plan(B, 1, pl.T, pl.h, pl.w, pl.n_text, 1)
            v = pl.transformer_forward(cur, f32(ts[i]).reshape(1), ne if cfg_i else pe, pe if cfg_i else None)
            vu, vt = (v[:B], v[B:]) if cfg_i else (None, v)
            nxt = solver.step(i, vt.reshape(cur.shape), vu.reshape(cur.shape) if vu is not None else None, gd, cur)
            cur = self.cast_latents(nxt, storage)
            all_lat.append(cur)
        return all_lat

    def _rollout_stepwise(self, plan, ts, sig, eta, guidance, latents, storage, step_noise, pe, ne, compute_log_prob, extra_keys, plan_2=None,
                          guidance_2=None):
        """Per-step engine calls (still all-HIP) for rollouts that ask for per-step callback tensors, and for two-expert pipelines."""
        B = latents.shape[0]

        def predict(i, cur):
            bt = self._boundary_timestep()
            low = plan_2 is not None and bt is not None and ts[i] < bt
            pl, gd = (plan_2, guidance_2) if low else (plan, guidance)
            cfg_i = ne is not None and gd > 1.0          # the reference decides CFG per expert (wan2_t2v.py:489-498)
            if not cfg_i and pl.n_cfg == 2:
                pl = pl.engine.plan(B, 1, pl.T, pl.h, pl.w, pl.n_text, 1)
            v = pl.transformer_forward(cur, torch.tensor(float(ts[i]), dtype=torch.float32).reshape(1), ne if cfg_i else pe, pe if cfg_i else None)
            return (v[B:], v[:B], gd) if cfg_i else (v, None, gd)

        return self._stepwise(ts, sig, eta, latents, storage, step_noise, compute_log_prob, extra_keys, predict)

    # ------------------------------------------------------------------ single step / replay (wan2_t2v.py:426-543)
    def forward(
        self,
        t: torch.Tensor,
        latents: torch.Tensor,
        prompt_embeds: torch.Tensor,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        guidance_scale: float = 5.0,
        guidance_scale_2: Optional[float] = None,
        t_next: Optional[torch.Tensor] = None,
        next_latents: Optional[torch.Tensor] = None,
        noise_level: Optional[float] = None,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        return_kwargs: List[str] = ["noise_pred", "next_latents", "next_latents_mean", "std_dev_t", "dt", "log_prob"],
        boundary_timestep: Optional[float] = None,
    ) -> SDESchedulerOutput:
        kw = dict(t=t, latents=latents, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, guidance_scale=guidance_scale,
                  guidance_scale_2=guidance_scale_2, t_next=t_next, next_latents=next_latents, noise_level=noise_level,
                  attention_kwargs=attention_kwargs, compute_log_prob=compute_log_prob, return_kwargs=return_kwargs, boundary_timestep=boundary_timestep)
        if not WanEngine.native_backward_enabled:          # MI355_WAN_NATIVE_BACKWARD=0 opts out of the native backward
            return self._forward_nograd(**kw)
        # optimize() (trainers/grpo.py:263): the replay WITH autograd runs on the engine's differentiable forward + native backward
        # (mi355_flow.autograd.wan_replay) when its backward covers the trainable set of the transformer THIS step runs on (Wan2.2: the
        # expert the timestep selects, wan2_t2v.py:476-487)
        return self._forward_dispatch(kw, replay_host=lambda: self._replay_host(self._expert(
            float(torch.as_tensor(t, dtype=torch.float32).reshape(-1)[0]), guidance_scale, guidance_scale_2, boundary_timestep)[0]))

    def _replay_host(self, eng):
        """What `mi355_flow.autograd` differentiates against for a step on `eng`: this adapter (single transformer / the high-noise expert), or
        the low-noise expert's (engine, live module binding) pair of a two-expert Wan2.2 pipeline."""
        if eng is self.engine or self.engine_2 is None:
            return self
        import types
        return types.SimpleNamespace(engine=self.engine_2, _live_weights=getattr(self, "_live_weights_2", None),
                                     _sync_weights=getattr(self, "_sync_weights", None))

    def _forward_impl(self, t, latents, prompt_embeds, negative_prompt_embeds, guidance_scale, guidance_scale_2, t_next, next_latents, noise_level,
                      attention_kwargs, compute_log_prob, return_kwargs, boundary_timestep, grad: bool, host=None) -> SDESchedulerOutput:
        self._before_engine_call()
        if attention_kwargs:
            raise NotImplementedError("mi355_flow: attention_kwargs are not supported by the native engine")
        if boundary_timestep is not None and self.engine_2 is None:
            raise ValueError("mi355_flow: boundary_timestep needs a two-expert (Wan2.2) adapter: no second transformer is bound")
        dev = latents.device
        B, _, T, h, w = latents.shape
        t = torch.as_tensor(t, device=dev, dtype=torch.float32).reshape(-1)
        t0 = t[0]                                       # `t = t[0] if t.ndim == 1 else t`: one scalar timestep per call
        if t_next is not None:
            t_next = torch.as_tensor(t_next, device=dev, dtype=torch.float32).reshape(-1)[0]
        eng, guidance_scale = self._expert(float(t0), guidance_scale, guidance_scale_2, boundary_timestep)
        do_cfg = negative_prompt_embeds is not None and guidance_scale > 1.0
        plan = eng.plan(B, 2 if do_cfg else 1, T, h, w, prompt_embeds.shape[1], 1)
        enc_a, enc_b = (negative_prompt_embeds, prompt_embeds) if do_cfg else (prompt_embeds, None)
        sched = self.scheduler
        if noise_level is None and not (sched.is_eval or sched.dynamics_type == "ODE"):
            noise_level = sched.get_noise_level_for_timestep(float(t0))          # Wan's schedulers look the level up by timestep
        if grad:
            from .autograd import wan_replay
            return self._scheduler_step(t0, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs, replay=(
                wan_replay, host if host is not None else self, plan,
                dict(train_args=(latents, t0.reshape(1), enc_a, enc_b), cfg_guidance=float(guidance_scale) if do_cfg else None)))
        v = plan.transformer_forward(latents, t0.reshape(1), enc_a, enc_b)
        return self._scheduler_step(t0, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs,
                                    v=(v[B:], v[:B], guidance_scale) if do_cfg else (v, None, guidance_scale))


class Wan2T2VNativeAdapter(StandaloneAdapterBase, WanRolloutMixin):
    """Standalone Wan2.1 T2V adapter (no Flow-Factory import): engine + UniPC-SDE scheduler (+ optional video decoder callable)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: Optional[WanConfig] = None,
                 scheduler: Optional[UniPCMultistepSDEScheduler] = None, latent_storage_dtype: Optional[str] = "fp16",
                 transformer_dtype: torch.dtype = torch.bfloat16, device: Union[str, torch.device] = "cuda",
                 video_decode: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                 state_dict_2: Optional[Dict[str, torch.Tensor]] = None, boundary_ratio: Optional[float] = None,
                 vae_state_dict: Optional[Dict[str, torch.Tensor]] = None, vae_config=None, vae_max_batch: int = 1):
        from .vae import WanVAEConfig, WanVAEDecoder
        self._init_engine(WanEngine, config or WanConfig(),
                          scheduler or UniPCMultistepSDEScheduler(flow_shift=3.0, sde_steps=[1, 2, 3], num_sde_steps=1),
                          latent_storage_dtype, transformer_dtype, device)
        self._bind(state_dict)
        if state_dict_2 is not None:            # Wan2.2: low-noise expert (`transformer_2`), same architecture
            if boundary_ratio is None:
                raise ValueError("mi355_flow: a two-expert Wan2.2 adapter needs `boundary_ratio` (pipeline.config.boundary_ratio)")
            self.engine_2 = WanEngine(config or WanConfig())
            self.engine_2.bind_state_dict(state_dict_2)
            self.engine_2.ready()
            self.boundary_ratio = float(boundary_ratio)
        self._video_decode = video_decode
        self._init_vae(WanVAEDecoder, vae_config or WanVAEConfig(), vae_state_dict, vae_max_batch)

    def encode_prompt(self, *a, **k):
        raise RuntimeError("mi355_flow standalone adapter has no text encoder: pass prompt_embeds (and negative_prompt_embeds for CFG)")

    def decode_latents(self, latents: torch.Tensor, output_type: str = "pt"):
        """wan2_t2v.py:215-230: de-normalise, vae.decode, postprocess_video -> (B, F, 3, H, W) in [0, 1]."""
        if self.vae_decoder is not None:
            if output_type not in ("pt", "np"):
                raise ValueError("mi355_flow standalone adapter decodes to 'pt' or 'np'")
            vid = self.vae_decoder.decode(latents, postprocess=True, out_dtype=torch.float32, max_batch=self.vae_max_batch)
            return vid if output_type == "pt" else vid.permute(0, 1, 3, 4, 2).cpu().numpy()
        return self._video_decode(latents) if self._video_decode is not None else None

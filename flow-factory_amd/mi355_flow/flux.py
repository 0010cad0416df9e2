"""FLUX.1 rollout on the native engine (mi355_flux_*): host mirror of `Flux1Adapter.inference` / `.forward`
(reference src/flow_factory/models/flux/flux1.py:151-289, :294-346) -- SURVEY.md 8(f) row N3.

Same contract as the SD3.5 path (`mi355_flow.adapter`): reference argument names and defaults, the reference's RNG draw
order, trajectory / log-prob / callback collectors, no CPU or PyTorch fallback.  FLUX specifics kept from the reference:
packed latents `(B, h/2*w/2, 64)`, `img_ids` from `prepare_latents`, `timestep = t / 1000`, embedded guidance (no CFG,
no negative prompt), dynamic-shift `mu` from the image sequence length.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import FluxCfg
from .engine import EngineBase, PlanBase, _bf16c, _ptr, _stream, dtype_code, sde_step
from .host import _DTYPE_MAP, VAE_SCALE_FACTOR, RolloutMixinBase, StandaloneAdapterBase  # noqa: F401  (re-exported)
from .samples import Flux1KontextSample, Flux1Sample
from .scheduler import FlowMatchEulerDiscreteSDEScheduler, SDESchedulerOutput, randn_tensor, set_scheduler_timesteps
from .trajectory import TrajectoryIndicesType


@dataclass
class FluxConfig:
    """diffusers FluxTransformer2DModel config fields the engine needs (FLUX.1-dev defaults)."""
    in_channels: int = 64
    num_layers: int = 19
    num_single_layers: int = 38
    num_attention_heads: int = 24
    attention_head_dim: int = 128
    joint_attention_dim: int = 4096
    pooled_projection_dim: int = 768
    guidance_embeds: bool = True
    axes_dims_rope: Tuple[int, int, int] = (16, 56, 56)
    time_proj_dim: int = 256
    eps: float = 1e-6

    @property
    def dim(self) -> int:
        return self.num_attention_heads * self.attention_head_dim

    def to_c(self) -> FluxCfg:
        return FluxCfg(self.in_channels, self.num_layers, self.num_single_layers, self.num_attention_heads, self.attention_head_dim,
                       self.joint_attention_dim, self.pooled_projection_dim, int(self.guidance_embeds), self.time_proj_dim,
                       (C.c_int32 * 3)(*self.axes_dims_rope), self.eps)


def pack_latents(lat: torch.Tensor) -> torch.Tensor:
    """FluxPipeline._pack_latents: (B, C, h, w) -> (B, h/2*w/2, 4C)."""
    B, Cc, h, w = lat.shape
    return lat.view(B, Cc, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (h // 2) * (w // 2), Cc * 4)


def unpack_latents(x: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """FluxPipeline._unpack_latents on the latent grid: (B, h/2*w/2, 4C) -> (B, C, h, w)."""
    B, _, ch = x.shape
    return x.view(B, h // 2, w // 2, ch // 4, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, ch // 4, h, w)


def prepare_latent_image_ids(hp: int, wp: int, device, dtype) -> torch.Tensor:
    """FluxPipeline._prepare_latent_image_ids: (hp*wp, 3) = [0, row, col]."""
    ids = torch.zeros(hp, wp, 3)
    ids[..., 1] = ids[..., 1] + torch.arange(hp)[:, None]
    ids[..., 2] = ids[..., 2] + torch.arange(wp)[None, :]
    return ids.reshape(hp * wp, 3).to(device=device, dtype=dtype)


def split_kontext_ids(latent_ids: torch.Tensor) -> Tuple[int, int, int, int]:
    """The packed grids `(hp, wp, hc, wc)` behind FLUX.1 Kontext's `latent_ids = cat([latent_ids, image_ids])` (reference
    flux1_kontext.py:277-281, :412).  The engine builds its rotary table from the grid sizes alone, so ids it would not reproduce are refused:
    the rows with first id 0 must be `prepare_latent_image_ids(hp, wp)` exactly, the rows with first id 1 the same construction on `hc x wc`
    with the first id set to 1, in that order, and there must be nothing else (several condition images, offset grids, shuffled rows)."""
    ids = torch.as_tensor(latent_ids).detach().to(device="cpu", dtype=torch.float32)
    if ids.dim() != 2 or ids.shape[1] != 3:
        raise ValueError(f"mi355_flow: latent_ids must be (Ni + Nc, 3), got {tuple(ids.shape)}")
    first = ids[:, 0]
    n0 = int((first == 0).sum())
    kinds = sorted(set(first.tolist()))
    if kinds != [0.0, 1.0]:
        raise ValueError(f"mi355_flow: latent_ids must hold target rows (first id 0) and ONE condition image (first id 1); found first ids {kinds}")
    if not bool((first[:n0] == 0).all()):
        raise ValueError("mi355_flow: latent_ids mixes target rows (first id 0) and condition rows (first id 1); the target rows must come first")

    def grid(rows: torch.Tensor, what: str, lead: float) -> Tuple[int, int]:
        hg, wg = int(rows[:, 1].max()) + 1, int(rows[:, 2].max()) + 1
        want = prepare_latent_image_ids(hg, wg, "cpu", torch.float32)
        want[:, 0] = lead
        if rows.shape != want.shape or not torch.equal(rows, want):
            raise ValueError(f"mi355_flow: the {what} rows of latent_ids are not the ({lead:g}, row, col) raster of one image: {rows.shape[0]} rows, "
                             f"rows {int(rows[:, 1].min())}..{hg - 1}, cols {int(rows[:, 2].min())}..{wg - 1} (shuffled, offset or several images)")
        return hg, wg

    hp, wp = grid(ids[:n0], "target", 0.0)
    hc, wc = grid(ids[n0:], "condition", 1.0)
    return hp, wp, hc, wc


def model_scalar(value: float, dtype: torch.dtype) -> float:
    """`x.to(hidden_states.dtype) * 1000` of FluxTransformer2DModel.forward for a python / fp32 scalar."""
    return float((torch.tensor(float(value), dtype=torch.float32).to(dtype) * 1000).float())


class FluxPlan(PlanBase):
    _PRE = "flux_"
    _CREATE = "plan_create_cond"      # a plain plan is its (0, 0) case, in C as well

    def __init__(self, engine: FluxEngine, batch: int, latent_h: int, latent_w: int, n_text: int, cond_h: int, cond_w: int, max_steps: int):
        """`cond_h x cond_w`: the unpacked latent grid of a FLUX.1 Kontext condition image, or 0 x 0.  Its `Nc` tokens follow each sample's `Ni`
        target tokens through the blocks (`Nx` rows per sample); `Ni`, `dv_shape` and every latent shape stay what the scheduler step sees."""
        self.batch, self.h, self.w, self.n_text = batch, latent_h, latent_w, n_text
        self.Ni = (latent_h // 2) * (latent_w // 2)
        self.Nc = (cond_h // 2) * (cond_w // 2)
        self.Nx = self.Ni + self.Nc
        super().__init__(engine, (batch, latent_h, latent_w, cond_h, cond_w, n_text), max_steps)
        self.dv_shape = (batch, self.Ni, self.C)

    def _condition(self, image_latents: Optional[torch.Tensor], device) -> Tuple[str, tuple]:
        """(symbol suffix, trailing C arguments) for this call's condition latents: per call, never plan state.  The pairing of plan and entry
        point is the engine's to refuse; the shape is checked here."""
        if image_latents is None:
            return "", ()
        if self.Nc and tuple(image_latents.shape) != (self.batch, self.Nc, self.C):
            raise ValueError(f"mi355_flow: image_latents must be {(self.batch, self.Nc, self.C)} for this plan, got {tuple(image_latents.shape)}")
        il = image_latents.to(device).contiguous()
        self._cond_keepalive = il        # read asynchronously by the call that follows
        return "_cond", (_ptr(il), dtype_code(il.dtype))

    def rope_table(self) -> torch.Tensor:
        """The plan's rotary table `(n_text + Ni + Nc, 64, 2)` = (cos, sin) fp32, on the host."""
        out = torch.empty((self.n_text + self.Nx, 64, 2), dtype=torch.float32)
        self._call("plan_rope_table", self._h, out.data_ptr())
        return out

    def _forward(self, symbol: str, latents, t_model, guidance_model, prompt_embeds, pooled, image_latents=None) -> torch.Tensor:
        B, dev = self.batch, latents.device
        assert latents.shape == (B, self.Ni, self.C), latents.shape
        suffix, tail = self._condition(image_latents, dev)
        tm = t_model.to(device=dev, dtype=torch.float32).reshape(-1)
        tm = (tm.expand(B) if tm.numel() == 1 else tm).contiguous()
        gm = None
        if guidance_model is not None:
            gm = guidance_model.to(device=dev, dtype=torch.float32).reshape(-1)
            gm = (gm.expand(B) if gm.numel() == 1 else gm).contiguous()
        out = torch.empty((B, self.Ni, self.C), device=dev, dtype=torch.bfloat16)
        latents = latents.contiguous()
        pe, pp = _bf16c(prompt_embeds), _bf16c(pooled)
        self._call(symbol + suffix, self._h, _stream(), _ptr(latents), dtype_code(latents.dtype), _ptr(tm), _ptr(gm), _ptr(pe), _ptr(pp), _ptr(out),
                   *tail)
        return out

    def transformer_forward(self, latents: torch.Tensor, t_model: torch.Tensor, guidance_model: Optional[torch.Tensor],
                            prompt_embeds: torch.Tensor, pooled: torch.Tensor, image_latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """latents (B, Ni, 64) packed; t_model / guidance_model (B,) = the values the network embeds; image_latents (B, Nc, 64) on a
        condition plan (the velocity is that of the Ni target tokens)."""
        return self._forward("forward", latents, t_model, guidance_model, prompt_embeds, pooled, image_latents)

    # ---------------------------------------------------------------- differentiable forward (optimize() replay)
    def forward_train(self, latents: torch.Tensor, t_model: torch.Tensor, guidance_model: Optional[torch.Tensor],
                      prompt_embeds: torch.Tensor, pooled: torch.Tensor, image_latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mi355_flux_forward_train: `transformer_forward` on per-block activation buffers -- the same kernel binaries, so the velocity is
        bit-identical -- keeping what `backward` needs in the plan's training stash (ONE per plan; every call takes a serial number)."""
        out = self._forward("forward_train", latents, t_model, guidance_model, prompt_embeds, pooled, image_latents)
        self._train_serial += 1
        return out

    def rollout(self, timesteps: Sequence[float], sigmas: Sequence[float], noise_levels: Sequence[float], dynamics: str,
                guidance_scale: float, init_latents: torch.Tensor, storage_dtype: torch.dtype, step_noise: Optional[torch.Tensor],
                prompt_embeds: torch.Tensor, pooled: torch.Tensor, image_latents: Optional[torch.Tensor] = None,
                keep_positions: Optional[Sequence[int]] = None, compute_log_prob: bool = True):
        """Returns (kept_latents [n_kept, B, Ni, 64] storage dtype, log_probs [N, B] fp32 (nan where not computed), final).
        `image_latents` (B, Nc, 64) on a condition plan: embedded once for the whole rollout."""
        shape = (self.batch, self.Ni, self.C)
        assert tuple(init_latents.shape) == shape, init_latents.shape
        pe, pp = _bf16c(prompt_embeds), _bf16c(pooled)
        suffix, tail = self._condition(image_latents, init_latents.device)
        return self._rollout(shape, timesteps, sigmas, noise_levels, dynamics, guidance_scale, init_latents, storage_dtype, step_noise,
                             (_ptr(pe), _ptr(pp)), keep_positions, compute_log_prob, symbol="rollout" + suffix, tail=tail)


class FluxEngine(EngineBase):
    """Owns the packed bf16 copy of the FLUX transformer weights (mi355_flux).  `plan(batch, latent_h, latent_w, n_text, max_steps)`, and
    `plan(..., cond=(hc, wc))` for FLUX.1 Kontext: the same transformer with a condition image's tokens behind the target's."""

    _ABI, _WHAT, _PLAN = "flux", "FLUX transformer", FluxPlan

    def __init__(self, cfg: FluxConfig = FluxConfig()):
        super().__init__(cfg)

    def plan(self, batch: int, latent_h: int, latent_w: int, n_text: int, max_steps: int, cond: Optional[Tuple[int, int]] = None):
        """The cached workspace for one shape; a condition plan (`cond`: the unpacked latent grid of the condition image) lives beside the
        plain plan of the same target shape."""
        cond_h, cond_w = cond or (0, 0)
        return super().plan(batch, latent_h, latent_w, n_text, int(cond_h), int(cond_w), max_steps)


class FluxRolloutMixin(RolloutMixinBase):
    """`inference()` / `forward()` of `Flux1Adapter` (reference models/flux/flux1.py:151-289, :294-346) on the engine.  Host classes
    provide `engine` (FluxEngine), `scheduler`, `device`, `latent_storage_dtype`, `encode_prompt`, `decode_latents(latents, height,
    width, output_type)`.  Used by the standalone `Flux1NativeAdapter` below and, mixed in FRONT of the reference's own `Flux1Adapter`,
    by `mi355_flow.flow_factory_plugin.Flux1NativeAdapter`."""

    _FAMILY = "FLUX.1"
    _sample_cls = Flux1Sample
    _set_timesteps = staticmethod(set_scheduler_timesteps)

    def _sde_step(self, *a, **k):
        return sde_step(*a, **k)          # this module's name, looked up per call

    # ------------------------------------------------------------------ rollout (flux1.py:151-289)
    @torch.no_grad()
    def inference(
        self,
        prompt: Optional[Union[str, List[str]]] = None,
        height: int = 512,
        width: int = 512,
        num_inference_steps: int = 28,
        guidance_scale: float = 3.5,
        generator: Optional[torch.Generator] = None,
        prompt_ids: Optional[torch.Tensor] = None,
        prompt_embeds: Optional[torch.Tensor] = None,
        pooled_prompt_embeds: Optional[torch.Tensor] = None,
        joint_attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        extra_call_back_kwargs: List[str] = [],
        trajectory_indices: TrajectoryIndicesType = "all",
    ) -> List[Flux1Sample]:
        self._before_engine_call()
        device = self.device
        self._check_joint_attention_kwargs(joint_attention_kwargs)
        if prompt_embeds is None:
            enc = self.encode_prompt(prompt)
            prompt_embeds, pooled_prompt_embeds, prompt_ids = enc["prompt_embeds"], enc["pooled_prompt_embeds"], enc["prompt_ids"]
        else:
            prompt_embeds, pooled_prompt_embeds = prompt_embeds.to(device), pooled_prompt_embeds.to(device)
        B = len(prompt_embeds)
        dtype = prompt_embeds.dtype
        Cl = self.engine.cfg.in_channels // 4
        # FluxPipeline.prepare_latents: height = 2 * (height // (vae_scale_factor * 2))
        h = 2 * (int(height) // (VAE_SCALE_FACTOR * 2))
        w = 2 * (int(width) // (VAE_SCALE_FACTOR * 2))
        N = int(num_inference_steps)
        Ni = (h // 2) * (w // 2)

        # RNG in the reference's order: prepare_latents draws (B, 16, h, w) in the prompt dtype and packs it; the scheduler then
        # draws one fp32 tensor of the PACKED shape per step (randn_tensor(noise_pred.shape)), also when noise_level == 0
        # (no step draws at all under ODE dynamics: the reference's ODE branch draws nothing)
        dyn = self.scheduler.dynamics_type
        latents = pack_latents(randn_tensor((B, Cl, h, w), generator=generator, device=device, dtype=dtype))
        latent_image_ids = prepare_latent_image_ids(h // 2, w // 2, device, dtype)
        step_noise = None
        if dyn != "ODE":
            step_noise = torch.empty((N, B, Ni, Cl * 4), device=device, dtype=torch.float32)
            for i in range(N):
                step_noise[i] = randn_tensor((B, Ni, Cl * 4), generator=None, device=device, dtype=torch.float32)

        timesteps = self._set_timesteps(self.scheduler, N, seq_len=latents.shape[1], device=device)
        storage = self.latent_storage_dtype or dtype
        plan = self.engine.plan(B, h, w, prompt_embeds.shape[1], N)
        traj, final = self._rollout_and_collect(plan, timesteps, N, guidance_scale, latents, storage, step_noise,
                                                (prompt_embeds, pooled_prompt_embeds), compute_log_prob, extra_call_back_kwargs,
                                                trajectory_indices)
        images = self.decode_latents(final, height, width, output_type="pt")
        return [
            self._sample_cls(
                timesteps=timesteps,
                **traj.per_sample(b),
                prompt=prompt[b] if isinstance(prompt, list) else prompt,
                prompt_ids=prompt_ids[b] if prompt_ids is not None else None,
                prompt_embeds=prompt_embeds[b],
                pooled_prompt_embeds=pooled_prompt_embeds[b],
                height=height, width=width,
                image=images[b] if images is not None else None,
                img_ids=latent_image_ids,
            )
            for b in range(B)
        ]

    def _rollout_stepwise(self, plan, ts, sig, eta, guidance, latents, storage, step_noise, pe, pp, compute_log_prob, extra_keys,
                          image_latents=None):
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)          # noqa: E731
        gm = (torch.tensor(float(guidance)).to(storage) * 1000).float().reshape(1) if self.engine.cfg.guidance_embeds else None
        il = () if image_latents is None else (image_latents,)

        def predict(i, cur):
            tm = ((f32(ts[i]) / f32(1000.0)).to(storage) * 1000).float().reshape(1)      # as mi355_flux_rollout's host math
            return plan.transformer_forward(cur, tm, gm, pe, pp, *il), None, 1.0

        return self._stepwise(ts, sig, eta, latents, storage, step_noise, compute_log_prob, extra_keys, predict)

    # ------------------------------------------------------------------ single step / replay (flux1.py:294-346)
    def forward(
        self,
        t: torch.Tensor,
        latents: torch.Tensor,
        prompt_embeds: torch.Tensor,
        pooled_prompt_embeds: torch.Tensor,
        img_ids: Optional[torch.Tensor] = None,
        t_next: Optional[torch.Tensor] = None,
        next_latents: Optional[torch.Tensor] = None,
        guidance_scale: Union[float, List[float]] = 3.5,
        noise_level: Optional[float] = None,
        joint_attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        return_kwargs: List[str] = ["noise_pred", "next_latents", "next_latents_mean", "std_dev_t", "dt", "log_prob"],
        height: Optional[int] = None,
        width: Optional[int] = None,
    ) -> SDESchedulerOutput:
        # optimize() (trainers/grpo.py:263): the replay of a stored transition WITH autograd runs on the engine's differentiable forward +
        # native backward (mi355_flow.autograd.flux_replay) when its backward covers the trainable set; the matching-loss trainers'
        # forward without a stored transition (noise_pred only) runs the same path with the log-prob switched off
        return self._forward_dispatch(dict(
            t=t, latents=latents, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds, img_ids=img_ids, t_next=t_next,
            next_latents=next_latents, guidance_scale=guidance_scale, noise_level=noise_level, joint_attention_kwargs=joint_attention_kwargs,
            compute_log_prob=compute_log_prob, return_kwargs=return_kwargs, height=height, width=width))

    def _forward_impl(self, t, latents, prompt_embeds, pooled_prompt_embeds, img_ids, t_next, next_latents, guidance_scale, noise_level,
                      joint_attention_kwargs, compute_log_prob, return_kwargs, height, width, grad: bool, host=None) -> SDESchedulerOutput:
        self._before_engine_call()
        self._check_joint_attention_kwargs(joint_attention_kwargs)
        B, Ni, _ = latents.shape
        dev = latents.device
        # the latent grid is recovered from img_ids (rows / cols) when given, else it must be square or passed explicitly
        if img_ids is not None:
            hp, wp = int(img_ids[:, 1].max().item()) + 1, int(img_ids[:, 2].max().item()) + 1
        elif height is not None and width is not None:
            hp, wp = int(height) // 16, int(width) // 16
        else:
            hp = wp = int(round(Ni ** 0.5))
        if hp * wp != Ni:
            raise ValueError(f"mi355_flow: cannot recover the latent grid of {Ni} packed tokens (pass img_ids or height/width)")
        plan = self.engine.plan(B, 2 * hp, 2 * wp, prompt_embeds.shape[1], 1)
        t = torch.as_tensor(t, device=dev, dtype=torch.float32).reshape(-1)
        # timestep = t.expand(B) / 1000 (fp32); the model does `.to(latents.dtype) * 1000` (rounded again to that dtype)
        tm = ((t.double() / 1000).float().to(latents.dtype) * 1000).float()   # exact quotient, as the fused rollout's host math
        g = torch.as_tensor(guidance_scale, device=dev, dtype=latents.dtype).reshape(-1)
        gm = (g * 1000).float()
        gm = gm if self.engine.cfg.guidance_embeds else None
        if t_next is not None:
            t_next = torch.as_tensor(t_next, device=dev, dtype=torch.float32).reshape(-1)
        if grad:
            from .autograd import flux_replay
            return self._scheduler_step(t, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs,
                                        replay=(flux_replay, host, plan, dict(tm=tm, gm=gm, prompt_embeds=prompt_embeds, pooled=pooled_prompt_embeds)))
        v = plan.transformer_forward(latents, tm, gm, prompt_embeds, pooled_prompt_embeds)
        return self._scheduler_step(t, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs, v=(v, None, 1.0))


class FluxKontextRolloutMixin(FluxRolloutMixin):
    """`inference()` / `forward()` of `Flux1KontextAdapter` (reference models/flux/flux1_kontext.py:337-506, :510-589) on the engine: the
    FLUX.1 transformer with the condition image's packed latents behind the target's in the image stream, rotary ids (1, row, col) on the
    condition image's own grid, and only the target rows of the prediction in the scheduler step.  Host classes provide what
    `FluxRolloutMixin` asks for plus `encode_image(images, condition_image_size, generator)` -> `condition_images`, `image_latents`,
    `image_ids` and `_standardize_image_input(images, output_type)`."""

    _FAMILY = "FLUX.1 Kontext"
    _sample_cls = Flux1KontextSample

    # ------------------------------------------------------------------ rollout (flux1_kontext.py:337-506)
    @torch.no_grad()
    def inference(
        self,
        images: Optional[Any] = None,
        prompt: Optional[Union[str, List[str]]] = None,
        condition_image_size: Optional[Union[int, Tuple[int, int]]] = None,
        num_inference_steps: int = 50,
        height: int = 1024,
        width: int = 1024,
        guidance_scale: float = 3.5,
        generator: Optional[torch.Generator] = None,
        max_sequence_length: int = 512,
        prompt_ids: Optional[torch.Tensor] = None,
        prompt_embeds: Optional[torch.Tensor] = None,
        pooled_prompt_embeds: Optional[torch.Tensor] = None,
        condition_images: Optional[Any] = None,
        image_latents: Optional[torch.Tensor] = None,
        image_ids: Optional[torch.Tensor] = None,
        joint_attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        extra_call_back_kwargs: List[str] = [],
        trajectory_indices: TrajectoryIndicesType = "all",
    ) -> List[Flux1KontextSample]:
        self._before_engine_call()
        device = self.device
        self._check_joint_attention_kwargs(joint_attention_kwargs)
        if prompt_embeds is None or pooled_prompt_embeds is None:
            enc = self.encode_prompt(prompt=prompt, max_sequence_length=max_sequence_length)
            prompt_embeds, pooled_prompt_embeds, prompt_ids = enc["prompt_embeds"], enc["pooled_prompt_embeds"], enc["prompt_ids"]
        else:
            prompt_embeds, pooled_prompt_embeds = prompt_embeds.to(device), pooled_prompt_embeds.to(device)
        # the condition arrives encoded (the reference's preprocessing stores all three), else it is encoded here -- before the latents are
        # drawn, as in the reference: the VAE's sampling consumes the same generator.  (Encoded latents and ids without the images they came
        # from, and no `images` to encode: the reference would fail in encode_image; here the samples simply carry no condition image.)
        if image_latents is None or image_ids is None or (condition_images is None and images is not None):
            enc = self.encode_image(images=images, condition_image_size=condition_image_size, generator=generator)
            condition_images, image_latents, image_ids = enc["condition_images"], enc["image_latents"], enc["image_ids"]
        else:
            if condition_images is not None:
                condition_images = self._standardize_image_input(condition_images, output_type="pt")
            image_latents, image_ids = image_latents.to(device), image_ids.to(device)
        if image_ids.dim() == 3:
            image_ids = image_ids[0]
        B = len(prompt_embeds)
        dtype = prompt_embeds.dtype
        Cl = self.engine.cfg.in_channels // 4
        h = 2 * (int(height) // (VAE_SCALE_FACTOR * 2))
        w = 2 * (int(width) // (VAE_SCALE_FACTOR * 2))
        N = int(num_inference_steps)
        Ni = (h // 2) * (w // 2)

        # RNG as FluxRolloutMixin.inference: the packed initial latents, then one fp32 draw of the TARGET shape per step (the scheduler sees
        # noise_pred[:, :Ni])
        dyn = self.scheduler.dynamics_type
        latents = pack_latents(randn_tensor((B, Cl, h, w), generator=generator, device=device, dtype=dtype))
        latent_ids = torch.cat([prepare_latent_image_ids(h // 2, w // 2, device, dtype), image_ids.to(device=device, dtype=dtype)], dim=0)
        _, _, hc, wc = split_kontext_ids(latent_ids)
        step_noise = None
        if dyn != "ODE":
            step_noise = torch.empty((N, B, Ni, Cl * 4), device=device, dtype=torch.float32)
            for i in range(N):
                step_noise[i] = randn_tensor((B, Ni, Cl * 4), generator=None, device=device, dtype=torch.float32)

        timesteps = self._set_timesteps(self.scheduler, N, seq_len=latents.shape[1], device=device)      # Ni: the condition does not shift mu
        storage = self.latent_storage_dtype or dtype
        plan = self.engine.plan(B, h, w, prompt_embeds.shape[1], N, cond=(2 * hc, 2 * wc))
        traj, final = self._rollout_and_collect(plan, timesteps, N, guidance_scale, latents, storage, step_noise,
                                                (prompt_embeds, pooled_prompt_embeds, image_latents), compute_log_prob,
                                                extra_call_back_kwargs, trajectory_indices)
        generated = self.decode_latents(final, height, width, output_type="pt")
        return [
            self._sample_cls(
                timesteps=timesteps,
                **traj.per_sample(b),
                image=generated[b] if generated is not None else None,
                height=height, width=width,
                latent_ids=latent_ids,
                prompt=prompt[b] if isinstance(prompt, list) else prompt,
                prompt_ids=prompt_ids[b] if prompt_ids is not None else None,
                prompt_embeds=prompt_embeds[b],
                pooled_prompt_embeds=pooled_prompt_embeds[b],
                image_latents=image_latents[b],
                condition_images=condition_images[b] if condition_images is not None else None,
            )
            for b in range(B)
        ]

    def _rollout_stepwise(self, plan, ts, sig, eta, guidance, latents, storage, step_noise, pe, pp, image_latents, compute_log_prob, extra_keys):
        return super()._rollout_stepwise(plan, ts, sig, eta, guidance, latents, storage, step_noise, pe, pp, compute_log_prob, extra_keys,
                                         image_latents=image_latents)

    # ------------------------------------------------------------------ single step / replay (flux1_kontext.py:510-589)
    def forward(
        self,
        t: torch.Tensor,
        latents: torch.Tensor,
        image_latents: torch.Tensor,
        latent_ids: torch.Tensor,
        prompt_embeds: torch.Tensor,
        pooled_prompt_embeds: torch.Tensor,
        t_next: Optional[torch.Tensor] = None,
        next_latents: Optional[torch.Tensor] = None,
        guidance_scale: float = 3.5,
        noise_level: Optional[float] = None,
        joint_attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        return_kwargs: List[str] = ["noise_pred", "next_latents", "next_latents_mean", "std_dev_t", "dt", "log_prob"],
    ) -> SDESchedulerOutput:
        # grad mode: the engine's differentiable forward + native backward, as FluxRolloutMixin.forward (the condition rides in the call record)
        return self._forward_dispatch(dict(
            t=t, latents=latents, image_latents=image_latents, latent_ids=latent_ids, prompt_embeds=prompt_embeds,
            pooled_prompt_embeds=pooled_prompt_embeds, t_next=t_next, next_latents=next_latents, guidance_scale=guidance_scale,
            noise_level=noise_level, joint_attention_kwargs=joint_attention_kwargs, compute_log_prob=compute_log_prob,
            return_kwargs=return_kwargs))

    def _forward_impl(self, t, latents, image_latents, latent_ids, prompt_embeds, pooled_prompt_embeds, t_next, next_latents, guidance_scale,
                      noise_level, joint_attention_kwargs, compute_log_prob, return_kwargs, grad: bool, host=None) -> SDESchedulerOutput:
        self._before_engine_call()
        self._check_joint_attention_kwargs(joint_attention_kwargs)
        B, Ni, _ = latents.shape
        dev = latents.device
        hp, wp, hc, wc = split_kontext_ids(latent_ids)
        if hp * wp != Ni or hc * wc != image_latents.shape[1]:
            raise ValueError(f"mi355_flow: latent_ids describe {hp * wp} target and {hc * wc} condition tokens, the latents hold {Ni} and "
                             f"{image_latents.shape[1]}")
        plan = self.engine.plan(B, 2 * hp, 2 * wp, prompt_embeds.shape[1], 1, cond=(2 * hc, 2 * wc))
        t = torch.as_tensor(t, device=dev, dtype=torch.float32).reshape(-1)
        tm = ((t.double() / 1000).float().to(latents.dtype) * 1000).float()   # as FluxRolloutMixin._forward_impl
        g = torch.as_tensor(guidance_scale, device=dev, dtype=latents.dtype).reshape(-1)
        gm = (g * 1000).float() if self.engine.cfg.guidance_embeds else None
        if t_next is not None:
            t_next = torch.as_tensor(t_next, device=dev, dtype=torch.float32).reshape(-1)
        image_latents = image_latents.to(dev)
        if grad:
            from .autograd import flux_replay
            # `train_args`: what `_FluxReplayFn` hands to `plan.forward_train`, in its backward's recompute too -- this step's condition
            call = dict(train_args=(latents, tm, gm, prompt_embeds, pooled_prompt_embeds, image_latents))
            return self._scheduler_step(t, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs,
                                        replay=(flux_replay, host, plan, call))
        v = plan.transformer_forward(latents, tm, gm, prompt_embeds, pooled_prompt_embeds, image_latents)
        return self._scheduler_step(t, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs, v=(v, None, 1.0))


# ----------------------------------------------------------------------------- operator-level wrappers (tests, microbench)


class Flux1NativeAdapter(StandaloneAdapterBase, FluxRolloutMixin):
    """Standalone FLUX.1 adapter (no Flow-Factory import): engine + scheduler (+ optional native VAE decoder)."""

    def __init__(self, state_dict: Union[Dict[str, torch.Tensor], torch.nn.Module], config: Optional[FluxConfig] = None,
                 scheduler: Optional[FlowMatchEulerDiscreteSDEScheduler] = None, latent_storage_dtype: Optional[str] = "fp16",
                 transformer_dtype: torch.dtype = torch.bfloat16, device: Union[str, torch.device] = "cuda",
                 vae_state_dict: Optional[Dict[str, torch.Tensor]] = None, vae_config=None, vae_max_batch: int = 4):
        from .vae import VAEConfig, VAEDecoder
        # FLUX.1 scheduler config: dynamic shifting (mu from the image sequence length)
        self._init_engine(FluxEngine, config or FluxConfig(),
                          scheduler or FlowMatchEulerDiscreteSDEScheduler(shift=3.0, use_dynamic_shifting=True, sde_steps=[1, 2, 3], num_sde_steps=1),
                          latent_storage_dtype, transformer_dtype, device)
        self._bind(state_dict)
        self._init_vae(VAEDecoder, vae_config or VAEConfig(scaling_factor=0.3611, shift_factor=0.1159), vae_state_dict, vae_max_batch)

    def encode_prompt(self, *a, **k):
        raise RuntimeError("mi355_flow standalone adapter has no text encoders: pass prompt_embeds / pooled_prompt_embeds")

    def decode_latents(self, latents: torch.Tensor, height: int, width: int, output_type: str = "pt"):
        """flux1.py:138-147: unpack, / scaling + shift, vae.decode, postprocess."""
        if self.vae_decoder is None:
            return None
        if output_type not in ("pt", "np"):
            raise ValueError("mi355_flow standalone adapter decodes to 'pt' or 'np'")
        lat = unpack_latents(latents, int(height) // VAE_SCALE_FACTOR, int(width) // VAE_SCALE_FACTOR).contiguous()
        return self._images_as(self.vae_decoder.decode(lat, postprocess=True, out_dtype=torch.bfloat16, max_batch=self.vae_max_batch), output_type)


class Flux1KontextNativeAdapter(FluxKontextRolloutMixin, Flux1NativeAdapter):
    """Standalone FLUX.1 Kontext adapter: `Flux1NativeAdapter`'s engine, scheduler and optional VAE decoder under the Kontext rollout.  There
    is no native VAE encoder: the condition arrives encoded (`condition_images` optional, `image_latents`, `image_ids`), as the reference's
    preprocessing stores it."""

    def encode_image(self, images=None, *a, **k):
        raise RuntimeError("mi355_flow standalone adapter has no VAE encoder: pass the encoded condition (image_latents, image_ids"
                           + (", not images=" if images is not None else "") + ")")

    def _standardize_image_input(self, images, output_type: str = "pt"):
        return [images[b] for b in range(len(images))]


def op_attention128(q: torch.Tensor, k: torch.Tensor, vT: torch.Tensor, S: int, n_first: Optional[int] = None, q_prescaled: bool = False):
    """q, k: [B, H, S_pad, 128] bf16; vT: [B, H, 128, S_pad] bf16 -> (o_first [B*n_first, H*128], o_rest [B*(S-n_first), H*128])."""
    lib = _lib.load()
    B, H, S_pad, _ = q.shape
    n_first = S if n_first is None else n_first
    D = H * 128
    o1 = torch.empty((B * n_first, D), device=q.device, dtype=torch.bfloat16)
    o2 = torch.empty((B * (S - n_first), D), device=q.device, dtype=torch.bfloat16) if n_first < S else None
    _lib.check(lib.mi355_op_attention128(_stream(), _ptr(q), _ptr(k), _ptr(vT), _ptr(o1) if n_first > 0 else None, D, n_first, _ptr(o2), D, B, H, S, S_pad,
                                         int(q_prescaled)), "op_attention128")
    return o1, o2


def _opt(t):
    return _ptr(t) if t is not None else None


def op_attention128_ex(q: torch.Tensor, k: torch.Tensor, vT: torch.Tensor, S: int, n_first: Optional[int] = None, q_prescaled: bool = False,
                       S_kv: int = 0, kv_len: Optional[torch.Tensor] = None, qmax2: Optional[torch.Tensor] = None,
                       kmax2: Optional[torch.Tensor] = None, score_bound: float = 0.0, lse: Optional[torch.Tensor] = None,
                       o_first: Optional[torch.Tensor] = None, o_rest: Optional[torch.Tensor] = None):
    """`op_attention128` with every field the engines use.  q [B, H, S_pad, 128]; k [B, H, S_kv_pad, 128], vT [B, H, 128, S_kv_pad] when S_kv > 0
    (cross-attention), else as q; kv_len int32 [B]; qmax2 / kmax2 uint32-as-int32 [B*H]; lse fp32 [B, H, S_pad] (written for rows < S).
    o_first / o_rest may be passed in (2-D, any row stride >= H*128: the stride is taken from the tensor) and are returned."""
    lib = _lib.load()
    B, H, S_pad, _ = q.shape
    n_first = S if n_first is None else n_first
    D = H * 128
    if o_first is None and n_first > 0:
        o_first = torch.empty((B * n_first, D), device=q.device, dtype=torch.bfloat16)
    if o_rest is None and n_first < S:
        o_rest = torch.empty((B * (S - n_first), D), device=q.device, dtype=torch.bfloat16)
    _lib.check(lib.mi355_op_attention128_ex(_stream(), _ptr(q), _ptr(k), _ptr(vT), _opt(o_first), o_first.stride(0) if o_first is not None else D, n_first,
                                            _opt(o_rest), o_rest.stride(0) if o_rest is not None else D, B, H, S, S_pad, int(q_prescaled), S_kv,
                                            k.shape[2] if S_kv > 0 else 0, _opt(kv_len), 0 if kv_len is None else int(kv_len.numel()), _opt(qmax2),
                                            _opt(kmax2), float(score_bound), _opt(lse)), "op_attention128_ex")
    return o_first, o_rest


def op_attention128_fwd_bwd_ex(q: torch.Tensor, k: torch.Tensor, vT: torch.Tensor, S: int, do_first: Optional[torch.Tensor],
                               do_rest: Optional[torch.Tensor], o_first: Optional[torch.Tensor], o_rest: Optional[torch.Tensor], n_first: int,
                               dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor, S_kv: int = 0, kv_len: Optional[torch.Tensor] = None,
                               score_bound: float = 0.0, lse: Optional[torch.Tensor] = None, delta: Optional[torch.Tensor] = None):
    """Training-mode forward + backward on caller-provided tensors (q pre-scaled by log2(e)/sqrt(128)).  o / dO are split at n_first like the
    forward's output; o_first and do_first share a row stride, o_rest and do_rest another.  dq [B, H, S_pad, 128], dk / dv like k."""
    lib = _lib.load()
    B, H, S_pad, _ = q.shape
    D = H * 128
    ld1 = o_first.stride(0) if o_first is not None else D
    ld2 = o_rest.stride(0) if o_rest is not None else D
    assert do_first is None or do_first.stride(0) == ld1
    assert do_rest is None or do_rest.stride(0) == ld2
    _lib.check(lib.mi355_op_attention128_fwd_bwd_ex(_stream(), _ptr(q), _ptr(k), _ptr(vT), _opt(do_first), _opt(do_rest), _opt(o_first), _opt(o_rest), ld1,
                                                    ld2, n_first, _ptr(dq), _ptr(dk), _ptr(dv), B, H, S, S_pad, S_kv, k.shape[2] if S_kv > 0 else 0,
                                                    _opt(kv_len), 0 if kv_len is None else int(kv_len.numel()), float(score_bound), _opt(lse),
                                                    _opt(delta)), "op_attention128_fwd_bwd_ex")


def op_rope_norm(src: torch.Tensor, q_col: int, k_col: int, nw_q: torch.Tensor, nw_k: torch.Tensor, cos_sin: torch.Tensor, B: int, H: int,
                 rows_per_sample: int, s_off: int, S_pad: int, eps: float = 1e-6, q_scale: float = 1.0):
    """src [M, ld] bf16 (q at q_col, k at k_col); cos_sin [S, 64, 2] fp32 -> q, k [B, H, S_pad, 128] bf16 (zero elsewhere)."""
    lib = _lib.load()
    M = src.shape[0]
    q = torch.zeros((B, H, S_pad, 128), device=src.device, dtype=torch.bfloat16)
    k = torch.zeros_like(q)
    _lib.check(lib.mi355_op_rope_norm(_stream(), _ptr(src), src.shape[1], q_col, k_col, _ptr(nw_q), _ptr(nw_k), _ptr(cos_sin), _ptr(q), _ptr(k),
                                      M, H, rows_per_sample, s_off, S_pad, eps, q_scale), "op_rope_norm")
    return q, k

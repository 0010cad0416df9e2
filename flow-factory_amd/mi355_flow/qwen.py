"""Qwen-Image rollout on the native engine (mi355_qwen_*): host mirror of `QwenImageAdapter.inference` / `.forward`
(reference src/flow_factory/models/qwen_image/qwen_image.py:288-438, :476-600) -- SURVEY.md 8(f) row N4 (config E).

Same contract as the SD3.5 / FLUX paths: reference argument names and defaults, the reference's RNG draw order, trajectory /
log-prob / callback collectors, no CPU or PyTorch fallback.  Qwen-Image specifics kept from the reference: packed latents
`(B, h/2*w/2, 64)`, `timestep = t.to(latents.dtype) / 1000`, ragged prompts (`prompt_embeds_mask`, `_pad_batch_prompt`), true CFG
with a negative prompt of its own length and the norm rescale of qwen_image.py:579-587.

What is different on MI355X: the 41 GB of bf16 weights stay resident (no FSDP2 gather per step: the reference shards the 20 B
parameters over 80 GB GPUs, one 288 GB MI355X holds model + workspace); the cond and uncond evaluations run as ONE forward batch
`[negative | positive]`; padded text keys are masked inside the attention kernel, so one launch serves prompts of any length.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import QwenCfg
from .engine import EngineBase, PlanBase, _bf16c, _ptr, _stream, dtype_code, sde_step
from .flux import pack_latents, unpack_latents
from .host import VAE_SCALE_FACTOR, RolloutMixinBase, StandaloneAdapterBase
from .samples import QwenImageSample
from .scheduler import FlowMatchEulerDiscreteSDEScheduler, SDESchedulerOutput, randn_tensor, set_scheduler_timesteps
from .trajectory import TrajectoryIndicesType

TEXT_PAD = 32     # plans are keyed by the padded text length: round up so that near-equal prompt lengths share one workspace


@dataclass
class QwenConfig:
    """diffusers QwenImageTransformer2DModel config fields the engine needs (Qwen-Image defaults)."""
    in_channels: int = 64
    num_layers: int = 60
    num_attention_heads: int = 24
    attention_head_dim: int = 128
    joint_attention_dim: int = 3584
    axes_dims_rope: Tuple[int, int, int] = (16, 56, 56)
    scale_rope: bool = True
    time_proj_dim: int = 256
    eps: float = 1e-6

    @property
    def dim(self) -> int:
        return self.num_attention_heads * self.attention_head_dim

    def to_c(self) -> QwenCfg:
        return QwenCfg(self.in_channels, self.num_layers, self.num_attention_heads, self.attention_head_dim, self.joint_attention_dim,
                       self.time_proj_dim, (C.c_int32 * 3)(*self.axes_dims_rope), int(self.scale_rope), self.eps)


def model_timestep(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The angle base of the sinusoidal projection: `timestep = t.to(latents.dtype)` (qwen_image.py:497), `timestep / 1000` in that
    dtype (:534), then `Timesteps(scale=1000)` multiplies by 1000 in fp32."""
    return (t.float().to(dtype) / 1000).float() * 1000.0


def pad_batch_prompt(prompt_embeds_mask, prompt_embeds, device):
    """`QwenImageAdapter._pad_batch_prompt` (qwen_image.py:238-284): lists of ragged tensors or padded batches -> (txt_seq_lens,
    mask (B, L), embeds (B, L, J)) truncated to the longest valid prompt L of the batch."""
    if isinstance(prompt_embeds_mask, (list, tuple)):
        lens = [int(m.sum()) for m in prompt_embeds_mask]
        mask = torch.nn.utils.rnn.pad_sequence([m.to(device) for m in prompt_embeds_mask], batch_first=True, padding_value=0)
    else:
        mask = prompt_embeds_mask.to(device)
        lens = [int(v) for v in mask.sum(dim=1).tolist()]
    L = max(lens)
    if isinstance(prompt_embeds, (list, tuple)):
        emb = torch.nn.utils.rnn.pad_sequence([e.to(device) for e in prompt_embeds], batch_first=True, padding_value=0.0)
    else:
        emb = prompt_embeds.to(device)
    return lens, mask[:, :L], emb[:, :L]


class QwenPlan(PlanBase):
    _PRE = "qwen_"

    def __init__(self, engine: QwenEngine, batch: int, n_cfg: int, latent_h: int, latent_w: int, n_text: int, max_steps: int):
        self.batch, self.n_cfg, self.h, self.w, self.n_text = batch, n_cfg, latent_h, latent_w, n_text
        self.Ni = (latent_h // 2) * (latent_w // 2)
        super().__init__(engine, (batch, n_cfg, latent_h, latent_w, n_text), max_steps)
        self.dv_shape = (batch, self.Ni, self.C)

    def _text(self, embeds: torch.Tensor, lens: Optional[Sequence[int]]):
        FB = self.batch * self.n_cfg
        assert embeds.shape == (FB, self.n_text, self.engine.cfg.joint_attention_dim), (embeds.shape, FB, self.n_text)
        lens_c = None
        if lens is not None:
            assert len(lens) == FB
            lens_c = (C.c_int32 * FB)(*[int(v) for v in lens])
        return _bf16c(embeds), lens_c

    def _forward(self, symbol: str, latents, t_model, embeds, lens, guidance_scale, return_raw: bool = False):
        B, dev = self.batch, latents.device
        assert latents.shape == (B, self.Ni, self.C), latents.shape
        tm = t_model.to(device=dev, dtype=torch.float32).reshape(-1)
        tm = (tm.expand(B) if tm.numel() == 1 else tm).contiguous()
        out = torch.empty((B, self.Ni, self.C), device=dev, dtype=torch.bfloat16)
        raw = torch.empty((B * self.n_cfg, self.Ni, self.C), device=dev, dtype=torch.bfloat16) if return_raw else None
        latents = latents.contiguous()
        pe, lens_c = self._text(embeds, lens)
        self._call(symbol, self._h, _stream(), _ptr(latents), dtype_code(latents.dtype), _ptr(tm), _ptr(pe), lens_c, float(guidance_scale),
                   _ptr(out), _ptr(raw))
        return (out, raw) if return_raw else out

    def transformer_forward(self, latents: torch.Tensor, t_model: torch.Tensor, embeds: torch.Tensor, lens: Optional[Sequence[int]] = None,
                            guidance_scale: float = 1.0, return_raw: bool = False):
        """latents (B, Ni, 64) packed; t_model (B,) = `model_timestep(t, latents.dtype)`; embeds (n_cfg*B, n_text, J), negative prompts
        first when n_cfg == 2; lens = valid text tokens per forward sample.  Returns the prediction the scheduler sees (B, Ni, 64) bf16
        (and the raw network outputs (n_cfg*B, Ni, 64) with return_raw)."""
        return self._forward("forward", latents, t_model, embeds, lens, guidance_scale, return_raw)

    # ---------------------------------------------------------------- differentiable forward (optimize() replay)
    def forward_train(self, latents: torch.Tensor, t_model: torch.Tensor, embeds: torch.Tensor, lens: Optional[Sequence[int]] = None,
                      guidance_scale: float = 1.0) -> torch.Tensor:
        """mi355_qwen_forward_train: `transformer_forward` on per-block activation buffers -- the same kernel binaries, so the prediction is
        bit-identical -- keeping what `backward` needs in the plan's training stash (ONE per plan; every call takes a serial number)."""
        out = self._forward("forward_train", latents, t_model, embeds, lens, guidance_scale)
        self._train_serial += 1
        return out

    def rollout(self, timesteps: Sequence[float], sigmas: Sequence[float], noise_levels: Sequence[float], dynamics: str,
                guidance_scale: float, init_latents: torch.Tensor, storage_dtype: torch.dtype, step_noise: Optional[torch.Tensor],
                embeds: torch.Tensor, lens: Optional[Sequence[int]] = None, keep_positions: Optional[Sequence[int]] = None,
                compute_log_prob: bool = True):
        """Returns (kept_latents [n_kept, B, Ni, 64] storage dtype, log_probs [N, B] fp32 (nan where not computed), final)."""
        shape = (self.batch, self.Ni, self.C)
        assert tuple(init_latents.shape) == shape, init_latents.shape
        pe, lens_c = self._text(embeds, lens)
        return self._rollout(shape, timesteps, sigmas, noise_levels, dynamics, guidance_scale, init_latents, storage_dtype, step_noise,
                             (_ptr(pe), lens_c), keep_positions, compute_log_prob)


class QwenEngine(EngineBase):
    """Owns the packed bf16 copy of the Qwen-Image transformer weights (mi355_qwen): 41 GB resident for the 60-layer model.
    `plan(batch, n_cfg, latent_h, latent_w, n_text, max_steps)`."""

    _ABI, _WHAT, _PLAN = "qwen", "Qwen-Image transformer", QwenPlan

    def __init__(self, cfg: QwenConfig = QwenConfig()):
        super().__init__(cfg)


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


class QwenRolloutMixin(RolloutMixinBase):
    """`inference()` / `forward()` of `QwenImageAdapter` (reference models/qwen_image/qwen_image.py:288-438, :476-600) on the engine.
    Host classes provide `engine` (QwenEngine), `scheduler`, `device`, `latent_storage_dtype`, `encode_prompt`,
    `decode_latents(latents, height, width, output_type)`.  Used by the standalone `QwenImageNativeAdapter` below and, mixed in FRONT of
    the reference's own `QwenImageAdapter`, by `mi355_flow.flow_factory_plugin.QwenImageNativeAdapter`."""

    _FAMILY = "Qwen-Image"
    _sample_cls = QwenImageSample
    _set_timesteps = staticmethod(set_scheduler_timesteps)

    def _sde_step(self, *a, **k):
        return sde_step(*a, **k)          # this module's name, looked up per call

    def _check_attention_kwargs(self, kw) -> None:
        self._check_joint_attention_kwargs(kw, "attention_kwargs")

    # ------------------------------------------------------------------ text: [negative | positive], zero-padded to the plan length
    def _forward_text(self, prompt_embeds, prompt_embeds_mask, negative_prompt_embeds, negative_prompt_embeds_mask, guidance_scale, device):
        """qwen_image.py:499-528: CFG runs when guidance_scale > 1 and a negative prompt (embeds + mask) is given.  Returns
        (n_cfg, embeds (n_cfg*B, L, J), lens, (pos_lens, pos_mask, pos_embeds), (neg...) or None)."""
        has_neg = negative_prompt_embeds is not None and negative_prompt_embeds_mask is not None
        do_cfg = float(guidance_scale) > 1.0 and has_neg
        pos = pad_batch_prompt(prompt_embeds_mask, prompt_embeds, device)
        neg = pad_batch_prompt(negative_prompt_embeds_mask, negative_prompt_embeds, device) if do_cfg else None
        L = max(pos[2].shape[1], neg[2].shape[1] if neg else 0)
        L = _round_up(L, TEXT_PAD)

        def padded(e):
            out = torch.zeros((e.shape[0], L, e.shape[2]), device=device, dtype=torch.bfloat16)
            out[:, :e.shape[1]] = e
            return out

        if do_cfg:
            if neg[2].shape[0] != pos[2].shape[0]:
                raise ValueError("mi355_flow: negative_prompt_embeds must have the batch size of prompt_embeds")
            return 2, torch.cat([padded(neg[2]), padded(pos[2])], dim=0), list(neg[0]) + list(pos[0]), pos, neg
        return 1, padded(pos[2]), list(pos[0]), pos, None

    # ------------------------------------------------------------------ rollout (qwen_image.py:288-438)
    @torch.no_grad()
    def inference(
        self,
        prompt: Union[str, List[str]] = None,
        negative_prompt: Union[str, List[str]] = None,
        num_inference_steps: int = 50,
        guidance_scale: float = 4.0,
        height: int = 1024,
        width: int = 1024,
        generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
        prompt_ids: Optional[Union[List[torch.Tensor], torch.Tensor]] = None,
        prompt_embeds: Optional[Union[List[torch.Tensor], torch.Tensor]] = None,
        prompt_embeds_mask: Optional[Union[List[torch.Tensor], torch.Tensor]] = None,
        negative_prompt_ids: Optional[Union[List[torch.Tensor], torch.Tensor]] = None,
        negative_prompt_embeds: Optional[Union[List[torch.Tensor], torch.Tensor]] = None,
        negative_prompt_embeds_mask: Optional[Union[List[torch.Tensor], torch.Tensor]] = None,
        attention_kwargs: Optional[Dict[str, Any]] = {},
        max_sequence_length: int = 1024,
        compute_log_prob: bool = False,
        extra_call_back_kwargs: List[str] = [],
        trajectory_indices: TrajectoryIndicesType = "all",
    ) -> List[QwenImageSample]:
        self._before_engine_call()
        device = self.device
        self._check_attention_kwargs(attention_kwargs)
        if (prompt is not None and (prompt_embeds is None or prompt_embeds_mask is None)) or (
                negative_prompt is not None and (negative_prompt_embeds is None or negative_prompt_embeds_mask is None)):
            enc = self.encode_prompt(prompt=prompt, negative_prompt=negative_prompt, guidance_scale=guidance_scale,
                                     max_sequence_length=max_sequence_length, device=device)
            prompt_ids, prompt_embeds, prompt_embeds_mask = enc["prompt_ids"], enc["prompt_embeds"], enc["prompt_embeds_mask"]
            negative_prompt_ids = enc.get("negative_prompt_ids")
            negative_prompt_embeds = enc.get("negative_prompt_embeds")
            negative_prompt_embeds_mask = enc.get("negative_prompt_embeds_mask")
        if prompt_embeds is None or prompt_embeds_mask is None:
            raise ValueError("mi355_flow: pass `prompt` or `prompt_embeds` + `prompt_embeds_mask`")
        B = len(prompt_embeds)
        dtype = getattr(self, "transformer_dtype", torch.bfloat16)
        Cl = self.engine.cfg.in_channels // 4
        # QwenImagePipeline.prepare_latents: height = 2 * (height // (vae_scale_factor * 2)); draws (B, 1, 16, h, w) and packs it
        h = 2 * (int(height) // (VAE_SCALE_FACTOR * 2))
        w = 2 * (int(width) // (VAE_SCALE_FACTOR * 2))
        N = int(num_inference_steps)
        Ni = (h // 2) * (w // 2)
        img_shapes = [[(1, h // 2, w // 2)]] * B

        # RNG in the reference's order: the initial latents, then one fp32 tensor of the PACKED shape per step (none under ODE)
        dyn = self.scheduler.dynamics_type
        latents = pack_latents(randn_tensor((B, 1, Cl, h, w), generator=generator, device=device, dtype=dtype).reshape(B, Cl, h, w))
        step_noise = None
        if dyn != "ODE":
            step_noise = torch.empty((N, B, Ni, Cl * 4), device=device, dtype=torch.float32)
            for i in range(N):
                step_noise[i] = randn_tensor((B, Ni, Cl * 4), generator=None, device=device, dtype=torch.float32)

        timesteps = self._set_timesteps(self.scheduler, N, seq_len=latents.shape[1], device=device)
        storage = self.latent_storage_dtype or dtype
        n_cfg, embeds, lens, _, _ = self._forward_text(prompt_embeds, prompt_embeds_mask, negative_prompt_embeds, negative_prompt_embeds_mask,
                                                       guidance_scale, device)
        plan = self.engine.plan(B, n_cfg, h, w, embeds.shape[1], N)
        traj, final = self._rollout_and_collect(plan, timesteps, N, guidance_scale, latents, storage, step_noise, (embeds, lens),
                                                compute_log_prob, extra_call_back_kwargs, trajectory_indices)
        images = self.decode_latents(final, height, width, output_type="pt")
        pick = lambda v, b: v[b] if v is not None else None
        return [
            self._sample_cls(
                timesteps=timesteps,
                **traj.per_sample(b),
                height=height, width=width,
                image=images[b] if images is not None else None,
                img_shapes=img_shapes[b],
                prompt=prompt[b] if isinstance(prompt, list) else prompt,
                prompt_ids=pick(prompt_ids, b),
                prompt_embeds=prompt_embeds[b],
                prompt_embeds_mask=prompt_embeds_mask[b],
                negative_prompt=negative_prompt[b] if isinstance(negative_prompt, list) else negative_prompt,
                negative_prompt_ids=pick(negative_prompt_ids, b),
                negative_prompt_embeds=pick(negative_prompt_embeds, b),
                negative_prompt_embeds_mask=pick(negative_prompt_embeds_mask, b),
            )
            for b in range(B)
        ]

    def _rollout_stepwise(self, plan, ts, sig, eta, guidance, latents, storage, step_noise, embeds, lens, compute_log_prob, extra_keys):
        def predict(i, cur):
            tm = model_timestep(torch.tensor(float(ts[i]), dtype=torch.float32).reshape(1), storage)
            return plan.transformer_forward(cur, tm, embeds, lens, guidance), None, 1.0

        return self._stepwise(ts, sig, eta, latents, storage, step_noise, compute_log_prob, extra_keys, predict)

    # ------------------------------------------------------------------ single step / replay (qwen_image.py:476-600)
    def forward(
        self,
        t: torch.Tensor,
        latents: torch.Tensor,
        prompt_embeds: torch.Tensor,
        prompt_embeds_mask: torch.Tensor,
        img_shapes: List[List[Tuple[int, int, int]]],
        negative_prompt_embeds: Optional[Union[List[torch.Tensor], torch.Tensor]] = None,
        negative_prompt_embeds_mask: Optional[Union[List[torch.Tensor], torch.Tensor]] = None,
        guidance_scale: float = 4.0,
        t_next: Optional[torch.Tensor] = None,
        next_latents: Optional[torch.Tensor] = None,
        noise_level: Optional[float] = None,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        return_kwargs: List[str] = ["noise_pred", "next_latents", "next_latents_mean", "std_dev_t", "dt", "log_prob"],
    ) -> SDESchedulerOutput:
        # optimize() (trainers/grpo.py:263; trainers/dgpo.py:352-364): the replay WITH autograd runs on the engine's differentiable forward +
        # native backward (mi355_flow.autograd.qwen_replay) when its backward covers the trainable set
        return self._forward_dispatch(dict(
            t=t, latents=latents, prompt_embeds=prompt_embeds, prompt_embeds_mask=prompt_embeds_mask, img_shapes=img_shapes,
            negative_prompt_embeds=negative_prompt_embeds, negative_prompt_embeds_mask=negative_prompt_embeds_mask,
            guidance_scale=guidance_scale, t_next=t_next, next_latents=next_latents, noise_level=noise_level,
            attention_kwargs=attention_kwargs, compute_log_prob=compute_log_prob, return_kwargs=return_kwargs))

    def _forward_impl(self, t, latents, prompt_embeds, prompt_embeds_mask, img_shapes, negative_prompt_embeds, negative_prompt_embeds_mask,
                      guidance_scale, t_next, next_latents, noise_level, attention_kwargs, compute_log_prob, return_kwargs,
                      grad: bool, host=None) -> SDESchedulerOutput:
        self._before_engine_call()
        self._check_attention_kwargs(attention_kwargs)
        B, Ni, _ = latents.shape
        dev = latents.device
        shape = img_shapes[0][0] if isinstance(img_shapes[0], (list, tuple)) and isinstance(img_shapes[0][0], (list, tuple)) else img_shapes[0]
        _, hp, wp = (int(v) for v in shape)
        if hp * wp != Ni:
            raise ValueError(f"mi355_flow: img_shapes {shape} does not match {Ni} packed tokens")
        n_cfg, embeds, lens, _, _ = self._forward_text(prompt_embeds, prompt_embeds_mask, negative_prompt_embeds, negative_prompt_embeds_mask,
                                                       guidance_scale, dev)
        plan = self.engine.plan(B, n_cfg, 2 * hp, 2 * wp, embeds.shape[1], 1)
        t = torch.as_tensor(t, device=dev, dtype=torch.float32).reshape(-1)
        tm = model_timestep(t, latents.dtype)
        if t_next is not None:
            t_next = torch.as_tensor(t_next, device=dev, dtype=torch.float32).reshape(-1)
        if grad:
            from .autograd import qwen_replay
            return self._scheduler_step(t, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs,
                                        replay=(qwen_replay, host, plan, dict(train_args=(latents, tm, embeds, lens, float(guidance_scale)))))
        v = plan.transformer_forward(latents, tm, embeds, lens, guidance_scale)
        return self._scheduler_step(t, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs, v=(v, None, 1.0))


class QwenImageNativeAdapter(StandaloneAdapterBase, QwenRolloutMixin):
    """Standalone Qwen-Image adapter (no Flow-Factory import): engine + scheduler.  `source` is a state dict or an `nn.Module`
    (possibly FSDP2-wrapped / LoRA-wrapped: bound through `mi355_flow.binding.LiveWeights`, re-bound when its parameters change)."""

    def __init__(self, source, config: Optional[QwenConfig] = None, scheduler: Optional[FlowMatchEulerDiscreteSDEScheduler] = None,
                 latent_storage_dtype: Optional[str] = "bf16", transformer_dtype: torch.dtype = torch.bfloat16,
                 device: Union[str, torch.device] = "cuda", vae_state_dict: Optional[Dict[str, torch.Tensor]] = None, vae_config=None,
                 vae_max_batch: int = 4):
        from .vae import WanVAEConfig, WanVAEDecoder
        # Qwen-Image scheduler config: dynamic exponential shifting (mu from the image sequence length), terminal sigma 0.02
        self._init_engine(QwenEngine, config or QwenConfig(), scheduler or FlowMatchEulerDiscreteSDEScheduler(
            shift=1.0, use_dynamic_shifting=True, base_shift=0.5, max_shift=0.9, base_image_seq_len=256, max_image_seq_len=8192,
            shift_terminal=0.02, sde_steps=[1, 2, 3], num_sde_steps=1), latent_storage_dtype, transformer_dtype, device)
        # AutoencoderKLQwenImage = the causal 3-D video VAE on one frame
        self._init_vae(WanVAEDecoder, vae_config or WanVAEConfig(), vae_state_dict, vae_max_batch)
        self._bind(source)

    def encode_prompt(self, *a, **k):
        raise RuntimeError("mi355_flow standalone adapter has no text encoder: pass prompt_embeds + prompt_embeds_mask")

    def decode_latents(self, latents: torch.Tensor, height: int, width: int, output_type: str = "pt"):
        """qwen_image.py:197-213: unpack to (B, 16, 1, h, w), latents / (1/std) + mean, vae.decode(...)[:, :, 0], postprocess."""
        if self.vae_decoder is None:
            return None
        if output_type not in ("pt", "np"):
            raise ValueError("mi355_flow standalone adapter decodes to 'pt' or 'np'")
        return self._images_as(decode_packed_latents(self.vae_decoder, latents, height, width, max_batch=self.vae_max_batch), output_type)


def decode_packed_latents(decoder, latents: torch.Tensor, height: int, width: int, postprocess: bool = True, max_batch: int = 4,
                          out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Packed (B, Ni, 64) latents -> (B, 3, H, W): `_unpack_latents` to one latent frame, the video VAE decoder on it, frame 0."""
    h = 2 * (int(height) // (VAE_SCALE_FACTOR * 2))
    w = 2 * (int(width) // (VAE_SCALE_FACTOR * 2))
    lat = unpack_latents(latents, h, w).unsqueeze(2).contiguous()
    return decoder.decode(lat, postprocess=postprocess, out_dtype=out_dtype, max_batch=max_batch)[:, 0]


def op_cfg_rescale(v_neg: torch.Tensor, v_pos: torch.Tensor, guidance_scale: float) -> torch.Tensor:
    """(rows, 64) bf16 x 2 -> the norm-rescaled true-CFG prediction (qwen_image.py:579-587)."""
    lib = _lib.load()
    a, b = _bf16c(v_neg), _bf16c(v_pos)
    out = torch.empty_like(a)
    rows = a.numel() // a.shape[-1]
    _lib.check(lib.mi355_op_cfg_rescale(_stream(), _ptr(a), _ptr(b), float(guidance_scale), _ptr(out), rows, a.shape[-1]), "op_cfg_rescale")
    return out


def op_rms_rows(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    lib = _lib.load()
    a = _bf16c(x)
    w = weight.float().contiguous()
    out = torch.empty_like(a)
    _lib.check(lib.mi355_op_rms_rows(_stream(), _ptr(a), _ptr(w), _ptr(out), a.numel() // a.shape[-1], a.shape[-1], eps), "op_rms_rows")
    return out


def op_cfg_rescale_bwd(v_neg: torch.Tensor, v_pos: torch.Tensor, guidance_scale: float, d_out: torch.Tensor):
    """Adjoint of `op_cfg_rescale` (norms differentiated through): d_out fp32 (rows, 64) -> (d_neg, d_pos) bf16."""
    lib = _lib.load()
    a, b = _bf16c(v_neg), _bf16c(v_pos)
    d = d_out.to(torch.float32).contiguous()
    dn, dp = torch.empty_like(a), torch.empty_like(a)
    rows = a.numel() // a.shape[-1]
    _lib.check(lib.mi355_op_cfg_rescale_bwd(_stream(), _ptr(a), _ptr(b), float(guidance_scale), _ptr(d), _ptr(dn), _ptr(dp), rows, a.shape[-1]),
               "op_cfg_rescale_bwd")
    return dn, dp

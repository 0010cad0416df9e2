"""Wan2.1 text-to-video rollout on the native engine (mi355_wan_*): host mirror of `Wan2_T2V_Adapter.inference` / `.forward`
(reference src/flow_factory/models/wan/wan2_t2v.py:234-421, :426-543) -- SURVEY.md 8(f) row N4, single-transformer Wan2.1.

Kept from the reference: latents `(B, 16, T, h, w)` drawn in fp32 (`prepare_latents(dtype=float32)`), `timestep = t.expand(B)` with
the scheduler's integer timesteps, classifier-free guidance as `u + g (c - u)` (here one forward over the batch [negative, positive]
instead of two passes), `UniPCMultistepSDEScheduler.step` in rollout mode = the four SDE / ODE dynamics with sigma = t / 1000.
Image-to-video with condition channels (Wan2.2-I2V-A14B; `Wan2_I2V_Adapter`, reference models/wan/wan2_i2v.py): `WanI2VRolloutMixin`,
`Wan2I2VNativeAdapter`, `wan_i2v_condition` below, on an engine created with `WanConfig.cond_channels`; Wan2.1-I2V's CLIP image
cross-attention branch with `WanConfig.image_dim` and `image_embeds=`.
Wan2.2-TI2V-5B in image-to-video use (`expand_timesteps`: frame 0 replaced by the encoded image, one timestep per token -- 0 on the tokens of
frame 0, t elsewhere; wan2_i2v.py:736-741): `WanTI2VRolloutMixin`, `Wan2TI2VNativeAdapter` on a text-to-video engine and a first-frame plan
(`WanEngine.plan(..., first_frame=True)`: two modulation rows per sample, picked by token in the kernels).  Its text-to-video use (an all-ones
mask) runs as the scalar-timestep forward.
Not covered (raise): `attention_kwargs`; the image embedder's `pos_embed` (first-and-last-frame checkpoints); any `first_frame_mask` other than
the reference's own (ones with frame 0 zero); two experts together with a first frame.  The causal 3-D video VAE decode is native too
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
from .samples import WanI2VSample, WanT2VSample
from .scheduler import FlowMatchEulerDiscreteSDEScheduler, SDESchedulerOutput, randn_tensor
from .trajectory import TrajectoryIndicesType

VAE_SCALE_SPATIAL, VAE_SCALE_TEMPORAL = 8, 4


@dataclass
class WanConfig:
    """diffusers WanTransformer3DModel config fields the engine needs (Wan2.1-T2V-1.3B defaults).  `in_channels` is the LATENT channel count
    (the scheduler's state); an image-to-video transformer takes `cond_channels` more at its patch embedding (4 mask + 16 latent = 20:
    `cat([latents, condition], 1)`, reference wan2_i2v.py:744) and, for Wan2.1-I2V, CLIP image embeddings of width `image_dim`."""
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
    cond_channels: int = 0
    image_dim: Optional[int] = None

    @property
    def dim(self) -> int:
        return self.num_attention_heads * self.attention_head_dim

    @classmethod
    def from_hf(cls, config) -> "WanConfig":
        """From a diffusers `WanTransformer3DModel.config` (object or dict).  The HF `in_channels` counts what the patch embedding sees:
        latent channels = `out_channels`, `cond_channels = in_channels - out_channels` (36 - 16 = 20 for the I2V transformers, 0 for T2V and
        for Wan2.2-TI2V-5B's 48 / 48), and the image branch exists iff `image_dim` is set (Wan2.1-I2V; Wan2.2-I2V-A14B has none)."""
        g = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
        inc = int(g("in_channels", 16))
        out = int(g("out_channels", None) or inc)
        if inc < out:
            raise ValueError(f"mi355_flow: Wan transformer with in_channels {inc} < out_channels {out}")
        image_dim = g("image_dim", None)
        return cls(in_channels=out, out_channels=out, num_layers=int(g("num_layers", 30)), num_attention_heads=int(g("num_attention_heads", 12)),
                   attention_head_dim=int(g("attention_head_dim", 128)), ffn_dim=int(g("ffn_dim", 8960)), text_dim=int(g("text_dim", 4096)),
                   freq_dim=int(g("freq_dim", 256)), patch_size=tuple(g("patch_size", (1, 2, 2))), eps=float(g("eps", 1e-6)),
                   cond_channels=inc - out, image_dim=int(image_dim) if image_dim else None)

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

    def __init__(self, engine: WanEngine, batch: int, n_cfg: int, T: int, h: int, w: int, n_text: int, max_steps: int, n_image: int = 0,
                 first_frame: bool = False):
        self.batch, self.n_cfg, self.T, self.h, self.w, self.n_text, self.n_image = batch, n_cfg, T, h, w, n_text, n_image
        self.cond_channels = engine.cfg.cond_channels          # > 0: an image-to-video plan, served by the `_i2v` entry points only
        # a first-frame plan (Wan2.2-TI2V-5B image-to-video: frame 0 replaced, its tokens at their own timestep), served by the `_ff` entry points
        self.first_frame = bool(first_frame)
        shape = (batch, n_cfg, T, h, w, n_text)
        if self.first_frame:
            if self.cond_channels or n_image:
                raise ValueError("mi355_flow: a first-frame Wan plan needs a text-to-video engine (cond_channels == 0, no image branch)")
            self._CREATE = "plan_create_ff"
        elif self.cond_channels:
            self._CREATE, shape = "plan_create_i2v", shape + (n_image,)
        elif n_image:
            raise ValueError("mi355_flow: n_image needs an image-to-video Wan engine (WanConfig.cond_channels > 0)")
        super().__init__(engine, shape, max_steps)
        # d loss / d v arrives as [uncond | text], as `engine.sde_step_bwd` returns it
        self.dv_shape = (batch * n_cfg, engine.cfg.out_channels, T, h, w)

    def _i2v_args(self, condition, image_embeds) -> Optional[tuple]:
        """(condition, its dtype code, image_embeds) as the `_i2v` entry points take them; None = a plain call.  A plain plan handed a
        condition still goes to the `_i2v` symbol, which refuses it (and the other way round): the C side owns that rule."""
        if condition is None and image_embeds is None and not self.cond_channels:
            return None
        if self.cond_channels:
            if condition is None:
                raise ValueError("mi355_flow: an image-to-video Wan plan needs `condition` (cat([mask (4), latent condition (16)], 1): wan_i2v_condition)")
            want = (self.batch, self.cond_channels, self.T, self.h, self.w)
            if tuple(condition.shape) != want:
                raise ValueError(f"mi355_flow: condition has shape {tuple(condition.shape)}, expected {want}")
            if self.n_image:
                want = (self.batch, self.n_image, self.engine.cfg.image_dim)
                if image_embeds is None or tuple(image_embeds.shape) != want:
                    raise ValueError(f"mi355_flow: this plan was created with n_image={self.n_image}: image_embeds "
                                     f"{None if image_embeds is None else tuple(image_embeds.shape)}, expected {want}")
        condition = condition.contiguous() if condition is not None else None
        image_embeds = _bf16c(image_embeds) if image_embeds is not None else None
        return condition, dtype_code(condition.dtype) if condition is not None else 0, image_embeds

    def _ff_arg(self, first_frame) -> Optional[torch.Tensor]:
        """`first_frame` (B, C, 1, h, w) as the `_ff` entry points take it; None = not a first-frame call.  A plain plan handed a first frame
        still goes to the `_ff` symbol, which refuses it (and the other way round): the C side owns that rule."""
        if first_frame is None:
            if self.first_frame:
                raise ValueError("mi355_flow: a first-frame Wan plan needs `first_frame` (B, C, 1, h, w): the encoded image's latents")
            return None
        want = (self.batch, self.C, 1, self.h, self.w)
        if tuple(first_frame.shape) != want:
            raise ValueError(f"mi355_flow: first_frame has shape {tuple(first_frame.shape)}, expected {want}")
        return first_frame.contiguous()

    def _forward(self, symbol: str, latents, t, enc_a, enc_b, condition=None, image_embeds=None, first_frame=None, t_pairs=False) -> torch.Tensor:
        B, Bp = self.batch, self.batch * self.n_cfg
        assert tuple(latents.shape) == (B, self.C, self.T, self.h, self.w), latents.shape
        dev = latents.device
        ff = self._ff_arg(first_frame)
        t = t.to(device=dev, dtype=torch.float32)
        pairs = bool(t_pairs)          # (t_head, t_rest) per sample, given explicitly
        if pairs and (ff is None or t.numel() % 2):
            raise ValueError("mi355_flow: `t_pairs` needs a first-frame plan and t of shape (., 2) = (t_head, t_rest) per sample")
        t = t.reshape(-1, 2) if pairs else t.reshape(-1, 1)
        n = t.shape[0]
        t = (t.expand(Bp, -1) if n == 1 else (t.repeat(self.n_cfg, 1) if n == B and self.n_cfg == 2 else t))
        assert t.shape[0] == Bp
        if ff is not None and not pairs:          # the reference's `first_frame_mask * t`: 0 on the tokens of frame 0, t on all others
            t = torch.cat([torch.zeros_like(t), t], dim=1)
        t = t.contiguous()
        out = torch.empty(self.dv_shape, device=dev, dtype=torch.bfloat16)
        latents = latents.contiguous()
        ea = _bf16c(enc_a)
        eb = _bf16c(enc_b) if enc_b is not None else None
        if ff is not None:
            if condition is not None or image_embeds is not None:
                raise ValueError("mi355_flow: `first_frame` does not go together with `condition` / `image_embeds`")
            self._call(symbol + "_ff", self._h, _stream(), _ptr(latents), dtype_code(latents.dtype), _ptr(t), _ptr(ea), _ptr(eb), _ptr(ff),
                       dtype_code(ff.dtype), _ptr(out))
            return out
        i2v = self._i2v_args(condition, image_embeds)
        if i2v is None:
            self._call(symbol, self._h, _stream(), _ptr(latents), dtype_code(latents.dtype), _ptr(t), _ptr(ea), _ptr(eb), _ptr(out))
        else:
            self._call(symbol + "_i2v", self._h, _stream(), _ptr(latents), dtype_code(latents.dtype), _ptr(t), _ptr(ea), _ptr(eb), _ptr(i2v[0]), i2v[1],
                       _ptr(i2v[2]), _ptr(out))
        return out

    def transformer_forward(self, latents: torch.Tensor, t: torch.Tensor, enc_a: torch.Tensor, enc_b: Optional[torch.Tensor] = None,
                            condition: Optional[torch.Tensor] = None, image_embeds: Optional[torch.Tensor] = None,
                            first_frame: Optional[torch.Tensor] = None, t_pairs: bool = False):
        """latents (B, 16, T, h, w); t (B*n_cfg,) or scalar; n_cfg == 2: enc_a = negative, enc_b = positive, output (2B, ...).
        Image-to-video plan: + condition (B, cond_channels, T, h, w), read by both CFG halves.
        First-frame plan: + first_frame (B, C, 1, h, w), which replaces frame 0 of the input; the tokens of frame 0 embed timestep 0 and the
        others `t` -- or, with `t_pairs=True`, t of shape (., 2) holds the pairs (t_head, t_rest) explicitly."""
        return self._forward("forward", latents, t, enc_a, enc_b, condition, image_embeds, first_frame, t_pairs)

    # ---------------------------------------------------------------- differentiable forward (optimize() replay)
    def forward_train(self, latents: torch.Tensor, t: torch.Tensor, enc_a: torch.Tensor, enc_b: Optional[torch.Tensor] = None,
                      condition: Optional[torch.Tensor] = None, image_embeds: Optional[torch.Tensor] = None,
                      first_frame: Optional[torch.Tensor] = None, t_pairs: bool = False) -> torch.Tensor:
        """mi355_wan_forward_train: `transformer_forward` on per-block activation buffers -- the same kernel binaries, so the prediction is
        bit-identical -- keeping what `backward` needs in the plan's training stash (ONE per plan; every call takes a serial number)."""
        out = self._forward("forward_train", latents, t, enc_a, enc_b, condition, image_embeds, first_frame, t_pairs)
        self._train_serial += 1
        return out

    def rollout(self, timesteps: Sequence[float], sigmas: Sequence[float], noise_levels: Sequence[float], dynamics: str, guidance: float,
                init_latents: torch.Tensor, storage_dtype: torch.dtype, step_noise: Optional[torch.Tensor], prompt_embeds: torch.Tensor,
                neg_embeds: Optional[torch.Tensor] = None, condition: Optional[torch.Tensor] = None, image_embeds: Optional[torch.Tensor] = None,
                keep_positions: Optional[Sequence[int]] = None, compute_log_prob: bool = True, first_frame: Optional[torch.Tensor] = None):
        shape = (self.batch, self.C, self.T, self.h, self.w)
        assert tuple(init_latents.shape) == shape, init_latents.shape
        pe = _bf16c(prompt_embeds)
        ne = _bf16c(neg_embeds) if neg_embeds is not None else None
        ff = self._ff_arg(first_frame)
        if ff is not None:
            if condition is not None or image_embeds is not None:
                raise ValueError("mi355_flow: `first_frame` does not go together with `condition` / `image_embeds`")
            return self._rollout(shape, timesteps, sigmas, noise_levels, dynamics, guidance, init_latents, storage_dtype, step_noise,
                                 (_ptr(pe), _ptr(ne)), keep_positions, compute_log_prob, symbol="rollout_ff", tail=(_ptr(ff), dtype_code(ff.dtype)))
        i2v = self._i2v_args(condition, image_embeds)
        if i2v is None:
            return self._rollout(shape, timesteps, sigmas, noise_levels, dynamics, guidance, init_latents, storage_dtype, step_noise,
                                 (_ptr(pe), _ptr(ne)), keep_positions, compute_log_prob)
        return self._rollout(shape, timesteps, sigmas, noise_levels, dynamics, guidance, init_latents, storage_dtype, step_noise,
                             (_ptr(pe), _ptr(ne)), keep_positions, compute_log_prob, symbol="rollout_i2v", tail=(_ptr(i2v[0]), i2v[1], _ptr(i2v[2])))


class WanEngine(EngineBase):
    """Owns the packed bf16 copy of one Wan transformer (mi355_wan).  `plan(batch, n_cfg, T, h, w, n_text, max_steps)`.
    `cfg.cond_channels > 0`: an image-to-video transformer (mi355_wan_create_i2v); its plans take `condition=`."""

    _ABI, _WHAT, _PLAN = "wan", "Wan transformer", WanPlan

    #: the native backward (end of round 4; its seven GPU tests are green on MI355X: profiles/r04u_*, r04v_*).  MI355_WAN_NATIVE_BACKWARD=0 keeps
    #: grad-mode forward() on the engine-valued replay (value = engine, gradient = the reference's torch path)
    native_backward_enabled = os.environ.get("MI355_WAN_NATIVE_BACKWARD", "1") != "0"

    def __init__(self, cfg: WanConfig = WanConfig()):
        super().__init__(cfg)

    def _create(self, c, h) -> None:
        cfg = self.cfg
        if cfg.image_dim and not cfg.cond_channels:
            raise ValueError("mi355_flow: image_dim needs an image-to-video Wan transformer (cond_channels > 0)")
        if not cfg.cond_channels:
            return super()._create(c, h)
        import ctypes as C
        from . import _lib
        _lib.check(self.lib.mi355_wan_create_i2v(C.byref(c), int(cfg.cond_channels), int(cfg.image_dim or 0), C.byref(h)), "wan_create_i2v")

    def plan(self, *shape_and_max_steps: int, n_image: int = 0, first_frame: bool = False):
        """`plan(batch, n_cfg, T, h, w, n_text, max_steps, n_image=0, first_frame=False)`; n_image = CLIP image tokens per sample of the image
        cross-attention branch (Wan2.1-I2V: 257), 0 = a plan without it; first_frame = the Wan2.2-TI2V image-to-video kind (frame 0 replaced
        by the encoded image, its tokens at timestep 0), a plan of its own beside the text-to-video plan of the same shape."""
        if not n_image and not first_frame:
            return super().plan(*shape_and_max_steps)
        *shape, max_steps = shape_and_max_steps
        key = tuple(shape) + (("first_frame",) if first_frame else ("n_image", int(n_image)))
        p = self._plans.get(key)
        if p is None or p.max_steps < max_steps:
            if p is not None:
                p.close()
            p = self._plans[key] = WanPlan(self, *shape, max_steps, n_image=int(n_image), first_frame=bool(first_frame))
        return p

    def bind_state_dict(self, state_dict, *a, **k) -> None:
        bad = [n for n in state_dict if "image_embedder.pos_embed" in n]
        if bad:
            raise NotImplementedError(f"mi355_flow: '{bad[0]}': the learned position embedding of the image embedder (first-and-last-frame "
                                      "Wan checkpoints) is not implemented natively")
        super().bind_state_dict(state_dict, *a, **k)

    def grad_supported(self, name: str) -> int:
        return super().grad_supported(name) if type(self).native_backward_enabled else 0


def _i2v_kw(condition, image_embeds, first_frame=None) -> Dict[str, Any]:
    """The image-to-video inputs as keywords of `transformer_forward` / `forward_train` / `rollout`; empty for text-to-video."""
    if first_frame is not None:
        return dict(first_frame=first_frame)
    return {} if condition is None and image_embeds is None else dict(condition=condition, image_embeds=image_embeds)


def _n_image_kw(image_embeds=None, plan=None, first_frame=None) -> Dict[str, int]:
    """`n_image=` / `first_frame=` for `WanEngine.plan` from the inputs of this call (or from the plan a smaller one replaces); empty without."""
    if first_frame is not None or getattr(plan, "first_frame", False):
        return dict(first_frame=True)
    n = image_embeds.shape[1] if image_embeds is not None else int(getattr(plan, "n_image", 0) or 0)
    return dict(n_image=n) if n else {}


def wan_first_frame_mask(T: int, h: int, w: int, device=None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The timestep mask of the `expand_timesteps` image-to-video pipelines as the reference's `prepare_latents` builds it
    (wan2_i2v.py:402-407): ones (1, 1, T, h, w) with frame 0 zero."""
    mask = torch.ones(1, 1, T, h, w, dtype=dtype, device=device)
    mask[:, :, 0] = 0
    return mask


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
    _first_frame_mode = False   # WanTI2VRolloutMixin: the `condition` of `_wan_inference`'s i2v hook is the first frame's latents (B, C, 1, h, w)
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
        return self._wan_inference(prompt, negative_prompt, height, width, num_frames, num_inference_steps, guidance_scale, guidance_scale_2, generator,
                                   prompt_ids, prompt_embeds, negative_prompt_ids, negative_prompt_embeds, compute_log_prob, attention_kwargs,
                                   extra_call_back_kwargs, trajectory_indices, eval_mode)

    def _wan_inference(self, prompt, negative_prompt, height, width, num_frames, num_inference_steps, guidance_scale, guidance_scale_2, generator,
                       prompt_ids, prompt_embeds, negative_prompt_ids, negative_prompt_embeds, compute_log_prob, attention_kwargs,
                       extra_call_back_kwargs, trajectory_indices, eval_mode, i2v=None):
        """Body of `inference()`.  `i2v` (image-to-video, `WanI2VRolloutMixin`): callable (B, T, h, w, height, width, num_frames, generator) ->
        (latents, condition, image_embeds, per-sample fields of the sample class), run where the reference calls `prepare_latents`."""
        device = self.device
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
        condition = image_embeds = None
        sample_fields = lambda b: {}          # noqa: E731
        first_frame = first_frame_mask = None
        if i2v is not None:          # (prepare_latents: the reference draws the latents there, before it encodes the condition)
            latents, condition, image_embeds, sample_fields = i2v(B, T, h, w, height, width, num_frames, generator)
            if self._first_frame_mode:          # Wan2.2-TI2V: the condition replaces frame 0 of the transformer input, nothing is concatenated
                first_frame, condition, first_frame_mask = condition, None, wan_first_frame_mask(T, h, w, device=device)
                if self.engine_2 is not None:
                    raise NotImplementedError("mi355_flow: a first frame (`expand_timesteps`) together with two experts is not implemented "
                                              "(Wan2.2-TI2V-5B has one transformer)")
        else:
            latents = randn_tensor((B, Cl, T, h, w), generator=generator, device=device, dtype=torch.float32)
        step_noise = None
        if self.scheduler.dynamics_type != "ODE" and not eval_mode:      # (the evaluation-mode solver is deterministic: the reference draws nothing)
            step_noise = torch.empty((N, B, Cl, T, h, w), device=device, dtype=torch.float32)
            for i in range(N):
                step_noise[i] = randn_tensor((B, Cl, T, h, w), generator=None, device=device, dtype=torch.float32)
        storage = self.latent_storage_dtype or torch.float32       # cast_latents(latents) with no default: fp32 stays fp32
        nimg = _n_image_kw(image_embeds, first_frame=first_frame)
        plan = self.engine.plan(B, 2 if do_cfg else 1, T, h, w, prompt_embeds.shape[1], N, **nimg)
        plan_2 = self.engine_2.plan(B, 2 if do_cfg else 1, T, h, w, prompt_embeds.shape[1], N, **nimg) if two else None
        sampler = None
        if eval_mode:
            if compute_log_prob or any(k != "noise_level" for k in extra_call_back_kwargs):
                raise NotImplementedError("mi355_flow: evaluation-mode Wan sampling returns latents only (the reference's UniPC step yields neither "
                                          "a log-prob nor per-step callback tensors: unipc_multistep.py:282-285)")
            sampler = self._rollout_eval_stepwise
        elif two:
            # two experts: per-step engine calls (each step picks its expert and guidance by the boundary rule; still all-HIP)
            sampler = self._rollout_stepwise
        elif any(k != "noise_level" for k in extra_call_back_kwargs):
            # per-step callback tensors.  The SAME rule as `RolloutMixinBase._rollout_and_collect` applies itself (host.py: keep the two in
            # step); it is decided here as well only because the image-to-video inputs go positionally into the fused rollout and as keywords
            # into a sampler, so which of the two runs must be known before the call
            sampler = self._rollout_stepwise
        # the image-to-video inputs travel with the prompt embeddings: positionally into the fused `plan.rollout`, as keywords into a sampler
        cond = (prompt_embeds, negative_prompt_embeds if do_cfg else None)
        ikw = _i2v_kw(condition, image_embeds, first_frame)
        rollout_kw = None
        if sampler is None and first_frame is not None:
            rollout_kw, ikw = ikw, {}          # (the first frame is a keyword of the fused `plan.rollout`)
        elif sampler is None and ikw:
            cond, ikw = cond + (condition, image_embeds), {}
        traj, final = self._rollout_and_collect(plan, timesteps, N, guidance_scale, latents, storage, step_noise, cond, compute_log_prob,
                                                extra_call_back_kwargs, trajectory_indices, sampler=sampler, rollout_kw=rollout_kw, plan_2=plan_2,
                                                guidance_2=g2, **ikw)
        if first_frame is not None:          # the reference's final merge before decode (wan2_i2v.py:605-606)
            final = (1 - first_frame_mask) * first_frame + first_frame_mask * final
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
                **sample_fields(b),
            )
            for b in range(B)
        ]

    def _rollout_eval_stepwise(self, plan, ts, sig, eta, guidance, latents, storage, step_noise, pe, ne, compute_log_prob, extra_keys,
                               plan_2=None, guidance_2=None, condition=None, image_embeds=None, first_frame=None):
        """`_rollout_eval` as a sampler of `_rollout_stepwise`'s signature: no log-probs, no per-step outputs."""
        all_lat = self._rollout_eval(plan, ts, sig, guidance, latents, storage, pe, ne, plan_2=plan_2, guidance_2=guidance_2, condition=condition,
                                     image_embeds=image_embeds, first_frame=first_frame)
        return all_lat, torch.full((len(ts), latents.shape[0]), float("nan"), device=latents.device), None

    def _rollout_eval(self, plan, ts, sig, guidance, latents, storage, pe, ne, plan_2=None, guidance_2=None, condition=None, image_embeds=None,
                      first_frame=None):
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
                pl = pl.engine.plan(B, 1, pl.T, pl.h, pl.w, pl.n_text, 1, **_n_image_kw(plan=pl))
            v = pl.transformer_forward(cur, f32(ts[i]).reshape(1), ne if cfg_i else pe, pe if cfg_i else None,
                                       **_i2v_kw(condition, image_embeds, first_frame))
            vu, vt = (v[:B], v[B:]) if cfg_i else (None, v)
            nxt = solver.step(i, vt.reshape(cur.shape), vu.reshape(cur.shape) if vu is not None else None, gd, cur)
            cur = self.cast_latents(nxt, storage)
            all_lat.append(cur)
        return all_lat

    def _rollout_stepwise(self, plan, ts, sig, eta, guidance, latents, storage, step_noise, pe, ne, compute_log_prob, extra_keys, plan_2=None,
                          guidance_2=None, condition=None, image_embeds=None, first_frame=None):
        """Per-step engine calls (still all-HIP) for rollouts that ask for per-step callback tensors, and for two-expert pipelines."""
        B = latents.shape[0]

        def predict(i, cur):
            bt = self._boundary_timestep()
            low = plan_2 is not None and bt is not None and ts[i] < bt
            pl, gd = (plan_2, guidance_2) if low else (plan, guidance)
            cfg_i = ne is not None and gd > 1.0          # the reference decides CFG per expert (wan2_t2v.py:489-498)
            if not cfg_i and pl.n_cfg == 2:
                pl = pl.engine.plan(B, 1, pl.T, pl.h, pl.w, pl.n_text, 1, **_n_image_kw(plan=pl))
            v = pl.transformer_forward(cur, torch.tensor(float(ts[i]), dtype=torch.float32).reshape(1), ne if cfg_i else pe, pe if cfg_i else None,
                                       **_i2v_kw(condition, image_embeds, first_frame))
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
                      attention_kwargs, compute_log_prob, return_kwargs, boundary_timestep, grad: bool, host=None, condition=None,
                      image_embeds=None, first_frame=None) -> SDESchedulerOutput:
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
        if first_frame is not None and self.engine_2 is not None:
            raise NotImplementedError("mi355_flow: a first frame (`expand_timesteps`) together with two experts is not implemented")
        plan = eng.plan(B, 2 if do_cfg else 1, T, h, w, prompt_embeds.shape[1], 1, **_n_image_kw(image_embeds, first_frame=first_frame))
        enc_a, enc_b = (negative_prompt_embeds, prompt_embeds) if do_cfg else (prompt_embeds, None)
        extra = (condition, image_embeds) if condition is not None or image_embeds is not None else ()
        if first_frame is not None:          # positional arguments of `forward_train`: (..., condition, image_embeds, first_frame)
            extra = (None, None, first_frame)
        sched = self.scheduler
        if noise_level is None and not (sched.is_eval or sched.dynamics_type == "ODE"):
            noise_level = sched.get_noise_level_for_timestep(float(t0))          # Wan's schedulers look the level up by timestep
        if grad:
            from .autograd import wan_replay
            return self._scheduler_step(t0, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs, replay=(
                wan_replay, host if host is not None else self, plan,
                dict(train_args=(latents, t0.reshape(1), enc_a, enc_b) + extra, cfg_guidance=float(guidance_scale) if do_cfg else None)))
        v = plan.transformer_forward(latents, t0.reshape(1), enc_a, enc_b, **_i2v_kw(condition, image_embeds, first_frame))
        return self._scheduler_step(t0, latents, t_next, next_latents, noise_level, compute_log_prob, return_kwargs,
                                    v=(v[B:], v[:B], guidance_scale) if do_cfg else (v, None, guidance_scale))


def wan_i2v_condition(latent_condition: torch.Tensor, num_frames: int, vae_scale_temporal: int = VAE_SCALE_TEMPORAL,
                      last_frame: bool = False) -> torch.Tensor:
    """The transformer-side condition of the I2V pipelines from the normalised VAE latents of the conditioning clip (first frame [+ last
    frame], zeros between): `cat([mask (vae_scale_temporal), latent_condition], 1)` -- the mask arithmetic of the reference's
    `prepare_latents` (wan2_i2v.py:409-422).  The pixel-frame mask (1 on the given frames) has its first frame repeated `vae_scale_temporal`
    times, so that `num_frames + vae_scale_temporal - 1` frames fold into T latent frames of `vae_scale_temporal` mask channels."""
    B, _, T, h, w = latent_condition.shape
    mask = torch.ones(B, 1, num_frames, h, w)
    if last_frame:
        mask[:, :, 1:-1] = 0
    else:
        mask[:, :, 1:] = 0
    first = torch.repeat_interleave(mask[:, :, 0:1], dim=2, repeats=vae_scale_temporal)
    mask = torch.concat([first, mask[:, :, 1:]], dim=2)
    if mask.shape[2] != T * vae_scale_temporal:
        raise ValueError(f"mi355_flow: {num_frames} frames do not fold into {T} latent frames at temporal scale {vae_scale_temporal}")
    mask = mask.view(B, -1, vae_scale_temporal, h, w).transpose(1, 2).to(latent_condition.device)
    return torch.concat([mask, latent_condition], dim=1)


class WanI2VRolloutMixin(WanRolloutMixin):
    """`inference()` / `forward()` of `Wan2_I2V_Adapter` (reference models/wan/wan2_i2v.py:425-652, :656-783) on an image-to-video engine
    (`WanConfig.cond_channels > 0`): the T2V loop whose transformer input is `cat([latents, condition], 1)`.  `condition` (and, once the image
    branch exists natively, `image_embeds`) travel with the prompt embeddings through the fused rollout, the step-wise and evaluation-mode
    loops, the replay and its native backward; the two-expert rule and the per-expert CFG are inherited (Wan2.2-I2V-A14B).
    `image_embeds` (B, Ni, image_dim) drive the image cross-attention branch of a Wan2.1-I2V engine (`WanConfig.image_dim`).
    Refused here: `expand_timesteps` pipelines (Wan2.2-TI2V-5B in I2V use: one timestep per token, wan2_i2v.py:736-741) and `first_frame_mask`
    -- they have no condition channels and run on `WanTI2VRolloutMixin` / `Wan2TI2VNativeAdapter`."""

    _sample_cls = WanI2VSample
    expand_timesteps = False

    def _refuse_expand_timesteps(self, first_frame_mask=None) -> None:
        if self.expand_timesteps or first_frame_mask is not None:
            raise NotImplementedError("mi355_flow: `expand_timesteps` image-to-video pipelines (Wan2.2-TI2V-5B) pass one timestep per token "
                                      "(first_frame_mask * t) and replace frame 0 instead of concatenating condition channels: use "
                                      "Wan2TI2VNativeAdapter / WanTI2VRolloutMixin (a text-to-video engine with a first-frame plan)")

    def _prepare_i2v(self, images, last_image, image_embeds, B, T, h, w, height, width, num_frames, generator):
        """-> (fp32 latents, condition, image_embeds, condition_images) from raw images: needs a VAE encoder (and CLIP for Wan2.1-I2V).
        Hook of the host class; standalone there is neither."""
        raise NotImplementedError("mi355_flow: the native Wan I2V adapter has no VAE encoder / CLIP image encoder: pass `condition=` "
                                  "(wan_i2v_condition of the normalised first-frame latents) instead of `images`")

    @torch.no_grad()
    def inference(
        self,
        images: Any = None,
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
        image_embeds: Optional[torch.Tensor] = None,
        condition_images: Optional[Any] = None,
        last_image: Optional[torch.Tensor] = None,
        compute_log_prob: bool = False,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        max_sequence_length: int = 512,
        extra_call_back_kwargs: List[str] = [],
        trajectory_indices: TrajectoryIndicesType = "all",
        condition: Optional[torch.Tensor] = None,
    ) -> List[WanI2VSample]:
        """The reference's signature plus `condition=` (B, 20, T, h, w): given, nothing is encoded (the standalone adapter's only way)."""
        self._refuse_expand_timesteps()
        eval_mode = bool(getattr(self.scheduler, "is_eval", False))
        device = self.device

        def i2v(B, T, h, w, height_, width_, frames, gen):
            if condition is None:
                return self._prepare_i2v(images, last_image, image_embeds, B, T, h, w, height_, width_, frames, gen)
            # RNG in the reference's order: prepare_latents draws the fp32 latents first (then one fp32 draw per SDE step)
            lat = randn_tensor((B, self.engine.cfg.in_channels, T, h, w), generator=gen, device=device, dtype=torch.float32)
            cond = condition.to(device)
            emb = image_embeds.to(device=device, dtype=self.transformer_dtype) if image_embeds is not None else None
            want = (B, self.engine.cfg.cond_channels, T, h, w)
            if tuple(cond.shape) != want:
                raise ValueError(f"mi355_flow: condition has shape {tuple(cond.shape)}, expected {want}")
            imgs = condition_images if condition_images is not None else images
            return lat, cond, emb, lambda b: dict(condition=cond[b], image_embeds=emb[b] if emb is not None else None, first_frame_mask=None,
                                                  condition_images=imgs[b] if imgs is not None else None)

        return self._wan_inference(prompt, negative_prompt, height, width, num_frames, num_inference_steps, guidance_scale, guidance_scale_2, generator,
                                   prompt_ids, prompt_embeds, negative_prompt_ids, negative_prompt_embeds, compute_log_prob, attention_kwargs,
                                   extra_call_back_kwargs, trajectory_indices, eval_mode, i2v=i2v)

    def forward(
        self,
        t: torch.Tensor,
        latents: torch.Tensor,
        prompt_embeds: torch.Tensor,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        guidance_scale: float = 5.0,
        guidance_scale_2: Optional[float] = None,
        image_embeds: Optional[torch.Tensor] = None,
        condition: Optional[torch.Tensor] = None,
        first_frame_mask: Optional[torch.Tensor] = None,
        boundary_timestep: Optional[float] = None,
        t_next: Optional[torch.Tensor] = None,
        next_latents: Optional[torch.Tensor] = None,
        noise_level: Optional[float] = None,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        return_kwargs: List[str] = ["noise_pred", "next_latents", "next_latents_mean", "std_dev_t", "dt", "log_prob"],
    ) -> SDESchedulerOutput:
        self._refuse_expand_timesteps(first_frame_mask)
        if condition is None:
            raise ValueError("mi355_flow: Wan I2V forward() needs `condition`")
        kw = dict(t=t, latents=latents, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, guidance_scale=guidance_scale,
                  guidance_scale_2=guidance_scale_2, t_next=t_next, next_latents=next_latents, noise_level=noise_level,
                  attention_kwargs=attention_kwargs, compute_log_prob=compute_log_prob, return_kwargs=return_kwargs, boundary_timestep=boundary_timestep,
                  condition=condition.to(latents.device), image_embeds=image_embeds)
        if not WanEngine.native_backward_enabled:
            return self._forward_nograd(**kw)
        return self._forward_dispatch(kw, replay_host=lambda: self._replay_host(self._expert(
            float(torch.as_tensor(t, dtype=torch.float32).reshape(-1)[0]), guidance_scale, guidance_scale_2, boundary_timestep)[0]))


class WanTI2VRolloutMixin(WanI2VRolloutMixin):
    """`inference()` / `forward()` of `Wan2_I2V_Adapter` for pipelines with `config.expand_timesteps` (Wan2.2-TI2V-5B in image-to-video use;
    reference models/wan/wan2_i2v.py:547-652, :736-741) on a TEXT-TO-VIDEO engine (no condition channels: TI2V-5B's transformer takes 48
    channels in and out) with a first-frame plan.  `condition` is the normalised VAE latents of the first frame, (B, C, 1, h, w): the
    transformer reads `(1 - first_frame_mask) * condition + first_frame_mask * latents` and one timestep per token, `first_frame_mask * t` --
    0 on the tokens of frame 0, t elsewhere.  The engine merges frame 0 where it patchifies and keeps two modulation rows per sample; the
    scheduler step and the log-prob run over all latents, frame 0 included, as the reference's do; the sample's `first_frame_mask` is the
    reference's (ones (1, 1, T, h, w), frame 0 zero) and the final latents are merged before decode.  Only that mask is native: any other
    `first_frame_mask` raises ValueError.  One transformer only (`engine_2` raises NotImplementedError)."""

    _first_frame_mode = True
    expand_timesteps = True

    def _refuse_expand_timesteps(self, first_frame_mask=None) -> None:
        """(the parent's refusal does not apply: this class IS the `expand_timesteps` path)"""

    def _prepare_i2v(self, images, last_image, image_embeds, B, T, h, w, height, width, num_frames, generator):
        """-> (fp32 latents, first-frame latents (B, C, 1, h, w), first_frame_mask, condition_images) from raw images: needs a VAE encoder.
        Hook of the host class (the plugin calls the reference's `prepare_latents`); standalone there is none."""
        raise NotImplementedError("mi355_flow: the native Wan TI2V adapter has no VAE encoder: pass `condition=` (the normalised first-frame "
                                  "latents, (B, C, 1, h, w)) instead of `images`")

    def _forward_impl(self, *args, condition=None, first_frame_mask=None, image_embeds=None, **kw) -> SDESchedulerOutput:
        """`forward()`'s call record keeps the reference's own names (`condition`, `first_frame_mask`: a grad fallback hands them to the
        reference's forward unchanged); the (checked) mask selects the engine's first-frame path and `condition` is that first frame."""
        return super()._forward_impl(*args, first_frame=condition, **kw)

    def _check_first_frame_mask(self, first_frame_mask, T: int, h: int, w: int) -> None:
        if first_frame_mask is None:
            raise ValueError("mi355_flow: Wan TI2V forward() needs `first_frame_mask` (the sample's: ones (1, 1, T, h, w) with frame 0 zero)")
        want = (1, 1, T, h, w)
        if tuple(first_frame_mask.shape) != want:
            raise ValueError(f"mi355_flow: first_frame_mask has shape {tuple(first_frame_mask.shape)}, expected {want} (the reference's own mask)")
        ref = wan_first_frame_mask(T, h, w, device=first_frame_mask.device, dtype=first_frame_mask.dtype)
        if not torch.equal(first_frame_mask, ref):
            raise ValueError("mi355_flow: only the reference's own first_frame_mask is native (ones with frame 0 zero: the first frame is the "
                             "condition, its tokens embed timestep 0); this mask has other values or another frame zero")

    @torch.no_grad()
    def inference(
        self,
        images: Any = None,
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
        image_embeds: Optional[torch.Tensor] = None,
        condition_images: Optional[Any] = None,
        last_image: Optional[torch.Tensor] = None,
        compute_log_prob: bool = False,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        max_sequence_length: int = 512,
        extra_call_back_kwargs: List[str] = [],
        trajectory_indices: TrajectoryIndicesType = "all",
        condition: Optional[torch.Tensor] = None,
    ) -> List[WanI2VSample]:
        """The reference's signature plus `condition=` (B, C, 1, h, w): the first frame's normalised latents (standalone: the only way)."""
        eval_mode = bool(getattr(self.scheduler, "is_eval", False))
        device = self.device
        if image_embeds is not None:
            raise ValueError("mi355_flow: Wan2.2-TI2V has no image cross-attention branch: `image_embeds` must be None")

        def i2v(B, T, h, w, height_, width_, frames, gen):
            if condition is None:
                lat, cond, mask, imgs = self._prepare_i2v(images, last_image, image_embeds, B, T, h, w, height_, width_, frames, gen)
                self._check_first_frame_mask(mask, T, h, w)
            else:
                # RNG in the reference's order: prepare_latents draws the fp32 latents first (then one fp32 draw per SDE step)
                lat = randn_tensor((B, self.engine.cfg.in_channels, T, h, w), generator=gen, device=device, dtype=torch.float32)
                cond = condition.to(device)
                mask = wan_first_frame_mask(T, h, w, device=device)
                imgs = condition_images if condition_images is not None else images
            want = (B, self.engine.cfg.in_channels, 1, h, w)
            if tuple(cond.shape) != want:
                raise ValueError(f"mi355_flow: condition (the first frame's latents) has shape {tuple(cond.shape)}, expected {want}")
            return lat, cond, None, lambda b: dict(condition=cond[b], image_embeds=None, first_frame_mask=mask,
                                                   condition_images=imgs[b] if imgs is not None else None)

        return self._wan_inference(prompt, negative_prompt, height, width, num_frames, num_inference_steps, guidance_scale, guidance_scale_2, generator,
                                   prompt_ids, prompt_embeds, negative_prompt_ids, negative_prompt_embeds, compute_log_prob, attention_kwargs,
                                   extra_call_back_kwargs, trajectory_indices, eval_mode, i2v=i2v)

    def forward(
        self,
        t: torch.Tensor,
        latents: torch.Tensor,
        prompt_embeds: torch.Tensor,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        guidance_scale: float = 5.0,
        guidance_scale_2: Optional[float] = None,
        image_embeds: Optional[torch.Tensor] = None,
        condition: Optional[torch.Tensor] = None,
        first_frame_mask: Optional[torch.Tensor] = None,
        boundary_timestep: Optional[float] = None,
        t_next: Optional[torch.Tensor] = None,
        next_latents: Optional[torch.Tensor] = None,
        noise_level: Optional[float] = None,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        compute_log_prob: bool = True,
        return_kwargs: List[str] = ["noise_pred", "next_latents", "next_latents_mean", "std_dev_t", "dt", "log_prob"],
    ) -> SDESchedulerOutput:
        if condition is None:
            raise ValueError("mi355_flow: Wan TI2V forward() needs `condition` (the first frame's latents, (B, C, 1, h, w))")
        if image_embeds is not None:
            raise ValueError("mi355_flow: Wan2.2-TI2V has no image cross-attention branch: `image_embeds` must be None")
        B, C, T, h, w = latents.shape
        self._check_first_frame_mask(first_frame_mask, T, h, w)
        if tuple(condition.shape) != (B, C, 1, h, w):
            raise ValueError(f"mi355_flow: condition (the first frame's latents) has shape {tuple(condition.shape)}, expected {(B, C, 1, h, w)}")
        kw = dict(t=t, latents=latents, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, guidance_scale=guidance_scale,
                  guidance_scale_2=guidance_scale_2, t_next=t_next, next_latents=next_latents, noise_level=noise_level,
                  attention_kwargs=attention_kwargs, compute_log_prob=compute_log_prob, return_kwargs=return_kwargs, boundary_timestep=boundary_timestep,
                  condition=condition.to(latents.device), first_frame_mask=first_frame_mask, image_embeds=None)
        if not WanEngine.native_backward_enabled:
            return self._forward_nograd(**kw)
        return self._forward_dispatch(kw, replay_host=lambda: self._replay_host(self._expert(
            float(torch.as_tensor(t, dtype=torch.float32).reshape(-1)[0]), guidance_scale, guidance_scale_2, boundary_timestep)[0]))


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


class Wan2I2VNativeAdapter(WanI2VRolloutMixin, Wan2T2VNativeAdapter):
    """Standalone Wan image-to-video adapter (no Flow-Factory import): `Wan2T2VNativeAdapter` on image-to-video engine(s) -- Wan2.2-I2V-A14B
    with `state_dict_2` / `boundary_ratio`.  `config` carries `cond_channels` (`WanConfig.from_hf` of the transformer's config).  There is no
    VAE encoder and no CLIP here: `inference(condition=..., prompt_embeds=...)` takes the condition ready-made (`wan_i2v_condition`)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: Optional[WanConfig] = None, *args, expand_timesteps: bool = False, **kw):
        config = config or WanConfig(cond_channels=20)
        if not config.cond_channels:
            raise ValueError("mi355_flow: Wan2I2VNativeAdapter needs an image-to-video config (WanConfig.cond_channels > 0)")
        self.expand_timesteps = bool(expand_timesteps)
        self._refuse_expand_timesteps()
        super().__init__(state_dict, config, *args, **kw)


class Wan2TI2VNativeAdapter(WanTI2VRolloutMixin, Wan2T2VNativeAdapter):
    """Standalone Wan2.2-TI2V-5B image-to-video adapter (no Flow-Factory import): `Wan2T2VNativeAdapter`'s engine (a text-to-video transformer:
    `WanConfig.from_hf` gives cond_channels == 0 for TI2V's 48 / 48 channels) driven through first-frame plans.  There is no VAE encoder here:
    `inference(condition=first_frame_latents (B, C, 1, h, w), prompt_embeds=...)`.  The TI2V residual VAE is not native: `video_decode=` callable
    or latents only.  One transformer: `state_dict_2` is refused."""

    vae_scale_spatial = 16          # the TI2V-5B VAE compresses 4 x 16 x 16 (`inference()` sizes the latents by it; an instance may override)

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: Optional[WanConfig] = None, *args, **kw):
        config = config or WanConfig(in_channels=48, out_channels=48, num_attention_heads=24, ffn_dim=14336)
        if config.cond_channels or config.image_dim:
            raise ValueError("mi355_flow: Wan2TI2VNativeAdapter needs a text-to-video config (cond_channels == 0, no image_dim): the first frame "
                             "replaces frame 0, nothing is concatenated (condition channels: Wan2I2VNativeAdapter)")
        if kw.get("state_dict_2") is not None:
            raise NotImplementedError("mi355_flow: a first frame (`expand_timesteps`) together with two experts is not implemented "
                                      "(Wan2.2-TI2V-5B has one transformer)")
        super().__init__(state_dict, config, *args, **kw)

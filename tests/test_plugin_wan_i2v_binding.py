"""CPU test of the Flow-Factory binding of Wan image-to-video (`mi355_flow.flow_factory_plugin.Wan2I2VNativeAdapter`) against the REFERENCE's
own `Wan2_I2V_Adapter`, on the pattern of tests/test_plugin_kontext_binding.py: the plugin class is constructed as Flow-Factory does --
`cls(config, accelerator)` with the reference's own I2V example YAML -- on a pseudo-pipeline whose VAE encode is a stand-in; the engine is a
computing double whose output depends on the condition it receives.  Checked: which class each method comes from; for `inference()` the RNG
order (latents first, then one draw per SDE step), the condition at the engine per sample, the reference's `WanI2VSample` and
`BaseSample.stack`; the no-grad `forward()` replay; `image_embeds` of a Wan2.1-I2V pipeline at the engine; the refusal of `expand_timesteps`;
a trainable image-branch parameter in grad mode (raise, and the documented opt-in).  Skips without the reference tree."""
import types

import pytest
import torch

from oracle import ref_package

pytestmark = pytest.mark.skipif(not ref_package.available(), reason="needs the reference tree (build container only)")

import _plugin_fakes as F  # noqa: E402

YAML = "/root/reference/examples/grpo/full/wan22/i2v.yaml"
NAMES = ["blocks.0.attn1.to_q.weight", "blocks.0.attn1.to_q.bias", "patch_embedding.weight", "blocks.0.attn2.add_k_proj.weight"]
TD = 32


def _shift(condition, image_embeds=None):
    s = 0.25 * condition.float().mean(dim=(1, 2, 3, 4), keepdim=True)
    return s if image_embeds is None else s + 0.5 * image_embeds.float().mean(dim=(1, 2)).view(-1, 1, 1, 1, 1)


class I2VPlan(F.WanStandinPlanStepwise):
    """The Wan stand-in network plus a term in the sample's own condition: a condition that did not arrive, or arrived at the wrong sample,
    changes the result."""

    def __init__(self, engine, key, n_image=0):
        super().__init__(engine, key)
        self.n_image = n_image

    def transformer_forward(self, latents, t, enc_a, enc_b=None, condition=None, image_embeds=None):
        v = super().transformer_forward(latents, t, enc_a, enc_b)
        self.engine.calls[-1][1].update(condition=condition, image_embeds=image_embeds)
        return (v.float() + _shift(condition, image_embeds).repeat(v.shape[0] // latents.shape[0], 1, 1, 1, 1)).to(torch.bfloat16)

    def rollout(self, timesteps, sigmas, noise_levels, dynamics, guidance, init_latents, storage_dtype, step_noise, prompt_embeds, neg_embeds=None,
                condition=None, image_embeds=None, keep_positions=None, compute_log_prob=True):
        from oracle import standin
        from oracle import wan_ref as W
        self.engine.calls.append(("rollout", dict(N=len(timesteps), n_cfg=self.n_cfg, condition=condition, image_embeds=image_embeds, init=init_latents,
                                                  noise=step_noise, keep=keep_positions)))
        den = lambda x, t, e: (standin.wan_denoiser(x, t, e, 0).float() + _shift(condition, image_embeds)).to(torch.bfloat16)      # noqa: E731
        out = W.rollout(None, None, prompt_embeds, neg_embeds, guidance, init_latents, step_noise, torch.tensor(timesteps).long(),
                        torch.tensor(sigmas, dtype=torch.float32), list(noise_levels), storage_dtype, dynamics_type=dynamics,
                        compute_log_prob=compute_log_prob, denoiser=den)
        return F._keep_rows(out, len(timesteps), keep_positions)


class I2VEngine(F._StandinFamilyEngine):
    NAMES = NAMES
    PLAN = I2VPlan

    native_backward_enabled = True

    def plan(self, *key, n_image=0):
        k = key + (n_image,)
        if k not in self._plans:
            self._plans[k] = I2VPlan(self, key, n_image)
        return self._plans[k]

    def grad_supported(self, name) -> int:          # the native backward's scope, as mi355_wan_grad_supported reports it
        return 1 if ".attn1.to_q." in name else 0


def _pipeline(transformer, expand_timesteps=False):
    """tests/test_plugin_binding._wan_pipeline plus what the I2V adapter touches: a VAE `encode` stand-in (a fixed function of the clip),
    `video_processor.preprocess`, no image encoder (Wan2.2-I2V-A14B has none)."""
    import torch.nn as nn
    from oracle import diffusers_stub as D
    vae = nn.Module()
    vae.add_module("decoder", nn.Linear(2, 2))
    vae.config = types.SimpleNamespace(z_dim=16, base_dim=96, dim_mult=(1, 2, 4, 4), num_res_blocks=2, temperal_downsample=(False, True, True),
                                       latents_mean=[0.05 * i for i in range(16)], latents_std=[1.0 + 0.1 * i for i in range(16)])
    vae.dtype = torch.float32

    def encode(video):          # (B, 3, F, H, W) -> latents (B, 16, (F - 1) / 4 + 1, H / 8, W / 8)
        B, _, Fr, H, W = video.shape
        first = torch.nn.functional.avg_pool2d(video[:, :, 0].float(), 8)                                   # (B, 3, h, w)
        lat = torch.zeros(B, 16, (Fr - 1) // 4 + 1, H // 8, W // 8)
        lat[:, :, 0] = first.mean(1, keepdim=True) * torch.linspace(0.5, 2.0, 16).view(1, 16, 1, 1)
        return types.SimpleNamespace(latents=lat)

    vae.encode = encode
    pipe = types.SimpleNamespace()
    pipe.transformer, pipe.vae, pipe.transformer_2 = transformer, vae, None
    pipe.text_encoder, pipe.tokenizer, pipe.image_encoder, pipe.image_processor = nn.Linear(2, 2), object(), None, None
    pipe.vae_scale_factor_temporal, pipe.vae_scale_factor_spatial = 4, 8
    pipe.config = types.SimpleNamespace(boundary_ratio=None, expand_timesteps=expand_timesteps)
    pipe.scheduler = D.UniPCMultistepScheduler(num_train_timesteps=1000, use_flow_sigmas=True, flow_shift=3.0)
    pipe.video_processor = types.SimpleNamespace(postprocess_video=lambda v, output_type="pt": v,
                                                 preprocess=lambda im, height=None, width=None: torch.stack(list(im)) * 2.0 - 1.0)
    pipe.maybe_free_model_hooks = lambda: None
    pipe.components = {"transformer": transformer, "vae": vae, "text_encoder": pipe.text_encoder}
    return pipe


def _tcfg(**kw):
    return types.SimpleNamespace(**{**dict(in_channels=36, out_channels=16, num_layers=1, num_attention_heads=1, attention_head_dim=128, ffn_dim=64,
                                           text_dim=TD, freq_dim=256, patch_size=(1, 2, 2), eps=1e-6, image_dim=None), **kw})


@pytest.fixture(scope="module")
def ref():
    ref_package.install()
    import mi355_flow.flow_factory_plugin as P
    if P._RefAdapter is None:      # imported earlier in this process without the reference on sys.path
        import importlib
        P = importlib.reload(P)
    assert P._RefAdapter is not None, P._IMPORT_ERROR
    return P


def _make(ref, monkeypatch, tcfg=None, expand_timesteps=False):
    import mi355_flow.vae as MV
    import mi355_flow.wan as MW
    from flow_factory.hparams import Arguments
    P = ref
    tr = F.build_module_tree({n: ((8, 8) if n.endswith("weight") else (8,)) for n in NAMES}, buffers=(), cls=F.FakeTransformer).bfloat16()
    tr.config = tcfg or _tcfg()
    monkeypatch.setattr(P, "WanEngine", I2VEngine)
    monkeypatch.setattr(MV, "WanVAEDecoder", F.FakeVideoVAEDecoder)
    monkeypatch.setattr(MW, "sde_step", F.oracle_sde_step)

    class Plug(P.Wan2I2VNativeAdapter):
        def load_pipeline(self):
            return _pipeline(tr, expand_timesteps)

        def _standardize_image_input(self, images, output_type="pil"):       # (PIL round trip of the reference: tensors stay tensors here)
            return images

    cfg = Arguments.load_from_yaml(YAML)
    cfg.model_args.finetune_type = "full"
    ad = Plug(cfg, F.FakeAccelerator())
    ad.post_init()
    F.FakeTransformer.calls = 0
    return ad, tr


def test_methods_come_from_the_mixin_and_the_reference(ref):
    from flow_factory.models.wan.wan2_i2v import Wan2_I2V_Adapter, WanI2VSample
    from mi355_flow.wan import WanI2VRolloutMixin, WanRolloutMixin
    K = ref.Wan2I2VNativeAdapter
    mro = K.__mro__
    assert mro.index(WanI2VRolloutMixin) < mro.index(WanRolloutMixin) < mro.index(Wan2_I2V_Adapter)
    assert K.inference is WanI2VRolloutMixin.inference and K._forward_impl is WanRolloutMixin._forward_impl
    assert K.encode_image is Wan2_I2V_Adapter.encode_image and K.prepare_latents is Wan2_I2V_Adapter.prepare_latents
    assert K.preprocess_func is Wan2_I2V_Adapter.preprocess_func
    assert K.decode_latents is ref.Wan2T2VNativeAdapter.decode_latents
    assert K._sample_cls is WanI2VSample


def test_rollout_and_replay_through_the_plugin(ref, monkeypatch):
    from flow_factory.models.wan.wan2_i2v import WanI2VSample as RefSample
    from flow_factory.samples import BaseSample
    from mi355_flow.wan import wan_i2v_condition
    ad, tr = _make(ref, monkeypatch)
    assert type(ad.scheduler).__module__.startswith("flow_factory.") and ad.engine.cfg.cond_channels == 20 and ad.engine.cfg.in_channels == 16
    ad.rollout()
    B, Nt, N, H, W, frames = 2, 7, 4, 32, 48, 5
    T, h, w = 2, 4, 6
    g = torch.Generator().manual_seed(3)
    pe, ne = torch.randn(B, Nt, TD, generator=g).bfloat16(), torch.randn(B, Nt, TD, generator=g).bfloat16()
    images = torch.rand(B, 3, H, W, generator=g)
    torch.manual_seed(11)
    samples = ad.inference(images=images, prompt=["a", "b"], height=H, width=W, num_frames=frames, num_inference_steps=N, guidance_scale=3.5,
                           prompt_embeds=pe, negative_prompt_embeds=ne, compute_log_prob=True, trajectory_indices="all")
    kind, call = ad.engine.calls[-1]
    assert kind == "rollout" and call["N"] == N and call["n_cfg"] == 2 and call["keep"] == list(range(N + 1)) and call["image_embeds"] is None
    # RNG order of the reference: prepare_latents draws the fp32 latents first, then one fp32 draw per step
    torch.manual_seed(11)
    init = torch.randn(B, 16, T, h, w)
    noise = torch.stack([torch.randn(B, 16, T, h, w) for _ in range(N)])
    assert torch.equal(call["init"], init) and torch.equal(call["noise"], noise)
    # the condition at the engine: the reference's own prepare_latents on the stand-in VAE = mask + normalised first-frame latents, per sample
    vc = ad.pipeline.vae.config
    enc = ad.pipeline.vae.encode(torch.cat([(images * 2 - 1).unsqueeze(2), torch.zeros(B, 3, frames - 1, H, W)], 2)).latents
    want = wan_i2v_condition((enc - torch.tensor(vc.latents_mean).view(1, 16, 1, 1, 1)) * (1.0 / torch.tensor(vc.latents_std).view(1, 16, 1, 1, 1)), frames)
    assert call["condition"].shape == (B, 20, T, h, w) and torch.equal(call["condition"], want)
    assert not torch.equal(want[0], want[1])
    assert len(samples) == B and all(type(s) is RefSample for s in samples)
    s0 = samples[0]
    assert s0.all_latents.shape == (N + 1, 16, T, h, w) and s0.first_frame_mask is None and s0.image_embeds is None
    assert torch.equal(samples[1].condition, want[1]) and torch.equal(s0.condition, want[0])
    stacked = BaseSample.stack(samples)
    assert stacked["condition"].shape == (B, 20, T, h, w) and stacked["all_latents"].shape[:2] == (B, N + 1)
    assert len(ad.engine.bind_log) == len(NAMES)

    # the no-grad replay of a stored transition: this call's condition at the engine, each sample its own
    i = int(ad.scheduler.current_sde_steps[0])
    ts = s0.timesteps
    kw = dict(t=ts[i].expand(B), t_next=ts[i + 1].expand(B), latents=stacked["all_latents"][:, i], next_latents=stacked["all_latents"][:, i + 1],
              condition=stacked["condition"], prompt_embeds=pe, negative_prompt_embeds=ne, guidance_scale=3.5, noise_level=None, compute_log_prob=True,
              return_kwargs=["log_prob", "noise_pred"])          # (noise_level None: the scheduler's own level at this timestep, as in the rollout)
    with torch.no_grad():
        out = ad.forward(**kw)
        swapped = ad.forward(**{**kw, "condition": stacked["condition"].flip(0)})
    kind, call = ad.engine.calls[-2]
    assert kind == "transformer_forward" and torch.equal(call["condition"], want) and call["n_cfg"] == 2
    assert out.noise_pred.shape == (B, 16, T, h, w) and torch.isfinite(out.log_prob).all()
    assert not torch.equal(swapped.noise_pred, out.noise_pred)
    assert s0.log_probs.shape == (1,)                                 # one SDE step in this schedule: its log-prob is the stored one
    torch.testing.assert_close(out.log_prob, torch.stack([s.log_probs[0] for s in samples]), rtol=1e-5, atol=1e-5)      # (fp32 operation order)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="expand_timesteps"):
        ad.forward(**{**kw, "first_frame_mask": torch.ones(1, 1, T, h, w)})
    assert F.FakeTransformer.calls == 0


def test_expand_timesteps_pipelines_are_refused(ref, monkeypatch):
    with pytest.raises(NotImplementedError, match="expand_timesteps"):
        _make(ref, monkeypatch, expand_timesteps=True)


def test_image_embeds_reach_the_engine_per_sample(ref, monkeypatch):
    """A Wan2.1-I2V pipeline (`image_dim` set): the engine is created with the branch, `image_embeds` travel with the condition into a plan with
    `n_image` image tokens, in the rollout and in the replay, and into the reference's samples."""
    from flow_factory.samples import BaseSample
    ad, tr = _make(ref, monkeypatch, tcfg=_tcfg(image_dim=16))
    assert ad.engine.cfg.image_dim == 16 and ad.engine.cfg.cond_channels == 20
    ad.rollout()
    B, Nt, N, H, W, frames, Ni = 2, 7, 4, 32, 48, 5, 5
    g = torch.Generator().manual_seed(3)
    pe, ne = torch.randn(B, Nt, TD, generator=g).bfloat16(), torch.randn(B, Nt, TD, generator=g).bfloat16()
    images, ie = torch.rand(B, 3, H, W, generator=g), torch.randn(B, Ni, 16, generator=g).bfloat16()
    torch.manual_seed(11)
    samples = ad.inference(images=images, image_embeds=ie, prompt=["a", "b"], height=H, width=W, num_frames=frames, num_inference_steps=N,
                           guidance_scale=3.5, prompt_embeds=pe, negative_prompt_embeds=ne, compute_log_prob=True, trajectory_indices="all")
    kind, call = ad.engine.calls[-1]
    assert kind == "rollout" and torch.equal(call["image_embeds"], ie) and all(k[-1] == Ni for k in ad.engine._plans)
    assert torch.equal(samples[1].image_embeds, ie[1])
    stacked = BaseSample.stack(samples)
    i = int(ad.scheduler.current_sde_steps[0])
    ts = samples[0].timesteps
    kw = dict(t=ts[i].expand(B), t_next=ts[i + 1].expand(B), latents=stacked["all_latents"][:, i], next_latents=stacked["all_latents"][:, i + 1],
              condition=stacked["condition"], image_embeds=stacked["image_embeds"], prompt_embeds=pe, negative_prompt_embeds=ne, guidance_scale=3.5,
              noise_level=None, compute_log_prob=True, return_kwargs=["log_prob", "noise_pred"])
    with torch.no_grad():
        out = ad.forward(**kw)
        swapped = ad.forward(**{**kw, "image_embeds": stacked["image_embeds"].flip(0)})
    kind, call = ad.engine.calls[-2]
    assert kind == "transformer_forward" and torch.equal(call["image_embeds"], ie)
    torch.testing.assert_close(out.log_prob, torch.stack([s.log_probs[0] for s in samples]), rtol=1e-5, atol=1e-5)      # (fp32 operation order)
    assert not torch.equal(swapped.noise_pred, out.noise_pred)


def test_trainable_image_branch_parameter_raises_with_the_documented_opt_in(ref, monkeypatch):
    """`attn2.add_k_proj.weight` trainable: outside the native backward's scope.  Grad-mode forward() raises by default and names the opt-in;
    with MI355_ALLOW_REFERENCE_AUTOGRAD=1 the reference's own `Wan2_I2V_Adapter.forward` runs with autograd -- the concatenated 36-channel
    input and the image embeddings reach the torch transformer -- and the values are the engine's."""
    ad, tr = _make(ref, monkeypatch, tcfg=_tcfg(image_dim=16))
    ad.rollout()
    ad.scheduler.set_timesteps(10, device="cpu")
    B, Nt, T, h, w, Ni = 2, 7, 2, 4, 6, 5
    g = torch.Generator().manual_seed(5)
    pe, ie = torch.randn(B, Nt, TD, generator=g).bfloat16(), torch.randn(B, Ni, 16, generator=g).bfloat16()
    lat, cond = torch.randn(B, 16, T, h, w, generator=g).half(), torch.randn(B, 20, T, h, w, generator=g)
    kw = dict(t=torch.tensor([900.0, 900.0]), t_next=torch.tensor([750.0, 750.0]), latents=lat, next_latents=(lat * 0.9).half(), condition=cond,
              image_embeds=ie, prompt_embeds=pe, guidance_scale=1.0, noise_level=0.7, compute_log_prob=True, return_kwargs=["log_prob", "noise_pred"])
    with torch.no_grad():
        native = ad.forward(**kw)
    wk = tr.get_submodule("blocks.0.attn2.add_k_proj").weight
    for prm in tr.parameters():
        prm.requires_grad_(False)
    wk.requires_grad_(True)
    seen = {}

    def torch_transformer(hidden_states=None, encoder_hidden_states_image=None, **kw_):
        seen.update(channels=hidden_states.shape[1], image=encoder_hidden_states_image)
        return (hidden_states[:, :16].float() * wk.float().mean(),)

    import contextlib
    tr.forward = torch_transformer
    tr.cache_context = lambda name: contextlib.nullcontext()          # (diffusers' per-branch cache scope: nothing to scope here)
    try:
        monkeypatch.delenv("MI355_ALLOW_REFERENCE_AUTOGRAD", raising=False)
        with torch.enable_grad(), pytest.raises(NotImplementedError, match="MI355_ALLOW_REFERENCE_AUTOGRAD"):
            ad.forward(**kw)
        monkeypatch.setenv("MI355_ALLOW_REFERENCE_AUTOGRAD", "1")
        with torch.enable_grad():
            out = ad.forward(**kw)
    finally:
        del tr.forward, tr.cache_context
    assert seen["channels"] == 36 and torch.equal(seen["image"], ie)
    assert out.log_prob.requires_grad and torch.equal(out.log_prob.detach(), native.log_prob)
    (gk,) = torch.autograd.grad(out.log_prob.sum(), wk)
    assert torch.isfinite(gk).all() and float(gk.abs().sum()) > 0

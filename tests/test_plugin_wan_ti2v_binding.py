"""CPU test of the Flow-Factory binding of Wan2.2-TI2V-5B image-to-video (`mi355_flow.flow_factory_plugin.Wan2TI2VNativeAdapter`) against the
REFERENCE's own `Wan2_I2V_Adapter`, on the pattern of tests/test_plugin_wan_i2v_binding.py: the plugin class is constructed as Flow-Factory does
-- `cls(config, accelerator)` with the reference's own I2V example YAML (which names the 5 B checkpoint as the alternative) -- on an
`expand_timesteps` pseudo-pipeline whose VAE is a stand-in; the engine is a computing double that runs the reference's step on what it is
handed: the network on `(1 - mask) * first_frame + mask * latents`, plus a term in the sample's own first frame.  Pinned: which class each
method comes from; the RNG order (latents first, then one draw per SDE step); the first frame at the engine per sample and the mask of the
samples; the reference's `WanI2VSample` / `BaseSample.stack`; the final merge before the reference's own decode; the no-grad `forward()`
replay; the refusal of a pipeline without `expand_timesteps`; a trainable parameter outside the native backward in grad mode (raise, and the
documented opt-in: the reference's own forward receives `condition` and `first_frame_mask`).  Skips without the reference tree."""
import types

import pytest
import torch

from oracle import ref_package

pytestmark = pytest.mark.skipif(not ref_package.available(), reason="needs the reference tree (build container only)")

import _plugin_fakes as F  # noqa: E402

YAML = "/root/reference/examples/grpo/full/wan22/i2v.yaml"
NAMES = ["blocks.0.attn1.to_q.weight", "blocks.0.attn1.to_q.bias", "patch_embedding.weight"]
TD, C = 32, 48


def _shift(first_frame):
    return 0.25 * first_frame.float().mean(dim=(1, 2, 3, 4), keepdim=True)


def _merge(x, first_frame):
    mask = torch.ones(1, 1, *x.shape[2:])
    mask[:, :, 0] = 0
    return ((1 - mask) * first_frame.float() + mask * x.float()).to(x.dtype)


class TI2VPlan(F.WanStandinPlanStepwise):
    """The Wan stand-in network on the merged input plus a term in the sample's own first frame: a first frame that did not arrive, or arrived
    at the wrong sample, changes the result."""

    def __init__(self, engine, key, first_frame=False):
        super().__init__(engine, key)
        self.first_frame = first_frame

    def transformer_forward(self, latents, t, enc_a, enc_b=None, first_frame=None):
        assert self.first_frame and first_frame is not None
        v = super().transformer_forward(_merge(latents, first_frame), t, enc_a, enc_b)
        self.engine.calls[-1][1].update(first_frame=first_frame)
        return (v.float() + _shift(first_frame).repeat(v.shape[0] // latents.shape[0], 1, 1, 1, 1)).to(torch.bfloat16)

    def rollout(self, timesteps, sigmas, noise_levels, dynamics, guidance, init_latents, storage_dtype, step_noise, prompt_embeds, neg_embeds=None,
                condition=None, image_embeds=None, keep_positions=None, compute_log_prob=True, first_frame=None):
        from oracle import standin
        from oracle import wan_ref as W
        assert self.first_frame and first_frame is not None and condition is None and image_embeds is None
        self.engine.calls.append(("rollout", dict(N=len(timesteps), n_cfg=self.n_cfg, first_frame=first_frame, init=init_latents, noise=step_noise,
                                                  keep=keep_positions)))
        den = lambda x, t, e: (standin.wan_denoiser(_merge(x, first_frame), t, e, 0).float() + _shift(first_frame)).to(torch.bfloat16)      # noqa: E731
        out = W.rollout(None, None, prompt_embeds, neg_embeds, guidance, init_latents, step_noise, torch.tensor(timesteps).long(),
                        torch.tensor(sigmas, dtype=torch.float32), list(noise_levels), storage_dtype, dynamics_type=dynamics,
                        compute_log_prob=compute_log_prob, denoiser=den)
        return F._keep_rows(out, len(timesteps), keep_positions)


class TI2VEngine(F._StandinFamilyEngine):
    NAMES = NAMES
    PLAN = TI2VPlan

    native_backward_enabled = True

    def plan(self, *key, n_image=0, first_frame=False):
        assert not n_image
        k = key + (first_frame,)
        if k not in self._plans:
            self._plans[k] = TI2VPlan(self, key, first_frame)
        return self._plans[k]

    def grad_supported(self, name) -> int:
        return 1 if ".attn1.to_q." in name else 0


def _pipeline(transformer, expand_timesteps=True):
    """tests/test_plugin_wan_i2v_binding._pipeline at the TI2V geometry: 48 latent channels, a 4 x 16 x 16 VAE whose `encode` / `decode` are
    stand-ins (`decode` keeps what it receives)."""
    import torch.nn as nn
    from oracle import diffusers_stub as D
    vae = nn.Module()
    vae.add_module("decoder", nn.Linear(2, 2))
    vae.config = types.SimpleNamespace(z_dim=C, latents_mean=[0.05 * i for i in range(C)], latents_std=[1.0 + 0.1 * i for i in range(C)])
    vae.dtype = torch.float32
    vae.decoded = []

    def encode(video):          # (B, 3, 1, H, W): the first frame alone (wan2_i2v.py:371-372) -> latents (B, 48, 1, H / 16, W / 16)
        B, _, Fr, H, W = video.shape
        assert Fr == 1
        first = torch.nn.functional.avg_pool2d(video[:, :, 0].float(), 16)
        return types.SimpleNamespace(latents=(first.mean(1, keepdim=True) * torch.linspace(0.5, 2.0, C).view(1, C, 1, 1)).unsqueeze(2))

    def decode(latents, return_dict=False):
        vae.decoded.append(latents.clone())
        return (latents[:, :3],)

    vae.encode, vae.decode = encode, decode
    pipe = types.SimpleNamespace()
    pipe.transformer, pipe.vae, pipe.transformer_2 = transformer, vae, None
    pipe.text_encoder, pipe.tokenizer, pipe.image_encoder, pipe.image_processor = nn.Linear(2, 2), object(), None, None
    pipe.vae_scale_factor_temporal, pipe.vae_scale_factor_spatial = 4, 16
    pipe.config = types.SimpleNamespace(boundary_ratio=None, expand_timesteps=expand_timesteps)
    pipe.scheduler = D.UniPCMultistepScheduler(num_train_timesteps=1000, use_flow_sigmas=True, flow_shift=3.0)
    pipe.video_processor = types.SimpleNamespace(postprocess_video=lambda v, output_type="pt": v,
                                                 preprocess=lambda im, height=None, width=None: torch.stack(list(im)) * 2.0 - 1.0)
    pipe.maybe_free_model_hooks = lambda: None
    pipe.components = {"transformer": transformer, "vae": vae, "text_encoder": pipe.text_encoder}
    return pipe


def _tcfg(**kw):
    return types.SimpleNamespace(**{**dict(in_channels=C, out_channels=C, num_layers=1, num_attention_heads=1, attention_head_dim=128, ffn_dim=64,
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


def _make(ref, monkeypatch, tcfg=None, expand_timesteps=True):
    import mi355_flow.wan as MW
    from flow_factory.hparams import Arguments
    P = ref
    tr = F.build_module_tree({n: ((8, 8) if n.endswith("weight") else (8,)) for n in NAMES}, buffers=(), cls=F.FakeTransformer).bfloat16()
    tr.config = tcfg or _tcfg()
    monkeypatch.setattr(P, "WanEngine", TI2VEngine)
    monkeypatch.setattr(MW, "sde_step", F.oracle_sde_step)

    class Plug(P.Wan2TI2VNativeAdapter):
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
    from mi355_flow.wan import WanI2VRolloutMixin, WanRolloutMixin, WanTI2VRolloutMixin
    K = ref.Wan2TI2VNativeAdapter
    mro = K.__mro__
    assert mro.index(WanTI2VRolloutMixin) < mro.index(WanI2VRolloutMixin) < mro.index(WanRolloutMixin) < mro.index(Wan2_I2V_Adapter)
    assert K.inference is WanTI2VRolloutMixin.inference and K._forward_impl is WanTI2VRolloutMixin._forward_impl
    assert K.prepare_latents is Wan2_I2V_Adapter.prepare_latents and K.preprocess_func is Wan2_I2V_Adapter.preprocess_func
    assert K._sample_cls is WanI2VSample
    assert ref.Wan2I2VNativeAdapter.inference is WanI2VRolloutMixin.inference          # the condition-channel class is what it was


def test_rollout_and_replay_through_the_plugin(ref, monkeypatch):
    from flow_factory.models.wan.wan2_i2v import WanI2VSample as RefSample
    from flow_factory.samples import BaseSample
    ad, tr = _make(ref, monkeypatch)
    assert type(ad.scheduler).__module__.startswith("flow_factory.") and ad.engine.cfg.cond_channels == 0 and ad.engine.cfg.in_channels == C
    assert ad.vae_scale_spatial == 16
    ad.rollout()
    B, Nt, N, H, W, frames = 2, 7, 4, 64, 96, 5
    T, h, w = 2, 4, 6
    g = torch.Generator().manual_seed(3)
    pe, ne = torch.randn(B, Nt, TD, generator=g).bfloat16(), torch.randn(B, Nt, TD, generator=g).bfloat16()
    images = torch.rand(B, 3, H, W, generator=g)
    torch.manual_seed(11)
    samples = ad.inference(images=images, prompt=["a", "b"], height=H, width=W, num_frames=frames, num_inference_steps=N, guidance_scale=3.5,
                           prompt_embeds=pe, negative_prompt_embeds=ne, compute_log_prob=True, trajectory_indices="all")
    kind, call = ad.engine.calls[-1]
    assert kind == "rollout" and call["N"] == N and call["n_cfg"] == 2 and all(k[-1] is True for k in ad.engine._plans)
    assert call["keep"] == list(range(N + 1))          # the fused rollout is told which positions to keep, as for the other Wan kinds
    # RNG order of the reference: prepare_latents draws the fp32 latents first, then one fp32 draw per step
    torch.manual_seed(11)
    init = torch.randn(B, C, T, h, w)
    noise = torch.stack([torch.randn(B, C, T, h, w) for _ in range(N)])
    assert torch.equal(call["init"], init) and torch.equal(call["noise"], noise)
    # the first frame at the engine: the reference's own prepare_latents on the stand-in VAE = the normalised latents of the first frame alone
    vc = ad.pipeline.vae.config
    enc = ad.pipeline.vae.encode((images * 2 - 1).unsqueeze(2)).latents
    want = (enc - torch.tensor(vc.latents_mean).view(1, C, 1, 1, 1)) * (1.0 / torch.tensor(vc.latents_std).view(1, C, 1, 1, 1))
    assert call["first_frame"].shape == (B, C, 1, h, w) and torch.equal(call["first_frame"], want) and not torch.equal(want[0], want[1])
    mask = torch.ones(1, 1, T, h, w)
    mask[:, :, 0] = 0
    assert len(samples) == B and all(type(s) is RefSample for s in samples)
    s0 = samples[0]
    assert s0.all_latents.shape == (N + 1, C, T, h, w) and s0.image_embeds is None
    assert torch.equal(s0.first_frame_mask, mask) and s0.first_frame_mask is samples[1].first_frame_mask
    assert torch.equal(samples[1].condition, want[1]) and torch.equal(s0.condition, want[0])
    stacked = BaseSample.stack(samples)
    assert stacked["condition"].shape == (B, C, 1, h, w) and stacked["all_latents"].shape[:2] == (B, N + 1)
    assert tuple(stacked["first_frame_mask"].shape) == (1, 1, T, h, w)          # shared by the batch, not stacked
    # the final merge before the reference's own decode: frame 0 = the condition, the other frames = the final latents (de-normalised there)
    (seen,) = ad.pipeline.vae.decoded
    final = stacked["all_latents"][:, N].float()
    merged = (1 - mask) * want + mask * final
    back = (seen - torch.tensor(vc.latents_mean).view(1, C, 1, 1, 1)) * (1.0 / torch.tensor(vc.latents_std).view(1, C, 1, 1, 1))
    torch.testing.assert_close(back, merged, rtol=1e-5, atol=1e-5)
    assert not torch.allclose(final[:, :, 0], want[:, :, 0], atol=1e-2)         # the scheduler stepped frame 0 like the others

    # the no-grad replay of a stored transition: the first frame at the engine, each sample its own; the stored log-prob comes back
    i = int(ad.scheduler.current_sde_steps[0])
    ts = s0.timesteps
    kw = dict(t=ts[i].expand(B), t_next=ts[i + 1].expand(B), latents=stacked["all_latents"][:, i], next_latents=stacked["all_latents"][:, i + 1],
              condition=stacked["condition"], first_frame_mask=stacked["first_frame_mask"], prompt_embeds=pe, negative_prompt_embeds=ne,
              guidance_scale=3.5, noise_level=None, compute_log_prob=True, return_kwargs=["log_prob", "noise_pred"])
    with torch.no_grad():
        out = ad.forward(**kw)
        swapped = ad.forward(**{**kw, "condition": stacked["condition"].flip(0)})
    kind, call = ad.engine.calls[-2]
    assert kind == "transformer_forward" and torch.equal(call["first_frame"], want) and call["n_cfg"] == 2
    assert out.noise_pred.shape == (B, C, T, h, w) and torch.isfinite(out.log_prob).all()
    assert not torch.equal(swapped.noise_pred, out.noise_pred)
    assert s0.log_probs.shape == (1,)
    torch.testing.assert_close(out.log_prob, torch.stack([s.log_probs[0] for s in samples]), rtol=1e-5, atol=1e-5)      # (fp32 operation order)
    # only the reference's own mask
    bad = mask.clone()
    bad[:, :, 1] = 0
    with torch.no_grad(), pytest.raises(ValueError, match="first_frame_mask"):
        ad.forward(**{**kw, "first_frame_mask": bad})
    with torch.no_grad(), pytest.raises(ValueError, match="first_frame_mask"):
        ad.forward(**{**kw, "first_frame_mask": None})
    assert F.FakeTransformer.calls == 0


def test_a_pipeline_without_expand_timesteps_is_refused(ref, monkeypatch):
    with pytest.raises(NotImplementedError, match="Wan2I2VNativeAdapter"):
        _make(ref, monkeypatch, expand_timesteps=False)


def test_trainable_parameter_outside_the_scope_raises_with_the_documented_opt_in(ref, monkeypatch):
    """`patch_embedding.weight` trainable: outside the native backward's scope.  Grad-mode forward() raises by default and names the opt-in;
    with MI355_ALLOW_REFERENCE_AUTOGRAD=1 the reference's own `Wan2_I2V_Adapter.forward` runs with autograd on ITS `expand_timesteps` branch --
    the torch transformer sees the merged 48-channel input and the (B, S) timestep, 0 on the tokens of frame 0 -- and the values are the engine's."""
    ad, tr = _make(ref, monkeypatch)
    ad.rollout()
    ad.scheduler.set_timesteps(10, device="cpu")
    B, Nt, T, h, w = 2, 7, 2, 4, 6
    g = torch.Generator().manual_seed(5)
    pe = torch.randn(B, Nt, TD, generator=g).bfloat16()
    lat, cond = torch.randn(B, C, T, h, w, generator=g).half(), torch.randn(B, C, 1, h, w, generator=g)
    mask = torch.ones(1, 1, T, h, w)
    mask[:, :, 0] = 0
    kw = dict(t=torch.tensor([900.0, 900.0]), t_next=torch.tensor([750.0, 750.0]), latents=lat, next_latents=(lat * 0.9).half(), condition=cond,
              first_frame_mask=mask, prompt_embeds=pe, guidance_scale=1.0, noise_level=0.7, compute_log_prob=True, return_kwargs=["log_prob", "noise_pred"])
    with torch.no_grad():
        native = ad.forward(**kw)
    wp = tr.get_submodule("patch_embedding").weight
    for prm in tr.parameters():
        prm.requires_grad_(False)
    wp.requires_grad_(True)
    seen = {}

    def torch_transformer(hidden_states=None, timestep=None, **kw_):
        seen.update(hidden=hidden_states.detach().clone(), timestep=timestep.detach().clone())
        return (hidden_states.float() * wp.float().mean(),)

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
    assert seen["hidden"].shape == (B, C, T, h, w)
    assert torch.equal(seen["hidden"][:, :, 0].float(), cond[:, :, 0].to(seen["hidden"].dtype).float())          # frame 0 = the condition
    assert torch.equal(seen["hidden"][:, :, 1:].float(), lat[:, :, 1:].to(seen["hidden"].dtype).float())
    hw = (h // 2) * (w // 2)
    want_ts = torch.tensor([0.0] * hw + [900.0] * ((T - 1) * hw))
    assert seen["timestep"].shape == (B, T * hw) and all(torch.equal(seen["timestep"][b].float(), want_ts) for b in range(B))
    assert out.log_prob.requires_grad and torch.equal(out.log_prob.detach(), native.log_prob)
    assert torch.equal(out.noise_pred.detach(), native.noise_pred)
    (gp,) = torch.autograd.grad(out.log_prob.sum(), wp)
    assert torch.isfinite(gp).all() and float(gp.abs().sum()) > 0

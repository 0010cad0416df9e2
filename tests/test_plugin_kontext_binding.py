"""CPU test of the Flow-Factory binding of FLUX.1 Kontext (`mi355_flow.flow_factory_plugin.Flux1KontextNativeAdapter`) against the
REFERENCE's own `Flux1KontextAdapter`, as tests/test_plugin_binding.py does for the other families: the plugin class is constructed as
Flow-Factory does -- `cls(config, accelerator)` with the reference's own example YAML -- on a pseudo-pipeline, the engine is a computing
double at the Python boundary.  Checked: which class each method comes from, the rollout through `inference()` (condition plan, the
condition latents at the engine, the reference's sample class and `BaseSample.stack`), the no-grad replay, and the grad-mode fallback
through the reference's `forward` with the engine's values.  Skips where the reference tree is absent.
"""
import types

import pytest
import torch

from oracle import ref_package

pytestmark = pytest.mark.skipif(not ref_package.available(), reason="needs the reference tree (build container only)")

import _plugin_fakes as F  # noqa: E402

YAML = "/root/reference/examples/grpo/full/flux1_kontext/default.yaml"
NAMES = ["transformer_blocks.0.attn.to_q.weight", "transformer_blocks.0.attn.to_q.bias", "x_embedder.weight"]


class KontextPlan(F.FluxStandinPlanModel):
    """`FluxStandinPlanModel` behind `FluxEngine.plan(..., cond=)`: the stand-in network plus a term in the sample's condition latents, so that
    a condition that did not arrive -- or arrived at the wrong sample -- changes the result."""

    def __init__(self, engine, key):
        super().__init__(engine, key[:5])
        self.cond = key[5]

    @staticmethod
    def _shift(image_latents):
        return 0.25 * image_latents.float().mean(dim=(1, 2), keepdim=True)

    def transformer_forward(self, latents, t_model, guidance_model, prompt_embeds, pooled, image_latents=None):
        v = super().transformer_forward(latents, t_model, guidance_model, prompt_embeds, pooled)
        self.engine.calls[-1][1]["image_latents"] = image_latents
        return (v.float() + self._shift(image_latents)).to(torch.bfloat16)

    def rollout(self, timesteps, sigmas, noise_levels, dynamics, guidance_scale, init_latents, storage_dtype, step_noise, prompt_embeds, pooled,
                image_latents=None, keep_positions=None, compute_log_prob=True):
        out = super().rollout(timesteps, sigmas, noise_levels, dynamics, guidance_scale, init_latents, storage_dtype, step_noise, prompt_embeds,
                              pooled, keep_positions=keep_positions, compute_log_prob=compute_log_prob)
        self.engine.calls[-1][1].update(image_latents=image_latents, keep=keep_positions)
        return out


class KontextEngine(F._StandinFamilyEngine):
    NAMES = NAMES
    PLAN = KontextPlan

    def plan(self, batch, latent_h, latent_w, n_text, max_steps, cond=None):
        return super().plan(batch, latent_h, latent_w, n_text, max_steps, cond)


@pytest.fixture(scope="module")
def ref():
    ref_package.install()
    import mi355_flow.flow_factory_plugin as P
    if P._RefAdapter is None:      # imported earlier in this process without the reference on sys.path
        import importlib
        P = importlib.reload(P)
    assert P._RefAdapter is not None, P._IMPORT_ERROR
    return P


@pytest.fixture()
def adapter(ref, monkeypatch):
    import mi355_flow.flux as MF
    from flow_factory.hparams import Arguments
    from oracle import make_rollout_golden as G
    P = ref
    tr = F.build_module_tree({n: ((8, 8) if n.endswith("weight") else (8,)) for n in NAMES}, buffers=(), cls=F.FakeTransformer).bfloat16()
    monkeypatch.setattr(P, "FluxEngine", KontextEngine)
    monkeypatch.setattr(P, "VAEDecoder", F.FakeVAEDecoder)
    monkeypatch.setattr(P, "VAEConfig", types.SimpleNamespace(from_hf=lambda c: c))
    monkeypatch.setattr(MF, "sde_step", F.oracle_sde_step)

    class Plug(P.Flux1KontextNativeAdapter):
        def load_pipeline(self):
            return G._flux_pipeline(tr)

    cfg = Arguments.load_from_yaml(YAML)
    cfg.model_args.finetune_type = "full"
    ad = Plug(cfg, F.FakeAccelerator())
    ad.post_init()
    F.FakeTransformer.calls = 0
    return ad, tr


def _condition(B, hc, wc, seed=0):
    from mi355_flow.flux import prepare_latent_image_ids
    g = torch.Generator().manual_seed(seed)
    image_ids = prepare_latent_image_ids(hc, wc, "cpu", torch.bfloat16)
    image_ids[:, 0] = 1
    return torch.randn(B, hc * wc, 64, generator=g).bfloat16(), image_ids


def test_methods_come_from_the_mixin_the_reference_and_the_flux_plugin(ref):
    from flow_factory.models.flux.flux1_kontext import Flux1KontextAdapter, Flux1KontextSample
    from mi355_flow.flux import FluxKontextRolloutMixin
    K = ref.Flux1KontextNativeAdapter
    mro = K.__mro__
    assert mro.index(FluxKontextRolloutMixin) < mro.index(Flux1KontextAdapter)
    assert K.inference is FluxKontextRolloutMixin.inference and K.forward is FluxKontextRolloutMixin.forward
    assert K.encode_image is Flux1KontextAdapter.encode_image and K._standardize_image_input is Flux1KontextAdapter._standardize_image_input
    assert K.decode_latents is ref.Flux1NativeAdapter.decode_latents
    assert K._sample_cls is Flux1KontextSample


def test_rollout_and_replay_through_the_plugin(adapter):
    from flow_factory.models.flux.flux1_kontext import Flux1KontextSample as RefSample
    from flow_factory.samples import BaseSample
    ad, tr = adapter
    assert type(ad.scheduler).__module__.startswith("flow_factory.")
    ad.rollout()
    B, Nt, N, hc, wc = 2, 7, 4, 2, 3
    g = torch.Generator().manual_seed(3)
    pe, pp = torch.randn(B, Nt, 128, generator=g).bfloat16(), torch.randn(B, 128, generator=g).bfloat16()
    il, image_ids = _condition(B, hc, wc)
    torch.manual_seed(11)
    samples = ad.inference(prompt=["a", "b"], height=64, width=64, num_inference_steps=N, guidance_scale=3.5, prompt_embeds=pe,
                           pooled_prompt_embeds=pp, image_latents=il, image_ids=image_ids.unsqueeze(0).repeat(B, 1, 1),
                           compute_log_prob=True, trajectory_indices="all")
    kind, call = ad.engine.calls[-1]
    assert kind == "rollout" and call["N"] == N and torch.equal(call["image_latents"], il) and call["keep"] == list(range(N + 1))
    (key,) = ad.engine._plans                                                     # one condition plan: the grid comes from the ids
    assert key == (B, 8, 8, Nt, N, (2 * hc, 2 * wc))
    assert len(ad.engine.bind_log) == len(NAMES)
    assert len(samples) == B and all(type(s) is RefSample for s in samples)
    s0 = samples[0]
    assert s0.all_latents.shape == (N + 1, 16, 64) and s0.latent_ids.shape == (16 + hc * wc, 3) and torch.equal(s0.latent_ids[16:], image_ids)
    assert torch.equal(samples[1].image_latents, il[1]) and s0.condition_images is None and s0.image.shape == (3, 64, 64)
    stacked = BaseSample.stack(samples)
    assert stacked["image_latents"].shape == (B, hc * wc, 64) and stacked["latent_ids"].shape == (16 + hc * wc, 3)      # shared, not stacked
    assert stacked["all_latents"].shape[:2] == (B, N + 1)

    # the no-grad replay of a stored transition: the condition plan again, this call's condition at the engine
    i = int(ad.scheduler.current_sde_steps[0])
    ts = s0.timesteps
    kw = dict(t=ts[i].expand(B), t_next=ts[i + 1].expand(B), latents=stacked["all_latents"][:, i], next_latents=stacked["all_latents"][:, i + 1],
              image_latents=stacked["image_latents"], latent_ids=stacked["latent_ids"], prompt_embeds=pe, pooled_prompt_embeds=pp,
              guidance_scale=3.5, noise_level=0.7, compute_log_prob=True, return_kwargs=["log_prob", "noise_pred"])
    with torch.no_grad():
        out = ad.forward(**kw)
        swapped = ad.forward(**{**kw, "image_latents": il.flip(0)})
    kind, call = ad.engine.calls[-2]
    assert kind == "transformer_forward" and torch.equal(call["image_latents"], il)
    assert (B, 8, 8, Nt, 1, (2 * hc, 2 * wc)) in ad.engine._plans
    assert out.noise_pred.shape == (B, 16, 64) and torch.isfinite(out.log_prob).all()
    assert not torch.equal(swapped.noise_pred, out.noise_pred)                     # each sample's own condition
    with torch.no_grad(), pytest.raises(ValueError, match="rows"):
        ad.forward(**{**kw, "latent_ids": stacked["latent_ids"].flip(0)})
    assert F.FakeTransformer.calls == 0


def test_grad_fallback_runs_the_references_forward_with_the_engines_values(adapter, monkeypatch):
    """A trainable parameter outside the native backward's scope: refused by default; with MI355_ALLOW_REFERENCE_AUTOGRAD=1 the reference's
    own `Flux1KontextAdapter.forward` runs with autograd -- the concatenated image stream and the joint ids reach the torch transformer --
    and the values are the engine's."""
    ad, tr = adapter
    ad.rollout()
    ad._set_timesteps(ad.scheduler, 10, seq_len=16, device="cpu")
    B, Nt, hc, wc = 2, 7, 2, 3
    g = torch.Generator().manual_seed(5)
    pe, pp = torch.randn(B, Nt, 128, generator=g).bfloat16(), torch.randn(B, 128, generator=g).bfloat16()
    il, image_ids = _condition(B, hc, wc, seed=1)
    from mi355_flow.flux import prepare_latent_image_ids
    latent_ids = torch.cat([prepare_latent_image_ids(4, 4, "cpu", torch.bfloat16), image_ids])
    lat = torch.randn(B, 16, 64, generator=g).half()
    kw = dict(t=torch.tensor([900.0, 900.0]), t_next=torch.tensor([750.0, 750.0]), latents=lat, next_latents=(lat * 0.9).half(), image_latents=il,
              latent_ids=latent_ids, prompt_embeds=pe, pooled_prompt_embeds=pp, guidance_scale=3.5, noise_level=0.7, compute_log_prob=True,
              return_kwargs=["log_prob", "noise_pred"])
    with torch.no_grad():
        native = ad.forward(**kw)
    wq = tr.get_submodule("transformer_blocks.0.attn.to_q").weight
    tr.get_submodule("x_embedder").weight.requires_grad_(True)                  # outside the engine's gradient scope
    wq.requires_grad_(True)
    seen = {}

    def torch_transformer(hidden_states=None, img_ids=None, **kw_):
        seen.update(rows=hidden_states.shape[1], img_ids=img_ids)
        return (hidden_states.float() * wq.float().mean(),)

    tr.forward = torch_transformer
    try:
        monkeypatch.delenv("MI355_ALLOW_REFERENCE_AUTOGRAD", raising=False)
        with torch.enable_grad(), pytest.raises(NotImplementedError, match="MI355_ALLOW_REFERENCE_AUTOGRAD"):
            ad.forward(**kw)
        monkeypatch.setenv("MI355_ALLOW_REFERENCE_AUTOGRAD", "1")
        with torch.enable_grad():
            out = ad.forward(**kw)
    finally:
        del tr.forward
    assert seen["rows"] == 16 + hc * wc and torch.equal(seen["img_ids"], latent_ids)
    assert out.log_prob.requires_grad and torch.equal(out.log_prob.detach(), native.log_prob)
    assert torch.equal(out.noise_pred.detach().float(), native.noise_pred.float()) and out.noise_pred.shape == (B, 16, 64)
    (gq,) = torch.autograd.grad(out.log_prob.sum(), wq)
    assert torch.isfinite(gq).all() and float(gq.abs().sum()) > 0

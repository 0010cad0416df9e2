"""CPU tests of the Wan image-to-video host layer (`mi355_flow.wan`: `wan_i2v_condition`, `WanConfig.from_hf`, `WanI2VRolloutMixin`;
`mi355_flow.samples.WanI2VSample`) against the reference's `Wan2_I2V_Adapter` (models/wan/wan2_i2v.py)."""
import dataclasses
import inspect
import types

import pytest
import torch


def _ref():
    from oracle import ref_package
    if not ref_package.available():
        pytest.skip("needs the reference tree (build container only)")
    return ref_package.load("flow_factory.models.wan.wan2_i2v")


@pytest.mark.parametrize("num_frames,last", [(1, False), (5, False), (81, False), (5, True), (81, True)])      # (a last frame needs a second one)
def test_wan_i2v_condition_equals_the_reference_prepare_latents(num_frames, last):
    """The reference's own `prepare_latents` (wan2_i2v.py:335-422) on a fake pipeline whose VAE encode returns a given tensor: its
    mask-and-concat equals `wan_i2v_condition` bit for bit."""
    from mi355_flow.wan import wan_i2v_condition
    M = _ref()
    B, H, W = 2, 32, 48
    T, h, w = (num_frames - 1) // 4 + 1, H // 8, W // 8
    g = torch.Generator().manual_seed(num_frames)
    encoded = torch.randn(B, 16, T, h, w, generator=g)
    mean, std = [0.1 * i for i in range(16)], [1.0 + 0.05 * i for i in range(16)]
    vae = types.SimpleNamespace(dtype=torch.float32, config=types.SimpleNamespace(latents_mean=mean, latents_std=std, z_dim=16),
                                encode=lambda video: types.SimpleNamespace(latents=encoded))
    pipe = types.SimpleNamespace(vae=vae, vae_scale_factor_temporal=4, vae_scale_factor_spatial=8, config=types.SimpleNamespace(expand_timesteps=False))
    image = torch.rand(B, 3, H, W, generator=g)
    lat, cond = M.Wan2_I2V_Adapter.prepare_latents(types.SimpleNamespace(pipeline=pipe), image=image, batch_size=B, num_channels_latents=16, height=H,
                                                   width=W, num_frames=num_frames, dtype=torch.float32, device=torch.device("cpu"),
                                                   generator=torch.Generator().manual_seed(1), last_image=image if last else None)
    latent_condition = (encoded - torch.tensor(mean).view(1, 16, 1, 1, 1)) * (1.0 / torch.tensor(std).view(1, 16, 1, 1, 1))
    mine = wan_i2v_condition(latent_condition, num_frames, 4, last_frame=last)
    assert lat.shape == (B, 16, T, h, w) and cond.shape == mine.shape == (B, 20, T, h, w)
    assert torch.equal(cond, mine)
    assert mine[:, :4, 0].eq(1).all() and (T == 1 or last or mine[:, :4, 1:].eq(0).all())


def test_wan_i2v_condition_refuses_frames_that_do_not_fold():
    from mi355_flow.wan import wan_i2v_condition
    with pytest.raises(ValueError, match="do not fold"):
        wan_i2v_condition(torch.zeros(1, 16, 3, 4, 4), 5)


def test_config_mapping_from_hf_configs():
    """HF `in_channels` counts what the patch embedding sees; the engine's is the latent count."""
    from mi355_flow.wan import WanConfig
    i2v_21 = dict(in_channels=36, out_channels=16, num_layers=40, num_attention_heads=40, attention_head_dim=128, ffn_dim=13824, text_dim=4096,
                  freq_dim=256, patch_size=(1, 2, 2), eps=1e-6, image_dim=1280, added_kv_proj_dim=5120)
    c = WanConfig.from_hf(i2v_21)
    assert (c.in_channels, c.out_channels, c.cond_channels, c.image_dim, c.dim, c.ffn_dim, c.num_layers) == (16, 16, 20, 1280, 5120, 13824, 40)
    c = WanConfig.from_hf(types.SimpleNamespace(**dict(i2v_21, image_dim=None, added_kv_proj_dim=None)))       # Wan2.2-I2V-A14B (each expert)
    assert (c.in_channels, c.out_channels, c.cond_channels, c.image_dim) == (16, 16, 20, None)
    c = WanConfig.from_hf(dict(in_channels=16, out_channels=16, num_layers=30, num_attention_heads=12, ffn_dim=8960))                    # T2V-1.3B
    assert c == WanConfig()
    c = WanConfig.from_hf(dict(in_channels=48, out_channels=48, num_layers=30, num_attention_heads=24, ffn_dim=14336))                   # TI2V-5B
    assert (c.in_channels, c.out_channels, c.cond_channels, c.image_dim) == (48, 48, 0, None)
    assert WanConfig(cond_channels=20).to_c().in_channels == 16           # the C struct (ABI) is unchanged: the latent count
    with pytest.raises(ValueError, match="in_channels"):
        WanConfig.from_hf(dict(in_channels=16, out_channels=36))


def test_wan_i2v_sample_field_parity_with_the_reference():
    from mi355_flow.samples import ImageConditionSample, WanI2VSample
    M = _ref()
    ref, mine = M.WanI2VSample, WanI2VSample
    assert [f.name for f in dataclasses.fields(mine)] == [f.name for f in dataclasses.fields(ref)]
    assert mine._shared_fields == ref._shared_fields == frozenset({"first_frame_mask"})
    assert mine._id_fields == ref._id_fields and issubclass(mine, ImageConditionSample)
    assert all(getattr(mine(), n) is None for n in ("image_embeds", "condition", "first_frame_mask"))


@pytest.mark.parametrize("fn_name", ["inference", "forward"])
def test_mixin_signatures_cover_the_reference(fn_name):
    """The trainer filters its kwargs by `inspect.signature`: every parameter of the reference's method, in its order, with its default.
    `inference()` adds `condition=` at the end (the standalone adapter has no VAE encoder) and lets `images` default to None."""
    from mi355_flow.wan import WanI2VRolloutMixin
    M = _ref()
    want = [(n, p.default) for n, p in inspect.signature(getattr(M.Wan2_I2V_Adapter, fn_name)).parameters.items()]
    got = [(n, p.default) for n, p in inspect.signature(getattr(WanI2VRolloutMixin, fn_name)).parameters.items()]
    if fn_name == "inference":
        assert got[-1] == ("condition", None) and got[1] == ("images", None)
        got, want = got[:-1], [("images", None) if n == "images" else (n, d) for n, d in want]
    assert got == want


def test_expand_timesteps_and_raw_images_are_refused_without_a_gpu():
    from mi355_flow.wan import WanI2VRolloutMixin
    m = WanI2VRolloutMixin()
    m.expand_timesteps = True
    with pytest.raises(NotImplementedError, match="expand_timesteps"):
        m.inference(images=None, prompt="a")
    m.expand_timesteps = False
    with pytest.raises(NotImplementedError, match="expand_timesteps"):
        m.forward(torch.zeros(1), torch.zeros(1, 16, 1, 4, 4), torch.zeros(1, 8, 64), condition=torch.zeros(1, 20, 1, 4, 4),
                  first_frame_mask=torch.ones(1, 1, 1, 4, 4))
    with pytest.raises(NotImplementedError, match="no VAE encoder"):
        m._prepare_i2v(None, None, None, 1, 1, 4, 4, 32, 32, 1, None)

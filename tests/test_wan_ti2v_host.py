"""CPU tests of the Wan2.2-TI2V image-to-video host layer (`mi355_flow.wan`: `wan_first_frame_mask`, `WanTI2VRolloutMixin`) against the
reference's `Wan2_I2V_Adapter` with `expand_timesteps` (models/wan/wan2_i2v.py:402-407, :736-741).  The engine's two-group rule rests on one
fact pinned here: the reference's per-token timestep is 0 on the FIRST hp * wp tokens of every sample and t on all others."""
import inspect
import types

import pytest
import torch


def _ref():
    from oracle import ref_package
    if not ref_package.available():
        pytest.skip("needs the reference tree (build container only)")
    return ref_package.load("flow_factory.models.wan.wan2_i2v")


def _prepare(M, B, H, W, num_frames, C=48):
    """the reference's own `prepare_latents` with `expand_timesteps=True` on a fake pipeline whose VAE encode returns a given tensor"""
    h, w = H // 16, W // 16
    g = torch.Generator().manual_seed(num_frames)
    encoded = torch.randn(B, C, 1, h, w, generator=g)
    mean, std = [0.1 * i for i in range(C)], [1.0 + 0.05 * i for i in range(C)]
    seen = {}

    def encode(video):
        seen["frames"] = video.shape[2]
        return types.SimpleNamespace(latents=encoded)

    vae = types.SimpleNamespace(dtype=torch.float32, config=types.SimpleNamespace(latents_mean=mean, latents_std=std, z_dim=C), encode=encode)
    pipe = types.SimpleNamespace(vae=vae, vae_scale_factor_temporal=4, vae_scale_factor_spatial=16, config=types.SimpleNamespace(expand_timesteps=True))
    image = torch.rand(B, 3, H, W, generator=g)
    out = M.Wan2_I2V_Adapter.prepare_latents(types.SimpleNamespace(pipeline=pipe), image=image, batch_size=B, num_channels_latents=C, height=H, width=W,
                                             num_frames=num_frames, dtype=torch.float32, device=torch.device("cpu"),
                                             generator=torch.Generator().manual_seed(1))
    want_cond = (encoded - torch.tensor(mean).view(1, C, 1, 1, 1)) * (1.0 / torch.tensor(std).view(1, C, 1, 1, 1))
    return out, want_cond, seen


@pytest.mark.parametrize("num_frames", [1, 5, 9, 81])
def test_first_frame_mask_equals_the_reference_prepare_latents(num_frames):
    from mi355_flow.wan import wan_first_frame_mask
    M = _ref()
    B, H, W = 2, 96, 160
    T, h, w = (num_frames - 1) // 4 + 1, H // 16, W // 16
    (lat, cond, mask), want_cond, seen = _prepare(M, B, H, W, num_frames)
    mine = wan_first_frame_mask(T, h, w)
    assert lat.shape == (B, 48, T, h, w) and cond.shape == (B, 48, 1, h, w) and seen["frames"] == 1      # the first frame alone is encoded
    assert mask.shape == mine.shape == (1, 1, T, h, w) and mask.dtype == mine.dtype and torch.equal(mask, mine)
    assert torch.equal(cond, want_cond)


@pytest.mark.parametrize("T,h,w", [(3, 6, 10), (1, 6, 10), (13, 30, 52)])
def test_reference_timesteps_are_zero_on_the_first_hp_wp_tokens_and_t_elsewhere(T, h, w):
    """The reference's expression (wan2_i2v.py:740-741) on the reference's mask, against `[0] * head_rows + [t] * (S - head_rows)` per sample:
    patchify orders tokens (frame, y, x), so frame 0 = the first hp * wp tokens -- the rule the kernels select the modulation row by.  The
    merge (:738) on that mask replaces frame 0 and nothing else."""
    from mi355_flow.wan import wan_first_frame_mask
    from oracle import wan_ref as R
    first_frame_mask = wan_first_frame_mask(T, h, w)
    B, t = 2, torch.tensor(874)
    temp_ts = (first_frame_mask[0][0][:, ::2, ::2] * t).flatten()
    timestep = temp_ts.unsqueeze(0).expand(B, -1)
    hp, wp = h // 2, w // 2
    head_rows, S = hp * wp, T * hp * wp
    want = torch.tensor([0.0] * head_rows + [874.0] * (S - head_rows))
    assert timestep.shape == (B, S) and all(torch.equal(timestep[b], want) for b in range(B))
    # the token order the rule relies on: token s of the oracle's (and the engine's) patchify comes from frame s // (hp * wp)
    frame = torch.arange(T, dtype=torch.float32).view(1, 1, T, 1, 1).expand(1, 1, T, h, w).contiguous()
    tok = R.patchify(frame)[0, :, 0]
    assert torch.equal(tok, (torch.arange(S) // head_rows).float())
    g = torch.Generator().manual_seed(T)
    condition, latents = torch.randn(B, 48, 1, h, w, generator=g), torch.randn(B, 48, T, h, w, generator=g)
    merged = (1 - first_frame_mask) * condition + first_frame_mask * latents
    assert torch.equal(merged[:, :, :1], condition) and torch.equal(merged[:, :, 1:], latents[:, :, 1:])


@pytest.mark.parametrize("fn_name", ["inference", "forward"])
def test_mixin_signatures_cover_the_reference(fn_name):
    """The trainer filters its kwargs by `inspect.signature`: every parameter of the reference's method, in its order, with its default.
    `inference()` adds `condition=` at the end (the standalone adapter has no VAE encoder) and lets `images` default to None."""
    from mi355_flow.wan import WanTI2VRolloutMixin
    M = _ref()
    want = [(n, p.default) for n, p in inspect.signature(getattr(M.Wan2_I2V_Adapter, fn_name)).parameters.items()]
    got = [(n, p.default) for n, p in inspect.signature(getattr(WanTI2VRolloutMixin, fn_name)).parameters.items()]
    if fn_name == "inference":
        assert got[-1] == ("condition", None) and got[1] == ("images", None)
        got, want = got[:-1], [("images", None) if n == "images" else (n, d) for n, d in want]
    assert got == want


def test_refusals_without_a_gpu():
    from mi355_flow.wan import Wan2I2VNativeAdapter, Wan2TI2VNativeAdapter, WanConfig, WanI2VRolloutMixin, WanTI2VRolloutMixin, wan_first_frame_mask
    m = WanTI2VRolloutMixin()
    t, lat, enc = torch.zeros(1), torch.zeros(1, 48, 3, 4, 4), torch.zeros(1, 8, 64)
    ff, good = torch.zeros(1, 48, 1, 4, 4), wan_first_frame_mask(3, 4, 4)
    with pytest.raises(ValueError, match="needs `condition`"):
        m.forward(t, lat, enc, first_frame_mask=good)
    with pytest.raises(ValueError, match="needs `first_frame_mask`"):
        m.forward(t, lat, enc, condition=ff)
    wrong_frame, wrong_value = torch.ones_like(good), good.clone()
    wrong_frame[:, :, 2] = 0
    wrong_value[0, 0, 1, 1, 1] = 0.5
    for bad in (good[:, :, :, :2], good.expand(2, 1, 3, 4, 4), wrong_frame, wrong_value, torch.ones_like(good), torch.zeros_like(good)):
        with pytest.raises(ValueError, match="first_frame_mask"):
            m.forward(t, lat, enc, condition=ff, first_frame_mask=bad)
    with pytest.raises(ValueError, match="has shape"):
        m.forward(t, lat, enc, condition=torch.zeros(1, 48, 3, 4, 4), first_frame_mask=good)
    with pytest.raises(ValueError, match="image_embeds"):
        m.forward(t, lat, enc, condition=ff, first_frame_mask=good, image_embeds=torch.zeros(1, 5, 16))
    with pytest.raises(NotImplementedError, match="no VAE encoder"):
        m._prepare_i2v(None, None, None, 1, 1, 4, 4, 64, 64, 1, None)
    with pytest.raises(ValueError, match="text-to-video config"):
        Wan2TI2VNativeAdapter({}, WanConfig(cond_channels=20))
    with pytest.raises(NotImplementedError, match="two experts"):
        Wan2TI2VNativeAdapter({}, WanConfig(in_channels=48, out_channels=48), state_dict_2={})
    # the condition-channel classes keep refusing `expand_timesteps`, and now name the class that serves it
    old = WanI2VRolloutMixin()
    with pytest.raises(NotImplementedError, match="expand_timesteps.*Wan2TI2VNativeAdapter"):
        old.forward(t, torch.zeros(1, 16, 3, 4, 4), enc, condition=torch.zeros(1, 20, 3, 4, 4), first_frame_mask=good)
    with pytest.raises(NotImplementedError, match="expand_timesteps.*Wan2TI2VNativeAdapter"):
        Wan2I2VNativeAdapter({}, WanConfig(cond_channels=20), expand_timesteps=True)

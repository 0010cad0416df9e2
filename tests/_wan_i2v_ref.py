"""TEST INFRASTRUCTURE ONLY: what the Wan image-to-video tests share.

The image cross-attention branch of Wan2.1-I2V has its oracle here: `wan_i2v_forward` restates the block loop of `oracle.wan_ref.wan_forward`
(importing its helpers) with the branch -- `condition_embedder.image_embedder` (LayerNorm with affine, eps 1e-5 -> Linear -> exact GELU ->
Linear -> LayerNorm with affine) on the CLIP hidden states, per block `k_img = RMSNorm_across_heads(add_k_proj(img); norm_added_k)`,
`v_img = add_v_proj(img)`, a second attention of the SAME normalised queries over the image keys, its output added to the text
cross-attention's before `attn2.to_out.0` -- restated from the published `WanTransformer3DModel`.
Channel-only image-to-video (Wan2.2-I2V-A14B: `cat([latents (16), condition (4 mask + 16 latent)], 1)` into a `Conv3d(36, D)` patch embedding,
16 channels out; reference models/wan/wan2_i2v.py:744) needs no oracle of its own: `oracle.wan_ref.wan_forward` with `in_channels=36,
out_channels=16` on the concatenated input IS the oracle, and the rollout loops of `oracle.wan_ref` are fed that input by `with_condition`.
NETWORK BODY: PARITY UNPINNED, like every model body here (oracle/wan_ref.py).
"""
import contextlib
import dataclasses

import torch

COND = 20          # 4 mask + 16 latent channels


def bf(x):
    return x.bfloat16().float()


def oracle_config(R, **kw):
    """The oracle's config of an image-to-video transformer: 36 channels in, 16 out."""
    base = kw.pop("base", None) or R.tiny_config()
    return dataclasses.replace(base, in_channels=16 + COND, out_channels=16, **kw)


def engine_config(wn, cfg_o, cond_channels=COND, image_dim=None):
    return wn.WanConfig(num_layers=cfg_o.num_layers, num_attention_heads=cfg_o.num_attention_heads, ffn_dim=cfg_o.ffn_dim, text_dim=cfg_o.text_dim,
                        cond_channels=cond_channels, image_dim=image_dim or None)


def make_condition(B, T, h, w, g, scale=1.0):
    """A synthetic condition of the real structure: a 0 / 1 mask (first latent frame given) over `scale` x normal latents."""
    mask = torch.zeros(B, 4, T, h, w)
    mask[:, :, 0] = 1.0
    return torch.cat([mask, bf(scale * torch.randn(B, 16, T, h, w, generator=g))], 1)


def image_shapes(cfg_o, image_dim):
    """HF names and shapes of the image branch's parameters."""
    D, ie = cfg_o.dim, "condition_embedder.image_embedder."
    out = {ie + "norm1.weight": (image_dim,), ie + "norm1.bias": (image_dim,), ie + "ff.net.0.proj.weight": (image_dim, image_dim),
           ie + "ff.net.0.proj.bias": (image_dim,), ie + "ff.net.2.weight": (D, image_dim), ie + "ff.net.2.bias": (D,),
           ie + "norm2.weight": (D,), ie + "norm2.bias": (D,)}
    for i in range(cfg_o.num_layers):
        for n in ("add_k_proj", "add_v_proj"):
            out[f"blocks.{i}.attn2.{n}.weight"], out[f"blocks.{i}.attn2.{n}.bias"] = (D, D), (D,)
        out[f"blocks.{i}.attn2.norm_added_k.weight"] = (D,)
    return out


def shapes(R, cfg_o, image_dim=0):
    out = dict(R.state_dict_shapes(cfg_o))
    if image_dim:
        out.update(image_shapes(cfg_o, image_dim))
    return out


def make_state_dict(R, cfg_o, seed, image_dim=0, std=0.03):
    """`oracle.wan_ref.make_synthetic_state_dict` plus the image branch's parameters (norm weights around 1), bf16-representable."""
    sd = dict(R.make_synthetic_state_dict(cfg_o, seed, std))
    g = torch.Generator().manual_seed(seed + 1000)
    for n, sh in (image_shapes(cfg_o, image_dim).items() if image_dim else ()):
        t = torch.randn(sh, generator=g) * std
        if "norm_added_k" in n or n.endswith(("norm1.weight", "norm2.weight")):
            t = t + 1.0
        sd[n] = t
    return {k: bf(v) for k, v in sd.items()}


def wan_i2v_forward(R, sd, cfg, latents, timestep, enc, image_embeds=None, quant=None, image_branch=True):
    """`oracle.wan_ref.wan_forward` (scalar timesteps) with the image cross-attention branch: latents (B, 36, T, h, w) already concatenated,
    image_embeds (B, Ni, image_dim).  `image_branch=False` drops the branch (what a forgotten term computes)."""
    import torch.nn.functional as F
    q = quant or (lambda x: x)
    D, H, eps = cfg.dim, cfg.num_attention_heads, cfg.eps
    lin = lambda n, x: F.linear(q(x), q(sd[n + ".weight"]), sd[n + ".bias"])      # noqa: E731
    ln = lambda x: F.layer_norm(x, (D,), eps=eps)                                # noqa: E731
    B, C, T, h, w = latents.shape
    cos, sin = R.rope_cos_sin(T, h // 2, w // 2, cfg.attention_head_dim)
    cos, sin = cos.to(latents.device), sin.to(latents.device)
    x = q(F.linear(q(R.patchify(latents.float())), q(sd["patch_embedding.weight"].reshape(D, -1)), sd["patch_embedding.bias"]))
    temb = q(lin("condition_embedder.time_embedder.linear_2",
                 F.silu(q(lin("condition_embedder.time_embedder.linear_1", q(R.timestep_embedding(timestep.float().flatten(), cfg.freq_dim).to(latents.device)))))))
    tproj = q(lin("condition_embedder.time_proj", q(F.silu(temb)))).view(B, 6, D)
    ctx = q(lin("condition_embedder.text_embedder.linear_2", q(F.gelu(lin("condition_embedder.text_embedder.linear_1", enc.float()), approximate="tanh"))))
    img = None
    if image_embeds is not None and image_branch:
        ie = "condition_embedder.image_embedder."
        Di = image_embeds.shape[-1]
        z = q(F.layer_norm(image_embeds.float(), (Di,), sd[ie + "norm1.weight"], sd[ie + "norm1.bias"], 1e-5))
        z = q(F.gelu(q(lin(ie + "ff.net.0.proj", z))))                         # exact (erf) GELU
        z = q(lin(ie + "ff.net.2", z))
        img = q(F.layer_norm(z, (D,), sd[ie + "norm2.weight"], sd[ie + "norm2.bias"], 1e-5))

    def attention(qq, kk, vv):
        o = F.scaled_dot_product_attention(q(qq), q(kk), q(vv))
        return q(o.transpose(1, 2).reshape(o.shape[0], o.shape[2], D))

    for i in range(cfg.num_layers):
        b = f"blocks.{i}"
        m = (sd[f"{b}.scale_shift_table"] + tproj.float()).unbind(-2)
        xn = q(ln(x) * (1 + m[1][:, None]) + m[0][:, None])
        qq = R.apply_rope(R._heads(R._rms(q(lin(f"{b}.attn1.to_q", xn)), sd[f"{b}.attn1.norm_q.weight"], eps), H), cos, sin)
        kk = R.apply_rope(R._heads(R._rms(q(lin(f"{b}.attn1.to_k", xn)), sd[f"{b}.attn1.norm_k.weight"], eps), H), cos, sin)
        vv = R._heads(lin(f"{b}.attn1.to_v", xn), H)
        x = q(x + q(lin(f"{b}.attn1.to_out.0", attention(qq, kk, vv))) * m[2][:, None])
        xn = q(F.layer_norm(x, (D,), sd[f"{b}.norm2.weight"], sd[f"{b}.norm2.bias"], eps))
        qq = R._heads(R._rms(q(lin(f"{b}.attn2.to_q", xn)), sd[f"{b}.attn2.norm_q.weight"], eps), H)
        kk = R._heads(R._rms(q(lin(f"{b}.attn2.to_k", ctx)), sd[f"{b}.attn2.norm_k.weight"], eps), H)
        vv = R._heads(lin(f"{b}.attn2.to_v", ctx), H)
        o = attention(qq, kk, vv)
        if img is not None:
            ki = R._heads(R._rms(q(lin(f"{b}.attn2.add_k_proj", img)), sd[f"{b}.attn2.norm_added_k.weight"], eps), H)
            vi = R._heads(lin(f"{b}.attn2.add_v_proj", img), H)
            o = q(o + attention(qq, ki, vi))
        x = q(x + q(lin(f"{b}.attn2.to_out.0", o)))
        xn = q(ln(x) * (1 + m[4][:, None]) + m[3][:, None])
        x = q(x + q(lin(f"{b}.ffn.net.2", q(F.gelu(lin(f"{b}.ffn.net.0.proj", xn), approximate="tanh")))) * m[5][:, None])
    mo = (sd["scale_shift_table"] + temb.float().unsqueeze(-2)).unbind(-2)
    xo = q(ln(x) * (1 + mo[1][:, None]) + mo[0][:, None])
    return R.unpatchify(q(lin("proj_out", xo)), T, h, w, cfg.out_channels)


def forward(R, sd, cfg_o, x, t, enc, cond, quant=None, image_embeds=None, image_branch=True):
    """The oracle on `cat([latents, condition], 1)`: `oracle.wan_ref.wan_forward` itself without image embeddings, `wan_i2v_forward` with."""
    x36 = torch.cat([x.float(), cond.float().to(x.device)], 1)
    if image_embeds is None:
        return R.wan_forward(sd, cfg_o, x36, t, enc, quant=quant)
    return wan_i2v_forward(R, sd, cfg_o, x36, t, enc, image_embeds.float().to(x.device), quant=quant, image_branch=image_branch)


@contextlib.contextmanager
def with_condition(R, cfg_o, cond, image_embeds=None):
    """Inside: `R.wan_forward(sd, <any cfg>, latents16, ...)` -- as the oracle's rollout loops call it -- runs the 36-channel network on
    `cat([latents, cond], 1)` (with the image branch when `image_embeds` are given)."""
    orig = R.wan_forward

    def fwd(sd, _cfg, latents, timestep, enc, quant=None):
        x36 = torch.cat([latents.float(), cond.float().to(latents.device)], 1)
        if image_embeds is not None:
            return wan_i2v_forward(R, sd, cfg_o, x36, timestep, enc, image_embeds.float(), quant=quant)
        return orig(sd, cfg_o, x36, timestep, enc, quant=quant)

    R.wan_forward = fwd
    try:
        yield
    finally:
        R.wan_forward = orig

"""TEST INFRASTRUCTURE ONLY: what the Wan2.2-TI2V image-to-video tests share.

The oracle is `oracle.wan_ref.wan_forward` itself: it takes a `(B, S)` timestep (one per token).  The reference's TI2V step (models/wan/
wan2_i2v.py:736-741) feeds the transformer `(1 - first_frame_mask) * condition + first_frame_mask * latents` and
`first_frame_mask[0][0][:, ::2, ::2] * t` per token; both are restated here from those two lines (`merged`, `token_timesteps`).
NETWORK BODY: PARITY UNPINNED, like every model body here (oracle/wan_ref.py).

The per-token timestep matters at these weights: on the tiny configuration the fp32 oracle with the SCALAR timestep on the same merged input
lies 7 % .. 14 % (rel-L2) from the per-token one, against a bf16 band of 0.5 % -- measured on the CPU before the first GPU run, and asserted
by the forward test, which could not tell the feature from its absence otherwise.
"""
import contextlib
import dataclasses

import torch

C = 48                # Wan2.2-TI2V-5B: 48 latent channels in and out


def bf(x):
    return x.bfloat16().float()


def oracle_config(R, **kw):
    base = kw.pop("base", None) or R.tiny_config()
    return dataclasses.replace(base, in_channels=C, out_channels=C, **kw)


def engine_config(wn, cfg_o):
    return wn.WanConfig(in_channels=C, out_channels=C, num_layers=cfg_o.num_layers, num_attention_heads=cfg_o.num_attention_heads,
                        ffn_dim=cfg_o.ffn_dim, text_dim=cfg_o.text_dim)


def make_state_dict(R, cfg_o, seed):
    return {k: bf(v) for k, v in R.make_synthetic_state_dict(cfg_o, seed).items()}


def first_frame_mask(T, h, w, device=None):
    """as the reference's `prepare_latents` builds it (wan2_i2v.py:402-407)"""
    m = torch.ones(1, 1, T, h, w, device=device)
    m[:, :, 0] = 0
    return m


def merged(x, ff):
    """wan2_i2v.py:738: (1 - first_frame_mask) * condition + first_frame_mask * latents"""
    m = first_frame_mask(*x.shape[2:], device=x.device)
    return (1 - m) * ff.float().to(x.device) + m * x.float()


def token_timesteps(t, B, T, h, w, device=None):
    """wan2_i2v.py:740-741: (first_frame_mask[0][0][:, ::2, ::2] * t).flatten(), expanded to the batch; t a 0-d or one-element tensor"""
    m = first_frame_mask(T, h, w, device=device)
    return (m[0][0][:, ::2, ::2] * t.reshape(()).to(m.device)).flatten().unsqueeze(0).expand(B, -1)


def forward(R, sd, cfg_o, x, t, enc, ff, quant=None, per_token=True):
    """The oracle on the merged input with the per-token timestep; `per_token=False`: the scalar timestep on the same input (what an engine
    that modulates per sample computes)."""
    B, _, T, h, w = x.shape
    ts = token_timesteps(t, B, T, h, w, device=x.device) if per_token else t.reshape(-1)[:1].to(x.device).expand(B)
    return R.wan_forward(sd, cfg_o, merged(x, ff), ts, enc, quant=quant)


def pair(R, sd, cfg_o, x, t, ne, pe, ff, n_cfg, quant=None, per_token=True):
    pos = forward(R, sd, cfg_o, x, t, pe, ff, quant=quant, per_token=per_token)
    return torch.cat([forward(R, sd, cfg_o, x, t, ne, ff, quant=quant, per_token=per_token), pos]) if n_cfg == 2 else pos


@contextlib.contextmanager
def with_first_frame(R, cfg_o, ff):
    """Inside: `R.wan_forward(sd, <any cfg>, latents, t (B,), ...)` -- as the oracle's rollout loops call it -- runs the network on the merged
    input with the per-token timestep; the loops' scheduler step keeps the unmerged latents, as the reference's does."""
    orig = R.wan_forward

    def fwd(sd, _cfg, latents, timestep, enc, quant=None):
        B, _, T, h, w = latents.shape
        return orig(sd, cfg_o, merged(latents, ff), token_timesteps(timestep.reshape(-1)[0], B, T, h, w, device=latents.device), enc, quant=quant)

    R.wan_forward = fwd
    try:
        yield
    finally:
        R.wan_forward = orig

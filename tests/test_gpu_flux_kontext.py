"""GPU tests of FLUX.1 Kontext on the FLUX engine (reference src/flow_factory/models/flux/flux1_kontext.py:337-589): the condition image's
packed latents behind the target's in the image stream (`cat([latents, image_latents], dim=1)`), rotary ids (1, row, col) on the condition
image's own grid, and only the target rows of the prediction in the scheduler step.  Everything goes through the C ABI
(`mi355_flux_plan_create_cond`, `mi355_flux_{forward,forward_train,rollout}_cond`, `mi355_flux_plan_rope_table`, `mi355_flux_backward`).

The reference is the oracle's own FLUX.1 forward (oracle/flux_ref.py takes arbitrary `img_ids`) on the concatenated stream, cut to the
target rows, followed by the oracle's scheduler step.  Weights are drawn at std 0.06: at the default 0.03 dropping the condition moves the
tiny model's output by 1.2e-2, inside the 2e-2 of the plain forward tests -- a test that passes with the feature broken.  Every oracle
comparison therefore also asserts its own sensitivity: the oracle WITHOUT the condition lies at least 3 x the applied tolerance away.

Shapes (target latent h, w / condition latent h, w / Nt / B), the smallest that cross the edges:
  (8,8 / 8,8 / 16 / 2)      Ni 16, Nc 16, S 48:   one key tile, equal grids, per-sample conditions
  (6,10 / 10,4 / 13 / 1)    Ni 15, Nc 10, S 38:   nothing a multiple of anything, non-square condition
  (16,16 / 8,12 / 64 / 2)   Ni 64, Nc 24, S 152:  three key tiles with a ragged last one, condition smaller than the target
"""
import math

import numpy as np
import pytest
import torch

import _plugin_fakes as PF

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 8, 8, 16, 2), (6, 10, 10, 4, 13, 1), (16, 16, 8, 12, 64, 2)]
STD = 0.06


def _bf(x):
    return x.bfloat16().float()


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


def _cos(a, b):
    a, b = a.detach().float().cpu().flatten(), b.detach().float().cpu().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import flux
    return flux


def _engine_cfg(fx, cfg_o):
    return fx.FluxConfig(num_layers=cfg_o.num_layers, num_single_layers=cfg_o.num_single_layers, num_attention_heads=cfg_o.num_attention_heads,
                         joint_attention_dim=cfg_o.joint_attention_dim, pooled_projection_dim=cfg_o.pooled_projection_dim,
                         guidance_embeds=cfg_o.guidance_embeds)


def _setup(fx, cfg_o, seed=77, std=STD):
    from oracle import flux_ref as R
    sd = {k: _bf(v) for k, v in R.make_synthetic_state_dict(cfg_o, seed, std=std).items()}
    return sd, _engine_cfg(fx, cfg_o)


def _cond_ids(hc, wc):
    from oracle import flux_ref as R
    ids = R.prepare_img_ids(hc, wc)
    ids[:, 0] = 1
    return ids


def _kontext_forward(sd, cfg_o, x, c, tm, gm, pool, enc, ids, cond_ids, quant=None):
    """The Kontext reference (flux1_kontext.py:559-575): the FLUX.1 forward on the concatenated stream and ids, target rows only."""
    from oracle import flux_ref as R
    out = R.flux_forward(sd, cfg_o, torch.cat([x, c], 1), tm, gm, pool, enc, torch.cat([ids, cond_ids.to(ids.device)]), quant=quant, premultiplied=True)
    return out[:, :x.shape[1]]


def _forward_inputs(cfg_o, h, w, ch, cw, Nt, B, seed):
    from oracle import flux_ref as R
    g = torch.Generator().manual_seed(seed)
    x = R.pack_latents(torch.randn(B, 16, h, w, generator=g)).half()
    c = R.pack_latents(torch.randn(B, 16, ch, cw, generator=g)).bfloat16()        # a different condition per sample
    enc = _bf(torch.randn(B, Nt, cfg_o.joint_attention_dim, generator=g))
    pool = _bf(torch.randn(B, cfg_o.pooled_projection_dim, generator=g))
    return x, c, enc, pool, torch.tensor([900.0, 412.5][:B]), torch.full((B,), 3500.0)


# ------------------------------------------------------------------------------------------------- 1. rotary table
@pytest.mark.parametrize("h,w,ch,cw,Nt,B", SHAPES)
def test_kontext_rope_table_matches_oracle(fx, h, w, ch, cw, Nt, B):
    """The plan's [S][64] (cos, sin) table of [text (0,0,0) | target (0, r, c) | condition (1, r, c) on its own grid].  The output tests cannot
    make this check: a first id of 0 in place of 1 moves the output by 1.1e-2 against a band of 8.5e-3; in the table it moves cos from 0.54 to 1.
    atol 2.4e-7 = 2 fp32 ulp of values in [-1, 1]: both sides evaluate the angle in float64 and round once to fp32; another `pow` can move the
    float64 angle by a last bit and the rounded value by one ulp."""
    from oracle import flux_ref as R
    cfg_o = R.tiny_config()
    eng = fx.FluxEngine(_engine_cfg(fx, cfg_o))
    try:
        plan = eng.plan(B, h, w, Nt, 1, cond=(ch, cw))
        assert (plan.Ni, plan.Nc, plan.Nx) == ((h // 2) * (w // 2), (ch // 2) * (cw // 2), (h // 2) * (w // 2) + (ch // 2) * (cw // 2))
        got = plan.rope_table()
        cos, sin = R.rope_cos_sin(torch.cat([torch.zeros(Nt, 3), R.prepare_img_ids(h // 2, w // 2), _cond_ids(ch // 2, cw // 2)]), cfg_o.axes_dims_rope)
        want = torch.stack([cos[:, 0::2], sin[:, 0::2]], dim=-1)
        assert got.shape == want.shape == (Nt + plan.Nx, 64, 2)
        err = float((got - want).abs().max())
        print(f"Kontext rotary table {h}x{w} / {ch}x{cw} / Nt {Nt}: max |engine - oracle| {err:.3e}")
        assert err <= 2.4e-7, err
        assert abs(float(got[Nt + plan.Ni, 0, 0]) - math.cos(1.0)) < 1e-6        # the first condition row: id (1, 0, 0)
        # a plain plan's table is the prefix
        plain = eng.plan(B, h, w, Nt, 1).rope_table()
        assert torch.equal(plain, got[:Nt + plan.Ni])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("h,w,ch,cw,Nt,B,guidance_embeds", [s + (ge,) for s, ge in zip(SHAPES, (True, True, False))])
def test_kontext_forward_matches_oracle(fx, h, w, ch, cw, Nt, B, guidance_embeds):
    from oracle import flux_ref as R
    from _gpu_oracle import check_in_band, ref_on_gpu, rel
    cfg_o = R.tiny_config()
    cfg_o.guidance_embeds = guidance_embeds
    sd, cfg = _setup(fx, cfg_o)
    eng = fx.FluxEngine(cfg)
    try:
        eng.bind_state_dict({k: v.cuda() for k, v in sd.items()})
        eng.ready()
        x, c, enc, pool, tm, gm = _forward_inputs(cfg_o, h, w, ch, cw, Nt, B, seed=h * w + Nt)
        ids, cids = R.prepare_img_ids(h // 2, w // 2), _cond_ids(ch // 2, cw // 2)
        plan = eng.plan(B, h, w, Nt, 1, cond=(ch, cw))
        got = plan.transformer_forward(x.cuda(), tm, gm if guidance_embeds else None, enc.cuda(), pool.cuda(), image_latents=c.cuda())
        assert got.shape == (B, plan.Ni, 64)
        ref, _, r, band = check_in_band(f"Kontext forward {h}x{w} / {ch}x{cw} / Nt {Nt} / B {B}", got, _kontext_forward, sd, cfg_o, x.float(),
                                        c.float(), tm, gm, pool, enc, ids, cids)
        tol = 1.5 * band + 1e-3
        no_cond = rel(ref_on_gpu(R.flux_forward, sd, cfg_o, x.float(), tm, gm, pool, enc, ids, premultiplied=True), ref)
        print(f"  without the condition the oracle moves by {no_cond:.3e} = {no_cond / tol:.1f} x the tolerance {tol:.3e}")
        assert no_cond >= 3 * tol, (no_cond, tol)
        if B > 1:       # per-sample conditions: swapping them is seen too
            swapped = rel(ref_on_gpu(_kontext_forward, sd, cfg_o, x.float(), c.float().flip(0), tm, gm, pool, enc, ids, cids), ref)
            assert swapped >= 3 * tol, (swapped, tol)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- 3. / 4. rollout
def _adapter(fx, cfg_o, sd, sched):
    ad = fx.Flux1KontextNativeAdapter({k: v.cuda() for k, v in sd.items()}, _engine_cfg(fx, cfg_o), sched, latent_storage_dtype="fp16")
    ad.rollout()
    return ad


def _rollout_case(cfg_o, B, Nt, ch, cw, seed=9):
    from oracle import flux_ref as R
    g = torch.Generator().manual_seed(seed)
    pe = torch.randn(B, Nt, cfg_o.joint_attention_dim, generator=g).bfloat16()
    pp = torch.randn(B, cfg_o.pooled_projection_dim, generator=g).bfloat16()
    il = R.pack_latents(torch.randn(B, 16, ch, cw, generator=g)).bfloat16()
    image_ids = _cond_ids(ch // 2, cw // 2).unsqueeze(0).expand(B, -1, -1)          # batched, as the reference's encode_image returns them
    cond_imgs = torch.rand(B, 3, ch * 8, cw * 8, generator=g)
    return pe, pp, il, image_ids, cond_imgs


def test_kontext_rollout_matches_oracle_and_replays(fx):
    """`test_flux_rollout_matches_oracle_and_replays` with a condition: N-step rollout (latents, per-step log-probs) against an oracle loop on
    identical draws in the reference's order; the replay of a stored transition through `forward(..., image_latents=, latent_ids=)` gives
    ratio == 1 exactly; a repeated call (the captured graph) repeats the bits."""
    from oracle import flux_ref as R
    from _gpu_oracle import bf16_round
    from mi355_flow.scheduler import FlowMatchEulerDiscreteSDEScheduler
    cfg_o = R.tiny_config()
    sd, _ = _setup(fx, cfg_o, seed=11)
    sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[0, 1, 2, 3], num_sde_steps=2, seed=42, dynamics_type="Flow-SDE",
                                               shift=3.0, use_dynamic_shifting=True)
    ad = _adapter(fx, cfg_o, sd, sched)
    try:
        B, Nt, N, H, W, ch, cw = 2, 16, 5, 128, 128, 8, 12
        h = w = H // 8
        Ni, Nc = (h // 2) * (w // 2), (ch // 2) * (cw // 2)
        pe, pp, il, image_ids, cond_imgs = _rollout_case(cfg_o, B, Nt, ch, cw)
        kw = dict(prompt=["a", "b"], height=H, width=W, num_inference_steps=N, guidance_scale=3.5, prompt_embeds=pe.cuda(),
                  pooled_prompt_embeds=pp.cuda(), condition_images=cond_imgs, image_latents=il.cuda(), image_ids=image_ids.cuda(),
                  trajectory_indices="all")
        torch.cuda.manual_seed(77)
        samples = ad.inference(**kw)
        # identical draws, in the reference's order
        torch.cuda.manual_seed(77)
        init = R.pack_latents(torch.randn((B, 16, h, w), device="cuda", dtype=torch.bfloat16)).cpu()
        noise = torch.stack([torch.randn((B, Ni, 64), device="cuda", dtype=torch.float32) for _ in range(N)]).cpu()
        ts = samples[0].timesteps.float().cpu()
        sig = ad.scheduler.sigmas.float().cpu()
        nl = ad.scheduler.host_noise_levels()
        assert sum(e > 0 for e in nl) == 2
        # seq_len = Ni for the dynamic shift: the plain FLUX.1 adapter's schedule at the same target size
        from mi355_flow.scheduler import set_scheduler_timesteps
        ref_sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[0, 1, 2, 3], num_sde_steps=2, seed=42, dynamics_type="Flow-SDE",
                                                       shift=3.0, use_dynamic_shifting=True)
        assert torch.equal(set_scheduler_timesteps(ref_sched, N, seq_len=Ni, device="cpu").float(), ts)
        ids = torch.cat([R.prepare_img_ids(h // 2, w // 2), _cond_ids(ch // 2, cw // 2)])

        def denoiser(quant):
            def run(hidden_states, timestep, guidance, pooled_projections, encoder_hidden_states, txt_ids, img_ids):
                tm = R.model_scalar(timestep, hidden_states.dtype)
                gm = R.model_scalar(guidance.float(), hidden_states.dtype)
                out = R.flux_forward(sd, cfg_o, torch.cat([hidden_states.float(), il.float()], 1), tm, gm, pooled_projections.float(),
                                     encoder_hidden_states.float(), img_ids, quant=quant, premultiplied=True)
                return out[:, :hidden_states.shape[1]]
            return run

        ref = R.rollout(sd, cfg_o, pe, pp, 3.5, init, noise, ts, sig, nl, ids, torch.float16, denoiser=denoiser(None))
        refq = R.rollout(sd, cfg_o, pe, pp, 3.5, init, noise, ts, sig, nl, ids, torch.float16, denoiser=denoiser(bf16_round))
        assert len(samples) == B and samples[0].all_latents.shape == (N + 1, Ni, 64) and samples[0].all_latents.dtype == torch.float16
        assert tuple(samples[0].latent_ids.shape) == (Ni + Nc, 3) and torch.equal(samples[0].latent_ids.float().cpu(), ids)
        sde = [i for i in range(N) if nl[i] > 0]
        for b in range(B):
            assert torch.equal(samples[b].image_latents.cpu(), il[b]) and samples[b].condition_images[0].shape == (3, ch * 8, cw * 8)
            got = samples[b].all_latents.float().cpu()
            for pos in range(N + 1):
                r_, q_ = ref["all_latents"][pos, b].float(), refq["all_latents"][pos, b].float()
                band = float((q_ - r_).norm() / r_.norm())
                err = float((got[pos] - r_).norm() / r_.norm())
                print(f"Kontext rollout sample {b} position {pos}: engine vs oracle {err:.3e}, band {band:.3e}")
                assert err < 1.5 * band + 1e-3, (b, pos, err, band)
            lp = samples[b].log_probs.cpu()
            assert lp.shape == (len(sde),)
            torch.testing.assert_close(lp, torch.stack([ref["log_probs"][i, b] for i in sde]), rtol=1e-3, atol=1e-4)
        # replay (grpo.py:229-263): stored (x_i, x_{i+1}) of an SDE step through forward()
        i = sde[0]
        x_i = torch.stack([s.all_latents[i] for s in samples]).cuda()
        x_n = torch.stack([s.all_latents[i + 1] for s in samples]).cuda()
        t = samples[0].timesteps[i].reshape(1).expand(B).cuda()
        t_next = samples[0].timesteps[i + 1].reshape(1).expand(B).cuda()
        out = ad.forward(t=t, latents=x_i, image_latents=torch.stack([s.image_latents for s in samples]).cuda(), latent_ids=samples[0].latent_ids,
                         prompt_embeds=pe.cuda(), pooled_prompt_embeds=pp.cuda(), t_next=t_next, next_latents=x_n, guidance_scale=3.5,
                         noise_level=nl[i], compute_log_prob=True, return_kwargs=["log_prob", "next_latents_mean"])
        old = torch.stack([s.log_probs[0] for s in samples]).cuda()
        assert torch.equal(torch.exp(out.log_prob - old), torch.ones_like(old))
        # the second call captures the loop as a graph, the third replays it: same seed, same bits; another condition changes them
        for _ in range(2):
            torch.cuda.manual_seed(77)
            again = ad.inference(**kw)
            for sa, sb in zip(samples, again):
                assert torch.equal(sa.all_latents, sb.all_latents) and torch.equal(sa.log_probs, sb.log_probs)
        torch.cuda.manual_seed(77)
        other = ad.inference(**dict(kw, image_latents=il.flip(0).cuda()))
        assert not torch.equal(other[0].all_latents[-1], samples[0].all_latents[-1])
    finally:
        ad.engine.close()


def test_kontext_fused_rollout_equals_stepwise(fx):
    """The fused rollout embeds the condition ONCE; the stepwise path (`_rollout_stepwise`: one `transformer_forward` per step with the same
    `image_latents`, taken when per-step callback tensors are asked for) embeds it every step.  Every kept latent and log-prob is bit-identical."""
    from oracle import flux_ref as R
    from mi355_flow.scheduler import FlowMatchEulerDiscreteSDEScheduler
    cfg_o = R.tiny_config()
    sd, _ = _setup(fx, cfg_o, seed=3)
    sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[0, 1, 2], num_sde_steps=2, seed=1, dynamics_type="Flow-SDE",
                                               shift=3.0, use_dynamic_shifting=True)
    ad = _adapter(fx, cfg_o, sd, sched)
    try:
        B, Nt, ch, cw = 2, 16, 8, 12
        pe, pp, il, image_ids, _ = _rollout_case(cfg_o, B, Nt, ch, cw, seed=1)
        kw = dict(prompt=["a", "b"], height=64, width=80, num_inference_steps=4, guidance_scale=3.5, prompt_embeds=pe.cuda(),
                  pooled_prompt_embeds=pp.cuda(), image_latents=il.cuda(), image_ids=image_ids[0].cuda())
        calls = []
        stepwise = ad._rollout_stepwise
        ad._rollout_stepwise = lambda *a, **k: (calls.append(1), stepwise(*a, **k))[1]
        torch.cuda.manual_seed(5)
        a = ad.inference(**kw)
        assert not calls
        torch.cuda.manual_seed(5)
        b = ad.inference(**kw, extra_call_back_kwargs=["noise_pred", "noise_level"])
        assert calls == [1]
        for sa, sb in zip(a, b):
            assert torch.equal(sa.all_latents, sb.all_latents) and torch.equal(sa.log_probs, sb.log_probs)
            assert sb.extra_kwargs["noise_pred"].shape[0] == 4 and sb.extra_kwargs["noise_pred"].shape[1:] == sa.all_latents.shape[1:]
            assert sa.condition_images is None and sa.all_latents.shape[1:] == (4 * 5, 64)
    finally:
        ad.engine.close()


# ------------------------------------------------------------------------------------------------- 5. training forward
@pytest.mark.parametrize("h,w,ch,cw,Nt,B", SHAPES[:2])
def test_kontext_forward_train_velocity_is_bit_identical(fx, h, w, ch, cw, Nt, B):
    from oracle import flux_ref as R
    cfg_o = R.tiny_config()
    sd, cfg = _setup(fx, cfg_o)
    eng = fx.FluxEngine(cfg)
    try:
        eng.bind_state_dict({k: v.cuda() for k, v in sd.items()})
        eng.ready()
        x, c, enc, pool, tm, gm = _forward_inputs(cfg_o, h, w, ch, cw, Nt, B, seed=3)
        plan = eng.plan(B, h, w, Nt, 1, cond=(ch, cw))
        args = (x.cuda(), tm, gm, enc.cuda(), pool.cuda())
        v = plan.transformer_forward(*args, image_latents=c.cuda()).clone()
        vt = plan.forward_train(*args, image_latents=c.cuda()).clone()
        assert torch.isfinite(v.float()).all() and torch.equal(v, vt)
        assert torch.equal(plan.transformer_forward(*args, image_latents=c.cuda()), v)       # ... and the stash run leaves the plan as it was
        assert plan.training_bytes > 0
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- 6. / 7. gradients
BLOCK_LINEARS = (".attn.to_q.", ".attn.to_k.", ".attn.to_v.", ".attn.to_out.0.", ".attn.add_q_proj.", ".attn.add_k_proj.", ".attn.add_v_proj.",
                 ".attn.to_add_out.", ".ff.net.0.proj.", ".ff.net.2.", ".ff_context.net.0.proj.", ".ff_context.net.2.", ".proj_mlp.", ".proj_out.")
# the reference's FLUX.1 Kontext default target modules (models/flux/flux1_kontext.py:139-146)
DEFAULT_TARGETS = ("attn.to_k.", "attn.to_q.", "attn.to_v.", "attn.to_out.0.", "attn.add_k_proj.", "attn.add_q_proj.", "attn.add_v_proj.",
                   "attn.to_add_out.", "ff.net.0.proj.", "ff.net.2.", "ff_context.net.0.proj.", "ff_context.net.2.")
CLIP = 1e-4


def _build(train_filter, seed=3, std=STD):
    from oracle import flux_ref as R
    from mi355_flow import flux
    from mi355_flow.scheduler import FlowMatchEulerDiscreteSDEScheduler
    cfg_o = R.tiny_config()
    mod = PF.build_module_tree(R.state_dict_shapes(cfg_o), buffers=(), seed=seed, std=std).cuda()
    with torch.no_grad():
        for prm in mod.parameters():
            prm.copy_(prm.bfloat16().float())
    for n, prm in mod.named_parameters():
        prm.requires_grad_(train_filter(n))
    sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, dynamics_type="Flow-SDE", shift=3.0)
    ad = flux.Flux1KontextNativeAdapter(mod, _engine_cfg(flux, cfg_o), sched, latent_storage_dtype="fp16")
    ad.rollout()
    return ad, mod, cfg_o


def _inputs(cfg_o, B, h, w, ch, cw, Nt, seed=0):
    from oracle import flux_ref as R
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    Ni = (h // 2) * (w // 2)
    return dict(x=R.pack_latents(mk(B, 16, h, w)).half(), x1=R.pack_latents(mk(B, 16, h, w)).half(),
                il=R.pack_latents(mk(B, 16, ch, cw)).bfloat16(), il2=R.pack_latents(mk(B, 16, ch, cw)).bfloat16(),
                pe=mk(B, Nt, cfg_o.joint_attention_dim).bfloat16(), pp=mk(B, cfg_o.pooled_projection_dim).bfloat16(), adv=mk(B), wnp=mk(B, Ni, 64),
                ids=torch.cat([R.prepare_img_ids(h // 2, w // 2), _cond_ids(ch // 2, cw // 2)]), Ni=Ni)


BLIND_BIASES = ("attn.to_v.bias", "proj_out.bias")        # of the single blocks: column sums of dY that cannot see the condition


def _ppo_kl_loss(log_prob, old, noise_pred, adv, wnp, kl_w):
    """PPO-clip on the replay log-prob (trainers/grpo.py: ratio = exp(lp - old), max of the unclipped and the clipped surrogate) + a KL-like
    term on the prediction; before any update ratio == 1 and the gradient is -adv * d log_prob."""
    ratio = torch.exp(log_prob - old)
    ppo = torch.maximum(-adv * ratio, -adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).sum()
    return ppo + kl_w * (wnp * noise_pred).mean()


def _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, sigma_max, kl_w, quant=None, with_condition=True):
    """The same loss through the fp32 oracle: the concatenated forward cut to the target rows + the Flow-SDE step in differentiable torch."""
    from oracle import flux_ref as R
    sd = {n: p_.detach().cpu().float().requires_grad_(p_.requires_grad) for n, p_ in mod.named_parameters()}
    x, x1 = inp["x"].float(), inp["x1"].float()
    B, Ni = x.shape[0], inp["Ni"]
    tm = R.model_scalar(torch.tensor(t) / 1000, torch.float16).reshape(-1).expand(B)
    gm = R.model_scalar(torch.full((B,), float(guidance)).half().float(), torch.float16)
    if with_condition:
        v = R.flux_forward(sd, cfg_o, torch.cat([x, inp["il"].float()], 1), tm, gm, inp["pp"].float(), inp["pe"].float(), inp["ids"], quant=quant,
                           premultiplied=True)[:, :Ni]
    else:
        v = R.flux_forward(sd, cfg_o, x, tm, gm, inp["pp"].float(), inp["pe"].float(), inp["ids"][:Ni], quant=quant, premultiplied=True)
    sigma, sigma_n = t / 1000.0, t_next / 1000.0
    dt = sigma_n - sigma
    std = math.sqrt(sigma / (1 - (sigma_max if sigma == 1.0 else sigma))) * eta
    mean = x * (1 + std ** 2 / (2 * sigma) * dt) + v * (1 + std ** 2 * (1 - sigma) / (2 * sigma)) * dt
    sv = std * math.sqrt(-dt)
    lp = (-((x1 - mean) ** 2) / (2 * sv ** 2) - math.log(sv) - math.log(math.sqrt(2 * math.pi))).mean(dim=(1, 2))
    _ppo_kl_loss(lp, lp.detach(), v, inp["adv"], inp["wnp"], kl_w).backward()
    return lp.detach(), {n: s.grad for n, s in sd.items() if s.requires_grad}


def _kw(inp, B, t, t_next, eta, guidance, il="il"):
    return dict(t=torch.full((B,), t), t_next=torch.full((B,), t_next), latents=inp["x"].cuda(), next_latents=inp["x1"].cuda(),
                image_latents=inp[il].cuda(), latent_ids=inp["ids"].cuda(), prompt_embeds=inp["pe"].cuda(), pooled_prompt_embeds=inp["pp"].cuda(),
                guidance_scale=guidance, noise_level=eta, compute_log_prob=True, return_kwargs=["log_prob", "noise_pred", "dt"])


def _pin_sigma_max(ad, smax):
    ad.scheduler.set_timesteps(4)
    ad.scheduler.sigmas = ad.scheduler.sigmas.clone()
    ad.scheduler.sigmas[1] = smax


@pytest.mark.parametrize("h,w,ch,cw,Nt,B,scope", [SHAPES[0] + ("blocks",), SHAPES[1] + ("default",)])
def test_kontext_replay_gradients_match_oracle_autograd_and_ratio_is_one(fx, h, w, ch, cw, Nt, B, scope):
    """Every trainable tensor against the oracle's autograd through the concatenated forward, with test_gpu_flux_backward.py's tolerances
    (rel < 3 x band + 5e-3, rel < 6e-2, cosine > 0.995) and its value-pinning tests' best-fit scale (within 5e-3 of 1; 1e-2 for tensors of
    fewer than 4 096 elements).  Sensitivity: the oracle's gradient WITHOUT the condition lies at least 3 x the tensor's tolerance away,
    asserted for every compared tensor (measured on the host: the minimum over the weight matrices is 0.17 against a tolerance of 0.039,
    4.5 x, on the last single block's `proj_mlp`; the median distance is 0.46) except the named `BLIND_BIASES`: the single blocks'
    `attn.to_v.bias` and `proj_out.bias`.  A weight gradient contracts dY with the layer's condition-dependent input; a bias gradient is
    the column sum of dY alone, and for these last layers that sum does not see the condition whatever the inputs: the loss's d v is a
    fixed weighting (advantages, KL weights) up to the small shift of the mean, and for `to_v` the sum over keys of dV equals the sum over
    queries of dO exactly, because softmax rows sum to one (measured 1.0 x to 2.7 x the tolerance, 0.02 to 0.07, for three seeds).  The
    exempt biases are compared to the oracle at the full tolerance like every tensor; their distance without the condition is printed."""
    filt = (lambda n: any(k in n for k in BLOCK_LINEARS)) if scope == "blocks" else (lambda n: any(k in n for k in DEFAULT_TARGETS))
    ad, mod, cfg_o = _build(filt)
    try:
        inp = _inputs(cfg_o, B, h, w, ch, cw, Nt, seed=5)
        t, t_next, eta, smax, guidance, kl_w = 900.0, 750.0, 0.7, 0.9, 3.5, 3.0
        _pin_sigma_max(ad, smax)
        kw = _kw(inp, B, t, t_next, eta, guidance)
        with torch.no_grad():
            ref_out = ad.forward(**kw)                      # the no-grad replay
        out = ad.forward(**kw)                              # grad mode: mi355_flux_forward_train_cond + the same scheduler-step kernel
        assert out.log_prob.requires_grad and out.noise_pred.requires_grad
        assert torch.equal(out.noise_pred.detach(), ref_out.noise_pred)
        assert torch.equal(out.log_prob.detach(), ref_out.log_prob)          # ratio == exp(0) == 1.0 EXACTLY in grad mode
        _ppo_kl_loss(out.log_prob, ref_out.log_prob, out.noise_pred, inp["adv"].cuda(), inp["wnp"].cuda(), kl_w).backward()
        lp_ref, g_ref = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, kl_w)
        _, g_band = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, kl_w, quant=lambda z: z.to(torch.bfloat16).float())
        _, g_none = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, kl_w, with_condition=False)
        np.testing.assert_allclose(out.log_prob.detach().cpu().numpy(), lp_ref.numpy(), rtol=5e-3)
        worst, worst_name, worst_band, worst_alpha, least_sens, least_blind, n = 0.0, None, 0.0, 0.0, float("inf"), float("inf"), 0
        for name, prm in mod.named_parameters():
            if not prm.requires_grad:
                assert prm.grad is None, name
                continue
            assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
            ref = g_ref[name]
            if float(ref.norm()) < 1e-12:
                assert float(prm.grad.float().norm()) < 1e-6, name
                continue
            r, band, c = _rel(prm.grad, ref), _rel(g_band[name], ref), _cos(prm.grad, ref)
            tol = min(3.0 * band + 5e-3, 6e-2)
            ge, gr = prm.grad.float().cpu().flatten().double(), ref.flatten().double()
            alpha = float((ge @ gr) / (gr @ gr))
            sens = _rel(g_none[name], ref)
            n, worst_band, worst_alpha = n + 1, max(worst_band, band), max(worst_alpha, abs(alpha - 1))
            if r > worst:
                worst, worst_name = r, name
            assert r < 3.0 * band + 5e-3 and r < 6e-2 and c > 0.995, (name, r, band, c)
            assert abs(alpha - 1) < (5e-3 if gr.numel() >= 4096 else 1e-2), (name, alpha, r, band)
            if name.startswith("single_transformer_blocks.") and name.endswith(BLIND_BIASES):
                least_blind = min(least_blind, sens / tol)
            else:
                least_sens = min(least_sens, sens / tol)
                assert sens >= 3 * tol, (name, sens, tol)
        print(f"Kontext replay ({scope}, {h}x{w} / {ch}x{cw}, Nt {Nt}, B {B}): {n} parameter gradients vs fp32 oracle autograd, worst rel-L2 {worst:.3e} "
              f"({worst_name}); bf16-emulating oracle band, worst {worst_band:.3e}; best-fit scale within {worst_alpha:.2e} of 1; without the condition "
              f"the oracle's gradients move by at least {least_sens:.1f} x the tolerance (the exempt single-block to_v / proj_out biases: {least_blind:.1f} x)")
        assert n >= (56 if scope == "blocks" else 40), n
    finally:
        ad.engine.close()


def test_kontext_two_grad_forwards_then_their_backwards(fx):
    """Two grad-mode forwards with DIFFERENT conditions on one plan before either backward (a loss that sums several forwards, as the
    reference's trainers can): the plan owns one stash, so each backward re-runs its own forward -- with its own condition, which rides in the
    call record -- and gives the gradients of the same step run alone, bit for bit."""
    ad, mod, cfg_o = _build(lambda n: any(k in n for k in DEFAULT_TARGETS), seed=9)
    try:
        h, w, ch, cw, Nt, B = SHAPES[0]
        inp = _inputs(cfg_o, B, h, w, ch, cw, Nt, seed=6)
        _pin_sigma_max(ad, 0.9)
        adv, wnp = inp["adv"].cuda(), inp["wnp"].cuda()
        params = {n: p for n, p in mod.named_parameters() if p.requires_grad}

        def loss_of(il):
            out = ad.forward(**_kw(inp, B, 900.0, 750.0, 0.7, 3.5, il=il))
            return _ppo_kl_loss(out.log_prob, out.log_prob.detach(), out.noise_pred, adv, wnp, 3.0)

        def grads_and_clear():
            g = {n: p.grad.clone() for n, p in params.items()}
            for p in params.values():
                p.grad = None
            return g

        alone = {}
        for il in ("il", "il2"):
            loss_of(il).backward()
            alone[il] = grads_and_clear()
        assert any(not torch.equal(alone["il"][n], alone["il2"][n]) for n in params)          # the two conditions give different gradients
        plan = ad.engine.plan(B, h, w, Nt, 1, cond=(ch, cw))
        before = getattr(plan, "recomputed_forwards", 0)
        la, lb = loss_of("il"), loss_of("il2")
        la.backward()
        got_a = grads_and_clear()
        lb.backward()
        got_b = grads_and_clear()
        for n in params:
            assert torch.equal(got_a[n], alone["il"][n]), n
            assert torch.equal(got_b[n], alone["il2"][n]), n
        # the first backward finds the second forward's stash, the second backward finds the first's re-run
        assert plan.recomputed_forwards - before == 2
        # ... and summed before one backward, as a trainer would
        (loss_of("il") + loss_of("il2")).backward()
        for n, p in params.items():
            assert torch.equal(p.grad, alone["il"][n] + alone["il2"][n]), n
    finally:
        ad.engine.close()


# ------------------------------------------------------------------------------------------------- 8. schedules
@pytest.mark.parametrize("two_stream", [1, 0])
def test_kontext_schedules_are_race_free(fx, two_stream):
    """The recorded launch schedule (`mi355_sched_trace`) of a condition-plan forward and of `forward_train` + `backward`, text chain of the
    double blocks on the side stream and off: every pair of launches touching the same bytes is ordered (tests/_sched_check.py)."""
    import _sched_check as SC
    from mi355_flow import _lib
    from test_gpu_schedules import _assert_race_free, _trace_of
    lib = _lib.load()
    lib.mi355_tune_set(14, two_stream)
    lib.mi355_tune_set(26, 1)
    ad, mod, cfg_o = _build(lambda n: any(k in n for k in BLOCK_LINEARS), seed=31)
    try:
        h, w, ch, cw, Nt, B = 8, 8, 10, 4, 13, 2
        inp = _inputs(cfg_o, B, h, w, ch, cw, Nt, seed=9)
        ad.scheduler.set_timesteps(4)
        kw = _kw(inp, B, 750.0, 500.0, 0.7, 3.5)
        plan = ad.engine.plan(B, h, w, Nt, 1, cond=(ch, cw))
        tm, gm = torch.tensor([900.0, 412.5]), torch.full((B,), 3500.0)
        fwd = lambda: plan.transformer_forward(kw["latents"], tm, gm, kw["prompt_embeds"], kw["pooled_prompt_embeds"], image_latents=kw["image_latents"])
        fwd()
        text = _trace_of(lib, fwd)
        names = {o.name for o in SC.parse(text).ops}
        assert "concat_rows" in names, sorted(names)
        if two_stream:
            _assert_race_free(text, "Kontext forward, two streams")
        else:
            assert SC.parse(text).streams() == ["s0"] and SC.parse(text).races() == []
        adv, wnp = inp["adv"].cuda(), inp["wnp"].cuda()

        def step():
            for prm in mod.parameters():
                prm.grad = None
            out = ad.forward(**kw)
            ((adv * out.log_prob).sum() + (wnp * out.noise_pred).mean()).backward()

        step()
        text = _trace_of(lib, step)
        s = SC.parse(text)
        names = {o.name for o in s.ops}
        assert {"concat_rows", "attention128_bwd", "attn128_bwd_prep", "rope_rms_bwd128", "ln_mod_bwd", "gate_mul", "transpose", "gemm.f32"} <= names, sorted(names)
        assert len(s.streams()) == (3 if two_stream else 2), s.streams()          # caller's stream, (text chain,) weight gradients
        races = s.races()
        assert races == [], races[:5]
        nw = SC.n_waits(text)
        needed = [k for k in range(nw) if SC.parse(text, drop_waits=[k]).races(limit=1)]
        print(f"Kontext optimize() step, two_stream {two_stream}: {sum(1 for o in s.ops if o.regions)} launches on {len(s.streams())} streams, {nw} stream "
              f"waits, {len(needed)} of them individually necessary, no race")
        assert nw > 0 and len(needed) >= 0.5 * nw, (nw, len(needed))
    finally:
        lib.mi355_tune_set(14, 2)
        ad.engine.close()


# ------------------------------------------------------------------------------------------------- 9. errors
def test_kontext_errors_and_plain_plan_beside_a_condition_plan(fx):
    from oracle import flux_ref as R
    cfg_o = R.tiny_config()
    sd, cfg = _setup(fx, cfg_o)
    h, w, ch, cw, Nt, B = SHAPES[0]
    x, c, enc, pool, tm, gm = _forward_inputs(cfg_o, h, w, ch, cw, Nt, B, seed=1)
    args = (x.cuda(), tm, gm, enc.cuda(), pool.cuda())
    bound = {k: v.cuda() for k, v in sd.items()}
    alone = fx.FluxEngine(cfg)
    try:
        alone.bind_state_dict(bound)
        alone.ready()
        want = alone.plan(B, h, w, Nt, 1).transformer_forward(*args).clone()
    finally:
        alone.close()
    eng = fx.FluxEngine(cfg)
    try:
        eng.bind_state_dict(bound)
        eng.ready()
        for bad in ((7, 8), (8, 0), (8, 1)):
            with pytest.raises(RuntimeError, match="bad condition grid"):
                eng.plan(B, h, w, Nt, 1, cond=bad)
        cplan = eng.plan(B, h, w, Nt, 2, cond=(ch, cw))
        plain = eng.plan(B, h, w, Nt, 2)
        assert cplan is not plain and eng.plan(B, h, w, Nt, 1, cond=(ch, cw)) is cplan and eng.plan(B, h, w, Nt, 1, cond=(ch, cw + 2)) is not cplan
        with pytest.raises(RuntimeError, match="condition tokens per sample.*mi355_flux_forward_cond"):
            cplan.transformer_forward(*args)                                       # a plain call on a condition plan
        with pytest.raises(RuntimeError, match="condition tokens per sample.*mi355_flux_forward_train_cond"):
            cplan.forward_train(*args)
        with pytest.raises(RuntimeError, match="no condition grid"):
            plain.transformer_forward(*args, image_latents=c.cuda())               # a _cond call on a plain plan
        with pytest.raises(RuntimeError, match="no condition grid"):
            plain.forward_train(*args, image_latents=c.cuda())
        with pytest.raises(ValueError, match="image_latents must be"):
            cplan.transformer_forward(*args, image_latents=c[:, :-1].cuda())       # a wrong shape
        with pytest.raises(ValueError, match="image_latents must be"):
            cplan.transformer_forward(*args, image_latents=c[:1].cuda())
        sched = ([1000.0, 500.0], [1.0, 0.5, 0.0], [0.0, 0.0], "ODE", 3.5, x.cuda(), torch.float16, None, enc.cuda(), pool.cuda())
        with pytest.raises(RuntimeError, match="mi355_flux_rollout_cond"):
            cplan.rollout(*sched)
        with pytest.raises(RuntimeError, match="no condition grid"):
            plain.rollout(*sched, image_latents=c.cuda())
        # the refused calls launched nothing, and the condition plan beside it leaves the plain plan's results as they were
        got = plain.transformer_forward(*args).clone()
        cond_out = cplan.transformer_forward(*args, image_latents=c.cuda())
        assert torch.isfinite(cond_out.float()).all() and not torch.equal(cond_out, got)
        assert torch.equal(got, want) and torch.equal(plain.transformer_forward(*args), want)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- 10. full width
# The existing full-width FLUX tests' weight scale.  It did not have to be raised: on the host the fp32 oracle without the condition lies 0.145 from
# the oracle with it at this scale, 11.6 x the tolerance of 1.25e-2 (band 7.7e-3); the test prints and asserts the same figure on the GPU.
FULL_WIDTH_STD = 0.02


def test_kontext_full_width_blocks(fx):
    """FLUX.1-dev WIDTH (D = 3072, 24 heads x 128, T5 width 4096), one double + one single block, target 32x32, condition 32x48, Nt 512,
    B = 1 (S = 1152): the large-grid kernels on Nx = 640 image rows, against the fp32 oracle on the GPU within 1.5 x band + 1e-3."""
    from oracle import flux_ref as R
    from _gpu_oracle import check_in_band, ref_on_gpu, rel
    cfg_o = R.FluxConfig(num_layers=1, num_single_layers=1)
    sd = {k: _bf(v) for k, v in R.make_synthetic_state_dict(cfg_o, seed=11, std=FULL_WIDTH_STD).items()}
    eng = fx.FluxEngine(fx.FluxConfig(num_layers=1, num_single_layers=1))
    try:
        eng.bind_state_dict({k: v.cuda() for k, v in sd.items()})
        eng.ready()
        B, h, w, ch, cw, Nt = 1, 32, 32, 32, 48, 512
        x, c, enc, pool, _, gm = _forward_inputs(cfg_o, h, w, ch, cw, Nt, B, seed=17)
        tm = torch.tensor([640.0])
        ids, cids = R.prepare_img_ids(h // 2, w // 2), _cond_ids(ch // 2, cw // 2)
        got = eng.plan(B, h, w, Nt, 1, cond=(ch, cw)).transformer_forward(x.cuda(), tm, gm, enc.cuda(), pool.cuda(), image_latents=c.cuda())
        ref, _, r, band = check_in_band(f"Kontext full-width 1 + 1 blocks, S = 1152, weight std {FULL_WIDTH_STD}", got, _kontext_forward, sd, cfg_o,
                                        x.float(), c.float(), tm, gm, pool, enc, ids, cids)
        tol = 1.5 * band + 1e-3
        no_cond = rel(ref_on_gpu(R.flux_forward, sd, cfg_o, x.float(), tm, gm, pool, enc, ids, premultiplied=True), ref)
        print(f"  without the condition the oracle moves by {no_cond:.3e} = {no_cond / tol:.1f} x the tolerance {tol:.3e}")
        assert no_cond >= 3 * tol, (no_cond, tol)
    finally:
        eng.close()

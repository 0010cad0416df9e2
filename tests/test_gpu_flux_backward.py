"""GPU tests of the native FLUX.1 backward (SURVEY.md 8(f) N1 over N3; reference src/flow_factory/trainers/grpo.py:263, :326-330 over
models/flux/flux1.py:294-346), through the C ABI (`mi355_flux_forward_train` / `mi355_flux_backward` / `mi355_sde_step_bwd`,
`mi355_op_attention128_fwd_bwd`, `mi355_op_rope_norm_fwd_bwd`):

  * head_dim-128 flash-attention backward vs torch autograd of fp32 SDPA on the same bf16 inputs, on BOTH forward kernels (the 8-wave
    running-max kernel and the hand-scheduled static kernel: each writes the log-sum-exp the backward consumes);
  * backward of the q | k producer (per-head RMSNorm + RoPE) vs autograd of the oracle's own functions;
  * the train / inference consistency invariant IN GRAD MODE: velocity and replay log-prob of `forward()` with autograd enabled are
    bit-identical to the no-grad replay and to the rollout's (ratio == exp(0) == 1 exactly);
  * weight gradients of a PPO-style loss (log-prob term + a KL-like noise_pred term) vs torch autograd through the fp32 oracle
    (oracle/flux_ref.py, differentiable) on identical bf16-rounded weights, with the band a bf16-emulating oracle sets;
  * an optimizer step changes the replay log-prob (weights are live) and the next backward still works.
"""
import math

import numpy as np
import pytest
import torch

import _plugin_fakes as PF

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


def _cos(a, b):
    a, b = a.detach().float().cpu().flatten(), b.detach().float().cpu().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------- attention backward, head_dim 128
@pytest.mark.parametrize("static", [0, 1])
@pytest.mark.parametrize("B,H,S", [(1, 2, 64), (1, 1, 100), (1, 2, 192), (2, 1, 256), (1, 1, 449), (2, 3, 333 + 256), (1, 2, 1000), (1, 2, 4608)])
def test_attention128_backward_matches_autograd(gpu, B, H, S, static):
    from mi355_flow import _lib
    from mi355_flow.engine import _ptr, _stream
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(S * 7 + H)
    S_pad = (S + 63) // 64 * 64
    c = 1.4426950408889634 / math.sqrt(128.0)
    q = torch.zeros(B, H, S_pad, 128, device="cuda", dtype=torch.bfloat16)
    k, v = torch.zeros_like(q), torch.zeros_like(q)
    q[:, :, :S] = (torch.randn(B, H, S, 128, device="cuda", generator=g) * c).bfloat16()          # stored q carries log2(e)/sqrt(128)
    k[:, :, :S] = (torch.randn(B, H, S, 128, device="cuda", generator=g) * 1.2).bfloat16()
    v[:, :, :S] = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    vT = v.transpose(2, 3).contiguous()
    do = torch.randn(B * S, H * 128, device="cuda", generator=g).bfloat16()
    o = torch.empty_like(do)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    # 60: the proven-bound (static softmax) hand-scheduled kernel; 0: the running-max kernel.  |score| here is ~ 1.2 * 11.3 * 4 sigma << 60
    _lib.check(lib.mi355_tune_set(21, 60 if static else 0))
    try:
        _lib.check(lib.mi355_op_attention128_fwd_bwd(_stream(), _ptr(q), _ptr(k), _ptr(vT), _ptr(do), _ptr(o), _ptr(dq), _ptr(dk), _ptr(dv),
                                                     B, H, S, S_pad), "op_attention128_fwd_bwd")
        # round 6: the shipped passes are the software-pipelined ones (csrc/gen_attn_bwd.py 128; 1 .. 72 tiles here: prologue-only, every ring-slot
        # wrap, ragged tails).  Same MFMAs / masks in the same order per output element as the round-4 kernels (mi355_tune_set(44, 0)): same bits.
        _lib.check(lib.mi355_tune_set(44, 0))
        dq0, dk0, dv0 = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
        _lib.check(lib.mi355_op_attention128_fwd_bwd(_stream(), _ptr(q), _ptr(k), _ptr(vT), _ptr(do), _ptr(o), _ptr(dq0), _ptr(dk0), _ptr(dv0),
                                                     B, H, S, S_pad), "op_attention128_fwd_bwd")
        _lib.check(lib.mi355_tune_set(44, 1))
        for name, a, b in (("dq", dq, dq0), ("dk", dk, dk0), ("dv", dv, dv0)):
            assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
        dq1, dk1, dv1 = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
        _lib.check(lib.mi355_op_attention128_fwd_bwd(_stream(), _ptr(q), _ptr(k), _ptr(vT), _ptr(do), _ptr(o), _ptr(dq1), _ptr(dk1), _ptr(dv1),
                                                     B, H, S, S_pad), "op_attention128_fwd_bwd")
        assert torch.equal(dq1, dq) and torch.equal(dk1, dk) and torch.equal(dv1, dv)       # run to run
    finally:
        lib.mi355_tune_set(21, 0)
        lib.mi355_tune_set(44, 1)
    qr = q[:, :, :S].float().requires_grad_(True)
    kr = k[:, :, :S].float().requires_grad_(True)
    vr = v[:, :, :S].float().requires_grad_(True)
    p = torch.softmax((qr @ kr.transpose(2, 3)) * math.log(2.0), dim=-1)
    oref = (p @ vr).transpose(1, 2).reshape(B * S, H * 128)
    oref.backward(do.float())
    assert _rel(o, oref) < 6e-3
    for name, got, ref in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        r = _rel(got[:, :, :S], ref)
        assert r < 2e-2 and _cos(got[:, :, :S], ref) > 0.9995, (name, r, static)
        if S_pad > S:
            assert float(got[:, :, S:].float().abs().max()) == 0.0          # padded rows are never written


def test_rope_norm_backward_matches_autograd(gpu):
    """d[q | k | v]_pre from (dq~, dk, dv): the stored q~ carries RMSNorm weight, rotation and the folded softmax scale."""
    from oracle import flux_ref as R
    from mi355_flow import _lib
    from mi355_flow.engine import _ptr, _stream
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    B, H, Nt, hp, wp = 2, 3, 5, 3, 4
    Ni, D = hp * wp, 3 * 128
    S, S_pad, qs = Nt + Ni, 64, 0.1275
    ids = torch.cat([torch.zeros(Nt, 3), R.prepare_img_ids(hp, wp)], 0)
    cos, sin = R.rope_cos_sin(ids)
    cs = torch.stack([cos[:, 0::2], sin[:, 0::2]], dim=-1).contiguous()       # [S, 64, 2]
    src = torch.randn(B * Ni, 2 * D, generator=g).bfloat16()
    wq, wk = 1 + 0.1 * torch.randn(128, generator=g), 1 + 0.1 * torch.randn(128, generator=g)
    dq = torch.zeros(B, H, S_pad, 128).bfloat16()
    dk, dv = torch.zeros_like(dq), torch.zeros_like(dq)
    dq[:, :, Nt:S] = torch.randn(B, H, Ni, 128, generator=g).bfloat16()
    dk[:, :, Nt:S] = torch.randn(B, H, Ni, 128, generator=g).bfloat16()
    dv[:, :, Nt:S] = torch.randn(B, H, Ni, 128, generator=g).bfloat16()
    dev = lambda t: t.cuda()
    q_out = torch.zeros(B, H, S_pad, 128, device="cuda", dtype=torch.bfloat16)
    k_out = torch.zeros_like(q_out)
    rstd = torch.zeros(B * Ni, 2 * H, device="cuda")
    out = torch.zeros(B * Ni, 3 * D, device="cuda", dtype=torch.bfloat16)
    a = [dev(src), dev(wq), dev(wk), dev(cs), dev(dq), dev(dk), dev(dv)]
    _lib.check(lib.mi355_op_rope_norm_fwd_bwd(_stream(), _ptr(a[0]), 2 * D, 0, D, _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), _ptr(q_out), _ptr(k_out), _ptr(rstd),
                                              _ptr(a[4]), _ptr(a[5]), _ptr(a[6]), _ptr(out), B * Ni, H, Ni, Nt, S_pad, 1e-6, qs), "op_rope_norm_fwd_bwd")
    x = src.float().requires_grad_(True)
    xv = x.view(B, Ni, 2, H, 128).permute(2, 0, 3, 1, 4)                       # (2, B, H, Ni, 128)
    rq = R.apply_rope(R._rms(xv[0], wq, 1e-6), cos[Nt:], sin[Nt:]) * qs
    rk = R.apply_rope(R._rms(xv[1], wk, 1e-6), cos[Nt:], sin[Nt:])
    ((rq * dq[:, :, Nt:S].float()).sum() + (rk * dk[:, :, Nt:S].float()).sum()).backward()
    # forward side outputs: the 1/rms the backward consumes
    r_ref = torch.rsqrt(src.float().view(B * Ni, 2, H, 128).pow(2).mean(-1) + 1e-6).reshape(B * Ni, 2 * H)
    assert torch.allclose(rstd.cpu(), r_ref, rtol=1e-4, atol=0)
    got = out.float().cpu()
    assert _rel(got[:, :2 * D], x.grad) < 1.5e-2, _rel(got[:, :2 * D], x.grad)        # the stored q~ / k are bf16: xhat is recovered to 2^-9
    dv_tok = dv[:, :, Nt:S].permute(0, 2, 1, 3).reshape(B * Ni, D)
    assert torch.equal(got[:, 2 * D:], dv_tok.float())


# ------------------------------------------------------------------------------------------------- model-level gradients
BLOCK_LINEARS = (".attn.to_q.", ".attn.to_k.", ".attn.to_v.", ".attn.to_out.0.", ".attn.add_q_proj.", ".attn.add_k_proj.", ".attn.add_v_proj.",
                 ".attn.to_add_out.", ".ff.net.0.proj.", ".ff.net.2.", ".ff_context.net.0.proj.", ".ff_context.net.2.", ".proj_mlp.", ".proj_out.")
# the reference's FLUX.1 default target modules (models/flux/flux1.py:76-84)
DEFAULT_TARGETS = ("attn.to_k.", "attn.to_q.", "attn.to_v.", "attn.to_out.0.", "attn.add_k_proj.", "attn.add_q_proj.", "attn.add_v_proj.",
                   "attn.to_add_out.", "ff.net.0.proj.", "ff.net.2.", "ff_context.net.0.proj.", "ff_context.net.2.")


def _build(train_filter, seed=3, std=0.05, guidance_embeds=True, cfg_o=None):
    from oracle import flux_ref as R
    from mi355_flow import flux
    from mi355_flow.scheduler import FlowMatchEulerDiscreteSDEScheduler
    cfg_o = cfg_o or R.tiny_config()
    cfg_o.guidance_embeds = guidance_embeds
    mod = PF.build_module_tree(R.state_dict_shapes(cfg_o), buffers=(), seed=seed, std=std).cuda()
    with torch.no_grad():
        for prm in mod.parameters():
            prm.copy_(prm.bfloat16().float())
    for n, prm in mod.named_parameters():
        prm.requires_grad_(train_filter(n))
    cfg = flux.FluxConfig(num_layers=cfg_o.num_layers, num_single_layers=cfg_o.num_single_layers, num_attention_heads=cfg_o.num_attention_heads,
                          joint_attention_dim=cfg_o.joint_attention_dim, pooled_projection_dim=cfg_o.pooled_projection_dim,
                          guidance_embeds=cfg_o.guidance_embeds)
    sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, dynamics_type="Flow-SDE", shift=3.0)
    ad = flux.Flux1NativeAdapter(mod, cfg, sched, latent_storage_dtype="fp16")
    ad.rollout()
    return ad, mod, cfg_o


def _inputs(cfg_o, B, h, w, Nt, seed=0):
    from oracle import flux_ref as R
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    Ni = (h // 2) * (w // 2)
    return dict(x=R.pack_latents(mk(B, 16, h, w)).half(), x1=R.pack_latents(mk(B, 16, h, w)).half(),
                pe=mk(B, Nt, cfg_o.joint_attention_dim).bfloat16(), pp=mk(B, cfg_o.pooled_projection_dim).bfloat16(), wlp=mk(B), wnp=mk(B, Ni, 64),
                img_ids=R.prepare_img_ids(h // 2, w // 2))


def _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, sigma_max, kl_w, quant=None, device="cpu"):
    """`device="cuda"`: the same plain-PyTorch fp32 oracle autograd on GPU tensors (tests/_gpu_oracle.py) -- the full-width cases."""
    from _gpu_oracle import oracle_loss_on
    return oracle_loss_on(device, _oracle_loss_impl, mod, cfg_o, inp, guidance, t, t_next, eta, sigma_max, kl_w, quant=quant)


def _oracle_loss_impl(mod, cfg_o, inp, guidance, t, t_next, eta, sigma_max, kl_w, quant=None):
    """The same loss through the fp32 oracle network + the Flow-SDE step written in differentiable torch (CPU)."""
    from oracle import flux_ref as R
    sd = {n: p_.detach().to(inp["x"].device).float().requires_grad_(p_.requires_grad) for n, p_ in mod.named_parameters()}
    x, x1 = inp["x"].float(), inp["x1"].float()
    B = x.shape[0]
    tm = R.model_scalar(torch.tensor(t) / 1000, torch.float16).reshape(-1).expand(B)
    gm = R.model_scalar(torch.full((B,), float(guidance)).half().float(), torch.float16)
    v = R.flux_forward(sd, cfg_o, x, tm, gm, inp["pp"].float(), inp["pe"].float(), inp["img_ids"], quant=quant, premultiplied=True)
    sigma, sigma_n = t / 1000.0, t_next / 1000.0
    dt = sigma_n - sigma
    std = math.sqrt(sigma / (1 - (sigma_max if sigma == 1.0 else sigma))) * eta
    mean = x * (1 + std ** 2 / (2 * sigma) * dt) + v * (1 + std ** 2 * (1 - sigma) / (2 * sigma)) * dt
    sv = std * math.sqrt(-dt)
    if sv > 0:
        lp = (-((x1 - mean) ** 2) / (2 * sv ** 2) - math.log(sv) - math.log(math.sqrt(2 * math.pi))).mean(dim=(1, 2))
    else:
        lp = torch.zeros(B)
    loss = (inp["wlp"] * lp).sum() + kl_w * (inp["wnp"] * v).mean()
    loss.backward()
    return lp.detach(), {n: s.grad for n, s in sd.items() if s.requires_grad}


@pytest.mark.parametrize("h,w,Nt,B,scope", [(8, 8, 16, 2, "blocks"), (6, 10, 13, 1, "default")])
def test_flux_replay_gradients_match_oracle_autograd_and_ratio_is_one(gpu, h, w, Nt, B, scope):
    from oracle import flux_ref as R
    filt = (lambda n: any(k in n for k in BLOCK_LINEARS)) if scope == "blocks" else (lambda n: any(k in n for k in DEFAULT_TARGETS))
    ad, mod, cfg_o = _build(filt)
    inp = _inputs(cfg_o, B, h, w, Nt, seed=5)
    t, t_next, eta, smax, guidance = 900.0, 750.0, 0.7, 0.9, 3.5
    ad.scheduler.set_timesteps(4)
    ad.scheduler.sigmas = ad.scheduler.sigmas.clone()
    ad.scheduler.sigmas[1] = smax
    kw = dict(t=torch.full((B,), t), t_next=torch.full((B,), t_next), latents=inp["x"].cuda(), next_latents=inp["x1"].cuda(),
              prompt_embeds=inp["pe"].cuda(), pooled_prompt_embeds=inp["pp"].cuda(), img_ids=inp["img_ids"].cuda(), guidance_scale=guidance,
              noise_level=eta, compute_log_prob=True, return_kwargs=["log_prob", "noise_pred", "dt"])
    with torch.no_grad():
        ref_out = ad.forward(**kw)                      # the no-grad replay
    out = ad.forward(**kw)                              # grad mode: mi355_flux_forward_train + the same scheduler-step kernel
    assert out.log_prob.requires_grad and out.noise_pred.requires_grad
    assert torch.equal(out.noise_pred.detach(), ref_out.noise_pred)      # the velocity: same kernel binaries on per-block buffers
    assert torch.equal(out.log_prob.detach(), ref_out.log_prob)          # ratio == exp(0) == 1.0 EXACTLY in grad mode
    kl_w = 3.0
    loss = (inp["wlp"].cuda() * out.log_prob).sum() + kl_w * (inp["wnp"].cuda() * out.noise_pred).mean()
    loss.backward()
    lp_ref, g_ref = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, kl_w)
    _, g_band = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, kl_w, quant=lambda z: z.to(torch.bfloat16).float())
    np.testing.assert_allclose(out.log_prob.detach().cpu().numpy(), lp_ref.numpy(), rtol=5e-3)
    worst, worst_name, worst_band, n = 0.0, None, 0.0, 0
    for name, prm in mod.named_parameters():
        if not prm.requires_grad:
            assert prm.grad is None, name
            continue
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
        ref = g_ref[name]
        if float(ref.norm()) < 1e-12:
            assert float(prm.grad.float().norm()) < 1e-6, name
            continue
        r, band = _rel(prm.grad, ref), _rel(g_band[name], ref)
        n += 1
        worst_band = max(worst_band, band)
        if r > worst:
            worst, worst_name = r, name
        assert r < 3.0 * band + 5e-3 and r < 6e-2 and _cos(prm.grad, ref) > 0.995, (name, r, band, _cos(prm.grad, ref))
    print(f"FLUX.1 replay ({scope}, {h}x{w}, Nt {Nt}, B {B}): {n} parameter gradients vs fp32 oracle autograd, worst rel-L2 {worst:.3e} ({worst_name}); "
          f"bf16-emulating oracle band, worst {worst_band:.3e}")
    assert n >= (56 if scope == "blocks" else 40), n
    ad.engine.close()


def test_flux_one_double_one_single_block_gradient_values_and_real_transition_log_prob(gpu):
    """VALUE, not direction (`test_gpu_wan_backward._compare_value`): one double + one single block, 2 048 image tokens over
    the batch, every non-null gradient tensor's best-fit scale on the fp32 oracle's autograd within 5e-3 of 1 and its noise within 1.5 x the
    bf16-emulating oracle's own; the replay log-prob of a REAL stored transition (x' from the engine's own rollout step) at rtol 1e-3."""
    from oracle import flux_ref as R
    from test_gpu_wan_backward import _compare_value
    ad, mod, cfg_o = _build(lambda n: any(k in n for k in BLOCK_LINEARS), seed=41, cfg_o=R.tiny_config(num_layers=1, num_single_layers=1))
    try:
        h, w, Nt, B = 64, 64, 24, 2
        inp = _inputs(cfg_o, B, h, w, Nt, seed=43)
        t, t_next, eta, smax, guidance = 900.0, 750.0, 0.7, 0.9, 3.5
        ad.scheduler.set_timesteps(4)
        ad.scheduler.sigmas = ad.scheduler.sigmas.clone()
        ad.scheduler.sigmas[1] = smax
        kw = dict(t=torch.full((B,), t), t_next=torch.full((B,), t_next), latents=inp["x"].cuda(), prompt_embeds=inp["pe"].cuda(),
                  pooled_prompt_embeds=inp["pp"].cuda(), img_ids=inp["img_ids"].cuda(), guidance_scale=guidance, noise_level=eta, compute_log_prob=True)
        torch.cuda.manual_seed(5)
        with torch.no_grad():
            o0 = ad.forward(**kw, return_kwargs=["next_latents", "log_prob"])           # the rollout step: draws the noise, stores x'
        inp["x1"] = o0.next_latents.half().cpu()
        out = ad.forward(**kw, next_latents=inp["x1"].cuda(), return_kwargs=["log_prob", "dt"])
        assert torch.equal(out.log_prob.detach(), o0.log_prob)
        inp["wlp"] = torch.ones(B)
        out.log_prob.sum().backward()
        lp_ref, g_ref = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, 0.0)
        _, g_band = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, 0.0, quant=lambda z: z.to(torch.bfloat16).float())
        np.testing.assert_allclose(out.log_prob.detach().cpu().numpy(), lp_ref.numpy(), rtol=1e-3)
        print(f"FLUX.1 one double + one single block, real transition: log-prob engine {out.log_prob.tolist()} vs oracle {lp_ref.tolist()}")
        g_ref = {k: v for k, v in g_ref.items() if v is not None}
        for n_, p_ in mod.named_parameters():
            if p_.requires_grad and n_ not in g_ref:
                assert p_.grad is None or float(p_.grad.float().norm()) == 0.0, n_
                p_.requires_grad_(False)
        _compare_value(mod, g_ref, g_band, "FLUX.1 one double + one single block (2 048 image tokens, real transition)")
    finally:
        ad.engine.close()


def test_flux_full_width_block_gradients_at_1024_token_count(gpu):
    """BASELINE.json configs[2]'s own width and token count: FLUX.1-dev WIDTH (D = 3072, 24 heads x 128), one double-stream + one single-stream
    block at 1024^2 (4096 image + 512 text = 4608 joint tokens), B = 1 -- the large-grid kernels (persistent GEMMs incl. the K = 7D = 21 504
    fused dgrad and the K = 15 360 proj_out, the hand-scheduled attention with its log-sum-exp, 72 query / key tiles in the backward passes,
    split-K weight gradients) -- the reference's default target modules, vs the oracle's autograd (fp32, on the GPU: tests/_gpu_oracle.py) and its bf16 band."""
    from oracle import flux_ref as R
    from mi355_flow import flux
    from mi355_flow.scheduler import FlowMatchEulerDiscreteSDEScheduler
    cfg_o = R.FluxConfig(num_layers=1, num_single_layers=1)
    mod = PF.build_module_tree(R.state_dict_shapes(cfg_o), buffers=(), seed=11, std=0.02).cuda()
    with torch.no_grad():
        for prm in mod.parameters():
            prm.copy_(prm.bfloat16().float())
    for n, prm in mod.named_parameters():
        prm.requires_grad_(any(k in n for k in DEFAULT_TARGETS))
    sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, dynamics_type="Flow-SDE", shift=3.0)
    ad = flux.Flux1NativeAdapter(mod, flux.FluxConfig(num_layers=1, num_single_layers=1), sched, latent_storage_dtype="fp16")
    ad.rollout()
    try:
        B, h, w, Nt = 1, 128, 128, 512
        inp = _inputs(cfg_o, B, h, w, Nt, seed=17)
        t, t_next, eta, smax, guidance = 900.0, 750.0, 0.7, 0.9, 3.5
        ad.scheduler.set_timesteps(4)
        ad.scheduler.sigmas = ad.scheduler.sigmas.clone()
        ad.scheduler.sigmas[1] = smax
        kw = dict(t=torch.full((B,), t), t_next=torch.full((B,), t_next), latents=inp["x"].cuda(), next_latents=inp["x1"].cuda(),
                  prompt_embeds=inp["pe"].cuda(), pooled_prompt_embeds=inp["pp"].cuda(), img_ids=inp["img_ids"].cuda(), guidance_scale=guidance,
                  noise_level=eta, compute_log_prob=True, return_kwargs=["log_prob", "noise_pred", "dt"])
        with torch.no_grad():
            ref_out = ad.forward(**kw)
        out = ad.forward(**kw)
        assert torch.equal(out.noise_pred.detach(), ref_out.noise_pred) and torch.equal(out.log_prob.detach(), ref_out.log_prob)
        kl_w = 3.0
        ((inp["wlp"].cuda() * out.log_prob).sum() + kl_w * (inp["wnp"].cuda() * out.noise_pred).mean()).backward()
        _, g_ref = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, kl_w, device="cuda")
        _, g_band = _oracle_loss(mod, cfg_o, inp, guidance, t, t_next, eta, smax, kl_w, quant=lambda z: z.to(torch.bfloat16).float(), device="cuda")
        worst, worst_name, worst_band, n = 0.0, None, 0.0, 0
        for name, prm in mod.named_parameters():
            if not prm.requires_grad:
                continue
            ref = g_ref[name]
            r, band = _rel(prm.grad, ref), _rel(g_band[name], ref)
            n, worst_band = n + 1, max(worst_band, band)
            if r > worst:
                worst, worst_name = r, name
            assert r < 3.0 * band + 5e-3 and _cos(prm.grad, ref) > 0.995, (name, r, band)
        print(f"FLUX.1 full-width 1 + 1 blocks at S = 4608: {n} parameter gradients vs fp32 oracle autograd, worst rel-L2 {worst:.3e} ({worst_name}); "
              f"bf16-emulating oracle band, worst {worst_band:.3e}; stash + scratch {ad.engine.plan(B, h, w, Nt, 1).training_bytes / 2 ** 30:.2f} GiB")
        assert n == 24 + 6
    finally:
        ad.engine.close()


def test_flux_optimizer_step_moves_the_policy_and_the_next_backward_works(gpu):
    ad, mod, cfg_o = _build(lambda n: any(k in n for k in DEFAULT_TARGETS), seed=9)
    B, h, w, Nt = 2, 8, 8, 16
    inp = _inputs(cfg_o, B, h, w, Nt, seed=6)
    ad.scheduler.set_timesteps(4)
    kw = dict(t=torch.full((B,), 900.0), t_next=torch.full((B,), 750.0), latents=inp["x"].cuda(), prompt_embeds=inp["pe"].cuda(),
              pooled_prompt_embeds=inp["pp"].cuda(), img_ids=inp["img_ids"].cuda(), guidance_scale=3.5, noise_level=0.7)
    torch.cuda.manual_seed(3)
    with torch.no_grad():
        o0 = ad.forward(**kw, return_kwargs=["next_latents", "log_prob"])          # a rollout step: samples x' and its log-prob
    kw2 = dict(kw, next_latents=o0.next_latents.half(), compute_log_prob=True, return_kwargs=["log_prob", "dt"])
    params = [p for p in mod.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=2e-3)
    adv = torch.tensor([1.0, -1.0]).cuda()
    ratios = []
    for it in range(2):
        out = ad.forward(**kw2)
        ratio = torch.exp(out.log_prob - o0.log_prob)
        ratios.append(ratio.detach().clone())
        loss = torch.mean(torch.maximum(-adv * ratio, -adv * torch.clamp(ratio, 1 - 1e-4, 1 + 1e-4)))
        loss.backward()
        gn = torch.nn.utils.clip_grad_norm_(params, 1.0)
        assert torch.isfinite(gn) and (float(gn) > 0 or it > 0)
        opt.step()
        opt.zero_grad()
    assert torch.equal(ratios[0], torch.ones_like(ratios[0])), ratios[0]            # before ANY update: exactly 1
    assert float((ratios[1] - 1).abs().max()) > 1e-7                                # the update moved the policy (weights are live)
    # the matching-loss trainers' call: autograd, no stored transition, noise_pred only
    out = ad.forward(**dict(kw, t_next=torch.zeros(B), noise_level=0.0, compute_log_prob=False, return_kwargs=["noise_pred"]))
    assert out.noise_pred.requires_grad
    out.noise_pred.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    # parameters outside the native scope are refused by name, standalone (the plugin routes them to the reference path)
    for n, p in mod.named_parameters():
        p.requires_grad_("norm1.linear" in n)
    with pytest.raises(NotImplementedError, match="outside the native backward"):
        ad.forward(**kw2)
    ad.engine.close()

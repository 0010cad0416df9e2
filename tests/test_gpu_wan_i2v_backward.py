"""GPU parity of the native backward on a Wan image-to-video engine (condition channels and the image cross-attention branch;
mi355_wan_forward_train_i2v + mi355_wan_backward) against
torch autograd through the CPU oracle fed the concatenated input (tests/_wan_i2v_ref.py).  Helpers and tolerances are
tests/test_gpu_wan_backward.py's own (`_compare`: rel-L2 < 3 x band + 5e-3, cosine > 0.99; `_compare_value`)."""
import math
import os

import numpy as np
import pytest
import torch

import _plugin_fakes as PF
import _wan_i2v_ref as I
from test_gpu_wan_backward import DEFAULT_TARGETS, _compare, _compare_value, _kw

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("MI355_WAN_NATIVE_BACKWARD") == "0", reason="MI355_WAN_NATIVE_BACKWARD=0 opts out")]


@pytest.fixture(scope="module")
def wn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import wan
    assert wan.WanEngine.native_backward_enabled
    return wan


DI = 128          # image_dim of the tiny configuration


def _build(wn, cfg_o, train_filter, seed=3, std=0.05, image_dim=0):
    """tests/test_gpu_wan_backward._build on the 36-channel transformer (with the image branch's parameters when `image_dim`) and the I2V adapter."""
    from oracle import wan_ref as R
    mod = PF.build_module_tree(I.shapes(R, cfg_o, image_dim), buffers=(), seed=seed, std=std).cuda()
    with torch.no_grad():
        for n, prm in mod.named_parameters():
            if ".norm_q." in n or ".norm_k." in n or "norm_added_k" in n or n.endswith(("norm2.weight", "norm1.weight")):
                prm.copy_(1.0 + 0.1 * prm / std)
            prm.copy_(prm.bfloat16().float())
    for n, prm in mod.named_parameters():
        prm.requires_grad_(train_filter(n))
    sched = wn.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, dynamics_type="Flow-SDE")
    ad = wn.Wan2I2VNativeAdapter(mod, I.engine_config(wn, cfg_o, image_dim=image_dim), sched, latent_storage_dtype="fp16")
    ad.rollout()
    ad.scheduler.set_timesteps(4)
    ad.scheduler.sigmas = ad.scheduler.sigmas.clone()
    ad.scheduler.sigmas[1] = SMAX
    return ad, mod


T0, T1, ETA, SMAX = 900.0, 750.0, 0.7, 0.9


def _inputs(cfg_o, B, T, h, w, Nt, seed=0, Ni=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    inp = dict(x=mk(B, 16, T, h, w).half(), x1=mk(B, 16, T, h, w).half(), pe=mk(B, Nt, cfg_o.text_dim).bfloat16(), ne=mk(B, Nt, cfg_o.text_dim).bfloat16(),
               wlp=mk(B), wnp=mk(B, 16, T, h, w), cond=I.make_condition(B, T, h, w, g))
    if Ni:
        inp["ie"] = mk(B, Ni, DI).bfloat16()
    return inp


def _oracle_loss(mod, cfg_o, inp, guidance, kl_w, quant=None, device="cpu", image_branch=True):
    from _gpu_oracle import oracle_loss_on
    return oracle_loss_on(device, _oracle_loss_impl, mod, cfg_o, inp, guidance, kl_w, quant=quant, image_branch=image_branch)


def _oracle_loss_impl(mod, cfg_o, inp, guidance, kl_w, quant=None, image_branch=True):
    """tests/test_gpu_wan_backward._oracle_loss_impl with the network fed `cat([x, condition], 1)`."""
    from oracle import wan_ref as R
    sd = {n: p_.detach().to(inp["x"].device).float().requires_grad_(p_.requires_grad) for n, p_ in mod.named_parameters()}
    x, x1 = inp["x"].float(), inp["x1"].float()
    B = x.shape[0]
    tt = torch.full((B,), T0)
    ikw = dict(image_embeds=inp.get("ie"), image_branch=image_branch)
    pos = I.forward(R, sd, cfg_o, x, tt, inp["pe"].float(), inp["cond"], quant=quant, **ikw)
    v = pos
    if guidance > 1.0:
        neg = I.forward(R, sd, cfg_o, x, tt, inp["ne"].float(), inp["cond"], quant=quant, **ikw)
        v = neg + guidance * (pos - neg)
    sigma, sigma_n = T0 / 1000.0, T1 / 1000.0
    dt = sigma_n - sigma
    std = math.sqrt(sigma / (1 - (SMAX if sigma == 1.0 else sigma))) * ETA
    mean = x * (1 + std ** 2 / (2 * sigma) * dt) + v * (1 + std ** 2 * (1 - sigma) / (2 * sigma)) * dt
    sv = std * math.sqrt(-dt)
    lp = (-((x1 - mean) ** 2) / (2 * sv ** 2) - math.log(sv) - math.log(math.sqrt(2 * math.pi))).mean(dim=(1, 2, 3, 4))
    ((inp["wlp"] * lp).sum() + kl_w * (inp["wnp"] * v).mean()).backward()
    return lp.detach(), {n: s.grad for n, s in sd.items() if s.requires_grad}


def _kw_i2v(inp, B, guidance):
    kw = dict(_kw(inp, B, T0, T1, ETA, guidance), condition=inp["cond"].cuda())
    if "ie" in inp:
        kw["image_embeds"] = inp["ie"].cuda()
    return kw


_default = lambda n: any(k in n for k in DEFAULT_TARGETS)      # noqa: E731
_bf16 = lambda z: z.to(torch.bfloat16).float()                 # noqa: E731


@pytest.mark.parametrize("guidance", [1.0, 5.0])
@pytest.mark.parametrize("B,T,h,w,Nt,Ni", [(2, 3, 8, 12, 9, 0), (2, 3, 8, 12, 9, 7), (1, 2, 6, 10, 64, 70)])
def test_i2v_replay_gradients_match_oracle_autograd_and_ratio_is_one(wn, B, T, h, w, Nt, Ni, guidance):
    """The default target modules trainable; every other parameter -- the image branch's among them -- keeps `grad is None` (`_compare`).
    Weight scale 0.08: `_compare` asks for cosine > 0.99, which only measures the engine where the bf16-emulating oracle ITSELF is well inside
    it.  At std 0.05 the oracle's own bf16 run has cosine 0.982 at B = 1, S = 30, Ni = 70, guidance 5 (0.97-0.99 over other input seeds; smaller
    scales are worse: 0.93 at 0.03), at 0.08 it is >= 0.995 at every shape, guidance and seed tried -- measured on the oracle alone, on the CPU,
    and asserted below before the engine is compared."""
    from oracle import wan_ref as R
    from test_gpu_wan_backward import _cos
    cfg_o = I.oracle_config(R)
    ad, mod = _build(wn, cfg_o, _default, std=0.08, image_dim=DI if Ni else 0)
    inp = _inputs(cfg_o, B, T, h, w, Nt, seed=5, Ni=Ni)
    kw = _kw_i2v(inp, B, guidance)
    with torch.no_grad():
        ref_out = ad.forward(**kw)
    out = ad.forward(**kw)
    assert out.log_prob.requires_grad and out.noise_pred.requires_grad
    assert torch.equal(out.noise_pred.detach(), ref_out.noise_pred) and torch.equal(out.log_prob.detach(), ref_out.log_prob)
    kl_w = 3.0
    ((inp["wlp"].cuda() * out.log_prob).sum() + kl_w * (inp["wnp"].cuda() * out.noise_pred).mean()).backward()
    lp_ref, g_ref = _oracle_loss(mod, cfg_o, inp, guidance, kl_w)
    _, g_band = _oracle_loss(mod, cfg_o, inp, guidance, kl_w, quant=_bf16)
    band_cos = min(_cos(g_band[n], g_ref[n]) for n in g_ref)
    print(f"bf16-emulating oracle vs fp32 oracle: worst gradient cosine {band_cos:.4f}")
    assert band_cos > 0.995, band_cos          # the configuration is well conditioned: the check below measures the engine
    np.testing.assert_allclose(out.log_prob.detach().cpu().numpy(), lp_ref.numpy(), rtol=2e-2)
    _compare(mod, g_ref, g_band, f"Wan I2V replay (B {B}, {T}x{h}x{w}, Nt {Nt}, Ni {Ni}, guidance {guidance})", 36)      # frozen ones: grad is None
    ad.engine.close()


def test_i2v_one_block_gradient_values(wn):
    """VALUE (`_compare_value`): one block, guidance 1, 4 096 video tokens over the batch, 257 image tokens.  This is where a dropped `dq_img`
    term shows: first, on the CPU, the oracle WITHOUT the image branch moves the gradient of `attn2.to_q.weight` by more than that tensor's
    tolerance (2 x band + 3e-3)."""
    from oracle import wan_ref as R
    from test_gpu_wan_backward import _rel
    cfg_o = I.oracle_config(R, base=R.tiny_config(num_layers=1))
    ad, mod = _build(wn, cfg_o, _default, seed=41, image_dim=DI)
    try:
        B, T, h, w, Nt, Ni = 2, 8, 32, 32, 64, 257
        inp = _inputs(cfg_o, B, T, h, w, Nt, seed=43, Ni=Ni)
        inp["wlp"] = torch.ones(B)
        lp_ref, g_ref = _oracle_loss(mod, cfg_o, inp, 1.0, 0.0)
        _, g_band = _oracle_loss(mod, cfg_o, inp, 1.0, 0.0, quant=_bf16)
        _, g_none = _oracle_loss(mod, cfg_o, inp, 1.0, 0.0, image_branch=False)
        n = "blocks.0.attn2.to_q.weight"
        moved, tol = _rel(g_none[n], g_ref[n]), 2.0 * _rel(g_band[n], g_ref[n]) + 3e-3
        print(f"oracle without the image branch: {n} gradient moves by rel-L2 {moved:.3e} (tolerance of that tensor {tol:.3e})")
        assert moved > tol, (moved, tol)
        out = ad.forward(**_kw_i2v(inp, B, 1.0))
        out.log_prob.sum().backward()
        np.testing.assert_allclose(out.log_prob.detach().cpu().numpy(), lp_ref.numpy(), rtol=2e-2)
        _compare_value(mod, g_ref, g_band, "Wan I2V one block (4 096 tokens, 257 image tokens, guidance 1)")
    finally:
        ad.engine.close()


def test_i2v_a_nograd_forward_between_forward_and_backward_changes_nothing(wn):
    """The KL reference pass: a training forward, then a no-grad forward with ANOTHER condition and other image embeddings (and other latents) on
    the same plan shape, then the backward -- gradients bit-identical to those without the intruder (the stash holds its own image K / V^T;
    the backward reads nothing below blocks.0, so the condition columns need no copy)."""
    from oracle import wan_ref as R
    cfg_o = I.oracle_config(R)
    ad, mod = _build(wn, cfg_o, _default, seed=7, image_dim=DI)
    B, T, h, w, Nt, Ni = 2, 2, 8, 12, 17, 70
    inp, other = _inputs(cfg_o, B, T, h, w, Nt, seed=5, Ni=Ni), _inputs(cfg_o, B, T, h, w, Nt, seed=6, Ni=Ni)
    wlp, wnp = inp["wlp"].cuda(), inp["wnp"].cuda()
    grads = []
    for intrude in (False, True):
        for prm in mod.parameters():
            prm.grad = None
        out = ad.forward(**_kw_i2v(inp, B, 5.0))
        if intrude:
            with torch.no_grad():
                o2 = ad.forward(**_kw_i2v(other, B, 5.0))
            assert not torch.equal(o2.noise_pred, out.noise_pred.detach())
        ((wlp * out.log_prob).sum() + (wnp * out.noise_pred).mean()).backward()
        grads.append({n: p_.grad.clone() for n, p_ in mod.named_parameters() if p_.requires_grad})
    assert len(grads[0]) >= 36
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n
    ad.engine.close()


@pytest.mark.parametrize("name", ["blocks.0.attn2.add_k_proj.weight", "patch_embedding.weight"])
def test_i2v_trainable_parameter_outside_the_scope_is_refused_in_grad_mode(wn, name):
    """The image branch's parameters and `patch_embedding` are outside the native backward's scope (and the reference's default target
    modules): `grad_supported` says so, and a grad-mode forward() with one of them trainable raises on the standalone adapter (under the
    Flow-Factory plugin the same refusal carries the documented opt-in, MI355_ALLOW_REFERENCE_AUTOGRAD=1: tests/test_plugin_wan_i2v_binding.py)."""
    from oracle import wan_ref as R
    cfg_o = I.oracle_config(R)
    ad, mod = _build(wn, cfg_o, lambda n: _default(n) or n == name, image_dim=DI)
    assert ad.engine.grad_supported(name) == 0 and ad.engine.grad_supported("blocks.0.attn2.to_q.weight") == 1
    inp = _inputs(cfg_o, 2, 2, 8, 12, 9, seed=5, Ni=7)
    with pytest.raises(NotImplementedError, match=name.split(".")[-2]):
        ad.forward(**_kw_i2v(inp, 2, 1.0))
    ad.engine.close()


def test_i2v_training_step_schedule_is_race_free(wn):
    """The emitted schedule of one I2V training step with the image branch (mi355_sched_trace) under tests/_sched_check.py; the new launches --
    `patchify_cols` (condition columns, latent columns), `gelu_erf` (image embedder), `add_bf16` (o_text + o_img per block, dq~_text + dq~_img per
    block) -- are in it with their regions."""
    import _sched_check as SC
    from mi355_flow import _lib
    from oracle import wan_ref as R
    from test_gpu_schedules import _trace_of
    lib = _lib.load()
    lib.mi355_tune_set(26, 1)
    cfg_o = I.oracle_config(R)
    ad, mod = _build(wn, cfg_o, _default, seed=31, image_dim=DI)
    B = 2
    inp = _inputs(cfg_o, B, 2, 8, 12, 17, seed=9, Ni=7)
    kw = _kw_i2v(inp, B, 5.0)
    wlp, wnp = inp["wlp"].cuda(), inp["wnp"].cuda()

    def step():
        for prm in mod.parameters():
            prm.grad = None
        out = ad.forward(**kw)
        ((wlp * out.log_prob).sum() + (wnp * out.noise_pred).mean()).backward()

    try:
        step()
        s = SC.parse(_trace_of(lib, step, reps=1))
        pc = [o for o in s.ops if o.name == "patchify_cols"]
        assert len(pc) == 2 and all(o.regions for o in pc), pc
        L = cfg_o.num_layers
        for nm, cnt in (("gelu_erf", 1), ("add_bf16", 2 * L)):
            ops = [o for o in s.ops if o.name == nm]
            assert len(ops) == cnt and all(o.regions for o in ops), (nm, len(ops))
        assert "patchify" not in {o.name for o in s.ops}
        assert {"attention128_bwd", "gemm_tn", "norm_rope_full_bwd"} <= {o.name for o in s.ops}
        races = s.races()
        assert races == [], races[:5]
        print(f"wan I2V optimize() step: {sum(1 for o in s.ops if o.regions)} launches on {len(s.streams())} stream(s), no race")
    finally:
        ad.engine.close()

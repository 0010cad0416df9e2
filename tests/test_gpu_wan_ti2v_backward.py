"""GPU parity of the native backward on a Wan first-frame plan (Wan2.2-TI2V-5B image-to-video: mi355_wan_forward_train_ff +
mi355_wan_backward, whose LayerNorm-modulate backward and gate products read the two-group modulation table) against torch autograd through
the oracle with per-token timesteps on the merged input (tests/_wan_ti2v_ref.py).  Helpers and tolerances are tests/test_gpu_wan_backward.py's
own (`_compare`: rel-L2 < 3 x band + 5e-3, cosine > 0.99; `_compare_value`)."""
import math
import os

import numpy as np
import pytest
import torch

import _plugin_fakes as PF
import _wan_ti2v_ref as TI
from test_gpu_wan_backward import DEFAULT_TARGETS, _compare, _compare_value, _kw

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("MI355_WAN_NATIVE_BACKWARD") == "0", reason="MI355_WAN_NATIVE_BACKWARD=0 opts out")]

C = TI.C
T0, T1, ETA, SMAX = 900.0, 750.0, 0.7, 0.9


@pytest.fixture(scope="module")
def wn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import wan
    assert wan.WanEngine.native_backward_enabled
    return wan


def _module(cfg_o, train_filter, seed=3, std=0.05):
    """tests/test_gpu_wan_backward._build's module on the 48-channel transformer"""
    from oracle import wan_ref as R
    mod = PF.build_module_tree(R.state_dict_shapes(cfg_o), buffers=(), seed=seed, std=std)
    with torch.no_grad():
        for n, prm in mod.named_parameters():
            if ".norm_q." in n or ".norm_k." in n or n.endswith("norm2.weight"):
                prm.copy_(1.0 + 0.1 * prm / std)
            prm.copy_(prm.bfloat16().float())
    for n, prm in mod.named_parameters():
        prm.requires_grad_(train_filter(n))
    return mod


def _build(wn, cfg_o, train_filter, seed=3, std=0.05):
    mod = _module(cfg_o, train_filter, seed, std).cuda()
    sched = wn.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, dynamics_type="Flow-SDE")
    ad = wn.Wan2TI2VNativeAdapter(mod, TI.engine_config(wn, cfg_o), sched, latent_storage_dtype="fp16")
    ad.rollout()
    ad.scheduler.set_timesteps(4)
    ad.scheduler.sigmas = ad.scheduler.sigmas.clone()
    ad.scheduler.sigmas[1] = SMAX
    return ad, mod


def _inputs(cfg_o, B, T, h, w, Nt, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    return dict(x=mk(B, C, T, h, w).half(), x1=mk(B, C, T, h, w).half(), pe=mk(B, Nt, cfg_o.text_dim).bfloat16(), ne=mk(B, Nt, cfg_o.text_dim).bfloat16(),
                wlp=mk(B), wnp=mk(B, C, T, h, w), ff=TI.bf(mk(B, C, 1, h, w)))


def _oracle_loss(mod, cfg_o, inp, guidance, kl_w, quant=None, device="cpu", per_token=True):
    from _gpu_oracle import oracle_loss_on
    lp, grads = oracle_loss_on(device, _oracle_loss_impl, mod, cfg_o, inp, guidance, kl_w, quant=quant, per_token=per_token)
    return lp, {n: g.cpu() for n, g in grads.items()}


def _oracle_loss_impl(mod, cfg_o, inp, guidance, kl_w, quant=None, per_token=True):
    """tests/test_gpu_wan_backward._oracle_loss_impl with the network fed the merged input and the per-token timestep; the scheduler step and
    the log-prob on the UNMERGED latents, all frames (the reference's)."""
    from oracle import wan_ref as R
    sd = {n: p_.detach().to(inp["x"].device).float().requires_grad_(p_.requires_grad) for n, p_ in mod.named_parameters()}
    x, x1 = inp["x"].float(), inp["x1"].float()
    t = torch.tensor(T0)
    pos = TI.forward(R, sd, cfg_o, x, t, inp["pe"].float(), inp["ff"], quant=quant, per_token=per_token)
    v = pos
    if guidance > 1.0:
        neg = TI.forward(R, sd, cfg_o, x, t, inp["ne"].float(), inp["ff"], quant=quant, per_token=per_token)
        v = neg + guidance * (pos - neg)
    sigma, sigma_n = T0 / 1000.0, T1 / 1000.0
    dt = sigma_n - sigma
    std = math.sqrt(sigma / (1 - (SMAX if sigma == 1.0 else sigma))) * ETA
    mean = x * (1 + std ** 2 / (2 * sigma) * dt) + v * (1 + std ** 2 * (1 - sigma) / (2 * sigma)) * dt
    sv = std * math.sqrt(-dt)
    lp = (-((x1 - mean) ** 2) / (2 * sv ** 2) - math.log(sv) - math.log(math.sqrt(2 * math.pi))).mean(dim=(1, 2, 3, 4))
    ((inp["wlp"] * lp).sum() + kl_w * (inp["wnp"] * v).mean()).backward()
    return lp.detach(), {n: s.grad for n, s in sd.items() if s.requires_grad}


def _kw_ti2v(wn, inp, B, guidance):
    T, h, w = inp["x"].shape[2:]
    return dict(_kw(inp, B, T0, T1, ETA, guidance), condition=inp["ff"].cuda(), first_frame_mask=wn.wan_first_frame_mask(T, h, w, device="cuda"))


_default = lambda n: any(k in n for k in DEFAULT_TARGETS)      # noqa: E731
_bf16 = lambda z: z.to(torch.bfloat16).float()                 # noqa: E731


@pytest.mark.parametrize("guidance", [1.0, 5.0])
@pytest.mark.parametrize("B,T,h,w,Nt", [(2, 3, 6, 10, 9), (2, 1, 6, 10, 17)])
def test_ti2v_replay_gradients_match_oracle_autograd_and_ratio_is_one(wn, B, T, h, w, Nt, guidance):
    """The default target modules trainable (weight scale 0.08: the bf16-emulating oracle's own gradient cosine is asserted > 0.995 first, as
    the I2V test does -- `_compare`'s cosine > 0.99 then measures the engine).  T = 1: every token is a head token."""
    from oracle import wan_ref as R
    from test_gpu_wan_backward import _cos
    cfg_o = TI.oracle_config(R)
    ad, mod = _build(wn, cfg_o, _default, std=0.08)
    inp = _inputs(cfg_o, B, T, h, w, Nt, seed=5)
    kw = _kw_ti2v(wn, inp, B, guidance)
    with torch.no_grad():
        ref_out = ad.forward(**kw)
    out = ad.forward(**kw)
    assert out.log_prob.requires_grad and out.noise_pred.requires_grad
    assert torch.equal(out.noise_pred.detach(), ref_out.noise_pred) and torch.equal(out.log_prob.detach(), ref_out.log_prob)      # ratio == 1
    kl_w = 3.0
    ((inp["wlp"].cuda() * out.log_prob).sum() + kl_w * (inp["wnp"].cuda() * out.noise_pred).mean()).backward()
    lp_ref, g_ref = _oracle_loss(mod, cfg_o, inp, guidance, kl_w)
    _, g_band = _oracle_loss(mod, cfg_o, inp, guidance, kl_w, quant=_bf16)
    band_cos = min(_cos(g_band[n], g_ref[n]) for n in g_ref)
    print(f"bf16-emulating oracle vs fp32 oracle: worst gradient cosine {band_cos:.4f}")
    assert band_cos > 0.995, band_cos
    np.testing.assert_allclose(out.log_prob.detach().cpu().numpy(), lp_ref.numpy(), rtol=2e-2)
    _compare(mod, g_ref, g_band, f"Wan TI2V replay (B {B}, {T}x{h}x{w}, Nt {Nt}, guidance {guidance})", 36)
    ad.engine.close()


def test_ti2v_one_block_gradient_values(wn):
    """VALUE (`_compare_value`): one block, guidance 1, 4 096 video tokens over the batch (256 head tokens per sample).  First, on the oracle:
    with the SCALAR timestep the gradient of `ffn.net.2.weight` (behind the gate) moves by more than that tensor's tolerance (2 x band + 3e-3),
    so a backward that read one modulation row per sample would not pass."""
    from oracle import wan_ref as R
    from test_gpu_wan_backward import _rel
    cfg_o = TI.oracle_config(R, base=R.tiny_config(num_layers=1))
    ad, mod = _build(wn, cfg_o, _default, seed=41)
    try:
        B, T, h, w, Nt = 2, 8, 32, 32, 64
        inp = _inputs(cfg_o, B, T, h, w, Nt, seed=43)
        inp["wlp"] = torch.ones(B)
        lp_ref, g_ref = _oracle_loss(mod, cfg_o, inp, 1.0, 0.0, device="cuda")
        _, g_band = _oracle_loss(mod, cfg_o, inp, 1.0, 0.0, quant=_bf16, device="cuda")
        _, g_scalar = _oracle_loss(mod, cfg_o, inp, 1.0, 0.0, device="cuda", per_token=False)
        n = "blocks.0.ffn.net.2.weight"
        moved, tol = _rel(g_scalar[n], g_ref[n]), 2.0 * _rel(g_band[n], g_ref[n]) + 3e-3
        print(f"oracle with the scalar timestep: {n} gradient moves by rel-L2 {moved:.3e} (tolerance of that tensor {tol:.3e})")
        assert moved > tol, (moved, tol)
        out = ad.forward(**_kw_ti2v(wn, inp, B, 1.0))
        out.log_prob.sum().backward()
        np.testing.assert_allclose(out.log_prob.detach().cpu().numpy(), lp_ref.numpy(), rtol=2e-2)
        _compare_value(mod, g_ref, g_band, "Wan TI2V one block (4 096 tokens, guidance 1)")
    finally:
        ad.engine.close()


def test_ti2v_backward_at_equal_timesteps_is_the_t2v_backward_bit_for_bit(wn):
    """Plan level: forward_train + backward on a first-frame plan with t_head == t_rest and the latents' own frame 0, against the text-to-video
    plan of the same engine: the prediction and every weight gradient are bit-identical (the split backward kernels read two equal rows)."""
    from oracle import wan_ref as R
    cfg_o = TI.oracle_config(R)
    eng = wn.WanEngine(TI.engine_config(wn, cfg_o))
    eng.bind_state_dict({n: p_.detach().cuda() for n, p_ in _module(cfg_o, _default, seed=9).named_parameters()})
    eng.ready()
    B, T, h, w, Nt = 2, 3, 6, 10, 9
    inp = _inputs(cfg_o, B, T, h, w, Nt, seed=2)
    x, pe, ne = inp["x"].cuda(), inp["pe"].cuda(), inp["ne"].cuda()
    names = [n for n in eng.param_names() if eng.grad_supported(n) == 1]
    assert len(names) >= 36
    shapes = R.state_dict_shapes(cfg_o)
    dv = torch.randn(2 * B, C, T, h, w, generator=torch.Generator().manual_seed(1)).cuda()

    def run(plan, t, **kw):
        grads = {n: torch.zeros(shapes[n], device="cuda", dtype=torch.float32) for n in names}
        for n in names:
            eng.set_grad(n, grads[n])
        try:
            v = plan.forward_train(x, t, ne, pe, **kw).clone()
            plan.backward(dv)
            torch.cuda.synchronize()
        finally:
            eng.clear_grads()
        return v, grads

    v_a, g_a = run(eng.plan(B, 2, T, h, w, Nt, 1), torch.tensor([611.0]))
    v_b, g_b = run(eng.plan(B, 2, T, h, w, Nt, 1, first_frame=True), torch.tensor([[611.0, 611.0]]), first_frame=x[:, :, :1].contiguous(), t_pairs=True)
    assert torch.equal(v_a, v_b)
    assert all(float(g_a[n].abs().max()) > 0 for n in names)
    for n in names:
        assert torch.equal(g_a[n], g_b[n]), n
    # ... and with the reference's timesteps (0, t) the gradients are others
    _, g_c = run(eng.plan(B, 2, T, h, w, Nt, 1, first_frame=True), torch.tensor([611.0]), first_frame=x[:, :, :1].contiguous())
    assert not torch.equal(g_c["blocks.0.ffn.net.2.weight"], g_a["blocks.0.ffn.net.2.weight"])
    eng.close()


def test_ti2v_training_step_schedule_is_race_free(wn):
    """The emitted schedule of one TI2V training step (mi355_sched_trace) under tests/_sched_check.py: the first-frame merge (`patchify_head`,
    behind `patchify`) is in it with its regions, and the modulation regions of `ln_mod` / `gemm.gate_res` / `ln_mod_bwd` / `gate_mul` cover
    two rows per sample."""
    import _sched_check as SC
    from mi355_flow import _lib
    from oracle import wan_ref as R
    from test_gpu_schedules import _trace_of
    lib = _lib.load()
    lib.mi355_tune_set(26, 1)
    cfg_o = TI.oracle_config(R)
    ad, mod = _build(wn, cfg_o, _default, seed=31)
    B = 2
    inp = _inputs(cfg_o, B, 2, 6, 10, 17, seed=9)
    kw = _kw_ti2v(wn, inp, B, 5.0)
    wlp, wnp = inp["wlp"].cuda(), inp["wnp"].cuda()

    def step():
        for prm in mod.parameters():
            prm.grad = None
        out = ad.forward(**kw)
        ((wlp * out.log_prob).sum() + (wnp * out.noise_pred).mean()).backward()

    try:
        step()
        s = SC.parse(_trace_of(lib, step, reps=1))
        names = [o.name for o in s.ops]
        for nm in ("patchify", "patchify_head"):
            ops = [o for o in s.ops if o.name == nm]
            assert len(ops) == 1 and all(o.regions for o in ops), (nm, len(ops))
        assert names.index("patchify") < names.index("patchify_head")
        assert {"ln_mod", "gemm.gate_res", "ln_mod_bwd", "gate_mul", "attention128_bwd", "gemm_tn", "norm_rope_full_bwd"} <= set(names)
        races = s.races()
        assert races == [], races[:5]
        print(f"wan TI2V optimize() step: {sum(1 for o in s.ops if o.regions)} launches on {len(s.streams())} stream(s), no race")
    finally:
        ad.engine.close()

"""GPU parity of the Wan image-to-video path -- the condition channels (Wan2.2-I2V-A14B) and the CLIP image cross-attention branch
(Wan2.1-I2V): mi355_wan_create_i2v and the `_i2v` entry points; reference models/wan/wan2_i2v.py:425-783 -- against the CPU oracle fed the
concatenated input (tests/_wan_i2v_ref.py over oracle/wan_ref.py; network body parity-unpinned).  Tolerances are tests/test_gpu_wan.py's:
forward / latents rel-L2 < 2e-2 on the tiny config, log-probs rtol 1e-3, `check_in_band` at full width."""
import pytest
import torch

import _wan_i2v_ref as I

pytestmark = pytest.mark.gpu

TOL = 2e-2
DI = 128          # image_dim of the tiny configuration


@pytest.fixture(scope="module")
def wn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import wan
    return wan


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _setup(wn, cfg_o, seed=55, image_dim=0):
    from oracle import wan_ref as R
    return I.make_state_dict(R, cfg_o, seed, image_dim), I.engine_config(wn, cfg_o, image_dim=image_dim)


def _engine(wn, sd, cfg):
    eng = wn.WanEngine(cfg)
    eng.bind_state_dict({k: v.cuda() for k, v in sd.items()})
    eng.ready()
    return eng


def _inputs(cfg_o, B, T, h, w, Nt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 16, T, h, w, generator=g).half()
    pe = I.bf(torch.randn(B, Nt, cfg_o.text_dim, generator=g))
    ne = I.bf(torch.randn(B, Nt, cfg_o.text_dim, generator=g))
    return x, pe, ne, I.make_condition(B, T, h, w, g)


def _image_embeds(B, Ni, seed, image_dim=DI):
    return I.bf(torch.randn(B, Ni, image_dim, generator=torch.Generator().manual_seed(seed))) if Ni else None


def _oracle_pair(R, sd, cfg_o, x, t, ne, pe, cond, n_cfg, ie=None, quant=None):
    B = x.shape[0]
    pos = I.forward(R, sd, cfg_o, x, t.expand(B), pe, cond, image_embeds=ie, quant=quant)
    return torch.cat([I.forward(R, sd, cfg_o, x, t.expand(B), ne, cond, image_embeds=ie, quant=quant), pos]) if n_cfg == 2 else pos


def _engine_pair(plan, x, t, ne, pe, cond, n_cfg, ie=None):
    kw = dict(condition=cond.cuda(), image_embeds=ie.cuda() if ie is not None else None)
    if n_cfg == 2:
        return plan.transformer_forward(x.cuda(), t, ne.cuda(), pe.cuda(), **kw).float().cpu()
    return plan.transformer_forward(x.cuda(), t, pe.cuda(), **kw).float().cpu()


# (B, T, h, w, Nt, Ni, n_cfg): channels only; a few image keys; image keys across one 64-key tile with a ragged S = 30; the real count of 257
# (Ni_pad = 320).  Then channel-only cases at the other geometries with the condition in bf16 / fp16: its dtype code is an argument of its own.
@pytest.mark.parametrize("B,T,h,w,Nt,Ni,n_cfg,cdt", [(2, 3, 8, 12, 9, 0, 1, torch.float32), (2, 3, 8, 12, 9, 7, 1, torch.float32),
                                                     (1, 2, 6, 10, 64, 70, 2, torch.float32), (2, 1, 16, 16, 17, 257, 2, torch.float32),
                                                     (2, 3, 8, 12, 9, 0, 2, torch.bfloat16), (1, 2, 6, 10, 64, 0, 2, torch.float16)])
def test_i2v_forward_matches_oracle(wn, B, T, h, w, Nt, Ni, n_cfg, cdt):
    """36-channel patch embedding through a K = 144 -> 192 padded GEMM (latents in columns 0..63, condition in 64..143); with Ni > 0 the image
    embedder, the per-block image K / V^T and the second cross-attention added onto the text one (the Ni = 0 cases bind an engine without the branch)."""
    from oracle import wan_ref as R
    cfg_o = I.oracle_config(R)
    sd, cfg = _setup(wn, cfg_o, image_dim=DI if Ni else 0)
    eng = _engine(wn, sd, cfg)
    x, pe, ne, cond = _inputs(cfg_o, B, T, h, w, Nt, seed=T * h + w + Nt)
    ie = _image_embeds(B, Ni, seed=Ni)
    t = torch.tensor([874.0])
    got = _engine_pair(eng.plan(B, n_cfg, T, h, w, Nt, 1, n_image=Ni), x, t, ne, pe, cond.to(cdt), n_cfg, ie)
    ref = _oracle_pair(R, sd, cfg_o, x, t, ne, pe, cond, n_cfg, ie)
    assert got.shape == ref.shape == (B * n_cfg, 16, T, h, w)
    r = _rel(got, ref)
    print(f"Wan I2V forward ({B}, {T}x{h}x{w}, Nt {Nt}, Ni {Ni}, n_cfg {n_cfg}, condition {cdt}): rel-L2 {r:.3e}")
    assert r < TOL, r
    eng.close()


def test_i2v_each_input_matters_and_reaches_its_own_sample(wn):
    """The oracle's output moves by more than 5 x the forward tolerance when the condition is zeroed, when `image_embeds` are zeroed, and when
    the two samples' conditions / image embeddings are swapped (asserted on the CPU first); the engine follows the oracle within tolerance in
    each case -- with CFG, so that both halves read the condition and the image keys of their own sample."""
    from oracle import wan_ref as R
    cfg_o = I.oracle_config(R)
    sd, cfg = _setup(wn, cfg_o, seed=56, image_dim=DI)
    B, T, h, w, Nt, Ni = 2, 3, 8, 12, 9, 7
    x, pe, ne, cond = _inputs(cfg_o, B, T, h, w, Nt, seed=3)
    ie = _image_embeds(B, Ni, seed=4)
    t = torch.tensor([874.0])
    cases = {"given": (cond, ie), "condition zeroed": (torch.zeros_like(cond), ie), "conditions swapped": (cond.flip(0), ie),
             "image_embeds zeroed": (cond, torch.zeros_like(ie)), "image_embeds swapped": (cond, ie.flip(0))}
    refs = {k: _oracle_pair(R, sd, cfg_o, x, t, ne, pe, c, 2, e) for k, (c, e) in cases.items()}
    for k in cases:
        if k != "given":
            moved = _rel(refs[k], refs["given"])
            print(f"oracle: {k} moves the output by rel-L2 {moved:.3e}")
            assert moved > 5 * TOL, (k, moved)
    eng = _engine(wn, sd, cfg)
    plan = eng.plan(B, 2, T, h, w, Nt, 1, n_image=Ni)
    for k, (c, e) in cases.items():
        r = _rel(_engine_pair(plan, x, t, ne, pe, c, 2, e), refs[k])
        print(f"engine vs oracle, {k}: rel-L2 {r:.3e}")
        assert r < TOL, (k, r)
    eng.close()


def test_i2v_patch_layout_is_exact(wn):
    """An I2V engine whose condition columns of `patch_embedding.weight` are zero, fed an arbitrary non-zero condition, computes bit for bit what a
    T2V engine with the same other weights computes: zero products add exactly (K = 192 with 128 zero-weight columns against K = 64), so any
    difference is a misplaced column or a dirty padding column."""
    from oracle import wan_ref as R
    cfg_t = R.tiny_config()
    sd_t = I.make_state_dict(R, cfg_t, 57)
    sd_i = dict(sd_t)
    D = cfg_t.dim
    sd_i["patch_embedding.weight"] = torch.cat([sd_t["patch_embedding.weight"], torch.zeros(D, I.COND, 1, 2, 2)], 1)
    e_t = _engine(wn, sd_t, wn.WanConfig(num_layers=cfg_t.num_layers, num_attention_heads=cfg_t.num_attention_heads, ffn_dim=cfg_t.ffn_dim,
                                         text_dim=cfg_t.text_dim))
    e_i = _engine(wn, sd_i, I.engine_config(wn, cfg_t))
    B, T, h, w, Nt = 2, 3, 8, 12, 9
    x, pe, ne, cond = _inputs(cfg_t, B, T, h, w, Nt, seed=11)
    t = torch.tensor([611.0])
    a = e_t.plan(B, 2, T, h, w, Nt, 1).transformer_forward(x.cuda(), t, ne.cuda(), pe.cuda())
    b = e_i.plan(B, 2, T, h, w, Nt, 1).transformer_forward(x.cuda(), t, ne.cuda(), pe.cuda(), condition=(7.0 * cond + 3.0).cuda())
    assert torch.equal(a, b)
    e_t.close(); e_i.close()


def _adapter(wn, sd, cfg, sched, **kw):
    ad = wn.Wan2I2VNativeAdapter({k: v.cuda() for k, v in sd.items()}, cfg, sched, latent_storage_dtype="fp16", **kw)
    ad.rollout()
    return ad


def test_i2v_rollout_matches_oracle_replays_and_refreshes_the_condition(wn):
    """On an engine with the image branch (Ni = 7).  N = 4 Flow-SDE with CFG against the oracle loop (per-step latents, log-probs rtol 1e-3); the
    engine's replay of a stored transition gives ratio exactly 1; the fused rollout equals the step-wise one bit for bit; a second rollout on
    the same plan with a DIFFERENT condition and other image embeddings gives their result (the hoisted condition columns and image K / V^T
    are rewritten by every call), and the first inputs again their own."""
    from oracle import wan_ref as R
    cfg_o = I.oracle_config(R)
    sd, cfg = _setup(wn, cfg_o, seed=12, image_dim=DI)
    sched = wn.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[0, 1, 2, 3], num_sde_steps=2, seed=42, dynamics_type="Flow-SDE")
    ad = _adapter(wn, sd, cfg, sched)
    B, Nt, N, H, W, frames, guidance = 2, 12, 4, 64, 96, 9, 5.0
    T, h, w = 3, 8, 12
    g = torch.Generator().manual_seed(4)
    pe = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    ne = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    cond_a, cond_b = I.make_condition(B, T, h, w, g), I.make_condition(B, T, h, w, g)
    ie_a, ie_b = _image_embeds(B, 7, seed=1), _image_embeds(B, 7, seed=2)
    kw = dict(prompt=["a", "b"], height=H, width=W, num_frames=frames, num_inference_steps=N, guidance_scale=guidance, prompt_embeds=pe.cuda(),
              negative_prompt_embeds=ne.cuda(), compute_log_prob=True, trajectory_indices="all")

    def run(cond, ie, **more):
        torch.cuda.manual_seed(31)
        return ad.inference(condition=cond.cuda(), image_embeds=ie.cuda(), **kw, **more)

    s_a = run(cond_a, ie_a)
    torch.cuda.manual_seed(31)          # RNG order of the reference: prepare_latents draws the fp32 latents first, then one fp32 draw per step
    init = torch.randn((B, 16, T, h, w), device="cuda", dtype=torch.float32).cpu()
    noise = torch.stack([torch.randn((B, 16, T, h, w), device="cuda", dtype=torch.float32) for _ in range(N)]).cpu()
    ts, sig = R.unipc_flow_schedule(N, 3.0)
    nl = ad.scheduler.host_noise_levels()
    sde = [i for i in range(N) if nl[i] > 0]
    assert len(sde) == 2

    def check(samples, cond, ie):
        with I.with_condition(R, cfg_o, cond, ie):
            ref = R.rollout(sd, cfg_o, pe, ne, guidance, init, noise, ts, sig, nl, torch.float16)
        for b in range(B):
            got = samples[b].all_latents.float().cpu()
            assert got.shape == (N + 1, 16, T, h, w)
            for pos in range(N + 1):
                assert _rel(got[pos], ref["all_latents"][pos, b]) < TOL, (b, pos)
            torch.testing.assert_close(samples[b].log_probs.cpu(), torch.stack([ref["log_probs"][i, b] for i in sde]), rtol=1e-3, atol=1e-4)
            assert torch.equal(samples[b].condition.cpu(), cond[b]) and samples[b].first_frame_mask is None
            assert torch.equal(samples[b].image_embeds.float().cpu(), ie[b])

    check(s_a, cond_a, ie_a)
    # replay of a stored transition: ratio == 1 exactly
    i = sde[0]
    x_i = torch.stack([s.all_latents[i] for s in s_a]).cuda()
    x_n = torch.stack([s.all_latents[i + 1] for s in s_a]).cuda()
    out = ad.forward(t=s_a[0].timesteps[i].reshape(1).expand(B).cuda(), latents=x_i, prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(),
                     guidance_scale=guidance, condition=torch.stack([s.condition for s in s_a]), image_embeds=torch.stack([s.image_embeds for s in s_a]), t_next=s_a[0].timesteps[i + 1].reshape(1).expand(B).cuda(),
                     next_latents=x_n, noise_level=nl[i], compute_log_prob=True, return_kwargs=["log_prob"])
    old = torch.stack([s.log_probs[0] for s in s_a]).cuda()
    assert torch.equal(torch.exp(out.log_prob - old), torch.ones_like(old))
    # fused == step-wise
    s_step = run(cond_a, ie_a, extra_call_back_kwargs=["noise_pred"])
    for sa, sb in zip(s_a, s_step):
        assert torch.equal(sa.all_latents, sb.all_latents) and torch.equal(sa.log_probs, sb.log_probs)
    # another condition on the same plan, then the first again
    s_b = run(cond_b, ie_b)
    check(s_b, cond_b, ie_b)
    assert not torch.equal(s_b[0].all_latents[1], s_a[0].all_latents[1])
    s_ab = run(cond_a, ie_b)                                            # only the image embeddings differ: the image K / V^T were refreshed
    assert not torch.equal(s_ab[0].all_latents[1], s_a[0].all_latents[1]) and not torch.equal(s_ab[0].all_latents[1], s_b[0].all_latents[1])
    s_a2 = run(cond_a, ie_a)
    for sa, sb in zip(s_a, s_a2):
        assert torch.equal(sa.all_latents, sb.all_latents) and torch.equal(sa.log_probs, sb.log_probs)
    ad.engine.close()


def test_i2v_evaluation_mode_sampling_matches_oracle(wn):
    """Evaluation mode (UniPC predictor-corrector) with CFG against `oracle.wan_ref.rollout_eval` fed the concatenated input."""
    from oracle import wan_ref as R
    cfg_o = I.oracle_config(R)
    sd, cfg = _setup(wn, cfg_o, seed=21)
    sched = wn.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[0, 1, 2], num_sde_steps=2, seed=42, dynamics_type="Flow-SDE")
    ad = _adapter(wn, sd, cfg, sched)
    ad.eval()
    B, Nt, N, H, W, frames, guidance = 2, 12, 4, 64, 96, 9, 4.0
    T, h, w = 3, 8, 12
    g = torch.Generator().manual_seed(4)
    pe = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    ne = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    cond = I.make_condition(B, T, h, w, g)
    torch.cuda.manual_seed(31)
    samples = ad.inference(condition=cond.cuda(), prompt=["a", "b"], height=H, width=W, num_frames=frames, num_inference_steps=N, guidance_scale=guidance,
                           prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), compute_log_prob=False, trajectory_indices="all")
    torch.cuda.manual_seed(31)
    init = torch.randn((B, 16, T, h, w), device="cuda", dtype=torch.float32).cpu()
    ts, sig = R.unipc_flow_schedule(N, 3.0)
    with I.with_condition(R, cfg_o, cond):
        ref = R.rollout_eval(sd, cfg_o, pe, ne, guidance, init, ts, sig, torch.float16)
    worst = max(_rel(samples[b].all_latents[pos].cpu(), ref["all_latents"][pos, b]) for b in range(B) for pos in range(1, N + 1))
    print(f"Wan I2V evaluation-mode sampling: worst latent rel-L2 vs the oracle loop {worst:.3e}")
    assert worst < TOL and samples[0].log_probs is None
    ad.engine.close()


def test_i2v_two_expert_rollout_matches_oracle_and_replays(wn):
    """Wan2.2-I2V-A14B's shape: two image-to-video engines without image branch, `boundary_ratio`; high-noise expert with CFG, low-noise without.
    Against `oracle.wan_ref.rollout_two_expert` fed the concatenated input; replay on either side of the boundary is bit-exact."""
    from oracle import wan_ref as R
    cfg_o = I.oracle_config(R)
    sd_hi, cfg = _setup(wn, cfg_o, seed=12)
    sd_lo, _ = _setup(wn, cfg_o, seed=99)
    sched = wn.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[0, 1, 2, 3, 4], num_sde_steps=5, seed=42, dynamics_type="Flow-SDE")
    ad = _adapter(wn, sd_hi, cfg, sched, state_dict_2={k: v.cuda() for k, v in sd_lo.items()}, boundary_ratio=0.9)
    B, Nt, N, H, W, frames, g1, g2 = 2, 12, 5, 64, 96, 9, 4.0, 1.0
    T, h, w = 3, 8, 12
    g = torch.Generator().manual_seed(4)
    pe = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    ne = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    cond = I.make_condition(B, T, h, w, g)
    torch.cuda.manual_seed(31)
    samples = ad.inference(condition=cond.cuda(), prompt=["a", "b"], height=H, width=W, num_frames=frames, num_inference_steps=N, guidance_scale=g1,
                           guidance_scale_2=g2, prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), compute_log_prob=True, trajectory_indices="all")
    torch.cuda.manual_seed(31)
    init = torch.randn((B, 16, T, h, w), device="cuda", dtype=torch.float32).cpu()
    noise = torch.stack([torch.randn((B, 16, T, h, w), device="cuda", dtype=torch.float32) for _ in range(N)]).cpu()
    ts, sig = R.unipc_flow_schedule(N, 3.0)
    hi_steps = [i for i in range(N) if float(ts[i]) >= 900.0]
    assert 0 < len(hi_steps) < N, ts
    nl = ad.scheduler.host_noise_levels()
    with I.with_condition(R, cfg_o, cond):
        ref = R.rollout_two_expert(sd_hi, sd_lo, cfg_o, 900.0, pe, ne, g1, g2, init, noise, ts, sig, nl, torch.float16)
    sde = [i for i in range(N) if nl[i] > 0]
    for b in range(B):
        for pos in range(N + 1):
            assert _rel(samples[b].all_latents[pos].cpu(), ref["all_latents"][pos, b]) < TOL, (b, pos)
        torch.testing.assert_close(samples[b].log_probs.cpu(), torch.stack([ref["log_probs"][i, b] for i in sde]), rtol=1e-3, atol=1e-4)
    for i in (hi_steps[-1], hi_steps[-1] + 1):
        x_i = torch.stack([s.all_latents[i] for s in samples]).cuda()
        x_n = torch.stack([s.all_latents[i + 1] for s in samples]).cuda()
        out = ad.forward(t=samples[0].timesteps[i].reshape(1).expand(B).cuda(), latents=x_i, prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(),
                         guidance_scale=g1, guidance_scale_2=g2, condition=cond.cuda(),
                         t_next=(samples[0].timesteps[i + 1] if i + 1 < N else torch.zeros(())).reshape(1).expand(B).cuda(),
                         next_latents=x_n, noise_level=nl[i], compute_log_prob=True, return_kwargs=["log_prob"])
        assert torch.equal(out.log_prob, torch.stack([s.log_probs[i] for s in samples]).cuda()), i
    ad.engine.close(); ad.engine_2.close()


def test_i2v_errors(wn):
    import ctypes as C
    from mi355_flow import _lib
    from mi355_flow.engine import _ptr, _stream
    small = dict(num_layers=1, num_attention_heads=1, ffn_dim=128, text_dim=64)
    e_i = wn.WanEngine(wn.WanConfig(cond_channels=20, **small))
    e_t = wn.WanEngine(wn.WanConfig(**small))
    assert "patch_embedding.weight" in e_i.param_names() and not any("add_k_proj" in n or "image_embedder" in n for n in e_i.param_names())
    lat, t, enc = torch.zeros(1, 16, 1, 4, 4).cuda(), torch.tensor([500.0]).cuda(), torch.zeros(1, 8, 64).cuda().bfloat16()
    cond, out = torch.ones(1, 20, 1, 4, 4).cuda(), torch.empty(1, 16, 1, 4, 4, dtype=torch.bfloat16).cuda()
    p_i, p_t = e_i.plan(1, 1, 1, 4, 4, 8, 1), e_t.plan(1, 1, 1, 4, 4, 8, 1)
    # a plain call on an image-to-video plan and the other way round: an error string, nothing runs (the weights are not even bound)
    with pytest.raises(RuntimeError, match="image-to-video plan"):
        p_i._call("forward", p_i._h, _stream(), _ptr(lat), 0, _ptr(t), _ptr(enc), None, _ptr(out))
    with pytest.raises(RuntimeError, match="image-to-video plan"):
        p_i._call("forward_train", p_i._h, _stream(), _ptr(lat), 0, _ptr(t), _ptr(enc), None, _ptr(out))
    with pytest.raises(RuntimeError, match="text-to-video plan"):
        p_t.transformer_forward(lat, t, enc, condition=cond)
    h = C.c_void_p()
    assert e_i.lib.mi355_wan_plan_create(e_i._h, 1, 1, 1, 4, 4, 8, 1, C.byref(h)) != 0 and b"plan_create_i2v" in e_i.lib.mi355_last_error()
    assert e_t.lib.mi355_wan_plan_create_i2v(e_t._h, 1, 1, 1, 4, 4, 8, 0, 1, C.byref(h)) != 0 and b"text-to-video engine" in e_t.lib.mi355_last_error()
    # bind, so that the remaining refusals are the ones under test
    for eng in (e_i, e_t):
        g = torch.Generator().manual_seed(1)
        shapes = {n: None for n in eng.param_names()}
        from oracle import wan_ref as R
        cfg_o = R.WanConfig(in_channels=36 if eng is e_i else 16, **small)
        eng.bind_state_dict({n: torch.randn(s, generator=g).cuda() * 0.02 for n, s in R.state_dict_shapes(cfg_o).items() if n in shapes})
        eng.ready()
    with pytest.raises(RuntimeError, match="no image cross-attention branch"):          # image_embeds on an engine without the branch
        p_i.transformer_forward(lat, t, enc, condition=cond, image_embeds=torch.zeros(1, 257, 1280).cuda())
    with pytest.raises(ValueError, match="needs `condition`"):
        p_i.transformer_forward(lat, t, enc)
    with pytest.raises(ValueError, match="condition has shape"):
        p_i.transformer_forward(lat, t, enc, condition=torch.ones(1, 20, 1, 4, 6).cuda())
    with pytest.raises(ValueError, match="condition has shape"):
        p_i.rollout([500.0], [0.5, 0.0], [0.0], "ODE", 1.0, lat, torch.float32, None, enc, condition=torch.ones(1, 16, 1, 4, 4).cuda())
    with pytest.raises(RuntimeError, match="elements in 5 dimensions, expected"):       # a T2V patch embedding does not bind into an I2V engine
        e_i.bind_tensor("patch_embedding.weight", torch.zeros(128, 16, 1, 2, 2).cuda())
    with pytest.raises(RuntimeError, match="no image cross-attention branch"):          # image tokens on an engine without the branch
        e_i.plan(1, 1, 1, 4, 4, 8, 1, n_image=257)
    assert e_i.lib.mi355_wan_create_i2v(C.byref(wn.WanConfig(**small).to_c()), 20, 1000, C.byref(h)) != 0 and b"image_dim" in e_i.lib.mi355_last_error()
    # an engine WITH the branch: its names are listed, a plan with image tokens needs them, one without refuses them; `pos_embed` is refused
    e_m = wn.WanEngine(wn.WanConfig(cond_channels=20, image_dim=128, **small))
    assert {"condition_embedder.image_embedder.norm1.weight", "condition_embedder.image_embedder.ff.net.0.proj.bias",
            "condition_embedder.image_embedder.ff.net.2.weight", "condition_embedder.image_embedder.norm2.bias", "blocks.0.attn2.add_k_proj.weight",
            "blocks.0.attn2.add_v_proj.bias", "blocks.0.attn2.norm_added_k.weight"} <= set(e_m.param_names())
    assert all(e_m.grad_supported(n) == 0 for n in e_m.param_names() if "image_embedder" in n or "add_" in n or n.startswith("patch_embedding"))
    img = torch.zeros(1, 5, 128).cuda()
    with pytest.raises(ValueError, match="created with n_image=5"):
        e_m.plan(1, 1, 1, 4, 4, 8, 1, n_image=5).transformer_forward(lat, t, enc, condition=cond)
    with pytest.raises(ValueError, match="created with n_image=5"):
        e_m.plan(1, 1, 1, 4, 4, 8, 1, n_image=5).transformer_forward(lat, t, enc, condition=cond, image_embeds=torch.zeros(1, 6, 128).cuda())
    with pytest.raises(RuntimeError, match="n_image == 0"):
        e_m.plan(1, 1, 1, 4, 4, 8, 1).transformer_forward(lat, t, enc, condition=cond, image_embeds=img)
    with pytest.raises(NotImplementedError, match="pos_embed"):
        e_m.bind_state_dict({"condition_embedder.image_embedder.pos_embed": torch.zeros(1, 514, 128)}, partial=True)
    with pytest.raises(RuntimeError, match="position embedding"):
        e_m.bind_tensor("condition_embedder.image_embedder.pos_embed", torch.zeros(1, 514, 128).cuda())
    e_m.close()
    # expand_timesteps (Wan2.2-TI2V-5B in I2V use), at construction and per call
    with pytest.raises(NotImplementedError, match="expand_timesteps"):
        wn.Wan2I2VNativeAdapter({}, wn.WanConfig(cond_channels=20, **small), expand_timesteps=True)
    mix = wn.WanI2VRolloutMixin()
    with pytest.raises(NotImplementedError, match="expand_timesteps"):
        mix.forward(t, lat, enc, condition=cond, first_frame_mask=torch.ones(1, 1, 1, 4, 4))
    e_i.close(); e_t.close()


def test_i2v_full_width_blocks_at_4608_tokens(wn):
    """Wan2.1-1.3B width (12 heads, ffn 8960, T5 width 4096) with the image branch at its real sizes (image_dim 1280, Ni 257, Nt 512), 2 blocks,
    4 x 48 x 96 latents = 4 608 tokens, B = 1 with CFG: `check_in_band` against the fp32 oracle."""
    from oracle import wan_ref as R
    from _gpu_oracle import check_in_band
    cfg_o = I.oracle_config(R, base=R.WanConfig(num_layers=2))
    sd, cfg = _setup(wn, cfg_o, seed=77, image_dim=1280)
    eng = _engine(wn, sd, cfg)
    B, T, h, w, Nt, Ni = 1, 4, 48, 96, 512, 257
    x, pe, ne, cond = _inputs(cfg_o, B, T, h, w, Nt, seed=5)
    ie = _image_embeds(B, Ni, seed=6, image_dim=1280)
    t = torch.tensor([601.0])
    got = eng.plan(B, 2, T, h, w, Nt, 1, n_image=Ni).transformer_forward(x.cuda(), t, ne.cuda(), pe.cuda(), condition=cond.cuda(), image_embeds=ie.cuda())
    pair = lambda sd_, x_, t_, ne_, pe_, c_, ie_, quant=None: _oracle_pair(R, sd_, cfg_o, x_, t_[:1], ne_, pe_, c_, 2, ie_, quant=quant)      # noqa: E731
    check_in_band("Wan I2V full-width 2 blocks, S = 4608, Ni 257, CFG pair", got, pair, sd, x.float(), t.expand(B), ne, pe, cond, ie)
    eng.close()


def test_i2v_40_head_width_block_at_1008_tokens(wn):
    """D = 5120 (40 heads: the real I2V-14B width, ffn 13 824), image_dim 1280, Ni 257, one block, 3 x 24 x 56 latents = 1 008 tokens, no CFG."""
    from oracle import wan_ref as R
    from _gpu_oracle import check_in_band
    cfg_o = I.oracle_config(R, base=R.WanConfig(num_layers=1, num_attention_heads=40, ffn_dim=13824))
    sd, cfg = _setup(wn, cfg_o, seed=78, image_dim=1280)
    eng = _engine(wn, sd, cfg)
    B, T, h, w, Nt, Ni = 1, 3, 24, 56, 226, 257
    x, pe, ne, cond = _inputs(cfg_o, B, T, h, w, Nt, seed=6)
    ie = _image_embeds(B, Ni, seed=7, image_dim=1280)
    t = torch.tensor([601.0])
    got = eng.plan(B, 1, T, h, w, Nt, 1, n_image=Ni).transformer_forward(x.cuda(), t, pe.cuda(), condition=cond.cuda(), image_embeds=ie.cuda())
    one = lambda sd_, x_, t_, pe_, c_, ie_, quant=None: I.forward(R, sd_, cfg_o, x_, t_, pe_, c_, image_embeds=ie_, quant=quant)      # noqa: E731
    check_in_band("Wan I2V 40-head width, 1 block, S = 1008, Ni 257", got, one, sd, x.float(), t.expand(B), pe, cond, ie)
    eng.close()

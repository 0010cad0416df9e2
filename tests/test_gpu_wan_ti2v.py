"""GPU parity of Wan2.2-TI2V-5B in image-to-video use (`expand_timesteps`; reference models/wan/wan2_i2v.py:547-652, :736-741): the first
latent frame replaced by the encoded image and one timestep per token -- 0 on the tokens of frame 0, t elsewhere -- through
mi355_wan_plan_create_ff and the `_ff` entry points, and `Wan2TI2VNativeAdapter` above them.  The oracle is `oracle.wan_ref.wan_forward` with its
`(B, S)` timestep on the merged input (tests/_wan_ti2v_ref.py; network body parity-unpinned), 48 latent channels on the tiny configuration.

Shapes: B = 2, T = 3, 6 x 10 latents: head_rows = 15, S = 45, M = 90 / 180 rows -- three sample boundaries and the splits inside one 128-row
GEMM tile; one case with T = 1 (every token is a head token), one without CFG.  The forward statement is `check_in_band`
(engine <= 1.5 x band + 1e-3), and the same test asserts that the fp32 oracle with the SCALAR timestep lies outside that region.
Rollout statements and tolerances are tests/test_gpu_wan_i2v.py's: per-step latents rel-L2 < 2e-2, log-probs rtol 1e-3."""
import pytest
import torch

import _wan_ti2v_ref as TI

pytestmark = pytest.mark.gpu

TOL = 2e-2
C = TI.C


@pytest.fixture(scope="module")
def wn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import wan
    return wan


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _engine(wn, sd, cfg):
    eng = wn.WanEngine(cfg)
    eng.bind_state_dict({k: v.cuda() for k, v in sd.items()})
    eng.ready()
    return eng


def _inputs(cfg_o, B, T, h, w, Nt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, T, h, w, generator=g).half()
    pe = TI.bf(torch.randn(B, Nt, cfg_o.text_dim, generator=g))
    ne = TI.bf(torch.randn(B, Nt, cfg_o.text_dim, generator=g))
    ff = TI.bf(torch.randn(B, C, 1, h, w, generator=g))
    return x, pe, ne, ff


def _fwd(plan, x, t, ne, pe, n_cfg, **kw):
    if n_cfg == 2:
        return plan.transformer_forward(x.cuda(), t, ne.cuda(), pe.cuda(), **kw)
    return plan.transformer_forward(x.cuda(), t, pe.cuda(), **kw)


@pytest.mark.parametrize("B,T,h,w,Nt,n_cfg,ffdt", [(2, 3, 6, 10, 9, 2, torch.float32), (2, 1, 6, 10, 9, 2, torch.bfloat16),
                                                   (2, 3, 6, 10, 9, 1, torch.float16)])
def test_ti2v_forward_matches_the_per_token_oracle_and_not_the_scalar_one(wn, B, T, h, w, Nt, n_cfg, ffdt):
    from oracle import wan_ref as R
    from _gpu_oracle import check_in_band, ref_on_gpu, rel
    cfg_o = TI.oracle_config(R)
    sd = TI.make_state_dict(R, cfg_o, 61)
    eng = _engine(wn, sd, TI.engine_config(wn, cfg_o))
    x, pe, ne, ff = _inputs(cfg_o, B, T, h, w, Nt, seed=T * h + w + Nt + n_cfg)
    ff = ff.to(ffdt).float()          # representable in the dtype it is handed over in
    t = torch.tensor([874.0])
    plan = eng.plan(B, n_cfg, T, h, w, Nt, 1, first_frame=True)
    got = _fwd(plan, x, t, ne, pe, n_cfg, first_frame=ff.to(ffdt).cuda())
    assert got.shape == (B * n_cfg, C, T, h, w)
    fn = lambda sd_, x_, t_, ne_, pe_, ff_, quant=None, per_token=True: TI.pair(R, sd_, cfg_o, x_, t_, ne_, pe_, ff_, n_cfg, quant=quant,      # noqa: E731
                                                                               per_token=per_token)
    ref, _, r, band = check_in_band(f"Wan TI2V forward ({B}, {T}x{h}x{w}, n_cfg {n_cfg}, first frame {ffdt})", got, fn, sd, x.float(), t, ne, pe, ff)
    # the same input with ONE timestep per sample -- what the engine computed before it had the two-group modulation -- is not accepted
    scalar = ref_on_gpu(fn, sd, x.float(), t, ne, pe, ff, per_token=False)
    away = rel(scalar, ref)
    print(f"  fp32 oracle with the scalar timestep vs the per-token one: {away:.3e} (acceptance region {1.5 * band + 1e-3:.3e})")
    assert away > 1.5 * band + 1e-3, (away, band)
    eng.close()


def test_ti2v_equal_timesteps_and_own_first_frame_is_the_t2v_forward_bit_for_bit(wn):
    """`forward_ff` with t_head == t_rest and first_frame == latents[:, :, :1] computes what `mi355_wan_forward` computes: the split kernels
    read two equal rows, the merge rewrites frame 0 with itself."""
    from oracle import wan_ref as R
    cfg_o = TI.oracle_config(R)
    eng = _engine(wn, TI.make_state_dict(R, cfg_o, 62), TI.engine_config(wn, cfg_o))
    B, T, h, w, Nt = 2, 3, 6, 10, 9
    x, pe, ne, _ = _inputs(cfg_o, B, T, h, w, Nt, seed=3)
    for n_cfg in (2, 1):
        t = torch.tensor([611.0])
        a = _fwd(eng.plan(B, n_cfg, T, h, w, Nt, 1), x, t, ne, pe, n_cfg)
        b = _fwd(eng.plan(B, n_cfg, T, h, w, Nt, 1, first_frame=True), x, torch.tensor([[611.0, 611.0]]), ne, pe, n_cfg,
                 first_frame=x[:, :, :1].contiguous().cuda(), t_pairs=True)
        assert torch.equal(a, b), n_cfg
    eng.close()


def test_ti2v_each_first_frame_reaches_its_own_sample_only(wn):
    from oracle import wan_ref as R
    cfg_o = TI.oracle_config(R)
    eng = _engine(wn, TI.make_state_dict(R, cfg_o, 63), TI.engine_config(wn, cfg_o))
    B, T, h, w, Nt = 2, 3, 6, 10, 9
    x, pe, ne, ff = _inputs(cfg_o, B, T, h, w, Nt, seed=4)
    plan = eng.plan(B, 2, T, h, w, Nt, 1, first_frame=True)
    t = torch.tensor([874.0])
    a = _fwd(plan, x, t, ne, pe, 2, first_frame=ff.cuda()).clone()
    ff2 = ff.clone()
    ff2[1] = TI.bf(torch.randn(C, 1, h, w, generator=torch.Generator().manual_seed(9)))
    b = _fwd(plan, x, t, ne, pe, 2, first_frame=ff2.cuda())
    for row in (0, B):          # sample 0 in both CFG halves: untouched, bit for bit
        assert torch.equal(a[row], b[row]), row
    for row in (1, B + 1):      # sample 1 in both halves: moved, and not only in frame 0 (attention mixes the frames)
        assert _rel(b[row], a[row]) > 5 * TOL and not torch.equal(a[row][:, 1:], b[row][:, 1:]), row
    # the latents' own frame 0 is never read
    x2 = x.clone()
    x2[:, :, 0] = 7.0
    assert torch.equal(_fwd(plan, x2, t, ne, pe, 2, first_frame=ff.cuda()), a)
    eng.close()


@pytest.mark.parametrize("ffdt", [torch.float32, torch.bfloat16, torch.float16])
def test_ti2v_patch_merge_is_exact(wn, ffdt):
    """A first-frame plan at equal timesteps, fed latents with a garbage frame 0 and a first frame of dtype `ffdt`, computes bit for bit what the
    text-to-video plan computes on the tensor merged on the host: the merge writes the same bf16 the patchify would."""
    from oracle import wan_ref as R
    cfg_o = TI.oracle_config(R)
    eng = _engine(wn, TI.make_state_dict(R, cfg_o, 64), TI.engine_config(wn, cfg_o))
    B, T, h, w, Nt = 2, 3, 6, 10, 9
    x, pe, ne, _ = _inputs(cfg_o, B, T, h, w, Nt, seed=5)
    ff = (3.0 * torch.randn(B, C, 1, h, w, generator=torch.Generator().manual_seed(6)) + 0.5).to(ffdt)      # NOT bf16-representable in fp32 / fp16
    host = torch.cat([ff.float(), x.float()[:, :, 1:]], 2)          # fp32 holds both dtypes exactly
    a = _fwd(eng.plan(B, 2, T, h, w, Nt, 1), host, torch.tensor([611.0]), ne, pe, 2)
    xg = x.clone()
    xg[:, :, 0] = -11.0
    b = _fwd(eng.plan(B, 2, T, h, w, Nt, 1, first_frame=True), xg, torch.tensor([[611.0, 611.0]]), ne, pe, 2, first_frame=ff.cuda(), t_pairs=True)
    assert torch.equal(a, b)
    eng.close()


# ------------------------------------------------------------------------------------------------- the standalone adapter
class _Decode:
    """`video_decode` stand-in: keeps what the adapter hands to the decoder"""

    def __init__(self):
        self.seen = None

    def __call__(self, latents):
        self.seen = latents.clone()
        return None


def _adapter(wn, sd, cfg, sched, **kw):
    dec = _Decode()
    ad = wn.Wan2TI2VNativeAdapter({k: v.cuda() for k, v in sd.items()}, cfg, sched, latent_storage_dtype="fp16", video_decode=dec, **kw)
    ad.rollout()
    return ad, dec


def test_ti2v_rollout_matches_oracle_replays_and_refreshes_the_first_frame(wn):
    """N = 4 Flow-SDE with CFG against the oracle loop (`oracle.wan_ref.rollout`: its scheduler step on the unmerged latents, the network on
    the merged input with per-token timesteps); fused == step-wise bit for bit; the `forward()` replay of a stored transition returns the
    rollout's log-prob exactly; the decoder receives the merged latents; a second rollout with another first frame gives that frame's result."""
    from oracle import wan_ref as R
    cfg_o = TI.oracle_config(R)
    sd = TI.make_state_dict(R, cfg_o, 12)
    sched = wn.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[0, 1, 2, 3], num_sde_steps=2, seed=42, dynamics_type="Flow-SDE")
    ad, dec = _adapter(wn, sd, TI.engine_config(wn, cfg_o), sched)
    B, Nt, N, guidance = 2, 12, 4, 5.0
    T, h, w = 3, 6, 10
    H, W, frames = h * 16, w * 16, 9
    g = torch.Generator().manual_seed(4)
    pe = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    ne = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    ff_a, ff_b = (TI.bf(torch.randn(B, C, 1, h, w, generator=g)) for _ in range(2))
    kw = dict(prompt=["a", "b"], height=H, width=W, num_frames=frames, num_inference_steps=N, guidance_scale=guidance, prompt_embeds=pe.cuda(),
              negative_prompt_embeds=ne.cuda(), compute_log_prob=True, trajectory_indices="all")

    def run(ff, **more):
        torch.cuda.manual_seed(31)
        return ad.inference(condition=ff.cuda(), **kw, **more)

    s_a = run(ff_a)
    seen_a = dec.seen
    torch.cuda.manual_seed(31)          # RNG order of the reference: prepare_latents draws the fp32 latents first, then one fp32 draw per step
    init = torch.randn((B, C, T, h, w), device="cuda", dtype=torch.float32).cpu()
    noise = torch.stack([torch.randn((B, C, T, h, w), device="cuda", dtype=torch.float32) for _ in range(N)]).cpu()
    ts, sig = R.unipc_flow_schedule(N, 3.0)
    nl = ad.scheduler.host_noise_levels()
    sde = [i for i in range(N) if nl[i] > 0]
    assert len(sde) == 2
    mask = TI.first_frame_mask(T, h, w)

    def check(samples, ff, seen):
        with TI.with_first_frame(R, cfg_o, ff):
            ref = R.rollout(sd, cfg_o, pe, ne, guidance, init, noise, ts, sig, nl, torch.float16)
        for b in range(B):
            got = samples[b].all_latents.float().cpu()
            assert got.shape == (N + 1, C, T, h, w)
            for pos in range(N + 1):
                assert _rel(got[pos], ref["all_latents"][pos, b]) < TOL, (b, pos)
            torch.testing.assert_close(samples[b].log_probs.cpu(), torch.stack([ref["log_probs"][i, b] for i in sde]), rtol=1e-3, atol=1e-4)
            assert torch.equal(samples[b].condition.cpu(), ff[b]) and samples[b].image_embeds is None
            assert torch.equal(samples[b].first_frame_mask.cpu(), mask) and samples[b].first_frame_mask.dtype == torch.float32
            # the scheduler steps frame 0 like every other frame (the reference's does): the stored latents do NOT carry the condition there ...
            assert not torch.equal(got[N][:, 0], ff[b][:, 0])
            # ... and what goes to the decoder does: (1 - mask) * condition + mask * latents
            assert torch.equal(seen[b, :, 0].cpu(), ff[b][:, 0]) and torch.equal(seen[b, :, 1:].cpu(), got[N][:, 1:])

    check(s_a, ff_a, seen_a)
    # replay of a stored transition: the rollout's log-prob, bit for bit
    i = sde[0]
    x_i = torch.stack([s.all_latents[i] for s in s_a]).cuda()
    x_n = torch.stack([s.all_latents[i + 1] for s in s_a]).cuda()
    out = ad.forward(t=s_a[0].timesteps[i].reshape(1).expand(B).cuda(), latents=x_i, prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(),
                     guidance_scale=guidance, condition=torch.stack([s.condition for s in s_a]), first_frame_mask=s_a[0].first_frame_mask,
                     t_next=s_a[0].timesteps[i + 1].reshape(1).expand(B).cuda(), next_latents=x_n, noise_level=nl[i], compute_log_prob=True,
                     return_kwargs=["log_prob"])
    assert torch.equal(out.log_prob, torch.stack([s.log_probs[0] for s in s_a]).cuda())
    # fused == step-wise
    s_step = run(ff_a, extra_call_back_kwargs=["noise_pred"])
    for sa, sb in zip(s_a, s_step):
        assert torch.equal(sa.all_latents, sb.all_latents) and torch.equal(sa.log_probs, sb.log_probs)
    # another first frame on the same plan, then the first again
    s_b = run(ff_b)
    check(s_b, ff_b, dec.seen)
    assert not torch.equal(s_b[0].all_latents[1], s_a[0].all_latents[1])
    s_a2 = run(ff_a)
    for sa, sb in zip(s_a, s_a2):
        assert torch.equal(sa.all_latents, sb.all_latents) and torch.equal(sa.log_probs, sb.log_probs)
    ad.engine.close()


def test_ti2v_evaluation_mode_sampling_matches_oracle(wn):
    """Evaluation mode (UniPC predictor-corrector) with CFG against `oracle.wan_ref.rollout_eval` on the merged input / per-token timesteps."""
    from oracle import wan_ref as R
    cfg_o = TI.oracle_config(R)
    sd = TI.make_state_dict(R, cfg_o, 21)
    sched = wn.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[0, 1, 2], num_sde_steps=2, seed=42, dynamics_type="Flow-SDE")
    ad, dec = _adapter(wn, sd, TI.engine_config(wn, cfg_o), sched)
    ad.eval()
    B, Nt, N, guidance = 2, 12, 4, 4.0
    T, h, w = 3, 6, 10
    g = torch.Generator().manual_seed(4)
    pe = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    ne = torch.randn(B, Nt, cfg_o.text_dim, generator=g).bfloat16()
    ff = TI.bf(torch.randn(B, C, 1, h, w, generator=g))
    torch.cuda.manual_seed(31)
    samples = ad.inference(condition=ff.cuda(), prompt=["a", "b"], height=h * 16, width=w * 16, num_frames=9, num_inference_steps=N,
                           guidance_scale=guidance, prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), compute_log_prob=False,
                           trajectory_indices="all")
    torch.cuda.manual_seed(31)
    init = torch.randn((B, C, T, h, w), device="cuda", dtype=torch.float32).cpu()
    ts, sig = R.unipc_flow_schedule(N, 3.0)
    with TI.with_first_frame(R, cfg_o, ff):
        ref = R.rollout_eval(sd, cfg_o, pe, ne, guidance, init, ts, sig, torch.float16)
    worst = max(_rel(samples[b].all_latents[pos].cpu(), ref["all_latents"][pos, b]) for b in range(B) for pos in range(1, N + 1))
    print(f"Wan TI2V evaluation-mode sampling: worst latent rel-L2 vs the oracle loop {worst:.3e}")
    assert worst < TOL and samples[0].log_probs is None
    assert torch.equal(dec.seen[:, :, 0].cpu(), ff[:, :, 0])
    ad.engine.close()


def test_ti2v_errors(wn):
    import ctypes as Ct
    from mi355_flow.engine import _ptr, _stream
    small = dict(num_layers=1, num_attention_heads=1, ffn_dim=128, text_dim=64)
    e_t = wn.WanEngine(wn.WanConfig(**small))
    e_i = wn.WanEngine(wn.WanConfig(cond_channels=20, **small))
    lat, t, enc = torch.zeros(1, 16, 1, 4, 4).cuda(), torch.tensor([500.0]).cuda(), torch.zeros(1, 8, 64).cuda().bfloat16()
    ff, out = torch.ones(1, 16, 1, 4, 4).cuda(), torch.empty(1, 16, 1, 4, 4, dtype=torch.bfloat16).cuda()
    p_t, p_f, p_i = e_t.plan(1, 1, 1, 4, 4, 8, 1), e_t.plan(1, 1, 1, 4, 4, 8, 1, first_frame=True), e_i.plan(1, 1, 1, 4, 4, 8, 1)
    assert p_t is not p_f and p_f.first_frame and not p_t.first_frame
    shape, sched = (1, 16, 1, 4, 4), ([500.0], [0.5, 0.0], [0.0], "ODE", 1.0, lat, torch.float32, None)
    # a plain call on a first-frame plan: an error that names the `_ff` entry point, nothing runs (the weights are not even bound)
    for sym in ("forward", "forward_train"):
        with pytest.raises(RuntimeError, match=f"first-frame plan.*mi355_wan_{sym}_ff"):
            p_f._call(sym, p_f._h, _stream(), _ptr(lat), 0, _ptr(t), _ptr(enc), None, _ptr(out))
    with pytest.raises(RuntimeError, match="first-frame plan.*mi355_wan_rollout_ff"):
        p_f._rollout(shape, *sched, (_ptr(enc), None), None, False)
    # the `_ff` entry points on the other two kinds
    with pytest.raises(RuntimeError, match="text-to-video plan: use mi355_wan_forward "):
        p_t.transformer_forward(lat, t, enc, first_frame=ff)
    with pytest.raises(RuntimeError, match="text-to-video plan: use mi355_wan_forward_train "):
        p_t.forward_train(lat, t, enc, first_frame=ff)
    with pytest.raises(RuntimeError, match="text-to-video plan: use mi355_wan_rollout "):
        p_t.rollout(*sched, enc, first_frame=ff)
    with pytest.raises(RuntimeError, match="image-to-video plan: use mi355_wan_forward_i2v"):
        p_i.transformer_forward(lat, t, enc, first_frame=ff)
    h = Ct.c_void_p()
    assert e_i.lib.mi355_wan_plan_create_ff(e_i._h, 1, 1, 1, 4, 4, 8, 1, Ct.byref(h)) != 0 and b"plan_create_i2v" in e_i.lib.mi355_last_error()
    with pytest.raises(ValueError, match="text-to-video engine"):
        e_i.plan(1, 1, 1, 4, 4, 8, 1, first_frame=True)
    # host-side checks of a first-frame plan
    with pytest.raises(ValueError, match="needs `first_frame`"):
        p_f.transformer_forward(lat, t, enc)
    with pytest.raises(ValueError, match="first_frame has shape"):
        p_f.transformer_forward(lat, t, enc, first_frame=torch.ones(1, 16, 2, 4, 4).cuda())
    with pytest.raises(ValueError, match="first_frame has shape"):
        p_f.rollout(*sched, enc, first_frame=torch.ones(1, 16, 1, 4, 6).cuda())
    with pytest.raises(ValueError, match="does not go together"):
        p_f.transformer_forward(lat, t, enc, first_frame=ff, condition=torch.ones(1, 20, 1, 4, 4).cuda())
    assert e_t.lib.mi355_wan_forward_ff(p_f._h, None, _ptr(lat), 0, _ptr(t), _ptr(enc), None, None, 0, _ptr(out)) != 0
    assert b"first_frame is NULL" in e_t.lib.mi355_last_error()
    assert e_t.lib.mi355_wan_forward_ff(p_f._h, None, _ptr(lat), 0, _ptr(t), _ptr(enc), None, _ptr(ff), 7, _ptr(out)) != 0
    assert b"first_frame dtype" in e_t.lib.mi355_last_error()
    # the mixin: only the reference's own mask, and the first frame is required
    mix = wn.WanTI2VRolloutMixin()
    lat3 = torch.zeros(1, 16, 3, 4, 4).cuda()
    good = wn.wan_first_frame_mask(3, 4, 4, device="cuda")
    with pytest.raises(ValueError, match="needs `condition`"):
        mix.forward(t, lat3, enc, first_frame_mask=good)
    with pytest.raises(ValueError, match="needs `first_frame_mask`"):
        mix.forward(t, lat3, enc, condition=ff)
    bad_value, bad_frame = good.clone(), torch.ones_like(good)
    bad_value[:, :, 1, 0, 0] = 0.5
    bad_frame[:, :, 1] = 0
    for bad in (good[:, :, :2], good.expand(1, 16, 3, 4, 4), bad_value, bad_frame, torch.ones_like(good)):
        with pytest.raises(ValueError, match="first_frame_mask"):
            mix.forward(t, lat3, enc, condition=ff, first_frame_mask=bad)
    with pytest.raises(ValueError, match="condition .* has shape"):
        mix.forward(t, lat3, enc, condition=torch.ones(1, 16, 3, 4, 4).cuda(), first_frame_mask=good)
    with pytest.raises(ValueError, match="text-to-video config"):
        wn.Wan2TI2VNativeAdapter({}, wn.WanConfig(cond_channels=20, **small))
    with pytest.raises(NotImplementedError, match="two experts"):
        wn.Wan2TI2VNativeAdapter({}, wn.WanConfig(**small), state_dict_2={})
    # the condition-channel classes keep refusing, and name the class that serves these pipelines
    with pytest.raises(NotImplementedError, match="expand_timesteps.*Wan2TI2VNativeAdapter"):
        wn.Wan2I2VNativeAdapter({}, wn.WanConfig(cond_channels=20, **small), expand_timesteps=True)
    e_t.close(); e_i.close()


def test_ti2v_full_width_blocks_at_4000_tokens(wn):
    """Wan2.2-TI2V-5B width (D = 3072: 24 heads, ffn 14336, 48 channels, T5 width 4096), 2 blocks, 5 x 40 x 80 latents = 4 000 tokens of which
    800 are head tokens, B = 1 with CFG: `check_in_band` against the fp32 oracle with per-token timesteps."""
    from oracle import wan_ref as R
    from _gpu_oracle import check_in_band
    cfg_o = TI.oracle_config(R, base=R.WanConfig(num_layers=2, num_attention_heads=24, ffn_dim=14336))
    sd = TI.make_state_dict(R, cfg_o, 77)
    eng = _engine(wn, sd, TI.engine_config(wn, cfg_o))
    B, T, h, w, Nt = 1, 5, 40, 80, 128
    x, pe, ne, ff = _inputs(cfg_o, B, T, h, w, Nt, seed=5)
    t = torch.tensor([601.0])
    got = eng.plan(B, 2, T, h, w, Nt, 1, first_frame=True).transformer_forward(x.cuda(), t, ne.cuda(), pe.cuda(), first_frame=ff.cuda())
    fn = lambda sd_, x_, t_, ne_, pe_, ff_, quant=None: TI.pair(R, sd_, cfg_o, x_, t_, ne_, pe_, ff_, 2, quant=quant)      # noqa: E731
    check_in_band("Wan TI2V full-width 2 blocks, S = 4000, head_rows 800, CFG pair", got, fn, sd, x.float(), t, ne, pe, ff)
    eng.close()

"""Operator-level tests of the fused scheduler step (csrc/sde_step.hip) and of its adjoint (sde_step_bwd_kernel, csrc/backward.hip), through
`mi355_flow.engine.sde_step` / `sde_step_bwd` and, for the write extent, through the raw C ABI.

The reference is tests/_sde_ref.py (plain torch on the CPU; pinned by tests/test_sde_ref.py): fp32 for the forward, fp64 autograd for the adjoint.

Shapes (B = 3 everywhere): the step runs 64 workgroups per sample, each on `roundup4(ceil(n / 64))` consecutive elements, 4 per thread and loop
iteration, on a vector path when n % 4 == 0 and on a scalar path otherwise.
    n = 4       one thread, 63 empty workgroups
    n = 6       scalar path, a tail of 2, bf16 / fp16 sample bases at 12-byte offsets
    n = 260     vector path, 33 non-empty chunks of 8, 31 empty ones
    n = 65796   vector path, 1032 elements per chunk: threads 0 and 1 take a second loop iteration; short last chunk of 780
    n = 65798   the same on the scalar path; above 65536 = 256 x 256, so the adjoint's grid-stride loop runs
Per-sample scalars: sample 0 has sigma == 1 (Flow-SDE substitutes sigma_max in the denominator); every reference log-prob is finite and
sigma_next^2 - std^2 > 0 for CPS (asserted in tests/test_sde_ref.py).

FORWARD tolerances are the project's own (tests/test_gpu_kernels.py::test_sde_step_matches_reference_fixtures, the kernel's header): ODE,
Flow-SDE and Dance-SDE bit-equal; CPS rtol 1e-6 with atol 1e-6 (fp32 storage) / 8e-3 (half storage: sin differs by an ulp between host and
device); log-prob rtol 2e-6 up to n = 260 and 1e-5 (reduction order, test_sde_step_cfg_and_large) at the two large n.

ADJOINT bound: per output row, e = max |dv - dv64| / max |dv64| must not exceed 8 E, E = the same figure for the fp32 CPU reference adjoint
of the same case.  The kernel and the fp32 reference do the same arithmetic in fp32 and differ in operation order and contraction only.
`pytest -s` prints e and E of every case before it asserts.

Observed on MI355X over the 894 output rows of the adjoint tests: E (non-zero) 8.0e-09 .. 4.9e-06, e 7.8e-09 .. 5.2e-06, largest e / E 2.7
(Dance-SDE, n = 6).  E is exactly 0 for 72 rows (a g_noise_pred-only gradient without CFG is a copy), and so is e there.  The large figures
are CPS sample 2 with a log-prob gradient: sigma_next^2 - std^2 = 9.3e-5 cancels a decimal digit, in the fp32 reference and in the kernel
alike (e / E <= 1.5), so the adjoint's `sinf` and clamped square root sit inside the bound.  Forward log-prob: largest relative error
7.5e-07 up to n = 260 (rtol 2e-6) and 1.2e-06 at the large n (rtol 1e-5).
"""
import functools

import numpy as np
import pytest
import torch

import _sde_ref
from oracle import scheduler_ref

pytestmark = pytest.mark.gpu

B = 3
SIGMA = (1.0, 0.875, 0.25)
SIGMA_NEXT = (0.9642857, 0.8181818, 0.03125)
ETA = (0.7, 0.35, 0.8)
SIGMA_MAX = 0.9642857
G = 4.5
NS = (4, 6, 260, 65796, 65798)
DYNS = scheduler_ref.DYNAMICS
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SENT = 776.0          # exact in bf16, fp16 and fp32
GUARD = 64
ADJ_FACTOR = 8.0


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import engine
    return engine


def _t(values):
    return torch.tensor(values, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """CPU inputs of one size, shared by every test and never modified"""
    g = torch.Generator().manual_seed(5000 + n)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(lat=r(B, n), vt=r(B, n).bfloat16(), vu=r(B, n).bfloat16(), eps=r(B, n), vt32=r(B, n), vu32=r(B, n),
                g_lp=r(B), g_np=r(B, n), g_mean=r(B, n))


@functools.lru_cache(maxsize=None)
def _scalars_gpu():
    return _t(SIGMA).cuda(), _t(SIGMA_NEXT).cuda(), _t(ETA).cuda()


@functools.lru_cache(maxsize=None)
def _forward_ref(dyn, sd, n):
    """fp32 CPU reference of the plain case (bf16 prediction, no CFG, noise given)"""
    i = _inputs(n)
    return _sde_ref.sde_step(i["vt"], i["lat"].to(DT[sd]), _t(SIGMA), _t(SIGMA_NEXT), _t(ETA), dyn, SIGMA_MAX, noise=i["eps"])


def _lp_rtol(n):
    return 2e-6 if n <= 260 else 1e-5


def _check_forward(o, ref, dyn, sd, n, tag):
    if dyn == "CPS":
        cmp = lambda a, b, w: np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 if sd == "fp32" else 8e-3, err_msg=str(tag + (w,)))
    else:
        cmp = lambda a, b, w: np.testing.assert_array_equal(a, b, err_msg=str(tag + (w,)))
    npy = lambda t: t.detach().float().cpu().numpy()
    assert torch.equal(o.noise_pred.cpu(), ref["noise_pred"].float()), tag          # the prediction does not depend on sin: always exact
    cmp(npy(o.next_latents_mean), npy(ref["next_latents_mean"]), "mean")
    cmp(npy(o.next_latents), npy(ref["next_latents"]), "next_latents")
    # storage-dtype copy: the ODE branch returns the unrounded mean and lets cast_latents round it, the SDE branches round inside the step
    cmp(npy(o.next_storage), npy(scheduler_ref.cast_latents(ref["next_latents"], DT[sd])), "next_storage")
    assert o.next_storage.dtype == DT[sd]
    cmp(npy(o.std_dev_t), npy(ref["std_dev_t"]), "std_dev_t")
    assert torch.equal(o.dt.cpu(), ref["dt"]), tag
    got, want = npy(o.log_prob).astype(np.float64), npy(ref["log_prob"]).astype(np.float64)
    assert np.isfinite(want).all(), tag
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.abs(got - want))
    print(f"[log_prob] {tag}: ref {want.tolist()} rel err {rel.tolist()} (rtol {_lp_rtol(n):g})")
    np.testing.assert_allclose(got, want, rtol=_lp_rtol(n), err_msg=str(tag))


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("sd", list(DT))
@pytest.mark.parametrize("dyn", DYNS)
def test_forward_grid(eng, dyn, sd, n):
    i = _inputs(n)
    sig, sig_n, eta = _scalars_gpu()
    o = eng.sde_step(i["vt"].cuda(), None, 1.0, i["lat"].to(DT[sd]).cuda(), sig, sig_n, eta, SIGMA_MAX, dyn, noise=i["eps"].cuda())
    torch.cuda.synchronize()
    _check_forward(o, _forward_ref(dyn, sd, n), dyn, sd, n, (dyn, sd, n))


def _cfg_cpu(vu, vt):
    """torch's own op-by-op combine in the tensors' dtype (sd3_5.py:431-433)"""
    return vu + G * (vt - vu)


@pytest.mark.parametrize("n", [260, 65798])
@pytest.mark.parametrize("dyn", ["Flow-SDE", "CPS"])
@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("vd", ["fp32", "fp16"])
def test_prediction_dtypes(eng, vd, cfg, dyn, n):
    """fp32 / fp16 predictions of standalone scheduler.step() callers are read exactly and combined op by op in their own dtype"""
    i = _inputs(n)
    sd = "bf16"
    vt, vu = i["vt32"].to(DT[vd]), (i["vu32"].to(DT[vd]) if cfg else None)
    v = _cfg_cpu(vu, vt) if cfg else vt
    assert v.dtype == DT[vd]
    lat = i["lat"].to(DT[sd])
    sig, sig_n, eta = _scalars_gpu()
    o = eng.sde_step(vt.cuda(), vu.cuda() if cfg else None, G, lat.cuda(), sig, sig_n, eta, SIGMA_MAX, dyn, noise=i["eps"].cuda())
    torch.cuda.synchronize()
    assert torch.equal(o.noise_pred.cpu(), v.float()), (vd, cfg, dyn, n)
    ref = _sde_ref.sde_step(v, lat, _t(SIGMA), _t(SIGMA_NEXT), _t(ETA), dyn, SIGMA_MAX, noise=i["eps"])
    _check_forward(o, ref, dyn, sd, n, (vd, cfg, dyn, n))


@pytest.mark.parametrize("n", [260, 65798])
@pytest.mark.parametrize("sd", ["fp32", "bf16"])
@pytest.mark.parametrize("dyn", ["Dance-SDE", "CPS", "ODE"])
def test_cfg_bf16_on_the_other_dynamics(eng, dyn, sd, n):
    """(Flow-SDE with CFG: tests/test_gpu_kernels.py::test_sde_step_cfg_and_large)"""
    i = _inputs(n)
    v = _cfg_cpu(i["vu"], i["vt"])
    assert v.dtype == torch.bfloat16
    lat = i["lat"].to(DT[sd])
    sig, sig_n, eta = _scalars_gpu()
    o = eng.sde_step(i["vt"].cuda(), i["vu"].cuda(), G, lat.cuda(), sig, sig_n, eta, SIGMA_MAX, dyn, noise=i["eps"].cuda())
    torch.cuda.synchronize()
    ref = _sde_ref.sde_step(v, lat, _t(SIGMA), _t(SIGMA_NEXT), _t(ETA), dyn, SIGMA_MAX, noise=i["eps"])
    _check_forward(o, ref, dyn, sd, n, ("cfg", dyn, sd, n))


@pytest.mark.parametrize("n", [65796, 65798])
@pytest.mark.parametrize("sd", list(DT))
@pytest.mark.parametrize("dyn", DYNS)
def test_replay_reproduces_the_rollout_log_prob_bit_for_bit(eng, dyn, sd, n):
    """ratio == 1: the replay of a stored step gives the rollout's log-prob, from the storage-dtype copy and from the fp32 value-rounded one"""
    i = _inputs(n)
    vt, lat, eps = i["vt"].cuda(), i["lat"].to(DT[sd]).cuda(), i["eps"].cuda()
    sig, sig_n, eta = _scalars_gpu()
    o = eng.sde_step(vt, None, 1.0, lat, sig, sig_n, eta, SIGMA_MAX, dyn, noise=eps)
    assert o.next_storage.dtype == DT[sd] and o.next_latents.dtype == torch.float32
    o_st = eng.sde_step(vt, None, 1.0, lat, sig, sig_n, eta, SIGMA_MAX, dyn, next_latents=o.next_storage)
    o_32 = eng.sde_step(vt, None, 1.0, lat, sig, sig_n, eta, SIGMA_MAX, dyn, next_latents=o.next_latents)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.log_prob).all())
    assert torch.equal(o_st.log_prob, o.log_prob), (dyn, sd, n, o.log_prob.tolist(), o_st.log_prob.tolist())
    assert torch.equal(o_32.log_prob, o.log_prob), (dyn, sd, n, o.log_prob.tolist(), o_32.log_prob.tolist())
    # a replay hands the provided next state through untouched
    assert torch.equal(o_st.next_storage, o.next_storage) and torch.equal(o_32.next_latents, o.next_latents)
    np.testing.assert_allclose(o.log_prob.cpu().numpy(), _forward_ref(dyn, sd, n)["log_prob"].numpy(), rtol=_lp_rtol(n))


# ------------------------------------------------------------------------------------------------- write extent (raw C ABI)
def _sent(count, dtype):
    return torch.full((count + GUARD,), SENT, device="cuda", dtype=dtype)


@pytest.mark.parametrize("n", [6, 65798])
@pytest.mark.parametrize("sd", list(DT))
def test_write_extent_of_the_step_and_its_adjoint(eng, sd, n):
    from mi355_flow import _lib
    from mi355_flow.engine import dtype_code
    lib = _lib.load()
    i = _inputs(n)
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    vt, vu, lat, eps = i["vt"].cuda(), i["vu"].cuda(), i["lat"].to(DT[sd]).cuda(), i["eps"].cuda()
    sig, sig_n, eta = _scalars_gpu()
    nxt, nxt32, mean, npred = _sent(B * n, DT[sd]), _sent(B * n, torch.float32), _sent(B * n, torch.float32), _sent(B * n, torch.float32)
    lp, std, dt = _sent(B, torch.float32), _sent(B, torch.float32), _sent(B, torch.float32)
    dyn = "Flow-SDE"
    _lib.check(lib.mi355_sde_step(st, B, n, p(vt), p(vu), _lib.BF16, G, p(lat), dtype_code(DT[sd]), p(eps), None, 0, p(sig), p(sig_n), p(eta), 1,
                                  SIGMA_MAX, _lib.DYNAMICS[dyn], 1, p(nxt), p(nxt32), p(mean), p(npred), p(lp), p(std), p(dt)), "sde_step")
    torch.cuda.synchronize()
    for name, buf, count in (("next_out", nxt, B * n), ("next_f32", nxt32, B * n), ("mean_out", mean, B * n), ("noise_pred_out", npred, B * n),
                             ("log_prob", lp, B), ("std_dev_t", std, B), ("dt", dt, B)):
        assert bool((buf[count:] == SENT).all()), (name, sd, n)
    # ... and everything inside the extent was written: the same values as through the wrapper
    o = eng.sde_step(vt, vu, G, lat, sig, sig_n, eta, SIGMA_MAX, dyn, noise=eps)
    torch.cuda.synchronize()
    for name, buf, want in (("next_out", nxt, o.next_storage), ("next_f32", nxt32, o.next_latents), ("mean_out", mean, o.next_latents_mean),
                            ("noise_pred_out", npred, o.noise_pred), ("log_prob", lp, o.log_prob), ("std_dev_t", std, o.std_dev_t), ("dt", dt, o.dt)):
        assert torch.equal(buf[:want.numel()], want.reshape(-1)), (name, sd, n)

    g_lp, g_np, g_mean = i["g_lp"].cuda(), i["g_np"].cuda(), i["g_mean"].cuda()
    for cfg in (False, True):
        rows = (2 if cfg else 1) * B
        dv = _sent(2 * B * n, torch.float32)
        _lib.check(lib.mi355_sde_step_bwd(st, B, n, p(vt), p(vu) if cfg else None, G, p(lat), dtype_code(DT[sd]), p(nxt), dtype_code(DT[sd]), p(sig),
                                          p(sig_n), p(eta), 1, SIGMA_MAX, _lib.DYNAMICS[dyn], 1, p(g_lp), p(g_np), p(g_mean), p(dv)), "sde_step_bwd")
        torch.cuda.synchronize()
        assert bool((dv[rows * n:] == SENT).all()), ("dv", cfg, sd, n)
        want = eng.sde_step_bwd(vt, vu if cfg else None, G, lat, nxt[:B * n].view(B, n), sig, sig_n, eta, SIGMA_MAX, dyn, True,
                                g_log_prob=g_lp, g_noise_pred=g_np, g_mean=g_mean)
        torch.cuda.synchronize()
        assert torch.equal(dv[:rows * n], want.reshape(-1)), ("dv", cfg, sd, n)


# ------------------------------------------------------------------------------------------------- tickets and the scratch ring
RING_N = 65796
RING_STEPS = 40


def _ring_inputs(k, i):
    """step k's inputs: rotations of the shared ones (distinct for every k, the CPU reference rotates the same way)"""
    roll = lambda t, s: torch.roll(t, shifts=s, dims=1)
    return roll(i["vt"], 3 * k + 1), roll(i["lat"], k).bfloat16(), roll(i["eps"], 7 * k + 2)


def test_tickets_reset_and_the_scratch_ring_wraps(eng):
    """40 launches back to back wrap the 16-slot ring more than twice: every slot's tickets must have reset themselves.  Then 16 launches on two
    streams, one per slot (never more: 17 launches in flight are outside the documented contract)."""
    i = _inputs(RING_N)
    sig, sig_n, eta = _scalars_gpu()
    cpu = [_ring_inputs(k, i) for k in range(RING_STEPS)]
    dev = [tuple(t.cuda() for t in c) for c in cpu]
    step = lambda k: eng.sde_step(dev[k][0], None, 1.0, dev[k][1], sig, sig_n, eta, SIGMA_MAX, "Flow-SDE", noise=dev[k][2], want=())
    torch.cuda.synchronize()
    burst = [step(k) for k in range(RING_STEPS)]              # no synchronisation in between
    torch.cuda.synchronize()
    single = []
    for k in range(RING_STEPS):
        single.append(step(k))
        torch.cuda.synchronize()
    distinct = set()
    for k in range(RING_STEPS):
        assert torch.equal(burst[k].log_prob, single[k].log_prob), (k, burst[k].log_prob.tolist(), single[k].log_prob.tolist())
        assert torch.equal(burst[k].next_storage, single[k].next_storage), k
        ref = _sde_ref.sde_step(cpu[k][0], cpu[k][1], _t(SIGMA), _t(SIGMA_NEXT), _t(ETA), "Flow-SDE", SIGMA_MAX, noise=cpu[k][2])
        np.testing.assert_allclose(burst[k].log_prob.cpu().numpy(), ref["log_prob"].numpy(), rtol=_lp_rtol(RING_N), err_msg=str(k))
        distinct.add(tuple(burst[k].log_prob.tolist()))
    assert len(distinct) == RING_STEPS                        # the inputs really differed

    # two streams, 8 launches each = 16 in flight at the most, one per slot; the ring counter is offset by one launch first
    torch.cuda.synchronize()
    step(0)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [None] * 16
    for k in range(8):
        with torch.cuda.stream(s1):
            outs[k] = step(k)
        with torch.cuda.stream(s2):
            outs[8 + k] = step(8 + k)
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    for k in range(16):
        assert torch.equal(outs[k].log_prob, single[k].log_prob), (k, outs[k].log_prob.tolist(), single[k].log_prob.tolist())
        assert torch.equal(outs[k].next_storage, single[k].next_storage), k


# ------------------------------------------------------------------------------------------------- adjoint
GRADS = {"lp": ("g_lp",), "mean": ("g_mean",), "np": ("g_np",), "all": ("g_lp", "g_mean", "g_np")}
_KW = {"g_lp": "g_log_prob", "g_mean": "g_mean", "g_np": "g_noise_pred"}


def _row_err(a, ref64):
    """per output row: max |a - ref64| / max |ref64| (inf where the reference row is all zeros and `a` is not)"""
    a, ref64 = a.double().reshape(a.shape[0], -1), ref64.reshape(ref64.shape[0], -1)
    num, den = (a - ref64).abs().amax(1), ref64.abs().amax(1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


def _check_adjoint(dv, args_cpu, kw_cpu, tag, rows=None):
    """dv (GPU result, on the CPU) against the fp64 reference, bounded by ADJ_FACTOR x the fp32 reference's own deviation, row by row"""
    ref64 = _sde_ref.sde_step_bwd(*args_cpu, dtype=torch.float64, **kw_cpu)
    ref32 = _sde_ref.sde_step_bwd(*args_cpu, dtype=torch.float32, **kw_cpu)
    assert dv.shape == ref64.shape and dv.dtype == torch.float32, tag
    if rows is not None:
        dv, ref64, ref32 = dv[rows], ref64[rows], ref32[rows]
    assert bool(torch.isfinite(dv).all()) and bool(torch.isfinite(ref64).all()), tag
    e, E = _row_err(dv, ref64), _row_err(ref32, ref64)
    print(f"[adjoint] {tag}: kernel e {['%.2e' % x for x in e.tolist()]}  fp32-reference E {['%.2e' % x for x in E.tolist()]}")
    assert bool((e <= ADJ_FACTOR * E).all()), (tag, e.tolist(), E.tolist())


def _adjoint_case(eng, dyn, sd, n, cfg, eta_values=ETA):
    i = _inputs(n)
    lat = i["lat"].to(DT[sd])
    vt, vu = i["vt"], (i["vu"] if cfg else None)
    sig, sig_n = _scalars_gpu()[:2]
    eta = _t(eta_values).cuda()
    o = eng.sde_step(vt.cuda(), vu.cuda() if cfg else None, G, lat.cuda(), sig, sig_n, eta, SIGMA_MAX, dyn, noise=i["eps"].cuda(), want=())
    torch.cuda.synchronize()
    nxt = o.next_storage
    gpu = lambda compute_log_prob, **kw: eng.sde_step_bwd(vt.cuda(), vu.cuda() if cfg else None, G, lat.cuda(), nxt, sig, sig_n, eta, SIGMA_MAX, dyn,
                                                          compute_log_prob, **{k: v.cuda() for k, v in kw.items()}).cpu()
    cpu_args = lambda clp: (vt, vu, G, lat, nxt.cpu(), _t(SIGMA), _t(SIGMA_NEXT), _t(eta_values), SIGMA_MAX, dyn, clp)
    return i, gpu, cpu_args


@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("n", [6, 65798])
@pytest.mark.parametrize("sd", list(DT))
@pytest.mark.parametrize("dyn", DYNS)
def test_adjoint_grid(eng, dyn, sd, n, cfg):
    i, gpu, cpu_args = _adjoint_case(eng, dyn, sd, n, cfg)
    for name, keys in GRADS.items():
        kw = {_KW[k]: i[k] for k in keys}
        dv = gpu(True, **kw)
        assert dv.shape == ((2 if cfg else 1) * B, n)
        tag = (dyn, sd, n, "cfg" if cfg else "nocfg", name)
        if dyn == "ODE" and name == "lp":
            assert not bool(dv.any()), tag                      # the ODE step has no log-prob
            assert not bool(_sde_ref.sde_step_bwd(*cpu_args(True), **kw).any())
            continue
        _check_adjoint(dv, cpu_args(True), kw, tag)


@pytest.mark.parametrize("n", [6, 65798])
@pytest.mark.parametrize("dyn", DYNS)
def test_adjoint_without_log_prob_ignores_its_gradient(eng, dyn, n):
    i, gpu, cpu_args = _adjoint_case(eng, dyn, "bf16", n, True)
    with_lp = gpu(False, g_log_prob=i["g_lp"], g_mean=i["g_mean"], g_noise_pred=i["g_np"])
    without = gpu(False, g_mean=i["g_mean"], g_noise_pred=i["g_np"])
    assert torch.equal(with_lp, without), (dyn, n)
    assert torch.equal(without, gpu(True, g_mean=i["g_mean"], g_noise_pred=i["g_np"])), (dyn, n)
    assert not torch.equal(without, gpu(True, g_log_prob=i["g_lp"], g_mean=i["g_mean"], g_noise_pred=i["g_np"])) or dyn == "ODE"
    _check_adjoint(with_lp, cpu_args(False), dict(g_log_prob=i["g_lp"], g_mean=i["g_mean"], g_noise_pred=i["g_np"]), (dyn, n, "no log-prob"))


@pytest.mark.parametrize("n", [6, 65798])
@pytest.mark.parametrize("sd", list(DT))
def test_adjoint_ode_log_prob_gradient_is_zero(eng, sd, n):
    i, gpu, _ = _adjoint_case(eng, "ODE", sd, n, True)
    dv = gpu(True, g_log_prob=i["g_lp"])
    assert dv.shape == (2 * B, n) and not bool(dv.any())


@pytest.mark.parametrize("n", [6, 65798])
@pytest.mark.parametrize("dyn", ["Flow-SDE", "Dance-SDE"])
def test_adjoint_of_a_noise_free_sample_in_a_noisy_batch(eng, dyn, n):
    """eta = 0 for sample 1 only: its std is 0, the log-prob term is guarded (`sv > 0`) and dv is the g_mean contribution alone.  The reference's
    own log-prob is NaN at eta = 0, so sample 1 is compared with the reference WITHOUT a log-prob gradient."""
    eta = (0.7, 0.0, 0.8)
    for cfg in (False, True):
        i, gpu, cpu_args = _adjoint_case(eng, dyn, "bf16", n, cfg, eta_values=eta)
        both = gpu(True, g_log_prob=i["g_lp"], g_mean=i["g_mean"])
        mean_only = gpu(True, g_mean=i["g_mean"])
        rows1 = [1, B + 1] if cfg else [1]
        rows02 = [0, 2, B, B + 2] if cfg else [0, 2]
        assert bool(torch.isfinite(both).all()), (dyn, n, cfg)
        assert torch.equal(both[rows1], mean_only[rows1]), (dyn, n, cfg)
        assert not torch.equal(both[rows02], mean_only[rows02])
        _check_adjoint(both, cpu_args(True), dict(g_mean=i["g_mean"]), (dyn, n, cfg, "eta=0 sample"), rows=rows1)
        # the noisy samples of the same batch, against a reference run on them alone
        a = cpu_args(True)
        pick = lambda t: t[[0, 2]] if torch.is_tensor(t) and t.dim() >= 1 and t.shape[0] == B else t
        a02 = tuple(pick(t) for t in a)
        ref_kw = dict(g_log_prob=i["g_lp"][[0, 2]], g_mean=i["g_mean"][[0, 2]])
        _check_adjoint(both[rows02], a02, ref_kw, (dyn, n, cfg, "noisy samples"))

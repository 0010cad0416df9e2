"""Pins tests/_sde_ref.py -- the reference of the scheduler-step operator tests -- on the CPU, before any kernel is judged by it:
against `oracle.scheduler_ref.sde_step` (same torch operations in the same order), against the fixtures the reference's own code wrote
(tests/golden/scheduler_steps.npz), and its adjoint against `_plugin_fakes.oracle_sde_step_bwd`."""
import os

import numpy as np
import pytest
import torch

import _plugin_fakes
import _sde_ref
from conftest import GOLDEN
from oracle import scheduler_ref

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
FIELDS = ("next_latents_mean", "next_latents", "std_dev_t", "dt")


def _cps_cmp(sd_name, tag):
    # tests/test_gpu_kernels.py::test_sde_step_matches_reference_fixtures, CPS branch
    return lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 if sd_name == "fp32" else 8e-3, err_msg=str(tag))


def _exact_cmp(tag):
    return lambda a, b: np.testing.assert_array_equal(a, b, err_msg=str(tag))


@pytest.mark.parametrize("sd_name", list(DT))
@pytest.mark.parametrize("dyn", scheduler_ref.DYNAMICS)
def test_fp32_helper_equals_the_oracle_step(dyn, sd_name):
    g = torch.Generator().manual_seed(11)
    shp = (3, 4, 5, 7)
    lat = torch.randn(shp, generator=g).to(DT[sd_name])
    v = torch.randn(shp, generator=g).bfloat16()
    eps = torch.randn(shp, generator=g)
    for sigma, sigma_next, eta, smax in ((0.9, 0.85, 0.7, 0.98), (1.0, 0.9642857, 0.7, 0.9642857), (0.25, 0.03125, 0.8, 0.98)):
        want = scheduler_ref.sde_step(v, lat, sigma, sigma_next, eta, dyn, sigma_max=smax, variance_noise=eps)
        got = _sde_ref.sde_step(v, lat, sigma, sigma_next, eta, dyn, smax, noise=eps)
        tag = (dyn, sd_name, sigma)
        cmp = _cps_cmp(sd_name, tag) if dyn == "CPS" else _exact_cmp(tag)
        for f in FIELDS:
            cmp(got[f].reshape(-1).numpy(), want[f].reshape(-1).numpy())      # (the oracle's std_dev_t / dt are (B, 1, 1, 1))
        assert torch.equal(got["noise_pred"], v.float())
        np.testing.assert_allclose(got["log_prob"].numpy(), want["log_prob"].numpy(), rtol=2e-6, atol=1e-6, err_msg=str(tag))
        # replay of the stored (storage-dtype) next state
        nxt = scheduler_ref.cast_latents(want["next_latents"], DT[sd_name])
        want2 = scheduler_ref.sde_step(v, lat, sigma, sigma_next, eta, dyn, sigma_max=smax, next_latents=nxt)
        got2 = _sde_ref.sde_step(v, lat, sigma, sigma_next, eta, dyn, smax, next_latents=nxt)
        np.testing.assert_allclose(got2["log_prob"].numpy(), want2["log_prob"].numpy(), rtol=2e-6, atol=1e-6, err_msg=str(tag))


def test_per_sample_scalars_equal_one_call_per_sample():
    """a [B] tensor of scalars is the same as B calls with one scalar each (what the oracle step can express)"""
    g = torch.Generator().manual_seed(12)
    shp = (3, 33)
    lat, v, eps = torch.randn(shp, generator=g), torch.randn(shp, generator=g).bfloat16(), torch.randn(shp, generator=g)
    sigma, sigma_next, eta = [1.0, 0.875, 0.25], [0.9642857, 0.8181818, 0.03125], [0.7, 0.35, 0.8]
    for dyn in scheduler_ref.DYNAMICS:
        got = _sde_ref.sde_step(v, lat, torch.tensor(sigma), torch.tensor(sigma_next), torch.tensor(eta), dyn, 0.9642857, noise=eps)
        for b in range(3):
            one = _sde_ref.sde_step(v[b:b + 1], lat[b:b + 1], sigma[b], sigma_next[b], eta[b], dyn, 0.9642857, noise=eps[b:b + 1])
            for f in FIELDS + ("log_prob",):
                assert torch.equal(got[f][b:b + 1], one[f]), (dyn, b, f)
            assert bool(torch.isfinite(one["log_prob"]).all())


def test_helper_reproduces_every_fixture_case():
    z = np.load(os.path.join(GOLDEN, "scheduler_steps.npz"))
    n = int(z["num_cases"][0])
    assert n >= 40
    for ci in range(n):
        k = f"c{ci}"
        dyn, sd_name, i, eta, clp, t, t_next, smax = [str(x) for x in z[k + "_meta"]]
        eta, clp, t, t_next, smax = float(eta), bool(int(clp)), float(t), float(t_next), float(smax)
        lat = torch.from_numpy(z[k + "_latents"]).to(DT[sd_name])
        v = torch.from_numpy(z[k + "_noise_pred"]).bfloat16()
        eps = torch.from_numpy(z[k + "_eps"])
        sigma, sigma_next = torch.tensor(t) / 1000, torch.tensor(t_next) / 1000
        o = _sde_ref.sde_step(v, lat, sigma, sigma_next, eta, dyn, smax, noise=eps, compute_log_prob=clp)
        tag = (ci, dyn, sd_name, i)
        cmp = _cps_cmp(sd_name, tag) if dyn == "CPS" else _exact_cmp(tag)
        B = lat.shape[0]
        cmp(o["next_latents_mean"].numpy(), z[k + "_mean"])
        cmp(o["next_latents"].numpy(), z[k + "_next"])
        cmp(o["std_dev_t"].numpy(), np.broadcast_to(z[k + "_std"].reshape(-1), (B,)))
        assert np.array_equal(o["dt"].numpy(), np.broadcast_to(z[k + "_dt"].reshape(-1), (B,))), tag
        if clp:
            np.testing.assert_allclose(o["log_prob"].numpy(), z[k + "_logp"], rtol=2e-6, atol=1e-6, err_msg=str(tag))
        else:
            assert o["log_prob"] is None
        if (k + "_replay_logp") in z.files:
            o2 = _sde_ref.sde_step(v, lat, sigma, sigma_next, eta, dyn, smax, next_latents=o["next_latents"].to(DT[sd_name]))
            np.testing.assert_allclose(o2["log_prob"].numpy(), z[k + "_replay_logp"], rtol=2e-6, atol=1e-6, err_msg=str(tag))


def _dyadic(g, shape, lo, hi, step):
    """values on a coarse dyadic grid, exact in bf16"""
    k = torch.randint(int(lo / step), int(hi / step) + 1, shape, generator=g)
    return (k.float() * step).bfloat16()


@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("dyn", scheduler_ref.DYNAMICS)
def test_fp32_adjoint_agrees_with_the_plugin_oracle(dyn, cfg):
    """`oracle_sde_step_bwd` differentiates the fp32 combine `u + g (c - u)`; this helper differentiates at the bf16 combine.  The predictions
    here lie on a 1/4 grid in [-2, 2]: with g = 4.5 every intermediate of the combine (difference: multiples of 1/4 up to 4; product: multiples
    of 1/8 up to 18; sum: multiples of 1/8 up to 20) has at most 8 significant bits, so the bf16 combine is exact and both differentiate at the
    same point.  What remains is fp32 rounding in a different operation order (du = dv - g dv there, (1 - g) dv here): a few 2^-24, bounded
    here by 1e-6 of the largest gradient entry of the sample."""
    g = torch.Generator().manual_seed(13)
    B, shp = 2, (2, 4, 3, 5)
    lat = torch.randn(shp, generator=g).bfloat16()
    vt = _dyadic(g, shp, -2.0, 2.0, 0.25)
    vu = _dyadic(g, shp, -2.0, 2.0, 0.25) if cfg else None
    if cfg:
        assert torch.equal(_sde_ref.consumed_prediction(vt, vu, 4.5).float(), vu.float() + 4.5 * (vt.float() - vu.float()))
    sigma, sigma_next, eta, smax = 0.875, 0.8181818, 0.35, 0.9642857
    v = _sde_ref.consumed_prediction(vt, vu, 4.5)
    fwd = _sde_ref.sde_step(v, lat, sigma, sigma_next, eta, dyn, smax, noise=torch.randn(shp, generator=g))
    nxt = scheduler_ref.cast_latents(fwd["next_latents"], torch.bfloat16)
    g_lp, g_np, g_mn = torch.randn(B, generator=g), torch.randn(shp, generator=g), torch.randn(shp, generator=g)
    for grads in (dict(g_log_prob=g_lp), dict(g_mean=g_mn), dict(g_noise_pred=g_np), dict(g_log_prob=g_lp, g_noise_pred=g_np, g_mean=g_mn)):
        want = _plugin_fakes.oracle_sde_step_bwd(vt, vu, 4.5, lat, nxt, sigma, sigma_next, eta, smax, dyn, True, **grads)
        got = _sde_ref.sde_step_bwd(vt, vu, 4.5, lat, nxt, sigma, sigma_next, eta, smax, dyn, True, dtype=torch.float32, **grads)
        assert got.shape == want.shape == ((2 * B if cfg else B),) + shp[1:] and got.dtype == torch.float32
        if dyn == "ODE" and set(grads) == {"g_log_prob"}:
            assert not bool(got.any()) and not bool(want.any())
            continue
        for b in range(got.shape[0]):
            scale = float(want[b].abs().max())
            assert scale > 0
            err = float((got[b] - want[b]).abs().max()) / scale
            assert err <= 1e-6, (dyn, cfg, sorted(grads), b, err)
        # fp64 runs the same graph: the fp32 result is its rounding, not another function
        got64 = _sde_ref.sde_step_bwd(vt, vu, 4.5, lat, nxt, sigma, sigma_next, eta, smax, dyn, True, dtype=torch.float64, **grads)
        assert got64.dtype == torch.float64
        assert float((got.double() - got64).abs().max()) <= 1e-5 * float(got64.abs().max())

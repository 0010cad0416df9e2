"""GPU parity tests of the individual HIP kernels, called through the C ABI.

Each kernel is compared with a plain fp32 PyTorch evaluation of the same op on the same
(bf16-rounded) inputs; tolerances are the bf16 output rounding (2^-8 relative) plus accumulation
noise and are written next to each check.  The scheduler step is compared against fixtures
produced by the reference's own code (tests/golden/scheduler_steps.npz).
"""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import engine
    return engine


def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (300, 260, 128), (4096, 1536, 1536), (666, 6144, 1536),
                                   (4096, 1536, 6144), (1000, 64, 1536), (3, 1536, 256), (8192, 3072, 1536)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear(eng, M, N, K, act):
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K + act)
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)).bfloat16()
    b = torch.randn(N, device="cuda", generator=g) * 0.1
    y = eng.op_linear(x, w, b, act)
    ref = x.float() @ w.float().t() + b
    if act == 1:
        ref = torch.nn.functional.silu(ref.bfloat16().float())
    elif act == 2:
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    # asymmetric operands: a transposed / mis-mapped fragment gives rel error ~1.4, not 1e-3
    assert _rel(y, ref) < 4e-3, (M, N, K, act, _rel(y, ref))
    assert float((y.float() - ref).abs().max()) < 0.06 * max(1.0, float(ref.abs().max()))
    if M * N * K <= 300 * 260 * 128:
        # the three smallest shapes, PER ELEMENT against fp64 (the bounds of tests/test_gpu_gemm_epilogues.py): one wrong element, row or
        # 8-column strip at a tile edge passes the two norms above
        from test_gpu_gemm_epilogues import _direct, _gelu, _silu, _staged
        pre64 = x.double() @ w.double().t() + b.double()
        pre32 = x.float() @ w.float().t() + b
        if act == 2:
            _direct(y, _gelu(pre64), _gelu(pre32), f"linear gelu {M}x{N}x{K}")
        else:
            _staged(y, pre64, pre32, _silu if act == 1 else None, f"linear act={act} {M}x{N}x{K}")


@pytest.mark.parametrize("key,M,N,K", [(40, 8192, 1536, 1536), (40, 8192, 3072, 1536), (40, 8192, 1536, 6144), (40, 4608, 3072, 3072), (40, 256, 192, 128),
                                       (40, 8192 + 256, 1536 + 192, 256), (32, 4096, 1536, 1536), (32, 4096, 1536, 6144), (32, 4096 + 77, 1536 + 8, 1536)])
def test_gemm_tile_shapes_give_the_same_bits(eng, key, M, N, K):
    """The round-6 tile shapes -- 256x192 (`gemm_w6_kernel`, mi355_tune_set key 40) and 128x192 (`gemm_mid_kernel`, key 32) -- against what the
    dispatch runs without them (256x256 / 128x128 tiles): every kernel accumulates an output element with the same MFMA, operand order and
    ascending k and shares the fused epilogues, so bias / GELU / in-place gated-residual outputs are BIT-IDENTICAL (what lets the batch-invariance
    tests mix kernels by grid size), and re-runs are deterministic.  Also pinned to a plain fp32 evaluation of the op."""
    from mi355_flow import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)).bfloat16()
    b = torch.randn(N, device="cuda", generator=g)
    rps = 1024 if M % 1024 == 0 else 333
    gate = torch.randn((M + rps - 1) // rps, N, device="cuda", generator=g).bfloat16()
    res0 = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    ops = {"bias": lambda: eng.op_linear(x, w, b, 0), "gelu": lambda: eng.op_linear(x, w, b, 2),
           "gate_res": lambda: eng.op_linear_gate_res(res0.clone(), x, w, b, gate, rps)}
    try:
        for name, fn in ops.items():
            _lib.check(lib.mi355_tune_set(key, 0))
            ref = fn()
            _lib.check(lib.mi355_tune_set(key, 2))            # wherever the kernel applies
            got = fn()
            assert torch.equal(got, ref), (name, float((got.float() - ref.float()).abs().max()))
            for _ in range(3):
                assert torch.equal(fn(), got), name
        lin = x.float() @ w.float().t() + b
        assert _rel(ops["bias"](), lin) < 4e-3
        grow = gate.float().repeat_interleave(rps, dim=0)[:M]
        assert _rel(ops["gate_res"](), res0.float() + grow * lin.bfloat16().float()) < 6e-3
    finally:
        lib.mi355_tune_set(key, 1 if key == 32 else 0)        # the shipped defaults (the 256x192 kernel is off: measured slower in-model)


@pytest.mark.parametrize("B,H,S,n_img", [(1, 2, 64, 64), (2, 3, 333 + 256, 256), (1, 2, 1000, 1000), (1, 24, 4429, 4096),
                                         (2, 2, 77, 64)])
def test_attention(eng, B, H, S, n_img):
    g = torch.Generator(device="cuda").manual_seed(S + H)
    S_pad = (S + 63) // 64 * 64
    q = torch.zeros(B, H, S_pad, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.zeros_like(q)
    v = torch.zeros_like(q)
    q[:, :, :S] = torch.randn(B, H, S, 64, device="cuda", generator=g).bfloat16()
    k[:, :, :S] = (torch.randn(B, H, S, 64, device="cuda", generator=g) * 1.5).bfloat16()
    v[:, :, :S] = torch.randn(B, H, S, 64, device="cuda", generator=g).bfloat16()
    vT = v.transpose(2, 3).contiguous()
    o_img, o_ctx = eng.op_attention(q, k, vT, S, n_img)
    ref = torch.nn.functional.scaled_dot_product_attention(q[:, :, :S].float(), k[:, :, :S].float(), v[:, :, :S].float())
    ref = ref.transpose(1, 2).reshape(B, S, H * 64)
    got = torch.cat([o_img.view(B, n_img, H * 64), o_ctx.view(B, S - n_img, H * 64)], 1)
    # P is rounded to bf16 before the PV product (2^-9 relative) and O to bf16 on store
    assert _rel(got, ref) < 6e-3, _rel(got, ref)
    assert float((got.float() - ref).abs().max()) < 0.05


@pytest.mark.parametrize("B,H,S,n_img", [(2, 3, 333 + 256, 256), (1, 4, 4429, 4096)])
def test_attention_static_bound_kernel(eng, B, H, S, n_img):
    """The no-running-max kernel (selected by the engine when the q/k norm weights prove |score| <= 60 in the log2 domain) against
    fp32 SDPA, and against the deferred-rescale kernel on the same inputs."""
    from mi355_flow import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(S)
    S_pad = (S + 63) // 64 * 64
    q = torch.zeros(B, H, S_pad, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.zeros_like(q)
    v = torch.zeros_like(q)
    # RMS-normalised rows like the engine's q / k (norm 8): |score| * 0.125 * log2(e) <= 11.6
    nrm = lambda t: t / t.pow(2).mean(-1, keepdim=True).sqrt()
    q[:, :, :S] = nrm(torch.randn(B, H, S, 64, device="cuda", generator=g)).bfloat16()
    k[:, :, :S] = nrm(torch.randn(B, H, S, 64, device="cuda", generator=g)).bfloat16()
    v[:, :, :S] = torch.randn(B, H, S, 64, device="cuda", generator=g).bfloat16()
    vT = v.transpose(2, 3).contiguous()
    dyn_img, dyn_ctx = eng.op_attention(q, k, vT, S, n_img)
    try:
        _lib.check(lib.mi355_tune_set(6, 12))
        o_img, o_ctx = eng.op_attention(q, k, vT, S, n_img)
    finally:
        _lib.check(lib.mi355_tune_set(6, 1))
    ref = torch.nn.functional.scaled_dot_product_attention(q[:, :, :S].float(), k[:, :, :S].float(), v[:, :, :S].float())
    ref = ref.transpose(1, 2).reshape(B, S, H * 64)
    got = torch.cat([o_img.view(B, n_img, H * 64), o_ctx.view(B, S - n_img, H * 64)], 1)
    dyn = torch.cat([dyn_img.view(B, n_img, H * 64), dyn_ctx.view(B, S - n_img, H * 64)], 1)
    assert _rel(got, ref) < 6e-3, _rel(got, ref)
    assert _rel(got, dyn) < 6e-3


def test_attention_online_softmax_rescale(eng):
    """Force the running-max update late in the key loop (cdna guide rule 26): one spiked key in the
    last tile must take over the softmax of its query row."""
    B, H, S = 1, 1, 512
    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn(B, H, S, 64, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, H, S, 64, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, H, S, 64, device="cuda", generator=g).bfloat16()
    k[0, 0, 500] = (q[0, 0, 7].float() * 4).bfloat16()  # huge score for query 7 at key 500
    o_img, _ = eng.op_attention(q, k, v.transpose(2, 3).contiguous(), S, S)
    ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float())[0, 0]
    assert _rel(o_img, ref) < 6e-3
    assert float((o_img[7].float() - v[0, 0, 500].float()).abs().max()) < 0.05


@pytest.mark.parametrize("M,D,rps", [(512, 1536, 256), (333 * 2, 1536, 333), (64, 128, 16)])
def test_ln_modulate(eng, M, D, rps):
    g = torch.Generator(device="cuda").manual_seed(M + D)
    x = (torch.randn(M, D, device="cuda", generator=g) * 2 + 0.3).bfloat16()
    nb = M // rps
    shift = torch.randn(nb, D, device="cuda", generator=g).bfloat16()
    scale = torch.randn(nb, D, device="cuda", generator=g).bfloat16()
    y = eng.op_ln_modulate(x, shift, scale, rps)
    ln = torch.nn.functional.layer_norm(x.float(), (D,), eps=1e-6)
    idx = torch.arange(M, device="cuda") // rps
    ref = ln * (1 + scale.float()[idx]) + shift.float()[idx]
    assert _rel(y, ref) < 3e-3  # bf16 output rounding
    assert float((y.float() - ref).abs().max()) < 0.05


DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def test_sde_step_matches_reference_fixtures(eng):
    """K15 vs the reference's own FlowMatchEulerDiscreteSDEScheduler.step (fixtures).  mean / x'
    follow the reference's fp32 op order (no FMA contraction): bit-exact; the log-prob differs only
    by reduction order: rtol 2e-6."""
    z = np.load(os.path.join(GOLDEN, "scheduler_steps.npz"))
    n = int(z["num_cases"][0])
    for ci in range(n):
        k = f"c{ci}"
        dyn, sd_name, i, eta, clp, t, t_next, smax = [str(x) for x in z[k + "_meta"]]
        eta, clp, t, t_next, smax = float(eta), bool(int(clp)), float(t), float(t_next), float(smax)
        lat = torch.from_numpy(z[k + "_latents"]).to(DT[sd_name]).cuda()
        v = torch.from_numpy(z[k + "_noise_pred"]).bfloat16().cuda()
        eps = torch.from_numpy(z[k + "_eps"]).cuda()
        sigma = float(np.float32(t) / np.float32(1000))
        sigma_next = float(np.float32(t_next) / np.float32(1000))
        o = eng.sde_step(v, None, 1.0, lat, sigma, sigma_next, eta, smax, dyn, noise=eps, compute_log_prob=clp)
        torch.cuda.synchronize()
        tag = (ci, dyn, sd_name, i)
        if dyn == "CPS":
            # std_dev_t = sigma' * sin(eta*pi/2): libm sin differs by an ulp between host and device
            cmp = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 if sd_name == "fp32" else 8e-3, err_msg=str(tag))
        else:
            cmp = lambda a, b: np.testing.assert_array_equal(a, b, err_msg=str(tag))
        cmp(o.next_latents_mean.cpu().numpy(), z[k + "_mean"])
        cmp(o.next_latents.cpu().numpy(), z[k + "_next"])
        # storage-dtype copy: the ODE branch of the reference returns the unrounded mean and lets
        # cast_latents round it (models/abc.py:172-182); the SDE branches round inside step() (:362)
        want_st = torch.from_numpy(z[k + "_next"]).to(DT[sd_name]).float().numpy()
        cmp(o.next_storage.float().cpu().numpy(), want_st)
        cmp(o.std_dev_t.cpu().numpy(), z[k + "_std"].reshape(-1))
        assert np.array_equal(o.dt.cpu().numpy(), z[k + "_dt"].reshape(-1)), tag
        if clp:
            np.testing.assert_allclose(o.log_prob.cpu().numpy(), z[k + "_logp"], rtol=2e-6, atol=1e-6, err_msg=str(tag))
        if (k + "_replay_logp") in z.files:
            nxt = o.next_storage
            o2 = eng.sde_step(v, None, 1.0, lat, sigma, sigma_next, eta, smax, dyn, next_latents=nxt)
            np.testing.assert_allclose(o2.log_prob.cpu().numpy(), z[k + "_replay_logp"], rtol=2e-6, atol=1e-6)
            # ratio == 1 invariant, engine vs engine: bit-identical
            assert torch.equal(o2.log_prob, o.log_prob), tag


def test_sde_step_cfg_and_large(eng):
    """CFG combine evaluated op-by-op in bf16 (sd3_5.py:431-433) + full-size sample (16x128x128)."""
    from oracle import rollout_ref, scheduler_ref
    g = torch.Generator().manual_seed(3)
    B, shp = 2, (2, 16, 128, 128)
    lat = torch.randn(shp, generator=g).half()
    vu = torch.randn(shp, generator=g).bfloat16()
    vt = torch.randn(shp, generator=g).bfloat16()
    eps = torch.randn(shp, generator=g)
    v = rollout_ref.cfg_combine_bf16(vu, vt, 4.5)
    ref = scheduler_ref.sde_step(v, lat, 0.9, 0.85, 0.7, "Flow-SDE", sigma_max=0.98, variance_noise=eps)
    o = eng.sde_step(vt.cuda(), vu.cuda(), 4.5, lat.cuda(), 0.9, 0.85, 0.7, 0.98, "Flow-SDE", noise=eps.cuda())
    assert torch.equal(o.noise_pred.cpu(), v.float())
    assert torch.equal(o.next_latents.cpu(), ref["next_latents"])
    np.testing.assert_allclose(o.log_prob.cpu().numpy(), ref["log_prob"].numpy(), rtol=1e-5)

"""The scheduler-step entry points (`mi355_sde_step`, `mi355_sde_step_bwd`) and the UniPC operators (`mi355_unipc_convert`,
`mi355_op_lincomb`) of csrc/engine.hip check their arguments before any HIP call: a bad argument returns non-zero on a box without a GPU
and mi355_last_error() names the entry point AND the argument (a failed launch would name a HIP error instead).  Pointers that must be
non-NULL to reach a later check are dummies: nothing dereferences them."""
import ctypes as C

import pytest

from mi355_flow import _lib

P = C.c_void_p(4096)      # never dereferenced
N = None


def _step(batch=3, n=8, v_text=P, v_uncond=N, v_dtype=1, latents=P, lat_dtype=1, noise=P, next_in=N, next_in_dtype=0, sigma=P, sigma_next=P,
          eta=P, scalar_stride=1, dynamics=1, compute_log_prob=1):
    return (batch, n, v_text, v_uncond, v_dtype, 1.0, latents, lat_dtype, noise, next_in, next_in_dtype, sigma, sigma_next, eta, scalar_stride,
            0.98, dynamics, compute_log_prob, P, N, N, N, P, N, N)


def _bwd(batch=3, n=8, v_text=P, latents=P, lat_dtype=1, next_in=P, next_in_dtype=1, sigma=P, eta=P, scalar_stride=1, dynamics=1, dv=P):
    return (batch, n, v_text, N, 1.0, latents, lat_dtype, next_in, next_in_dtype, sigma, P, eta, scalar_stride, 0.98, dynamics, 1, P, N, N, dv)


def _lincomb(n_terms=2, tensors=(4096, 4096), dtypes=(1, 1), out=P, out_dtype=1, n=8, null_arrays=False):
    t = (C.c_void_p * 5)(*tensors)
    d = (C.c_int * 5)(*dtypes)
    c = (C.c_float * 5)(1.0, 1.0)
    if null_arrays:
        return (n_terms, None, d, c, out, out_dtype, n)
    return (n_terms, t, d, c, out, out_dtype, n)


CASES = [
    # entry point, arguments after the stream, fragment the message must carry
    ("mi355_sde_step", _step(v_text=N), "null argument"),
    ("mi355_sde_step", _step(eta=N), "null argument"),
    ("mi355_sde_step", _step(noise=N), "needs `noise`"),
    ("mi355_sde_step", _step(dynamics=4), "unknown dynamics 4"),
    ("mi355_sde_step", _step(lat_dtype=3), "bad latent dtype 3"),
    ("mi355_sde_step", _step(v_dtype=-1), "bad noise_pred dtype -1"),
    ("mi355_sde_step", _step(batch=0), "batch must be positive (got 0)"),
    ("mi355_sde_step", _step(batch=-2), "batch must be positive (got -2)"),
    ("mi355_sde_step", _step(n=0), "n must be positive (got 0)"),
    ("mi355_sde_step", _step(n=-4), "n must be positive (got -4)"),
    ("mi355_sde_step", _step(batch=4097), "per-slot limit of 4096"),
    ("mi355_sde_step", _step(scalar_stride=2), "scalar_stride must be 0"),
    ("mi355_sde_step", _step(scalar_stride=-1), "scalar_stride must be 0"),
    ("mi355_sde_step", _step(next_in=P, next_in_dtype=3), "bad next_in_dtype 3"),
    ("mi355_sde_step", _step(next_in=P, next_in_dtype=-1), "bad next_in_dtype -1"),
    ("mi355_sde_step", _step(compute_log_prob=3), "compute_log_prob must be 0, 1 or 2 (got 3)"),
    ("mi355_sde_step", _step(compute_log_prob=-1), "compute_log_prob must be 0, 1 or 2 (got -1)"),
    ("mi355_sde_step_bwd", _bwd(v_text=N), "null argument"),
    ("mi355_sde_step_bwd", _bwd(next_in=N), "null argument"),
    ("mi355_sde_step_bwd", _bwd(dv=N), "null argument"),
    ("mi355_sde_step_bwd", _bwd(dynamics=-1), "unknown dynamics -1"),
    ("mi355_sde_step_bwd", _bwd(lat_dtype=3), "bad dtype"),
    ("mi355_sde_step_bwd", _bwd(next_in_dtype=3), "bad dtype"),
    ("mi355_sde_step_bwd", _bwd(batch=0), "batch must be positive (got 0)"),
    ("mi355_sde_step_bwd", _bwd(n=0), "n must be positive (got 0)"),
    ("mi355_sde_step_bwd", _bwd(n=-1), "n must be positive (got -1)"),
    ("mi355_sde_step_bwd", _bwd(batch=65536), "y limit of 65535"),
    ("mi355_sde_step_bwd", _bwd(scalar_stride=2), "scalar_stride must be 0"),
    ("mi355_unipc_convert", (N, N, 1, 1.0, P, 1, 0.5, P, 8), "null argument"),
    ("mi355_unipc_convert", (P, N, 1, 1.0, N, 1, 0.5, P, 8), "null argument"),
    ("mi355_unipc_convert", (P, N, 1, 1.0, P, 1, 0.5, N, 8), "null argument"),
    ("mi355_unipc_convert", (P, N, 1, 1.0, P, 1, 0.5, P, 6), "positive multiple of 4 (got 6)"),
    ("mi355_unipc_convert", (P, N, 1, 1.0, P, 1, 0.5, P, 0), "positive multiple of 4 (got 0)"),
    ("mi355_unipc_convert", (P, N, 3, 1.0, P, 1, 0.5, P, 8), "bad v_dtype 3"),
    ("mi355_unipc_convert", (P, N, 1, 1.0, P, -1, 0.5, P, 8), "bad sample_dtype -1"),
    ("mi355_op_lincomb", _lincomb(null_arrays=True), "null argument"),
    ("mi355_op_lincomb", _lincomb(out=N), "null argument"),
    ("mi355_op_lincomb", _lincomb(n_terms=0), "1..5 terms (got 0)"),
    ("mi355_op_lincomb", _lincomb(n_terms=6), "1..5 terms (got 6)"),
    ("mi355_op_lincomb", _lincomb(n=10), "positive multiple of 4 (got 10)"),
    ("mi355_op_lincomb", _lincomb(out_dtype=3), "bad out_dtype 3"),
    ("mi355_op_lincomb", _lincomb(dtypes=(1, 5)), "bad dtypes[1] = 5"),
    ("mi355_op_lincomb", _lincomb(tensors=(4096, None)), "tensors[1] is NULL"),
]

ENTRY_POINTS = ["mi355_sde_step", "mi355_sde_step_bwd", "mi355_unipc_convert", "mi355_op_lincomb"]


@pytest.mark.parametrize("fn_name,args,fragment", CASES, ids=[f"{c[0]}-{i}-{c[2].replace(' ', '_')}" for i, c in enumerate(CASES)])
def test_bad_arguments_are_refused_before_any_hip_call(fn_name, args, fragment):
    lib = _lib.load()
    assert len(args) + 1 == len(_lib.SIGNATURES[fn_name][1])
    rc = getattr(lib, fn_name)(None, *args)
    assert rc != 0
    msg = lib.mi355_last_error().decode()
    assert msg.startswith(fn_name + ":") and fragment in msg, msg
    with pytest.raises(RuntimeError, match=fn_name):
        _lib.check(rc, fn_name)


def test_every_entry_point_has_a_null_and_a_range_case():
    for fn_name in ENTRY_POINTS:
        frags = [c[2] for c in CASES if c[0] == fn_name]
        assert "null argument" in frags and len(frags) >= 3, fn_name
        assert fn_name in _lib.SIGNATURES

"""The operator entry points of the two-group modulation kernels (`mi355_op_*_split`) and the first-frame entry points of the Wan engine check
their arguments before any HIP call, like their siblings (tests/test_backward_ops_args.py, tests/test_gemm_epi_args.py): bad arguments return
non-zero on a box without a GPU, and mi355_last_error() names the operator AND the argument.  Pointers that must be non-NULL to reach a check
are dummies: nothing dereferences them."""
import ctypes as C

import pytest

from mi355_flow import _lib

P = C.c_void_p(4096)      # never dereferenced
N = None


def _gemm(epi=5, M=16, Nn=8, K=64, rps=4, head_rows=2, aux=P, stash=N):
    # A, lda, W, ldw, M, N, K, epi, bias, out, ldo, aux, ld_aux, rows_per_sample, q, k, nw_q, nw_k, H, S_pad, s_off, eps, hd_shift, q_scale, hp, wp,
    # patch, out_ch, stash, ld_stash, rstd_out, head_rows
    return (P, K, P, K, M, Nn, K, epi, P, P, Nn, aux, Nn, rps, N, N, N, N, 0, 0, 0, 1e-6, 0, 0.0, 0, 0, 0, 0, stash, Nn, N, head_rows)


CASES = [
    # operator, arguments after the stream, fragment the message must carry
    ("ln_modulate_split", (N, P, P, P, 4, 8, 2, 1e-6, 1), "null argument"),
    ("ln_modulate_split", (P, P, P, P, 4, 12, 2, 1e-6, 1), "multiple of 8"),
    ("ln_modulate_split", (P, P, P, P, 4, 8, 0, 1e-6, 0), "rows_per_sample 0"),
    ("ln_modulate_split", (P, P, P, P, 4, 8, 2, 1e-6, 3), "head_rows = 3 outside"),
    ("ln_modulate_split", (P, P, P, P, 4, 8, 2, 1e-6, -1), "head_rows = -1 outside"),
    ("ln_mod_bwd_split", (N, P, N, P, P, 56, 0, 8, 0, 0, 4, 8, 2, 1e-6, 0, N, 1), "null argument"),
    ("ln_mod_bwd_split", (P, P, N, P, P, 80, 0, 8, 0, 0, 4, 12, 2, 1e-6, 0, N, 1), "multiple of 8"),
    ("ln_mod_bwd_split", (P, P, N, P, P, 56, 0, 8, 0, 0, 4, 8, 2, 1e-6, 0, N, 3), "head_rows = 3 outside"),
    ("ln_mod_bwd_split", (P, P, N, P, P, 56, 0, 8, 0, 0, 4, 8, 2, 1e-6, 0, P, 1), "modulation gradients (dmod)"),
    ("gate_bwd_split", (P, N, 8, N, P, N, 8, 4, 8, 2, 1), "null argument"),
    ("gate_bwd_split", (P, P, 12, N, P, N, 12, 4, 12, 2, 1), "multiple of 8"),
    ("gate_bwd_split", (P, P, 8, N, P, N, 8, 4, 8, 2, 3), "head_rows = 3 outside"),
    ("gate_bwd_split", (P, P, 8, P, P, P, 8, 4, 8, 2, 1), "gate gradient (dgate)"),
    ("gemm_epi_split", _gemm(aux=N), "null argument (aux)"),
    ("gemm_epi_split", _gemm(K=96), "K = 96 is not a multiple of 64"),
    ("gemm_epi_split", _gemm(head_rows=-1), "head_rows = -1 is negative"),
    ("gemm_epi_split", _gemm(head_rows=5), "head_rows = 5 exceeds rows_per_sample = 4"),
    ("gemm_epi_split", _gemm(epi=0), "only the gated-residual epilogue"),
]

OPERATORS = ["ln_modulate_split", "ln_mod_bwd_split", "gate_bwd_split", "gemm_epi_split"]


@pytest.mark.parametrize("op,args,fragment", CASES, ids=[f"{c[0]}-{c[2].replace(' ', '_')}" for c in CASES])
def test_bad_arguments_are_refused_before_any_hip_call(op, args, fragment):
    lib = _lib.load()
    fn = getattr(lib, "mi355_op_" + op)
    assert len(args) + 1 == len(_lib.SIGNATURES["mi355_op_" + op][1])
    rc = fn(None, *args)
    assert rc != 0
    msg = lib.mi355_last_error().decode()
    assert msg.startswith("mi355_op_" + op + ":") and fragment in msg, msg
    with pytest.raises(RuntimeError, match="mi355_op_" + op):
        _lib.check(rc, "op_" + op)


def test_every_split_operator_has_a_null_and_a_shape_case():
    for op in OPERATORS:
        frags = [c[2] for c in CASES if c[0] == op]
        assert any("null argument" in f for f in frags) and len(frags) >= 2, op
        assert "mi355_op_" + op in _lib.SIGNATURES


def test_the_unsplit_operators_keep_their_messages():
    """the shared argument checks report the entry point that was called"""
    lib = _lib.load()
    assert lib.mi355_op_gate_bwd(None, P, N, 8, N, P, N, 8, 4, 8, 2) != 0 and lib.mi355_last_error().decode().startswith("mi355_op_gate_bwd: null")
    assert lib.mi355_op_ln_mod_bwd(None, N, P, N, P, P, 56, 0, 8, 0, 0, 4, 8, 2, 1e-6, 0, N) != 0
    assert lib.mi355_last_error().decode().startswith("mi355_op_ln_mod_bwd: null")
    assert lib.mi355_op_gemm_epi(None, *_gemm(aux=N)[:-1]) != 0 and lib.mi355_last_error().decode().startswith("mi355_op_gemm_epi: null argument (aux)")


def test_first_frame_entry_points_refuse_null_handles():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.mi355_wan_plan_create_ff(None, 1, 1, 1, 4, 4, 8, 1, C.byref(h)) != 0 and b"null argument" in lib.mi355_last_error()
    assert lib.mi355_wan_forward_ff(None, None, P, 0, P, P, None, P, 0, P) != 0 and lib.mi355_last_error() == b"mi355_wan_forward_ff: null argument"
    assert lib.mi355_wan_forward_train_ff(None, None, P, 0, P, P, None, P, 0, P) != 0
    assert lib.mi355_last_error() == b"mi355_wan_forward_train_ff: null argument"
    fa = (C.c_float * 1)(0.0)
    assert lib.mi355_wan_rollout_ff(None, None, 1, fa, fa, fa, 0, 1.0, P, 0, 0, None, P, None, None, None, None, None, 0, P, 0) != 0
    assert lib.mi355_last_error() == b"mi355_wan_rollout_ff: null argument"
    # the plain entry points keep their own names
    assert lib.mi355_wan_forward(None, None, P, 0, P, P, None, P) != 0 and lib.mi355_last_error() == b"mi355_wan_forward: null argument"
    assert lib.mi355_wan_forward_train(None, None, P, 0, P, P, None, P) != 0 and lib.mi355_last_error() == b"mi355_wan_forward_train: null argument"

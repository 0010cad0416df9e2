"""The operator entry points of the backward's helper kernels (`mi355_op_*`, csrc/engine_train.inc) check their arguments before any HIP
call: NULL pointers and bad shapes return non-zero on a box without a GPU, and mi355_last_error() names the operator AND the argument (a
failed launch would name a HIP error instead).  Pointers that must be non-NULL to reach a shape check are dummies: nothing dereferences them."""
import ctypes as C

import pytest

from mi355_flow import _lib

P = C.c_void_p(4096)      # never dereferenced
N = None

CASES = [
    # operator, arguments after the stream, fragment the message must carry
    ("ln_mod_bwd", (N, P, N, P, P, 56, 0, 8, 0, 0, 4, 8, 2, 1e-6, 0, N), "null argument"),
    ("ln_mod_bwd", (P, P, N, P, P, 80, 0, 8, 0, 0, 4, 12, 2, 1e-6, 0, N), "multiple of 8"),
    ("ln_mod_bwd", (P, P, N, P, P, 6 * 4104, 0, 4104, 0, 0, 4, 4104, 2, 1e-6, 0, P), "wider than 4096"),
    ("ln_mod_bwd", (P, P, N, P, P, 6 * 6152, 0, 6152, 0, 0, 4, 6152, 2, 1e-6, 0, N), "wider than 6144"),
    ("ln_mod_bwd", (P, P, N, P, P, 56, 0, 8, 0, 0, 4, 8, 0, 1e-6, 0, N), "rows_per_sample 0"),
    ("gate_bwd", (P, N, 8, N, P, N, 8, 4, 8, 2), "null argument"),
    ("gate_bwd", (P, P, 12, N, P, N, 12, 4, 12, 2), "multiple of 8"),
    ("gate_bwd", (P, P, 8, P, P, N, 8, 4, 8, 2), "go together"),
    ("silu_bwd", (P, N, P, 8), "null argument"),
    ("silu_bwd", (P, P, P, 12), "multiple of 8"),
    ("gelu_fwd", (N, P, 8), "null argument"),
    ("gelu_fwd", (P, P, 12), "multiple of 8"),
    ("transpose", (N, 64, 0, P, 64, 0, 64, 64, 64, 1, N, N, 0, 1), "null argument"),
    ("transpose", (P, 64, 0, P, 64, 0, 64, 64, 63, 1, N, N, 0, 1), "rows_pad = 63 is below rows = 64"),
    ("transpose", (P, 64, 0, P, 64, 0, 64, 64, 64, 1, P, N, 0, 1), "go together"),
    ("transpose", (P, 64, 0, P, 64, 0, 64, 64, 64, 2, P, P, 0, 1), "one matrix"),
    ("transpose", (P, 64, 0, P, 64, 0, 64, 64, 64, 1, P, P, 2, 1), "fp32 or bf16"),
    ("colsum", (P, 8, 4, 8, N, P, 0, 0), "null argument"),
    ("colsum", (P, 8, 0, 8, P, P, 0, 0), "bad shape"),
    ("colsum", (P, 8, 4, 8, P, P, 2, 0), "fp32 or bf16"),
    ("splitk_reduce", (N, 16, 2, P, 0, 16, 0, N, 0, 0, N, 0), "null argument"),
    ("splitk_reduce", (P, 16, 0, P, 0, 16, 0, N, 0, 0, N, 0), "nsplit = 0"),
    ("splitk_reduce", (P, 16, 2, P, 0, 16, 0, P, 4, 8, N, 0), "go together"),
    ("splitk_reduce", (P, 16, 2, P, 0, 16, 1, P, 4, 8, P, 0), "accumulate must be 0"),
    ("f32_to_bf16_pad", (P, N, 5, 64, 7), "null argument"),
    ("f32_to_bf16_pad", (P, P, 5, 4, 7), "rows_pad = 4 is below rows = 5"),
    ("unpatch_bwd", (N, P, 2, 16, 3, 5, 2), "null argument"),
    ("unpatch_bwd", (P, P, 2, 16, 3, 5, 0), "bad shape"),
    ("attn_bwd_prep", (P, P, P, P, N, P, P, P, 1, 1, 64, 64, 64), "null argument"),
    ("attn_bwd_prep", (P, P, P, P, P, P, P, P, 1, 1, 64, 100, 64), "not a multiple of 64"),
    ("attn_bwd_prep", (P, P, P, P, P, P, P, P, 1, 1, 65, 64, 64), "S_pad is below S"),
    ("attn_bwd_prep", (P, P, P, P, P, P, P, P, 1, 1, 64, 64, 65), "n_img outside"),
    ("attn_bwd_prep", (P, N, P, P, P, P, P, P, 1, 1, 64, 64, 32), "o_ctx is NULL"),
    ("rms_bwd_gather", (P, P, P, P, N, P, P, P, P, P, P, 1.0, P, P, 1, 1, 64, 64, 32, N, N, N, N, N), "null argument"),
    ("rms_bwd_gather", (P, P, P, P, P, P, P, P, P, P, P, 1.0, P, P, 1, 1, 64, 96, 32, N, N, N, N, N), "not a multiple of 64"),
    ("rms_bwd_gather", (P, P, P, P, P, P, P, P, P, P, P, 1.0, P, P, 1, 1, 70, 64, 32, N, N, N, N, N), "S_pad is below S"),
    ("rms_bwd_gather", (P, P, P, P, P, P, N, P, P, P, P, 1.0, P, P, 1, 1, 64, 64, 32, N, N, N, N, N), "context-stream"),
    ("rms_bwd_gather", (P, P, P, P, P, P, P, P, P, P, P, 1.0, P, P, 1, 1, 64, 64, 32, N, P, N, N, N), "need dw_part"),
]

OPERATORS = ["ln_mod_bwd", "gate_bwd", "silu_bwd", "gelu_fwd", "transpose", "colsum", "splitk_reduce", "f32_to_bf16_pad", "unpatch_bwd",
             "attn_bwd_prep", "rms_bwd_gather"]


@pytest.mark.parametrize("op,args,fragment", CASES, ids=[f"{c[0]}-{c[2].replace(' ', '_')}" for c in CASES])
def test_bad_arguments_are_refused_before_any_hip_call(op, args, fragment):
    lib = _lib.load()
    fn = getattr(lib, "mi355_op_" + op)
    assert len(args) + 1 == len(_lib.SIGNATURES["mi355_op_" + op][1])
    rc = fn(None, *args)
    assert rc != 0 and rc != 2                      # (2 is mi355_op_splitk_reduce's "takes two launches", not an error)
    msg = lib.mi355_last_error().decode()
    assert msg.startswith("mi355_op_" + op + ":") and fragment in msg, msg
    with pytest.raises(RuntimeError, match="mi355_op_" + op):
        _lib.check(rc, "op_" + op)


def test_every_backward_operator_has_a_null_and_a_shape_case():
    for op in OPERATORS:
        frags = [c[2] for c in CASES if c[0] == op]
        assert "null argument" in frags and len(frags) >= 2, op
        assert "mi355_op_" + op in _lib.SIGNATURES

"""`mi355_op_gemm_epi` (csrc/engine.hip) checks every argument before any HIP call: on a box without a GPU a NULL pointer the chosen epilogue
needs, or a shape / stride the kernels' vector accesses cannot take, returns non-zero and mi355_last_error() names the operator AND the
argument (a failed launch would name a HIP error instead).  Pointers that must be non-NULL to reach a later check are dummies: nothing
dereferences them.  Same pattern as tests/test_backward_ops_args.py."""
import ctypes as C

import pytest

from mi355_flow import _lib

P = C.c_void_p(4096)      # never dereferenced (16-byte aligned)
ODD = C.c_void_p(4104)    # 8-byte aligned only
BIAS, SILU, GELU, POSADD, ADDSRC, GATE_RES, QK_NORM, VT, UNPATCH, DGELU = 0, 1, 2, 3, 4, 5, 6, 7, 8, 12

ORDER = ["A", "lda", "W", "ldw", "M", "N", "K", "epi", "bias", "out", "ldo", "aux", "ld_aux", "rows_per_sample", "q", "k", "nw_q", "nw_k", "H",
         "S_pad", "s_off", "eps", "hd_shift", "q_scale", "hp", "wp", "patch", "out_ch", "stash", "ld_stash", "rstd_out"]
# a call that passes every check of every epilogue kind it is given to (M = 128 = 2 << 6 for VT, N = 128 = 2 * 1 * 64 for QK_NORM = 2 * 2 * 32)
GOOD = dict(A=P, lda=64, W=P, ldw=64, M=128, N=128, K=64, epi=BIAS, bias=P, out=P, ldo=128, aux=P, ld_aux=128, rows_per_sample=64, q=P, k=P, nw_q=P,
            nw_k=P, H=1, S_pad=64, s_off=0, eps=1e-6, hd_shift=0, q_scale=0.0, hp=8, wp=8, patch=2, out_ch=32, stash=None, ld_stash=0, rstd_out=None)


def _args(**kw):
    d = dict(GOOD)
    d.update(kw)
    return tuple(d[n] for n in ORDER)


CASES = [
    # changed arguments, fragment the message must carry
    (dict(epi=9), "epi = 9 is not one of the fused epilogues"),              # EPI_BIAS_ROW: the VAE's, out of scope
    (dict(epi=13), "epi = 13 is not one of the fused epilogues"),            # EPI_QK_NORM_RSTD is selected by rstd_out, not by the caller
    (dict(A=None), "null argument (A, W, bias)"),
    (dict(bias=None), "null argument (A, W, bias)"),
    (dict(M=0), "bad shape M = 0"),
    (dict(K=96, lda=96, ldw=96), "K = 96 is not a multiple of 64"),
    (dict(N=130, ldo=136, ld_aux=136), "N = 130 is not a multiple of 4"),
    (dict(lda=68), "lda = 68 must be a multiple of 8"),
    (dict(lda=56), "lda = 56 must be a multiple of 8 and at least K"),
    (dict(ldw=68), "ldw = 68 must be a multiple of 8"),
    (dict(A=ODD), "A and W must be 16-byte aligned"),
    (dict(epi=POSADD, rows_per_sample=0), "rows_per_sample 0 is below 1"),
    (dict(out=None), "null argument (out)"),
    (dict(epi=DGELU, out=None), "null argument (out)"),
    (dict(ldo=124), "ldo = 124 is below N"),
    (dict(out=ODD), "out must be 16-byte aligned when ldo is a multiple of 8"),
    (dict(epi=POSADD, aux=None), "null argument (aux)"),
    (dict(epi=ADDSRC, aux=None), "null argument (aux)"),
    (dict(epi=GATE_RES, aux=None), "null argument (aux)"),
    (dict(epi=DGELU, aux=None), "null argument (aux)"),
    (dict(epi=POSADD, ld_aux=132), "ld_aux = 132 must be a multiple of 8"),
    (dict(epi=ADDSRC, ld_aux=120), "ld_aux = 120 must be a multiple of 8 and at least N"),
    (dict(epi=GATE_RES, N=132, ldo=136, ld_aux=136), "N = 132 is not a multiple of 8 (gated residual)"),
    (dict(epi=SILU, stash=P, ld_stash=128), "stash is written by the GELU and the gated-residual epilogues only"),
    (dict(epi=GELU, stash=P, ld_stash=120), "ld_stash = 120 is below N"),
    (dict(epi=GELU, stash=ODD, ld_stash=128), "stash must be 16-byte aligned when ld_stash is a multiple of 8"),
    (dict(epi=BIAS, rstd_out=P), "rstd_out is written by the q/k-norm epilogue only"),
    (dict(epi=QK_NORM, q=None), "null argument (q, k, nw_q, nw_k)"),
    (dict(epi=QK_NORM, nw_k=None), "null argument (q, k, nw_q, nw_k)"),
    (dict(epi=QK_NORM, H=2), "N = 128 is not 2 * H * 64 = 256"),
    (dict(epi=QK_NORM, H=0), "H = 0 is below 1"),
    (dict(epi=QK_NORM, s_off=8), "S_pad = 64 is below s_off + rows_per_sample = 8 + 64"),
    (dict(epi=QK_NORM, s_off=-8), "S_pad = 64 is below s_off + rows_per_sample = -8 + 64"),
    (dict(epi=VT, q=None), "null argument (q = vT)"),
    (dict(epi=VT, H=1), "M = 128 is not H << hd = 64"),
    (dict(epi=VT, H=2, hd_shift=7), "M = 128 is not H << hd = 256"),
    (dict(epi=VT, H=2, hd_shift=5), "hd_shift = 5"),
    (dict(epi=VT, H=2, S_pad=60, rows_per_sample=60), "S_pad = 60 must be a multiple of 8"),
    (dict(epi=VT, H=2, S_pad=56), "S_pad = 56 is below s_off + rows_per_sample = 0 + 64"),
    (dict(epi=UNPATCH, patch=0), "bad shape hp = 8, wp = 8, patch = 0"),
    (dict(epi=UNPATCH, hp=3, wp=5), "M = 128 is not a multiple of hp * wp = 15"),
    (dict(epi=UNPATCH, out_ch=16), "N = 128 is not patch * patch * out_ch = 64"),
]


@pytest.mark.parametrize("changes,fragment", CASES, ids=[f"{i:02d}-{c[1][:40].replace(' ', '_')}" for i, c in enumerate(CASES)])
def test_bad_arguments_are_refused_before_any_hip_call(changes, fragment):
    lib = _lib.load()
    args = _args(**changes)
    assert len(args) + 1 == len(_lib.SIGNATURES["mi355_op_gemm_epi"][1])
    rc = lib.mi355_op_gemm_epi(None, *args)
    assert rc != 0
    msg = lib.mi355_last_error().decode()
    assert msg.startswith("mi355_op_gemm_epi:") and fragment in msg, msg
    with pytest.raises(RuntimeError, match="mi355_op_gemm_epi"):
        _lib.check(rc, "op_gemm_epi")


def test_every_epilogue_kind_has_a_null_and_a_shape_case():
    for epi, null_frag in ((BIAS, "null argument (out)"), (POSADD, "null argument (aux)"), (ADDSRC, "null argument (aux)"), (GATE_RES, "null argument (aux)"),
                           (DGELU, "null argument (aux)"), (QK_NORM, "null argument (q, k"), (VT, "null argument (q = vT)")):
        mine = [c for c in CASES if c[0].get("epi", BIAS) == epi]
        assert any(c[1].startswith(null_frag) for c in mine) and len(mine) >= 2, epi
    assert len([c for c in CASES if c[0].get("epi") == UNPATCH]) >= 3


def test_last_kernel_record_is_per_thread_and_starts_at_none():
    """mi355_gemm_last_kernel() is a host-side record per thread: a thread that never launched a GEMM reads 0 (none), whatever others did."""
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(_lib.load().mi355_gemm_last_kernel()))
    t.start()
    t.join()
    assert seen == [0]

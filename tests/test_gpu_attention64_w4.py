"""Operator-level tests of the hand-scheduled head_dim-64 static-softmax forward (attn64_w4_kernel, tune key 45; csrc/gen_attn64_w4.py).

Operands, padding, runners and bounds are those of test_gpu_attention_edges.py (reference: tests/_attn_ref.py, float64 attention on the same
bf16-rounded operands).  The kernel rounds P to bf16 before P @ V and O to bf16 on store like the compiler-scheduled kernels (rows within
C_FWD x 2^-8 of the row norm), but sums l from the fp32 exponentials, so its log-sum-exp error is fp32 noise (~1e-6); it is still asserted at
the family's LSE_TOL64, and the measured worst is printed (`pytest -s`).

Shapes: S covers 1 .. 5 key tiles and 8 (the 4-stage ring wraps), the 32-query chain, 64-query wave and 256-query workgroup edges, and
S % 64 in {0, 1, 31, 32, 33, 63}; every S runs the splits n_img in {0, 1, 77, S - 1, S} that fit.  Output buffers carry 8 guard rows behind
each half of the split: they, and the log-sum-exp padding, must still hold the sentinel.
"""
import pytest
import torch

import _attn_ref as R
import test_gpu_attention_edges as E

gpu = pytest.mark.gpu
GUARD = 8
WORST = {"row": 0.0, "rel": 0.0, "lse": 0.0}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import _lib
    return _lib.load()


class key45:
    def __init__(self, lib, v):
        self.lib, self.v = lib, v

    def __enter__(self):
        from mi355_flow import _lib
        _lib.check(self.lib.mi355_tune_set(45, self.v), "tune_set")

    def __exit__(self, *exc):
        self.lib.mi355_tune_set(45, 1)


def run(q, k, vT, S, n_img, bound, lse=False):
    """fwd64 of the edges module with guard rows behind both halves of the split; returns o [B, S, D] (and L)."""
    from mi355_flow import engine
    B, H = q.shape[:2]
    D = H * 64
    full1 = R.filled((B * n_img + GUARD, D), "cuda")
    full2 = R.filled((B * (S - n_img) + GUARD, D), "cuda")
    o1 = full1[:B * n_img] if n_img > 0 else None
    o2 = full2[:B * (S - n_img)] if n_img < S else None
    L = R.filled((B, H, q.shape[2]), "cuda", torch.float32) if lse else None
    engine.op_attention_ex(q, k, vT, S, n_img, True, bound, L, o1, o2)
    torch.cuda.synchronize()
    R.assert_untouched("guard rows behind o_img", full1[B * n_img:])
    R.assert_untouched("guard rows behind o_ctx", full2[B * (S - n_img):])
    o = E.joined(o1, o2, B, S, D, n_img)
    return (o, L) if lse else o


def check(name, o, ref, L=None):
    """check_fwd of the edges module (rows, rel-L2, log-sum-exp and its padding), with the figures kept for the printout"""
    n0 = len(E.REPORT)
    try:
        E.check_fwd(name, o, ref, L, d=64)
    finally:
        for nm, w, r in (E.REPORT[n0:] if "key45=1" in name else []):
            if nm.endswith("lse(abs/max(1,|L|))"):
                WORST["lse"] = max(WORST["lse"], r)
            else:
                WORST["row"], WORST["rel"] = max(WORST["row"], w), max(WORST["rel"], r)
        print(f"  {name}: " + ", ".join(f"{nm.rsplit(' ', 1)[1]} worst {w:.3g} / {r:.3g}" for nm, w, r in E.REPORT[n0:]))


SHAPES = [1, 31, 33, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 320, 449]


@gpu
@pytest.mark.parametrize("S", SHAPES)
def test_fwd64_w4_shapes_and_splits(lib, S):
    B, H = 2, 3
    q, k, v = E.operands("randn", B, H, S, 64)
    qp, kp, vT = E.padded(q, k, v)
    qg, kg, vTg = E.padded(q, k, v, garbage=True)
    ref = R.reference(q, k, v)
    for n_img in sorted({n for n in (0, 1, 77, S - 1, S) if 0 <= n <= S}):
        with key45(lib, 1):
            o, L = run(qp, kp, vT, S, n_img, 60.0, lse=True)
            o2 = run(qp, kp, vT, S, n_img, 60.0)
            og = run(qg, kg, vTg, S, n_img, 60.0)
        assert torch.equal(o, o2), "the LSE and non-LSE instantiations differ"
        assert torch.equal(o, og), "padding leaked into the output"
        check(f"fwd64w4 S={S} n_img={n_img} key45=1", o, ref, L)
        with key45(lib, 0):
            o0, L0 = run(qp, kp, vT, S, n_img, 60.0, lse=True)
        check(f"fwd64w4 S={S} n_img={n_img} key45=0", o0, ref, L0)
    print(f"  worst so far: row {WORST['row']:.3f} x 2^-8, rel-L2 {WORST['rel']:.3e}, log-sum-exp {WORST['lse']:.3e}")


@gpu
@pytest.mark.parametrize("S", [100, 333])
def test_fwd64_w4_scores_at_the_static_bound(lib, S):
    B, H = 1, 2
    q, k, v = E.operands("bound55", B, H, S, 64)
    ref = R.reference(q, k, v)
    assert 50 < ref["max_abs_score"] < 58
    qp, kp, vT = E.padded(q, k, v)
    with key45(lib, 1):
        o, L = run(qp, kp, vT, S, S, 60.0, lse=True)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(L[:, :, :S]).all())
    check(f"fwd64w4 bound55 S={S} key45=1", o, ref, L)

"""Operator-level tests of the backward's streaming / reduction kernels (csrc/backward.hip) through the `mi355_op_*` entry points.

Every kernel is compared, PER ELEMENT, with a plain fp64 torch evaluation of the formula in its header comment (written here; never a second
launch of project code), on bf16-rounded inputs from a seeded generator, at the smallest shapes that reach each branch of its launcher.
Every output buffer is filled with a sentinel first and carries a guard band: whatever lies outside the documented extent must still hold
the sentinel afterwards, documented padding must be exactly 0.

Three kinds of assertion, no norm over a tensor anywhere:

* EXACT (`torch.equal`): copies (transpose, pad-convert, unpatch, the doh / dv gathers, -lse), one exact fp32 product rounded once
  (gate * dx: bf16 x bf16 is exact in fp32), fixed-order fp32 sums (split-K: `s = part[0]; s = s + part[k] ...` in split order).
* SUM BOUND, for fp32 sums of terms that are exact in fp32 (column sums, delta, dgate):
      |got - ref64| <= n * 2^-24 * sum_i |term_i|       (+ 2^-8 * |ref64| for a bf16 output)
  n = number of terms, the sum taken from the fp64 reference: n - 1 additions in ANY order, each with relative error 2^-24 on a partial sum
  that never exceeds sum |term_i|.  A pre-filled output that is accumulated into counts as one more term.
* ARITHMETIC BOUND, for everything with fp32 arithmetic before the rounding (ln_mod_bwd, RMSNorm backward, dw, silu_bwd, gelu_fwd):
      |got - ref64| <= 16 * E                           (+ 2^-8 * |ref64| for a bf16 output)
  E = max |ref32 - ref64| over the tensor, ref32 = the same formula in plain fp32 torch on the same inputs, computed in the test.  The 16
  covers butterfly reduction order, v_rcp / v_exp and atomics in arbitrary order: a few fp32 ulps of the same intermediates as ref32's own.

E observed on MI355X, smallest .. largest over the cases of a family (`pytest -s` prints each figure, and the error, before it asserts):
    ln_mod_bwd dres          1.9e-07 .. 8.0e-07    (largest excess of the error over the bf16 term: 5.3e-08)
    ln_mod_bwd dmod          2.3e-07 .. 6.4e-06    (largest error 4.1e-06)
    silu_bwd                 1.5e-07 .. 1.9e-06    (the error stays inside the bf16 term)
    gelu_fwd                 7.6e-08 .. 3.3e-07    (the error stays inside the bf16 term)
    rms_bwd_gather dq, dk    1.5e-06 .. 7.2e-05    (xhat = y / (w * q_scale) reaches ~50; largest excess over the bf16 term: 2.1e-07)
    rms_bwd_gather dw        1.4e-05 .. 1.8e-04    (largest error 1.7e-04, at E = 1.8e-04)
No family came near 16 E.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 777.0          # finite in bf16 and fp32
GUARD = 64            # elements of guard band behind every output
Q_SCALE = float(torch.tensor(0.125 * 1.4426950408889634, dtype=torch.float32))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def eng(gpu):
    from mi355_flow import engine
    return engine


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rnd(g, *shape, scale=1.0, dtype=torch.bfloat16):
    """bf16-rounded normal values, stored as `dtype`"""
    return (torch.randn(*shape, device="cuda", generator=g) * scale).bfloat16().to(dtype)


def _sent(n, dtype):
    return torch.full((n + GUARD,), SENT, device="cuda", dtype=dtype)


def _is_sent(t):
    return bool((t == SENT).all())


def _sum_bound(got, ref64, abs64, n, what):
    """fp32 sum of n exactly representable terms, any order; bf16 outputs are rounded once more"""
    tol = n * 2.0 ** -24 * abs64
    if got.dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * ref64.abs()
    err = (got.double() - ref64).abs()
    worst = float((err - tol).max())
    print(f"[sum bound] {what}: max err {float(err.max()):.3e}, max tol {float(tol.max()):.3e}, n {n}")
    assert bool((err <= tol).all()), (what, worst, int((err > tol).sum()))


def _arith_bound(got, ref64, ref32, what):
    E = float((ref32.double() - ref64).abs().max())
    tol = torch.full_like(ref64, 16.0 * E)
    if got.dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * ref64.abs()
    err = (got.double() - ref64).abs()
    print(f"[arith bound] {what}: E {E:.3e}, max err {float(err.max()):.3e}, max (err - 2^-8|ref|) {float((err - (tol - 16.0 * E)).max()):.3e}")
    assert bool((err <= tol).all()), (what, E, float((err - tol).max()), int((err > tol).sum()))


# ------------------------------------------------------------------------------------------------- ln_mod_bwd
def _ln_mod_bwd_ref(dt, x, dy, dy2, mod, offs, rps, eps, dres0, want_dmod):
    """g = dy (1 + scale) [+ dy2 (1 + scale2)]; dx = rstd (g - mean g - xhat mean(g xhat)); dshift = sum dy, dscale = sum dy xhat per sample"""
    shift_off, scale_off, shift2_off, scale2_off = offs
    M, D = x.shape
    b = torch.arange(M, device=x.device) // rps
    x, dy, mod = x.to(dt), dy.to(dt), mod.to(dt)
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    xhat = xc * rstd
    g = dy * (1.0 + mod[b, scale_off:scale_off + D])
    if dy2 is not None:
        dy2 = dy2.to(dt)
        g = g + dy2 * (1.0 + mod[b, scale2_off:scale2_off + D])
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    if dres0 is not None:
        dx = dx + dres0.to(dt)
    dmod = None
    if want_dmod:
        nb = mod.shape[0]
        dmod = torch.zeros(nb, mod.shape[1], device=x.device, dtype=dt)
        dmod[:, shift_off:shift_off + D].index_add_(0, b, dy)
        dmod[:, scale_off:scale_off + D].index_add_(0, b, dy * xhat)
        if dy2 is not None:
            dmod[:, shift2_off:shift2_off + D].index_add_(0, b, dy2)
            dmod[:, scale2_off:scale2_off + D].index_add_(0, b, dy2 * xhat)
    return dx, dmod


def _ln_offsets(D):
    return 8, D + 8, 3 * D, 5 * D + 8          # shift, scale, shift2, scale2: distinct, 16-byte aligned, inside mod_ld = 6 D + 8


LN_CASES = [  # D, dmod, dy2, accumulate, M
    (64, 1, 1, 1, 74), (64, 0, 0, 0, 74), (1536, 1, 0, 0, 74), (1536, 0, 1, 1, 74), (2048, 1, 1, 0, 74), (2048, 0, 0, 1, 74),
    (2056, 1, 1, 1, 74), (2056, 0, 1, 0, 74), (4096, 1, 1, 1, 74), (4096, 0, 0, 0, 74), (4104, 0, 1, 1, 74), (5120, 0, 1, 0, 74),
    (6144, 0, 1, 1, 74), (64, 1, 1, 0, 1), (2056, 0, 0, 1, 1),
]


@pytest.mark.parametrize("D,with_dmod,with_dy2,acc,M", LN_CASES)
def test_ln_mod_bwd(eng, D, with_dmod, with_dy2, acc, M):
    rps, eps = 37, 1e-6
    nb = (M + rps - 1) // rps
    mod_ld = 6 * D + 8
    offs = _ln_offsets(D)
    g = _gen(D * 8 + with_dmod * 4 + with_dy2 * 2 + acc + M)
    x = _rnd(g, M, D, scale=2.0) + 1.0
    x = x.bfloat16()
    dy = _rnd(g, M, D)
    dy2 = _rnd(g, M, D) if with_dy2 else None
    mod = _rnd(g, nb, mod_ld, scale=0.5)
    dres = _sent(M * D, torch.bfloat16)
    dres0 = None
    if acc:
        dres0 = _rnd(g, M, D)
        dres[:M * D] = dres0.reshape(-1)
    dmod = dmod0 = None
    if with_dmod:
        dmod = _sent(nb * mod_ld, torch.float32)
        dmod0 = _rnd(g, nb, mod_ld, dtype=torch.float32)          # "ADDED": the buffer arrives non-zero
        dmod[:nb * mod_ld] = dmod0.reshape(-1)
    eng.op_ln_mod_bwd(x, dy, dy2, dres, mod, mod_ld, offs[0], offs[1], offs[2], offs[3], M, D, rps, eps, acc, dmod)
    torch.cuda.synchronize()
    r64, m64 = _ln_mod_bwd_ref(torch.float64, x, dy, dy2, mod, offs, rps, eps, dres0, with_dmod)
    r32, m32 = _ln_mod_bwd_ref(torch.float32, x, dy, dy2, mod, offs, rps, eps, dres0, with_dmod)
    assert _is_sent(dres[M * D:])
    _arith_bound(dres[:M * D].view(M, D), r64, r32, f"ln_mod_bwd dres D={D}")
    if with_dmod:
        assert _is_sent(dmod[nb * mod_ld:])
        got = dmod[:nb * mod_ld].view(nb, mod_ld)
        touched = torch.zeros(mod_ld, dtype=torch.bool, device="cuda")
        for o in (offs[:2] if not with_dy2 else offs):
            touched[o:o + D] = True
        assert torch.equal(got[:, ~touched], dmod0[:, ~touched])      # nothing outside the two / four documented D-wide ranges moved
        _arith_bound(got[:, touched], (m64 + dmod0.double())[:, touched], (m32 + dmod0)[:, touched], f"ln_mod_bwd dmod D={D}")


@pytest.mark.parametrize("D,with_dmod", [(4104, 1), (6152, 0), (6152, 1), (12, 0), (12, 1)])
def test_ln_mod_bwd_refuses_and_writes_nothing(eng, D, with_dmod):
    M, rps = 4, 2
    mod_ld = 6 * D + 8
    offs = _ln_offsets(D // 8 * 8)
    x = torch.ones(M * D + 8, device="cuda", dtype=torch.bfloat16)
    mod = torch.ones(2 * mod_ld, device="cuda", dtype=torch.bfloat16)
    dres = _sent(M * D, torch.bfloat16)
    dmod = _sent(2 * mod_ld, torch.float32) if with_dmod else None
    with pytest.raises(RuntimeError, match="mi355_op_ln_mod_bwd"):
        eng.op_ln_mod_bwd(x, x, None, dres, mod, mod_ld, offs[0], offs[1], offs[2], offs[3], M, D, rps, 1e-6, 0, dmod)
    torch.cuda.synchronize()
    assert _is_sent(dres) and (dmod is None or _is_sent(dmod))


# ------------------------------------------------------------------------------------------------- gate_mul / gate_bwd
@pytest.mark.parametrize("with_dgate", [False, True])
@pytest.mark.parametrize("D,M,rps", [(8, 130, 37), (2056, 130, 37), (8, 64, 64), (2056, 64, 64)])
def test_gate_bwd(eng, D, M, rps, with_dgate):
    nb = (M + rps - 1) // rps
    gate_ld, dg_ld = D + 8, D + 3
    g = _gen(D + M + rps)
    dx, y = _rnd(g, M, D), _rnd(g, M, D)
    gate = _rnd(g, nb + 1, gate_ld)          # one more row than samples: a read of the wrong sample's gate stays inside the tensor
    dy = _sent(M * D, torch.bfloat16)
    dgate = dgate0 = None
    if with_dgate:
        dgate = _sent(nb * dg_ld, torch.float32)
        dgate0 = _rnd(g, nb, dg_ld, dtype=torch.float32)
        dgate[:nb * dg_ld] = dgate0.reshape(-1)
    eng.op_gate_bwd(dx, gate, gate_ld, y if with_dgate else None, dy, dgate, dg_ld, M, D, rps)
    torch.cuda.synchronize()
    b = torch.arange(M, device="cuda") // rps
    assert _is_sent(dy[M * D:])
    assert torch.equal(dy[:M * D].view(M, D), (dx.float() * gate[b, :D].float()).bfloat16())      # one exact fp32 product, rounded once
    if with_dgate:
        assert _is_sent(dgate[nb * dg_ld:])
        got = dgate[:nb * dg_ld].view(nb, dg_ld)
        assert torch.equal(got[:, D:], dgate0[:, D:])
        term = dx.double() * y.double()
        ref = dgate0[:, :D].double().index_add(0, b, term)
        abs_ = dgate0[:, :D].double().abs().index_add(0, b, term.abs())
        _sum_bound(got[:, :D], ref, abs_, min(rps, M) + 1, f"dgate D={D} M={M}")


def test_gate_bwd_refuses_half_a_pair_and_ragged_width(eng):
    t = torch.ones(64, device="cuda", dtype=torch.bfloat16)
    dy = _sent(64, torch.bfloat16)
    dg = _sent(64, torch.float32)
    with pytest.raises(RuntimeError, match="mi355_op_gate_bwd"):
        eng.op_gate_bwd(t, t, 12, None, dy, None, 12, 2, 12, 1)
    with pytest.raises(RuntimeError, match="mi355_op_gate_bwd"):
        eng.op_gate_bwd(t, t, 8, t, dy, None, 8, 2, 8, 1)
    with pytest.raises(RuntimeError, match="mi355_op_gate_bwd"):
        eng.op_gate_bwd(t, t, 8, None, dy, dg, 8, 2, 8, 1)
    torch.cuda.synchronize()
    assert _is_sent(dy) and _is_sent(dg)


# ------------------------------------------------------------------------------------------------- silu_bwd / gelu_fwd
def _act_inputs(n):
    g = _gen(n)
    pre = torch.linspace(-12.0, 12.0, n, device="cuda")
    pre[n // 2] = 0.0
    pre[n // 2 + 1] = -0.0
    pre[1] = -1.28                     # next to the zero of silu'
    pre = pre.bfloat16()
    assert float(pre[0]) == -12.0 and float(pre[-1]) == 12.0 and bool((pre == 0).sum() >= 2)
    return pre, _rnd(g, n)


def _silu_bwd_ref(dt, dy, pre):
    x = pre.to(dt)
    sg = 1.0 / (1.0 + torch.exp(-x))
    return dy.to(dt) * (sg * (1.0 + x * (1.0 - sg)))


def _gelu_ref(dt, pre):
    x = pre.to(dt)
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


@pytest.mark.parametrize("n", [8, 8 * 1000 + 8])
def test_silu_bwd_and_gelu_fwd(eng, n):
    pre, dy = _act_inputs(n)
    dx, out = _sent(n, torch.bfloat16), _sent(n, torch.bfloat16)
    eng.op_silu_bwd(dy, pre, dx, n)
    eng.op_gelu_fwd(pre, out, n)
    torch.cuda.synchronize()
    assert _is_sent(dx[n:]) and _is_sent(out[n:])
    _arith_bound(dx[:n], _silu_bwd_ref(torch.float64, dy, pre), _silu_bwd_ref(torch.float32, dy, pre), f"silu_bwd n={n}")
    _arith_bound(out[:n], _gelu_ref(torch.float64, pre), _gelu_ref(torch.float32, pre), f"gelu_fwd n={n}")


def test_silu_bwd_and_gelu_fwd_refuse_ragged_length(eng):
    pre, dy = _act_inputs(16)
    dx = _sent(16, torch.bfloat16)
    with pytest.raises(RuntimeError, match="mi355_op_silu_bwd"):
        eng.op_silu_bwd(dy, pre, dx, 12)
    with pytest.raises(RuntimeError, match="mi355_op_gelu_fwd"):
        eng.op_gelu_fwd(pre, dx, 12)
    torch.cuda.synchronize()
    assert _is_sent(dx)


# ------------------------------------------------------------------------------------------------- transpose (+ column sums)
def _transpose_expected(inp2d, rows, cols, rows_pad, ld_out, total):
    """the whole output buffer as it must look: sentinel, with [cols][rows_pad] of every ld_out-wide row = in^T | zeros"""
    exp = torch.full((total,), SENT, device="cuda", dtype=torch.bfloat16)
    v = exp[:cols * ld_out].view(cols, ld_out)
    v[:, :rows] = inp2d[:rows, :cols].t()
    v[:, rows:rows_pad] = 0
    return exp


TR_CASES = [  # rows, cols, rows_pad, ld_in, ld_out, input offset
    (64, 64, 64, 64, 64, 0),            # vector
    (100, 72, 128, 72, 128, 0),         # vector
    (100, 70, 128, 72, 128, 0),         # vector, partial-chunk load
    (100, 64, 100, 64, 104, 0),         # vector, store tail
    (37, 5, 37, 5, 37, 0),              # scalar
    (64, 64, 64, 64, 64, 1),            # scalar through misalignment
]


@pytest.mark.parametrize("rows,cols,rows_pad,ld_in,ld_out,off", TR_CASES)
def test_transpose(eng, rows, cols, rows_pad, ld_in, ld_out, off):
    g = _gen(rows * 1000 + cols + off)
    buf = _rnd(g, rows * ld_in + 8)
    inp = buf[off:off + rows * ld_in]
    out = _sent(cols * ld_out, torch.bfloat16)
    eng.op_transpose(inp, ld_in, 0, out, ld_out, 0, rows, cols, rows_pad)
    torch.cuda.synchronize()
    assert torch.equal(out, _transpose_expected(inp.view(rows, ld_in), rows, cols, rows_pad, ld_out, out.numel()))


def test_transpose_batched_with_gaps_between_the_matrices(eng):
    rows, cols, rows_pad, ld_in, ld_out, batch = 100, 72, 128, 72, 128, 3
    bs_in, bs_out = rows * ld_in + 16, cols * ld_out + 24
    g = _gen(3)
    inp = _rnd(g, batch * bs_in)
    out = _sent(batch * bs_out, torch.bfloat16)
    eng.op_transpose(inp, ld_in, bs_in, out, ld_out, bs_out, rows, cols, rows_pad, batch)
    torch.cuda.synchronize()
    for z in range(batch):
        src = inp[z * bs_in:z * bs_in + rows * ld_in].view(rows, ld_in)
        assert torch.equal(out[z * bs_out:(z + 1) * bs_out], _transpose_expected(src, rows, cols, rows_pad, ld_out, bs_out)), z
    assert _is_sent(out[batch * bs_out:])


def test_transpose_refuses_rows_pad_below_rows(eng):
    inp = torch.ones(64 * 64, device="cuda", dtype=torch.bfloat16)
    out = _sent(64 * 64, torch.bfloat16)
    with pytest.raises(RuntimeError, match="mi355_op_transpose"):
        eng.op_transpose(inp, 64, 0, out, 64, 0, 64, 64, 63)
    torch.cuda.synchronize()
    assert _is_sent(out)


TRC_CASES = [  # rows, cols, rows_pad, ld_in, ld_out
    (100, 70, 128, 72, 128),            # vector, partial-chunk load
    (37, 5, 37, 5, 37),                 # scalar
    (200, 72, 200, 72, 200),            # 4 row tiles, the last one ragged
    (64 * 33 + 5, 72, 64 * 34, 72, 64 * 34),      # 34 row tiles: the four-chain loop of the finish
]


def _transpose_colsum(eng, rows, cols, rows_pad, ld_in, ld_out, cs_dtype, finish, seed):
    g = _gen(seed)
    inp = _rnd(g, rows * ld_in)
    ntile = (rows_pad + 63) // 64
    out = _sent(cols * ld_out, torch.bfloat16)
    scratch = _sent(ntile * cols, torch.float32)
    colsum = _sent(cols, cs_dtype)
    eng.op_transpose(inp, ld_in, 0, out, ld_out, 0, rows, cols, rows_pad, 1, scratch, colsum, finish)
    torch.cuda.synchronize()
    src = inp.view(rows, ld_in)
    assert torch.equal(out, _transpose_expected(src, rows, cols, rows_pad, ld_out, out.numel()))
    assert _is_sent(scratch[ntile * cols:]) and _is_sent(colsum[cols:])
    return src, scratch, colsum, ntile


@pytest.mark.parametrize("cs_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,cols,rows_pad,ld_in,ld_out", TRC_CASES)
def test_transpose_colsum(eng, rows, cols, rows_pad, ld_in, ld_out, cs_dtype):
    src, scratch, colsum, ntile = _transpose_colsum(eng, rows, cols, rows_pad, ld_in, ld_out, cs_dtype, True, rows + cols)
    v = src[:rows, :cols].double()
    _sum_bound(colsum[:cols], v.sum(0), v.abs().sum(0), rows, f"transpose_colsum {rows}x{cols} {cs_dtype}")
    # the row-tile partials the finish summed: each the sum of its (up to) 64 rows
    part = scratch[:ntile * cols].view(ntile, cols)
    vp = torch.zeros(ntile * 64, cols, device="cuda", dtype=torch.float64)
    vp[:rows] = v
    vp = vp.view(ntile, 64, cols)
    _sum_bound(part, vp.sum(1), vp.abs().sum(1), 64, f"transpose_colsum partials {rows}x{cols}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,cols,rows_pad,ld_in,ld_out", [TRC_CASES[0], TRC_CASES[3]])
def test_unfinished_transpose_colsum_then_one_launch_reduce_equals_the_two_launches(eng, rows, cols, rows_pad, ld_in, ld_out, dtype):
    _, _, cs2, _ = _transpose_colsum(eng, rows, cols, rows_pad, ld_in, ld_out, dtype, True, rows + cols)
    _, scratch, cs1, ntile = _transpose_colsum(eng, rows, cols, rows_pad, ld_in, ld_out, dtype, False, rows + cols)
    assert _is_sent(cs1)                                                  # finish = false leaves the column sums alone
    nsplit, n = 3, 1000
    part = _rnd(_gen(5), nsplit * n, dtype=torch.float32) + 0.37          # (not bf16-representable sums: the rounding is exercised)
    two, one = _sent(n, dtype), _sent(n, dtype)
    assert eng.op_splitk_reduce(part, n, nsplit, two, n) is True
    assert eng.op_splitk_reduce(part, n, nsplit, one, n, False, scratch, ntile, cols, cs1) is True
    torch.cuda.synchronize()
    assert torch.equal(two[:n], _splitk_ref(part, n, nsplit, n, None, dtype))
    assert torch.equal(one, two) and torch.equal(cs1, cs2)                # guard bands included


@pytest.mark.parametrize("n,out_dtype,cs_dtype", [(1001, torch.float32, torch.float32), (1000, torch.float32, torch.bfloat16),
                                                   (1000, torch.bfloat16, torch.float32)])
def test_one_launch_reduce_reports_not_supported_and_writes_nothing(eng, n, out_dtype, cs_dtype):
    nsplit, nslab, cols = 3, 4, 72
    part = _rnd(_gen(6), nsplit * n, dtype=torch.float32)
    scratch = _rnd(_gen(7), nslab * cols, dtype=torch.float32)
    out, cs = _sent(n, out_dtype), _sent(cols, cs_dtype)
    assert eng.op_splitk_reduce(part, n, nsplit, out, n, False, scratch, nslab, cols, cs) is False
    torch.cuda.synchronize()
    assert _is_sent(out) and _is_sent(cs)
    from mi355_flow import _lib
    assert b"mi355_op_splitk_reduce" in _lib.load().mi355_last_error()
    # no stale bf16 mark survived the refused call: the same buffers now take a plain fp32 reduction
    if out_dtype == torch.float32:
        assert eng.op_splitk_reduce(part, n, nsplit, out, n) is True
        torch.cuda.synchronize()
        assert torch.equal(out[:n], _splitk_ref(part, n, nsplit, n, None, torch.float32)) and _is_sent(out[n:])


# ------------------------------------------------------------------------------------------------- colsum
COLSUM_CASES = [  # M, N, ld, accumulate, dtype
    (1, 8, 8, 0, torch.float32),
    (127, 260, 260, 1, torch.float32),
    (129, 260, 264, 0, torch.bfloat16),            # ld % 8 == 0: vector groups + the last group straddling N on the scalar path
    (129, 1536, 1544, 1, torch.bfloat16),
    (1000, 1536, 1536, 0, torch.float32),
    (1000, 8, 11, 1, torch.bfloat16),
    (127, 1536, 1539, 0, torch.float32),
    (8269, 1536, 1544, 0, torch.float32),          # M >= 8192: 64 slabs; vector ld
    (8269, 260, 263, 1, torch.bfloat16),           # scalar ld
    (8269, 8, 16, 1, torch.float32),
    (129, 260, 268, 1, torch.float32),
]


@pytest.mark.parametrize("M,N,ld,acc,dtype", COLSUM_CASES)
def test_colsum(eng, M, N, ld, acc, dtype):
    g = _gen(M * 7 + N + ld)
    dy = _rnd(g, M * ld)
    scratch = _sent(64 * N, torch.float32)
    out = _sent(N, dtype)
    out0 = _rnd(g, N, scale=3.0, dtype=dtype)
    if acc:
        out[:N] = out0
    eng.op_colsum(dy, ld, M, N, scratch, out, acc)
    torch.cuda.synchronize()
    assert _is_sent(out[N:]) and _is_sent(scratch[64 * N:])
    v = dy.view(M, ld)[:, :N].double()
    ref, abs_ = v.sum(0), v.abs().sum(0)
    if acc:
        ref, abs_ = ref + out0.double(), abs_ + out0.double().abs()
    _sum_bound(out[:N], ref, abs_, M + acc, f"colsum M={M} N={N} ld={ld} {dtype}")


# ------------------------------------------------------------------------------------------------- split-K second stage
def _splitk_ref(part, stride, nsplit, n, out0, dtype):
    """fixed order: s = part[0]; s = s + part[k]; (+ out); rounded once for a bf16 buffer"""
    s = part[0:n].clone()
    for k in range(1, nsplit):
        s = s + part[k * stride:k * stride + n]
    if out0 is not None:
        s = s + out0.float()
    return s.to(dtype)


GRID_CAP = 16384 * 256        # grid_for() in backward.hip: at most 16384 workgroups of 256 threads
SPLITK_CASES = [  # nsplit, n, stride, output advanced by one fp32 element, accumulate, dtype
    (1, 4, 4, 0, 0, torch.float32),
    (3, 1000, 1000, 0, 1, torch.float32),          # vector
    (7, 1000, 1004, 0, 0, torch.bfloat16),         # vector
    (7, 1000, 1004, 0, 1, torch.bfloat16),
    (3, 1000, 1001, 0, 1, torch.bfloat16),         # scalar through the stride
    (7, 1001, 1001, 0, 1, torch.float32),          # scalar through n
    (3, 1001, 1005, 0, 0, torch.bfloat16),
    (3, 1000, 1000, 1, 0, torch.float32),          # scalar through misalignment
    (3, 1000, 1004, 1, 1, torch.bfloat16),
    (1, GRID_CAP + 257, GRID_CAP + 257, 0, 1, torch.float32),      # the grid-stride loop runs twice for 257 threads
]


@pytest.mark.parametrize("nsplit,n,stride,adv,acc,dtype", SPLITK_CASES)
def test_splitk_reduce(eng, nsplit, n, stride, adv, acc, dtype):
    g = _gen(nsplit * 13 + n % 1000 + stride % 1000 + adv)
    part = torch.randn(nsplit * stride, device="cuda", generator=g)          # full fp32 mantissas: the order of the sum matters
    lead = adv * (1 if dtype == torch.float32 else 2)                          # 4 bytes either way
    buf = torch.full((lead + n + GUARD,), SENT, device="cuda", dtype=dtype)
    out = buf[lead:]
    out0 = None
    if acc:
        out0 = _rnd(g, n, scale=2.0, dtype=dtype)
        out[:n] = out0
    assert eng.op_splitk_reduce(part, stride, nsplit, out, n, acc) is True
    torch.cuda.synchronize()
    assert _is_sent(buf[:lead]) and _is_sent(out[n:])
    assert torch.equal(out[:n], _splitk_ref(part, stride, nsplit, n, out0, dtype))


def test_splitk_reduce_refuses_zero_splits(eng):
    part = torch.ones(16, device="cuda")
    out = _sent(16, torch.float32)
    with pytest.raises(RuntimeError, match="mi355_op_splitk_reduce"):
        eng.op_splitk_reduce(part, 16, 0, out, 16)
    torch.cuda.synchronize()
    assert _is_sent(out)


# ------------------------------------------------------------------------------------------------- f32_to_bf16_pad / unpatch_bwd
def test_f32_to_bf16_pad_rounds_to_nearest_even_and_zeroes_the_padding(eng):
    rows, rows_pad, cols = 5, 64, 7
    inp = torch.randn(rows * cols, device="cuda", generator=_gen(1))
    e = 2.0 ** -20
    ties = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 - e, 1 + 2.0 ** -8 + e, 1 + 3 * 2.0 ** -8 - e, 1 + 3 * 2.0 ** -8 + e,
            -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)]
    inp[:len(ties)] = torch.tensor(ties, dtype=torch.float32)
    out = _sent(rows_pad * cols, torch.bfloat16)
    eng.op_f32_to_bf16_pad(inp, out, rows, rows_pad, cols)
    torch.cuda.synchronize()
    assert out[0].item() == 1.0 and out[1].item() == 1 + 2.0 ** -6 and out[2].item() == 1.0 and out[3].item() == 1 + 2.0 ** -7
    assert torch.equal(out[:rows * cols], inp.bfloat16())
    assert bool((out[rows * cols:rows_pad * cols] == 0).all()) and _is_sent(out[rows_pad * cols:])
    with pytest.raises(RuntimeError, match="mi355_op_f32_to_bf16_pad"):
        eng.op_f32_to_bf16_pad(inp, out, rows, rows - 1, cols)


def test_unpatch_bwd_is_the_permutation_of_the_forward(eng):
    Bp, C, hp, wp, p = 2, 16, 3, 5, 2
    dv = torch.randn(Bp, C, hp * p, wp * p, device="cuda", generator=_gen(2))
    n = Bp * hp * wp * p * p * C
    out = _sent(n, torch.bfloat16)
    eng.op_unpatch_bwd(dv, out, Bp, C, hp, wp, p)
    torch.cuda.synchronize()
    # out[(b, ty, tx)][(pp * p + qq) * C + c] = dv[b][c][ty * p + pp][tx * p + qq]
    ref = dv.view(Bp, C, hp, p, wp, p).permute(0, 2, 4, 3, 5, 1).reshape(-1).bfloat16()
    assert torch.equal(out[:n], ref) and _is_sent(out[n:])


# ------------------------------------------------------------------------------------------------- attention backward: prologue
def _token_rows(B, S, n_img, img_rows, ctx_rows, H):
    """token-major image / context rows -> [B][H][S][64] in joint order; a missing stream reads as zeros"""
    D = H * 64
    full = torch.zeros(B, S, D, device="cuda", dtype=torch.bfloat16)
    if n_img > 0 and img_rows is not None:
        full[:, :n_img] = img_rows.view(B, n_img, D)
    if n_img < S and ctx_rows is not None:
        full[:, n_img:] = ctx_rows.view(B, S - n_img, D)
    return full.view(B, S, H, 64).permute(0, 2, 1, 3)


PREP_CASES = [  # B, H, S, n_img, S_pad, do_ctx, o_ctx
    (2, 3, 150, 100, 192, True, True),
    (2, 3, 150, 100, 192, False, True),
    (1, 1, 64, 64, 64, False, False),
    (1, 2, 77, 0, 128, True, True),
    (1, 2, 77, 40, 192, True, True),              # S_pad = roundup64(S) + 64: a whole padding tile beyond the last query tile
]


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("B,H,S,n_img,S_pad,has_do_ctx,has_o_ctx", PREP_CASES)
def test_attn_bwd_prep(eng, B, H, S, n_img, S_pad, has_do_ctx, has_o_ctx, fast):
    from mi355_flow import _lib
    lib = _lib.load()
    g = _gen(S * 10 + n_img + H)
    D, n_ctx = H * 64, S - n_img
    o_img = _rnd(g, B * n_img, D) if n_img else None
    do_img = _rnd(g, B * n_img, D) if n_img else None
    o_ctx = _rnd(g, B * n_ctx, D) if (n_ctx and has_o_ctx) else None
    do_ctx = _rnd(g, B * n_ctx, D) if (n_ctx and has_do_ctx) else None
    lse = _rnd(g, B, H, S_pad, scale=4.0, dtype=torch.float32)
    bhs = B * H * S_pad
    doh, delta, nld = _sent(bhs * 64, torch.bfloat16), _sent(bhs, torch.float32), _sent(bhs * 2, torch.float32)
    assert lib.mi355_tune_set(25, fast) == 0
    try:
        eng.op_attn_bwd_prep(o_img, o_ctx, do_img, do_ctx, lse, doh, delta, nld, B, H, S, S_pad, n_img)
        torch.cuda.synchronize()
    finally:
        lib.mi355_tune_set(25, 1)
    assert _is_sent(doh[bhs * 64:]) and _is_sent(delta[bhs:]) and _is_sent(nld[bhs * 2:])
    doh, delta, nld = doh[:bhs * 64].view(B, H, S_pad, 64), delta[:bhs].view(B, H, S_pad), nld[:bhs * 2].view(B, H, S_pad // 64, 2, 64)
    do_h, o_h = _token_rows(B, S, n_img, do_img, do_ctx, H), _token_rows(B, S, n_img, o_img, o_ctx, H)
    # every row of [S, S_pad) is zero, in all three buffers
    assert bool((doh[:, :, S:] == 0).all()) and bool((delta[:, :, S:] == 0).all())
    nl_rows = nld.permute(0, 1, 3, 2, 4).reshape(B, H, 2, S_pad)          # [.., 0, s] = -lse, [.., 1, s] = -delta
    assert bool((nl_rows[:, :, :, S:] == 0).all())
    assert torch.equal(doh[:, :, :S], do_h)
    assert torch.equal(nl_rows[:, :, 0, :S], -lse[:, :, :S])
    assert torch.equal(nl_rows[:, :, 1, :S], -delta[:, :, :S])
    term = do_h.double() * o_h.double()
    _sum_bound(delta[:, :, :S], term.sum(-1), term.abs().sum(-1), 64, f"delta S={S} n_img={n_img} fast={fast}")
    _sum_bound(nl_rows[:, :, 1, :S], -term.sum(-1), term.abs().sum(-1), 64, f"nld[1] S={S} n_img={n_img} fast={fast}")


# ------------------------------------------------------------------------------------------------- RMSNorm backward + gather
def _rms_ref(dt, y, dy, w, rstd):
    """y, dy [B][S][H][64]; w [64] (already carrying q_scale for q); rstd [B][S][H]: xhat = y / w (0 where |w| <= 1e-20), g = dy w,
    dx = r (g - xhat mean(g xhat)); second result: dy * xhat (the summand of the norm-weight gradient)"""
    y, dy, w, rstd = y.to(dt), dy.to(dt), w.to(dt), rstd.to(dt)
    ok = w.abs() > 1e-20
    xhat = torch.where(ok, y / torch.where(ok, w, torch.ones_like(w)), torch.zeros_like(y))
    gg = dy * w
    dx = rstd.unsqueeze(-1) * (gg - xhat * (gg * xhat).mean(-1, keepdim=True))
    return dx, dy * xhat


@pytest.mark.parametrize("kernel", ["general", "fast", "dw"])
@pytest.mark.parametrize("H", [3, 9])
def test_rms_bwd_gather(eng, H, kernel):
    from mi355_flow import _lib
    lib = _lib.load()
    B, S, n_img, S_pad = 2, 150, 100, 192
    n_ctx, D = S - n_img, H * 64
    g = _gen(H * 3 + len(kernel))
    q, k, dq, dk, dv = (_rnd(g, B, H, S_pad, 64) for _ in range(5))
    rstd_img = (torch.rand(B * n_img, 2 * H, device="cuda", generator=g) * 1.5 + 0.5).bfloat16().float()
    rstd_ctx = (torch.rand(B * n_ctx, 2 * H, device="cuda", generator=g) * 1.5 + 0.5).bfloat16().float()
    nw = [(_rnd(g, 64, scale=0.5, dtype=torch.float32) + 1.0).bfloat16().float() for _ in range(4)]      # q, k, cq, ck
    for i, w in enumerate(nw):
        w[5 + 13 * i] = 0.0                                                  # one exact zero each: the |w| > 1e-20 guard gives xhat = 0
    out_img, out_ctx = _sent(B * n_img * 3 * D, torch.bfloat16), _sent(B * n_ctx * 3 * D, torch.bfloat16)
    nwg = (B * S + 31) // 32
    dw_part = _sent(nwg * 256, torch.float32) if kernel == "dw" else None
    dws = [None] * 4
    if kernel == "dw":
        dws = [_sent(64, torch.float32) for _ in range(4)]
        if H == 3:
            dws[1] = dws[2] = None                                           # NULL for two of the four outputs
    assert lib.mi355_tune_set(25, 0 if kernel == "general" else 1) == 0
    try:
        eng.op_rms_bwd_gather(q, k, dq, dk, dv, rstd_img, rstd_ctx, nw[0], nw[1], nw[2], nw[3], Q_SCALE, out_img, out_ctx, B, H, S, S_pad, n_img,
                              dw_part, *dws)
        torch.cuda.synchronize()
    finally:
        lib.mi355_tune_set(25, 1)
    assert _is_sent(out_img[B * n_img * 3 * D:]) and _is_sent(out_ctx[B * n_ctx * 3 * D:])
    if dw_part is not None:
        assert _is_sent(dw_part[nwg * 256:]) and not bool((dw_part[:nwg * 256] == SENT).any())
    out_img, out_ctx = out_img[:B * n_img * 3 * D].view(B, n_img, 3, H, 64), out_ctx[:B * n_ctx * 3 * D].view(B, n_ctx, 3, H, 64)
    got = torch.cat([out_img, out_ctx], 1)                                   # [B][S][3][H][64] in joint order
    tok = lambda t: t[:, :, :S].permute(0, 2, 1, 3)                          # [B][H][S_pad][64] -> [B][S][H][64]
    assert torch.equal(got[:, :, 2], tok(dv))                                # the dv third is a copy
    rstd = torch.cat([rstd_img.view(B, n_img, 2, H), rstd_ctx.view(B, n_ctx, 2, H)], 1)      # [B][S][2][H]
    img = (torch.arange(S, device="cuda") < n_img).view(1, S, 1, 1)
    res = {}
    for dt in (torch.float64, torch.float32):
        qs = torch.tensor(Q_SCALE, dtype=torch.float32, device="cuda").to(dt)
        wq = torch.where(img, nw[0].to(dt) * qs, nw[2].to(dt) * qs)          # [1][S][1][64]
        wk = torch.where(img, nw[1].to(dt), nw[3].to(dt))
        dxq, sq = _rms_ref(dt, tok(q), tok(dq), wq, rstd[:, :, 0])
        dxk, sk = _rms_ref(dt, tok(k), tok(dk), wk, rstd[:, :, 1])
        dw = [sq[:, :n_img].sum((0, 1, 2)) * qs, sk[:, :n_img].sum((0, 1, 2)), sq[:, n_img:].sum((0, 1, 2)) * qs, sk[:, n_img:].sum((0, 1, 2))]
        res[dt] = (dxq, dxk, dw)
    _arith_bound(got[:, :, 0], res[torch.float64][0], res[torch.float32][0], f"rms_bwd dq H={H} {kernel}")
    _arith_bound(got[:, :, 1], res[torch.float64][1], res[torch.float32][1], f"rms_bwd dk H={H} {kernel}")
    for i, name in enumerate(("dw_q", "dw_k", "dw_cq", "dw_ck")):
        if dws[i] is not None:
            assert _is_sent(dws[i][64:])
            _arith_bound(dws[i][:64], res[torch.float64][2][i], res[torch.float32][2][i], f"rms_bwd {name} H={H}")
            assert float(dws[i][5 + 13 * i]) == 0.0                          # the zero weight's xhat is 0: so is its gradient

"""Operator-level tests of the fused GEMM epilogues (csrc/gemm.hip: `epilogue_part` / `store_row8`) on every kernel family, through
`mi355_op_gemm_epi`.  Same conventions as tests/test_gpu_backward_ops.py: bf16-rounded inputs from a seeded generator (w ~ 1/sqrt(K), a
distinct bias per column, operand rows wider than K), a plain fp64 torch reference written here from the formula of each epilogue (never a
second launch of project code), every output buffer pre-filled with a sentinel and followed by a guard band, and PER-ELEMENT assertions.
Every case asserts the kernel family `mi355_gemm_last_kernel()` reports: a case that the dispatch sends elsewhere fails.

Notation: pre64 = fp64 A.W^T + bias, pre32 = the same in plain fp32 torch, E = max |pre32 - pre64|, delta = 16 E (the project's arithmetic bound).

* DIRECT epilogues (GELU, q/k RMSNorm and its rstd side output) apply fp32 arithmetic to the fp32 sum and round once:
      |got - f(pre64)| <= 2^-8 |f(pre64)| + 16 E_f,      E_f = max |f32(pre32) - f64(pre64)|.
* STAGED epilogues round pre to bf16 once (the LDS staging) and apply the rest, f, to that bf16 value r:
      |got - f(r)| <= 2^-8 |f(r)| + 16 E_f,              E_f = max |f32(r) - f64(r)| (fp32 torch against fp64 on the same, exact, inputs)
  with r = bf16(pre64).  Where pre64 lies within delta of a bf16 rounding boundary the neighbour is accepted as well: r in {bf16(pre64 - delta),
  bf16(pre64 + delta)}; where delta exceeds the spacing of bf16 itself (|pre64| of a few hundred delta: more than two admissible roundings) got
  must lie between f at the two outermost ones, within the same tolerance.  For f = identity (BIAS, V^T, unpatchify, the stash) the
  tolerance is ZERO: got must BE one of the admissible roundings.
  The neighbour rule may rescue at most 1 % of the elements of a case (asserted), and the fp32 torch reference itself -- bf16(pre32)
  against bf16(pre64) -- must stay inside that 1 % too (asserted; also run on the CPU, with bf16(f32(bf16(pre32))) in the kernel's
  place, for all 127 distinct staged cases before the first GPU run: largest share 0.019 %, every case passed).
* What a kernel shows of its own r is used exactly: with a stash, GATE_RES must equal bf16(fma(gate, stash, x)) bit for bit.
* Everything outside the documented extent still holds the sentinel bit for bit: rows >= M, columns [N, ld), q / k rows and V^T tokens
  outside [s_off, s_off + rows_per_sample) of every (b, h), rows of a partial last sample, stash padding, guard bands.
* BIT IDENTITY: for every epilogue, all output buffers of every admissible family equal the 128x128 kernel's, and a re-run's.

Figures observed on MI355X, smallest .. largest over the cases of an epilogue on all families (`pytest -s` prints E, E_f, the largest error in
units of its tolerance and both shares for every check, before it asserts).  K is 64 .. 192 everywhere, so E is that of a short fp32 sum:
    staged       checks  E                    E_f                  neighbour rule used by   (fp32 reference alone)
    bias             17  5.7e-07 .. 2.0e-06   0                    <= 0.012 % of a case     <= 0.015 %
    silu             17  5.7e-07 .. 2.0e-06   2.4e-07 .. 5.1e-07   <= 0.006 %
    posadd           17  5.7e-07 .. 2.0e-06   0 .. 1.2e-07         <= 0.003 %
    addsrc_silu      17  5.7e-07 .. 2.0e-06   3.7e-07 .. 6.5e-07   <= 0.002 %
    gate_res         33  5.2e-07 .. 2.0e-06   6.0e-08 .. 4.8e-07   <= 0.002 %
    dgelu            17  5.7e-07 .. 2.0e-06   8.5e-07 .. 2.5e-06   <= 0.004 %
    stash            34  5.2e-07 .. 2.0e-06   0                    <= 0.012 %
    vT               21  4.8e-07 .. 2.0e-06   0                    <= 0.009 %               <= 0.008 %
    unpatch           3  2.7e-07 .. 7.2e-07   0                    0
  Every element was within its tolerance for an admissible rounding; the largest error is the final bf16 rounding's (0.94 .. 1.00 of the
  tolerance, as in the fp32 emulation on the CPU).  The kernels need the neighbour rule no more often than the fp32 torch reference does:
  they do NOT sit near delta, and the factor 16 was not widened.  (Whether the MFMA's internal adder rounds or truncates stays unmeasured:
  at K <= 192 its sums are as close to fp64 as torch's.)
    direct       checks  E_f                  largest (err - 2^-8 |ref|) / E_f      (allowed: 16)
    gelu             33  6.1e-07 .. 1.8e-06   0.08
    qk_norm          25  8.5e-07 .. 2.7e-06   0.15
    qk rstd_out      13  1.3e-07 .. 2.0e-07   1.00
  Wrong references, tried and not committed: without the staging rounding every POSADD, SILU, GATE_RES and DGELU case fails (ADDSRC_SILU: the
  six largest of 16); with gate[m % rows_per_sample] every GATE_RES case fails.

Two bugs this module found, both fixed with it:
  * EPI_QK_NORM has no column guard, and launch_epi gave N = 128 H with H odd to 256-wide tiles (ping-pong, simple 256x256): two heads that
    do not exist were scattered over the next sample and behind the buffers.  Such grids now run on the 128x128 kernel (cases `-to-simple128`).
  * EPI_DGELU on the guard-free path (ping-pong, 4-wave, 256x192, mid-size whole tiles) was an ulp off the guarded path in a few elements:
    hipcc contracted gelu_tanh' differently in the two instantiations (`test_every_family_gives_the_same_bits[dgelu]`).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"          # (the fp32-reference-only check of the 1 % cap runs these helpers on the CPU)
SENT = 777.0          # finite in bf16 and fp32
GUARD = 64            # elements of guard band behind every output
Q_SCALE = float(torch.tensor(0.125 * 1.4426950408889634, dtype=torch.float32))
CAP = 0.01            # largest share of a case's elements that the either-neighbour rule may rescue

BIAS, SILU, GELU, POSADD, ADDSRC, GATE_RES, QK_NORM, VT, UNPATCH, DGELU = 0, 1, 2, 3, 4, 5, 6, 7, 8, 12
NAMES = {BIAS: "bias", SILU: "silu", GELU: "gelu", POSADD: "posadd", ADDSRC: "addsrc_silu", GATE_RES: "gate_res", QK_NORM: "qk_norm", VT: "vT",
         UNPATCH: "unpatch", DGELU: "dgelu"}
# mi355_tune_set: the shipped defaults of the keys that steer launch_epi, and what sends a launch to each family
DEFAULTS = {0: 1, 3: 128, 19: 3072, 31: 512, 32: 1, 34: 160, 37: 256, 40: 0}
TUNE = {
    "simple128": {3: 1 << 30, 32: 0},        # no grid is large enough for a 256-wide kernel, mid-size kernel off
    "simple256": {0: 0},                     # (from 200 tiles of 256x256)
    "pingpong": {0: 3, 32: 0},               # (from 513 tiles of 128x128: launch_epi's cost rule)
    "w4": {0: 2, 32: 0},                     # (the same rule; whole tiles, K % 128 == 0)
    "256x192": {40: 2, 32: 0},               # wherever it applies: whole tiles, K % 128 == 0
    "mid128x192": {32: 2, 34: 1, 37: 1 << 20},      # wherever it applies: from one tile, no one-round cap
    "mid192x128": {32: 2, 34: 1, 37: 1 << 20},
}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert not torch.backends.cuda.matmul.allow_tf32          # pre32 is PLAIN fp32
    return torch.device("cuda")


@pytest.fixture(scope="module")
def eng(gpu):
    from mi355_flow import engine
    return engine


class _tuned:
    """the dispatch knobs of one family; the shipped defaults again afterwards, whatever happened"""

    def __init__(self, family):
        from mi355_flow import _lib
        self.lib, self.family = _lib.load(), family

    def __enter__(self):
        for k, v in {**DEFAULTS, **TUNE[self.family]}.items():
            assert self.lib.mi355_tune_set(k, v) == 0

    def __exit__(self, *exc):
        for k, v in DEFAULTS.items():
            self.lib.mi355_tune_set(k, v)


# ------------------------------------------------------------------------------------------------- inputs
def _cpu_gen(seed):
    return torch.Generator().manual_seed(seed)          # CPU generator: the same values wherever the helpers run


def _rnd(g, *shape, scale=1.0, dtype=torch.bfloat16):
    """bf16-rounded normal values, stored as `dtype`"""
    return (torch.randn(*shape, generator=g) * scale).bfloat16().to(dtype).to(DEV)


def _sent(n, dtype):
    return torch.full((n + GUARD,), SENT, device=DEV, dtype=dtype)


def _is_sent(t):
    return bool((t == SENT).all())


def _bf(x64):
    return x64.to(torch.bfloat16)


_OPERANDS = {}


def _operands(M, N, K, lda, ldw):
    """A [M][lda], W [N][ldw] (the columns [K, ld) hold values as well: they must not be read), and the product in fp64 and in plain fp32:
    computed once per shape, shared by every case of that shape, never modified"""
    key = (M, N, K, lda, ldw, DEV)
    if key not in _OPERANDS:
        g = _cpu_gen(M * 31 + N * 7 + K + lda + ldw)
        A = _rnd(g, M, lda)
        W = _rnd(g, N, ldw, scale=1.0 / math.sqrt(K))
        acc64 = A[:, :K].double() @ W[:, :K].double().t()
        acc32 = A[:, :K].float() @ W[:, :K].float().t()
        _OPERANDS[key] = (A, W, acc64, acc32)
    return _OPERANDS[key]


_AUX = {}


def _aux(tag, rows, cols, scale=1.0):
    key = (tag, rows, cols, scale, DEV)
    if key not in _AUX:
        _AUX[key] = _rnd(_cpu_gen(len(tag) * 1000003 + rows * 17 + cols), rows, cols, scale=scale)
    return _AUX[key]


# ------------------------------------------------------------------------------------------------- formulas (dt = fp64: reference; fp32: E_f)
def _silu(x):
    return x / (1.0 + torch.exp(-x))


def _gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


def _gelu_grad(x):
    c = math.sqrt(2.0 / math.pi)
    t = torch.tanh(c * (x + 0.044715 * x * x * x))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3.0 * 0.044715 * x * x)


def _qk_ref(dt, pre, nw_q, nw_k, H, eps, q_scale):
    """per (row, 64-column head): rstd = 1/sqrt(mean(pre^2) + eps), y = pre * rstd * nw (* q_scale for q); returns y [M][N], rstd [M][2H]"""
    M = pre.shape[0]
    x = pre.to(dt).view(M, 2 * H, 64)
    rstd = 1.0 / torch.sqrt((x * x).mean(-1) + eps)
    wq = nw_q.to(dt) * (torch.tensor(q_scale, dtype=torch.float32, device=pre.device).to(dt) if q_scale != 0.0 else 1.0)
    w = torch.cat([wq.view(1, 64).expand(H, 64), nw_k.to(dt).view(1, 64).expand(H, 64)], 0)
    return (x * rstd.unsqueeze(-1) * w).reshape(M, 2 * H * 64), rstd


# ------------------------------------------------------------------------------------------------- the two bounds
def _direct(got, ref64, ref32, what):
    """fp32 arithmetic on the fp32 sum, rounded once"""
    E_f = float((ref32.double() - ref64).abs().max())
    tol = torch.full_like(ref64, 16.0 * E_f)
    if got.dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * ref64.abs()
    err = (got.double() - ref64).abs()
    print(f"[direct] {what}: E_f {E_f:.3e}, max err {float(err.max()):.3e}, max (err - 2^-8|ref|) / E_f {float((err - (tol - 16.0 * E_f)).max()) / max(E_f, 1e-300):.2f}")
    assert bool((err <= tol).all()), (what, E_f, float((err - tol).max()), int((err > tol).sum()))


def _more_than_two(r_lo, r_hi):
    """more than two bf16 values in [r_lo, r_hi]: the bit patterns, put in the order of the values, are at least two steps apart"""
    def order(r):
        v = r.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(v >= 0, v, -(v & 0x7FFF))
    return order(r_hi) - order(r_lo) >= 2


def _staged(got, pre64, pre32, f, what):
    """got [M][N] bf16 = bf16(f(bf16(pre))); f maps a tensor r [M][N] of dtype fp64 / fp32 to f(r) in that dtype; f = None: the identity, exact"""
    E = float((pre32.double() - pre64).abs().max())
    delta = 16.0 * E
    r0, r_lo, r_hi = _bf(pre64), _bf(pre64 - delta), _bf(pre64 + delta)
    exact = f is None
    if exact:
        f = lambda r: r
    E_f = 0.0 if exact else float((f(r0.float()).double() - f(r0.double())).abs().max())
    rel = 0.0 if exact else 2.0 ** -8
    g = got.double()

    def excess(r):          # error above the tolerance: <= 0 passes
        F = f(r.double())
        return (g - F).abs() - (rel * F.abs() + 16.0 * E_f), F

    x0, F0 = excess(r0)
    ok0 = x0 <= 0
    ok = ok0
    if not bool(ok0.all()):
        x1, F1 = excess(r_lo)
        x2, F2 = excess(r_hi)
        lo, hi = torch.minimum(F1, F2), torch.maximum(F1, F2)
        between = _more_than_two(r_lo, r_hi) & (g >= lo - (rel * lo.abs() + 16.0 * E_f)) & (g <= hi + (rel * hi.abs() + 16.0 * E_f))
        ok = ok0 | (x1 <= 0) | (x2 <= 0) | between
    used = float((ok & ~ok0).double().mean())
    used32 = float((pre32.bfloat16() != r0).double().mean())          # what the fp32 reference alone would need the rule for
    scale = rel * F0.abs() + 16.0 * E_f
    worst = float(torch.where(ok0 & (scale > 0), (g - F0).abs() / scale.clamp_min(1e-300), torch.zeros_like(g)).max())
    print(f"[staged] {what}: E {E:.3e}, E_f {E_f:.3e}, largest err / tol {worst:.3f}, neighbour share {used:.5f} (fp32 reference: {used32:.5f})")
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError((what, "elements out of bound", int(bad.shape[0]), "first", i, "got", float(g[i]), "f(r)", float(F0[i]),
                              "pre64", float(pre64[i]), "E", E, "E_f", E_f))
    assert used <= CAP and used32 <= CAP, (what, used, used32)


# ------------------------------------------------------------------------------------------------- one case = inputs + launch + checks
class Case:
    def __init__(self, epi, M, N, K, family="simple128", pad_a=0, pad_w=0, ldo_x=0, rps=37, s_off=0, stash_x=None, rstd=False, hd_shift=0,
                 q_scale=0.0, unpatch=None, expect=None):
        self.epi, self.M, self.N, self.K, self.family = epi, M, N, K, family
        self.lda, self.ldw, self.ldo = K + pad_a, K + pad_w, N + ldo_x
        self.rps, self.s_off, self.stash_x, self.rstd, self.hd_shift, self.q_scale = rps, s_off, stash_x, rstd, hd_shift, q_scale
        self.unpatch = unpatch          # (B, hp, wp, patch, out_ch)
        self.expect = expect or family          # the family the dispatch must report under `family`'s knobs
        self.eps = 1e-6

    def __repr__(self):
        s = f"{NAMES[self.epi]}-{self.family}-{self.M}x{self.N}x{self.K}-lda{self.lda}-ldw{self.ldw}-ldo{self.ldo}-rps{self.rps}-off{self.s_off}"
        if self.stash_x is not None:
            s += f"-stash{self.N + self.stash_x}"
        if self.rstd:
            s += "-rstd"
        if self.hd_shift:
            s += f"-hd{1 << self.hd_shift}"
        if self.q_scale:
            s += "-qscale"
        if self.expect != self.family:
            s += "-to-" + self.expect
        return s


def _inputs(c):
    """everything a launch reads; deterministic per case, built once per launch series"""
    M, N, K = c.M, c.N, c.K
    A, W, acc64, acc32 = _operands(M, N, K, c.lda, c.ldw)
    nbias = M if c.epi == VT else N
    bias = _rnd(_cpu_gen(nbias + 5), nbias, scale=0.5, dtype=torch.float32)
    b = bias.view(M, 1) if c.epi == VT else bias.view(1, N)
    inp = dict(A=A, W=W, bias=bias, pre64=acc64 + b.double(), pre32=acc32 + b)
    ld_aux = (N + 7) // 8 * 8 + 8
    inp["ld_aux"] = ld_aux
    if c.epi in (POSADD, ADDSRC):
        inp["aux"] = _aux("table", min(c.rps, M), ld_aux)
    elif c.epi == GATE_RES:
        inp["aux"] = _aux("gate", (M + c.rps - 1) // c.rps + 1, ld_aux)          # one more row than samples: a read of the wrong sample's gate stays inside
        inp["x0"] = _aux("residual", M, N)
    elif c.epi == DGELU:
        inp["aux"] = _aux("preact", M, ld_aux, scale=1.5)
    elif c.epi == QK_NORM:
        g = _cpu_gen(77)
        inp["nw_q"] = (_rnd(g, 64, scale=0.5, dtype=torch.float32) + 1.0).bfloat16().float()
        inp["nw_k"] = (_rnd(g, 64, scale=0.5, dtype=torch.float32) + 1.0).bfloat16().float()
    return inp


def _launch(eng, c, inp):
    """fresh sentinel-filled output buffers, one launch under the family's knobs; returns the buffers"""
    M, N = c.M, c.N
    o = {}
    kw = dict(rows_per_sample=c.rps, eps=c.eps)
    if c.epi in (QK_NORM, VT):
        hd = 64 if c.epi == QK_NORM else (1 << (c.hd_shift or 6))
        H = N // 128 if c.epi == QK_NORM else M // hd
        n_tok = M if c.epi == QK_NORM else N
        B = (n_tok + c.rps - 1) // c.rps
        S_pad = (c.s_off + c.rps + 7) // 8 * 8 + 8
        c.dims = (B, H, hd, S_pad)
        o["q"] = _sent(B * H * S_pad * hd, torch.bfloat16)
        kw.update(q=o["q"], H=H, S_pad=S_pad, s_off=c.s_off, hd_shift=c.hd_shift)
        if c.epi == QK_NORM:
            o["k"] = _sent(B * H * S_pad * 64, torch.bfloat16)
            kw.update(k=o["k"], nw_q=inp["nw_q"], nw_k=inp["nw_k"], q_scale=c.q_scale)
            if c.rstd:
                o["rstd"] = _sent(M * 2 * H, torch.float32)
                kw.update(rstd_out=o["rstd"])
    elif c.epi == UNPATCH:
        B, hp, wp, p, ch = c.unpatch
        o["out"] = _sent(B * ch * hp * p * wp * p, torch.bfloat16)
        kw.update(out=o["out"], hp=hp, wp=wp, patch=p, out_ch=ch)
    else:
        o["out"] = _sent(M * c.ldo, torch.bfloat16)
        if c.epi == GATE_RES:
            o["out"][:M * c.ldo].view(M, c.ldo)[:, :N] = inp["x0"]
        kw.update(out=o["out"], ldo=c.ldo)
        if "aux" in inp:
            kw.update(aux=inp["aux"], ld_aux=inp["ld_aux"])
        if c.stash_x is not None:
            o["stash"] = _sent(M * (N + c.stash_x), torch.bfloat16)
            kw.update(stash=o["stash"], ld_stash=N + c.stash_x)
    with _tuned(c.family):
        family = eng.op_gemm_epi(c.epi, inp["A"], c.lda, inp["W"], c.ldw, M, N, c.K, inp["bias"], **kw)
        torch.cuda.synchronize()
    assert family == c.expect, f"{c!r}: the dispatch launched {family}, not {c.expect}"
    return o


def _rows(buf, M, ld, N, what):
    """[M][N] of a row-major buffer with row stride ld; the columns [N, ld) and the guard band must hold the sentinel"""
    v = buf[:M * ld].view(M, ld)
    assert _is_sent(v[:, N:]) and _is_sent(buf[M * ld:]), f"{what}: written outside [M][N]"
    return v[:, :N]


def _scattered(c, buf, n_tok, what):
    """q / k [B][H][S_pad][64] -> [n_tok][H * 64], vT [B][H][hd][S_pad] -> [H * hd][n_tok]; everything else must hold the sentinel"""
    B, H, hd, S_pad = c.dims
    tok = torch.arange(n_tok, device=buf.device)
    b, s = tok // c.rps, c.s_off + tok % c.rps
    body = buf[:B * H * S_pad * hd]
    assert _is_sent(buf[B * H * S_pad * hd:]), f"{what}: guard band"
    if c.epi == QK_NORM:
        v = body.view(B, H, S_pad, 64)
        got = v[b, :, s, :].reshape(n_tok, H * 64)
        rest = v.clone()
        rest[b, :, s, :] = SENT
    else:
        v = body.view(B, H, hd, S_pad)
        got = v[b, :, :, s].permute(1, 2, 0).reshape(H * hd, n_tok)
        rest = v.clone()
        rest[b, :, :, s] = SENT
    assert _is_sent(rest), f"{what}: written outside [s_off, s_off + rows) of a (b, h)"
    return got


def _after_staging(c, inp):
    """what a staged row-major epilogue applies to r = bf16(pre), [M][N] in r's dtype; None = nothing (exact)"""
    M, N = c.M, c.N
    m = torch.arange(M, device=inp["pre64"].device)
    if c.epi == SILU:
        return _silu
    if c.epi == POSADD:
        return lambda r: r + inp["aux"][m % c.rps, :N].to(r.dtype)
    if c.epi == ADDSRC:
        return lambda r: _silu((r + inp["aux"][m % c.rps, :N].to(r.dtype)).bfloat16().to(r.dtype))
    if c.epi == GATE_RES:
        return lambda r: inp["aux"][m // c.rps, :N].to(r.dtype) * r + inp["x0"].to(r.dtype)
    if c.epi == DGELU:
        return lambda r: r * _gelu_grad(inp["aux"][:M, :N].to(r.dtype))
    assert c.epi in (BIAS, VT, UNPATCH)
    return None


def _check(c, inp, o):
    M, N = c.M, c.N
    pre64, pre32 = inp["pre64"], inp["pre32"]
    what = repr(c)
    if c.epi == QK_NORM:
        B, H, hd, S_pad = c.dims
        got = torch.cat([_scattered(c, o["q"], M, what + " q"), _scattered(c, o["k"], M, what + " k")], 1)
        (y64, r64), (y32, r32) = (_qk_ref(dt, p, inp["nw_q"], inp["nw_k"], H, c.eps, c.q_scale) for dt, p in ((torch.float64, pre64), (torch.float32, pre32)))
        _direct(got, y64, y32, what)
        if c.rstd:
            assert _is_sent(o["rstd"][M * 2 * H:])
            _direct(o["rstd"][:M * 2 * H].view(M, 2 * H), r64, r32, what + " rstd_out")
        return
    if c.epi == VT:
        _staged(_scattered(c, o["q"], N, what), pre64, pre32, None, what)
        return
    if c.epi == UNPATCH:
        B, hp, wp, p, ch = c.unpatch
        n = B * ch * hp * p * wp * p
        assert _is_sent(o["out"][n:])
        # out[b][c][ty * p + pp][tx * p + qq] = pre[(b, ty, tx)][(pp * p + qq) * ch + c]
        got = o["out"][:n].view(B, ch, hp, p, wp, p).permute(0, 2, 4, 3, 5, 1).reshape(M, N)
        _staged(got, pre64, pre32, None, what)
        return
    got = _rows(o["out"], M, c.ldo, N, what)
    m = torch.arange(M, device=got.device)
    if c.epi == GELU:
        _direct(got, _gelu(pre64), _gelu(pre32), what)
    else:
        _staged(got, pre64, pre32, _after_staging(c, inp), what)
    if c.stash_x is not None:
        st = _rows(o["stash"], M, N + c.stash_x, N, what + " stash")
        _staged(st, pre64, pre32, None, what + " stash")
        if c.epi == GATE_RES:       # the kernel's own rounding of pre is visible: one fma, rounded to fp32 and then to bf16 as the kernel does
            want = (inp["aux"][m // c.rps, :N].double() * st.double() + inp["x0"].double()).float().bfloat16()
            assert torch.equal(got, want), what + ": out != bf16(fma(gate, stash, x))"


def _run(eng, c):
    inp = _inputs(c)
    o = _launch(eng, c, inp)
    _check(c, inp, o)
    return inp, o


# ------------------------------------------------------------------------------------------------- the 128x128 kernel: every epilogue, every store path
def _simple128_cases():
    cs = []
    # (K, lda - K, ldw - K, ldo - N, s_off): K = 64 is the single-K-tile case, 192 an odd tile count; ldo = N + 4 takes the scalar store path
    variants = [(64, 8, 16, 4, 0), (128, 0, 0, 0, 5), (192, 16, 8, 8, 0)]
    for epi in (BIAS, SILU, GELU, POSADD, ADDSRC, GATE_RES, DGELU):
        for K, pa, pw, lx, _ in variants:
            # M = 130 = 3 samples of 37 rows + a partial one, two tile rows; N = 136: two tile columns, the second 8 wide
            cs.append(Case(epi, 130, 136, K, pad_a=pa, pad_w=pw, ldo_x=lx))
    for epi in (GELU, GATE_RES):
        for sx in (8, 4):          # ld_stash a multiple of 8 and not; ldo the other way round
            cs.append(Case(epi, 130, 136, 128, pad_a=8, ldo_x=12 - sx, stash_x=sx))
        cs.append(Case(epi, 128, 128, 64, rps=64, stash_x=0))          # one whole tile: the guard-free path of a kernel that has both
    for K, pa, pw, _, so in variants:          # N = 2 * H * 64: H = 1 (q and k in one tile), 3 (k starts inside the second tile column)
        cs.append(Case(QK_NORM, 130, 128 if K == 64 else 384, K, pad_a=pa, pad_w=pw, s_off=so, q_scale=Q_SCALE if K != 128 else 0.0))
        cs.append(Case(QK_NORM, 130, 128 if K == 64 else 384, K, pad_a=pa, pad_w=pw, s_off=so, q_scale=Q_SCALE if K != 128 else 0.0, rstd=True))
    # V^T: M = H << hd features (192 = a whole tile row + half of one), N tokens; rows_per_sample | s_off a multiple of 8 (16-byte stores) and
    # not (scalar); N = 132: the last group of 8 tokens is ragged
    cs.append(Case(VT, 192, 136, 64, pad_a=8, pad_w=16, rps=40, s_off=8))
    cs.append(Case(VT, 256, 132, 128, rps=40, s_off=8, hd_shift=7))
    cs.append(Case(VT, 192, 136, 192, pad_a=16, pad_w=8, rps=37, s_off=5))
    cs.append(Case(VT, 192, 132, 128, rps=37, s_off=0))
    cs.append(Case(VT, 256, 136, 128, rps=40, s_off=3, hd_shift=7))
    for K, pa, pw, _, _ in variants:          # B = 2, 3 x 5 patches of 2 x 2, 16 channels: M = 30, N = 64
        cs.append(Case(UNPATCH, 30, 64, K, pad_a=pa, pad_w=pw, unpatch=(2, 3, 5, 2, 16)))
    return cs


@pytest.mark.parametrize("c", _simple128_cases(), ids=repr)
def test_simple128_every_epilogue(eng, c):
    _run(eng, c)


# ------------------------------------------------------------------------------------------------- the other families
def _epi_case(epi, M, N, K, family, **kw):
    """the epilogue's own arguments for an M x N grid of family `family`"""
    if epi == QK_NORM:
        return [Case(epi, M, N, K, family, q_scale=Q_SCALE, **kw), Case(epi, M, N, K, family, q_scale=Q_SCALE, rstd=True, **kw)]
    if epi in (GELU, GATE_RES):
        return [Case(epi, M, N, K, family, **kw), Case(epi, M, N, K, family, stash_x=8, **kw)]
    return [Case(epi, M, N, K, family, **kw)]


ROWWISE = (BIAS, SILU, GELU, POSADD, ADDSRC, GATE_RES, DGELU)


def _family_cases():
    cs = []
    # ---- mid-size kernel, 128x192 tiles: 64- and 32-column chunks per wave.  N = 384: whole tiles; N = 192 + 40: the second tile column ends
    # inside a wave's first 64-column chunk, N = 192 + 96 + 64 + 24 = 376: inside the 32-column tail chunk of the second wave
    for epi in ROWWISE:
        cs += _epi_case(epi, 256, 384, 64, "mid128x192", rps=64)                          # whole tiles, one K-tile
        cs += _epi_case(epi, 300, 384, 128, "mid128x192", pad_a=8)                        # ragged M, N a multiple of 192
        cs += _epi_case(epi, 256, 232, 192, "mid128x192", pad_w=8)                        # ragged N = 192 + 40
        cs += _epi_case(epi, 130, 376, 128, "mid128x192", ldo_x=4)                        # both, the edge in the 32-column chunk, scalar stores
    # ---- its 192x128 form under V^T (features x tokens)
    cs.append(Case(VT, 384, 256, 128, "mid192x128", rps=128, s_off=8))                    # whole tiles, 16-byte stores
    cs.append(Case(VT, 384, 256, 64, "mid192x128", rps=128, s_off=8, hd_shift=7))
    cs.append(Case(VT, 320, 132, 192, "mid192x128", rps=40, s_off=8))                     # ragged both ways (320 = 192 + 128: the second wave row's 64-row chunk is cut)
    cs.append(Case(VT, 448, 136, 128, "mid192x128", rps=37, s_off=5))                     # scalar stores; 448 = 2 * 192 + 64: a 32-row chunk wholly outside
    # ---- 256x192 kernel: whole tiles only
    for epi in ROWWISE:
        cs += _epi_case(epi, 512, 384, 128, "256x192", rps=200)
    cs += _epi_case(QK_NORM, 512, 384, 256, "256x192", rps=200, s_off=5)
    cs.append(Case(VT, 512, 384, 128, "256x192", rps=192, s_off=8))
    cs.append(Case(VT, 512, 384, 128, "256x192", rps=192, s_off=8, hd_shift=7))
    # ---- the three kernels that launch_epi gives only large grids: > 512 tiles of 128x128 (ping-pong, 4-wave), >= 200 of 256x256 (simple)
    for epi in ROWWISE + (QK_NORM, VT):
        vt = dict(rps=1024, s_off=8) if epi == VT else dict(rps=1000)
        cs += _epi_case(epi, 4352, 2048, 128, "w4", **vt)
        cs += _epi_case(epi, 4352, 2048, 64, "pingpong", **vt)                            # whole tiles, ONE K-tile: every step ends a tile
        if epi == VT:
            cs.append(Case(VT, 4288, 2048, 128, "pingpong", rps=1024, s_off=8))           # ragged M (features: 67 heads)
            cs.append(Case(VT, 4352, 1992, 192, "pingpong", rps=664, s_off=8))            # ragged N
            cs.append(Case(VT, 4352, 1992, 128, "pingpong", rps=996, s_off=0))            # ... and scalar stores
            cs.append(Case(VT, 4352, 4096, 192, "pingpong", rps=1024, s_off=8, hd_shift=7))      # 272 tiles on 256 workgroups
            cs.append(Case(VT, 4352, 3072, 64, "simple256", rps=1024, s_off=8))
            cs.append(Case(VT, 4288, 3072, 128, "simple256", rps=1024, s_off=8))
            cs.append(Case(VT, 4352, 3000, 192, "simple256", rps=1000, s_off=8))
        elif epi == QK_NORM:
            cs += _epi_case(epi, 4230, 2048, 128, "pingpong", rps=1000, s_off=5)
            # N = 128 H with H odd would leave a 256-wide tile two heads that do not exist, and the q / k scatter has no column guard: before
            # this test the ping-pong / simple 256x256 kernels wrote them over the next sample and behind the buffers.  launch_epi now
            # gives such grids to the 128x128 kernel (so no 256-wide kernel has a ragged-N q / k case): asserted, with the sentinels
            cs += _epi_case(epi, 4608, 1920, 192, "pingpong", rps=1000, expect="simple128")      # 15 heads
            cs += _epi_case(epi, 4352, 4096, 192, "pingpong", rps=1000)
            cs += _epi_case(epi, 4352, 3072, 64, "simple256", rps=1000)
            cs += _epi_case(epi, 4230, 3072, 128, "simple256", rps=1000, s_off=5)
            cs += _epi_case(epi, 4352, 2944, 192, "simple256", rps=1000, expect="simple128")     # 23 heads
        else:
            cs += _epi_case(epi, 4230, 2048, 128, "pingpong", pad_a=8, **vt)              # ragged M
            cs += _epi_case(epi, 4352, 1992, 192, "pingpong", pad_w=8, **vt)              # ragged N
            cs += _epi_case(epi, 4352, 4096, 192, "pingpong", **vt)                       # 272 tiles on 256 workgroups: 16 of them run two
            cs += _epi_case(epi, 4352, 3072, 64, "simple256", **vt)
            cs += _epi_case(epi, 4230, 3072, 128, "simple256", ldo_x=4, **vt)
            cs += _epi_case(epi, 4352, 3000, 192, "simple256", **vt)
    return cs


@pytest.mark.parametrize("c", _family_cases(), ids=repr)
def test_every_family_every_epilogue(eng, c):
    _run(eng, c)


# ------------------------------------------------------------------------------------------------- bit identity across the families
IDENTITY = [  # epilogue, M, N, K, families beside the 128x128 anchor, the epilogue's arguments
    (BIAS, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192", "mid128x192"), dict(rps=1000)),
    (SILU, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192", "mid128x192"), dict(rps=1000)),
    (GELU, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192", "mid128x192"), dict(rps=1000, stash_x=8)),
    (POSADD, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192", "mid128x192"), dict(rps=1000)),
    (ADDSRC, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192", "mid128x192"), dict(rps=1000)),
    (GATE_RES, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192", "mid128x192"), dict(rps=1000, stash_x=8)),
    (DGELU, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192", "mid128x192"), dict(rps=1000)),
    (QK_NORM, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192"), dict(rps=1000, s_off=5, q_scale=Q_SCALE, rstd=True)),
    (VT, 4608, 3072, 128, ("simple256", "pingpong", "w4", "256x192", "mid192x128"), dict(rps=1536, s_off=8)),
]


@pytest.mark.parametrize("epi,M,N,K,families,kw", IDENTITY, ids=[NAMES[i[0]] for i in IDENTITY])
def test_every_family_gives_the_same_bits(eng, epi, M, N, K, families, kw):
    """4608 x 3072 (multiples of 768) is whole tiles for every family: 18 x 12 = 216 tiles of 256x256 (the simple 256x256 kernel is reached from
    200; the ping-pong / 4-wave cost rule needs more than 512 tiles of 128x128), 18 x 16 of 256x192, 36 x 16 of 128x192 and 24 x 24 of 192x128
    (the mid-size kernel's one-round cap lifted).  The 128x128 kernel is the anchor and is itself checked against the fp64 reference."""
    anchor = Case(epi, M, N, K, "simple128", **kw)
    inp = _inputs(anchor)
    ref = _launch(eng, anchor, inp)
    _check(anchor, inp, ref)
    for fam in families:
        c = Case(epi, M, N, K, fam, **kw)
        for rerun in range(2):
            o = _launch(eng, c, inp)
            for name in ref:
                assert torch.equal(o[name], ref[name]), (NAMES[epi], fam, name, "re-run" if rerun else "first run")
    if epi == QK_NORM:          # the header's promise: rstd_out does not change the q / k bits
        kw2 = dict(kw, rstd=False)
        for fam in ("simple128",) + families:
            o = _launch(eng, Case(epi, M, N, K, fam, **kw2), inp)
            assert torch.equal(o["q"], ref["q"]) and torch.equal(o["k"], ref["k"]), fam

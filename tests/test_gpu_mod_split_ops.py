"""Operator-level tests of the TWO-GROUP modulation kernels (Wan2.2-TI2V image-to-video: the tokens of frame 0 at their own timestep):
`mi355_op_ln_modulate_split`, `mi355_op_gemm_epi_split` (gated residual), `mi355_op_ln_mod_bwd_split`, `mi355_op_gate_bwd_split`.
With head_rows > 0 token row m reads modulation row

        2 * (m // rows_per_sample) + (m % rows_per_sample >= head_rows)

Conventions, helpers and tolerances are those of tests/test_gpu_gemm_epilogues.py (G) and tests/test_gpu_backward_ops.py (Bk), imported
unchanged: bf16-rounded inputs from seeded generators, fp64 references written here from the formula, sentinel prefill plus guard bands,
per-element assertions, the staged-epilogue tolerance rule with its 1 % cap on the neighbour rule (`G._staged`), the arithmetic bound
16 E (`Bk._arith_bound`).  The modulation tables are random per row, so the two groups of a sample (and neighbouring samples) differ in
every column; they carry one more row than the launch may read, so that a wrong row index stays inside the tensor.

Shapes: rows_per_sample 45 (4 samples, M = 180: a ragged second 128-row tile) and 192 (4 samples, M = 768 = 3 x 256; 3 samples for the
row kernels); head_rows in {1, 15, rows_per_sample - 1, rows_per_sample} (+ 64 at 192).  The split then falls inside an 8-row store group
(1, 44, 191), inside a 16-row MFMA block (15), on a tile boundary (192 + 64 = 256; sample 2 of 192 rows starts at 384 = 3 x 128), inside the
ragged last tile (rows 135 + 1, 135 + 15, 135 + 44 of M = 180) and after the last row of a sample (head_rows == rows_per_sample: only row 2 b).
The gated residual runs on every kernel family that admits the shape, asserted through `mi355_gemm_last_kernel()`:
    M = 180: 128x128, mid 128x192 (N = 376, aligned and scalar stores), ping-pong and simple 256x256 (N = 51200: the grids they need)
    M = 768: 128x128, mid 128x192, 256x192 (N = 384), simple 256x256, ping-pong, 4-wave (N = 17152)
with and without `stash`, all bit-identical to the 128x128 kernel, which is checked against the fp64 formula.

Wrong references, tried once on MI355X and not committed (`_group_row` replaced): the group chosen by `m < head_rows` instead of per sample,
and the two groups swapped.  Every split case of all four operators failed under each of them.
"""

import pytest
import torch

import test_gpu_backward_ops as Bk
import test_gpu_gemm_epilogues as G

pytestmark = pytest.mark.gpu

GATE_RES = G.GATE_RES
SENT, GUARD = G.SENT, G.GUARD


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert not torch.backends.cuda.matmul.allow_tf32
    return torch.device("cuda")


@pytest.fixture(scope="module")
def eng(gpu):
    from mi355_flow import engine
    return engine


def _group_row(m, rps, head_rows):
    """the modulation row of token row m (a tensor of row indices); head_rows == 0: one row per sample"""
    b = m // rps
    if head_rows == 0:
        return b
    return 2 * b + ((m - b * rps) >= head_rows).long()


def _heads(rps):
    return [1, 15, rps - 1, rps] + ([64] if rps == 192 else [])


# ------------------------------------------------------------------------------------------------- gated residual, every family
class Shape:
    def __init__(self, M, N, K, rps, families, ldo_x=0):
        self.M, self.N, self.K, self.rps, self.families, self.ldo_x = M, N, K, rps, families, ldo_x
        self.lda, self.ldw, self.ldo = K + 8, K + 16, N + ldo_x
        self.ld_aux = (N + 7) // 8 * 8 + 8

    def __repr__(self):
        return f"{self.M}x{self.N}x{self.K}-rps{self.rps}-ldo{self.ldo}"


GATE_SHAPES = {
    45: [Shape(180, 376, 128, 45, ("mid128x192",)), Shape(180, 376, 128, 45, ("mid128x192",), ldo_x=4),
         Shape(180, 51200, 64, 45, ("simple256", "pingpong"))],
    192: [Shape(768, 384, 128, 192, ("mid128x192", "256x192")), Shape(768, 17152, 128, 192, ("simple256", "pingpong", "w4"))],
}


def _gate_inputs(s, table_rows):
    A, W, acc64, acc32 = G._operands(s.M, s.N, s.K, s.lda, s.ldw)
    bias = G._rnd(G._cpu_gen(s.N + 5), s.N, scale=0.5, dtype=torch.float32)
    return dict(A=A, W=W, bias=bias, pre64=acc64 + bias.view(1, -1).double(), pre32=acc32 + bias.view(1, -1),
                aux=G._aux("gate2", table_rows, s.ld_aux), x0=G._aux("residual", s.M, s.N))


def _gate_launch(eng, s, inp, family, head_rows, stash, split_entry=True, aux=None):
    M, N = s.M, s.N
    o = {"out": G._sent(M * s.ldo, torch.bfloat16)}
    o["out"][:M * s.ldo].view(M, s.ldo)[:, :N] = inp["x0"]
    kw = dict(out=o["out"], ldo=s.ldo, aux=inp["aux"] if aux is None else aux, ld_aux=s.ld_aux, rows_per_sample=s.rps, eps=1e-6)
    if stash:
        o["stash"] = G._sent(M * (N + 8), torch.bfloat16)
        kw.update(stash=o["stash"], ld_stash=N + 8)
    with G._tuned(family):
        if split_entry:
            got = eng.op_gemm_epi_split(GATE_RES, inp["A"], s.lda, inp["W"], s.ldw, M, N, s.K, inp["bias"], head_rows, **kw)
        else:
            got = eng.op_gemm_epi(GATE_RES, inp["A"], s.lda, inp["W"], s.ldw, M, N, s.K, inp["bias"], **kw)
        torch.cuda.synchronize()
    assert got == family, f"{s!r} head_rows {head_rows}: the dispatch launched {got}, not {family}"
    return o


def _gate_check(s, inp, o, head_rows, stash, what):
    M, N = s.M, s.N
    got = G._rows(o["out"], M, s.ldo, N, what)
    m = torch.arange(M, device=got.device)
    row = _group_row(m, s.rps, head_rows)
    G._staged(got, inp["pre64"], inp["pre32"], lambda r: inp["aux"][row, :N].to(r.dtype) * r + inp["x0"].to(r.dtype), what)
    if stash:
        st = G._rows(o["stash"], M, N + 8, N, what + " stash")
        G._staged(st, inp["pre64"], inp["pre32"], None, what + " stash")
        want = (inp["aux"][row, :N].double() * st.double() + inp["x0"].double()).float().bfloat16()      # the kernel's own rounding of pre is visible
        assert torch.equal(got, want), what + ": out != bf16(fma(gate[group row], stash, x))"


@pytest.mark.parametrize("stash", [False, True], ids=["plain", "stash"])
@pytest.mark.parametrize("rps,head_rows", [(r, h) for r in (45, 192) for h in _heads(r)])
def test_gate_res_split_every_family(eng, rps, head_rows, stash):
    for s in GATE_SHAPES[rps]:
        nb = s.M // rps
        inp = _gate_inputs(s, 2 * nb + 1)
        what = f"gate_res_split {s!r} head_rows {head_rows}" + (" stash" if stash else "")
        ref = _gate_launch(eng, s, inp, "simple128", head_rows, stash)
        _gate_check(s, inp, ref, head_rows, stash, what)
        for fam in s.families:
            o = _gate_launch(eng, s, inp, fam, head_rows, stash)
            for name in ref:
                assert torch.equal(o[name], ref[name]), (what, fam, name, "differs from the 128x128 kernel")


@pytest.mark.parametrize("rps", [45, 192])
def test_gate_res_split_identities(eng, rps):
    """bit for bit: head_rows == 0 through the new entry point is the old entry point; both groups given the same vectors is the old entry point"""
    for s in GATE_SHAPES[rps]:
        nb = s.M // rps
        inp = _gate_inputs(s, 2 * nb + 1)
        one = inp["aux"][:nb + 1].contiguous()                       # one row per sample
        both = one[:nb].repeat_interleave(2, 0).contiguous()         # rows 2 b and 2 b + 1 = sample b's
        both = torch.cat([both, inp["aux"][-1:]], 0).contiguous()
        for fam in ("simple128",) + s.families:
            old = _gate_launch(eng, s, inp, fam, 0, True, split_entry=False, aux=one)
            new0 = _gate_launch(eng, s, inp, fam, 0, True, aux=one)
            for name in old:
                assert torch.equal(new0[name], old[name]), (repr(s), fam, name, "head_rows == 0")
            for h in (1, 15, rps):
                same = _gate_launch(eng, s, inp, fam, h, True, aux=both)
                for name in old:
                    assert torch.equal(same[name], old[name]), (repr(s), fam, name, "equal groups", h)


# ------------------------------------------------------------------------------------------------- LayerNorm-modulate
def _ln_ref(dt, x, shift, scale, row, eps):
    x = x.to(dt)
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    return xc * rstd * (1.0 + scale[row].to(dt)) + shift[row].to(dt)


LN_SHAPES = [(45, 180), (45, 170), (192, 576)]          # (rows_per_sample, M); 170: a partial last sample


@pytest.mark.parametrize("D", [64, 3072, 5120])          # the three instantiations: <= 2048, <= 4096, <= 6144
@pytest.mark.parametrize("rps,M,head_rows", [(r, M, h) for r, M in LN_SHAPES for h in _heads(r)])
def test_ln_modulate_split(eng, rps, M, head_rows, D):
    eps = 1e-6
    nb = (M + rps - 1) // rps
    g = Bk._gen(D * 7 + M + head_rows)
    x = (Bk._rnd(g, M, D, scale=2.0) + 1.0).bfloat16()
    mod = Bk._rnd(g, 2, 2 * nb + 1, D, scale=0.5)          # [shift | scale][rows][D], one allocation
    out = Bk._sent(M * D, torch.bfloat16)
    eng.op_ln_modulate_split(x, mod[0], mod[1], out, M, D, rps, eps, head_rows)
    torch.cuda.synchronize()
    assert Bk._is_sent(out[M * D:])
    row = _group_row(torch.arange(M, device="cuda"), rps, head_rows)
    Bk._arith_bound(out[:M * D].view(M, D), _ln_ref(torch.float64, x, mod[0], mod[1], row, eps), _ln_ref(torch.float32, x, mod[0], mod[1], row, eps),
                    f"ln_modulate_split D={D} rps={rps} M={M} head_rows={head_rows}")


@pytest.mark.parametrize("D", [64, 3072, 5120])
def test_ln_modulate_split_identities(eng, D):
    M, rps, eps = 180, 45, 1e-6
    nb = M // rps
    g = Bk._gen(D + 3)
    x = (Bk._rnd(g, M, D, scale=2.0) + 1.0).bfloat16()
    one = Bk._rnd(g, 2, nb, D, scale=0.5)
    both = one.repeat_interleave(2, 1).contiguous()
    old = eng.op_ln_modulate(x, one[0], one[1], rps, eps)
    new0 = Bk._sent(M * D, torch.bfloat16)
    eng.op_ln_modulate_split(x, one[0], one[1], new0, M, D, rps, eps, 0)
    torch.cuda.synchronize()
    assert torch.equal(new0[:M * D].view(M, D), old) and Bk._is_sent(new0[M * D:])
    for h in (1, 15, rps):
        same = Bk._sent(M * D, torch.bfloat16)
        eng.op_ln_modulate_split(x, both[0], both[1], same, M, D, rps, eps, h)
        torch.cuda.synchronize()
        assert torch.equal(same[:M * D].view(M, D), old), h


# ------------------------------------------------------------------------------------------------- LayerNorm-modulate backward
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("D,with_dy2", [(64, 1), (3072, 0), (5120, 1)])
@pytest.mark.parametrize("rps,M,head_rows", [(r, M, h) for r, M in LN_SHAPES for h in _heads(r)])
def test_ln_mod_bwd_split(eng, rps, M, head_rows, D, with_dy2, acc):
    eps = 1e-6
    nb = (M + rps - 1) // rps
    mod_ld = 6 * D + 8
    offs = Bk._ln_offsets(D)
    g = Bk._gen(D * 8 + with_dy2 * 2 + acc + M + head_rows)
    x = (Bk._rnd(g, M, D, scale=2.0) + 1.0).bfloat16()
    dy = Bk._rnd(g, M, D)
    dy2 = Bk._rnd(g, M, D) if with_dy2 else None
    mod = Bk._rnd(g, 2 * nb + 1, mod_ld, scale=0.5)
    dres = Bk._sent(M * D, torch.bfloat16)
    dres0 = None
    if acc:
        dres0 = Bk._rnd(g, M, D)
        dres[:M * D] = dres0.reshape(-1)
    eng.op_ln_mod_bwd_split(x, dy, dy2, dres, mod, mod_ld, offs[0], offs[1], offs[2], offs[3], M, D, rps, eps, acc, head_rows)
    torch.cuda.synchronize()
    assert Bk._is_sent(dres[M * D:])
    # the reference of tests/test_gpu_backward_ops.py with one modulation row per TOKEN row: rows_per_sample 1 on the gathered table
    per_row = mod[_group_row(torch.arange(M, device="cuda"), rps, head_rows)]
    r64, _ = Bk._ln_mod_bwd_ref(torch.float64, x, dy, dy2, per_row, offs, 1, eps, dres0, False)
    r32, _ = Bk._ln_mod_bwd_ref(torch.float32, x, dy, dy2, per_row, offs, 1, eps, dres0, False)
    Bk._arith_bound(dres[:M * D].view(M, D), r64, r32, f"ln_mod_bwd_split D={D} rps={rps} M={M} head_rows={head_rows} acc={acc}")


@pytest.mark.parametrize("D", [64, 3072, 5120])
def test_ln_mod_bwd_split_identities(eng, D):
    M, rps, eps = 180, 45, 1e-6
    nb = M // rps
    mod_ld = 6 * D + 8
    offs = Bk._ln_offsets(D)
    g = Bk._gen(D + 11)
    x = (Bk._rnd(g, M, D, scale=2.0) + 1.0).bfloat16()
    dy, dy2 = Bk._rnd(g, M, D), Bk._rnd(g, M, D)
    one = Bk._rnd(g, nb, mod_ld, scale=0.5)
    both = one.repeat_interleave(2, 0).contiguous()

    def run(fn, mod, *tail):
        dres = Bk._sent(M * D, torch.bfloat16)
        fn(x, dy, dy2, dres, mod, mod_ld, offs[0], offs[1], offs[2], offs[3], M, D, rps, eps, 0, *tail)
        torch.cuda.synchronize()
        return dres

    old = run(eng.op_ln_mod_bwd, one)
    assert torch.equal(run(eng.op_ln_mod_bwd_split, one, 0), old)
    for h in (1, 15, rps):
        assert torch.equal(run(eng.op_ln_mod_bwd_split, both, h), old), h


# ------------------------------------------------------------------------------------------------- gate backward
@pytest.mark.parametrize("D", [8, 3072])
@pytest.mark.parametrize("rps,M,head_rows", [(r, M, h) for r, M in LN_SHAPES for h in _heads(r)])
def test_gate_bwd_split(eng, rps, M, head_rows, D):
    nb = (M + rps - 1) // rps
    gate_ld = D + 8
    g = Bk._gen(D + M + rps + head_rows)
    dx = Bk._rnd(g, M, D)
    gate = Bk._rnd(g, 2 * nb + 1, gate_ld)
    dy = Bk._sent(M * D, torch.bfloat16)
    eng.op_gate_bwd_split(dx, gate, gate_ld, None, dy, None, 0, M, D, rps, head_rows)
    torch.cuda.synchronize()
    row = _group_row(torch.arange(M, device="cuda"), rps, head_rows)
    assert Bk._is_sent(dy[M * D:])
    assert torch.equal(dy[:M * D].view(M, D), (dx.float() * gate[row, :D].float()).bfloat16())      # one exact fp32 product, rounded once


def test_gate_bwd_split_identities(eng):
    M, rps, D = 180, 45, 3072
    nb = M // rps
    g = Bk._gen(5)
    dx = Bk._rnd(g, M, D)
    one = Bk._rnd(g, nb, D + 8)
    both = one.repeat_interleave(2, 0).contiguous()

    def run(fn, gate, *tail):
        dy = Bk._sent(M * D, torch.bfloat16)
        fn(dx, gate, D + 8, None, dy, None, 0, M, D, rps, *tail)
        torch.cuda.synchronize()
        return dy

    old = run(eng.op_gate_bwd, one)
    assert torch.equal(run(eng.op_gate_bwd_split, one, 0), old)
    for h in (1, 15, rps):
        assert torch.equal(run(eng.op_gate_bwd_split, both, h), old), h


# ------------------------------------------------------------------------------------------------- what stays refused
def test_modulation_gradients_of_a_split_table_are_refused(eng):
    """dmod / dgate together with head_rows > 0: an error, nothing is written"""
    M, rps, D = 8, 4, 64
    mod_ld = 6 * D + 8
    offs = Bk._ln_offsets(D)
    t = torch.ones(M * D, device="cuda", dtype=torch.bfloat16)
    mod = torch.ones(5 * mod_ld, device="cuda", dtype=torch.bfloat16)
    dres, dmod = Bk._sent(M * D, torch.bfloat16), Bk._sent(4 * mod_ld, torch.float32)
    with pytest.raises(RuntimeError, match="mi355_op_ln_mod_bwd_split.*dmod"):
        eng.op_ln_mod_bwd_split(t, t, None, dres, mod, mod_ld, offs[0], offs[1], offs[2], offs[3], M, D, rps, 1e-6, 0, 2, dmod)
    dy, dg = Bk._sent(M * D, torch.bfloat16), Bk._sent(4 * D, torch.float32)
    with pytest.raises(RuntimeError, match="mi355_op_gate_bwd_split.*dgate"):
        eng.op_gate_bwd_split(t, mod, D, t, dy, dg, D, M, D, rps, 2)
    with pytest.raises(RuntimeError, match="mi355_op_gate_bwd_split.*head_rows"):
        eng.op_gate_bwd_split(t, mod, D, None, dy, None, 0, M, D, rps, rps + 1)
    with pytest.raises(RuntimeError, match="mi355_op_ln_modulate_split.*head_rows"):
        eng.op_ln_modulate_split(t, mod, mod[D:], dres, M, D, rps, 1e-6, rps + 1)
    torch.cuda.synchronize()
    assert Bk._is_sent(dres) and Bk._is_sent(dmod) and Bk._is_sent(dy) and Bk._is_sent(dg)

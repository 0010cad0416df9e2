"""Bit identity of the tile-uniform GEMM epilogues (csrc/gemm.hip, `mi355_tune_set` key 46) against the general ones.

With key 46 = 1 (default) the two persistent 256x256 kernels (ping-pong, 4-wave) run builds whose epilogues address a tile from scalar base
pointers and per-tile lane offsets and take the sample index -- the gate row, the batch index of the q / k / V^T scatters -- once per tile;
the launcher selects them only for whole tiles that each lie inside one sample (and, on the 4-wave kernel, only for the epilogues that look
at the sample: its bias / GELU launches run the general build under both keys).  Key 46 = 0 runs the general epilogues everywhere.  Nothing in
the value path differs, so every output buffer -- out, the stash, q, k, V^T, rstd_out, INCLUDING its padding columns, the rows of the scatter
targets outside [s_off, s_off + rows_per_sample) and the guard band behind it, all pre-filled with a sentinel -- must be `torch.equal` under
the two keys.  Each case also equals the 128x128 kernel at key 46 = 0 (which tests/test_gpu_gemm_epilogues.py holds against the fp64
formulas): the two keys cannot be equal by both being wrong.  Every launch asserts the kernel family `mi355_gemm_last_kernel()` reports AND
whether it ran a tile-uniform build (`mi355_gemm_last_epilogue_tile_uniform()`), against `_expect_tile_uniform`, the selection rule written
out here from the documented contract: a shape that should take the new code and silently ran the general one fails, and so does the reverse.

Helpers, inputs and sentinels are those of tests/test_gpu_gemm_epilogues.py (G), imported unchanged.

Shapes.  launch_epi gives a grid to the ping-pong / 4-wave kernels only from 128 tiles of 256x256 that are more than 512 tiles of 128x128, so
the edges below sit in the smallest grids those kernels can be reached with (65 .. 130 tile rows of 2 .. 1 tile columns); the families that
run the general epilogues under both keys (simple 256x256, 256x192, both mid-size forms) get the same edges at M = 512 / 768 where their
dispatch admits it.  What each shape can catch:
  * rows_per_sample 256: the tile edge IS the sample edge -- the gate row and the batch index must change from one tile to the next;
  * rows_per_sample 512, s_off 8, S_pad > rows, ldo > N: the scatter offset and the row strides;
  * rows_per_sample 384: every second tile straddles two samples -- the launch must take the general kernels;
  * rows_per_sample 333, M = 50 x 333: ragged, the general kernels (the 4-wave kernel does not admit the grid: the ping-pong kernel runs);
  * N = 256 with H = 2: the q | k boundary in the middle of ONE tile (is_k differs between a wave's column halves); N = 512 with H = 4;
  * V^T (tokens are the columns): 512 tokens of 256 / 512 per sample, 768 tokens of 384 (straddle), 668 of 334 (ragged, scalar stores);
  * K = 128 (one K pair of the 4-wave loop) and K = 256;
  * the two-group gate table (head_rows 64) has no tile-uniform build: general kernels under both keys.
"""
import pytest
import torch

import test_gpu_gemm_epilogues as G

pytestmark = pytest.mark.gpu

KEY = 46
BIAS, GELU, POSADD, GATE_RES, QK_NORM, VT = G.BIAS, G.GELU, G.POSADD, G.GATE_RES, G.QK_NORM, G.VT


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mi355_flow import engine
    return engine


@pytest.fixture(autouse=True)
def _default_key_afterwards():
    yield
    from mi355_flow import _lib
    _lib.load().mi355_tune_set(KEY, 1)


# (name, epilogue, Case arguments, head_rows)
EPILOGUES = [
    ("bias", BIAS, {}, 0),
    ("gelu", GELU, {}, 0),
    ("gelu-stash", GELU, dict(stash_x=8), 0),
    ("posadd", POSADD, {}, 0),
    ("gate_res", GATE_RES, {}, 0),
    ("gate_res-stash", GATE_RES, dict(stash_x=8), 0),
    ("gate_res-split64", GATE_RES, {}, 64),
    ("qk_norm", QK_NORM, dict(q_scale=G.Q_SCALE), 0),
    ("qk_norm_rstd", QK_NORM, dict(q_scale=G.Q_SCALE, rstd=True), 0),
]
# row-wise and q | k shapes: (M, N, K, Case arguments, ((family knobs, family that must run), ...))
BOTH = (("pingpong", "pingpong"), ("w4", "w4"))
ROW_SHAPES = [
    (16640, 512, 256, dict(rps=256), BOTH),
    (33280, 256, 128, dict(rps=256), BOTH),
    (16896, 512, 128, dict(rps=512, s_off=8, ldo_x=8), BOTH),
    (16896, 512, 128, dict(rps=384), BOTH),
    (16650, 512, 128, dict(rps=333), (("pingpong", "pingpong"), ("w4", "pingpong"))),
    (25600, 512, 128, dict(rps=256), (("simple256", "simple256"),)),
    (512, 384, 128, dict(rps=256), (("256x192", "256x192"), ("mid128x192", "mid128x192"))),
    (768, 384, 256, dict(rps=384, s_off=8), (("256x192", "256x192"), ("mid128x192", "mid128x192"))),
]
# V^T: M features, N token columns
VT_SHAPES = [
    (16640, 512, 128, dict(rps=256), BOTH),
    (16640, 512, 256, dict(rps=512, s_off=8), BOTH),
    (11264, 768, 128, dict(rps=384, s_off=8), BOTH),
    (11264, 668, 128, dict(rps=334), (("pingpong", "pingpong"), ("w4", "pingpong"))),          # (the operator wants N % 4 == 0: 334, not 333)
    (25600, 512, 128, dict(rps=256), (("simple256", "simple256"),)),
    (512, 384, 128, dict(rps=192, s_off=8), (("256x192", "256x192"),)),
    (384, 512, 128, dict(rps=256), (("mid192x128", "mid192x128"),)),
    (384, 768, 128, dict(rps=384, s_off=8), (("mid192x128", "mid192x128"),)),
]


def _launch(eng, c, inp, key, head_rows):
    """fresh sentinel-filled buffers, one launch under the family's knobs and key 46 = `key`; returns the buffers and the family that ran"""
    from mi355_flow import _lib
    M, N = c.M, c.N
    o, kw = {}, dict(rows_per_sample=c.rps, eps=c.eps)
    if c.epi in (QK_NORM, VT):
        hd = 64
        H = N // 128 if c.epi == QK_NORM else M // hd
        n_tok = M if c.epi == QK_NORM else N
        B = (n_tok + c.rps - 1) // c.rps
        S_pad = (c.s_off + c.rps + 7) // 8 * 8 + 8
        c.dims = (B, H, hd, S_pad)
        o["q"] = G._sent(B * H * S_pad * hd, torch.bfloat16)
        kw.update(q=o["q"], H=H, S_pad=S_pad, s_off=c.s_off)
        if c.epi == QK_NORM:
            o["k"] = G._sent(B * H * S_pad * 64, torch.bfloat16)
            kw.update(k=o["k"], nw_q=inp["nw_q"], nw_k=inp["nw_k"], q_scale=c.q_scale)
            if c.rstd:
                o["rstd"] = G._sent(M * 2 * H, torch.float32)
                kw.update(rstd_out=o["rstd"])
    else:
        o["out"] = G._sent(M * c.ldo, torch.bfloat16)
        if c.epi == GATE_RES:
            o["out"][:M * c.ldo].view(M, c.ldo)[:, :N] = inp["x0"]
        kw.update(out=o["out"], ldo=c.ldo)
        if "aux" in inp:
            kw.update(aux=inp["aux"], ld_aux=inp["ld_aux"])
        if c.stash_x is not None:
            o["stash"] = G._sent(M * (N + c.stash_x), torch.bfloat16)
            kw.update(stash=o["stash"], ld_stash=N + c.stash_x)
    lib = _lib.load()
    with G._tuned(c.family):
        assert lib.mi355_tune_set(KEY, key) == 0
        if head_rows:
            ran = eng.op_gemm_epi_split(c.epi, inp["A"], c.lda, inp["W"], c.ldw, M, N, c.K, inp["bias"], head_rows, **kw)
        else:
            ran = eng.op_gemm_epi(c.epi, inp["A"], c.lda, inp["W"], c.ldw, M, N, c.K, inp["bias"], **kw)
        torch.cuda.synchronize()
        tu = lib.mi355_gemm_last_epilogue_tile_uniform()
        lib.mi355_tune_set(KEY, 1)
    return o, ran, tu


def _expect_tile_uniform(c, ran, key, head_rows):
    """the documented selection (include/mi355_flow.h, key 46): ping-pong / 4-wave launches of whole tiles that each lie inside one sample"""
    if key == 0 or ran not in ("pingpong", "w4") or c.M % 256 or c.N % 256 or head_rows or c.epi == POSADD:
        return 0
    if c.epi in (BIAS, GELU):
        return int(ran == "pingpong" and c.ldo % 8 == 0)          # (the 4-wave kernel has no such build for the bias-type epilogues)
    if c.epi == VT:
        return int(c.rps % 256 == 0 and c.s_off % 8 == 0)
    return int(c.rps % 256 == 0)          # gated residual, q | k


def _extent(c, o, what):
    """nothing outside the documented extent of any output is written"""
    M, N = c.M, c.N
    if c.epi == QK_NORM:
        G._scattered(c, o["q"], M, what + " q")
        G._scattered(c, o["k"], M, what + " k")
        if c.rstd:
            assert G._is_sent(o["rstd"][M * 2 * c.dims[1]:]), what + " rstd_out: guard band"
    elif c.epi == VT:
        G._scattered(c, o["q"], N, what)
    else:
        G._rows(o["out"], M, c.ldo, N, what)
        if c.stash_x is not None:
            G._rows(o["stash"], M, N + c.stash_x, N, what + " stash")


def _one(eng, epi, M, N, K, kw, head_rows, families):
    anchor = G.Case(epi, M, N, K, "simple128", **kw)
    inp = G._inputs(anchor)
    if head_rows:          # two gate rows per sample (+ one: a wrong row index stays inside the tensor)
        inp["aux"] = G._aux("gate2", 2 * ((M + anchor.rps - 1) // anchor.rps) + 1, inp["ld_aux"])
    ref, ran, tu = _launch(eng, anchor, inp, 0, head_rows)
    assert ran == "simple128" and tu == 0, (repr(anchor), ran, tu)
    _extent(anchor, ref, repr(anchor))
    for fam, expect in families:
        c = G.Case(epi, M, N, K, fam, **kw)
        outs = {}
        for key in (0, 1):
            outs[key], ran, tu = _launch(eng, c, inp, key, head_rows)
            assert ran == expect, f"{c!r} key {KEY} = {key}: the dispatch launched {ran}, not {expect}"
            assert tu == _expect_tile_uniform(c, ran, key, head_rows), f"{c!r} key {KEY} = {key}: tile-uniform build {tu}"
        _extent(c, outs[1], f"{c!r} key {KEY} = 1")
        for name in ref:
            assert torch.equal(outs[1][name], outs[0][name]), (repr(c), name, f"key {KEY} = 1 differs from key {KEY} = 0")
            assert torch.equal(outs[0][name], ref[name]), (repr(c), name, f"key {KEY} = 0 differs from the 128x128 kernel")


@pytest.mark.parametrize("M,N,K,kw,families", ROW_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-rps{s[3]['rps']}" for s in ROW_SHAPES])
@pytest.mark.parametrize("name,epi,ekw,head_rows", EPILOGUES, ids=[e[0] for e in EPILOGUES])
def test_both_keys_give_the_same_bits(eng, name, epi, ekw, head_rows, M, N, K, kw, families):
    if epi == QK_NORM:
        # a q | k launch has N = 128 H: the mid-size kernel does not take it, and a 256-wide kernel only even H
        families = tuple(f for f in families if not f[0].startswith("mid"))
        if N % 256:
            families = tuple(f for f in families if f[0] == "256x192")
        kw = {k: v for k, v in kw.items() if k != "ldo_x"}
    else:
        kw = dict(kw, s_off=0)
    _one(eng, epi, M, N, K, dict(kw, **ekw), head_rows, families)


@pytest.mark.parametrize("M,N,K,kw,families", VT_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-rps{s[3]['rps']}" for s in VT_SHAPES])
def test_both_keys_give_the_same_bits_vT(eng, M, N, K, kw, families):
    _one(eng, VT, M, N, K, kw, 0, families)

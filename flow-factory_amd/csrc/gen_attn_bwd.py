#!/usr/bin/env python3
"""Generator of the software-pipelined main loops of the flash-attention BACKWARD: the dK/dV pass (one key per lane, query tiles streamed)
and the dQ pass (one query per lane, key tiles streamed), in three variants that share ONE schedule:

    64     csrc/attn_bwd64_asm.inc    head_dim 64, 32 rows per wave, two waves per SIMD           (attention_bwd.hip)
    64x2   csrc/attn_bwd64x2_asm.inc  head_dim 64, two 32-row blocks per wave, one wave per SIMD  (attention_bwd.hip)
    128    csrc/attn_bwd128_asm.inc   head_dim 128, one wave per SIMD, tail masks                 (attention128_bwd.hip)

The schedule.  Per 32-row half tile h a wave runs  A: the S and dP chains (MFMAs)  ->  V: 16 v_exp + 8 v_pk_mul + 8..16 v_cvt_pk  ->
B: the second products (MFMAs).  Written as C++ these are three serial phases per wave -- a wave issues in order, so while it sits in front
of an MFMA waiting for the matrix pipe it cannot issue the VALU work that follows.  Here the phases of THREE consecutive halves are
interleaved in program order:

    body(h) =   B(h-1)   ||   V(h)   ||   A(h+1)          one MFMA, then the fillers of its gap, then the next MFMA ...

so every MFMA gap carries VALU / LDS work of another half and the matrix pipe is fed back to back by ONE wave.  S / dP of consecutive halves
alternate between two register buffers X and Y.

The ring.  Tiles arrive by LDS-DMA loads (lds_dma, stage) into a 4-slot LDS ring, three tiles ahead; the loop ALWAYS issues a tile's loads
(past the end it re-loads the last tile into a slot nobody reads) so that `s_waitcnt vmcnt(N)` has one N.

Bit identity.  Same MFMAs, same operand order and the same accumulation order per output element as the C++ kernels of the same pass: the
results are BIT-IDENTICAL in every variant (tests/test_gpu_backward.py and tests/test_gpu_flux_backward.py compare them).

How this file is organised.  The schedule exists once: ring_step, sync, body, main_loop, check and main below.  A variant is a description
(variant_64, variant_64x2, variant_128; each docstring has the variant's why and its fixed register map): a few plain facts plus a dkv and
a dq pass table holding the MFMA operand tables (mf_A, mf_B), the LDS read lists (rd_A, rd_T), the VALU gap placement (valu) and their gap
lists.  The registers are fixed: the C++ shell sees clobber lists only.  A new variant is one more such function and one more VARIANTS
entry (plus its Makefile rule and its line in tests/test_generated_asm.py).

usage: python gen_attn_bwd.py {64|64x2|128} > attn_bwd<variant>_asm.inc      (the Makefile does this; the .inc files are committed)
"""
import re
import sys
from collections import defaultdict
from types import SimpleNamespace as NS

from asmgen import ar, clobbers, emit, read_acc_macros, regs, sr, vr

X = 16                                 # S / dP buffer of the even halves (every variant); V.Y: of the odd halves
# scalar registers (clobbered)
S_B0, S_B1, S_B2 = 70, 72, 74          # 64-bit source bases of the streamed operands (next tile to load)
S_NT, S_CNT, S_LT, S_LDSL, S_STA, S_STT, S_D, S_M0, S_EX, S_W1K, S_WNL, S_INC, S_T = 76, 77, 78, 79, 80, 81, 82, 83, 84, 86, 87, 88, 89
S_B0H, S_B1H = 90, 92                  # the same bases + half a tile (rows +32: this wave's second 8-row group; the instruction offset field ends at 4095)

V = None          # the variant being emitted
ABL = set()       # ablation builds (timing only, results garbage): "novalu", "nolds", "nosync"; only a variant's `ablations` fill it


# ---------------------------------------------------------------------------------------------------------------- instruction formatters

def mfma(d, a, b, c=None):
    return f"v_mfma_f32_32x32x16_bf16 {d}, {a}, {b}, {c or d}"


def v_exp(r):
    return f"v_exp_f32 {vr(r)}, {vr(r)}"


def pk_mul(dp, s):                     # dZ pair = dP pair * P pair, in place
    return f"v_pk_mul_f32 {vr(dp, 2)}, {vr(dp, 2)}, {vr(s, 2)}"


def cvt_pk(dst, src):
    return f"v_cvt_pk_bf16_f32 {vr(dst)}, {vr(src)}, {vr(src + 1)}"


def lds_dma(g, base, off=0):
    return f"global_load_lds_dwordx4 %[{g}], {sr(base)}" + (f" offset:{off}" if off else "")


# ------------------------------------------------------------------------------------------------- table pieces that several passes share

def chains(n, nk, frag, rows, c0=()):
    """mf_A: the S and dP chains (w = 0, 1) of every row block b into v[n + 32 b + 16 w ...], nk k-steps each: k-step kk multiplies the
    streamed fragment at frag = (vr | ar, base) + 4 nk w + 4 kk by the lane's row fragment a[rows[b] + 4 nk w + 4 kk ...].  c0[b]: where
    the first k-step takes -L | -Delta as its C operand from (vdst != src2) instead of finding them in the buffer."""
    F, fb = frag
    out = []
    for kk in range(nk):
        for b, row in enumerate(rows):
            for w in range(2):
                d = vr(n + 32 * b + 16 * w, 16)
                c = vr(c0[b] + 16 * w, 16) if c0 and kk == 0 else d
                out.append(mfma(d, F(fb + 4 * nk * w + 4 * kk, 4), ar(row + 4 * nk * w + 4 * kk, 4), c))
    return out


def rd_nld(dst, qb):
    """dK/dV pass: the C operands (-L | -Delta of the half's 32 queries) into v[dst : dst + 32)"""
    return [f"ds_read_b128 {vr(dst + 16 * w + 4 * i, 4)}, %[la] offset:{256 * w + o + 128 * qb}" for w in range(2) for i, o in enumerate((0, 16, 64, 80))]


def derived(DR):
    """Read addresses kept in registers instead of derived at use.  Fragment kk sits at 16-byte chunk (2 kk + lg) ^ swizzle(row) =
    chunk(kk = 0) ^ 2 kk: its address is r0 ^ 32 kk (ring slots are multiples of 512 bytes); piece db = 1 of a transposed read is
    chunk ^ 4 = address ^ 64.  v[DR : DR + 3) = r0 ^ 32 kk (kk = 1..3), v[DR + 3], v[DR + 4] = a0 / a1 ^ 64; re-derived by ring_step.
    -> (raddr, taddr, derive_A, derive_T)"""
    return (lambda kk: "%[r0]" if kk == 0 else vr(DR + kk - 1), lambda i: f"%[a{i}]" if i < 2 else vr(DR + 3 + i - 2),
            [f"v_xor_b32 {vr(DR + k - 1)}, {32 * k}, %[r0]" for k in (1, 2, 3)], [f"v_xor_b32 {vr(DR + 3)}, 64, %[a0]", f"v_xor_b32 {vr(DR + 4)}, 64, %[a1]"])


# ------------------------------------------------------------------------------------------------------------------------- the variants
# A variant:  prefix (of its macros), Y, TILE (bytes of one operand tile; rows +32 are TILE / 2 on), pieces (the (base, instruction offset) of
#   the LDS-DMA loads a wave issues per tile), nblk (32-row blocks per wave), readers (MFMAs of B per packed register group: check),
#   masked_last (an unmasked steady loop plus a separately masked last iteration) with MK, t_extra (more instructions of the transposed-side
#   ring step), ablations ((macro tag, ABL) builds of the dK/dV loop), sregs (scalar clobbers), read_acc (read-out bases), header, passes.
# A pass:  name (in macros), label (in asm labels), nld_ring (-L | -Delta belong to the streamed rows: a third source base, 512 more bytes per
#   ring slot) or splat ((first register, operand names) per block: they are the lane's own), nacc (accumulators to zero), rows (the row-load
#   table: per block (VGPR, global offset operand, pointer operand, byte offset, AGPR) of each 4-register fragment), vhi / ahi (clobbers
#   v[16:vhi), a[0:ahi)), mf_A(n) / mf_B() with nA / nB (the MFMAs), rd_A(n, qb) / rd_T(qb) with rdA_gaps / rdT_gaps (the LDS reads and the
#   gap each sits in), valu(c, qb, masked) ({gap: [VALU instructions]}), a_addrs / t_addrs (address operands a ring step moves) with
#   derive_A / derive_T (addresses re-derived from them; none where they are formed at use), and what check() expects: PZ, npk (packed
#   registers), exp_users (consumers of an exp), exp_after (MFMAs ahead of a block's first exp), ntr (transposed reads).

def variant_64():
    """head_dim 64, 32 rows per wave, two waves per SIMD (csrc/attn_bwd64_asm.inc, included by attention_bwd.hip).

    Why: per 32-row half tile a wave runs  A: 8 MFMAs (S and dP chains)  ->  V: 16 v_exp + 8 v_pk_mul + 8..16 v_cvt_pk  ->  B: 8 (4) MFMAs
    (second products).  Written as C++ (rounds 3-6) these are three serial phases per wave and with two waves per SIMD the passes ran at
    0.43 MFMA-busy (profiles/r06f_pmc_summary_train_mid1.txt).  With the three halves interleaved the matrix pipe is fed back to back by ONE
    wave (the second wave of the SIMD fills what is left).

    Registers (fixed; the C++ shell sees clobber lists only).  S/dP of consecutive halves alternate between buffers X and Y:
        dK/dV pass   v[16:47] X (s | dp)   v[48:79] Y   v[80:95] packed P | dZ   v[96:127] A fragments (Q kk0..3 | dO kk0..3)
                     v[128:159] transposed fragments   a[64:95] this lane's key / value rows (MFMA B operands)
                     a[0:63] accumulators dV^T db0 | dK^T db0 | dV^T db1 | dK^T db1 (read out by ABWD64_READ_ACC_n behind the loop)
        dQ pass      v[16:47] X   v[48:79] Y   v[80:87] packed dZ   v[96:127] A fragments (K | V)   v[128:143] transposed K fragments
                     v[144:175] -L | -Delta splats (C operands)   a[32:63] this lane's q~ / dO rows   a[0:31] accumulators dQ^T db0 | db1
    (asm operands: at most 30 per statement, a "+" operand counting twice -- hence fixed accumulators and the in-asm address arithmetic.)
    No tail masks: padded query / key rows must be ZERO in q, k, v and dO (they are: zero-initialised workspaces that only rows < S are ever
    written to; attention_bwd.hip states the contract) -- a zero row contributes exactly 0 to every second product.

    Only this variant has ablation builds of its dK/dV loop (scripts/attn_bwd_ablate.py; results are garbage): what bounds it?"""
    Y, PZ, AF, TR = 48, 80, 96, 128
    NLD = 144                     # dQ pass: -L splat v[144:159], -Delta splat v[160:175]

    def rows(kv):                 # this lane's rows through the fragment registers: a[kv : kv + 32) <- v[AF : AF + 32)
        return [[(AF + 16 * w + 4 * i, "grow", f"p{w}", 32 * i, kv + 16 * w + 4 * i) for i in range(4) for w in range(2)]]

    def dkv():
        kv = 64                                               # a[64:79] key row fragments kk0..3, a[80:95] value row fragments

        def mf_B():                                           # dV^T += dO^T . P, dK^T += Q^T . dZ: [dO db0 | dO db1 | Q db0 | Q db1] x 4 regs per k-step
            out = []
            for hs in range(2):
                t = TR + 16 * hs
                pf, zf = vr(PZ + 4 * hs, 4), vr(PZ + 8 + 4 * hs, 4)
                out += [mfma(ar(0, 16), vr(t, 4), pf), mfma(ar(16, 16), vr(t + 8, 4), zf), mfma(ar(32, 16), vr(t + 4, 4), pf), mfma(ar(48, 16), vr(t + 12, 4), zf)]
            return out

        def rd_A(n, qb):                                      # C operands (-L | -Delta of the half's 32 queries) straight into buffer n, then the fragments
            out = rd_nld(n, qb)
            # fragment kk sits at 16-byte chunk (2 kk + lg) ^ swizzle(row) = chunk(kk = 0) ^ 2 kk: its address is r0 ^ 32 kk (ring slots are multiples of
            # 512 bytes) -- formed in the destination's first register instead of held in three more address registers (this pass has none to spare:
            # 256 unified registers at two waves per SIMD); entries are (instructions of one gap slot)
            for kk in range(4):
                for dst, off in ((AF + 4 * kk, 4096 * qb), (AF + 16 + 4 * kk, 8192 + 4096 * qb)):
                    if kk == 0:
                        out.append(f"ds_read_b128 {vr(dst, 4)}, %[r0] offset:{off}")
                    else:
                        out.append(f"v_xor_b32 {vr(dst)}, {32 * kk}, %[r0]\\nds_read_b128 {vr(dst, 4)}, {vr(dst)} offset:{off}")
            return out

        def rd_T(qb):
            out = []
            for hs in range(2):
                for (blk, off) in ((0, 8192), (8, 0)):       # dO tile at +8192, Q tile at +0; k-step hs: rows +16 = +2048 bytes
                    for i in range(4):                       # pieces (db, jj) = (0,0) (0,1) (1,0) (1,1): db = 1 is chunk ^ 4 = address ^ 64
                        dst = TR + 16 * hs + blk + 2 * i
                        o = off + 2048 * hs + 4096 * qb
                        if i < 2:
                            out.append(f"ds_read_b64_tr_b16 {vr(dst, 2)}, %[a{i}] offset:{o}")
                        else:
                            out.append(f"v_xor_b32 {vr(dst)}, 64, %[a{i - 2}]\\nds_read_b64_tr_b16 {vr(dst, 2)}, {vr(dst)} offset:{o}")
            return out

        def valu(c, qb, masked):
            """{gap: [instr]} of V on buffer c: exps from gap 1 (the S chain's last MFMA is three MFMAs back), the packed outputs behind the
            MFMAs of B that read their old values (pf0 / zf0: m0..m3, pf1 / zf1: m4..m7)."""
            g = defaultdict(list)
            for r in range(8):
                g[1 + r // 2].append(v_exp(c + r))
            for r in range(8, 16):
                g[5 + (r - 8)].append(v_exp(c + r))
            for j, gp in enumerate((5, 6, 7, 8, 7, 9, 11, 13)):
                g[gp].append(pk_mul(c + 16 + 2 * j, c + 2 * j))
            for j, gp in enumerate((5, 6, 7, 8, 8, 9, 11, 13)):
                g[gp].append(cvt_pk(PZ + j, c + 2 * j))
            for j, gp in enumerate((6, 7, 8, 9, 8, 10, 12, 14)):
                g[gp].append(cvt_pk(PZ + 8 + j, c + 16 + 2 * j))
            return g

        return NS(name="DKV", label="DKV", nld_ring=True, splat=[], nacc=64, rows=rows(kv), vhi=160, ahi=96,
                  mf_A=lambda n: chains(n, 4, (vr, AF), [kv]), mf_B=mf_B, rd_A=rd_A, rd_T=rd_T, valu=valu, nB=8, nA=8,
                  rdA_gaps=[0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5],      # C operands first (needed by m8 / m9), fragment kk3 last (read by m15 of the previous body)
                  rdT_gaps=[8, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 11, 11, 12, 12],      # (from the gap behind B's last MFMA; three gaps of flight before the next body)
                  a_addrs=["la", "r0"], t_addrs=["a0", "a1"], derive_A=[], derive_T=[], PZ=PZ, npk=16, exp_users=2, exp_after=[2], ntr=16)

    def dq():
        kv = 32                                               # a[32:47] q~ row fragments, a[48:63] dO row fragments

        def mf_B():                                           # dQ^T += K^T . dZ^T: [K db0 | K db1] x 4 regs per k-step
            out = []
            for hs in range(2):
                zf = vr(PZ + 4 * hs, 4)
                out += [mfma(ar(0, 16), vr(TR + 8 * hs, 4), zf), mfma(ar(16, 16), vr(TR + 8 * hs + 4, 4), zf)]
            return out

        def rd_A(n, kb):
            return [f"ds_read_b128 {vr(AF + 16 * w + 4 * kk, 4)}, %[r{kk}] offset:{8192 * w + 4096 * kb}" for kk in range(4) for w in range(2)]

        def rd_T(kb):
            return [f"ds_read_b64_tr_b16 {vr(TR + 8 * hs + 2 * i, 2)}, %[a{i}] offset:{2048 * hs + 4096 * kb}" for hs in range(2) for i in range(4)]

        def valu(c, kb, masked):
            g = defaultdict(list)
            for r in range(12):
                g[1 + r // 2].append(v_exp(c + r))
            for r in range(12, 16):
                g[7 + (r - 12)].append(v_exp(c + r))
            for j, gp in enumerate((7, 7, 8, 8, 9, 9, 9, 11)):
                g[gp].append(pk_mul(c + 16 + 2 * j, c + 2 * j))
            for j, gp in enumerate((8, 8, 10, 10, 10, 10, 11, 11)):
                g[gp].append(cvt_pk(PZ + j, c + 16 + 2 * j))
            return g

        return NS(name="DQ", label="DQ", nld_ring=False, splat=[(NLD, "nl", "nd")], nacc=32, rows=rows(kv), vhi=176, ahi=64,
                  mf_A=lambda n: chains(n, 4, (vr, AF), [kv], [NLD]), mf_B=mf_B, rd_A=rd_A, rd_T=rd_T, valu=valu, nB=4, nA=8,
                  rdA_gaps=[0, 0, 0, 0, 1, 1, 1, 1], rdT_gaps=[5, 5, 6, 6, 7, 7, 8, 8],
                  a_addrs=["r0", "r1", "r2", "r3"], t_addrs=["a0", "a1", "a2", "a3"], derive_A=[], derive_T=[], PZ=PZ, npk=8, exp_users=1, exp_after=[2], ntr=8)

    return NS(prefix="ABWD64", Y=Y, TILE=8192, nblk=1, readers=2, masked_last=False, t_extra=[], passes=(dkv(), dq()),
              # this wave's LDS-DMA pieces of a tile: rows [8 w, 8 w + 8) and [8 (w + 4), ..) of the first operand, the same of the second
              pieces=[(S_B0, 0), (S_B0H, 0), (S_B1, 0), (S_B1H, 0)],
              ablations=[("NOVALU", {"novalu"}), ("NOLDS", {"nolds"}), ("NOSYNC", {"nosync"}), ("MFMAONLY", {"novalu", "nolds", "nosync"})],
              sregs=regs("s", 70, 94) + ["scc", "memory"], read_acc=(0, 16, 32, 48),
              header=["// GENERATED by gen_attn_bwd.py 64 -- do not edit.  Software-pipelined main loops of the head_dim-64 attention backward (attention_bwd.hip);",
                      "// see the generator's docstring."])


def variant_64x2():
    """The TWO-ROW-BLOCK form at head_dim 64 (csrc/attn_bwd64x2_asm.inc, included by attention_bwd.hip).

    Variant 64's loops give a wave 32 keys (queries) and run two waves per SIMD; they are bound by the wave's own instruction issue
    (~135 instructions per 16 MFMAs, VALU and LDS costs add).  Here a wave owns 64 keys (dK/dV pass) or 64 queries (dQ pass) =
    two 32-row blocks b = 0, 1, ONE wave per SIMD with the 512-register budget: the streamed operand's row fragments, its transposed fragments
    and the -L | -Delta reads of a half tile feed BOTH blocks' MFMAs, so a body is 32 (24) MFMAs for 1.2 x the instructions of a 16 (12)-MFMA
    body.  Same schedule, same arithmetic: every output row sees the same MFMAs in the same order as in the round-3 kernels and in variant
    64's.  No tail masks (the zero-padding contract of attention_bwd.hip).

    Registers (fixed).  S / dP of consecutive halves alternate between X and Y; block b's share of a buffer is + 32 b (s | dp):
        dK/dV pass   v[16:79] X   v[80:143] Y   v[144:175] packed (block b: P at + 16 b, dZ at + 16 b + 8)   v[176:207] -L | -Delta (C operands of
                     both blocks' chains)   v[208:239] row fragments (Q kk0..3 | dO kk0..3)   v[240:244] derived read addresses
                     a[0:127] accumulators (block b: dV^T db0, db1, dK^T db0, db1 at 64 b + 0 / 16 / 32 / 48)   a[128:191] the lane's key / value rows
                     (block b: K at 128 + 32 b, V at 144 + 32 b)   a[192:223] transposed fragments [dO db0 | dO db1 | Q db0 | Q db1] x k-step
        dQ pass      v[16:79] X   v[80:143] Y   v[144:159] packed dZ (block b at + 8 b)   v[160:223] -L | -Delta splats (block b at + 32 b)
                     v[224:226] derived read addresses
                     a[0:63] dQ^T (block b: db0, db1 at 32 b + 0 / 16)   a[64:127] the lane's q~ / dO rows (block b: q~ at 64 + 32 b, dO at 80 + 32 b)
                     a[128:143] transposed K fragments   a[144:175] row fragments (K kk0..3 | V kk0..3; ds_read_b128 writes AGPRs directly)
    LDS / tile ring: variant 64's (4 slots, three tiles ahead, one vmcnt; the loop always issues a tile's loads)."""
    Y, TILE = 80, 8192

    def rows(KV):                 # block b's first-operand fragments kk0..3 at a[KV + 32 b ..], second at a[KV + 32 b + 16 ..]; loaded through buffer X
        return [[(X + 16 * w + 4 * kk, f"grow{b}", f"p{w}", 32 * kk, KV + 32 * b + 16 * w + 4 * kk) for w in range(2) for kk in range(4)] for b in range(2)]

    def dkv():
        PZ, LD, AF, DR, KV, TRA = 144, 176, 208, 240, 128, 192
        raddr, taddr, derive_A, derive_T = derived(DR)

        def mf_B():
            """k-step 0 of both blocks first (they read the packed registers' first halves), then k-step 1"""
            out = []
            for hs in range(2):
                t = TRA + 16 * hs
                for b in range(2):
                    pf, zf = vr(PZ + 16 * b + 4 * hs, 4), vr(PZ + 16 * b + 8 + 4 * hs, 4)
                    out += [mfma(ar(64 * b, 16), ar(t, 4), pf), mfma(ar(64 * b + 32, 16), ar(t + 8, 4), zf),
                            mfma(ar(64 * b + 16, 16), ar(t + 4, 4), pf), mfma(ar(64 * b + 48, 16), ar(t + 12, 4), zf)]
            return out

        def rd_A(n, qb):
            return rd_nld(LD, qb) + [f"ds_read_b128 {vr(AF + 16 * w + 4 * kk, 4)}, {raddr(kk)} offset:{TILE * w + 4096 * qb}" for kk in range(4) for w in range(2)]

        def rd_T(qb):
            return [f"ds_read_b64_tr_b16 {ar(TRA + 16 * hs + blk + 2 * i, 2)}, {taddr(i)} offset:{off + 2048 * hs + 4096 * qb}"
                    for hs in range(2) for (blk, off) in ((0, TILE), (8, 0)) for i in range(4)]       # dO tile at + 8192, Q tile at + 0; k-step hs: rows + 16 = + 2048 bytes

        def valu(c, qb, masked):
            g = defaultdict(list)
            for b in range(2):
                s, d, pz = c + 32 * b, c + 32 * b + 16, PZ + 16 * b
                e0 = 1 + 8 * b                               # block 0's chains end four MFMAs before block 1's: its exps start at gap 1, block 1's at gap 9
                for r in range(16):
                    g[e0 + r].append(v_exp(s + r))
                for j in range(8):
                    m = e0 + 2 * j + 3
                    g[m].append(pk_mul(d + 2 * j, s + 2 * j))
                    lo = 9 if j < 4 else 17                  # behind the MFMAs of B that read the old packed values (m0..m7 / m8..m15)
                    g[max(m, lo)].append(cvt_pk(pz + j, s + 2 * j))
                    g[max(m + 1, lo)].append(cvt_pk(pz + 8 + j, d + 2 * j))
            return g

        return NS(name="DKV2", label="DKV2", nld_ring=True, splat=[], nacc=128, rows=rows(KV), vhi=245, ahi=224,
                  mf_A=lambda n: chains(n, 4, (vr, AF), [KV, KV + 32], [LD, LD]), mf_B=mf_B, rd_A=rd_A, rd_T=rd_T, valu=valu, nB=16, nA=16,
                  rdA_gaps=[g for g in range(8) for _ in range(2)],             # 16 reads: C operands first, fragment k-step 3 last
                  rdT_gaps=[16 + i // 2 for i in range(16)],                    # from the gap behind B's last MFMA
                  a_addrs=["la", "r0"], t_addrs=["a0", "a1"], derive_A=derive_A, derive_T=derive_T, PZ=PZ, npk=32, exp_users=2, exp_after=[2, 8], ntr=16)

    def dq():
        PZ, NLD, AFA, DR, KV, TRA = 144, 160, 144, 224, 64, 128          # (AFA: the K | V row fragments live in AGPRs a[144:175]: ds_read_b128 writes them directly)
        raddr, _, derive_A, _ = derived(DR)                              # (four transposed-read address operands: this pass has operand slots to spare and no free VGPR block)

        def mf_B():
            out = []
            for hs in range(2):
                t = TRA + 8 * hs
                for b in range(2):
                    zf = vr(PZ + 8 * b + 4 * hs, 4)
                    out += [mfma(ar(32 * b, 16), ar(t, 4), zf), mfma(ar(32 * b + 16, 16), ar(t + 4, 4), zf)]
            return out

        def rd_A(n, kb):
            return [f"ds_read_b128 {ar(AFA + 16 * w + 4 * kk, 4)}, {raddr(kk)} offset:{TILE * w + 4096 * kb}" for kk in range(4) for w in range(2)]

        def rd_T(kb):
            return [f"ds_read_b64_tr_b16 {ar(TRA + 8 * hs + 2 * i, 2)}, %[a{i}] offset:{2048 * hs + 4096 * kb}" for hs in range(2) for i in range(4)]

        def valu(c, kb, masked):
            g = defaultdict(list)
            for b in range(2):
                s, d, pz = c + 32 * b, c + 32 * b + 16, PZ + 8 * b
                e0 = 1 + 6 * b
                for r in range(16):
                    g[e0 + r].append(v_exp(s + r))
                for j in range(8):
                    m = e0 + 2 * j + 3
                    g[m].append(pk_mul(d + 2 * j, s + 2 * j))
                    g[max(m + 1, 5 if j < 4 else 9)].append(cvt_pk(pz + j, d + 2 * j))
            return g

        return NS(name="DQ2", label="DQ2", nld_ring=False, splat=[(NLD + 32 * b, f"nl{b}", f"nd{b}") for b in range(2)], nacc=64, rows=rows(KV), vhi=227, ahi=176,
                  mf_A=lambda n: chains(n, 4, (ar, AFA), [KV, KV + 32], [NLD, NLD + 32]), mf_B=mf_B, rd_A=rd_A, rd_T=rd_T, valu=valu, nB=8, nA=16,
                  rdA_gaps=[0, 0, 1, 1, 2, 2, 3, 3], rdT_gaps=[8 + i // 2 for i in range(8)],
                  a_addrs=["r0"], t_addrs=["a0", "a1", "a2", "a3"], derive_A=derive_A, derive_T=[], PZ=PZ, npk=16, exp_users=1, exp_after=[2, 6], ntr=8)

    return NS(prefix="ABWD64X2", Y=Y, TILE=TILE, nblk=2, readers=2, masked_last=False, t_extra=[], passes=(dkv(), dq()),
              pieces=[(S_B0, 0), (S_B0H, 0), (S_B1, 0), (S_B1H, 0)], ablations=[], sregs=regs("s", 70, 94) + ["scc", "memory"], read_acc=range(0, 128, 16),
              header=["// GENERATED by gen_attn_bwd.py 64x2 -- do not edit.  Two-row-block software-pipelined main loops of the head_dim-64 attention backward",
                      "// (attention_bwd.hip); see the generator's docstring."])


def variant_128():
    """head_dim 128 (csrc/attn_bwd128_asm.inc, included by attention128_bwd.hip): the two passes of FLUX.1 / Qwen-Image / Wan.  The schedule is
    variant 64's carried to 128 the way attention128_bwd.hip carries the kernels:

    per 32-row half h:  A = the S and dP chains (8 k-steps each: 16 MFMAs),  V = 16 v_exp + mask + 8 v_pk_mul + 8..16 v_cvt_pk,  B = the second
    products (dV^T, dK^T: 16 MFMAs; dQ^T: 8).  These kernels run ONE wave per SIMD (512 registers: 128 / 64 accumulator registers), so nothing
    but the wave's own instruction order can put VALU work under MFMAs: the round-4 kernels issue both halves' chains back to back and overlap
    half of the exp / pack arithmetic; here every MFMA gap of a body carries fillers of another half.  Same MFMAs, operand order and accumulation
    order per output element as the round-4 kernels, same masks where they can act (the last tile: queries >= S / keys >= the sample's key count
    get P = 0; the loop's other tiles run a copy of the body without the 32 mask instructions per half).

    Registers (fixed).  S / dP of consecutive halves alternate between X and Y:
        both passes  v[16:47] X (s | dp)   v[48:79] Y   v[80:95] packed P | dZ (dQ pass: dZ only)   v[96:159] A fragments (first operand k-steps
                     0..7 | second operand k-steps 0..7)   v[224:228] derived read addresses   s[36:67] the half's 16 lane masks
        dK/dV pass   v[160:223] transposed fragments (d half 0 | d half 1: [dO db0 | dO db1 | Q db0 | Q db1] x (k-step 0 | k-step 1))
                     a[0:63] dV^T blocks 0..3, a[64:127] dK^T blocks 0..3, a[128:159] / a[160:191] this lane's key / value row fragments
        dQ pass      v[160:191] transposed K fragments, v[192:223] -L | -Delta splats (C operands)
                     a[0:63] dQ^T blocks 0..3, a[64:95] / a[96:127] this lane's q~ / dO row fragments
    LDS: a [64][128] operand tile is two [64][64] sub-tiles (8 KiB each, 128-byte rows, the head_dim-64 swizzle); stage = first operand (16 KiB) |
    second operand (16 KiB) [| -L | -Delta (512 B)]; 4-slot ring, three tiles ahead, ONE `vmcnt` (the loop always issues a tile's loads; past the
    end it re-loads the last tile into a slot nobody reads)."""
    Y, PZ, AF, TR = 48, 80, 96, 160
    NLD = 192
    DR = 224                      # derived addresses: v224..226 = r0 ^ 32 kk (kk = 1..3), v227 / v228 = a0 / a1 ^ 64
    MK = 36                       # s[36:67]: 16 lane masks of the half V works on
    SUB, TILE = 8192, 16384
    raddr, taddr, derive_A, derive_T = derived(DR)

    def rows(kv):                 # this lane's rows (2 x 8 fragments) through the fragment registers: a[kv : kv + 64) <- v[AF : AF + 64)
        return [[(AF + 32 * w + 4 * i, "grow", f"p{w}", 32 * i, kv + 32 * w + 4 * i) for i in range(8) for w in range(2)]]

    def rd_frags(qb):
        return [f"ds_read_b128 {vr(AF + 32 * w + 4 * j, 4)}, {raddr(j & 3)} offset:{TILE * w + (j >> 2) * SUB + 4096 * qb}" for j in range(8) for w in range(2)]

    def masked_exps(c, qb, masked):
        """exps from gap 1; lane mask of element r = (this lane's remaining valid rows) > 32 qb + 16 (r >> 3) + (r & 7), applied behind its exp"""
        g = defaultdict(list)
        if masked:
            for r in range(16):
                g[r].append(f"v_cmp_lt_i32_e64 {sr(MK + 2 * r)}, {32 * qb + 16 * (r >> 3) + (r & 7)}, %[vrem]")
        for r in range(16):
            g[r + 1].append(v_exp(c + r))
            if masked:
                g[r + 3].append(f"v_cndmask_b32_e64 {vr(c + r)}, 0, {vr(c + r)}, {sr(MK + 2 * r)}")
        return g

    def dkv():
        kv = 128

        def mf_B():
            """k-step 0 of both d halves first (they read pf0 / zf0), then k-step 1: the packed registers of the NEXT half may be written behind m7 / m15"""
            out = []
            for hs in range(2):
                pf, zf = vr(PZ + 4 * hs, 4), vr(PZ + 8 + 4 * hs, 4)
                for dh in range(2):
                    t = TR + 32 * dh + 16 * hs
                    out += [mfma(ar(32 * dh, 16), vr(t, 4), pf), mfma(ar(64 + 32 * dh, 16), vr(t + 8, 4), zf),
                            mfma(ar(32 * dh + 16, 16), vr(t + 4, 4), pf), mfma(ar(64 + 32 * dh + 16, 16), vr(t + 12, 4), zf)]
            return out

        def rd_T(qb):
            return [f"ds_read_b64_tr_b16 {vr(TR + 32 * dh + 16 * hs + blk + 2 * i, 2)}, {taddr(i)} offset:{off + 2048 * hs + 4096 * qb}"
                    for hs in range(2) for dh in range(2) for (blk, off) in ((0, TILE + dh * SUB), (8, dh * SUB)) for i in range(4)]       # dO sub-tile, Q sub-tile of this d half

        def valu(c, qb, masked):
            g = masked_exps(c, qb, masked)
            for j in range(8):
                g[2 * j + 6].append(pk_mul(c + 16 + 2 * j, c + 2 * j))
                lo = 9 if j < 4 else 17                      # behind the MFMAs of B that read the old packed values (m0..m7 / m8..m15)
                g[max(2 * j + 6, lo)].append(cvt_pk(PZ + j, c + 2 * j))
                g[max(2 * j + 7, lo)].append(cvt_pk(PZ + 8 + j, c + 16 + 2 * j))
            return g

        return NS(name="DKV", label="DKV128", nld_ring=True, splat=[], nacc=128, rows=rows(kv), vhi=229, ahi=192,
                  mf_A=lambda n: chains(n, 8, (vr, AF), [kv]), mf_B=mf_B, rd_A=lambda n, qb: rd_nld(n, qb) + rd_frags(qb), rd_T=rd_T, valu=valu, nB=16, nA=16,
                  rdA_gaps=[g for g in range(12) for _ in range(2)],            # 24 reads, two per gap: C operands first, fragment k-step 7 last
                  rdT_gaps=[16 + i // 3 for i in range(32)],                    # 32 reads from the gap behind B's last MFMA (16..26)
                  a_addrs=["la", "r0"], t_addrs=["a0", "a1"], derive_A=derive_A, derive_T=derive_T, PZ=PZ, npk=16, exp_users=2, exp_after=[2], ntr=32)

    def dq():
        kv = 64

        def mf_B():
            out = []
            for hs in range(2):
                zf = vr(PZ + 4 * hs, 4)
                for dh in range(2):
                    t = TR + 16 * dh + 8 * hs
                    out += [mfma(ar(32 * dh, 16), vr(t, 4), zf), mfma(ar(32 * dh + 16, 16), vr(t + 4, 4), zf)]
            return out

        def rd_T(kb):
            return [f"ds_read_b64_tr_b16 {vr(TR + 16 * dh + 8 * hs + 2 * i, 2)}, {taddr(i)} offset:{dh * SUB + 2048 * hs + 4096 * kb}"
                    for hs in range(2) for dh in range(2) for i in range(4)]

        def valu(c, kb, masked):
            g = masked_exps(c, kb, masked)
            for j in range(8):
                g[2 * j + 6].append(pk_mul(c + 16 + 2 * j, c + 2 * j))
                g[max(2 * j + 7, 5 if j < 4 else 9)].append(cvt_pk(PZ + j, c + 16 + 2 * j))
            return g

        return NS(name="DQ", label="DQ128", nld_ring=False, splat=[(NLD, "nl", "nd")], nacc=64, rows=rows(kv), vhi=229, ahi=128,
                  mf_A=lambda n: chains(n, 8, (vr, AF), [kv], [NLD]), mf_B=mf_B, rd_A=lambda n, kb: rd_frags(kb), rd_T=rd_T, valu=valu, nB=8, nA=16,
                  rdA_gaps=[0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5],        # (two MFMAs of flight before the wait in front of m8)
                  rdT_gaps=[8 + i // 2 for i in range(16)],
                  a_addrs=["r0"], t_addrs=["a0", "a1"], derive_A=derive_A, derive_T=derive_T, PZ=PZ, npk=8, exp_users=1, exp_after=[2], ntr=16)

    # The masks (32 VALU instructions per half) only matter in the LAST tile -- rows beyond S / keys beyond the sample's key count -- (a lane whose
    # own key is masked in the dK/dV pass is zeroed by the shell at the end): nt - 2 unmasked iterations, then one whose second body is masked;
    # the transposed-side ring step also moves the lane's count of remaining valid rows to the next tile.
    return NS(prefix="ABWD128", Y=Y, TILE=TILE, nblk=1, readers=4, masked_last=True, MK=MK, t_extra=["v_subrev_u32 %[vrem], 64, %[vrem]"], passes=(dkv(), dq()),
              # per operand: sub-tile 0 rows w.., rows w + 32..; sub-tile 1 (d 64..127: + 128 bytes)
              pieces=[(base, off) for (lo, hi) in ((S_B0, S_B0H), (S_B1, S_B1H)) for (base, off) in ((lo, 0), (hi, 0), (lo, 128), (hi, 128))],
              ablations=[], sregs=regs("s", MK, MK + 32) + regs("s", 70, 94) + ["scc", "vcc", "memory"], read_acc=range(0, 128, 16),
              header=["// GENERATED by gen_attn_bwd.py 128 -- do not edit.  Software-pipelined main loops of the head_dim-128 attention backward (attention128_bwd.hip);",
                      "// see the generator's docstring."])


VARIANTS = {"64": variant_64, "64x2": variant_64x2, "128": variant_128}


# ------------------------------------------------------------------------------------------------------------------------- the schedule

def slot(P):
    """bytes of a ring slot: both operand tiles [| the tile's 128 -L | -Delta floats]"""
    return 2 * V.TILE + (512 if P.nld_ring else 0)


def stage(P):
    """this wave's LDS-DMA pieces of tile S_LT into ring slot S_LDSL: V.pieces, 4096 bytes of LDS apart, and (dK/dV pass) 32 of the tile's 128
    -L | -Delta floats (first 8 lanes).  The instruction offset of an LDS-DMA load is added to the global AND to the LDS address: M0 carries
    the destination minus it."""
    out, prev = [], None
    for (base, off) in V.pieces:
        out += [f"s_add_i32 m0, s{S_W1K}, s{S_LDSL}" if prev is None else f"s_add_i32 m0, m0, {4096 - off + prev}", "s_nop 0", lds_dma("g0", base, off)]
        prev = off
    if P.nld_ring:
        out += [f"s_add_i32 m0, s{S_WNL}, s{S_LDSL}", f"s_mov_b64 {sr(S_EX)}, exec", "s_mov_b64 exec, 0xff", lds_dma("g2", S_B2), f"s_mov_b64 exec, {sr(S_EX)}"]
    return out


def ring_step(P, idx_reg, addrs, derive, extra=()):
    """the read addresses `addrs` move to the next ring slot (slot index in idx_reg); `derive` re-derives the addresses kept in registers"""
    out = [f"s_add_i32 s{idx_reg}, s{idx_reg}, 1", f"s_mov_b32 s{S_D}, {slot(P)}", f"s_cmp_eq_u32 s{idx_reg}, 4",
           f"s_cselect_b32 s{S_D}, {-3 * slot(P)}, s{S_D}", f"s_cselect_b32 s{idx_reg}, 0, s{idx_reg}"]
    out += [f"v_add_u32 %[{a}], s{S_D}, %[{a}]" for a in addrs]
    return out + list(derive) + list(extra)


def sync(P):
    """tile t + 1 landed for every wave; slot of tile t - 1 is free: load tile min(t + 3, nt - 1) into it; advance the load state"""
    nloads = len(V.pieces) + P.nld_ring
    out = ([] if "nosync" in ABL else [f"s_waitcnt vmcnt({nloads})", "s_barrier"] + stage(P))
    out += [f"s_cmp_lt_u32 s{S_LT}, s{S_NT}", f"s_cselect_b32 s{S_INC}, 1, 0", f"s_add_u32 s{S_LT}, s{S_LT}, s{S_INC}"]     # S_NT holds nt - 1 here
    t = V.TILE.bit_length() - 1                           # bytes per tile = 1 << shift: 64 rows x 128 (256) B; 128 floats
    for (b, sh) in [(S_B0, t), (S_B1, t)] + ([(S_B2, 9)] if P.nld_ring else []) + [(S_B0H, t), (S_B1H, t)]:
        out += [f"s_lshl_b32 s{S_T}, s{S_INC}, {sh}", f"s_add_u32 s{b}, s{b}, s{S_T}", f"s_addc_u32 s{b + 1}, s{b + 1}, 0"]
    out += [f"s_add_i32 s{S_LDSL}, s{S_LDSL}, {slot(P)}", f"s_cmp_eq_u32 s{S_LDSL}, {4 * slot(P)}", f"s_cselect_b32 s{S_LDSL}, 0, s{S_LDSL}"]
    return out


def body(P, cur, nxt, has_B, has_A, qb_cur, qb_A, qb_T, pre=(), masked=True):
    """B(h-1) || V(h) on buffer cur (half qb_cur of its tile: the mask constants) || A(h+1) into nxt (reads: half qb_A of the A-side tile);
    transposed reads of half h (qb_T = qb_cur).  qb_cur and masked act in variant 128 only."""
    fill = defaultdict(list)
    if has_A:
        for gp, ins in zip(P.rdA_gaps, P.rd_A(nxt, qb_A)):
            fill[gp].append(ins)
    for gp, lst in P.valu(cur, qb_cur, masked).items():
        fill[gp] += lst
    for gp, ins in zip(P.rdT_gaps, P.rd_T(qb_T)):
        fill[gp].append(ins)
    if "novalu" in ABL:
        fill = {g: [i for i in v if not i.startswith(("v_exp", "v_pk_mul", "v_cvt_pk"))] for g, v in fill.items()}
    if "nolds" in ABL:
        fill = {g: [i for i in v if "ds_read" not in i] for g, v in fill.items()}
    out = list(pre)
    out.append("s_waitcnt lgkmcnt(0)")                    # the transposed fragments of B(h-1) (read during the previous body)
    mfB, mfA = P.mf_B(), P.mf_A(nxt)
    ngap = P.nB + P.nA
    for g in range(ngap):
        is_B = g < P.nB
        if g == P.nB:
            out.append("s_waitcnt lgkmcnt(0)")            # A(h+1)'s fragments and C operands (read in this body's first gaps)
        if (has_B if is_B else has_A):
            out.append(mfB[g] if is_B else mfA[g - P.nB])
        out += fill.get(g, [])
    for g in sorted(k for k in fill if k >= ngap):
        out += fill[g]
    return out


def main_loop(P):
    Y = V.Y
    L = [f"s_mov_b32 s{S_M0}, m0", f"s_mov_b64 {sr(S_B0)}, %[b0]", f"s_mov_b64 {sr(S_B1)}, %[b1]"]
    if P.nld_ring:
        L.append(f"s_mov_b64 {sr(S_B2)}, %[b2]")
    for (lo, hi) in ((S_B0, S_B0H), (S_B1, S_B1H)):
        L += [f"s_add_u32 s{hi}, s{lo}, {V.TILE // 2}", f"s_addc_u32 s{hi + 1}, s{lo + 1}, 0"]
    L += [f"s_sub_u32 s{S_NT}, %[nt], 1",                 # nt - 1: loop count and the last tile's index
          f"s_mov_b32 s{S_CNT}, s{S_NT}", f"s_min_u32 s{S_LT}, s{S_NT}, 3", f"s_mov_b32 s{S_LDSL}, {3 * slot(P)}",
          f"s_mov_b32 s{S_STA}, 0", f"s_mov_b32 s{S_STT}, 0",
          f"s_lshl_b32 s{S_W1K}, %[wv], 10"]              # LDS-DMA destinations of this wave inside a slot (the dynamic LDS base is 0: checked by the shell)
    if P.nld_ring:
        L += [f"s_lshl_b32 s{S_WNL}, %[wv], 7", f"s_add_u32 s{S_WNL}, s{S_WNL}, {2 * V.TILE}"]
    for i in range(P.nacc):
        L.append(f"v_accvgpr_write_b32 {ar(i)}, 0")
    # ---- this lane's rows (MFMA B operands of the first products) into AGPRs through VGPRs, a row block at a time (loads in table order, moves
    #      in register order)
    for blk in P.rows:
        L += [f"global_load_dwordx4 {vr(vreg, 4)}, %[{goff}], %[{base}] offset:{off}" for (vreg, goff, base, off, areg) in blk]
        L.append("s_waitcnt vmcnt(0)")                    # (also tiles 0..2, staged by the shell: the barrier below publishes tile 0)
        for (vreg, goff, base, off, areg) in sorted(blk, key=lambda row: row[4]):
            L += [f"v_accvgpr_write_b32 {ar(areg + e)}, {vr(vreg + e)}" for e in range(4)]
    for (dst, nl, nd) in P.splat:                         # dQ pass: the lane's own -L | -Delta as the C operands of its chains
        for i in range(16):
            L += [f"v_mov_b32 {vr(dst + i)}, %[{nl}]", f"v_mov_b32 {vr(dst + 16 + i)}, %[{nd}]"]
    L += P.derive_A + P.derive_T
    L.append("s_barrier")
    # ---- prologue: A(0) alone, then body(0) without B
    L += P.rd_A(X, 0)
    L.append("s_waitcnt lgkmcnt(0)")
    L += P.mf_A(X)
    L += ["s_nop 15", "s_nop 15"]
    L += body(P, X, Y, False, True, 0, 1, 0)

    # ---- nt - 1 iterations: sync(t + 1) | body(2t + 1) on Y (A-side addresses -> tile t + 1) | body(2t + 2) on X (transposed side, masks -> tile t + 1)
    def iteration(masked):
        return (body(P, Y, X, True, True, 1, 0, 1, pre=sync(P) + ring_step(P, S_STA, P.a_addrs, P.derive_A), masked=False) +
                body(P, X, Y, True, True, 0, 1, 0, pre=ring_step(P, S_STT, P.t_addrs, P.derive_T, extra=V.t_extra), masked=masked))
    L += [f"s_cmp_eq_u32 s{S_CNT}, 0", f"s_cbranch_scc1 L_{P.label}_tail%="]
    if V.masked_last:
        L += [f"s_sub_u32 s{S_CNT}, s{S_CNT}, 1", f"s_cmp_eq_u32 s{S_CNT}, 0", f"s_cbranch_scc1 L_{P.label}_last%="]
    L.append(f"L_{P.label}_loop%=:")
    L += iteration(False)
    L += [f"s_sub_u32 s{S_CNT}, s{S_CNT}, 1", f"s_cmp_lg_u32 s{S_CNT}, 0", f"s_cbranch_scc1 L_{P.label}_loop%="]
    if V.masked_last:
        L.append(f"L_{P.label}_last%=:")
        L += iteration(True)
    L.append(f"L_{P.label}_tail%=:")
    # ---- body(2 nt - 1) without A, then B(2 nt - 1)
    L += body(P, Y, X, True, False, 1, 0, 1)
    L += ["s_waitcnt lgkmcnt(0)", "s_nop 7"]
    L += P.mf_B()
    L += [f"s_mov_b32 m0, s{S_M0}", "s_waitcnt vmcnt(0)", "s_nop 15", "s_nop 15"]
    return L


def check(P):
    """structural checks on a steady-state body: MFMA count, no packed output written before the MFMAs of B that read its old value, every exp at
    least two instructions ahead of its first consumer (transcendental-use hazard; variant 128: mask compare, exp, select, consumer in order)"""
    Y = V.Y
    b = [part for ins in body(P, Y, X, True, True, 1, 0, 1) for part in ins.split("\\n")]
    assert sum(1 for ins in b if ins.startswith("v_mfma")) == P.nA + P.nB
    for reg in range(P.PZ, P.PZ + P.npk):
        w = [i for i, ins in enumerate(b) if ins.startswith(f"v_cvt_pk_bf16_f32 v{reg},")]
        assert len(w) == 1, (P.name, reg, w)
        lo = P.PZ + 4 * ((reg - P.PZ) // 4)
        readers = [i for i, ins in enumerate(b) if ins.startswith("v_mfma") and f", v[{lo}:{lo + 3}], a[" in ins]
        assert len(readers) == V.readers and all(r < w[0] for r in readers), (P.name, reg, readers, w)
    n_mf = lambda upto: sum(1 for ins in b[:upto] if ins.startswith("v_mfma"))
    for blk in range(V.nblk):
        first_exp = len(b)
        for reg in range(Y + 32 * blk, Y + 32 * blk + 16):
            e = [i for i, ins in enumerate(b) if ins == f"v_exp_f32 v{reg}, v{reg}"]
            assert len(e) == 1
            first_exp, after = min(first_exp, e[0]), e[0] + 1
            if V.masked_last:
                k = [i for i, ins in enumerate(b) if ins.startswith(f"v_cmp_lt_i32_e64 s[{V.MK + 2 * (reg - Y)}:")]
                c = [i for i, ins in enumerate(b) if ins.startswith(f"v_cndmask_b32_e64 v{reg},")]
                assert len(k) == 1 and len(c) == 1 and k[0] + 2 < c[0] and e[0] + 1 < c[0], (P.name, reg, e, k, c)
                after = c[0]
            pair = f"v[{reg & ~1}:{(reg & ~1) + 1}]"
            users = [i for i, ins in enumerate(b) if (ins.startswith("v_pk_mul") and ins.endswith(pair)) or
                     (ins.startswith("v_cvt_pk") and re.search(rf", v{reg}(,|$)", ins))]
            assert len(users) == P.exp_users and all(u > after for u in users), (P.name, reg, e, users)
        # the S / dP chains' results are three MFMAs old when a block's first exp reads them (block 1's chains end four MFMAs behind block 0's)
        assert n_mf(first_exp) >= P.exp_after[blk], (P.name, blk, first_exp)
    # every transposed-fragment register is written once per body, behind the last MFMA of B
    lastB = max(i for i, ins in enumerate(b) if ins.startswith("v_mfma_f32_32x32x16_bf16 a["))
    tr_w = [i for i, ins in enumerate(b) if ins.startswith("ds_read_b64_tr_b16")]
    assert len(tr_w) == P.ntr and min(tr_w) > lastB, (P.name, lastB, min(tr_w))


def main():
    global V
    if len(sys.argv) != 2 or sys.argv[1] not in VARIANTS:
        sys.exit(f"usage: python {sys.argv[0]} {{{'|'.join(VARIANTS)}}} > attn_bwd<variant>_asm.inc")
    V = VARIANTS[sys.argv[1]]()
    for P in V.passes:
        check(P)
    print("\n".join(V.header))
    for P in V.passes:
        emit(f"{V.prefix}_{P.name}_ASM", main_loop(P))
    for tag, abl in V.ablations:                          # of the dK/dV loop
        ABL.update(abl)
        emit(f"{V.prefix}_{V.passes[0].name}_ASM_{tag}", main_loop(V.passes[0]))
        ABL.clear()
    for P in V.passes:
        print(f"#define {V.prefix}_{P.name}_CLOBBERS " + clobbers(*regs("v", 16, P.vhi), *regs("a", 0, P.ahi), *V.sregs))
    print()
    read_acc_macros(V.prefix, V.read_acc)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generator of the hand-scheduled key loop of the 4-wave head_dim-64 attention forward (csrc/attn64_w4_asm.inc, included by attention.hip).
The head_dim-64 form of gen_attn128_w4.py.

Static-softmax flash attention (|score| <= 60 proven by the caller, q pre-scaled: no running max), 4 waves per workgroup, each wave TWO chains
of 32 queries (one query per lane, like attn_kernel) so that the softmax of one chain runs on the VALU under the MFMAs of the other:

    per 64-key tile and wave:   S_c^T = K . Q_c^T   8 MFMAs (2 key blocks x 4 k-steps)          c = 0, 1
                                P_c   = exp2(S_c)   32 v_exp + 32 v_add (row sums, fp32) + 16 v_cvt_pk (in-place compaction: P lives in S's registers)
                                O_c^T += V^T . P_c  8 MFMAs (4 key steps x 2 d blocks)
    MFMA order across tiles:    S0(t) | PV1(t-1) | S1(t) | [sync] | PV0(t) | S0(t+1) | ...          (four phases of 8 MFMAs per tile)
    softmax0(t) sits behind the MFMAs of PV1(t-1) and S1(t), softmax1(t) behind PV0(t) and S0(t+1).
    Fragments: the 8 K fragments of a tile feed S0 and S1 from buffer X, its 8 V^T fragments feed PV0 and PV1 from buffer Y: 16 ds_read_b128 per
    tile and wave for 32 MFMAs.  V^T(t) is read behind the MFMAs of S1(t) (after PV1(t-1), Y's last consumer), K(t+1) behind those of PV0(t)
    (after S1(t), X's last consumer, and after the sync that proves tile t + 1 landed): one read per gap in two of the four phases.  Every MFMA
    waits with a COUNTED lgkmcnt for exactly the fragment it multiplies (resolve_waits: the one lgkmcnt(0) of a tile is the count of phase 1's
    last fragment, with nothing issued behind it); the steady state never uses vmcnt(0) and has one barrier per tile.

Registers (fixed; the C++ shell sees clobber lists only):
    a[0:63]     O accumulators, O[c][db] at a[(c*2 + db)*16 ...]          a[64:95]    Q fragments (MFMA B operand), Q[c][kk] at a[64 + (c*4 + kk)*4 ...]
    v[32:95]    S / P, S[c][kb] at v[32 + (c*2 + kb)*16 ...]              v[96:127]   fragment buffer X (K), v[128:159] buffer Y (V^T)
LDS (dynamic base must be 0): [0, 32 KiB) V^T ring, [32, 64 KiB) K ring, 4 stages of 8 KiB each (stage t & 3).  K / V^T tiles arrive by
global_load_lds_dwordx4 (2 + 2 wave-instructions per wave and tile) issued TWO tiles ahead (phase 1 of tile t loads tile t + 2; the shell stages
tiles 0 and 1); the sync between phases 3 and 4 waits with vmcnt(4) for tile t + 1 only; the layouts (128-byte rows, 16-byte chunks
XOR-swizzled) are attn_kernel's.  The read bases hold lane part + stage; the K ring's 32 KiB sit in the ds_read offset field, so a base rotates
with two VALU instructions per tile.
The LAST tile masks keys >= S: v_cmp_gt_i32 / v_cndmask per score register against (valid keys in the tile - 8 * half-wave).
A wave with no query below S runs the *_STAGE bodies: the same loads, waits and barriers, nothing else.

Structural checks run on every generation (main -> check_all): check_softmax (the in-place compaction never overwrites a live value) and
check_stream, which replays the straight-line instruction stream of 1 .. 7 tiles and asserts that every MFMA finds the fragment of the tile it
expects, read from the ring stage that tile was loaded into, after the sync that proves it landed, and retired by an s_waitcnt whose count
equals the number of reads issued behind it; that every vmcnt equals the number of loads issued behind the tile it waits for; and that every
register named lies inside the budget of A64_CLOBBERS.

Emitted macros: A64_BODY_MULTI (n_tiles >= 3: first tile, `mid` = n_tiles - 3 loop iterations, next-to-last, last), A64_BODY_TWO, A64_BODY_SINGLE,
A64_STAGE_MULTI / _TWO, A64_CLOBBERS, A64_WRITE_Q_c_kk(frag), A64_READ_O_c_db(dst); under MI355_ABLATE the timing-only forms of A64_BODY_MULTI.
usage: python gen_attn64_w4.py > attn64_w4_asm.inc
"""
import re

from asmgen import clobbers, emit, interleave, regs

S_BASE, FX, FY, V_END = 32, 96, 128, 160
O_BASE, Q_BASE, A_END = 0, 64, 96
K_RING = 0x8000            # LDS offset of the K ring (the V^T ring is at 0); a stage is 0x2000
# fixed scalars
S_KSRC, S_VSRC, S_MK, S_MV, S_CNT, S_M0SAVE = 80, 82, 84, 85, 86, 87
S_LO, S_HI = 80, 88
NPH = 8                    # MFMAs per phase


class I(str):
    """an instruction with what the structural checks need to know about it"""
    def __new__(cls, s, **meta):
        o = str.__new__(cls, s)
        o.meta = meta
        return o


def sreg(c, kb, r=0, n=16):
    b = S_BASE + (c * 2 + kb) * 16 + r
    return f"v[{b}:{b + n - 1}]" if n > 1 else f"v{b}"


def oreg(c, db):
    b = O_BASE + (c * 2 + db) * 16
    return f"a[{b}:{b + 15}]"


def qreg(c, kk):
    b = Q_BASE + (c * 4 + kk) * 4
    return f"a[{b}:{b + 3}]"


def frag(buf, slot):
    b = buf + slot * 4
    return f"v[{b}:{b + 3}]"


def mfma_s(c, t):
    """S_c = K . Q_c^T: 8 MFMAs on buffer X, key blocks alternate so that dependent MFMAs are two apart"""
    out = []
    for kk in range(4):
        for kb in range(2):
            cin = "0" if kk == 0 else sreg(c, kb)
            slot = kk * 2 + kb
            out.append(I(f"v_mfma_f32_32x32x16_bf16 {sreg(c, kb)}, {frag(FX, slot)}, {qreg(c, kk)}, {cin}", use=(FX, slot), expect=("K", t, slot)))
    return out


def mfma_pv(c, t):
    """O_c += V^T . P_c on buffer Y: key step cc (16 keys) x d block db; P fragment cc = registers (cc & 1) * 4 .. + 3 of S[c][cc >> 1] (compacted)"""
    out = []
    for cc in range(4):
        pb = S_BASE + (c * 2 + (cc >> 1)) * 16 + (cc & 1) * 4
        for db in range(2):
            slot = cc * 2 + db
            out.append(I(f"v_mfma_f32_32x32x16_bf16 {oreg(c, db)}, {frag(FY, slot)}, v[{pb}:{pb + 3}], {oreg(c, db)}", use=(FY, slot), expect=("V", t, slot)))
    return out


def reads_k(t):
    return [I(f"ds_read_b128 {frag(FX, kk * 2 + kb)}, %[vk{kk}] offset:{K_RING + kb * 4096}", rd=(FX, kk * 2 + kb), tag=("K", t, kk * 2 + kb))
            for kk in range(4) for kb in range(2)]


def reads_v(t):
    return [I(f"ds_read_b128 {frag(FY, cc * 2 + db)}, %[vc{cc}] offset:{db * 4096}", rd=(FY, cc * 2 + db), tag=("V", t, cc * 2 + db))
            for cc in range(4) for db in range(2)]


def softmax(c, masked):
    """VALU stream of one chain's softmax in dependency order; entries are lists of instructions that may share a gap.  Row sums are plain f32
    adds of the exponentials, two partial sums (gen_attn128_w4.py has the measurement against v_dot2_f32_bf16 of the packed pairs; packed f32
    adds are dearer still beside MFMAs)."""
    ops = []
    for r in range(32):
        kb, rr = r >> 4, r & 15
        reg = sreg(c, kb, rr, 1)
        grp = []
        if masked:
            kconst = 32 * kb + 16 * (rr >> 3) + (rr & 7)
            grp += [f"v_cmp_gt_i32 vcc, %[vrem], {kconst}", f"v_cndmask_b32 {reg}, %[vneg], {reg}, vcc"]
        grp.append(f"v_exp_f32 {reg}, {reg}")
        ops.append(grp)
        if r >= 1:                               # row sum of the PREVIOUS register (its exp has had a gap to complete); two partial sums
            pk, prr = (r - 1) >> 4, (r - 1) & 15
            ops.append([f"v_add_f32 %[l{c}{(r - 1) & 1}], %[l{c}{(r - 1) & 1}], {sreg(c, pk, prr, 1)}"])
        if r >= 3 and (r & 1):                   # pack the pair (r - 3, r - 2): both summed already
            i = (r - 3) >> 1
            kbp, ii = i >> 3, i & 7
            ops.append([f"v_cvt_pk_bf16_f32 {sreg(c, kbp, ii, 1)}, {sreg(c, kbp, 2 * ii, 1)}, {sreg(c, kbp, 2 * ii + 1, 1)}"])
    ops.append([f"v_add_f32 %[l{c}1], %[l{c}1], {sreg(c, 1, 15, 1)}"])
    ops.append([f"v_cvt_pk_bf16_f32 {sreg(c, 1, 7, 1)}, {sreg(c, 1, 14, 1)}, {sreg(c, 1, 15, 1)}"])
    return ops


def check_softmax():
    """the in-place compaction never overwrites a value that is still to be read"""
    for c in (0, 1):
        for masked in (False, True):
            live = {(kb, rr): "s" for kb in range(2) for rr in range(16)}      # s: score, e: exp'd, a: added, p: packed-away, P: packed pair
            for grp in softmax(c, masked):
                for ins in grp:
                    f = ins.replace(",", "").split()
                    num = lambda tok: int(tok[1:]) - S_BASE - c * 32
                    if f[0] == "v_exp_f32":
                        n = num(f[1]); assert live[(n >> 4, n & 15)] == "s"; live[(n >> 4, n & 15)] = "e"
                    elif f[0] == "v_add_f32":
                        n = num(f[3]); assert live[(n >> 4, n & 15)] == "e", (ins, live[(n >> 4, n & 15)]); live[(n >> 4, n & 15)] = "a"
                    elif f[0] == "v_cvt_pk_bf16_f32":
                        d, a, b = num(f[1]), num(f[2]), num(f[3])
                        assert live[(a >> 4, a & 15)] == "a" and live[(b >> 4, b & 15)] == "a", ins
                        assert live[(d >> 4, d & 15)] == "p" or d in (a, b), ins      # the destination's old value has been consumed
                        live[(a >> 4, a & 15)] = live[(b >> 4, b & 15)] = "p"
                        live[(d >> 4, d & 15)] = "P"
            assert sorted(k for k, v in live.items() if v == "P") == [(kb, i) for kb in range(2) for i in range(8)], live


def spread(ops, gaps):
    """assign the op groups to the gaps in order, as evenly as possible; returns {gap: [instructions]}"""
    out = {g: [] for g in gaps}
    n, m = len(ops), len(gaps)
    for i, grp in enumerate(ops):
        out[gaps[i * m // n]] += grp
    return out


def loads(t):
    """2 K + 2 V^T LDS-DMA pieces of tile t (this wave's groups w, w + 4)"""
    out = []
    for i in range(2):
        out.append((f"s_add_i32 m0, s{S_MK}, {i * 4096}", I(f"global_load_lds_dwordx4 %[gk{i}], s[{S_KSRC}:{S_KSRC + 1}]", ld=t, ring="mk")))
        out.append((f"s_add_i32 m0, s{S_MV}, {i * 4096}", I(f"global_load_lds_dwordx4 %[gv{i}], s[{S_VSRC}:{S_VSRC + 1}]", ld=t, ring="mv")))
    return out


def rotate_after_loads():
    """source bases += one tile; LDS-DMA destinations -> next stage (both rings 4 stages of 0x2000; K ring at K_RING)"""
    return [f"s_add_u32 s{S_KSRC}, s{S_KSRC}, 8192", f"s_addc_u32 s{S_KSRC + 1}, s{S_KSRC + 1}, 0",
            f"s_add_u32 s{S_VSRC}, s{S_VSRC}, 128", f"s_addc_u32 s{S_VSRC + 1}, s{S_VSRC + 1}, 0",
            f"s_add_i32 s{S_MK}, s{S_MK}, 0x2000", f"s_and_b32 s{S_MK}, s{S_MK}, 0x7fff", I(f"s_or_b32 s{S_MK}, s{S_MK}, 0x{K_RING:x}", rot="mk"),
            f"s_add_i32 s{S_MV}, s{S_MV}, 0x2000", I(f"s_and_b32 s{S_MV}, s{S_MV}, 0x7fff", rot="mv")]


def rotate_base(name):
    """a fragment read base (lane part + stage * 0x2000 < 0x8000) -> next stage"""
    if "norot" in ABL:
        return {}
    return {2 * k: [f"v_add_u32 %[{name}{k}], 0x2000, %[{name}{k}]", I(f"v_and_b32 %[{name}{k}], 0x7fff, %[{name}{k}]", rot=name if k == 3 else None)]
            for k in range(4)}


def merge(*dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out.setdefault(k, [])
            out[k] += v
    return out


HAZ = "s_nop 7"          # an XDL write must be >= 12 wait states ahead of a VALU read of the same register (hipcc inserts s_nop 11 there)

ABL = set()        # ablation builds (timing only, results garbage): "novalu", "noread", "noload", "nosync", "norot" (read bases stay at stage 0); "stage": the loads / waits / barriers only


def rd(reads):
    return {} if "noread" in ABL else {i: [r] for i, r in enumerate(reads)}


def tile(first, last, has_loads=None, t=0):
    """one tile; returns (phases, pending) where `pending` = {gap: [...]} fillers for phase 1 of the NEXT tile (softmax1's second half).
    `t` only labels the instructions for check_stream."""
    L = []
    if has_loads is None:
        has_loads = not last
    assert not (last and has_loads)
    sm0, sm1 = softmax(0, last), softmax(1, last)
    if "novalu" in ABL:
        sm0, sm1 = [["s_nop 0"]], [["s_nop 0"]]
    # ---- phase 1: S0(t) on X | loads of tile t + 2 | (softmax1(t-1) tail: merged in by flatten as `carry`)
    f1 = {}
    if has_loads and "noload" not in ABL:
        ld = {}
        for j, (m0, g) in enumerate(loads(t + 2)):
            ld.setdefault(2 * j, []).append(m0)
            ld.setdefault(2 * j + 1, []).append(g)
        f1 = merge(ld, {NPH - 1: rotate_after_loads()})                  # behind the last load; SALU only
    L.append(("ph1", mfma_s(0, t), f1))
    # ---- softmax0(t) window: phases 2 + 3 (or phase 3 alone on the first tile); nothing in its first gap (MFMA -> VALU hazard) nor in its last
    if not first:
        win = [("ph2", g) for g in range(1, NPH)] + [("ph3", g) for g in range(0, NPH - 1)]
    else:
        win = [("ph3", g) for g in range(1, NPH - 1)]
    sp0 = spread(sm0, win)
    sp0[win[0]] = [HAZ] + sp0[win[0]]
    # ---- phase 2: PV1(t-1) on Y
    if not first:
        L.append(("ph2", mfma_pv(1, t - 1), {g: v for (p, g), v in sp0.items() if p == "ph2"}))
    # ---- phase 3: S1(t) on X | reads V^T(t) -> Y | K read bases -> next stage (phase 4 of the PREVIOUS tile made the last read through them)
    f3 = merge(rd(reads_v(t)), {g: v for (p, g), v in sp0.items() if p == "ph3"})
    if not last:
        f3 = merge(f3, rotate_base("vk"))
    L.append(("ph3", mfma_s(1, t), f3))
    if not last and "nosync" not in ABL:
        # tile t + 1 (issued one iteration ago, or by the shell) must have landed; this iteration's 4 loads (tile t + 2) stay in flight
        L.append(("sync", [I("s_waitcnt vmcnt(%d)" % (4 if has_loads and "noload" not in ABL else 0), sync=t), "s_barrier"], {}))
    # ---- phase 4: PV0(t) on Y | reads K(t+1) -> X | V^T read bases -> next stage | softmax1(t) first half
    if not last:
        win1 = [("ph4", g) for g in range(1, NPH)] + [("nx1", g) for g in range(0, NPH - 1)]
    else:
        win1 = [("ph4", g) for g in range(1, NPH)]
    sp1 = spread(sm1, win1)
    sp1[win1[0]] = [HAZ] + sp1[win1[0]]
    f4 = {g: v for (p, g), v in sp1.items() if p == "ph4"}
    if not last:
        f4 = merge(rd(reads_k(t + 1)), f4, rotate_base("vc"))
    L.append(("ph4", mfma_pv(0, t), f4))
    pending = {g: v for (p, g), v in sp1.items() if p == "nx1"}
    if last:
        L.append(("ph5", ["s_nop 3"] + mfma_pv(1, t), {}))        # the V^T(t) fragments are still in Y; softmax1 finished inside phase 4
    return L, pending


def flatten(L, carry):
    out = []
    for name, mf, fill in L:
        if name == "sync" or name == "ph5":
            out += mf if name == "sync" or "stage" not in ABL else []
            continue
        if name == "ph1":
            fill = merge(fill, carry)
        if "stage" in ABL:          # a wave without queries: the loads, their bookkeeping, the waits and the barriers
            out += [i for g in sorted(fill) for i in fill[g] if name == "ph1" and not i.startswith("v_")]
            continue
        out += interleave(mf, fill)
    return out


def resolve_waits(lines, outstanding):
    """put `s_waitcnt lgkmcnt(N)` in front of every MFMA whose fragment is not known to have arrived: N = the ds_reads issued behind that
    fragment's.  `outstanding`: the (buffer, slot) of the reads in flight where `lines` begins, oldest first (LDS returns data in order)."""
    out, queue = [], list(outstanding)
    for ins in lines:
        m = getattr(ins, "meta", {})
        if "rd" in m:
            queue.append(m["rd"])
        if "use" in m and m["use"] in queue:
            n = len(queue) - 1 - max(i for i, s in enumerate(queue) if s == m["use"])
            out.append(I(f"s_waitcnt lgkmcnt({n})", wait_for=m["use"]))
            queue = queue[len(queue) - n:]
        out.append(ins)
    return out, queue


K_SLOTS = [(FX, s) for s in range(8)]          # every tile begins with the 8 K reads of phase 4 (or of the prologue) in flight


def tile_lines(first, last, has_loads, carry, t):
    L, pend = tile(first, last, has_loads, t)
    lines, left = resolve_waits(flatten(L, carry), [] if ABL & {"noread", "stage"} else K_SLOTS)
    assert left == ([] if last or ABL & {"noread", "stage"} else K_SLOTS), left
    return lines, pend


def prologue():
    out = [f"s_mov_b32 s{S_M0SAVE}, m0", f"s_mov_b64 s[{S_KSRC}:{S_KSRC + 1}], %[ksrc]", f"s_mov_b64 s[{S_VSRC}:{S_VSRC + 1}], %[vsrc]",
           f"s_mov_b32 s{S_MK}, %[mk]", f"s_mov_b32 s{S_MV}, %[mv]", f"s_mov_b32 s{S_CNT}, %[mid]"]
    if "stage" in ABL:
        return out
    return out + [f"v_accvgpr_write_b32 a{i}, 0" for i in range(O_BASE, O_BASE + 64)] + \
        ["v_mov_b32 %[l00], 0", "v_mov_b32 %[l01], 0", "v_mov_b32 %[l10], 0", "v_mov_b32 %[l11], 0"] + \
        ([] if "noread" in ABL else reads_k(0))                          # K(0) fragments for the very first phase (exposed once per workgroup)


def epilogue():
    return [f"s_mov_b32 m0, s{S_M0SAVE}"] + ([] if "stage" in ABL else ["s_nop 15", "s_nop 15"])


def body_multi(unroll=None):
    """n_tiles >= 3: first tile (loads tile 2), `mid` = n_tiles - 3 loop iterations, the tile before the last (no loads left), the last tile.
    unroll = k: the straight-line stream with k loop iterations, for check_stream"""
    k = 0 if unroll is None else unroll
    first, pend_f = tile_lines(True, False, True, {}, 0)
    mids = [tile_lines(False, False, True, pend_f, 1 + i) for i in range(max(k, 1))]
    pen, pend_p = tile_lines(False, False, False, pend_f, k + 1)
    last, _ = tile_lines(False, True, False, pend_f, k + 2)
    assert all(p == pend_f for _, p in mids) and pend_p == pend_f
    assert all(str.__eq__(a, b) for m, _ in mids for a, b in zip(m, mids[0][0]))      # the loop body does not depend on t
    if unroll is not None:
        return prologue() + first + [i for m, _ in mids[:k] for i in m] + pen + last + epilogue()
    out = prologue() + first
    out += [f"s_cmp_eq_u32 s{S_CNT}, 0", "s_cbranch_scc1 L_a64_pen%=", "L_a64_loop%=:"]
    out += mids[0][0]
    out += [f"s_sub_u32 s{S_CNT}, s{S_CNT}, 1", f"s_cmp_lg_u32 s{S_CNT}, 0", "s_cbranch_scc1 L_a64_loop%=", "L_a64_pen%=:"]
    return out + pen + last + epilogue()


def body_two():
    """n_tiles == 2 (both tiles staged by the shell)"""
    first, pend = tile_lines(True, False, False, {}, 0)
    last, _ = tile_lines(False, True, False, pend, 1)
    return prologue() + first + last + epilogue()


def body_single():
    only, _ = tile_lines(True, True, False, {}, 0)
    return prologue() + only + epilogue()


# ------------------------------------------------------------------------------------------------------------------------ structural checks
def check_stream(lines, n_tiles):
    """replay a straight-line stream (see the module docstring for what is asserted)"""
    fragtag, rdseq, lds_q, issued = {}, {}, [], 0            # fragment contents, sequence number of each slot's last read, reads in flight
    vm_q = []                                                # loads in flight (tile numbers); the shell waited for tiles 0 and 1
    stage = {"vk": 0, "vc": 0, "mk": 2, "mv": 2}             # which tile's ring stage each base points at
    landed = min(1, n_tiles - 1)                             # tiles <= landed are in LDS for every wave (the shell's barrier: 0 and 1)
    n_mfma = 0
    for ins in lines:
        for kind, a, b in re.findall(r"\b([vas])\[?(\d+)(?::(\d+))?\]?", ins if not ins.startswith(("s_nop", "s_waitcnt", "L_")) else ""):
            lo, hi = int(a), int(b or a)
            ok = {"v": S_BASE <= lo and hi < V_END, "a": hi < A_END, "s": S_LO <= lo and hi < S_HI}[kind]
            assert ok, ("register outside the declared budget", ins)
        m = getattr(ins, "meta", {})
        if "rd" in m:
            what, tt, slot = m["tag"]
            assert stage["vk" if what == "K" else "vc"] == tt, ("read base points at another tile's stage", ins, stage, tt)
            assert tt <= landed, ("read of a tile no sync has proven landed", ins, tt, landed)
            fragtag[m["rd"]], rdseq[m["rd"]] = m["tag"], issued
            lds_q.append(issued)
            issued += 1
        elif "wait_for" in m:
            n = int(re.search(r"lgkmcnt\((\d+)\)", ins).group(1))
            assert n == issued - 1 - rdseq[m["wait_for"]] and n <= 15, ("lgkmcnt is not the number of reads issued behind the awaited one", ins)
            lds_q = lds_q[len(lds_q) - n:] if n else []
        elif "use" in m:
            n_mfma += 1
            assert fragtag.get(m["use"]) == m["expect"], ("MFMA on a fragment of another tile / slot", ins, fragtag.get(m["use"]), m["expect"])
            assert rdseq[m["use"]] not in lds_q, ("MFMA on a fragment whose read has not been waited for", ins)
        elif "ld" in m:
            assert stage[m["ring"]] == m["ld"] and m["ld"] < n_tiles, ("load into another tile's stage, or of a tile that does not exist", ins, stage)
            assert m["ld"] - 4 < 0 or m["ld"] - 4 <= landed - 2, ins        # the stage's previous tenant (tile - 4) is long consumed by every wave
            vm_q.append(m["ld"])
        elif "sync" in m:
            n = int(re.search(r"vmcnt\((\d+)\)", ins).group(1))
            need = m["sync"] + 1
            assert n == sum(1 for x in vm_q if x > need), ("vmcnt is not the number of loads issued behind the awaited tile's", ins, vm_q)
            vm_q = vm_q[len(vm_q) - n:] if n else []
            assert all(x > need for x in vm_q)
            landed = need
        if m.get("rot"):
            stage[m["rot"]] += 1
    assert n_mfma == 32 * n_tiles and not vm_q and landed == n_tiles - 1, (n_mfma, vm_q, landed, n_tiles)


def check_all():
    global ABL
    assert not ABL
    check_softmax()
    check_stream(body_single(), 1)
    check_stream(body_two(), 2)
    for k in range(5):                      # 3 .. 7 tiles: every slot of the ring and its wrap
        check_stream(body_multi(unroll=k), 3 + k)
    # the staging-only bodies issue the same loads, vmcnt waits and barriers, in the same order, as the full bodies
    sig = lambda ls: [str(i) for i in ls if i.startswith(("global_load_lds", "s_barrier", "s_waitcnt vmcnt", "s_add_i32 m0", "s_cbranch", "L_"))]
    full = sig(body_multi()), sig(body_two())
    ABL = {"stage"}
    stg = sig(body_multi()), sig(body_two())
    ABL = set()
    assert full == stg and full[0].count("s_barrier") == 3 and full[1].count("s_barrier") == 1


def main():
    global ABL
    check_all()
    print("// GENERATED by gen_attn64_w4.py -- do not edit.  Key loop of attn64_w4_kernel (attention.hip); see the generator's docstring.")
    emit("A64_BODY_MULTI", body_multi())
    emit("A64_BODY_TWO", body_two())
    emit("A64_BODY_SINGLE", body_single())
    ABL = {"stage"}
    emit("A64_STAGE_MULTI", body_multi())
    emit("A64_STAGE_TWO", body_two())
    print("#ifdef MI355_ABLATE          // timing only: results are garbage")
    for name, ab in (("NOVALU", {"novalu"}), ("NOREAD", {"noread"}), ("MFMA", {"novalu", "noread"}), ("MFMA_NOSYNC", {"novalu", "noread", "nosync", "noload"}),
                     ("NOROT", {"norot"})):
        ABL = ab
        emit(f"A64_BODY_MULTI_{name}", body_multi())
    print("#endif")
    ABL = set()
    print("#define A64_CLOBBERS " + clobbers(*regs("a", 0, A_END), *regs("v", S_BASE, V_END), *regs("s", S_LO, S_HI), "vcc", "scc", "memory"))
    print()
    print("#define A64_WQ_(x, r0, r1, r2, r3) asm volatile(\"v_accvgpr_write_b32 a\" #r0 \", %0\\n v_accvgpr_write_b32 a\" #r1 \", %1\\n"
          " v_accvgpr_write_b32 a\" #r2 \", %2\\n v_accvgpr_write_b32 a\" #r3 \", %3\" : : \"v\"(x[0]), \"v\"(x[1]), \"v\"(x[2]), \"v\"(x[3]))")
    for c in range(2):
        for kk in range(4):
            b = Q_BASE + (c * 4 + kk) * 4
            print(f"#define A64_WRITE_Q_{c}_{kk}(x) A64_WQ_(x, {b}, {b + 1}, {b + 2}, {b + 3})")
    print("#define A64_RO_(d, i, r) { float t_; asm volatile(\"v_accvgpr_read_b32 %0, a\" #r : \"=v\"(t_)); d[i] = t_; }")
    for c in range(2):
        for db in range(2):
            b = O_BASE + (c * 2 + db) * 16
            print(f"#define A64_READ_O_{c}_{db}(d) " + " ".join(f"A64_RO_(d, {i}, {b + i})" for i in range(16)))


if __name__ == "__main__":
    main()

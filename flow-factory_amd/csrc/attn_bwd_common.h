// mi355_flow -- what the flash-attention BACKWARD kernels of head_dim 64 (attention_bwd.hip) and 128 (attention128_bwd.hip) share: the tile
// layout in LDS, the per-lane addresses into it, the LDS-DMA stagers and counted waits of the 4-slot ring, the work decomposition and the
// output transpose.  The layout below is also the CONTRACT of the generated main loops (gen_attn_bwd.py -> attn_bwd*_asm.inc): their asm
// operands are named at the end of this comment, and every function that fills one says so.
//
// Tiles.  A streamed operand tile is [TB = 64 rows][HD] bf16, kept as HD / 64 SUB-TILES of [64 rows][64 d] (8 KiB each, d halves one after
// the other), so an LDS row is 128 bytes at either head_dim.  A ring slot is  tile A | tile B  (Q | dO in the dK/dV pass, K | V in the dQ
// pass), in the dK/dV pass followed by the tile's 64 -L and 64 -Delta floats (512 bytes).  Inside a row the 16-byte chunks are XOR-swizzled:
// physical chunk = logical ^ swz2(row).
//
// Lane addresses (byte offsets inside a sub-tile; lg = lane >> 5):
//   frag_offset(prow, lg, kk)    the ds_read_b128 A fragment of k-step kk: row row_perm(lane & 31), logical chunk 2 kk + lg;
//   tr_piece_offset(.., db, jj)  the 8-byte piece this lane supplies to the `ds_read_b64_tr_b16` of d block db: row 8 lg + 4 jj + (i >> 2),
//                                columns 32 db + 16 g1 + 4 (i & 3) .. (i = lane & 15, g1 = (lane >> 4) & 1); + 2048 bytes per 16-row step,
//                                + 4096 for the second 32-row half.
// A row's 128 bytes are bits 0..6 of the offset, the chunk index bits 4..6, and an XOR with swz2 stays inside them, so
//   frag_offset(.., kk)           = frag_offset(.., 0) ^ 32 kk            (chunk 2 kk + lg = 2 kk ^ lg)
//   tr_piece_offset(.., 1, jj)    = tr_piece_offset(.., 0, jj) ^ 64       (chunk 4 db + ..  = 4 db ^ ..)
// which is how the generated loops form the addresses they are not handed.
//
// Operands of the generated loops (ABWD*_ASM; "+v" ones are advanced round the ring by the loop):
//   la            nld_read_offset<HD>(lg): the half-wave's -L | -Delta C operands inside slot 0 (dK/dV pass)
//   r0 (r1..r3)   frag_offset(.., 0) (.. 3): the head_dim-64 dQ loop takes all four, every other loop forms r0 ^ 32 kk itself
//   a0, a1 (a2, a3)  tr_piece_offset(.., 0, 0 / 1) (and (.., 1, 0 / 1): the head_dim-64 dQ loops take all four, the others form a0 / a1 ^ 64)
//   g0            dma_src_offset<HD>(wave, lane): this lane's 16 bytes of the 8 rows a wave's LDS-DMA instruction moves, from the tile's base
//   g2            dma_nld_offset(wave, lane): its 16 bytes of the tile's -L | -Delta floats (lanes 0..7)
//   grow(0, 1)    own_row_offset<HD>(row, lg): the lane's own key (query) row's first fragment, from p0 / p1
//   b0, b1, b2    tile_addr<HD>() / nld_addr() of the first tile the loop stages itself (first_loop_tile(nt)) of A, B, -L | -Delta
//   p0, p1        the (b, h)'s rows of the operands held per lane: k, v (dK/dV pass) or q, dO (dQ pass)
//   nl, nd        -L, -Delta of the lane's query (dQ pass);   vrem: head_dim 128's tail masks (attention128_bwd.hip)
//   nt, wv        tile count, wave index.  The loops address the ring from LDS byte 0: require_lds_base0().
#pragma once
#include "kernels.h"

namespace mi355 {
namespace {

constexpr int TB = 64;                     // rows of the streamed dimension per tile
constexpr int SUB = TB * 64 * 2;           // one [64][64] bf16 sub-tile: 8 KiB
// NWAVES waves x 32 lanes-of-interest keys (pass 1) / queries (pass 2) per workgroup.  At head_dim 64: 4 waves, two (three) workgroups per
// CU: 8-wave workgroups (one per CU, half the L2 -> LDS operand traffic: every workgroup streams ALL tiles of its (b, h)) measured 4-8 %
// SLOWER (profiles/r03u_attn_bwd_waves_ab.txt) -- independent barriers per CU overlap better than one.
constexpr int NWAVES = 4;
constexpr int NSTAGE = 4;                  // ring slots: loads run three tiles ahead
constexpr float LN2 = 0.6931471805599453f;

template <int HD> constexpr int tile_bytes = TB * HD * 2;                                    // one operand tile
template <int HD, bool NLD> constexpr int slot_bytes = 2 * tile_bytes<HD> + (NLD ? 512 : 0);   // tile A | tile B [| -L[64] | -Delta[64]]

// Swizzle: physical 16-byte chunk = logical ^ swz2(row), swz2 = f ^ ((f & 1) << 2) with f = (row >> 1) & 7: a permutation of the 8 even (odd)
// rows a ds_read_b128 lane group touches (conflict-free), and rows r, r + 2 of a transposed read's 4-row block sit in different 64-byte
// halves of their 128-byte rows (4 rows x 64 bytes = 64 distinct banks).
__device__ __forceinline__ int swz2(int row) {
    const int f = (row >> 1) & 7;
    return f ^ ((f & 1) << 2);
}

__device__ __forceinline__ bf16x8 frag4(unsigned a, unsigned b, unsigned c, unsigned d) {
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    const u32x4 u = {a, b, c, d};
    return __builtin_bit_cast(bf16x8, u);
}

// ---- lane addresses (see the file head); prow = row_perm(lane & 31), lg = lane >> 5
__device__ __forceinline__ int frag_offset(int prow, int lg, int kk) { return prow * 128 + (((2 * kk + lg) ^ swz2(prow)) << 4); }
__device__ __forceinline__ int tr_piece_offset(int lane, int lg, int db, int jj) {
    const int i = lane & 15, g1 = (lane >> 4) & 1;
    const int row = 8 * lg + 4 * jj + (i >> 2);
    const int ch = 4 * db + 2 * g1 + ((i & 3) >> 1);
    return row * 128 + ((ch ^ swz2(row)) << 4) + (i & 1) * 8;
}
// (Every kernel fills its offR[kk] / trb[db][jj] tables, or its asm operands, by `#pragma unroll` loops of its own over these two: hipcc
// simplifies a helper before it inlines it, and a table unrolled in a helper reaches the kernel's entry block in another instruction order --
// the register allocation of the pipelined shells has no slack for that.)
template <int HD> __device__ __forceinline__ unsigned nld_read_offset(int lg) { return (unsigned)(2 * tile_bytes<HD> + 32 * lg); }
template <int HD> __device__ __forceinline__ unsigned dma_src_offset(int wave, int lane) {
    const int srow = wave * 8 + (lane >> 3);
    return (unsigned)(srow * (2 * HD) + (((lane & 7) ^ swz2(srow)) << 4));
}
__device__ __forceinline__ unsigned dma_nld_offset(int wave, int lane) { return (unsigned)(wave * 128 + (lane & 7) * 16); }
template <int HD> __device__ __forceinline__ unsigned own_row_offset(int row, int lg) { return (unsigned)(row * (2 * HD) + lg * 16); }
template <int HD> __device__ __forceinline__ unsigned long long tile_addr(const bf16_t* rows, int t) {
    return (unsigned long long)(rows + (long)t * TB * HD);
}
__device__ __forceinline__ unsigned long long nld_addr(const float* nld, int t) { return (unsigned long long)(nld + (long)t * 2 * TB); }

// The generated loops address the ring from LDS byte 0 (the kernels that include them must own no static LDS)
__device__ __forceinline__ void require_lds_base0(const char* smem) {
    if ((unsigned)(size_t)(__attribute__((address_space(3))) const char*)smem != 0u) __builtin_trap();
}

// ---- work decomposition.  Every kernel takes block `wid % nblk` of (b, h) `wid / nblk`, wid = xcd_remap(blockIdx.x, nblk * H * B): the blocks
// of one (b, h) share an L2.  The key range (head_dim 128 only; launch_attention_bwd() of head_dim 64 has neither form and its kernels do not
// read these fields): S_kv > 0 = the keys are another sequence (cross-attention) with its own padded row count; kv_len = ragged text
// (Qwen-Image), sample b's keys end at kv_len[b].
// (p BY VALUE: behind a reference to the kernel's parameter block hipcc no longer proves the later kv_len[b] load unclobbered and turns that
// scalar load into a vector load + readfirstlane)
__device__ __forceinline__ int key_count(const AttnBwdParams p) { return p.S_kv > 0 ? p.S_kv : p.S; }
__device__ __forceinline__ long key_rows_pad(const AttnBwdParams p) { return p.S_kv > 0 ? p.S_kv_pad : p.S_pad; }      // k, v, dk, dv: [B][H][.][HD]
__device__ __forceinline__ int valid_keys(const int* kv_len, long b, int Sk) {
    return kv_len ? min(Sk, max(1, __builtin_amdgcn_readfirstlane(kv_len[b]))) : Sk;
}

// ---- the ring: LDS-DMA in, counted waits
// one [64 rows][HD] row-major operand tile -> LDS (128-byte rows, chunks XOR-swizzled by swz2(row)): a wave's instruction moves 8 rows of a
// sub-tile, 8 / NWAVES instructions per wave and sub-tile
template <int HD>
__device__ __forceinline__ void stage_tile(const bf16_t* src, char* dst, int wave, int lane) {
#pragma unroll
    for (int sub = 0; sub < HD / 64; ++sub) {
        const bf16_t* s = src + sub * 64;
        char* d = dst + sub * SUB;
#pragma unroll
        for (int i = 0; i < 8 / NWAVES; ++i) {
            const int grp = wave + i * NWAVES;
            const int row = grp * 8 + (lane >> 3);
            const int c = (lane & 7) ^ swz2(row);
            __builtin_amdgcn_global_load_lds((gptr_t)(s + (long)row * HD + c * 8), (lptr_t)(d + grp * 1024), 16, 0, 0);
        }
    }
}
// tile t of the two streamed operands -> ring slot `buf`; NLD: and the tile's -L | -Delta, 128 contiguous floats of p.nld ([b h][tile][2][64]):
// wave w moves floats 32 w .. 32 w + 31 with the first 8 lanes of one 16-byte LDS-DMA instruction, so every wave issues the same number of VM
// operations per tile: HD / 16 (+ 1).  nld_src = this lane's 16 bytes of them: tile t's floats + 32 wave + 4 (lane & 7) (formed by the caller:
// the pipelined shells and the older kernels keep different parts of that sum in registers).
template <int HD, bool NLD>
__device__ __forceinline__ void stage_slot(char* smem, int buf, const bf16_t* A, const bf16_t* B, const float* nld_src, int t, int wave, int lane) {
    char* base = smem + buf * slot_bytes<HD, NLD>;
    if constexpr (HD == 64) {      // (each file's order of forming the two tile addresses: the pipelined shells' register allocation hangs on it)
        stage_tile<HD>(A + (long)t * TB * HD, base, wave, lane);
        stage_tile<HD>(B + (long)t * TB * HD, base + tile_bytes<HD>, wave, lane);
    } else {
        const bf16_t* a = A + (long)t * TB * HD;
        const bf16_t* b = B + (long)t * TB * HD;
        stage_tile<HD>(a, base, wave, lane);
        stage_tile<HD>(b, base + tile_bytes<HD>, wave, lane);
    }
    if constexpr (NLD)
        if (lane < 8) __builtin_amdgcn_global_load_lds((gptr_t)nld_src, (lptr_t)(base + 2 * tile_bytes<HD> + wave * 128), 16, 0, 0);
}
// The generated loops find tiles 0..2 in slots 0..2 and ALWAYS three tiles' loads in flight (past the end the last tile is loaded again, into
// a slot nobody reads): their shells stage slot t <- tile min(t, nt - 1) for t = 0, 1, 2; the loop's own first load is tile min(nt - 1, 3)
__device__ __forceinline__ int first_loop_tile(int nt) { return nt - 1 < 3 ? nt - 1 : 3; }
// `ahead` tiles were issued after the one about to be read, PER VM operations each (vmcnt retires in order), then the workgroup barrier
template <int PER>
__device__ __forceinline__ void wait_tiles_ahead(int ahead) {
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// ---- transposed reads and the MFMAs they feed, as inline assembly with the fragments in FIXED registers:
//  * hipcc guards every C-level LDS read it knows to be an LDS read (the `ds_read_tr16_b64` builtin, address-space-3 pointers) with
//    `s_waitcnt vmcnt(0)` while any LDS-DMA is in flight -- it cannot tell the ring stages apart -- which would drain the tiles just put in
//    flight (the plain fragment reads go through generic pointers and are not guarded);
//  * a fragment is two 64-bit reads into the halves of one 4-register MFMA operand: as separate asm outputs they would need packing moves.
// LDS returns in order, so `lgkmcnt(n)` retires all but the last n reads (compiler-issued fragment reads in flight only make it wait longer).
#define TR_RD(dst, a, off) "ds_read_b64_tr_b16 " dst ", " a " offset:" #off "\n\t"
#define MFMA32(acc, afrag, b) "v_mfma_f32_32x32x16_bf16 " acc ", " afrag ", " b ", " acc "\n\t"
#define TR_CLOBBER16 "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239"
#define TR_CLOBBER32 TR_CLOBBER16, "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255"

// ---- epilogue.  Call with the accumulators read out (ABWD*_READ_ACC_n in the order of the loop's register map): every wave is done with the
// ring (the generated loops end with vmcnt(0): its LDS-DMA writes too), which becomes the waves' private output-transpose regions.
// OPAQUE (the pipelined shells): the lane arithmetic below hangs off an opaque copy of the lane id -- hipcc would otherwise form those
// addresses in front of the loop and keep them alive across it, where the head_dim-64 shell has sixteen VGPRs and not one more (one more
// register and the kernel drops to one wave per SIMD).
struct OutStage {
    char* ob;
    int lane;
};
template <int HD, bool OPAQUE>
__device__ __forceinline__ OutStage epilogue_begin(char* smem, int wave, int lane) {
    __syncthreads();
    if constexpr (OPAQUE) asm volatile("" : "+v"(lane));
    return {smem + wave * (32 * 2 * HD), lane};
}
// accumulators acc[db][r] = X^T[d = 32 db + 8 (r>>2) + 4 lg + (r&3)][column = lane & 31] -> rows dst[(row0 + column)][0..HD) bf16, scaled,
// for rows < row_limit: through the wave's 32 rows x 2 HD bytes of LDS (16-byte chunks XOR-swizzled by row & 7), HD / 8 lanes per row out
template <int HD>
__device__ __forceinline__ void store_rows(const f32x16 (&acc)[HD / 32], float scale, OutStage o, bf16_t* dst, int row0, int row_limit) {
    constexpr int LSH = HD == 64 ? 3 : 4;      // log2(lanes per row)
    static_assert(HD == 64 || HD == 128, "head_dim");
    const int lane = o.lane, lq = lane & 31, lg = lane >> 5;
#pragma unroll
    for (int db = 0; db < HD / 32; ++db)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int d0 = 32 * db + 8 * a + 4 * lg;
            uint2 w = {pack_bf16(acc[db][4 * a] * scale, acc[db][4 * a + 1] * scale),
                       pack_bf16(acc[db][4 * a + 2] * scale, acc[db][4 * a + 3] * scale)};
            const int chunk = (d0 >> 3) ^ (lq & 7);
            *(uint2*)(o.ob + lq * (2 * HD) + chunk * 16 + (d0 & 7) * 2) = w;
        }
    __builtin_amdgcn_wave_barrier();      // wave-private region, in-order LDS
#pragma unroll
    for (int it = 0; it < (32 << LSH) / 64; ++it) {
        const int r = it * (64 >> LSH) + (lane >> LSH), c = lane & ((1 << LSH) - 1);
        const uint4 val = *(const uint4*)(o.ob + r * (2 * HD) + ((c ^ (r & 7)) << 4));
        if (row0 + r < row_limit) *(uint4*)(dst + (long)(row0 + r) * HD + c * 8) = val;
    }
    __builtin_amdgcn_wave_barrier();
}

}  // namespace
}  // namespace mi355

// mi355_flow -- attention with head_dim 128 (FLUX.1 joint / single-stream attention): non-causal
// softmax(q k^T / sqrt(128)) v, flash-style, for gfx950.  Same construction as attention.hip (d = 64):
//   q, k : [B][H][S_pad][128] bf16 (per-head RMSNorm + RoPE already applied), vT : [B][H][128][S_pad] bf16;
//   one wave = 32 queries, one query per lane: S^T = K.Q^T (8 k-steps of 16 over d) and O^T += V^T.P^T (4 blocks of 32
//   d-rows) on v_mfma_f32_32x32x16_bf16; K rows fed in the permuted order that makes the packed softmax registers the
//   B fragments of the second MFMA; deferred rescale with -m as the MFMA C operand.
// Per 64-key tile a wave issues 32 MFMAs (1024 cycles) against the same ~130 VALU slots as d = 64, so this kernel is
// MFMA-bound where the d = 64 one is VALU-co-bound.  The K tile is kept as TWO 64x64 sub-tiles (d halves) so that every
// LDS row stays 128 bytes and the conflict-free XOR swizzle of the d = 64 kernel carries over unchanged.
#include "kernels.h"

namespace mi355 {
namespace {

constexpr int HD = 128;
constexpr int KV = 64;                          // keys per tile
constexpr int QW = 32;                          // queries per wave
constexpr int SUB_BYTES = KV * 64 * 2;          // one 64x64 bf16 sub-tile (8 KiB)
constexpr int K_BYTES = 2 * SUB_BYTES;          // K tile: d halves
constexpr int V_BYTES = HD * KV * 2;            // V^T tile: 128 rows (d) x 64 keys
constexpr int STAGE_BYTES = K_BYTES + V_BYTES;  // 32 KiB
constexpr float SCALE_LOG2E = 0.08838834764831845f * 1.4426950408889634f;   // 1/sqrt(128) * log2(e)

// STATIC: |score| <= p.score_bound <= 60 proven by the caller (see attention.hip): no running max, no rescale.
template <int NWAVE, bool STATIC = false>
__global__ __launch_bounds__(NWAVE * 64, 2) void attn128_kernel(Attn128Params p) {
    constexpr int QB = QW * NWAVE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 31, lg = lane >> 5;
    // XCD-aware work order (blockIdx % 8 = XCD): the q-blocks of one (b, h) share an L2
    const int nqb = (p.S + QB - 1) / QB;
    const int wid = xcd_remap(blockIdx.x, nqb * p.H * p.B);
    const int qblk = wid % nqb;
    const int bhi = wid / nqb;
    const int h = bhi % p.H, b = bhi / p.H;
    const long bh = (long)b * p.H + h;
    if (p.mode) {       // data-dependent static / running-max split: every workgroup decides by its own (b, h) (wave-uniform loads)
        const float bound = sqrtf(__uint_as_float(p.qmax2[bh]) * __uint_as_float(p.kmax2[bh])) * 1.01f;
        if ((bound <= 60.f) != (p.mode == 1)) return;
    }
    // keys / values may be a different sequence (cross-attention): S_kv == 0 means self-attention over the S queries
    int Skv = p.S_kv > 0 ? p.S_kv : p.S;
    if (p.kv_len) Skv = min(Skv, max(1, __builtin_amdgcn_readfirstlane(p.kv_len[b])));
    const int Skv_pad = p.S_kv > 0 ? p.S_kv_pad : p.S_pad;
    const bf16_t* Qg = p.q + bh * p.S_pad * HD;
    const bf16_t* Kg = p.k + bh * Skv_pad * HD;
    const bf16_t* Vg = p.vT + bh * HD * Skv_pad;

    // ---- Q fragments (B operand): lane holds Q[q][kk*16 + lg*8 .. +8], kk = 0..7
    const int q_row = qblk * QB + wave * QW + lq;
    const int q_ld = q_row < p.S ? q_row : p.S - 1;
    bf16x8 qf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) qf[kk] = *(const bf16x8*)(Qg + (long)q_ld * HD + kk * 16 + lg * 8);
    if (!p.q_prescaled) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
            u32x4 u = __builtin_bit_cast(u32x4, qf[kk]);
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = pack_bf16(bf_lo(u[e]) * SCALE_LOG2E, bf_hi(u[e]) * SCALE_LOG2E);
            qf[kk] = __builtin_bit_cast(bf16x8, u);
        }
    }

    // ---- staging: a tile = 32 glds groups of 8 rows x 128 B: groups 0..15 = K (sub-tile g>>3, rows 8*(g&7)..), 16..31 = V^T rows
    constexpr int NG = 16 / NWAVE;
    const bf16_t* srcK[NG];
    const bf16_t* srcV[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        const int g = wave + i * NWAVE;                   // 0..15
        const int krow = (g & 7) * 8 + (lane >> 3);       // key inside the tile
        const int kc = (lane & 7) ^ ((krow >> 1) & 7);
        srcK[i] = Kg + (long)krow * HD + (g >> 3) * 64 + kc * 8;            // + tile*64*HD
        const int vrow = g * 8 + (lane >> 3);             // d
        const int vc = (lane & 7) ^ ((vrow >> 1) & 7);
        srcV[i] = Vg + (long)vrow * Skv_pad + vc * 8;                        // + tile*64
    }
    auto stage = [&](int t, int buf) {
        char* base = smem + buf * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int g = wave + i * NWAVE;
            __builtin_amdgcn_global_load_lds((gptr_t)(srcK[i] + (long)t * KV * HD), (lptr_t)(base + g * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(srcV[i] + (long)t * KV), (lptr_t)(base + K_BYTES + g * 1024), 16, 0, 0);
        }
    };

    // ---- fragment read offsets
    const int krow = row_perm(lq);
    int offK[4];
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) offK[k4] = krow * 128 + (((2 * k4 + lg) ^ ((krow >> 1) & 7)) << 4);
    int offV[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) offV[c] = K_BYTES + lq * 128 + (((2 * c + lg) ^ ((lq >> 1) & 7)) << 4);

    f32x16 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = (f32x16){0};
    float l_run = 0.f;
    const int nt = (Skv + KV - 1) / KV;
    stage(0, 0);

    constexpr float THR = 6.0f;
    float m_run = 0.f;
    f32x16 negm = (f32x16){0};
    const bool wave_active = (qblk * QB + wave * QW) < p.S;   // waves past the last query only help staging
    for (int t = 0; t < nt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < nt) stage(t + 1, (t + 1) & 1);
        if (!wave_active) continue;
        const char* sb = smem + (t & 1) * STAGE_BYTES;
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const bf16x8 kf = *(const bf16x8*)(sb + offK[0] + kb * 4096);
            if constexpr (STATIC) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[0], (f32x16){0}, 0, 0, 0);
            else s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[0], negm, 0, 0, 0);
        }
#pragma unroll
        for (int kk = 1; kk < 8; ++kk) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const bf16x8 kf = *(const bf16x8*)(sb + (kk >> 2) * SUB_BYTES + offK[kk & 3] + kb * 4096);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], s[kb], 0, 0, 0);
            }
        }
        if (t == nt - 1) {
            const int kbase = t * KV + 8 * lg;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kbase + 32 * kb + 16 * (r >> 3) + (r & 7);
                    if (key >= Skv) s[kb][r] = -1e30f;
                }
        }
        float mx = 0.f;
        if constexpr (!STATIC) {
        mx = fmaxf(fmaxf(s[0][0], s[0][1]), s[0][2]);
#pragma unroll
        for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, s[0][r]), s[0][r + 1]);
        mx = fmaxf(mx, s[0][15]);
#pragma unroll
        for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, s[1][r]), s[1][r + 1]);
        }
        if (!STATIC && (t == 0 || __any(mx > THR))) {
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float delta = (t == 0) ? mx : fmaxf(mx, 0.f);
            // (the first tile may LOWER m: delta < 0.  l and O are still zero then, and for a query whose first-tile scores are all below -128
            //  2^(-delta) overflows to inf: 0 * inf = NaN in l and O.  Clamped: the factor of the first tile is 1, every later one is unchanged.)
            const float alpha = __builtin_amdgcn_exp2f(fminf(-delta, 0.f));
            m_run += delta;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kb][r] -= delta;
#pragma unroll
            for (int r = 0; r < 16; ++r) negm[r] = -m_run;
            l_run *= alpha;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
        }
        float psum = 0.f;
        unsigned pk[2][8];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(s[kb][r]);
                const float p1 = __builtin_amdgcn_exp2f(s[kb][r + 1]);
                psum += p0 + p1;
                pk[kb][r >> 1] = pack_bf16(p0, p1);
            }
        l_run += psum;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int kb = c >> 1, sh = (c & 1) * 4;
            typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
            const u32x4 uu = {pk[kb][sh + 0], pk[kb][sh + 1], pk[kb][sh + 2], pk[kb][sh + 3]};
            const bf16x8 pf = __builtin_bit_cast(bf16x8, uu);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const bf16x8 vf = *(const bf16x8*)(sb + offV[c] + db * 4096);
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[db], 0, 0, 0);
            }
        }
    }

    // ---- finalize: 1/l, stage O through LDS (row = query, 256 B; 16-byte chunks XOR-swizzled by q & 7) for full-row stores
    l_run += __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_run;
    // training-mode forward: log2-sum-exp per query for the backward (a store only; the rollout passes lse == nullptr and runs this same binary)
    if (p.lse && lg == 0 && q_row < p.S) p.lse[bh * p.S_pad + q_row] = m_run + __log2f(l_run);
    __syncthreads();
    char* ob = smem + wave * (QW * HD * 2);
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int d0 = 32 * db + 8 * a + 4 * lg;
            uint2 w = {pack_bf16(o[db][4 * a] * inv, o[db][4 * a + 1] * inv), pack_bf16(o[db][4 * a + 2] * inv, o[db][4 * a + 3] * inv)};
            const int chunk = (d0 >> 3) ^ (lq & 7);
            *(uint2*)(ob + lq * 256 + chunk * 16 + (d0 & 7) * 2) = w;
        }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int r = it * 4 + (lane >> 4), c = lane & 15;
        const uint4 val = *(const uint4*)(ob + r * 256 + ((c ^ (r & 7)) << 4));
        const int qi = qblk * QB + wave * QW + r;
        if (qi < p.S) {
            bf16_t* dst = (qi < p.n_first) ? p.o_first + ((long)b * p.n_first + qi) * p.ld_first
                                           : p.o_rest + ((long)b * (p.S - p.n_first) + (qi - p.n_first)) * p.ld_rest;
            uint4 v = val;
            if (p.o_add) {      // optional addend (a RUNTIME branch, like lse): store bf16(bf16(o) + o_add); o_add may be the output buffer itself
                const uint4 ad = *(const uint4*)(p.o_add + ((long)b * p.S + qi) * p.ld_first + h * HD + c * 8);      // (n_first == S: launch_attention128)
                v.x = pack_bf16(bf_lo(v.x) + bf_lo(ad.x), bf_hi(v.x) + bf_hi(ad.x));
                v.y = pack_bf16(bf_lo(v.y) + bf_lo(ad.y), bf_hi(v.y) + bf_hi(ad.y));
                v.z = pack_bf16(bf_lo(v.z) + bf_lo(ad.z), bf_hi(v.z) + bf_hi(ad.z));
                v.w = pack_bf16(bf_lo(v.w) + bf_lo(ad.w), bf_hi(v.w) + bf_hi(ad.w));
            }
            *(uint4*)(dst + h * HD + c * 8) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 4-wave kernel with a HAND-SCHEDULED key loop (attn128_w4_asm.inc, generated by gen_attn128_w4.py: its docstring has the schedule): one
// wave per SIMD, TWO chains of 32 queries per wave, the softmax of one chain on the VALU under the MFMAs of the other; static softmax
// only (score_bound <= 60), self-attention only (S_kv == 0; per-sample key counts `kv_len` supported).  Same LDS images, same K-row
// permutation, same arithmetic per element as attn128_kernel<8, true> (row sums are formed in another order: results agree to fp32
// rounding of l, not bit for bit).  The shell owns addressing, Q fragments (written to AGPRs before the loop), finalisation and stores.
#include "attn128_w4_asm.inc"

template <int RG>
__global__ __launch_bounds__(256) void attn128_w4_kernel(Attn128Params p) {
    constexpr int QB = 256;                         // 4 waves x 2 chains x 32 queries
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 31, lg = lane >> 5;
    const int nqb = (p.S + QB - 1) / QB;
    const int wid = xcd_remap(blockIdx.x, nqb * p.H * p.B);
    const int qblk = wid % nqb;
    const int bhi = wid / nqb;
    const int h = bhi % p.H, b = bhi / p.H;
    const long bh = (long)b * p.H + h;
    if (p.mode) {       // data-dependent static / running-max split: every workgroup decides by its own (b, h) (wave-uniform loads)
        const float bound = sqrtf(__uint_as_float(p.qmax2[bh]) * __uint_as_float(p.kmax2[bh])) * 1.01f;
        if ((bound <= 60.f) != (p.mode == 1)) return;
    }
    int Skv = p.S;
    if (p.kv_len) Skv = min(Skv, max(1, __builtin_amdgcn_readfirstlane(p.kv_len[b])));
    const bf16_t* Qg = p.q + bh * p.S_pad * HD;
    const bf16_t* Kg = p.k + bh * p.S_pad * HD;
    const bf16_t* Vg = p.vT + bh * HD * p.S_pad;
    const int nt = (Skv + KV - 1) / KV;

    // ---- K(0), V^T(0) -> stage 0 of their rings (V ring at LDS 0, K ring at 64 KiB); wave w stages groups w, w + 4, w + 8, w + 12
    unsigned gk[4], gv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int g = wave + 4 * i;
        const int krow = (g & 7) * 8 + (lane >> 3);
        const int kc = (lane & 7) ^ ((krow >> 1) & 7);
        gk[i] = (unsigned)((krow * HD + (g >> 3) * 64 + kc * 8) * 2);
        const int vrow = g * 8 + (lane >> 3);
        const int vc = (lane & 7) ^ ((vrow >> 1) & 7);
        gv[i] = (unsigned)(((long)vrow * p.S_pad + vc * 8) * 2);
        __builtin_amdgcn_global_load_lds((gptr_t)((const char*)Kg + gk[i]), (lptr_t)(smem + 65536 + g * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)((const char*)Vg + gv[i]), (lptr_t)(smem + g * 1024), 16, 0, 0);
        if (nt > 1) {                           // tile 1 -> stage 1 (the loop loads two tiles ahead)
            __builtin_amdgcn_global_load_lds((gptr_t)((const char*)Kg + gk[i] + KV * HD * 2), (lptr_t)(smem + 65536 + 16384 + g * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)((const char*)Vg + gv[i] + KV * 2), (lptr_t)(smem + 16384 + g * 1024), 16, 0, 0);
        }
    }
    // ---- Q fragments -> a[128:191] (the MFMA B operand of the S^T products)
    {
#define A128_LOADQ(C, KK)                                                                                           \
        {                                                                                                          \
            const int q_row = qblk * QB + wave * 64 + C * 32 + lq;                                                \
            const int q_ld = q_row < p.S ? q_row : p.S - 1;                                                        \
            typedef __attribute__((ext_vector_type(4))) unsigned u32x4;                                            \
            u32x4 u = *(const u32x4*)(Qg + (long)q_ld * HD + KK * 16 + lg * 8);                                    \
            if (!p.q_prescaled)                                                                                    \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) u[e] = pack_bf16(bf_lo(u[e]) * SCALE_LOG2E, bf_hi(u[e]) * SCALE_LOG2E); \
            A128_WRITE_Q_##C##_##KK(u);                                                                            \
        }
        A128_LOADQ(0, 0) A128_LOADQ(0, 1) A128_LOADQ(0, 2) A128_LOADQ(0, 3) A128_LOADQ(0, 4) A128_LOADQ(0, 5) A128_LOADQ(0, 6) A128_LOADQ(0, 7)
        A128_LOADQ(1, 0) A128_LOADQ(1, 1) A128_LOADQ(1, 2) A128_LOADQ(1, 3) A128_LOADQ(1, 4) A128_LOADQ(1, 5) A128_LOADQ(1, 6) A128_LOADQ(1, 7)
#undef A128_LOADQ
    }
    // ---- fragment read bases (lane part; stage and block offsets are immediates / rotated inside the loop)
    const int krow = row_perm(lq);
    unsigned vk0, vk1, vk2, vk3, vc0, vc1, vc2, vc3, vp0 = 0, vp1 = 0, vp2 = 0, vp3 = 0;
    {
        unsigned t[4], u[4];
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) t[k4] = 65536u + (unsigned)(krow * 128 + (((2 * k4 + lg) ^ ((krow >> 1) & 7)) << 4));
#pragma unroll
        for (int c = 0; c < 4; ++c) u[c] = (unsigned)(lq * 128 + (((2 * c + lg) ^ ((lq >> 1) & 7)) << 4));
        vk0 = t[0]; vk1 = t[1]; vk2 = t[2]; vk3 = t[3]; vc0 = u[0]; vc1 = u[1]; vc2 = u[2]; vc3 = u[3];
    }
    const int rem = Skv - (nt - 1) * KV;                           // valid keys of the last tile, 1 .. 64
    const int vrem = rem - 8 * lg;
    const float vneg = -1e30f;
    // loads inside the loop start with tile 2: sources two tiles ahead, destinations stage 2
    const unsigned long long ksrc = (unsigned long long)Kg + 2ull * KV * HD * 2, vsrc = (unsigned long long)Vg + 2ull * KV * 2;
    const unsigned mk = __builtin_amdgcn_readfirstlane(65536u + 32768u + wave * 1024u), mv = __builtin_amdgcn_readfirstlane(32768u + wave * 1024u);
    const int mid = nt - 3;
    float l00, l01, l10, l11;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#define A128_OPERANDS                                                                                                                       \
        : [l00] "=&v"(l00), [l01] "=&v"(l01), [l10] "=&v"(l10), [l11] "=&v"(l11), [vk0] "+v"(vk0), [vk1] "+v"(vk1), [vk2] "+v"(vk2),        \
          [vk3] "+v"(vk3), [vc0] "+v"(vc0), [vc1] "+v"(vc1), [vc2] "+v"(vc2), [vc3] "+v"(vc3), [vp0] "+v"(vp0), [vp1] "+v"(vp1),            \
          [vp2] "+v"(vp2), [vp3] "+v"(vp3)                                                                                                  \
        : [gk0] "v"(gk[0]), [gk1] "v"(gk[1]), [gk2] "v"(gk[2]), [gk3] "v"(gk[3]), [gv0] "v"(gv[0]), [gv1] "v"(gv[1]), [gv2] "v"(gv[2]),     \
          [gv3] "v"(gv[3]), [vrem] "v"(vrem), [vneg] "v"(vneg), [ksrc] "s"(ksrc), [vsrc] "s"(vsrc), [mk] "s"(mk), [mv] "s"(mv), [mid] "s"(mid) \
        : A128_CLOBBERS
    if (nt == 1) asm volatile(A128_BODY_SINGLE A128_OPERANDS);
    else if (nt == 2) asm volatile(A128_BODY_TWO A128_OPERANDS);
    else if constexpr (RG == 101) asm volatile(A128_BODY_MULTI_NOVALU A128_OPERANDS);       // ablations: timing only
    else if constexpr (RG == 102) asm volatile(A128_BODY_MULTI_NOREAD A128_OPERANDS);
    else if constexpr (RG == 103) asm volatile(A128_BODY_MULTI_MFMA A128_OPERANDS);
    else if constexpr (RG == 104) asm volatile(A128_BODY_MULTI_MFMA_NOSYNC A128_OPERANDS);
    else asm volatile(A128_BODY_MULTI A128_OPERANDS);
#undef A128_OPERANDS
    // ---- finalize per chain: 1 / l, O through LDS (row = query, 256 B, chunks XOR-swizzled by q & 7; the V ring is free: every wave is
    //      past the loop's last barrier-protected read only after this barrier) for full-row stores
    __syncthreads();
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    const int lqe = lane_e & 31, lge = lane_e >> 5;
#define A128_FINISH(C)                                                                                              \
    {                                                                                                              \
        float l = l##C##0 + l##C##1;                                                                               \
        l += __shfl_xor(l, 32, 64);                                                                                \
        const float inv = 1.0f / l;                                                                                \
        if (p.lse && lge == 0) {          /* training-mode forward: log2-sum-exp (static softmax: no running max) */ \
            const int ql = qblk * QB + wave * 64 + C * 32 + lqe;                                                   \
            if (ql < p.S) p.lse[bh * p.S_pad + ql] = __log2f(l);                                                   \
        }                                                                                                          \
        char* ob = smem + (wave * 2 + C) * (32 * HD * 2);                                                          \
        f32x16 o;                                                                                                  \
        A128_STORE_DB(C, 0) A128_STORE_DB(C, 1) A128_STORE_DB(C, 2) A128_STORE_DB(C, 3)                            \
        __builtin_amdgcn_wave_barrier();                                                                           \
        _Pragma("unroll") for (int it = 0; it < 8; ++it) {                                                         \
            const int r = it * 4 + (lane_e >> 4), c = lane_e & 15;                                                 \
            const uint4 val = *(const uint4*)(ob + r * 256 + ((c ^ (r & 7)) << 4));                                \
            const int qi = qblk * QB + wave * 64 + C * 32 + r;                                                     \
            if (qi < p.S) {                                                                                        \
                bf16_t* dst = (qi < p.n_first) ? p.o_first + ((long)b * p.n_first + qi) * p.ld_first                \
                                               : p.o_rest + ((long)b * (p.S - p.n_first) + (qi - p.n_first)) * p.ld_rest; \
                *(uint4*)(dst + h * HD + c * 8) = val;                                                             \
            }                                                                                                      \
        }                                                                                                          \
    }
#define A128_STORE_DB(C, DB)                                                                                        \
        A128_READ_O_##C##_##DB(o)                                                                                  \
        _Pragma("unroll") for (int a = 0; a < 4; ++a) {                                                            \
            const int d0 = 32 * DB + 8 * a + 4 * lge;                                                              \
            uint2 w = {pack_bf16(o[4 * a] * inv, o[4 * a + 1] * inv), pack_bf16(o[4 * a + 2] * inv, o[4 * a + 3] * inv)}; \
            const int chunk = (d0 >> 3) ^ (lqe & 7);                                                               \
            *(uint2*)(ob + lqe * 256 + chunk * 16 + (d0 & 7) * 2) = w;                                             \
        }
    A128_FINISH(0)
    A128_FINISH(1)
#undef A128_STORE_DB
#undef A128_FINISH
}

template <int RG>
static hipError_t launch128_w4(const Attn128Params& p, hipStream_t stream) {
    constexpr int smem = 131072;                    // V ring 64 KiB + K ring 64 KiB
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)attn128_w4_kernel<RG>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(attn128_w4_kernel<RG>, dim3(((p.S + 255) / 256) * p.H * p.B), dim3(256), smem, stream, p);
    return hipGetLastError();
}

int g_attn128_variant = 0;   // 0 (default): the 4-wave hand-scheduled kernel where it applies (static softmax, self-attention), else 8 waves x 32
                             // queries, 1 workgroup / CU; 1: 4 compiler-scheduled waves, 2 workgroups / CU; 5: never the hand-scheduled kernel (A/B)

template <int NWAVE, bool STATIC>
hipError_t launch128(const Attn128Params& p, hipStream_t stream) {
    auto kern = attn128_kernel<NWAVE, STATIC>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * STAGE_BYTES);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    constexpr int QB = 32 * NWAVE;
    hipLaunchKernelGGL(kern, dim3(((p.S + QB - 1) / QB) * p.H * p.B), dim3(NWAVE * 64), 2 * STAGE_BYTES, stream, p);
    return hipGetLastError();
}

}  // namespace

int g_attn128_op_bound = 0;   // operator-level entry (unit tests, A/B): the |score| bound it asserts (0 = none: running-max kernel)
void set_attn128_variant(int v) { g_attn128_variant = v; }
void set_attn128_op_bound(int v) { g_attn128_op_bound = v; }
int get_attn128_op_bound() { return g_attn128_op_bound; }
int get_attn128_variant() { return g_attn128_variant; }

hipError_t launch_attention128(const Attn128Params& p, hipStream_t stream) {
    if (sched_trace_on()) {
        const size_t q = (size_t)p.B * p.H * p.S_pad * 256, kv = (size_t)p.B * p.H * (p.S_kv > 0 ? p.S_kv_pad : p.S_pad) * 256;
        const size_t r1 = (size_t)p.B * p.n_first, r2 = (size_t)p.B * (p.S - p.n_first);
        sched_trace_launch("attention128", stream, {treg(p.q, q), treg(p.k, kv), treg(p.vT, kv), treg(p.kv_len, p.kv_len ? (size_t)p.B * 4 : 0),
                                                    treg(p.o_add, p.o_add && r1 ? ((r1 - 1) * p.ld_first + (size_t)p.H * 128) * 2 : 0)},
                           {treg(p.o_first, r1 ? ((r1 - 1) * p.ld_first + (size_t)p.H * 128) * 2 : 0),
                            treg(p.o_rest, r2 ? ((r2 - 1) * p.ld_rest + (size_t)p.H * 128) * 2 : 0)});
    }
    if (p.S <= 0 || p.S_pad < p.S || p.n_first < 0 || p.n_first > p.S) return hipErrorInvalidValue;
    if (p.S_kv > 0 ? (p.S_kv_pad % KV != 0 || p.S_kv_pad < p.S_kv) : (p.S_pad % KV != 0)) return hipErrorInvalidValue;
    // the addend is read by the attn128_kernel epilogue only (cross-attention never takes the hand-scheduled kernel), with the output's own strides
    if (p.o_add && (p.S_kv <= 0 || p.n_first != p.S || p.qmax2)) return hipErrorInvalidValue;
    if (g_attn128_variant == 1) return launch128<4, false>(p, stream);
    bool stat = p.score_bound > 0.f && p.score_bound <= 60.f;
    if (!stat && p.qmax2 && p.kmax2 && p.S_kv == 0 && g_attn128_variant == 0) {
        // no weight-side proof (Wan: RMSNorm across heads), but the producers of q and k measured their row norms: both kernels are launched and
        // every workgroup runs or exits by its own (b, h).  (b, h) pairs whose scores can exceed 60 keep the running max; the others -- all of
        // them for ordinary activations -- take the hand-scheduled static kernel.  The exiting workgroups cost a few microseconds per launch.
        Attn128Params a = p;
        a.mode = 1; a.score_bound = 60.f;
        hipError_t e = launch128_w4<16>(a, stream);
        if (e != hipSuccess) return e;
        a.mode = 2; a.score_bound = 0.f;
        return launch128<8, false>(a, stream);
    }
    if (stat && p.S_kv == 0 && g_attn128_variant != 5) {         // the 4-wave hand-scheduled kernel wherever it applies (default)
        if (g_attn128_variant == 101) return launch128_w4<101>(p, stream);      // (ablation builds: timing only)
        if (g_attn128_variant == 102) return launch128_w4<102>(p, stream);
        if (g_attn128_variant == 103) return launch128_w4<103>(p, stream);
        if (g_attn128_variant == 104) return launch128_w4<104>(p, stream);
        return launch128_w4<16>(p, stream);
    }
    if (stat) return launch128<8, true>(p, stream);
    return launch128<8, false>(p, stream);
}

}  // namespace mi355

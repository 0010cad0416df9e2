// mi355_flow -- shared device helpers (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace mi355 {

typedef unsigned short bf16_t;  // raw bfloat16 bits
typedef __attribute__((ext_vector_type(8))) short bf16x8;   // one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) float f32x4;    // 16x16 MFMA accumulator
typedef __attribute__((ext_vector_type(16))) float f32x16;  // 32x32 MFMA accumulator
typedef __attribute__((ext_vector_type(2))) __bf16 bf16v2;
typedef __attribute__((ext_vector_type(2))) float f32v2;

enum DType : int { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2 };

__device__ __forceinline__ float bf2f(bf16_t b) { return __uint_as_float(((unsigned)b) << 16); }
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// two floats -> packed bf16x2 (round-to-nearest-even; lowers to v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    f32v2 v = {lo, hi};
    bf16v2 r = __builtin_convertvector(v, bf16v2);
    return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ bf16_t f2bf(float f) { return (bf16_t)(pack_bf16(f, 0.f) & 0xffffu); }
__device__ __forceinline__ float round_bf16(float f) { return bf2f(f2bf(f)); }

// 1/x by v_rcp_f32 (1 ulp): every use below is followed by a bf16 rounding (2^-9), an IEEE division would cost ~10 VALU ops
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float silu_f(float x) { return x * fast_rcp(1.0f + __expf(-x)); }
// GELU(tanh approximation), as torch.nn.functional.gelu(approximate="tanh"):
//   0.5 x (1 + tanh(u)) = x * sigmoid(2u),  u = sqrt(2/pi) (x + 0.044715 x^3)
// evaluated as x / (1 + 2^(-x (c0 + c1 x^2))) with log2(e) folded into the constants: 5 VALU + v_exp + v_rcp per element
__device__ __forceinline__ float gelu_tanh_f(float x) {
    const float c0 = 2.0f * 0.7978845608028654f * 1.4426950408889634f;
    const float c1 = c0 * 0.044715f;
    const float t = x * (c0 + c1 * x * x);
    return x * fast_rcp(1.0f + __builtin_amdgcn_exp2f(-t));
}

// d/dx of gelu_tanh_f: s + x s (1 - s) 2u'(x), s = sigmoid(2u), 2u = x (k0 + k1 x^2), (2u)' = k0 + 3 k1 x^2
// The guard-free and the guarded EPI_DGELU epilogues of gemm.hip are different instantiations and must agree bit for bit whichever kernel a grid
// selects: every multiply-add is an explicit fma and contraction is off, so that hipcc cannot fuse in one of them what it leaves unfused in the
// other (tests/test_gpu_gemm_epilogues.py found the ping-pong kernel's dpre an ulp off the 128x128 kernel's; the q/k epilogue has the same rule).
__device__ __forceinline__ float gelu_tanh_grad_f(float x) {
#pragma clang fp contract(off)
    const float k0 = 2.0f * 0.7978845608028654f, k1 = k0 * 0.044715f;
    const float x2 = x * x;
    const float s = fast_rcp(1.0f + __expf(-x * __builtin_fmaf(k1, x2, k0)));
    return __builtin_fmaf(x * s * (1.0f - s), __builtin_fmaf(3.0f * k1, x2, k0), s);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float row16_sum_dpp(float v) {      // sum over the 16 lanes of a DPP row, in every lane
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xf, 0xf, false));
    };
    using std::integral_constant;
    v += dpp(v, integral_constant<int, 0xB1>{});      // quad_perm [1,0,3,2]
    v += dpp(v, integral_constant<int, 0x4E>{});      // quad_perm [2,3,0,1]
    v += dpp(v, integral_constant<int, 0x141>{});     // row_half_mirror
    v += dpp(v, integral_constant<int, 0x140>{});     // row_mirror
    return v;
}

// 8 bf16 (one 16-byte access) <-> 8 floats
__device__ __forceinline__ void unpack8(const uint4 u, float (&v)[8]) {
    v[0] = bf_lo(u.x); v[1] = bf_hi(u.x); v[2] = bf_lo(u.y); v[3] = bf_hi(u.y);
    v[4] = bf_lo(u.z); v[5] = bf_hi(u.z); v[6] = bf_lo(u.w); v[7] = bf_hi(u.w);
}
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    return make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
}

// source / destination of an LDS-DMA load (__builtin_amdgcn_global_load_lds)
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// XCD-aware work order: the hardware deals workgroup ids round-robin over the 8 XCDs (id % 8), each with a private L2.  Workgroup `wid` of
// `nwg` takes the work item at its XCD's contiguous share of [0, nwg) + its turn on that XCD, so neighbouring items (the blocks of one
// (batch, head), the tiles of one operand panel) hit the same L2.
__device__ __forceinline__ int xcd_remap(int wid, int nwg) {
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = wid & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (wid >> 3);
}

// The 32x32x16 MFMA's output row i (0..31) -> row offset inside the 32-row block its A operand is fed in: with this order the 16 accumulator
// registers of a block, packed to bf16 in register order, ARE the B fragments of a second product (8 consecutive rows per lane)
__device__ __forceinline__ int row_perm(int i) {
    const int a = i >> 3, g = (i >> 2) & 1, b = i & 3;
    return 16 * (a >> 1) + 8 * g + 4 * (a & 1) + b;
}

// storage-dtype load/store of a latent element (fp32 / bf16 / fp16)
__device__ __forceinline__ float load_as_f32(const void* p, long i, int dt) {
    if (dt == DT_F32) return ((const float*)p)[i];
    if (dt == DT_BF16) return bf2f(((const bf16_t*)p)[i]);
    return (float)(((const _Float16*)p)[i]);
}
// value-round an fp32 to the storage dtype (the reference's `.to(dtype).float()`), with the
// fp16 clamp of cast_latents (reference models/abc.py:172-182)
__device__ __forceinline__ float round_to_dtype(float v, int dt) {
    if (dt == DT_F32) return v;
    if (dt == DT_BF16) return round_bf16(v);
    v = fminf(fmaxf(v, -65504.0f), 65504.0f);
    return (float)((_Float16)v);
}
__device__ __forceinline__ void store_from_f32(void* p, long i, int dt, float v) {
    if (dt == DT_F32) ((float*)p)[i] = v;
    else if (dt == DT_BF16) ((bf16_t*)p)[i] = f2bf(v);
    else ((_Float16*)p)[i] = (_Float16)fminf(fmaxf(v, -65504.0f), 65504.0f);
}

}  // namespace mi355

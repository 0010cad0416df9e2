// mi355_flow -- HBM-bound helper kernels of the MMDiT forward (ops K0-prologue, K1, K4, K12 of
// SURVEY.md 2.3): LayerNorm+AdaLN-modulate, patchify (im2col of the k2/s2 conv), pos-embed crop,
// sinusoidal timestep projection, dtype conversion.  All 16-byte vectorised, one wave per row
// where a row reduction is needed.
#include "kernels.h"

namespace mi355 {
namespace {

// ------------------------------------------------------------------ LayerNorm + modulate
// One wave per row; the row (D <= 8*64*MAXC) stays in registers: exact two-pass mean/variance.
// LN_MAXC 16-byte chunks per lane: 4 -> D <= 2048 (SD3.5, D = 1536), 8 -> D <= 4096 (FLUX.1, D = 3072), 12 -> D <= 6144 (the 40-head Wan
// transformers, D = 5120: Wan2.1-14B and both Wan2.2-A14B experts)
// SPLIT (two-group modulation, head_rows > 0): the first head_rows rows of sample b read modulation row 2 b, the others row 2 b + 1.  A compile-time
// flag: the unsplit instantiations keep their code.
template <int LN_MAXC, bool SPLIT = false>
__global__ __launch_bounds__(256) void ln_mod_kernel(LnModParams p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.M) return;
    const int nchunk = p.D >> 3;  // 8 bf16 per 16-byte chunk
    float v[LN_MAXC][8];
    float sum = 0.f;
    const bf16_t* xr = p.x + (long)row * p.D;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
            const uint4 u = *(const uint4*)(xr + ch * 8);
            v[c][0] = bf_lo(u.x); v[c][1] = bf_hi(u.x); v[c][2] = bf_lo(u.y); v[c][3] = bf_hi(u.y);
            v[c][4] = bf_lo(u.z); v[c][5] = bf_hi(u.z); v[c][6] = bf_lo(u.w); v[c][7] = bf_hi(u.w);
#pragma unroll
            for (int e = 0; e < 8; ++e) sum += v[c][e];
        }
    }
    const float mean = wave_sum(sum) / (float)p.D;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[c][e] - mean; sq += d * d; }
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)p.D + p.eps);
    const int b = row / p.rows_per_sample;
    long mrow = b;
    if constexpr (SPLIT) mrow = 2L * b + ((row - b * p.rows_per_sample) >= p.head_rows ? 1 : 0);
    const bf16_t* mod = p.mod + mrow * p.mod_ld;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
            float nv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) nv[e] = (v[c][e] - mean) * rstd;
            {
                const uint4 sc = *(const uint4*)(mod + p.scale_off + ch * 8);
                const uint4 sh = *(const uint4*)(mod + p.shift_off + ch * 8);
                uint4 o;
                o.x = pack_bf16(nv[0] * (1.f + bf_lo(sc.x)) + bf_lo(sh.x), nv[1] * (1.f + bf_hi(sc.x)) + bf_hi(sh.x));
                o.y = pack_bf16(nv[2] * (1.f + bf_lo(sc.y)) + bf_lo(sh.y), nv[3] * (1.f + bf_hi(sc.y)) + bf_hi(sh.y));
                o.z = pack_bf16(nv[4] * (1.f + bf_lo(sc.z)) + bf_lo(sh.z), nv[5] * (1.f + bf_hi(sc.z)) + bf_hi(sh.z));
                o.w = pack_bf16(nv[6] * (1.f + bf_lo(sc.w)) + bf_lo(sh.w), nv[7] * (1.f + bf_hi(sc.w)) + bf_hi(sh.w));
                *(uint4*)(p.out + (long)row * p.D + ch * 8) = o;
            }
            if (p.out2) {
                const uint4 sc = *(const uint4*)(mod + p.scale2_off + ch * 8);
                const uint4 sh = *(const uint4*)(mod + p.shift2_off + ch * 8);
                uint4 o;
                o.x = pack_bf16(nv[0] * (1.f + bf_lo(sc.x)) + bf_lo(sh.x), nv[1] * (1.f + bf_hi(sc.x)) + bf_hi(sh.x));
                o.y = pack_bf16(nv[2] * (1.f + bf_lo(sc.y)) + bf_lo(sh.y), nv[3] * (1.f + bf_hi(sc.y)) + bf_hi(sh.y));
                o.z = pack_bf16(nv[4] * (1.f + bf_lo(sc.z)) + bf_lo(sh.z), nv[5] * (1.f + bf_hi(sc.z)) + bf_hi(sh.z));
                o.w = pack_bf16(nv[6] * (1.f + bf_lo(sc.w)) + bf_lo(sh.w), nv[7] * (1.f + bf_hi(sc.w)) + bf_hi(sh.w));
                *(uint4*)(p.out2 + (long)row * p.D + ch * 8) = o;
            }
        }
    }
}

// ------------------------------------------------------------------ patchify (im2col, k = c*p*p + py*p + px)
// A token's C*p*p features go to columns col0 .. col0 + C*p*p of its row of `ld` elements (ld == C*p*p, col0 == 0: the dense layout).
__global__ void patchify_kernel(const void* lat, int dt, bf16_t* out, int B, int rep, int C, int h, int w, int p, int col0, int ld) {
    const int hp = h / p, wp = w / p, K = C * p * p;
    const long total = (long)B * rep * hp * wp * K;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const long tok = i / K;
        const int tx = (int)(tok % wp);
        const int ty = (int)((tok / wp) % hp);
        const int bb = (int)(tok / ((long)wp * hp));
        const int b = bb % B;  // cat([latents, latents]): replica r uses sample bb - r*B
        const int c = k / (p * p), py = (k / p) % p, px = k % p;
        const long src = (((long)b * C + c) * h + ty * p + py) * w + tx * p + px;
        out[tok * ld + col0 + k] = f2bf(load_as_f32(lat, src, dt));
    }
}

// first-frame merge (Wan2.2-TI2V image-to-video): the patches of ONE frame ff [B][C][h][w] go to rows [0, hp*wp) of every sample's `rps` rows of the
// dense patch matrix (both CFG replicas) -- the same element-wise conversion as patchify_kernel, so the rows equal those of a patchified merged tensor
__global__ void patchify_head_kernel(const void* ff, int dt, bf16_t* out, int B, int rep, int C, int h, int w, int p, int rps) {
    const int hp = h / p, wp = w / p, K = C * p * p;
    const long total = (long)B * rep * hp * wp * K;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const long tok = i / K;
        const int tx = (int)(tok % wp);
        const int ty = (int)((tok / wp) % hp);
        const int bb = (int)(tok / ((long)wp * hp));
        const int b = bb % B;
        const int c = k / (p * p), py = (k / p) % p, px = k % p;
        const long src = (((long)b * C + c) * h + ty * p + py) * w + tx * p + px;
        out[((long)bb * rps + ty * wp + tx) * K + k] = f2bf(load_as_f32(ff, src, dt));
    }
}

__global__ void pos_crop_kernel(const bf16_t* pos, bf16_t* out, int max_size, int hp, int wp, int D) {
    const int top = (max_size - hp) / 2, left = (max_size - wp) / 2;
    const int chunks = D >> 3;
    const long total = (long)hp * wp * chunks;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % chunks);
        const long tok = i / chunks;
        const int tx = (int)(tok % wp), ty = (int)(tok / wp);
        const long src = ((long)(top + ty) * max_size + left + tx) * D + ch * 8;
        *(uint4*)(out + tok * D + ch * 8) = *(const uint4*)(pos + src);
    }
}

// diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin]
__global__ void time_proj_kernel(const float* t, int rows, int dim, int t_round_dt, bf16_t* out) {
    const int half = dim / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * half) return;
    const int r = i / half, j = i % half;
    const float tv = round_to_dtype(t[r], t_round_dt);
    const float freq = expf(-9.210340371976184f * (float)j / (float)half);  // -ln(10000) * j / half
    const float a = tv * freq;
    out[(long)r * dim + j] = f2bf(cosf(a));
    out[(long)r * dim + half + j] = f2bf(sinf(a));
}

__global__ void convert_kernel(const void* src, int sdt, void* dst, int ddt, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = load_as_f32(src, i, sdt);
        store_from_f32(dst, i, ddt, v);  // fp16 destination clamps at +-65504 (cast_latents)
    }
}

// [rows][cols] of any dtype -> bf16 rows of `ld` elements, columns cols .. ld zero (a weight whose K is padded to the GEMM's multiple)
__global__ void convert_rows_kernel(const void* src, int sdt, bf16_t* dst, long rows, int cols, int ld) {
    const long total = rows * ld;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ld);
        const long r = i / ld;
        dst[i] = c < cols ? f2bf(load_as_f32(src, r * cols + c, sdt)) : f2bf(0.f);
    }
}

__global__ void gelu_erf_kernel(bf16_t* x, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = bf2f(x[i]);
        x[i] = f2bf(0.5f * v * (1.0f + erff(v * 0.70710678118654752f)));
    }
}

__global__ void add_bf16_kernel(const bf16_t* a, const bf16_t* b, bf16_t* out, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = f2bf(bf2f(a[i]) + bf2f(b[i]));
}

inline int grid_for(long total, int block) {
    long g = (total + block - 1) / block;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

}  // namespace

hipError_t launch_ln_mod(const LnModParams& p, hipStream_t stream) {
    if (sched_trace_on()) {
        const size_t xb = (size_t)p.M * p.D * 2, nb = (size_t)((p.M + p.rows_per_sample - 1) / (p.rows_per_sample > 0 ? p.rows_per_sample : 1));
        const size_t mrows = nb * (p.head_rows > 0 ? 2 : 1);      // two modulation rows per sample with the two-group split
        const size_t mb = mrows ? ((mrows - 1) * p.mod_ld + p.D) * 2 : 0;
        sched_trace_launch("ln_mod", stream, {treg(p.x, xb), treg(p.mod + p.shift_off, mb), treg(p.mod + p.scale_off, mb),
                                              treg(p.out2 ? p.mod + p.shift2_off : nullptr, mb), treg(p.out2 ? p.mod + p.scale2_off : nullptr, mb)},
                           {treg(p.out, xb), treg(p.out2, p.out2 ? xb : 0)});
    }
    if (p.D % 8 != 0 || p.D > 12 * 64 * 8 || p.M <= 0) return hipErrorInvalidValue;
    if (p.head_rows < 0 || (p.head_rows > 0 && (p.rows_per_sample <= 0 || p.head_rows > p.rows_per_sample))) return hipErrorInvalidValue;
    if (p.head_rows > 0) {
        if (p.D <= 2048) hipLaunchKernelGGL((ln_mod_kernel<4, true>), dim3((p.M + 3) / 4), dim3(256), 0, stream, p);
        else if (p.D <= 4096) hipLaunchKernelGGL((ln_mod_kernel<8, true>), dim3((p.M + 3) / 4), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((ln_mod_kernel<12, true>), dim3((p.M + 3) / 4), dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    if (p.D <= 2048) hipLaunchKernelGGL(ln_mod_kernel<4>, dim3((p.M + 3) / 4), dim3(256), 0, stream, p);
    else if (p.D <= 4096) hipLaunchKernelGGL(ln_mod_kernel<8>, dim3((p.M + 3) / 4), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(ln_mod_kernel<12>, dim3((p.M + 3) / 4), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_patchify(const void* lat, int dt, bf16_t* patches, int B, int rep, int C, int h, int w, int p,
                           hipStream_t stream) {
    if (sched_trace_on())
        sched_trace_launch("patchify", stream, {treg(lat, (size_t)B * C * h * w * (dt == DT_F32 ? 4 : 2))}, {treg(patches, (size_t)B * rep * C * h * w * 2)});
    const long total = (long)B * rep * (h / p) * (w / p) * C * p * p;
    hipLaunchKernelGGL(patchify_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, lat, dt, patches, B, rep, C, h,
                       w, p, 0, C * p * p);
    return hipGetLastError();
}

hipError_t launch_patchify_cols(const void* lat, int dt, bf16_t* patches, int B, int rep, int C, int h, int w, int p, int col0, int ld,
                                hipStream_t stream) {
    const int K = C * p * p;
    if (C < 1 || col0 < 0 || col0 + K > ld || h % p || w % p) return hipErrorInvalidValue;
    const long rows = (long)B * rep * (h / p) * (w / p);
    // The trace region is ONE span, first to last element touched: it also covers the columns of the rows in between that this launch does not
    // write.  Conservative: the latent-column and the condition-column launch of one patch buffer claim overlapping bytes although they write
    // disjoint ones -- harmless while both run on one stream (they do), a false race in the checker if they ever move to different streams.
    if (sched_trace_on())
        sched_trace_launch("patchify_cols", stream, {treg(lat, (size_t)B * C * h * w * (dt == DT_F32 ? 4 : 2))},
                           {treg(patches + col0, (size_t)((rows - 1) * ld + K) * 2)});
    hipLaunchKernelGGL(patchify_kernel, dim3(grid_for(rows * K, 256)), dim3(256), 0, stream, lat, dt, patches, B, rep, C, h, w, p, col0, ld);
    return hipGetLastError();
}

hipError_t launch_patchify_head(const void* ff, int dt, bf16_t* patches, int B, int rep, int C, int h, int w, int p, int rps, hipStream_t stream) {
    if (B < 1 || rep < 1 || C < 1 || p < 1 || h % p || w % p || rps < (h / p) * (w / p)) return hipErrorInvalidValue;
    const int K = C * p * p, head = (h / p) * (w / p);
    if (sched_trace_on())
        sched_trace_launch("patchify_head", stream, {treg(ff, (size_t)B * C * h * w * (dt == DT_F32 ? 4 : 2))},
                           {tregs(patches, (size_t)head * K * 2, (size_t)rps * K * 2, (size_t)B * rep)});
    hipLaunchKernelGGL(patchify_head_kernel, dim3(grid_for((long)B * rep * head * K, 256)), dim3(256), 0, stream, ff, dt, patches, B, rep, C, h, w, p, rps);
    return hipGetLastError();
}

hipError_t launch_pos_crop(const bf16_t* pos, bf16_t* out, int max_size, int hp, int wp, int D, hipStream_t stream) {
    if (hp > max_size || wp > max_size || D % 8) return hipErrorInvalidValue;
    const long total = (long)hp * wp * (D >> 3);
    hipLaunchKernelGGL(pos_crop_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, pos, out, max_size, hp, wp, D);
    return hipGetLastError();
}

hipError_t launch_time_proj(const float* t, int rows, int dim, int t_round_dt, bf16_t* out, hipStream_t stream) {
    if (sched_trace_on()) sched_trace_launch("time_proj", stream, {treg(t, (size_t)rows * 4)}, {treg(out, (size_t)rows * dim * 2)});
    const int total = rows * (dim / 2);
    hipLaunchKernelGGL(time_proj_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, t, rows, dim, t_round_dt, out);
    return hipGetLastError();
}

// One wave that samples {s_memtime (core clocks, slows down with the power throttle), s_memrealtime (100 MHz wall clock)} every
// ~sleep_iters * 8 k core clocks: launched on a side stream it sits in one wave slot beside the kernels under test and shows the core
// clock they are actually delivered (profiles/r02_power_clock_notes.txt: 1.44 GHz inside the bf16 GEMM at the 1.35 kW cap, not the 2.4 GHz
// the roofline peaks are quoted at).  Measurement tool (scripts/clock_under_load.py), never on the product path.
__global__ void clock_probe_kernel(long long* out, int n, int sleep_iters) {
    if (threadIdx.x != 0) return;
    for (int i = 0; i < n; ++i) {
        const long long c = clock64(), w = wall_clock64();
        out[2 * i] = c;
        out[2 * i + 1] = w;
        for (int k = 0; k < sleep_iters; ++k) __builtin_amdgcn_s_sleep(127);
    }
}

hipError_t launch_clock_probe(long long* out, int n, int sleep_iters, hipStream_t stream) {
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, stream, out, n, sleep_iters);
    return hipGetLastError();
}

hipError_t launch_convert(const void* src, int src_dt, void* dst, int dst_dt, long n, hipStream_t stream) {
    if (sched_trace_on())
        sched_trace_launch("convert", stream, {treg(src, (size_t)n * (src_dt == DT_F32 ? 4 : 2))}, {treg(dst, (size_t)n * (dst_dt == DT_F32 ? 4 : 2))});
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(convert_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, src, src_dt, dst, dst_dt, n);
    return hipGetLastError();
}

hipError_t launch_gelu_erf(bf16_t* x, long n, hipStream_t stream) {
    if (sched_trace_on()) sched_trace_launch("gelu_erf", stream, {treg(x, (size_t)n * 2)}, {treg(x, (size_t)n * 2)});
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gelu_erf_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, x, n);
    return hipGetLastError();
}

hipError_t launch_add_bf16(const bf16_t* a, const bf16_t* b, bf16_t* out, long n, hipStream_t stream) {
    if (sched_trace_on()) sched_trace_launch("add_bf16", stream, {treg(a, (size_t)n * 2), treg(b, (size_t)n * 2)}, {treg(out, (size_t)n * 2)});
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(add_bf16_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, a, b, out, n);
    return hipGetLastError();
}

hipError_t launch_convert_rows(const void* src, int src_dt, bf16_t* dst, long rows, int cols, int ld, hipStream_t stream) {
    if (rows < 1 || cols < 1 || ld < cols) return hipErrorInvalidValue;
    if (sched_trace_on())
        sched_trace_launch("convert_rows", stream, {treg(src, (size_t)rows * cols * (src_dt == DT_F32 ? 4 : 2))}, {treg(dst, (size_t)rows * ld * 2)});
    hipLaunchKernelGGL(convert_rows_kernel, dim3(grid_for(rows * ld, 256)), dim3(256), 0, stream, src, src_dt, dst, rows, cols, ld);
    return hipGetLastError();
}

}  // namespace mi355

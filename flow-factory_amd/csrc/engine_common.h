// mi355_flow -- host scaffolding shared by the engine translation units (engine.hip, flux_engine.hip, qwen_engine.hip, wan_engine.hip and the
// two VAE engines): error propagation into mi355_last_error(), the zero-initialised GEMM descriptor, the weight arenas + name table of a
// transformer engine (ParamTable), the weights of a double-stream block (DoubleW: FLUX.1 and Qwen-Image), the two-phase workspace allocator
// (Carver) and the hipGraph of a captured rollout loop (RolloutGraph).
#pragma once
#include <string.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"

#define HIPCHK(x)                                                                                                            \
    do {                                                                                                                     \
        hipError_t _e = (x);                                                                                                 \
        if (_e != hipSuccess) return mi355::errorf("%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__);  \
    } while (0)
#define CHK(x)             \
    do {                   \
        int _r = (x);      \
        if (_r) return _r; \
    } while (0)

namespace mi355 {

// C[M][N] = A[M][K] . W[N][K]^T with epilogue `epi`; every optional field zero, rows_per_sample = M, eps = 1e-6
inline GemmParams make_gemm(const bf16_t* A, long lda, const bf16_t* W, long ldw, long M, int N, int K, int epi, const float* bias,
                            bf16_t* out, long ldo) {
    GemmParams g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = (int)M; g.N = N; g.K = K; g.epi = epi; g.bias = bias;
    g.out = out; g.ldo = ldo; g.rows_per_sample = M > 0 ? (int)M : 1; g.eps = 1e-6f;
    return g;
}

// value-round an fp32 to a storage dtype on the host (bf16 / fp16 round-to-nearest-even)
inline float host_round(float v, int dt) {
    if (dt == DT_F32) return v;
    if (dt == DT_BF16) {
        unsigned u;
        memcpy(&u, &v, 4);
        u += 0x7fffu + ((u >> 16) & 1u);
        u &= 0xffff0000u;
        memcpy(&v, &u, 4);
        return v;
    }
    return (float)(_Float16)v;
}

// ---- weights of a transformer engine ------------------------------------------------------------------------------------------------
struct ParamSlot {
    void* dst;      // device destination (bf16_t* or float*)
    int dst_dt;     // DT_BF16 / DT_F32
    int64_t numel;  // elements expected
    bool bound;
};

// The bf16 and fp32 weight arenas and the table of parameter names.  The engine's layout() runs twice: a sizing pass (arenas null: a16 / a32
// only count and return null, reg records nothing), then, after alloc(), the real pass.  `who` = the calling C-ABI function, for the messages.
struct ParamTable {
    char* arena16 = nullptr;
    char* arena32 = nullptr;
    size_t used16 = 0, used32 = 0;
    std::map<std::string, ParamSlot> slots;
    std::vector<std::string> names;

    bf16_t* a16(int64_t n) {
        size_t bytes = ((size_t)n * 2 + 255) & ~(size_t)255;
        char* p = arena16 ? arena16 + used16 : nullptr;
        used16 += bytes;
        return (bf16_t*)p;
    }
    float* a32(int64_t n) {
        size_t bytes = ((size_t)n * 4 + 255) & ~(size_t)255;
        char* p = arena32 ? arena32 + used32 : nullptr;
        used32 += bytes;
        return (float*)p;
    }
    void reg(const std::string& name, void* dst, int dt, int64_t numel) {
        if (!arena16) return;
        slots[name] = ParamSlot{dst, dt, numel, false};
        names.push_back(name);
    }
    // linear: weight [out][in] bf16 at w (row offset allowed by caller), bias fp32
    void lin(const std::string& name, bf16_t* w, float* b, int out_f, int in_f) {
        reg(name + ".weight", w, DT_BF16, (int64_t)out_f * in_f);
        reg(name + ".bias", b, DT_F32, out_f);
    }
    // both arenas at the sizes the sizing pass counted; on failure nothing stays allocated
    int alloc(const char* who) {
        const hipError_t e1 = hipMalloc((void**)&arena16, used16);
        const hipError_t e2 = hipMalloc((void**)&arena32, used32);
        if (e1 == hipSuccess && e2 == hipSuccess) return 0;
        const int r = errorf("%s: hipMalloc of %zu + %zu bytes failed (%s)", who, used16, used32, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        release();
        return r;
    }
    void release() {
        if (arena16) (void)hipFree(arena16);
        if (arena32) (void)hipFree(arena32);
        arena16 = arena32 = nullptr;
    }
    const char* param_name(int i) const { return i < 0 || i >= (int)names.size() ? nullptr : names[i].c_str(); }
    // one parameter from a device tensor of any supported dtype, converted into its arena slot on `stream`
    int bind(const char* who, const char* name, const void* src, int dtype, int ndim, const int64_t* shape, hipStream_t stream) {
        auto it = slots.find(name);
        if (it == slots.end()) return errorf("%s: unknown parameter '%s'", who, name);
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= shape[i];
        if (n != it->second.numel)
            return errorf("%s: '%s' has %lld elements, expected %lld", who, name, (long long)n, (long long)it->second.numel);
        if (dtype < 0 || dtype > 2) return errorf("%s: bad dtype %d", who, dtype);
        HIPCHK(launch_convert(src, dtype, it->second.dst, it->second.dst_dt, n, stream));
        it->second.bound = true;
        return 0;
    }
    int ready() const {
        for (auto& kv : slots)
            if (!kv.second.bound) return errorf("parameter '%s' has not been bound", kv.first.c_str());
        return 0;
    }
};

// weights of one double-stream block (FLUX.1 double blocks, Qwen-Image blocks): image stream, then the text stream's (c...) counterparts
struct DoubleW {
    bf16_t *w_qk, *w_v, *w_o, *w_cqk, *w_cv, *w_co, *w_ff1, *w_ff2, *w_cff1, *w_cff2;
    float *b_qk, *b_v, *b_o, *b_cqk, *b_cv, *b_co, *b_ff1, *b_ff2, *b_cff1, *b_cff2;
    float *nq, *nk, *ncq, *nck;
    int mod_img, mod_ctx;     // first of the six modulation columns of each stream
    float bound = 0.f;        // proven |score| bound of the block's attention (update_score_bounds)
};

// ---- device workspaces ------------------------------------------------------------------------------------------------------------------
// Two-phase allocator of one device workspace: take() names each buffer once, next to its size (256-byte granules, in call order); alloc()
// makes the single hipMalloc and then writes every recorded pointer.  The pointers taken must stay where they are until alloc() has run
// (size a vector of per-block structs before taking into its elements).
struct Carver {
    struct Rec { void* slot; size_t off; };
    std::vector<Rec> recs;
    size_t off = 0;

    template <class T> void take(T*& dst, int64_t elems) {      // (a char* buffer is sized in bytes)
        recs.push_back(Rec{&dst, off});
        off += ((size_t)elems * sizeof(T) + 255) & ~(size_t)255;
    }
    // `zero`: hipMemset of the whole workspace, complete on return.  A failure leaves *base null; the message reads "<who>: hipMalloc of N bytes<what> failed".
    int alloc(char** base, size_t* bytes, bool zero, const char* who, const char* what = "") {
        if (hipMalloc((void**)base, off) != hipSuccess) {
            *base = nullptr;
            return errorf("%s: hipMalloc of %zu bytes%s failed", who, off, what);
        }
        // (hipMemset on device memory may return before the fill has run, and it runs on the NULL stream, which the engines' non-blocking streams do
        //  not wait for -- gemm_tn.hip met exactly that.  The zero padding of these workspaces is a CONTRACT of the attention backward passes
        //  (attention_bwd.hip), so the fill has completed before any pointer is handed out.  Plans and training states are created outside stream
        //  capture: every zeroed workspace belongs to a *_plan_create or to the first training call of a plan, and RolloutGraph captures only the
        //  rollout loop of an existing plan.  So a device synchronise is legal here, and it is paid once per workspace, never per step.)
        if (zero && (hipMemset(*base, 0, off) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) {
            (void)hipFree(*base);
            *base = nullptr;
            return errorf("%s: hipMemset failed", who);
        }
        for (const Rec& r : recs) {
            char* p = *base + r.off;
            memcpy(r.slot, &p, sizeof(p));
        }
        *bytes = off;
        return 0;
    }
};

// ---- captured rollout loop --------------------------------------------------------------------------------------------------------------
inline int float_bits(float f) { int i; memcpy(&i, &f, 4); return i; }

// hipGraph of an engine's whole N-step loop.  The first call of a plan runs eagerly (`warmed`); from then on the loop is one graph launch,
// re-captured whenever the configuration key (everything the captured launches depend on; floats as their bit patterns) changes.
struct RolloutGraph {
    static constexpr int NKEY = 16;
    hipGraphExec_t gexec = nullptr;
    hipStream_t cap_stream = nullptr;   // capture happens on a plan-owned stream: the caller's may be the legacy default stream (torch's
                                        // current stream unless the user switched), which cannot be captured; the graph is LAUNCHED on the caller's
    bool warmed = false;
    int key[NKEY] = {0};

    // `prepare` creates what must exist before the capture (streams, events, side buffers); `body(stream)` issues the loop on plan-owned
    // buffers only.  eager_key = the engine's mi355_tune_set key that selects eager launches (named in the error).
    int launch(const int (&k)[NKEY], hipStream_t st, const char* who, int n_steps, int eager_key, const std::function<int()>& prepare,
               const std::function<int(hipStream_t)>& body) {
        if (!gexec || memcmp(key, k, sizeof(key)) != 0) {
            CHK(prepare());
            if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; }
            hipGraph_t graph = nullptr;
            hipError_t ce = hipSuccess;
            if (!cap_stream) ce = hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking);
            if (ce == hipSuccess) ce = hipStreamBeginCapture(cap_stream, hipStreamCaptureModeRelaxed);
            if (ce == hipSuccess) {
                const int rc = body(cap_stream);                // nothing executes: launches / D2D copies become graph nodes
                ce = hipStreamEndCapture(cap_stream, &graph);
                if (rc != 0 || ce != hipSuccess || !graph) {
                    if (graph) (void)hipGraphDestroy(graph);
                    graph = nullptr;
                }
            }
            if (graph) {
                ce = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
                (void)hipGraphDestroy(graph);
                if (ce != hipSuccess) gexec = nullptr;
            }
            if (!gexec) {
                // no silent fallback (header convention): the caller decides whether to retry with eager launches
                const hipError_t last = hipGetLastError();
                return errorf("%s: hipGraph capture / instantiation of the %d-step loop failed (%s); mi355_tune_set(%d, 0) selects eager launches",
                              who, n_steps, hipGetErrorString(ce != hipSuccess ? ce : last), eager_key);
            }
            memcpy(key, k, sizeof(key));
        }
        HIPCHK(hipGraphLaunch(gexec, st));
        return 0;
    }
    void release() {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        gexec = nullptr;
        cap_stream = nullptr;
    }
};

}  // namespace mi355

// mi355_flow -- training-side helpers shared by the engines' *_train.inc files: the gradient-buffer registry of an engine (all four engines), and,
// for the native backward passes of the head_dim-128 engines (flux_train.inc, qwen_train.inc, wan_train.inc), everything that is not a family's
// own program: the per-engine / per-plan training state and its life cycle, the set_grad family behind the C ABI, the backward scratch and its
// carving, the dgrad / wgrad GEMM wrappers, the backward of a linear layer and of a gated MLP, the attention-backward and q | k producer backward
// sequences, and the backward of a double-stream block (FLUX.1 and Qwen-Image run the same one, told apart by a DoubleBackSched).  A change to the
// text-chain fork / join or to the weight-gradient slot hand-over is made once, here.  (The SD3.5 engine's training file, engine_train.inc,
// predates this header and keeps its own dgrad / wgrad helpers: head_dim 64, per-block dual attention, side-stream scratch pairs.)
#pragma once
#include "engine_common.h"

namespace mi355 {

// Parameter name -> caller-owned gradient buffer (absent = frozen; every backward OVERWRITES the buffers), with the buffers' dtype bookkeeping
// (grad_buf_mark): fp32 when registered -- the *_set_grad_typed functions re-mark a bf16 buffer afterwards -- and un-marked when it leaves.
// Which names an engine accepts is the engine's own rule (its trainable-name predicate and refusal messages).
struct LinGrad { float *w = nullptr, *b = nullptr; };      // the registered gradient buffers of one linear layer (null = frozen)
struct GradRegistry {
    std::map<std::string, float*> grads;
    void set(const std::string& name, float* grad) {       // null un-registers
        auto prev = grads.find(name);
        if (prev != grads.end() && prev->second != grad) grad_buf_mark(prev->second, DT_F32);    // (a re-registration un-marks the buffer it replaces)
        if (!grad) { if (prev != grads.end()) grads.erase(prev); return; }
        grads[name] = grad;
        grad_buf_mark(grad, DT_F32);
    }
    void clear() {
        for (auto& kv : grads) grad_buf_mark(kv.second, DT_F32);
        grads.clear();
    }
    float* find(const std::string& name) const {
        auto it = grads.find(name);
        return it == grads.end() ? nullptr : it->second;
    }
    LinGrad linear(const std::string& layer) const { return LinGrad{find(layer + ".weight"), find(layer + ".bias")}; }
};

// One in-flight weight-gradient group: its operands in contraction-contiguous form (aT: the dY columns, [rows <= aT_rows][M_pad]; xT: the
// layer input, [rows <= xT_rows][M_pad]) + the events that hand it to the side stream and back.
struct WgradSlot {
    bf16_t *aT = nullptr, *xT = nullptr;
    hipEvent_t ready = nullptr, done = nullptr;
    bool busy = false;
};
constexpr int WG_SLOTS = 3;

// backward scratch of one plan (device pointers into the plan's training workspace).  Row counts: M = every token row of the forward batch,
// Mc = its context rows; wide / widec hold [rows][3D + F] (the fused q|k|v|mlp gradient of a single-stream block, or [rows][3D] + [rows][F]).
struct TrainScratch {
    bf16_t *g1, *g1c, *g2, *g2c, *g3, *g3c, *wide, *widec, *hid;
    bf16_t *doh, *v, *dq, *dk, *dvh;          // attention backward: dO head-major, V row-major, dq~ / dk / dv head-major
    float *delta, *nld;
    float *part, *csum, *zero_bias;
    size_t part_floats;
    bf16_t* hid_c = nullptr;                  // the text chain's own gelu(pre) / column-sum scratch when it runs on a second stream
    float* csum_c = nullptr;
    // weight gradients: the operand transposes (+ the bias column sums) run on the backward's own stream, the split-K GEMMs and their
    // reductions on `wside` when it exists (mi355_tune_set(26, .)): they are off the critical path -- nothing in the backward reads a weight
    // gradient -- and their partial last rounds (144 output tiles x 2 splits on 256 CUs) fill with the dgrad chain's kernels and vice versa
    WgradSlot slot[WG_SLOTS];
    int n_slots = 1, next_slot = 0;
    long aT_rows = 0, xT_rows = 0;
    hipStream_t wside = nullptr;
    bool tn_default = false;                  // weight gradients on row-major operands by default (set per engine from measurements: Wan yes, FLUX.1 / Qwen-Image no)
};

struct AttnGeom {
    int B, H, D, S, S_pad;                    // forward batch, heads, H * 128, joint sequence length (padded to 64)
    const float2* cs;                         // rotary table [S][64]
    const int* kv_len;                        // optional device [B]: valid keys per sample (ragged text at the END of the joint sequence)
    int S_kv = 0, S_kv_pad = 0;               // cross-attention: keys / values are another sequence ([B][H][S_kv_pad][128]); 0 = self
};

// out[M][N] (row stride ldo) = A[M][K] (row stride lda) . WT[N][K]^T  (WT = transposed weight: a dgrad), optional fused gelu'(pre)
static inline int t_dgrad(const TrainScratch& t, hipStream_t st, const bf16_t* A, long lda, int K, const bf16_t* WT, int M, int N, bf16_t* out, long ldo,
                          const bf16_t* gelu_pre, long ld_pre) {
    GemmParams g = make_gemm(A, lda, WT, K, M, N, K, gelu_pre ? EPI_DGELU : EPI_BIAS, t.zero_bias, out, ldo);
    if (gelu_pre) { g.aux = gelu_pre; g.ld_aux = ld_pre; }
    HIPCHK(launch_gemm(g, st));
    return 0;
}

// ---- weight gradients -------------------------------------------------------------------------------------------------------------
struct WgradSeg { int col0, N; float* gw; float* gb; };      // dW[N][K] = dY[:, col0 : col0 + N]^T . X (overwritten), db[N] = column sums
struct WgradX { const bf16_t* p; long ld; int K; };          // X = [X0 | X1 ...] column blocks (a single block for every layer but FLUX.1's proj_out)

static inline int t_wgrad_streams_init(TrainScratch& t, bool side) {
    t.n_slots = 1;
    if (!side) return 0;
    HIPCHK(hipStreamCreateWithFlags(&t.wside, hipStreamNonBlocking));
    for (int i = 0; i < WG_SLOTS; ++i) {
        HIPCHK(hipEventCreateWithFlags(&t.slot[i].ready, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&t.slot[i].done, hipEventDisableTiming));
    }
    t.n_slots = WG_SLOTS;
    return 0;
}
static inline void t_wgrad_streams_destroy(TrainScratch& t) {
    for (int i = 0; i < WG_SLOTS; ++i) {
        if (t.slot[i].ready) (void)hipEventDestroy(t.slot[i].ready);
        if (t.slot[i].done) (void)hipEventDestroy(t.slot[i].done);
    }
    if (t.wside) (void)hipStreamDestroy(t.wside);
    t.wside = nullptr;
}
// every gradient written so far is complete on `st` (end of the backward)
static inline int t_wgrad_join(TrainScratch& t, hipStream_t st) {
    for (int i = 0; i < t.n_slots; ++i)
        if (t.slot[i].busy) { HIPCHK(ev_wait(st, t.slot[i].done)); t.slot[i].busy = false; }
    return 0;
}

// ---- training state of an engine and of a plan ------------------------------------------------------------------------------------------
// Both are created on first use, owned through these bases (the engine / plan structs hold `EngineTrain* train` / `PlanTrain* train` and
// `delete` them), and a family derives from them to add only its own members: its per-block transposed-weight and stash pointers.
struct EngineTrain {         // per engine: the transposed weights (dgrad operands; stale after a bind_weight) + the registered gradient buffers
    char* arenaT = nullptr; size_t bytes = 0;
    bf16_t* projT = nullptr;
    bool dirty = true;
    GradRegistry grads;
    virtual ~EngineTrain() { if (arenaT) (void)hipFree(arenaT); }
};
struct PlanTrain {           // per plan: ONE workspace = activation stash of the last training-mode forward + backward scratch
    char* ws = nullptr; size_t ws_bytes = 0;
    bool have_forward = false;
    TrainScratch sc;
    virtual ~PlanTrain() {
        t_wgrad_streams_destroy(sc);
        if (ws) (void)hipFree(ws);
    }
};
template <class S> static inline S* engine_train_state(EngineTrain*& t) {      // S = the family's EngineTrain
    if (!t) t = new S();
    return static_cast<S*>(t);
}
static inline void engine_train_mark_dirty(EngineTrain* t) {
    if (t) t->dirty = true;
}

// The set_grad family of an engine E (a ParamTable with a `train` pointer) whose training state is S: `fam` = the C-ABI prefix for the messages
// ("mi355_flux"), `ok` = the family's trainable-name predicate.
typedef bool (*TrainableName)(const std::string&);
template <class S, class E> static int t_set_grad(E* e, const char* fam, TrainableName ok, const char* name, float* grad) {
    if (!e || !name) return errorf("%s_set_grad: null argument", fam);
    if (e->slots.find(name) == e->slots.end()) return errorf("%s_set_grad: unknown parameter '%s'", fam, name);
    if (grad && !ok(name))
        return errorf("%s_set_grad: '%s' lies outside the native backward's scope (the linear layers inside the transformer blocks)", fam, name);
    engine_train_state<S>(e->train)->grads.set(name, grad);
    return 0;
}
template <class S, class E> static int t_set_grad_typed(E* e, const char* fam, TrainableName ok, const char* name, void* grad, int dtype) {
    if (dtype == DT_F32 || !grad) return t_set_grad<S>(e, fam, ok, name, (float*)grad);
    if (dtype != DT_BF16) return errorf("%s_set_grad_typed: gradient buffers are fp32 or bf16 (dtype %d)", fam, dtype);
    if (!e || !name) return errorf("%s_set_grad_typed: null argument", fam);
    if (!ok(name)) return errorf("%s_set_grad_typed: bf16 gradient buffers are limited to the linear layers inside the transformer blocks ('%s')", fam, name);
    const int rc = t_set_grad<S>(e, fam, ok, name, (float*)grad);
    if (rc == 0) grad_buf_mark(grad, DT_BF16);
    return rc;
}
template <class S, class E> static int t_clear_grads(E* e) {
    if (!e) return errorf("null engine");
    engine_train_state<S>(e->train)->grads.clear();
    return 0;
}
static inline int t_grad_supported(const ParamTable* e, TrainableName ok, const char* name) {
    if (!e || !name || !e->slots.count(name)) return 1;
    return ok(name) ? 0 : 1;
}

// The common tail of a plan's training workspace, after the family's own take() calls: the attention-backward scratch, the weight-gradient
// operand slots, the split-K partials, the column-sum partials and the zero bias; then the allocation and the weight-gradient stream.
struct ScratchSizes {
    int D, F;
    int64_t q_el, kv_el, bhs;     // elements of a head-major q (doh, dq), of a head-major k / v (v, dk, dvh), and B * H * S_pad
    long aT_rows, xT_rows;        // rows of an operand slot: the widest dY group, the widest layer input
    int M_pad;                    // columns of an operand slot: the longest token count a weight gradient contracts over (padded to 64)
    int64_t zero_bias;            // the widest dgrad output
    int Mc;                       // rows of the text chain when it can run on its own stream (its own gelu / column-sum scratch), else 0
};
// A failure deletes `t` (mi355_last_error: the failing call).
static inline int t_train_alloc(Carver& c, PlanTrain* t, const char* who, const ScratchSizes& z) {
    TrainScratch& sc = t->sc;
    const int D = z.D, F = z.F;
    c.take(sc.doh, z.q_el); c.take(sc.v, z.kv_el); c.take(sc.dq, z.q_el); c.take(sc.dk, z.kv_el); c.take(sc.dvh, z.kv_el);
    c.take(sc.delta, z.bhs); c.take(sc.nld, z.bhs * 2);
    const bool side = get_wgrad_side() != 0;
    for (int i = 0; i < (side ? WG_SLOTS : 1); ++i) { c.take(sc.slot[i].aT, (int64_t)z.aT_rows * z.M_pad); c.take(sc.slot[i].xT, (int64_t)z.xT_rows * z.M_pad); }
    sc.part_floats = (size_t)16 * D * D > (size_t)2 * F * D ? (size_t)16 * D * D : (size_t)2 * F * D;
    auto row_tiles = [](int rows_pad) { return (int64_t)(rows_pad / 64 > 64 ? rows_pad / 64 : 64); };
    c.take(sc.part, (int64_t)sc.part_floats); c.take(sc.csum, row_tiles(z.M_pad) * F); c.take(sc.zero_bias, z.zero_bias);
    if (z.Mc > 0) { c.take(sc.hid_c, (int64_t)z.Mc * F); c.take(sc.csum_c, row_tiles((z.Mc + 63) / 64 * 64) * F); }
    sc.aT_rows = z.aT_rows; sc.xT_rows = z.xT_rows;
    if (c.alloc(&t->ws, &t->ws_bytes, true, who, " of activation stash + backward scratch") != 0 || t_wgrad_streams_init(sc, side) != 0) {
        delete t;
        return 1;
    }
    return 0;
}

// One GEMM of a group on stream `ws`: dW = aT[N][M_pad] . xT[K][M_pad]^T, split-K over the token dimension into partial buffers + a fixed-order
// reduction (deterministic; the reduction rounds to bf16 itself for a bf16 gradient buffer)
static inline int t_wgrad_gemm(const TrainScratch& t, hipStream_t ws, const bf16_t* aT, const bf16_t* xT, int N, int K, int M_pad, float* gw) {
    const int split = wgrad_split(N, K, M_pad, t.part_floats, ws == t.wside && t.wside != nullptr);
    GemmParams g = make_gemm(aT, M_pad, xT, M_pad, N, K, M_pad, EPI_F32, nullptr, nullptr, K);
    g.q_scale = 1.0f;
    if (split <= 1 && grad_buf_dtype(gw) == DT_F32) {
        g.out_f32 = gw; g.k_split = 1;
        HIPCHK(launch_gemm(g, ws));
        return 0;
    }
    if ((size_t)N * K > t.part_floats) return errorf("wgrad: a %d x %d gradient does not fit the split-K scratch", N, K);   // (bf16 output, single split)
    g.out_f32 = t.part; g.k_split = split; g.split_stride = (long)N * K;
    HIPCHK(launch_gemm(g, ws));
    HIPCHK(launch_splitk_reduce(t.part, (long)N * K, split, gw, (long)N * K, 0, ws));
    return 0;
}

// The weight (and bias) gradients of the linear layers that share the input X: dY [M][..] holds their output gradients side by side.
// On `st`: X^T once, the dY column blocks transposed (rows zero-padded to M_pad; the bias gradient = the column sums taken on the way).
// On the side stream (or `st`): one split-K GEMM + reduction per layer.  A group larger than a slot's aT is cut (X^T is taken again).
static inline int t_wgrad_group(TrainScratch& t, hipStream_t st, const bf16_t* dY, long ldY, const WgradSeg* seg, int nseg, const WgradX* xs, int nx,
                                int M, int M_pad, bool ctx_chain = false) {
    float* csum = ctx_chain && t.csum_c ? t.csum_c : t.csum;          // (column-sum partials: one scratch per stream that takes them)
    int K = 0;
    for (int i = 0; i < nx; ++i) K += xs[i].K;
    // Round 6: operands as they lie in HBM (csrc/gemm_tn.hip: dY [M][ldY], X [M][ldX] row-major, MFMA fragments through transposed LDS reads;
    // a ragged last m-tile reads zeros) -- neither dY^T nor X^T is made, and the 256 x 256-tile form runs the large weights (N x K >= 160 tiles)
    // at the ping-pong kernel's bytes per FLOP instead of the 2-stage kernel's.  Same products, same split boundaries over M_pad, same fixed-order
    // reduction.  These GEMMs read dY itself, which the backward overwrites next: they run on `st`, not on the side stream that the copies made
    // safe.  Measured per engine (profiles/r06w_*, optimize() step, row-major vs copies): Wan2.1 at 20 280 tokens 1033 vs 1053 ms (its 1536-wide
    // weights need 7-way split-K on the copies' path and its ragged M a padded transpose of 40 560 rows) -- ON; FLUX.1 251 vs 239 ms and Qwen-Image
    // 472 vs 468 ms (3072-wide weights: the 2-stage 256 x 256 kernel beside the dgrad chain on the side stream is the better schedule) -- OFF.
    // mi355_tune_set(39, 2) = row-major wherever it applies, 0 = never, 1 (default) = the engine's measured default.
    if ((get_wgrad_tn_mode() == 2 || (get_wgrad_tn_mode() == 1 && t.tn_default)) && nx == 1 && M_pad % 64 == 0) {
        bool ok = true;
        for (int i = 0; i < nseg && ok; ++i)
            if (seg[i].gw) {
                GemmTnParams tp{dY + seg[i].col0, ldY, xs[0].p, xs[0].ld, M, seg[i].N, K, t.part, (long)K, 1, (long)seg[i].N * K, nullptr, 0};
                tp.M_pad = M_pad;
                ok = gemm_tn_ok(tp) && (size_t)seg[i].N * K <= t.part_floats;
            }
        if (ok) {
            CHK(t_wgrad_join(t, st));                  // earlier side-stream GEMMs may still be reading / writing t.part
            for (int i = 0; i < nseg; ++i) {
                const int N = seg[i].N;
                if (seg[i].gb) HIPCHK(launch_colsum(dY + seg[i].col0, ldY, M, N, csum, seg[i].gb, 0, st));
                if (!seg[i].gw) continue;
                int split = wgrad_split(N, K, M_pad, t.part_floats, false);
                int tile256 = 0;
                if (N % 256 == 0 && K % 256 == 0) {
                    const long t256 = (long)(N / 256) * (K / 256);
                    int s256 = (int)(256 / t256 > 0 ? 256 / t256 : 1);
                    const int cap = (M_pad / 64) / 2 > 0 ? (M_pad / 64) / 2 : 1;
                    if (s256 > cap) s256 = cap;
                    while (s256 > 1 && (size_t)s256 * N * K > t.part_floats) --s256;
                    if (t256 * s256 >= 160) { tile256 = 1; split = s256; }
                }
                if (split < 1) split = 1;
                const bool direct = split == 1 && grad_buf_dtype(seg[i].gw) == DT_F32;
                GemmTnParams tp{dY + seg[i].col0, ldY, xs[0].p, xs[0].ld, M, N, K, direct ? seg[i].gw : t.part, (long)K, split, (long)N * K, nullptr, tile256};
                tp.M_pad = M_pad;
                HIPCHK(launch_gemm_tn(tp, st));
                if (!direct) HIPCHK(launch_splitk_reduce(t.part, (long)N * K, split, seg[i].gw, (long)N * K, 0, st));
            }
            return 0;
        }
    }
    if (K > t.xT_rows) return errorf("wgrad: K = %d exceeds the transposed-input scratch (%ld rows)", K, t.xT_rows);
    int i = 0;
    while (i < nseg) {
        if (!seg[i].gw) {                              // bias only (or nothing): no GEMM
            if (seg[i].gb) HIPCHK(launch_colsum(dY + seg[i].col0, ldY, M, seg[i].N, csum, seg[i].gb, 0, st));
            ++i;
            continue;
        }
        WgradSlot& s = t.slot[t.next_slot];
        t.next_slot = (t.next_slot + 1) % t.n_slots;
        if (s.busy) { HIPCHK(ev_wait(st, s.done)); s.busy = false; }       // the slot's previous GEMMs have read aT / xT
        int r0 = 0;
        for (int x = 0; x < nx; ++x) {
            HIPCHK(launch_transpose(xs[x].p, xs[x].ld, 0, s.xT + (size_t)r0 * M_pad, M_pad, 0, M, xs[x].K, M_pad, 1, st));
            r0 += xs[x].K;
        }
        const int first = i;
        long rows = 0;
        for (; i < nseg && seg[i].gw && rows + seg[i].N <= t.aT_rows; ++i) {
            bf16_t* aT = s.aT + (size_t)rows * M_pad;
            if (seg[i].gb) HIPCHK(launch_transpose_colsum(dY + seg[i].col0, ldY, aT, M_pad, M, seg[i].N, M_pad, csum, seg[i].gb, st));
            else HIPCHK(launch_transpose(dY + seg[i].col0, ldY, 0, aT, M_pad, 0, M, seg[i].N, M_pad, 1, st));
            rows += seg[i].N;
        }
        if (i == first) return errorf("wgrad: N = %d exceeds the transposed-gradient scratch (%ld rows)", seg[i].N, t.aT_rows);
        hipStream_t ws = st;
        if (t.wside) {
            HIPCHK(ev_record(s.ready, st));
            HIPCHK(ev_wait(t.wside, s.ready));
            ws = t.wside;
        }
        rows = 0;
        for (int j = first; j < i; ++j) {
            CHK(t_wgrad_gemm(t, ws, s.aT + (size_t)rows * M_pad, s.xT, seg[j].N, K, M_pad, seg[j].gw));
            rows += seg[j].N;
        }
        if (t.wside) { HIPCHK(ev_record(s.done, t.wside)); s.busy = true; }
    }
    return 0;
}

// single layer
static inline int t_wgrad(TrainScratch& t, hipStream_t st, const bf16_t* dY, long ldY, int col0, int N, const bf16_t* X, long ldX, int K, int M,
                          int M_pad, float* gw, float* gb, bool ctx_chain = false) {
    if (!gw && !gb) return 0;
    const WgradSeg seg{col0, N, gw, gb};
    const WgradX x{X, ldX, K};
    return t_wgrad_group(t, st, dY, ldY, &seg, 1, &x, 1, M, M_pad, ctx_chain);
}

// flash-attention backward of one head_dim-128 attention: o / dO token-major (row stride D), the first n_first positions of a sample in
// (o_first, do_first), the rest in (o_rest, do_rest); a null dO = that part of the output has no consumer.  Results: head-major dq~, dk, dv
// in t.dq / t.dk / t.dvh.
static inline int t_attention128_backward(const TrainScratch& t, const AttnGeom& a, hipStream_t st, const bf16_t* q, const bf16_t* k, const bf16_t* vT,
                                          const float* lse, const bf16_t* o_first, const bf16_t* o_rest, const bf16_t* do_first, const bf16_t* do_rest,
                                          int n_first) {
    Attn128BwdPrepParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.o_first = o_first; pp.ld_o_first = a.D; pp.o_rest = o_rest; pp.ld_o_rest = a.D;
    pp.do_first = do_first; pp.ld_do_first = a.D; pp.do_rest = do_rest; pp.ld_do_rest = a.D; pp.n_first = n_first;
    pp.lse = lse; pp.doh = t.doh; pp.delta = t.delta; pp.nld = t.nld; pp.B = a.B; pp.H = a.H; pp.S = a.S; pp.S_pad = a.S_pad;
    HIPCHK(launch_attn128_bwd_prep(pp, st));
    const int Skp = a.S_kv > 0 ? a.S_kv_pad : a.S_pad;
    const long hs = (long)Skp * 128;
    HIPCHK(launch_transpose(vT, Skp, hs, t.v, 128, hs, 128, Skp, 128, a.B * a.H, st));      // V^T [128][S_pad] -> V [S_pad][128] per (b, h)
    AttnBwdParams ab{q, k, t.v, t.doh, lse, t.delta, t.nld, t.dq, t.dk, t.dvh, a.B, a.H, a.S, a.S_pad, a.kv_len, a.S_kv, a.S_kv_pad};
    HIPCHK(launch_attention128_bwd(ab, st));
    return 0;
}

// backward of the q | k producer (per-head RMSNorm + RoPE) of ONE stream's M rows (rps rows per sample, joint positions s_off ..) + gather of
// (dq~, dk, dv) to token-major [dq_pre | dk_pre | dv] rows (row stride ld_out)
static inline int t_rope_back(const TrainScratch& t, const AttnGeom& a, hipStream_t st, const bf16_t* q, const bf16_t* k, const float* rstd,
                              const float* nq, const float* nk, bf16_t* out, long ld_out, int M, int rps, int s_off) {
    RopeRmsBwdParams r;
    memset(&r, 0, sizeof(r));
    r.q = q; r.k = k; r.dq = t.dq; r.dk = t.dk; r.dv = t.dvh; r.rstd = rstd; r.nw_q = nq; r.nw_k = nk; r.cs = a.cs;
    r.q_scale = 0.08838834764831845f * 1.4426950408889634f;
    r.out = out; r.ld_out = ld_out; r.M = M; r.H = a.H; r.rows_per_sample = rps; r.s_off = s_off; r.S_pad = a.S_pad;
    HIPCHK(launch_rope_rms_bwd128(r, st));
    return 0;
}

// ---- layers of one token stream ----------------------------------------------------------------------------------------------------------
// One stream of token rows in the backward: where its launches go, its rows, and its own scratch ([M][D] g1 / g2 / g3, [M][3D + F] wide,
// [M][F] hid).  `side`: the text chain on its own stream (its weight gradients take their column sums in csum_c).
struct TrainChain {
    hipStream_t st;
    int M, M_pad, rps;                        // rows, padded to 64, rows per sample
    bf16_t *g1, *g2, *g3, *wide, *hid;
    bool side;
};
// the step's modulation rows [B][ld] and the LayerNorm epsilon; head_rows > 0: two rows per sample [2 B][ld], the first head_rows rows of a sample
// read row 2 b, the others row 2 b + 1 (Wan2.2-TI2V image-to-video; no modulation gradients)
struct ModRows { const bf16_t* mod; long ld; float eps; int head_rows = 0; };

// d res (+)= LNmod'(x)(dy): backward of the modulated LayerNorm (shift / scale at columns shift_off / scale_off of the modulation rows)
static inline int t_ln_back(const TrainChain& c, const ModRows& m, int D, const bf16_t* x, const bf16_t* dy, bf16_t* dres, int shift_off, int scale_off,
                            int accumulate) {
    LnModBwdParams l{x, dy, nullptr, dres, m.mod, m.ld, scale_off, 0, c.M, D, c.rps, m.eps, accumulate, nullptr, shift_off, 0, m.head_rows};
    HIPCHK(launch_ln_mod_bwd(l, c.st));
    return 0;
}

// Backward of y = X . W^T + b from dY [M][N]: the weight / bias gradient where one is registered, then dX [M][K] = dY . W on the transposed
// weight WT, with the optional fused gelu'(pre).
static inline int t_linear_back(TrainScratch& t, const TrainChain& c, const bf16_t* dY, long ldY, int N, const bf16_t* X, long ldX, int K,
                                const bf16_t* WT, LinGrad g, bf16_t* dX, long ld_dX, const bf16_t* gelu_pre = nullptr, long ld_pre = 0) {
    CHK(t_wgrad(t, c.st, dY, ldY, 0, N, X, ldX, K, c.M, c.M_pad, g.w, g.b, c.side));
    return t_dgrad(t, c.st, dY, ldY, N, WT, c.M, K, dX, ld_dX, gelu_pre, ld_pre);
}

// Backward of the gated MLP x' = x + gate * W2 . gelu(W1 . LNmod(x)) of one stream: dres = d x' on entry, d x on return.  m0 = the first of the
// block's six modulation columns [shift | scale | gate] x (attention, MLP); stash: x_mid = x, xn = LNmod(x), pre = W1 . xn; w1T / w2T transposed.
// gelu(pre), the input of W2, is recomputed into c.hid only when W2's weight gradient is wanted.
static inline int t_mlp_back(TrainScratch& t, const TrainChain& c, const ModRows& m, int m0, int D, int F, bf16_t* dres, const bf16_t* x_mid,
                             const bf16_t* xn, const bf16_t* pre, const bf16_t* w1T, const bf16_t* w2T, LinGrad g1, LinGrad g2) {
    bf16_t* dpre = c.wide + (size_t)c.M * 3 * D;          // [M][F] behind the [M][3D] q|k|v gradient
    HIPCHK(launch_gate_mul(dres, m.mod + m0 + 5 * D, m.ld, c.g1, c.M, D, c.rps, c.st, m.head_rows));
    if (g2.w) HIPCHK(launch_gelu_fwd(pre, c.hid, (long)c.M * F, c.st));
    CHK(t_linear_back(t, c, c.g1, D, D, c.hid, F, F, w2T, g2, dpre, F, pre, F));
    CHK(t_linear_back(t, c, dpre, F, F, xn, D, D, w1T, g1, c.g3, D));
    return t_ln_back(c, m, D, x_mid, c.g3, dres, m0 + 3 * D, m0 + 4 * D, 1);
}

// ---- double-stream block (FLUX.1 double blocks, Qwen-Image blocks) ---------------------------------------------------------------------------
// per-block activation stash of the training-mode forward (the family's forward_core fills it): what the backward of the block needs
struct DoubleStash {
    bf16_t *x_in, *xn, *x_mid, *xn_mlp, *pre, *o_img;
    bf16_t *c_in, *cn, *c_mid, *cn_mlp, *cpre, *o_ctx;
    bf16_t *q, *k, *vT;
    float *lse, *rstd_img, *rstd_ctx;
};
struct DoubleWT { bf16_t *qkv, *o, *cqkv, *co, *ff1, *ff2, *cff1, *cff2; };   // transposed weights (dgrad operands)
struct DoubleGrads { LinGrad q, k, v, o, cq, ck, cv, co, ff1, ff2, cff1, cff2; };

// What tells the two families apart: the order of the joint sequence and the names of the two MLPs (the attention names are shared).
struct DoubleBackSched {
    bool image_first;                 // image rows first in the joint sequence (Qwen-Image) or context rows first (FLUX.1)
    const char *mlp_img, *mlp_ctx;    // parameter-name leaves of the image / text MLP
    bool last_text_dead;              // the text output of the LAST block has no consumer (Qwen-Image; FLUX.1's feeds the single-stream blocks)
};

static inline void t_double_stash_take(Carver& c, DoubleStash& k, int Mi, int Mc, int D, int F, int H, int64_t qk_el, int64_t bhs) {
    c.take(k.x_in, (int64_t)Mi * D); c.take(k.xn, (int64_t)Mi * D); c.take(k.x_mid, (int64_t)Mi * D); c.take(k.xn_mlp, (int64_t)Mi * D);
    c.take(k.pre, (int64_t)Mi * F); c.take(k.o_img, (int64_t)Mi * D);
    c.take(k.c_in, (int64_t)Mc * D); c.take(k.cn, (int64_t)Mc * D); c.take(k.c_mid, (int64_t)Mc * D); c.take(k.cn_mlp, (int64_t)Mc * D);
    c.take(k.cpre, (int64_t)Mc * F); c.take(k.o_ctx, (int64_t)Mc * D);
    c.take(k.q, qk_el); c.take(k.k, qk_el); c.take(k.vT, qk_el);
    c.take(k.lse, bhs); c.take(k.rstd_img, (int64_t)Mi * 2 * H); c.take(k.rstd_ctx, (int64_t)Mc * 2 * H);
}
static inline void t_double_wt_take(Carver& c, DoubleWT& w, int D, int F) {
    c.take(w.qkv, (int64_t)D * 3 * D); c.take(w.o, (int64_t)D * D); c.take(w.cqkv, (int64_t)D * 3 * D); c.take(w.co, (int64_t)D * D);
    c.take(w.ff1, (int64_t)D * F); c.take(w.ff2, (int64_t)F * D); c.take(w.cff1, (int64_t)D * F); c.take(w.cff2, (int64_t)F * D);
}
// W [rows][cols] -> out[c][col0 + r] with row stride ld_out
static inline hipError_t t_transpose_weight(const bf16_t* w, int rows, int cols, bf16_t* out, long ld_out, int col0, hipStream_t st) {
    return launch_transpose(w, cols, 0, out + col0, ld_out, 0, rows, cols, rows, 1, st);
}
static inline int t_double_wt_fill(const DoubleW& b, DoubleWT& w, int D, int F, hipStream_t st) {
    HIPCHK(t_transpose_weight(b.w_qk, 2 * D, D, w.qkv, 3 * D, 0, st)); HIPCHK(t_transpose_weight(b.w_v, D, D, w.qkv, 3 * D, 2 * D, st));
    HIPCHK(t_transpose_weight(b.w_o, D, D, w.o, D, 0, st));
    HIPCHK(t_transpose_weight(b.w_cqk, 2 * D, D, w.cqkv, 3 * D, 0, st)); HIPCHK(t_transpose_weight(b.w_cv, D, D, w.cqkv, 3 * D, 2 * D, st));
    HIPCHK(t_transpose_weight(b.w_co, D, D, w.co, D, 0, st));
    HIPCHK(t_transpose_weight(b.w_ff1, F, D, w.ff1, F, 0, st)); HIPCHK(t_transpose_weight(b.w_ff2, D, F, w.ff2, D, 0, st));
    HIPCHK(t_transpose_weight(b.w_cff1, F, D, w.cff1, F, 0, st)); HIPCHK(t_transpose_weight(b.w_cff2, D, F, w.cff2, D, 0, st));
    return 0;
}
static inline DoubleGrads t_double_grads(const GradRegistry& r, const DoubleBackSched& d, int i) {
    const std::string blk = "transformer_blocks." + std::to_string(i);
    auto L = [&](const std::string& leaf) { return r.linear(blk + leaf); };
    return DoubleGrads{L(".attn.to_q"), L(".attn.to_k"), L(".attn.to_v"), L(".attn.to_out.0"), L(".attn.add_q_proj"), L(".attn.add_k_proj"),
                       L(".attn.add_v_proj"), L(".attn.to_add_out"), L(std::string(d.mlp_img) + ".net.0.proj"), L(std::string(d.mlp_img) + ".net.2"),
                       L(std::string(d.mlp_ctx) + ".net.0.proj"), L(std::string(d.mlp_ctx) + ".net.2")};
}

// Backward of one double-stream block: dx / dc = the gradient of the block's image / text output on entry, of its inputs on return.  The image
// chain `im` runs on the backward's stream; the text chain `tx` on the same one, or (tx.side) on the plan's side stream: it joins before the
// joint attention backward, which reads the text rows' dO (and whose predecessor's text chain has read dq / dk / dv), and forks after it, when
// dq / dk / dv are written.  Scratch is per chain; the weight-gradient operand slots are shared through their events.  Same kernels and
// operands either way: bit-identical.
// `dead_text`: the block's text output has no consumer.  Its text MLP and text out-projection are skipped, the text rows' dO is null, and d c
// STARTS at this block's attention.  (Frozen by construction: the gradient of an unused output is exactly zero; registered buffers are still
// overwritten.)
static inline int t_double_block_back(TrainScratch& t, const DoubleBackSched& d, const AttnGeom& a, int F, const ModRows& m, const DoubleW& b,
                                      const DoubleStash& k, const DoubleWT& w, const DoubleGrads& g, const TrainChain& im, const TrainChain& tx,
                                      bf16_t* dx, bf16_t* dc, bool dead_text, hipEvent_t ev_join, hipEvent_t ev_fork) {
    const int D = a.D, mi = b.mod_img, mc = b.mod_ctx;
    const bool two = tx.side;
    // ---- MLP of both streams
    CHK(t_mlp_back(t, im, m, mi, D, F, dx, k.x_mid, k.xn_mlp, k.pre, w.ff1, w.ff2, g.ff1, g.ff2));
    if (!dead_text) CHK(t_mlp_back(t, tx, m, mc, D, F, dc, k.c_mid, k.cn_mlp, k.cpre, w.cff1, w.cff2, g.cff1, g.cff2));
    // ---- joint attention: out-projections of both streams
    HIPCHK(launch_gate_mul(dx, m.mod + mi + 2 * D, m.ld, im.g1, im.M, D, im.rps, im.st));
    CHK(t_linear_back(t, im, im.g1, D, D, k.o_img, D, D, w.o, g.o, im.g2, D));
    if (!dead_text) {
        HIPCHK(launch_gate_mul(dc, m.mod + mc + 2 * D, m.ld, tx.g1, tx.M, D, tx.rps, tx.st));
        CHK(t_linear_back(t, tx, tx.g1, D, D, k.o_ctx, D, D, w.co, g.co, tx.g2, D));
        if (two) { HIPCHK(ev_record(ev_join, tx.st)); HIPCHK(ev_wait(im.st, ev_join)); }
    } else {
        const struct { float* p; size_t n; } zero[6] = {{g.co.w, (size_t)D * D}, {g.co.b, (size_t)D}, {g.cff1.w, (size_t)F * D}, {g.cff1.b, (size_t)F},
                                                        {g.cff2.w, (size_t)D * F}, {g.cff2.b, (size_t)D}};
        for (const auto& z : zero)
            if (z.p) HIPCHK(hipMemsetAsync(z.p, 0, z.n * grad_buf_esize(z.p), im.st));
    }
    const bf16_t* do_ctx = dead_text ? nullptr : tx.g2;
    if (d.image_first) CHK(t_attention128_backward(t, a, im.st, k.q, k.k, k.vT, k.lse, k.o_img, k.o_ctx, im.g2, do_ctx, im.rps));
    else CHK(t_attention128_backward(t, a, im.st, k.q, k.k, k.vT, k.lse, k.o_ctx, k.o_img, do_ctx, im.g2, tx.rps));
    if (two) { HIPCHK(ev_record(ev_fork, im.st)); HIPCHK(ev_wait(tx.st, ev_fork)); }
    // ---- q | k | v producers of both streams, in the order of the joint sequence
    auto rope_img = [&](int s_off) { return t_rope_back(t, a, im.st, k.q, k.k, k.rstd_img, b.nq, b.nk, im.wide, 3 * D, im.M, im.rps, s_off); };
    auto rope_ctx = [&](int s_off) { return t_rope_back(t, a, tx.st, k.q, k.k, k.rstd_ctx, b.ncq, b.nck, tx.wide, 3 * D, tx.M, tx.rps, s_off); };
    if (d.image_first) { CHK(rope_img(0)); CHK(rope_ctx(im.rps)); }
    else { CHK(rope_ctx(0)); CHK(rope_img(tx.rps)); }
    const WgradSeg si[3] = {{0, D, g.q.w, g.q.b}, {D, D, g.k.w, g.k.b}, {2 * D, D, g.v.w, g.v.b}};
    const WgradSeg sx[3] = {{0, D, g.cq.w, g.cq.b}, {D, D, g.ck.w, g.ck.b}, {2 * D, D, g.cv.w, g.cv.b}};
    const WgradX xi{k.xn, D, D}, xc{k.cn, D, D};
    CHK(t_wgrad_group(t, im.st, im.wide, 3 * D, si, 3, &xi, 1, im.M, im.M_pad));
    CHK(t_wgrad_group(t, tx.st, tx.wide, 3 * D, sx, 3, &xc, 1, tx.M, tx.M_pad, tx.side));
    CHK(t_dgrad(t, im.st, im.wide, 3 * D, 3 * D, w.qkv, im.M, D, im.g3, D, nullptr, 0));
    CHK(t_dgrad(t, tx.st, tx.wide, 3 * D, 3 * D, w.cqkv, tx.M, D, tx.g3, D, nullptr, 0));
    CHK(t_ln_back(im, m, D, k.x_in, im.g3, dx, mi, mi + D, 1));
    return t_ln_back(tx, m, D, k.c_in, tx.g3, dc, mc, mc + D, dead_text ? 0 : 1);
}

// The L double-stream blocks of an engine, last to first.  ev_join / ev_fork: the plan's per-block events of the text chain, [L] = start / end
// (read only when the text chain has its own stream).
static inline int t_double_blocks_back(TrainScratch& t, const DoubleBackSched& d, const AttnGeom& a, int F, const ModRows& m, int L, const DoubleW* b,
                                       const DoubleStash* k, const DoubleWT* w, const GradRegistry& r, const TrainChain& im, const TrainChain& tx,
                                       bf16_t* dx, bf16_t* dc, const hipEvent_t* ev_join, const hipEvent_t* ev_fork) {
    const bool two = tx.side;
    if (two) {          // d x / d c, the stash and the transposed weights are complete on the backward's stream
        HIPCHK(ev_record(ev_fork[L], im.st));
        HIPCHK(ev_wait(tx.st, ev_fork[L]));
    }
    for (int i = L - 1; i >= 0; --i)
        CHK(t_double_block_back(t, d, a, F, m, b[i], k[i], w[i], t_double_grads(r, d, i), im, tx, dx, dc, d.last_text_dead && i + 1 == L,
                                two ? ev_join[i] : nullptr, two ? ev_fork[i] : nullptr));
    if (two) {          // the backward's stream goes on only after the text chain
        HIPCHK(ev_record(ev_join[L], tx.st));
        HIPCHK(ev_wait(im.st, ev_join[L]));
    }
    return 0;
}

}  // namespace mi355

// mi355_flow -- differentiable denoise step for the `optimize()` replay (SURVEY.md 8(f) N1; reference
// src/flow_factory/trainers/grpo.py:185-342: forward-with-grad on stored (x_i, x_{i+1}), replay log-prob, backward).
// Textually included at the end of engine.hip (shares its engine / plan structs and launch helpers).
//
//   mi355_denoise_step_train    : mi355_denoise_step on engine.hip's forward_core with the plan's training stash (see there);
//   mi355_denoise_step_backward : d loss / d weights from the upstream gradients of (log_prob, noise_pred, next_latents_mean).
//
// Scope of the weight gradients.  DEFAULT scope: the linear layers of the transformer blocks -- attn.{to_q,to_k,to_v,to_out.0,add_q_proj,
// add_k_proj,add_v_proj,to_add_out}, attn2.{to_q,to_k,to_v,to_out.0}, ff.net.{0.proj,2}, ff_context.net.{0.proj,2} (weights and biases): the
// reference's default target modules for full fine-tuning and LoRA (models/abc.py:382-385) and every superset of them inside the blocks.
// FULL scope (mi355_engine_set_train_scope(e, 1) before the forward; `target_modules: all`): additionally every AdaLN modulation linear
// (norm1 / norm1_context / norm_out .linear), the q/k RMSNorm weights, the timestep / pooled-text MLPs, context_embedder, the patch embedding
// and proj_out -- i.e. every parameter of the transformer (pos_embed.pos_embed is a buffer).  The forward then also stashes the un-gated
// projections (d gate needs them) and the backward adds: per-sample token sums of d shift / d scale / d gate (fp32 atomics, the only
// non-bit-reproducible gradients), the 50 modulation wgrads (M = batch), the conditioning MLPs' backward, norm-weight partial sums.
// The data gradient runs through the whole network in both scopes.
//
// Backward of one block, image stream (context stream alike), all activations / gradients bf16 with fp32 accumulation:
//   dy   = gate * dx                                   gate_mul_kernel
//   dpre = (dy . W_ff2) * gelu'(pre)                   dgrad GEMM on the transposed weight, EPI_DGELU
//   dxn  = dpre . W_ff1                                dgrad GEMM
//   dx  += LNmod'(x_mid)(dxn)                          ln_mod_bwd_kernel
//   do   = (gate * dx) . W_o                           gate_mul + dgrad GEMM
//   (dq~, dk, dv) = attention'(q~, k, v, o, do, L)     attn_bwd_prep + 3 transposes + attention_bwd (2 passes)
//   d[q|k|v]_pre  = RMSNorm'(dq~, dk) | dv             rms_bwd_gather_kernel -> token-major [M][3D]
//   dxn  = d[q|k|v]_pre . [W_q; W_k; W_v]              ONE dgrad GEMM (K = 3D) on the transposed, concatenated weight
//   dx  += LNmod'(x_in)(dxn [, dxn2 of the dual attention])
//   dW   = dY^T . X  (fp32)                            transposes to contraction-contiguous operands + split-K GEMM (EPI_F32) + fixed-order
//                                                      reduction; db = column sums
// dgrad GEMMs reuse the forward kernels (C = A . W'^T with W' = W^T kept in a second weight arena, refreshed after every re-bind).

struct TrainWT {   // transposed weights of one block (dgrad operands)
    bf16_t *qkv, *o, *cqkv, *co, *qkv2, *o2, *ff1, *ff2, *cff1, *cff2;
};
struct GradSlot { float* g = nullptr; };

struct TrainEngineState {
    char* arenaT = nullptr; size_t bytes = 0;
    std::vector<TrainWT> wt;
    bf16_t* proj = nullptr;
    bf16_t* wmodT = nullptr;            // [D][mod_cols]: transposed modulation weights (only when the conditioning MLPs are trainable)
    bool wmod_dirty = true;
    bool full = false;                  // mi355_engine_set_train_scope
    bool dirty = true;
    GradRegistry grads;                 // parameter name -> gradient buffer (caller-owned), absent = frozen
};

static void train_mark_dirty(mi355_engine* e) {
    if (e->train) { e->train->dirty = true; e->train->wmod_dirty = true; }
}
static TrainEngineState* train_state(mi355_engine* e) {      // created on first use
    if (!e->train) e->train = new TrainEngineState();
    return e->train;
}

static bool trainable_name(const std::string& n) {
    static const char* ok[] = {".attn.to_q.", ".attn.to_k.", ".attn.to_v.", ".attn.to_out.0.", ".attn.add_q_proj.", ".attn.add_k_proj.",
                               ".attn.add_v_proj.", ".attn.to_add_out.", ".attn2.to_q.", ".attn2.to_k.", ".attn2.to_v.", ".attn2.to_out.0.",
                               ".ff.net.0.proj.", ".ff.net.2.", ".ff_context.net.0.proj.", ".ff_context.net.2."};
    if (n.rfind("transformer_blocks.", 0) != 0) return false;
    for (const char* k : ok)
        if (n.find(k) != std::string::npos) return true;
    return false;
}

extern "C" int mi355_engine_set_grad(mi355_engine* e, const char* name, float* grad) {
    if (!e || !name) return errorf("mi355_engine_set_grad: null argument");
    if (e->slots.find(name) == e->slots.end()) return errorf("mi355_engine_set_grad: unknown parameter '%s'", name);
    TrainEngineState* s = train_state(e);
    if (grad && !strcmp(name, "pos_embed.pos_embed")) return errorf("mi355_engine_set_grad: pos_embed.pos_embed is a buffer, not a trainable parameter");
    if (grad && !trainable_name(name) && !s->full)
        return errorf("mi355_engine_set_grad: '%s' lies outside the transformer blocks' linear layers: select the full scope with "
                      "mi355_engine_set_train_scope(engine, 1) BEFORE the training-mode forward", name);
    s->grads.set(name, grad);
    return 0;
}
// the same with the buffer's dtype: MI355_F32, or MI355_BF16 for the weights / biases of the linear layers inside the transformer blocks (the
// kernels that finish those gradients round their fp32 sums to bf16 on the way out: the values of `fp32 buffer -> bf16`, minus the round trip)
extern "C" int mi355_engine_set_grad_typed(mi355_engine* e, const char* name, void* grad, int dtype) {
    if (dtype == DT_F32 || !grad) return mi355_engine_set_grad(e, name, (float*)grad);
    if (dtype != DT_BF16) return errorf("mi355_engine_set_grad_typed: gradient buffers are fp32 or bf16 (dtype %d)", dtype);
    if (!e || !name) return errorf("mi355_engine_set_grad_typed: null argument");
    if (!trainable_name(name)) return errorf("mi355_engine_set_grad_typed: bf16 gradient buffers are limited to the linear layers inside the transformer blocks ('%s')", name);
    const int rc = mi355_engine_set_grad(e, name, (float*)grad);
    if (rc == 0) grad_buf_mark(grad, DT_BF16);
    return rc;
}
// 0: gradients of the blocks' linear layers only (default); 1: of every parameter (the next training-mode forward stashes more)
extern "C" int mi355_engine_set_train_scope(mi355_engine* e, int full) {
    if (!e) return errorf("null engine");
    train_state(e)->full = full != 0;
    return 0;
}
extern "C" int mi355_engine_clear_grads(mi355_engine* e) {
    if (!e) return errorf("null engine");
    train_state(e)->grads.clear();
    return 0;
}
// 0 = a gradient for `name` can be produced in the default scope, 2 = only in the full scope, 1 = never
extern "C" int mi355_engine_grad_supported(mi355_engine* e, const char* name) {
    if (!e || !name || !e->slots.count(name) || !strcmp(name, "pos_embed.pos_embed")) return 1;
    return trainable_name(name) ? 0 : 2;
}

static float* grad_of(mi355_engine* e, const std::string& name) { return train_state(e)->grads.find(name); }

// ---- transposed weights -------------------------------------------------------------------------------------------
static int ensure_transposed_weights(mi355_engine* e, hipStream_t st) {
    TrainEngineState* s = train_state(e);
    const int D = e->D, F = e->F, L = e->L;
    const int NO = e->cfg.patch_size * e->cfg.patch_size * e->cfg.out_channels;
    if (!s->arenaT) {
        Carver c;
        s->wt.resize(L);
        for (int i = 0; i < L; ++i) {
            const BlockW& b = e->blk[i];
            TrainWT& w = s->wt[i];
            c.take(w.qkv, (int64_t)D * 3 * D); c.take(w.o, (int64_t)D * D);
            c.take(w.cqkv, (int64_t)D * 3 * D); if (!b.last) c.take(w.co, (int64_t)D * D);
            if (b.dual) { c.take(w.qkv2, (int64_t)D * 3 * D); c.take(w.o2, (int64_t)D * D); }
            c.take(w.ff1, (int64_t)D * F); c.take(w.ff2, (int64_t)F * D);
            if (!b.last) { c.take(w.cff1, (int64_t)D * F); c.take(w.cff2, (int64_t)F * D); }
        }
        c.take(s->proj, (int64_t)D * NO);
        CHK(c.alloc(&s->arenaT, &s->bytes, false, "training", " for the transposed weights"));
        s->dirty = true;
    }
    if (!s->dirty) return 0;
    // W [rows][cols] -> out[c][col0 + r] with row stride ld_out
    auto tr = [&](const bf16_t* w, int rows, int cols, bf16_t* out, long ld_out, int col0) {
        return launch_transpose(w, cols, 0, out + col0, ld_out, 0, rows, cols, rows, 1, st);
    };
    for (int i = 0; i < L; ++i) {
        const BlockW& b = e->blk[i];
        TrainWT& w = s->wt[i];
        HIPCHK(tr(b.w_qk, 2 * D, D, w.qkv, 3 * D, 0)); HIPCHK(tr(b.w_v, D, D, w.qkv, 3 * D, 2 * D));
        HIPCHK(tr(b.w_o, D, D, w.o, D, 0));
        HIPCHK(tr(b.w_cqk, 2 * D, D, w.cqkv, 3 * D, 0)); HIPCHK(tr(b.w_cv, D, D, w.cqkv, 3 * D, 2 * D));
        if (!b.last) HIPCHK(tr(b.w_co, D, D, w.co, D, 0));
        if (b.dual) {
            HIPCHK(tr(b.w_qk2, 2 * D, D, w.qkv2, 3 * D, 0)); HIPCHK(tr(b.w_v2, D, D, w.qkv2, 3 * D, 2 * D));
            HIPCHK(tr(b.w_o2, D, D, w.o2, D, 0));
        }
        HIPCHK(tr(b.w_ff1, F, D, w.ff1, F, 0));      // [F][D] -> [D][F]
        HIPCHK(tr(b.w_ff2, D, F, w.ff2, D, 0));      // [D][F] -> [F][D]
        if (!b.last) { HIPCHK(tr(b.w_cff1, F, D, w.cff1, F, 0)); HIPCHK(tr(b.w_cff2, D, F, w.cff2, D, 0)); }
    }
    HIPCHK(tr(e->w_proj, NO, D, s->proj, NO, 0));    // [NO][D] -> [D][NO]
    s->dirty = false;
    return 0;
}

// ---- training workspace ----------------------------------------------------------------------------------------------
static int train_of(mi355_plan* p, mi355_train** out) {
    if (p->train) { *out = p->train; return 0; }
    mi355_engine* e = p->e;
    const int D = e->D, F = e->F, L = e->L, H = e->cfg.num_heads;
    const int Mi = p->Mi, Mc = p->Mc, Ni = p->Ni;
    const int Ni_pad = (Ni + 63) / 64 * 64;
    const int64_t qk_el = (int64_t)p->Bp * H * p->S_pad * 64, qk2_el = (int64_t)p->Bp * H * Ni_pad * 64;
    mi355_train* t = new mi355_train();
    t->p = p;
    t->Mi_pad = (Mi + 63) / 64 * 64; t->Mc_pad = (Mc + 63) / 64 * 64;
    const int Mmax_pad = t->Mi_pad > t->Mc_pad ? t->Mi_pad : t->Mc_pad;
    Carver c;
    t->blk.resize(L);
    for (int i = 0; i < L; ++i) {      // (a block without a dual attention / the last block's context stream has no such buffers: they stay null)
        const BlockW& b = e->blk[i];
        TrainBlk& k = t->blk[i];
        c.take(k.x_in, (int64_t)Mi * D); c.take(k.xn, (int64_t)Mi * D); if (b.dual) c.take(k.xn2, (int64_t)Mi * D);
        c.take(k.x_mid, (int64_t)Mi * D); c.take(k.xn_mlp, (int64_t)Mi * D); c.take(k.pre, (int64_t)Mi * F);
        c.take(k.o_img, (int64_t)Mi * D); if (b.dual) c.take(k.o2, (int64_t)Mi * D);
        c.take(k.c_in, (int64_t)Mc * D); c.take(k.cn, (int64_t)Mc * D);
        if (!b.last) { c.take(k.c_mid, (int64_t)Mc * D); c.take(k.cn_mlp, (int64_t)Mc * D); c.take(k.cpre, (int64_t)Mc * F); }
        c.take(k.o_ctx, (int64_t)Mc * D);
        c.take(k.q, qk_el); c.take(k.k, qk_el); c.take(k.vT, qk_el);
        if (b.dual) { c.take(k.q2, qk2_el); c.take(k.k2, qk2_el); c.take(k.vT2, qk2_el); }
        c.take(k.lse, (int64_t)p->Bp * H * p->S_pad); if (b.dual) c.take(k.lse2, (int64_t)p->Bp * H * Ni_pad);
        c.take(k.rstd_img, (int64_t)Mi * 2 * H); c.take(k.rstd_ctx, (int64_t)Mc * 2 * H); if (b.dual) c.take(k.rstd2, (int64_t)Mi * 2 * H);
    }
    c.take(t->x_final, (int64_t)Mi * D);
    c.take(t->mod, (int64_t)p->Bp * e->mod_cols); c.take(t->vnet, (int64_t)p->Bp * p->n_lat);
    c.take(t->dx, (int64_t)Mi * D); c.take(t->dc, (int64_t)Mc * D); c.take(t->dy, (int64_t)Mi * D); c.take(t->dyc, (int64_t)Mc * D);
    c.take(t->dpre, (int64_t)Mi * F); c.take(t->hid, (int64_t)Mi * F); c.take(t->dpre_c, (int64_t)Mc * F);
    c.take(t->dxn, (int64_t)Mi * D); c.take(t->dxn2, (int64_t)Mi * D); c.take(t->dcn, (int64_t)Mc * D);
    c.take(t->do_img, (int64_t)Mi * D); c.take(t->do_ctx, (int64_t)Mc * D);
    c.take(t->doh, qk_el); c.take(t->v, qk_el); c.take(t->nld, (int64_t)p->Bp * H * p->S_pad * 2);
    c.take(t->dq, qk_el); c.take(t->dk, qk_el); c.take(t->dv, qk_el);
    c.take(t->dqkv_img, (int64_t)Mi * 3 * D); c.take(t->dqkv_ctx, (int64_t)Mc * 3 * D);
    c.take(t->aT, (int64_t)F * Mmax_pad); c.take(t->xT, (int64_t)F * Mmax_pad);
    c.take(t->aT_c, (int64_t)F * t->Mc_pad); c.take(t->xT_c, (int64_t)F * t->Mc_pad); c.take(t->hid_c, (int64_t)Mc * F);
    c.take(t->dproj, (int64_t)Mi * 64);
    c.take(t->delta, (int64_t)p->Bp * H * p->S_pad); c.take(t->dv32, (int64_t)p->Bp * p->n_lat);
    t->part_floats = (size_t)16 * D * D > (size_t)2 * F * D ? (size_t)16 * D * D : (size_t)2 * F * D;
    c.take(t->part, (int64_t)t->part_floats); c.take(t->csum, (int64_t)(Mmax_pad / 64 > 64 ? Mmax_pad / 64 : 64) * F); c.take(t->zero_bias, F > 3 * D ? F : 3 * D);
    c.take(t->part_c, (int64_t)t->part_floats); c.take(t->csum_c, (int64_t)(t->Mc_pad / 64 > 64 ? t->Mc_pad / 64 : 64) * F);
    if (c.alloc(&t->ws, &t->ws_bytes, true, "training", " of activation stash + backward scratch") != 0) { delete t; return 1; }
    p->train = t;
    *out = t;
    return 0;
}

static int train_full_of(mi355_train* t) {
    if (t->wsf) return 0;
    mi355_plan* p = t->p;
    mi355_engine* e = p->e;
    const int D = e->D, L = e->L, T = e->cfg.time_proj_dim, P = e->cfg.pooled_projection_dim, J = e->cfg.joint_attention_dim;
    const int Mi = p->Mi, Mc = p->Mc, Bp = p->Bp;
    Carver c;
    t->fblk.resize(L);
    for (int i = 0; i < L; ++i) {
        const BlockW& b = e->blk[i];
        TrainBlkFull& f = t->fblk[i];
        c.take(f.y_o, (int64_t)Mi * D); if (b.dual) c.take(f.y_o2, (int64_t)Mi * D); c.take(f.y_ff, (int64_t)Mi * D);
        if (!b.last) { c.take(f.y_co, (int64_t)Mc * D); c.take(f.y_cff, (int64_t)Mc * D); }
    }
    const int maxw = D > T ? (D > P ? D : P) : (T > P ? T : P);
    c.take(t->xn_out, (int64_t)Mi * D); c.take(t->patches, (int64_t)Mi * e->KP); c.take(t->enc, (int64_t)Mc * J); c.take(t->pool, (int64_t)Bp * P);
    c.take(t->tproj, (int64_t)Bp * T); c.take(t->h1, (int64_t)Bp * D); c.take(t->p1, (int64_t)Bp * D); c.take(t->pemb, (int64_t)Bp * D);
    c.take(t->semb, (int64_t)Bp * D); c.take(t->dmod16, (int64_t)64 * e->mod_cols);
    c.take(t->temb, (int64_t)64 * D); c.take(t->dtemb, (int64_t)64 * D); c.take(t->dh1, (int64_t)64 * D); c.take(t->pre1, (int64_t)64 * D);
    c.take(t->dsemb, (int64_t)64 * D); c.take(t->wT_small, (int64_t)D * maxw);
    c.take(t->dmod, (int64_t)Bp * e->mod_cols); c.take(t->dw_part, (int64_t)rms_bwd_grid(Bp, p->S) * 4 * 64);
    CHK(c.alloc(&t->wsf, &t->wsf_bytes, true, "training (full scope)"));
    return 0;
}

static void train_release(mi355_plan* p) {
    mi355_train* t = p->train;
    if (!t) return;
    if (t->wsf) (void)hipFree(t->wsf);
    if (t->ws) (void)hipFree(t->ws);
    for (hipEvent_t ev : t->ev) (void)hipEventDestroy(ev);
    if (t->side) (void)hipStreamDestroy(t->side);
    delete t;
    p->train = nullptr;
}
static void train_release_engine(mi355_engine* e) {
    if (!e->train) return;
    if (e->train->arenaT) (void)hipFree(e->train->arenaT);
    if (e->train->wmodT) (void)hipFree(e->train->wmodT);
    delete e->train;
    e->train = nullptr;
}
extern "C" int64_t mi355_plan_training_bytes(mi355_plan* p) {
    return p && p->train ? (int64_t)(p->train->ws_bytes + p->train->wsf_bytes) : 0;
}

// ---- training-mode forward: forward_core (engine.hip) on the per-block stash ------------------------------------------------------------
// key 22: the context-stream chain of the training forward and of the backward on a side stream (1 = default).  Its GEMMs have 666 rows at
// B = 2 (72 workgroups of 128 x 128 on 256 CUs, 45-58 us each, ~10 ms of a 112 ms optimize() step when run in line); beside the image
// stream's launches they cost nothing.  Same kernels and operands either way: the results are bit-identical.
// (static int g_train_two_stream: defined in engine.hip beside the other tunables)
static int train_side_init(mi355_train* t) {
    if (t->side) return 0;
    // failure-atomic: the stream and ALL events are built in locals and published together -- a half-built state (stream set, events short)
    // would send every later forward / backward through `if (t->side) return 0` and index t->ev out of bounds
    const size_t n = 2 * ((size_t)t->p->e->L + 1);
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev;
    hipError_t err = hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
    for (size_t i = 0; err == hipSuccess && i < n; ++i) {
        hipEvent_t a;
        err = hipEventCreateWithFlags(&a, hipEventDisableTiming);
        if (err == hipSuccess) ev.push_back(a);
    }
    if (err != hipSuccess) {
        for (hipEvent_t a : ev) (void)hipEventDestroy(a);
        if (side) (void)hipStreamDestroy(side);
        return errorf("training: side stream / event creation failed: %s", hipGetErrorString(err));
    }
    t->ev = ev;
    t->side = side;
    return 0;
}
static int train_sync(mi355_train* t, int idx, hipStream_t from, hipStream_t to) { return ev_sync(t->ev[idx], from, to); }

extern "C" int mi355_denoise_step_train(mi355_plan* p, void* stream, const void* latents, int lat_dtype, const float* t, const void* enc_a,
                                        const void* pooled_a, const void* enc_b, const void* pooled_b, float guidance, const void* next_in,
                                        int next_in_dtype, const float* sigma, const float* sigma_next, const float* eta, int scalar_stride,
                                        float sigma_max, int dynamics, int compute_log_prob, float* next_f32, float* mean_out,
                                        float* noise_pred_out, float* log_prob, float* std_dev_t, float* dt) {
    if (!p || !latents || !t) return errorf("mi355_denoise_step_train: null argument");
    if (!next_in) return errorf("mi355_denoise_step_train: the differentiable step is the REPLAY of a stored transition: next_in is required");
    CHK(mi355_engine_weights_ready(p->e));
    hipStream_t st = (hipStream_t)stream;
    CHK(update_score_bounds(p->e, st));
    mi355_train* tr = nullptr;
    CHK(train_of(p, &tr));
    tr->fwd_full = train_state(p->e)->full;
    if (tr->fwd_full) CHK(train_full_of(tr));
    CHK(prepare_prompt(p, st, enc_a, pooled_a, enc_b, pooled_b));
    HIPCHK(hipMemcpyAsync(p->t_dev, t, (size_t)p->Bp * 4, hipMemcpyDeviceToDevice, st));
    CHK(prepare_conditioning(p, st, 1, lat_dtype));
    if (tr->fwd_full) {
        // inputs / intermediates of the conditioning path and the context embedder (their weight gradients need them; the plan's own
        // copies may be overwritten by a no-grad forward before the backward runs)
        mi355_engine* e = p->e;
        const int D = e->D, J = e->cfg.joint_attention_dim, P = e->cfg.pooled_projection_dim, T = e->cfg.time_proj_dim;
        const size_t eb = (size_t)p->B * p->Nt * J * 2, pb = (size_t)p->B * P * 2, db = (size_t)p->Bp * D * 2;
        HIPCHK(hipMemcpyAsync(tr->enc, enc_a, eb, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(tr->pool, pooled_a, pb, hipMemcpyDeviceToDevice, st));
        if (p->ncfg == 2) {
            HIPCHK(hipMemcpyAsync((char*)tr->enc + eb, enc_b, eb, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync((char*)tr->pool + pb, pooled_b, pb, hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(hipMemcpyAsync(tr->tproj, p->tproj, (size_t)p->Bp * T * 2, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(tr->h1, p->h1, db, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(tr->p1, p->p1, db, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(tr->pemb, p->pemb, db, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(tr->semb, p->semb, db, hipMemcpyDeviceToDevice, st));
    }
    // the text chain on the training state's side stream (shared with the backward), never a third stream or a late fork; the mid-size-GEMM
    // hint stays at its default and key 29 is honoured only inside ln_mod
    FwdSched s{};
    s.mid_hint = 1;
    if (g_train_two_stream) {
        CHK(train_side_init(tr));
        s.side = tr->side; s.join = tr->ev.data(); s.fork = tr->ev.data() + 1; s.ev_stride = 2;
    }
    CHK(forward_core(p, st, s, latents, lat_dtype, p->mod_all, p->v, tr));
    HIPCHK(copy_d2d(tr->mod, p->mod_all, (size_t)p->Bp * p->e->mod_cols * 2, st));
    HIPCHK(copy_d2d(tr->vnet, p->v, (size_t)p->Bp * p->n_lat * 2, st));
    const bf16_t* vu = p->ncfg == 2 ? p->v : nullptr;
    const bf16_t* vt = p->ncfg == 2 ? p->v + (int64_t)p->B * p->n_lat : p->v;
    return sde_call(st, p->B, p->n_lat, vt, vu, MI355_BF16, guidance, latents, lat_dtype, nullptr, next_in, next_in_dtype, sigma, sigma_next, eta,
                    scalar_stride, sigma_max, dynamics, compute_log_prob, nullptr, next_f32, mean_out, noise_pred_out, log_prob, std_dev_t, dt);
}

// ---- backward helpers ------------------------------------------------------------------------------------------------------
// out[M][N] = A[M][K] . WT[N][K]^T   (WT = transposed weight: a dgrad), bf16 out, optional fused gelu'(aux)
static int dgrad(mi355_train* t, hipStream_t st, const bf16_t* A, int K, const bf16_t* WT, int M, int N, bf16_t* out, const bf16_t* gelu_pre) {
    GemmParams g = gp(A, K, WT, K, M, N, K, gelu_pre ? EPI_DGELU : EPI_BIAS, t->zero_bias, out, N);
    if (gelu_pre) { g.aux = gelu_pre; g.ld_aux = N; }
    HIPCHK(gemm_p(g, st));
    return 0;
}

// (Round 4 kept an opt-in schedule here -- mi355_tune_set(26, 2): this engine's weight-gradient GEMMs on a third stream through a ring of operand
// slots, as the head_dim-128 engines do by default.  Measured neutral on the 349 M-parameter set in round 4 and, in round 5, on the reference's
// default target set: 86.5 / 86.7 ms serial vs 87.2 / 86.2 ms at B = 2, 1024^2, 31.4 vs 32.5 ms at 512^2 (profiles/r05h_*): removed.)
// dW[N][K] (fp32, overwritten) = dY[:, col0 : col0+N]^T . X ;  db[N] = column sums.  M rows; x_is_ready: the operand scratch already holds X^T
struct WgradScratch { bf16_t* aT; bf16_t* xT; float* part; float* csum; };
static int wgrad(mi355_train* t, hipStream_t st, const bf16_t* dY, long ldY, int col0, int N, const bf16_t* X, int K, int M, int M_pad,
                 float* gw, float* gb, bool x_ready, const WgradScratch* wsp = nullptr) {
    WgradScratch w = wsp ? *wsp : WgradScratch{t->aT, t->xT, t->part, t->csum};
    if (gb && !gw) HIPCHK(launch_colsum(dY + col0, ldY, M, N, w.csum, gb, 0, st));
    if (!gw) return 0;
    hipStream_t ws = st;
    const int split = wgrad_split(N, K, M_pad, t->part_floats, false);
    const bool reduce_follows = !(split <= 1 && grad_buf_dtype(gw) == DT_F32);
    // the fixed-order finish of the bias gradient's column sums rides in the weight gradient's split-K reduction launch where there is one
    // (always with bf16 gradient buffers; round 6: one launch per gradient pair fewer; g_fuse_colsum, mi355_tune_set(38, 0) = two launches)
    const bool fuse = gb && reduce_follows && g_fuse_colsum && grad_buf_dtype(gb) == grad_buf_dtype(gw) && ((long)N * K) % 4 == 0;
    // Round 6: operands as they lie in HBM -- dY [M][ldY] and X [M][K] row-major -- on the transposed-LDS-read kernel (gemm_tn.hip): neither
    // dY^T nor X^T is made (N and K multiples of 128; any M: a ragged last m-tile reads zeros for the missing rows).  Same partial sums bit for bit (same MFMA, operand order, m order and
    // split boundaries); the bias gradient takes the slab column-sum kernel (its fixed order differs from the transpose tiles': fp32 sums of
    // the same values in another association).  g_wgrad_tn: mi355_tune_set(39, .).
    {
        GemmTnParams tp{dY + col0, ldY, X, (long)K, M, N, K, reduce_follows ? w.part : gw, (long)K, reduce_follows ? split : 1, (long)N * K, nullptr, 0};
        tp.M_pad = M_pad;             // ragged M (the text stream's 333 rows per sample): the last m-tile's missing rows read zeros, like the copies' padding
        if (g_wgrad_tn && M_pad % 64 == 0 && (!reduce_follows || (size_t)N * K * (size_t)(split > 1 ? split : 1) <= t->part_floats) && gemm_tn_ok(tp)) {
            // mi355_tune_set(39, 2): 256 x 256 tiles (one 8-wave workgroup per CU, half the L2 -> LDS bytes per FLOP of the 128 x 128 form, which that
            // path bounds) where the shape gives a one-round grid: split over m so that tiles x split fills the chip (N = K = 1536: 36 tiles x 7).
            // NOT the default: the GEMM itself is faster (46 vs 57 us at M = 8192), the reduction over 7 instead of 4 fp32 partials takes the gain
            // back (18 vs 10 us): optimize() 84.7 ms either way over 2 x 6 interleaved runs (profiles/r06m_*).
            int sp = split;
            if (g_wgrad_tn == 2 && reduce_follows && N % 256 == 0 && K % 256 == 0) {
                const int t256 = (N / 256) * (K / 256);
                int s256 = 256 / t256;
                const int cap = (M / 64) / 2 > 0 ? (M / 64) / 2 : 1;
                if (s256 > cap) s256 = cap;
                while (s256 > 1 && (size_t)s256 * N * K > t->part_floats) --s256;
                if (s256 >= 1 && t256 * s256 >= 160) { tp.tile256 = 1; sp = s256; tp.k_split = sp; }
            }
            // bias gradient: with a finishing launch to ride in, the 128 x 128 form takes the per-split column sums from the dY fragments it holds
            // anyway (one slab per split); otherwise (and for the 256 x 256 form: no registers to spare) the slab column-sum kernel reads dY once more
            int nslab = 0;
            if (gb && fuse && !tp.tile256) { tp.colsum = w.csum; nslab = sp > 1 ? sp : 1; }
            else if (gb) HIPCHK(launch_colsum(dY + col0, ldY, M, N, w.csum, gb, 0, st, fuse ? &nslab : nullptr));
            HIPCHK(launch_gemm_tn(tp, ws));
            if (reduce_follows) {
                hipError_t fe = hipErrorNotSupported;
                if (fuse) fe = launch_splitk_reduce_colsum(w.part, (long)N * K, sp, gw, (long)N * K, w.csum, nslab, N, gb, ws);
                if (fe == hipErrorNotSupported) {
                    HIPCHK(launch_splitk_reduce(w.part, (long)N * K, sp, gw, (long)N * K, 0, ws));
                    if (fuse) HIPCHK(launch_colsum_finish(w.csum, nslab, N, gb, ws));
                } else HIPCHK(fe);
            }
            (wsp ? t->xT_c_holds : t->xT_holds) = nullptr;      // (the transposed-input scratch was not refreshed for this X)
            return 0;
        }
    }
    const bf16_t*& holds = wsp ? t->xT_c_holds : t->xT_holds;
    if (!x_ready || holds != X) { HIPCHK(launch_transpose(X, K, 0, w.xT, M_pad, 0, M, K, M_pad, 1, st)); holds = X; }
    // dY streams through once: its transpose for the wgrad GEMM and, on the way, its column sums (the bias gradient)
    if (gb) HIPCHK(launch_transpose_colsum(dY + col0, ldY, w.aT, M_pad, M, N, M_pad, w.csum, gb, st, !fuse));
    else HIPCHK(launch_transpose(dY + col0, ldY, 0, w.aT, M_pad, 0, M, N, M_pad, 1, st));
    GemmParams g = gp(w.aT, M_pad, w.xT, M_pad, N, K, M_pad, EPI_F32, nullptr, nullptr, K);
    g.q_scale = 1.0f;
    if (split <= 1 && grad_buf_dtype(gw) == DT_F32) {
        g.out_f32 = gw; g.k_split = 1;
        HIPCHK(gemm_p(g, ws));
    } else {
        if ((size_t)N * K > t->part_floats) return errorf("wgrad: a %d x %d gradient does not fit the split-K scratch", N, K);   // (bf16 output, single split)
        g.out_f32 = w.part; g.k_split = split; g.split_stride = (long)N * K;
        HIPCHK(gemm_p(g, ws));
        hipError_t fe = hipErrorNotSupported;
        if (fuse) fe = launch_splitk_reduce_colsum(w.part, (long)N * K, split, gw, (long)N * K, w.csum, (M_pad + 63) / 64, N, gb, ws);
        if (fe == hipErrorNotSupported) {
            HIPCHK(launch_splitk_reduce(w.part, (long)N * K, split, gw, (long)N * K, 0, ws));
            if (fuse) HIPCHK(launch_colsum_finish(w.csum, (M_pad + 63) / 64, N, gb, ws));      // (did not qualify after all: finish separately)
        } else HIPCHK(fe);
    }
    return 0;
}

// flash-attention backward of one attention: o / do token-major (image rows [, context rows]) -> dqkv token-major
static int attention_backward(mi355_plan* p, mi355_train* t, hipStream_t st, const bf16_t* q, const bf16_t* k, const bf16_t* vT, const float* lse,
                              const bf16_t* o_img, const bf16_t* o_ctx, const bf16_t* do_img, const bf16_t* do_ctx, int S, int S_pad, int n_img,
                              const float* rstd_img, const float* rstd_ctx, const float* nq, const float* nk, const float* ncq, const float* nck,
                              bf16_t* out_img, bf16_t* out_ctx, float* g_nq = nullptr, float* g_nk = nullptr, float* g_ncq = nullptr,
                              float* g_nck = nullptr) {
    mi355_engine* e = p->e;
    const int H = e->cfg.num_heads, BH = p->Bp * H;
    AttnBwdPrepParams pp{o_img, o_ctx, do_img, do_ctx, lse, t->doh, t->delta, t->nld, p->Bp, H, S, S_pad, n_img};
    HIPCHK(launch_attn_bwd_prep(pp, st));
    const long hs = (long)S_pad * 64;
    HIPCHK(launch_transpose(vT, S_pad, hs, t->v, 64, hs, 64, S_pad, 64, BH, st));
    AttnBwdParams ab{q, k, t->v, t->doh, lse, t->delta, t->nld, t->dq, t->dk, t->dv, p->Bp, H, S, S_pad};
    HIPCHK(launch_attention_bwd(ab, st));
    const float qs = get_attn_variant() >= 1 ? 0.125f * 1.4426950408889634f : 1.0f;
    const bool want_dw = g_nq || g_nk || g_ncq || g_nck;
    RmsBwdParams rb{q, k, t->dq, t->dk, t->dv, rstd_img, rstd_ctx, nq, nk, ncq, nck, qs, out_img, out_ctx, p->Bp, H, S, S_pad, n_img,
                    want_dw ? t->dw_part : nullptr};
    HIPCHK(launch_rms_bwd_gather(rb, st));
    if (want_dw) HIPCHK(launch_rms_dw_finish(t->dw_part, rms_bwd_grid(p->Bp, S), qs, g_nq, g_nk, g_ncq, g_nck, st));
    return 0;
}

// ---- full scope: gradients of everything outside the blocks' linear layers, after the block loop (t->dx = d x0, t->dc = d c0, t->dmod filled)
static int full_scope_tail(mi355_plan* p, mi355_train* t, hipStream_t st) {
    mi355_engine* e = p->e;
    TrainEngineState* ts = train_state(e);
    const int D = e->D, T = e->cfg.time_proj_dim, P = e->cfg.pooled_projection_dim, J = e->cfg.joint_attention_dim, Bp = p->Bp;
    auto GN = [&](const char* n) { return grad_of(e, n); };
    // patch embedding (conv k=p, s=p as a linear over the im2col patches) and context embedder
    if (GN("pos_embed.proj.weight") || GN("pos_embed.proj.bias"))
        CHK(wgrad(t, st, t->dx, D, 0, D, t->patches, e->KP, p->Mi, t->Mi_pad, GN("pos_embed.proj.weight"), GN("pos_embed.proj.bias"), false));
    if (GN("context_embedder.weight") || GN("context_embedder.bias"))
        CHK(wgrad(t, st, t->dc, D, 0, D, t->enc, J, p->Mc, t->Mc_pad, GN("context_embedder.weight"), GN("context_embedder.bias"), false));
    // AdaLN modulation linears: mod[b][:] = semb[b] . W_mod^T + b_mod  ->  dW rows = d mod^T . semb (M = B'), db = column sums
    HIPCHK(launch_f32_to_bf16_pad(t->dmod, t->dmod16, Bp, 64, e->mod_cols, st));
    bool xr = false;
    auto mod_w = [&](const std::string& name, int r0, int rows) -> int {
        float* gw = grad_of(e, name + ".weight");
        float* gb = grad_of(e, name + ".bias");
        if (!gw && !gb) return 0;
        CHK(wgrad(t, st, t->dmod16, e->mod_cols, r0, rows, t->semb, D, Bp, 64, gw, gb, xr));
        if (gw) xr = true;
        return 0;
    };
    for (int i = 0; i < e->L; ++i) {
        const BlockW& b = e->blk[i];
        const std::string pre = "transformer_blocks." + std::to_string(i);
        CHK(mod_w(pre + ".norm1.linear", b.mod_img, (b.dual ? 9 : 6) * D));
        CHK(mod_w(pre + ".norm1_context.linear", b.mod_ctx, (b.last ? 2 : 6) * D));
    }
    CHK(mod_w("norm_out.linear", e->mod_out, 2 * D));
    // conditioning MLPs: semb = silu(temb), temb = linear_2(silu(linear_1(tproj))) + text_linear_2(silu(text_linear_1(pooled)))
    const char* cond[8] = {"time_text_embed.timestep_embedder.linear_1.weight", "time_text_embed.timestep_embedder.linear_1.bias",
                           "time_text_embed.timestep_embedder.linear_2.weight", "time_text_embed.timestep_embedder.linear_2.bias",
                           "time_text_embed.text_embedder.linear_1.weight", "time_text_embed.text_embedder.linear_1.bias",
                           "time_text_embed.text_embedder.linear_2.weight", "time_text_embed.text_embedder.linear_2.bias"};
    bool any = false;
    for (const char* c : cond) any = any || GN(c);
    if (!any) return 0;
    if (!ts->wmodT) {
        if (hipMalloc((void**)&ts->wmodT, (size_t)D * e->mod_cols * 2) != hipSuccess) return errorf("training: hipMalloc of the transposed modulation weights failed");
        ts->wmod_dirty = true;
    }
    if (ts->wmod_dirty) {
        HIPCHK(launch_transpose(e->w_mod, D, 0, ts->wmodT, e->mod_cols, 0, e->mod_cols, D, e->mod_cols, 1, st));
        ts->wmod_dirty = false;
    }
    {   // d semb [B'][D] = d mod . W_mod: a skinny GEMM with K = mod_cols (499 200 for SD3.5-medium): split-K over 64 slices, fp32 partials
        const int nt = e->mod_cols / 64;
        int split = nt < 64 ? nt : 64;
        while (split > 1 && (size_t)split * Bp * D > t->part_floats) --split;
        GemmParams g = gp(t->dmod16, e->mod_cols, ts->wmodT, e->mod_cols, Bp, D, e->mod_cols, EPI_F32, nullptr, nullptr, D);
        g.q_scale = 1.0f; g.out_f32 = t->part; g.k_split = split; g.split_stride = (long)Bp * D;
        HIPCHK(gemm_p(g, st));
        HIPCHK(launch_splitk_reduce(t->part, (long)Bp * D, split, t->csum, (long)Bp * D, 0, st));
        HIPCHK(launch_convert(t->csum, DT_F32, t->dsemb, DT_BF16, (long)Bp * D, st));
    }
    {   // temb (pre-SiLU) recomputed: linear_2(h1) + bias + pemb
        GemmParams g = gp(t->h1, D, e->w_t2, D, Bp, D, D, EPI_POSADD, e->b_t2, t->temb, D);
        g.aux = t->pemb; g.ld_aux = D; g.rows_per_sample = Bp;
        HIPCHK(gemm_p(g, st));
    }
    HIPCHK(launch_silu_bwd(t->dsemb, t->temb, t->dtemb, (long)Bp * D, st));                                  // d temb = d t_emb = d pooled_emb
    // timestep branch
    CHK(wgrad(t, st, t->dtemb, D, 0, D, t->h1, D, Bp, 64, GN(cond[2]), GN(cond[3]), false));
    if (GN(cond[0]) || GN(cond[1])) {
        HIPCHK(launch_transpose(e->w_t2, D, 0, t->wT_small, D, 0, D, D, D, 1, st));
        CHK(dgrad(t, st, t->dtemb, D, t->wT_small, Bp, D, t->dh1, nullptr));
        GemmParams g = gp(t->tproj, T, e->w_t1, T, Bp, D, T, EPI_BIAS, e->b_t1, t->pre1, D);
        HIPCHK(gemm_p(g, st));
        HIPCHK(launch_silu_bwd(t->dh1, t->pre1, t->dh1, (long)Bp * D, st));
        CHK(wgrad(t, st, t->dh1, D, 0, D, t->tproj, T, Bp, 64, GN(cond[0]), GN(cond[1]), false));
    }
    // pooled-text branch
    CHK(wgrad(t, st, t->dtemb, D, 0, D, t->p1, D, Bp, 64, GN(cond[6]), GN(cond[7]), false));
    if (GN(cond[4]) || GN(cond[5])) {
        HIPCHK(launch_transpose(e->w_p2, D, 0, t->wT_small, D, 0, D, D, D, 1, st));
        CHK(dgrad(t, st, t->dtemb, D, t->wT_small, Bp, D, t->dh1, nullptr));
        GemmParams g = gp(t->pool, P, e->w_p1, P, Bp, D, P, EPI_BIAS, e->b_p1, t->pre1, D);
        HIPCHK(gemm_p(g, st));
        HIPCHK(launch_silu_bwd(t->dh1, t->pre1, t->dh1, (long)Bp * D, st));
        CHK(wgrad(t, st, t->dh1, D, 0, D, t->pool, P, Bp, 64, GN(cond[4]), GN(cond[5]), false));
    }
    return 0;
}

extern "C" int mi355_denoise_step_backward(mi355_plan* p, void* stream, const void* latents, int lat_dtype, float guidance, const void* next_in,
                                           int next_in_dtype, const float* sigma, const float* sigma_next, const float* eta, int scalar_stride,
                                           float sigma_max, int dynamics, int compute_log_prob, const float* g_log_prob, const float* g_noise_pred,
                                           const float* g_mean) {
    if (!p || !latents || !next_in) return errorf("mi355_denoise_step_backward: null argument");
    if (!p->train) return errorf("mi355_denoise_step_backward: no training-mode forward has run on this plan");
    if (get_attn_variant() < 1) return errorf("mi355_denoise_step_backward: needs the pre-scaled-q attention variant (mi355_tune_set(1, 1))");
    mi355_train* t = p->train;
    mi355_engine* e = p->e;
    hipStream_t st = (hipStream_t)stream;
    CHK(ensure_transposed_weights(e, st));
    TrainEngineState* ts = train_state(e);
    const int D = e->D, F = e->F;
    const int Mi = p->Mi, Mc = p->Mc, Ni = p->Ni, Nt = p->Nt;
    const int Ni_pad = (Ni + 63) / 64 * 64;
    const bf16_t* mod = t->mod;
    const long mld = e->mod_cols;
    const int NO = e->cfg.patch_size * e->cfg.patch_size * e->cfg.out_channels;
    auto G = [&](int i, const char* leaf) { return grad_of(e, "transformer_blocks." + std::to_string(i) + leaf); };
    const bool full = t->fwd_full;
    if (!full)
        for (auto& kv : ts->grads.grads)
            if (!trainable_name(kv.first))
                return errorf("mi355_denoise_step_backward: a gradient is registered for '%s' but the forward ran in the default scope "
                            "(mi355_engine_set_train_scope(engine, 1) must precede it)", kv.first.c_str());
    float* dmod = full ? t->dmod : nullptr;
    if (full) HIPCHK(hipMemsetAsync(t->dmod, 0, (size_t)p->Bp * e->mod_cols * 4, st));
    // dy = gate * dx  [+ d gate += sum_tokens dx * y in the full scope]
    auto gate_back = [&](hipStream_t s_, const bf16_t* dxp, int gate_off, const bf16_t* y, bf16_t* dy, long M, int rps) -> hipError_t {
        if (full) return launch_gate_bwd(dxp, mod + gate_off, mld, y, dy, dmod + gate_off, mld, M, D, rps, s_);
        return launch_gate_mul(dxp, mod + gate_off, mld, dy, M, D, rps, s_);
    };
    // LayerNorm-modulate backward [+ d shift / d scale in the full scope]
    auto ln_back = [&](hipStream_t s_, const bf16_t* x, const bf16_t* dy1, const bf16_t* dy2, bf16_t* dres, int M, int rps, int shift_off, int scale_off,
                       int shift2_off, int scale2_off, int accumulate) -> hipError_t {
        LnModBwdParams l{x, dy1, dy2, dres, mod, mld, scale_off, scale2_off, M, D, rps, e->cfg.eps, accumulate, dmod, shift_off, shift2_off};
        return launch_ln_mod_bwd(l, s_);
    };
    // The context stream's chain (MLP backward, attention out-projection dgrad | join | attention backward | fork | q|k|v dgrad, norm1
    // backward, and its weight gradients with their own scratch) on the side stream: in the default scope -- the full scope's d-modulation
    // sums (fp32 atomics of both streams into one table) stay on one stream.
    const bool two = g_train_two_stream != 0 && !full;
    if (two) CHK(train_side_init(t));
    hipStream_t cs = two ? t->side : st;
    bf16_t* dpre_c = two ? t->dpre_c : t->dpre;
    bf16_t* hid_c = two ? t->hid_c : t->hid;
    const WgradScratch wsc_{t->aT_c, t->xT_c, t->part_c, t->csum_c};
    const WgradScratch* wsc = two ? &wsc_ : nullptr;
    if (two) CHK(train_sync(t, 2 * e->L + 1, st, cs));       // the caller's stream up to here (the stash, the re-bound weights) before any side work

    // ---- d loss / d v  from the step's adjoint, then proj_out and norm_out
    {
        SdeBwdParams s;
        memset(&s, 0, sizeof(s));
        s.v_uncond = p->ncfg == 2 ? t->vnet : nullptr;
        s.v_text = p->ncfg == 2 ? t->vnet + (int64_t)p->B * p->n_lat : t->vnet;
        s.guidance = guidance; s.latents = latents; s.lat_dt = lat_dtype; s.next_in = next_in; s.next_in_dt = next_in_dtype;
        s.sigma = sigma; s.sigma_next = sigma_next; s.eta = eta; s.scalar_stride = scalar_stride; s.sigma_max = sigma_max;
        s.dynamics = dynamics; s.compute_log_prob = compute_log_prob; s.B = p->B; s.n = p->n_lat;
        s.g_lp = g_log_prob; s.g_np = g_noise_pred; s.g_mean = g_mean; s.dv = t->dv32;
        HIPCHK(launch_sde_step_bwd(s, st));
    }
    HIPCHK(launch_unpatch_bwd(t->dv32, t->dproj, p->Bp, e->cfg.out_channels, p->hp, p->wp, e->cfg.patch_size, st));
    if (full && (grad_of(e, "proj_out.weight") || grad_of(e, "proj_out.bias")))
        CHK(wgrad(t, st, t->dproj, NO, 0, NO, t->xn_out, D, Mi, t->Mi_pad, grad_of(e, "proj_out.weight"), grad_of(e, "proj_out.bias"), false));
    CHK(dgrad(t, st, t->dproj, NO, ts->proj, Mi, D, t->dxn, nullptr));
    HIPCHK(ln_back(st, t->x_final, t->dxn, nullptr, t->dx, Mi, Ni, e->mod_out + 1 * D, e->mod_out + 0 * D, 0, 0, 0));   // norm_out: scale first
    for (int i = e->L - 1; i >= 0; --i) {
        const BlockW& b = e->blk[i];
        const TrainBlk& k = t->blk[i];
        const TrainWT& w = ts->wt[i];
        const int mi = b.mod_img, mc = b.mod_ctx;
        // ---- MLP, image stream
        HIPCHK(gate_back(st, t->dx, mi + 5 * D, full ? t->fblk[i].y_ff : nullptr, t->dy, Mi, Ni));
        if (G(i, ".ff.net.2.weight") || G(i, ".ff.net.2.bias")) {
            if (G(i, ".ff.net.2.weight")) HIPCHK(launch_gelu_fwd(k.pre, t->hid, (long)Mi * F, st));
            CHK(wgrad(t, st, t->dy, D, 0, D, t->hid, F, Mi, t->Mi_pad, G(i, ".ff.net.2.weight"), G(i, ".ff.net.2.bias"), false));
        }
        CHK(dgrad(t, st, t->dy, D, w.ff2, Mi, F, t->dpre, k.pre));
        if (G(i, ".ff.net.0.proj.weight") || G(i, ".ff.net.0.proj.bias"))
            CHK(wgrad(t, st, t->dpre, F, 0, F, k.xn_mlp, D, Mi, t->Mi_pad, G(i, ".ff.net.0.proj.weight"), G(i, ".ff.net.0.proj.bias"), false));
        CHK(dgrad(t, st, t->dpre, F, w.ff1, Mi, D, t->dxn, nullptr));
        HIPCHK(ln_back(st, k.x_mid, t->dxn, nullptr, t->dx, Mi, Ni, mi + 3 * D, mi + 4 * D, 0, 0, 1));
        // ---- MLP, context stream
        if (!b.last) {
            HIPCHK(gate_back(cs, t->dc, mc + 5 * D, full ? t->fblk[i].y_cff : nullptr, t->dyc, Mc, Nt));
            if (G(i, ".ff_context.net.2.weight") || G(i, ".ff_context.net.2.bias")) {
                if (G(i, ".ff_context.net.2.weight")) HIPCHK(launch_gelu_fwd(k.cpre, hid_c, (long)Mc * F, cs));
                CHK(wgrad(t, cs, t->dyc, D, 0, D, hid_c, F, Mc, t->Mc_pad, G(i, ".ff_context.net.2.weight"), G(i, ".ff_context.net.2.bias"), false, wsc));
            }
            CHK(dgrad(t, cs, t->dyc, D, w.cff2, Mc, F, dpre_c, k.cpre));
            if (G(i, ".ff_context.net.0.proj.weight") || G(i, ".ff_context.net.0.proj.bias"))
                CHK(wgrad(t, cs, dpre_c, F, 0, F, k.cn_mlp, D, Mc, t->Mc_pad, G(i, ".ff_context.net.0.proj.weight"),
                          G(i, ".ff_context.net.0.proj.bias"), false, wsc));
            CHK(dgrad(t, cs, dpre_c, F, w.cff1, Mc, D, t->dcn, nullptr));
            HIPCHK(ln_back(cs, k.c_mid, t->dcn, nullptr, t->dc, Mc, Nt, mc + 3 * D, mc + 4 * D, 0, 0, 1));
        }
        // ---- dual (image-only) attention
        if (b.dual) {
            HIPCHK(gate_back(st, t->dx, mi + 8 * D, full ? t->fblk[i].y_o2 : nullptr, t->dy, Mi, Ni));
            if (G(i, ".attn2.to_out.0.weight") || G(i, ".attn2.to_out.0.bias"))
                CHK(wgrad(t, st, t->dy, D, 0, D, k.o2, D, Mi, t->Mi_pad, G(i, ".attn2.to_out.0.weight"), G(i, ".attn2.to_out.0.bias"), false));
            CHK(dgrad(t, st, t->dy, D, w.o2, Mi, D, t->do_img, nullptr));
            CHK(attention_backward(p, t, st, k.q2, k.k2, k.vT2, k.lse2, k.o2, nullptr, t->do_img, nullptr, Ni, Ni_pad, Ni, k.rstd2, nullptr,
                                   b.nq2, b.nk2, b.nq2, b.nk2, t->dqkv_img, nullptr, full ? G(i, ".attn2.norm_q.weight") : nullptr,
                                   full ? G(i, ".attn2.norm_k.weight") : nullptr, nullptr, nullptr));
            bool xr = false;
            const char* nm[3] = {".attn2.to_q", ".attn2.to_k", ".attn2.to_v"};
            for (int j = 0; j < 3; ++j) {
                float* gw = G(i, (std::string(nm[j]) + ".weight").c_str());
                float* gb = G(i, (std::string(nm[j]) + ".bias").c_str());
                if (gw || gb) { CHK(wgrad(t, st, t->dqkv_img, 3 * D, j * D, D, k.xn2, D, Mi, t->Mi_pad, gw, gb, xr)); if (gw) xr = true; }
            }
            CHK(dgrad(t, st, t->dqkv_img, 3 * D, w.qkv2, Mi, D, t->dxn2, nullptr));
        }
        // ---- joint attention
        HIPCHK(gate_back(st, t->dx, mi + 2 * D, full ? t->fblk[i].y_o : nullptr, t->dy, Mi, Ni));
        if (G(i, ".attn.to_out.0.weight") || G(i, ".attn.to_out.0.bias"))
            CHK(wgrad(t, st, t->dy, D, 0, D, k.o_img, D, Mi, t->Mi_pad, G(i, ".attn.to_out.0.weight"), G(i, ".attn.to_out.0.bias"), false));
        CHK(dgrad(t, st, t->dy, D, w.o, Mi, D, t->do_img, nullptr));
        if (!b.last) {
            HIPCHK(gate_back(cs, t->dc, mc + 2 * D, full ? t->fblk[i].y_co : nullptr, t->dyc, Mc, Nt));
            if (G(i, ".attn.to_add_out.weight") || G(i, ".attn.to_add_out.bias"))
                CHK(wgrad(t, cs, t->dyc, D, 0, D, k.o_ctx, D, Mc, t->Mc_pad, G(i, ".attn.to_add_out.weight"), G(i, ".attn.to_add_out.bias"), false, wsc));
            CHK(dgrad(t, cs, t->dyc, D, w.co, Mc, D, t->do_ctx, nullptr));
        }
        if (two) CHK(train_sync(t, 2 * i, cs, st));          // join: the attention backward reads do_ctx and overwrites dqkv_ctx
        CHK(attention_backward(p, t, st, k.q, k.k, k.vT, k.lse, k.o_img, k.o_ctx, t->do_img, b.last ? nullptr : t->do_ctx, p->S, p->S_pad, Ni,
                               k.rstd_img, k.rstd_ctx, b.nq, b.nk, b.ncq, b.nck, t->dqkv_img, t->dqkv_ctx, full ? G(i, ".attn.norm_q.weight") : nullptr,
                               full ? G(i, ".attn.norm_k.weight") : nullptr, full ? G(i, ".attn.norm_added_q.weight") : nullptr,
                               full ? G(i, ".attn.norm_added_k.weight") : nullptr));
        if (two) CHK(train_sync(t, 2 * i + 1, st, cs));      // fork: dqkv_ctx is complete (and do_ctx may be overwritten)
        {
            bool xr = false;
            const char* nm[3] = {".attn.to_q", ".attn.to_k", ".attn.to_v"};
            for (int j = 0; j < 3; ++j) {
                float* gw = G(i, (std::string(nm[j]) + ".weight").c_str());
                float* gb = G(i, (std::string(nm[j]) + ".bias").c_str());
                if (gw || gb) { CHK(wgrad(t, st, t->dqkv_img, 3 * D, j * D, D, k.xn, D, Mi, t->Mi_pad, gw, gb, xr)); if (gw) xr = true; }
            }
            xr = false;
            const char* cn[3] = {".attn.add_q_proj", ".attn.add_k_proj", ".attn.add_v_proj"};
            for (int j = 0; j < 3; ++j) {
                float* gw = G(i, (std::string(cn[j]) + ".weight").c_str());
                float* gb = G(i, (std::string(cn[j]) + ".bias").c_str());
                if (gw || gb) { CHK(wgrad(t, cs, t->dqkv_ctx, 3 * D, j * D, D, k.cn, D, Mc, t->Mc_pad, gw, gb, xr, wsc)); if (gw) xr = true; }
            }
        }
        CHK(dgrad(t, st, t->dqkv_img, 3 * D, w.qkv, Mi, D, t->dxn, nullptr));
        CHK(dgrad(t, cs, t->dqkv_ctx, 3 * D, w.cqkv, Mc, D, t->dcn, nullptr));
        HIPCHK(ln_back(st, k.x_in, t->dxn, b.dual ? t->dxn2 : nullptr, t->dx, Mi, Ni, mi + 0 * D, mi + 1 * D, mi + 6 * D, mi + 7 * D, 1));
        // the last block's context stream has no later consumer: its norm1_context (AdaLayerNormContinuous: scale first) starts dc
        if (b.last) HIPCHK(ln_back(cs, k.c_in, t->dcn, nullptr, t->dc, Mc, Nt, mc + 1 * D, mc + 0 * D, 0, 0, 0));
        else HIPCHK(ln_back(cs, k.c_in, t->dcn, nullptr, t->dc, Mc, Nt, mc + 0 * D, mc + 1 * D, 0, 0, 1));
    }
    if (two) CHK(train_sync(t, 2 * e->L, cs, st));           // the caller's stream goes on only after the context chain
    if (full) CHK(full_scope_tail(p, t, st));
    return 0;
}

// ---- operator-level entry point (unit tests): attention forward (with log-sum-exp) + backward on caller-provided tensors ------------
// q (already scaled by log2(e)/8), k: [B][H][S_pad][64], vT: [B][H][64][S_pad]; d_o token-major [B*S][H*64] -> o [B*S][H*64], dq, dk, dv
// [B][H][S_pad][64].  Scratch is allocated and freed inside (test helper, synchronises).
extern "C" int mi355_op_attention_fwd_bwd(void* stream, const void* q, const void* k, const void* vT, const void* d_o, void* o, void* dq, void* dk,
                                          void* dv, int B, int H, int S, int S_pad) {
    if (!q || !k || !vT || !d_o || !o || !dq || !dk || !dv) return errorf("mi355_op_attention_fwd_bwd: null argument");
    if (B <= 0 || H <= 0 || S <= 0 || S_pad < S || S_pad % 64) return errorf("mi355_op_attention_fwd_bwd: bad shape (S %d, S_pad %d)", S, S_pad);
    hipStream_t st = (hipStream_t)stream;
    const size_t el = (size_t)B * H * S_pad * 64;
    char* ws = nullptr;
    const size_t bytes = el * 2 * 2 + (size_t)B * H * S_pad * 4 * 4;
    HIPCHK(hipMalloc((void**)&ws, bytes));
    HIPCHK(hipMemsetAsync(ws, 0, bytes, st));
    bf16_t* doh = (bf16_t*)ws; bf16_t* v = doh + el;
    float* lse = (float*)(v + el); float* delta = lse + (size_t)B * H * S_pad; float* nld = delta + (size_t)B * H * S_pad;
    AttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vT, (bf16_t*)o, nullptr, B, H, S, S_pad, S, 1,
                 g_attn_static >= 2 ? (float)g_attn_static : 0.f, lse};
    hipError_t err = launch_attention(a, st);
    AttnBwdPrepParams pp{(const bf16_t*)o, nullptr, (const bf16_t*)d_o, nullptr, lse, doh, delta, nld, B, H, S, S_pad, S};
    if (err == hipSuccess) err = launch_attn_bwd_prep(pp, st);
    const long hs = (long)S_pad * 64;
    if (err == hipSuccess) err = launch_transpose((const bf16_t*)vT, S_pad, hs, v, 64, hs, 64, S_pad, 64, B * H, st);
    AttnBwdParams ab{(const bf16_t*)q, (const bf16_t*)k, v, doh, lse, delta, nld, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, B, H, S, S_pad};
    if (err == hipSuccess) err = launch_attention_bwd(ab, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    (void)hipFree(ws);
    if (err != hipSuccess) return errorf("mi355_op_attention_fwd_bwd: %s", hipGetErrorString(err));
    return 0;
}

// The same with the fields the helper above pins exposed: the image / context split of o and dO (AttnBwdPrepParams::n_img; do_ctx may be NULL:
// that part of the output has no consumer), the |score| bound as an argument, and optional copies of the forward's log2-sum-exp and of the
// backward's delta = rowsum(dO * O), both [B][H][S_pad] fp32 (rows >= S: zero, as the zeroed scratch holds them).
extern "C" int mi355_op_attention_fwd_bwd_ex(void* stream, const void* q, const void* k, const void* vT, const void* do_img, const void* do_ctx,
                                             void* o_img, void* o_ctx, void* dq, void* dk, void* dv, int B, int H, int S, int S_pad, int n_img,
                                             float score_bound, float* lse_out, float* delta_out) {
    if (!q || !k || !vT || !dq || !dk || !dv) return errorf("mi355_op_attention_fwd_bwd_ex: null argument");
    if (B <= 0 || H <= 0 || S <= 0 || S_pad < S || S_pad % 64) return errorf("mi355_op_attention_fwd_bwd_ex: bad shape (S %d, S_pad %d)", S, S_pad);
    if (n_img < 0 || n_img > S) return errorf("mi355_op_attention_fwd_bwd_ex: n_img %d outside [0, S = %d]", n_img, S);
    if (n_img > 0 && (!o_img || !do_img)) return errorf("mi355_op_attention_fwd_bwd_ex: o_img / do_img is NULL but n_img > 0");
    if (n_img < S && !o_ctx) return errorf("mi355_op_attention_fwd_bwd_ex: o_ctx is NULL but S > n_img");
    if (!(score_bound >= 0.f)) return errorf("mi355_op_attention_fwd_bwd_ex: negative score_bound");
    if (get_attn_variant() == 0) return errorf("mi355_op_attention_fwd_bwd_ex: q is pre-scaled here, which the plain forward (mi355_tune_set(1, 0)) does not take");
    hipStream_t st = (hipStream_t)stream;
    const size_t bhs = (size_t)B * H * S_pad, el = bhs * 64;
    char* ws = nullptr;
    const size_t bytes = el * 2 * 2 + bhs * 4 * 4;
    HIPCHK(hipMalloc((void**)&ws, bytes));
    hipError_t err = hipMemsetAsync(ws, 0, bytes, st);       // the zero-padding contract of the backward, on the caller's stream
    bf16_t* doh = (bf16_t*)ws; bf16_t* v = doh + el;
    float* lse = (float*)(v + el); float* delta = lse + bhs; float* nld = delta + bhs;
    AttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)vT, (bf16_t*)o_img, (bf16_t*)o_ctx, B, H, S, S_pad, n_img, 1, score_bound, lse};
    if (err == hipSuccess) err = launch_attention(a, st);
    AttnBwdPrepParams pp{(const bf16_t*)o_img, (const bf16_t*)o_ctx, (const bf16_t*)do_img, (const bf16_t*)do_ctx, lse, doh, delta, nld, B, H, S, S_pad,
                         n_img};
    if (err == hipSuccess) err = launch_attn_bwd_prep(pp, st);
    const long hs = (long)S_pad * 64;
    if (err == hipSuccess) err = launch_transpose((const bf16_t*)vT, S_pad, hs, v, 64, hs, 64, S_pad, 64, B * H, st);
    AttnBwdParams ab{(const bf16_t*)q, (const bf16_t*)k, v, doh, lse, delta, nld, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, B, H, S, S_pad};
    if (err == hipSuccess) err = launch_attention_bwd(ab, st);
    if (err == hipSuccess && lse_out) err = hipMemcpyAsync(lse_out, lse, bhs * 4, hipMemcpyDeviceToDevice, st);
    if (err == hipSuccess && delta_out) err = hipMemcpyAsync(delta_out, delta, bhs * 4, hipMemcpyDeviceToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    (void)hipFree(ws);
    if (err != hipSuccess) return errorf("mi355_op_attention_fwd_bwd_ex: %s", hipGetErrorString(err));
    return 0;
}

// ---- operator-level entry points of the backward's streaming / reduction kernels (backward.hip; tests/test_gpu_backward_ops.py) ----------
// One per launcher family: arguments are checked before any HIP call, the launch goes to the caller's stream, nothing is allocated and
// nothing synchronises.  Buffer extents are the caller's business (the launchers' header comments in kernels.h state them).
// An output that may be a bf16 gradient buffer carries a dtype: it is marked for the launch and un-marked after it.
static int op_out_dtype_ok(int dt) { return dt == DT_F32 || dt == DT_BF16; }

static int op_ln_mod_bwd(const char* who, void* stream, const void* x, const void* dy, const void* dy2, void* dres, const void* mod, int64_t mod_ld,
                         int shift_off, int scale_off, int shift2_off, int scale2_off, int M, int D, int rows_per_sample, float eps,
                         int accumulate, float* dmod, int head_rows) {
    if (!x || !dy || !dres || !mod) return errorf("%s: null argument", who);
    if (M <= 0 || rows_per_sample <= 0) return errorf("%s: bad shape (M %d, rows_per_sample %d)", who, M, rows_per_sample);
    if (D <= 0 || D % 8) return errorf("%s: D = %d is not a positive multiple of 8", who, D);
    if (D > (dmod ? 4096 : 6144)) return errorf("%s: D = %d is wider than %d (%s modulation gradients)", who, D, dmod ? 4096 : 6144, dmod ? "with" : "without");
    if (scale_off < 0 || (dy2 && scale2_off < 0) || (dmod && (shift_off < 0 || (dy2 && shift2_off < 0))) || mod_ld < D)
        return errorf("%s: bad modulation layout (mod_ld %lld)", who, (long long)mod_ld);
    if (head_rows < 0 || head_rows > rows_per_sample) return errorf("%s: head_rows = %d outside [0, rows_per_sample = %d]", who, head_rows, rows_per_sample);
    if (head_rows > 0 && dmod) return errorf("%s: modulation gradients (dmod) of a two-group table (head_rows = %d) are not implemented", who, head_rows);
    LnModBwdParams p{(const bf16_t*)x, (const bf16_t*)dy, (const bf16_t*)dy2, (bf16_t*)dres, (const bf16_t*)mod, (long)mod_ld, scale_off, scale2_off,
                     M, D, rows_per_sample, eps, accumulate, dmod, shift_off, shift2_off, head_rows};
    hipError_t err = launch_ln_mod_bwd(p, (hipStream_t)stream);
    if (err != hipSuccess) return errorf("%s: %s", who, hipGetErrorString(err));
    return 0;
}

extern "C" int mi355_op_ln_mod_bwd(void* stream, const void* x, const void* dy, const void* dy2, void* dres, const void* mod, int64_t mod_ld,
                                   int shift_off, int scale_off, int shift2_off, int scale2_off, int M, int D, int rows_per_sample, float eps,
                                   int accumulate, float* dmod) {
    return op_ln_mod_bwd("mi355_op_ln_mod_bwd", stream, x, dy, dy2, dres, mod, mod_ld, shift_off, scale_off, shift2_off, scale2_off, M, D, rows_per_sample,
                         eps, accumulate, dmod, 0);
}
// two-group table: head_rows > 0 = row m reads modulation row 2 (m / rows_per_sample) + (m % rows_per_sample >= head_rows); refused together with dmod
extern "C" int mi355_op_ln_mod_bwd_split(void* stream, const void* x, const void* dy, const void* dy2, void* dres, const void* mod, int64_t mod_ld,
                                         int shift_off, int scale_off, int shift2_off, int scale2_off, int M, int D, int rows_per_sample, float eps,
                                         int accumulate, float* dmod, int head_rows) {
    return op_ln_mod_bwd("mi355_op_ln_mod_bwd_split", stream, x, dy, dy2, dres, mod, mod_ld, shift_off, scale_off, shift2_off, scale2_off, M, D,
                         rows_per_sample, eps, accumulate, dmod, head_rows);
}

// y == NULL && dgate == NULL: dy = gate * dx only (launch_gate_mul); both given: dgate += sum dx * y as well (launch_gate_bwd)
static int op_gate_bwd(const char* who, void* stream, const void* dx, const void* gate, int64_t gate_ld, const void* y, void* dy, float* dgate, int64_t dg_ld,
                       int64_t M, int D, int rows_per_sample, int head_rows) {
    if (!dx || !gate || !dy) return errorf("%s: null argument", who);
    if ((y == nullptr) != (dgate == nullptr)) return errorf("%s: y and dgate go together (both NULL: the product only)", who);
    if (M <= 0 || rows_per_sample <= 0) return errorf("%s: bad shape (M %lld, rows_per_sample %d)", who, (long long)M, rows_per_sample);
    if (D <= 0 || D % 8) return errorf("%s: D = %d is not a positive multiple of 8", who, D);
    if (gate_ld < D || (dgate && dg_ld < D)) return errorf("%s: a row stride is below D = %d", who, D);
    if (head_rows < 0 || head_rows > rows_per_sample) return errorf("%s: head_rows = %d outside [0, rows_per_sample = %d]", who, head_rows, rows_per_sample);
    if (head_rows > 0 && dgate) return errorf("%s: the gate gradient (dgate) of a two-group table (head_rows = %d) is not implemented", who, head_rows);
    hipError_t err = y ? launch_gate_bwd((const bf16_t*)dx, (const bf16_t*)gate, (long)gate_ld, (const bf16_t*)y, (bf16_t*)dy, dgate, (long)dg_ld, (long)M, D,
                                         rows_per_sample, (hipStream_t)stream)
                       : launch_gate_mul((const bf16_t*)dx, (const bf16_t*)gate, (long)gate_ld, (bf16_t*)dy, (long)M, D, rows_per_sample, (hipStream_t)stream,
                                         head_rows);
    if (err != hipSuccess) return errorf("%s: %s", who, hipGetErrorString(err));
    return 0;
}

extern "C" int mi355_op_gate_bwd(void* stream, const void* dx, const void* gate, int64_t gate_ld, const void* y, void* dy, float* dgate, int64_t dg_ld,
                                 int64_t M, int D, int rows_per_sample) {
    return op_gate_bwd("mi355_op_gate_bwd", stream, dx, gate, gate_ld, y, dy, dgate, dg_ld, M, D, rows_per_sample, 0);
}
// two-group gate table: head_rows > 0 = row m reads gate row 2 (m / rows_per_sample) + (m % rows_per_sample >= head_rows); refused together with dgate
extern "C" int mi355_op_gate_bwd_split(void* stream, const void* dx, const void* gate, int64_t gate_ld, const void* y, void* dy, float* dgate,
                                       int64_t dg_ld, int64_t M, int D, int rows_per_sample, int head_rows) {
    return op_gate_bwd("mi355_op_gate_bwd_split", stream, dx, gate, gate_ld, y, dy, dgate, dg_ld, M, D, rows_per_sample, head_rows);
}

extern "C" int mi355_op_silu_bwd(void* stream, const void* dy, const void* pre, void* dx, int64_t n) {
    if (!dy || !pre || !dx) return errorf("mi355_op_silu_bwd: null argument");
    if (n <= 0 || n % 8) return errorf("mi355_op_silu_bwd: n = %lld is not a positive multiple of 8", (long long)n);
    hipError_t err = launch_silu_bwd((const bf16_t*)dy, (const bf16_t*)pre, (bf16_t*)dx, (long)n, (hipStream_t)stream);
    if (err != hipSuccess) return errorf("mi355_op_silu_bwd: %s", hipGetErrorString(err));
    return 0;
}

extern "C" int mi355_op_gelu_fwd(void* stream, const void* pre, void* out, int64_t n) {
    if (!pre || !out) return errorf("mi355_op_gelu_fwd: null argument");
    if (n <= 0 || n % 8) return errorf("mi355_op_gelu_fwd: n = %lld is not a positive multiple of 8", (long long)n);
    hipError_t err = launch_gelu_fwd((const bf16_t*)pre, (bf16_t*)out, (long)n, (hipStream_t)stream);
    if (err != hipSuccess) return errorf("mi355_op_gelu_fwd: %s", hipGetErrorString(err));
    return 0;
}

// scratch == NULL && colsum == NULL: launch_transpose (with batch strides); both given (batch 1): launch_transpose_colsum, `finish` = 0 leaves
// the ((rows_pad + 63) / 64) x cols row-tile partials in `scratch` for mi355_op_splitk_reduce to finish
extern "C" int mi355_op_transpose(void* stream, const void* in, int64_t ld_in, int64_t bs_in, void* out, int64_t ld_out, int64_t bs_out, int rows, int cols,
                                  int rows_pad, int batch, float* scratch, void* colsum, int colsum_dtype, int finish) {
    if (!in || !out) return errorf("mi355_op_transpose: null argument");
    if (rows <= 0 || cols <= 0 || batch <= 0) return errorf("mi355_op_transpose: bad shape (rows %d, cols %d, batch %d)", rows, cols, batch);
    if (rows_pad < rows) return errorf("mi355_op_transpose: rows_pad = %d is below rows = %d", rows_pad, rows);
    if (ld_in < cols || ld_out < rows_pad) return errorf("mi355_op_transpose: a row stride is below its row (ld_in %lld, ld_out %lld)", (long long)ld_in, (long long)ld_out);
    if ((scratch == nullptr) != (colsum == nullptr)) return errorf("mi355_op_transpose: scratch and colsum go together");
    hipError_t err;
    if (!scratch) {
        err = launch_transpose((const bf16_t*)in, (long)ld_in, (long)bs_in, (bf16_t*)out, (long)ld_out, (long)bs_out, rows, cols, rows_pad, batch, (hipStream_t)stream);
    } else {
        if (batch != 1) return errorf("mi355_op_transpose: the column sums are taken of one matrix (batch %d)", batch);
        if (!op_out_dtype_ok(colsum_dtype)) return errorf("mi355_op_transpose: column sums are fp32 or bf16 (dtype %d)", colsum_dtype);
        grad_buf_mark(colsum, colsum_dtype);
        err = launch_transpose_colsum((const bf16_t*)in, (long)ld_in, (bf16_t*)out, (long)ld_out, rows, cols, rows_pad, scratch, (float*)colsum,
                                      (hipStream_t)stream, finish != 0);
        grad_buf_mark(colsum, DT_F32);
    }
    if (err != hipSuccess) return errorf("mi355_op_transpose: %s", hipGetErrorString(err));
    return 0;
}

// out[n] (+)= sum_m dy[m][n]; scratch: 64 * N floats
extern "C" int mi355_op_colsum(void* stream, const void* dy, int64_t ld, int64_t M, int N, float* scratch, void* out, int out_dtype, int accumulate) {
    if (!dy || !scratch || !out) return errorf("mi355_op_colsum: null argument");
    if (M <= 0 || N <= 0 || ld < N) return errorf("mi355_op_colsum: bad shape (M %lld, N %d, ld %lld)", (long long)M, N, (long long)ld);
    if (!op_out_dtype_ok(out_dtype)) return errorf("mi355_op_colsum: the output is fp32 or bf16 (dtype %d)", out_dtype);
    grad_buf_mark(out, out_dtype);
    hipError_t err = launch_colsum((const bf16_t*)dy, (long)ld, (long)M, N, scratch, (float*)out, accumulate, (hipStream_t)stream);
    grad_buf_mark(out, DT_F32);
    if (err != hipSuccess) return errorf("mi355_op_colsum: %s", hipGetErrorString(err));
    return 0;
}

// out[i] (+)= sum_s part[s * stride + i].  cs_scratch / colsum given: the one-launch pair launch_splitk_reduce_colsum (out overwritten, colsum =
// fixed-order sum of `nslab` x `cols` partials); a pair that does not qualify returns 2 with nothing launched -- its own value, not an error of the call.
extern "C" int mi355_op_splitk_reduce(void* stream, const float* part, int64_t stride, int nsplit, void* out, int out_dtype, int64_t n, int accumulate,
                                      const float* cs_scratch, int nslab, int cols, void* colsum, int colsum_dtype) {
    if (!part || !out) return errorf("mi355_op_splitk_reduce: null argument");
    if (nsplit <= 0) return errorf("mi355_op_splitk_reduce: nsplit = %d", nsplit);
    if (n <= 0 || stride < n) return errorf("mi355_op_splitk_reduce: bad shape (n %lld, stride %lld)", (long long)n, (long long)stride);
    if (!op_out_dtype_ok(out_dtype)) return errorf("mi355_op_splitk_reduce: the output is fp32 or bf16 (dtype %d)", out_dtype);
    if ((cs_scratch == nullptr) != (colsum == nullptr)) return errorf("mi355_op_splitk_reduce: cs_scratch and colsum go together");
    hipError_t err;
    if (!colsum) {
        grad_buf_mark(out, out_dtype);
        err = launch_splitk_reduce(part, (long)stride, nsplit, (float*)out, (long)n, accumulate, (hipStream_t)stream);
        grad_buf_mark(out, DT_F32);
    } else {
        if (nslab <= 0 || cols <= 0) return errorf("mi355_op_splitk_reduce: bad column-sum shape (nslab %d, cols %d)", nslab, cols);
        if (!op_out_dtype_ok(colsum_dtype)) return errorf("mi355_op_splitk_reduce: column sums are fp32 or bf16 (dtype %d)", colsum_dtype);
        if (accumulate) return errorf("mi355_op_splitk_reduce: the one-launch pair overwrites its outputs (accumulate must be 0)");
        grad_buf_mark(out, out_dtype);
        grad_buf_mark(colsum, colsum_dtype);
        err = launch_splitk_reduce_colsum(part, (long)stride, nsplit, (float*)out, (long)n, cs_scratch, nslab, cols, (float*)colsum, (hipStream_t)stream);
        grad_buf_mark(colsum, DT_F32);
        grad_buf_mark(out, DT_F32);
        if (err == hipErrorNotSupported) {
            errorf("mi355_op_splitk_reduce: this pair takes two launches (n %% 4, stride %% 4, 16-byte alignment or mixed output dtypes)");
            return 2;
        }
    }
    if (err != hipSuccess) return errorf("mi355_op_splitk_reduce: %s", hipGetErrorString(err));
    return 0;
}

extern "C" int mi355_op_f32_to_bf16_pad(void* stream, const float* in, void* out, int64_t rows, int64_t rows_pad, int64_t cols) {
    if (!in || !out) return errorf("mi355_op_f32_to_bf16_pad: null argument");
    if (rows <= 0 || cols <= 0) return errorf("mi355_op_f32_to_bf16_pad: bad shape (rows %lld, cols %lld)", (long long)rows, (long long)cols);
    if (rows_pad < rows) return errorf("mi355_op_f32_to_bf16_pad: rows_pad = %lld is below rows = %lld", (long long)rows_pad, (long long)rows);
    hipError_t err = launch_f32_to_bf16_pad(in, (bf16_t*)out, (long)rows, (long)rows_pad, (long)cols, (hipStream_t)stream);
    if (err != hipSuccess) return errorf("mi355_op_f32_to_bf16_pad: %s", hipGetErrorString(err));
    return 0;
}

extern "C" int mi355_op_unpatch_bwd(void* stream, const float* dv, void* out, int Bp, int C, int hp, int wp, int patch) {
    if (!dv || !out) return errorf("mi355_op_unpatch_bwd: null argument");
    if (Bp <= 0 || C <= 0 || hp <= 0 || wp <= 0 || patch <= 0)
        return errorf("mi355_op_unpatch_bwd: bad shape (Bp %d, C %d, hp %d, wp %d, patch %d)", Bp, C, hp, wp, patch);
    hipError_t err = launch_unpatch_bwd(dv, (bf16_t*)out, Bp, C, hp, wp, patch, (hipStream_t)stream);
    if (err != hipSuccess) return errorf("mi355_op_unpatch_bwd: %s", hipGetErrorString(err));
    return 0;
}

static const char* op_attn_split_error(int B, int H, int S, int S_pad, int n_img) {
    if (B <= 0 || H <= 0 || S <= 0) return "B, H and S must be positive";
    if (S_pad % 64) return "S_pad is not a multiple of 64";
    if (S_pad < S) return "S_pad is below S";
    if (n_img < 0 || n_img > S) return "n_img outside [0, S]";
    return nullptr;
}

// the general or the 16-byte form by mi355_tune_set(25, .)
extern "C" int mi355_op_attn_bwd_prep(void* stream, const void* o_img, const void* o_ctx, const void* do_img, const void* do_ctx, const float* lse, void* doh,
                                      float* delta, float* nld, int B, int H, int S, int S_pad, int n_img) {
    if (!lse || !doh || !delta || !nld) return errorf("mi355_op_attn_bwd_prep: null argument");
    if (const char* why = op_attn_split_error(B, H, S, S_pad, n_img)) return errorf("mi355_op_attn_bwd_prep: %s (S %d, S_pad %d, n_img %d)", why, S, S_pad, n_img);
    if (n_img > 0 && (!o_img || !do_img)) return errorf("mi355_op_attn_bwd_prep: o_img / do_img is NULL but n_img > 0");
    if (n_img < S && !o_ctx) return errorf("mi355_op_attn_bwd_prep: o_ctx is NULL but S > n_img");
    AttnBwdPrepParams pp{(const bf16_t*)o_img, (const bf16_t*)o_ctx, (const bf16_t*)do_img, (const bf16_t*)do_ctx, lse, (bf16_t*)doh, delta, nld, B, H, S, S_pad, n_img};
    hipError_t err = launch_attn_bwd_prep(pp, (hipStream_t)stream);
    if (err != hipSuccess) return errorf("mi355_op_attn_bwd_prep: %s", hipGetErrorString(err));
    return 0;
}

// dw_part given ([rms_bwd_grid(B, S)][4][64] floats): the general kernel at 8 tokens per wave leaves its norm-weight partials there and
// launch_rms_dw_finish sums them into whichever of dw_q / dw_k / dw_cq / dw_ck is not NULL; otherwise the general or the 16-byte form by key 25
extern "C" int mi355_op_rms_bwd_gather(void* stream, const void* q, const void* k, const void* dq, const void* dk, const void* dv, const float* rstd_img,
                                       const float* rstd_ctx, const float* nw_q, const float* nw_k, const float* nw_cq, const float* nw_ck, float q_scale,
                                       void* out_img, void* out_ctx, int B, int H, int S, int S_pad, int n_img, float* dw_part, float* dw_q, float* dw_k,
                                       float* dw_cq, float* dw_ck) {
    if (!q || !k || !dq || !dk || !dv) return errorf("mi355_op_rms_bwd_gather: null argument");
    if (const char* why = op_attn_split_error(B, H, S, S_pad, n_img)) return errorf("mi355_op_rms_bwd_gather: %s (S %d, S_pad %d, n_img %d)", why, S, S_pad, n_img);
    if (n_img > 0 && (!rstd_img || !nw_q || !nw_k || !out_img)) return errorf("mi355_op_rms_bwd_gather: an image-stream tensor is NULL but n_img > 0");
    if (n_img < S && (!rstd_ctx || !nw_cq || !nw_ck || !out_ctx)) return errorf("mi355_op_rms_bwd_gather: a context-stream tensor is NULL but S > n_img");
    if (!dw_part && (dw_q || dw_k || dw_cq || dw_ck)) return errorf("mi355_op_rms_bwd_gather: norm-weight gradients need dw_part");
    RmsBwdParams rb{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)dq, (const bf16_t*)dk, (const bf16_t*)dv, rstd_img, rstd_ctx, nw_q, nw_k, nw_cq, nw_ck,
                    q_scale, (bf16_t*)out_img, (bf16_t*)out_ctx, B, H, S, S_pad, n_img, dw_part};
    hipError_t err = launch_rms_bwd_gather(rb, (hipStream_t)stream);
    if (err == hipSuccess && dw_part) err = launch_rms_dw_finish(dw_part, rms_bwd_grid(B, S), q_scale, dw_q, dw_k, dw_cq, dw_ck, (hipStream_t)stream);
    if (err != hipSuccess) return errorf("mi355_op_rms_bwd_gather: %s", hipGetErrorString(err));
    return 0;
}

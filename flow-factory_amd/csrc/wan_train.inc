// mi355_flow -- Wan2.1 / Wan2.2 T2V differentiable transformer forward + native backward for the `optimize()` replay (SURVEY.md 8(f) N1 over N4;
// reference src/flow_factory/trainers/grpo.py:263, :326-330 over models/wan/wan2_t2v.py:426-543).  Textually included at the end of wan_engine.hip.
// Written at the end of round 4 on the FLUX.1 / Qwen-Image machinery (train_common.h: the training state's life cycle, the set_grad family, the
// scratch carving, t_linear_back / t_mlp_back and the attention backward; the block loop below is Wan's own program); its GPU tests (tests/test_gpu_wan_backward.py: operator level,
// three tiny shapes with and without CFG, Wan2.1-1.3B width at 4 608 tokens, an optimizer-step loop) are green on MI355X (profiles/r04u_*, r04v_*).
// Not yet measured: a full-depth (30-layer) step timing and the emitted schedule's race check (the cross-stream pattern is train_common.h's).
//
//   mi355_wan_forward_train : mi355_wan_forward's own launch sequence (forward_core) on per-block activation buffers -- same kernel binaries: the
//                             prediction is bit-identical -- keeping what the backward needs in the plan's training stash (ONE per plan);
//   mi355_wan_backward      : d loss / d v [Bp][C][T][h][w] fp32 (both CFG halves: [uncond | text], as mi355_sde_step_bwd produces it) -> fp32 (or
//                             bf16) weight gradients into the buffers registered with mi355_wan_set_grad[_typed].
// Gradient scope: weights and biases of blocks.N.{attn1.{to_q,to_k,to_v,to_out.0}, attn2.{to_q,to_k,to_v,to_out.0}, ffn.net.{0.proj,2}} -- the
// reference's Wan default target modules (wan2_t2v.py:74-85).  Norm weights, scale_shift_table, patch / time / text embedders, proj_out: never.
// A block's backward, in reverse: FFN (gated) | cross-attention (un-gated residual; queries = image tokens, keys / values = the text tokens' k / v
// of THIS block: their gradient reaches attn2.to_k / to_v through the k-norm backward, the text embedder behind them is frozen) | self-attention
// (gated; 3-D RoPE; q / k RMSNorm across ALL heads: norm_rope_full_bwd).  Attention backward = the head_dim-128 passes with a separate key length.

namespace {

struct WBlkWT { bf16_t *qkv, *o, *q2, *o2, *ff1, *ff2; };

struct WanTrainState : EngineTrain {       // per engine
    std::vector<WBlkWT> wt;
};
struct mi355_wan_train : PlanTrain {       // per plan
    std::vector<WTrainBlk> blk;
    bf16_t *x_final, *mod, *kx, *vTx, *ctx;     // this step's modulation rows, cross-attention k / v and text context (the plan's own copies may be
    float* rstd_kx;                             // overwritten by a no-grad forward -- the KL reference pass -- before the backward runs); [L][Mc]
    bf16_t *dx, *dproj, *widec;
    bf16_t *ki = nullptr, *vTi = nullptr;       // image branch: this step's image K / V^T (own copies, for the reason kx / vTx are)
    bf16_t* dq_img = nullptr;                   // head-major dq~ of the image cross-attention, added to the text cross-attention's
    int M_pad, Mc_pad;
};

}  // namespace

static WanTrainState* wan_train_state(mi355_wan* e) { return engine_train_state<WanTrainState>(e->train); }

static bool wan_trainable_name(const std::string& n) {
    static const char* ok[] = {".attn1.to_q.", ".attn1.to_k.", ".attn1.to_v.", ".attn1.to_out.0.", ".attn2.to_q.", ".attn2.to_k.", ".attn2.to_v.",
                               ".attn2.to_out.0.", ".ffn.net.0.proj.", ".ffn.net.2."};
    if (n.rfind("blocks.", 0) != 0) return false;
    for (const char* k : ok)
        if (n.find(k) != std::string::npos) return true;
    return false;
}

extern "C" int mi355_wan_set_grad(mi355_wan* e, const char* name, float* grad) {
    return t_set_grad<WanTrainState>(e, "mi355_wan", wan_trainable_name, name, grad);
}
extern "C" int mi355_wan_set_grad_typed(mi355_wan* e, const char* name, void* grad, int dtype) {
    return t_set_grad_typed<WanTrainState>(e, "mi355_wan", wan_trainable_name, name, grad, dtype);
}
extern "C" int mi355_wan_clear_grads(mi355_wan* e) { return t_clear_grads<WanTrainState>(e); }
// 0 = the native backward produces a gradient for `name`, 1 = it does not
extern "C" int mi355_wan_grad_supported(mi355_wan* e, const char* name) { return t_grad_supported(e, wan_trainable_name, name); }
extern "C" int64_t mi355_wan_plan_training_bytes(mi355_wan_plan* p) { return p && p->train ? (int64_t)p->train->ws_bytes : 0; }

// ---- transposed weights (dgrad operands) -------------------------------------------------------------------------------------------
static int wan_ensure_transposed(mi355_wan* e, hipStream_t st) {
    WanTrainState* s = wan_train_state(e);
    const int D = e->D, F = e->F, L = e->L, NO = e->NO;
    if (!s->arenaT) {
        Carver c;
        s->wt.resize(L);
        for (WBlkWT& w : s->wt) {
            c.take(w.qkv, (int64_t)D * 3 * D); c.take(w.o, (int64_t)D * D); c.take(w.q2, (int64_t)D * D); c.take(w.o2, (int64_t)D * D);
            c.take(w.ff1, (int64_t)D * F); c.take(w.ff2, (int64_t)F * D);
        }
        c.take(s->projT, (int64_t)D * NO);
        CHK(c.alloc(&s->arenaT, &s->bytes, false, "wan training", " for the transposed weights"));
        s->dirty = true;
    }
    if (!s->dirty) return 0;
    auto tr = [&](const bf16_t* w, int rows, int cols, bf16_t* out, long ld_out, int col0) { return t_transpose_weight(w, rows, cols, out, ld_out, col0, st); };
    for (int i = 0; i < L; ++i) {
        const WanBlockW& b = e->blk[i];
        WBlkWT& w = s->wt[i];
        HIPCHK(tr(b.w_qk, 2 * D, D, w.qkv, 3 * D, 0)); HIPCHK(tr(b.w_v, D, D, w.qkv, 3 * D, 2 * D));     // [3D][D] -> [D][3D]
        HIPCHK(tr(b.w_o, D, D, w.o, D, 0)); HIPCHK(tr(b.w_q2, D, D, w.q2, D, 0)); HIPCHK(tr(b.w_o2, D, D, w.o2, D, 0));
        HIPCHK(tr(b.w_ff1, F, D, w.ff1, F, 0)); HIPCHK(tr(b.w_ff2, D, F, w.ff2, D, 0));
    }
    HIPCHK(tr(e->w_proj, NO, D, s->projT, NO, 0));          // [NO][D] -> [D][NO]
    s->dirty = false;
    return 0;
}

// ---- training workspace ----------------------------------------------------------------------------------------------
static int wan_train_of(mi355_wan_plan* p, mi355_wan_train** out) {
    if (p->train) { *out = static_cast<mi355_wan_train*>(p->train); return 0; }
    mi355_wan* e = p->e;
    const int D = e->D, F = e->F, L = e->L, H = e->H, NO = e->NO;
    const int M = p->M, Mc = p->Mc;
    const int64_t qk_el = (int64_t)p->Bp * H * p->S_pad * 128, kx_el = (int64_t)p->Bp * H * p->Nt_pad * 128;
    const int64_t bhs = (int64_t)p->Bp * H * p->S_pad;
    const int64_t ki_el = (int64_t)p->Bp * H * p->Ni_pad * 128;
    mi355_wan_train* t = new mi355_wan_train();
    t->M_pad = (M + 63) / 64 * 64; t->Mc_pad = (Mc + 63) / 64 * 64;
    TrainScratch& sc = t->sc;
    Carver c;
    t->blk.resize(L);
    for (WTrainBlk& k : t->blk) {
        c.take(k.x_in, (int64_t)M * D); c.take(k.xn1, (int64_t)M * D); c.take(k.o1, (int64_t)M * D); c.take(k.x_mid1, (int64_t)M * D);
        c.take(k.xn2, (int64_t)M * D); c.take(k.o2, (int64_t)M * D); c.take(k.x_mid2, (int64_t)M * D); c.take(k.xn3, (int64_t)M * D);
        c.take(k.pre, (int64_t)M * F);
        c.take(k.q, qk_el); c.take(k.k, qk_el); c.take(k.vT, qk_el); c.take(k.q2, qk_el);
        c.take(k.lse1, bhs); c.take(k.lse2, bhs); c.take(k.rstd_q, M); c.take(k.rstd_k, M); c.take(k.rstd_q2, M);
        k.o3 = k.o23 = nullptr; k.lse3 = nullptr;
        if (p->Ni) { c.take(k.o3, (int64_t)M * D); c.take(k.o23, (int64_t)M * D); c.take(k.lse3, bhs); }
    }
    if (p->Ni) { c.take(t->ki, ki_el * L); c.take(t->vTi, ki_el * L); c.take(t->dq_img, qk_el); }
    c.take(t->x_final, (int64_t)M * D); c.take(t->mod, (int64_t)p->Bp * p->groups * p->mod_cols);
    c.take(t->kx, kx_el * L); c.take(t->vTx, kx_el * L); c.take(t->ctx, (int64_t)Mc * D); c.take(t->rstd_kx, (int64_t)L * Mc);
    c.take(t->dx, (int64_t)M * D); c.take(t->dproj, (int64_t)M * NO); c.take(t->widec, (int64_t)Mc * 2 * D);
    c.take(sc.g1, (int64_t)M * D); c.take(sc.g2, (int64_t)M * D); c.take(sc.g3, (int64_t)M * D);
    c.take(sc.wide, (int64_t)M * (3 * D + F)); c.take(sc.hid, (int64_t)M * F);
    // kv_el: the cross-attention backward puts its transposed V and its dK / dV -- stride Nt_pad * 128 per (batch, head) -- into the same v / dk /
    // dvh scratch as the self-attention: those three hold the LONGER of the two key counts, a 512-token prompt on a single small frame has
    // Nt_pad > S_pad (ADVICE r4).
    // Mmax_pad: operand slots and column-sum partials serve the text-side weight gradients too: rows = the LONGER of the two token counts -- a clip
    // shorter than its prompt overflowed slots sized by the video rows in the first GPU run of this file, profiles/r04t_wan_bwd_diag.txt.
    const int64_t kv_el = std::max(std::max(qk_el, kx_el), ki_el);
    const int Mmax_pad = t->M_pad > t->Mc_pad ? t->M_pad : t->Mc_pad;
    const int rows_T = F > 3 * D ? F : 3 * D;
    CHK(t_train_alloc(c, t, "wan training", ScratchSizes{D, F, qk_el, kv_el, bhs, rows_T, F, Mmax_pad, rows_T, 0}));
    sc.g1c = sc.g2c = sc.g3c = nullptr; sc.widec = t->widec;
    sc.tn_default = true;          // weight gradients on row-major operands (train_common.h: measured -1.9 % on the config-D step)
    p->train = t;
    *out = t;
    return 0;
}

// arguments as mi355_wan_forward; v_out [Bp][C][T][h][w] bf16 (both CFG halves)
static int wan_forward_train(mi355_wan_plan* p, void* stream, const void* latents, int lat_dtype, const float* t_in, const void* enc_a,
                             const void* enc_b, void* v_out, bool i2v, const void* condition, int cond_dtype, const void* image_embeds, bool ff = false,
                             const void* first_frame = nullptr, int ff_dtype = 0) {
    const char* who = ff ? "mi355_wan_forward_train_ff" : "mi355_wan_forward_train";      // the entry point the messages name
    if (!p || !latents || !t_in || !enc_a || !v_out) return errorf("%s: null argument", who);
    if (lat_dtype < 0 || lat_dtype > 2) return errorf("%s: bad latent dtype %d", who, lat_dtype);
    hipStream_t st = (hipStream_t)stream;
    // (image-to-video: the backward reads nothing below blocks.0 -- the patch embedder is frozen and block 0's input is stashed -- so the
    //  condition columns of the plan's patch buffer need no copy in the training stash, a deliberate difference from the image K / V^T below,
    //  which the backward does read: a later no-grad forward may overwrite the plan's patch buffer freely)
    CHK(check_kind(p, "mi355_wan_forward_train", i2v, condition, cond_dtype, image_embeds, ff, first_frame, ff_dtype));
    CHK(mi355_wan_weights_ready(p->e));
    CHK(refresh_derived(p->e, st));
    mi355_wan_train* t = nullptr;
    CHK(wan_train_of(p, &t));
    mi355_wan* e = p->e;
    const int64_t kx_el = (int64_t)p->Bp * e->H * p->Nt_pad * 128;
    HIPCHK(hipMemcpyAsync(p->t_dev, t_in, (size_t)p->Bp * p->groups * 4, hipMemcpyDeviceToDevice, st));
    CHK(write_i2v_inputs(p, st, condition, cond_dtype, image_embeds));
    p->ff = first_frame; p->ff_dt = ff_dtype;      // (first-frame plan: like the condition columns, the merged patch rows need no copy in the stash)
    CHK(prepare_prompt(p, st, enc_a, enc_b, t->rstd_kx));
    CHK(prepare_conditioning(p, st, 1));
    // this step's cross-attention k / v, text context and modulation rows: the plan's own copies may be overwritten by a no-grad forward on other
    // weights (the KL reference pass, trainers/grpo.py:281-292) between this forward and its backward
    HIPCHK(copy_d2d(t->kx, p->kx, (size_t)kx_el * e->L * 2, st));
    HIPCHK(copy_d2d(t->vTx, p->vTx, (size_t)kx_el * e->L * 2, st));
    HIPCHK(copy_d2d(t->ctx, p->ctx, (size_t)p->Mc * e->D * 2, st));
    HIPCHK(copy_d2d(t->mod, p->mod_all, (size_t)p->Bp * p->groups * p->mod_cols * 2, st));
    if (p->Ni) {
        const size_t ki_b = (size_t)p->Bp * e->H * p->Ni_pad * 128 * e->L * 2;
        HIPCHK(copy_d2d(t->ki, p->ki, ki_b, st));
        HIPCHK(copy_d2d(t->vTi, p->vTi, ki_b, st));
    }
    CHK(forward_core(p, st, latents, lat_dtype, p->mod_all, (bf16_t*)v_out, t->blk.data(), t->x_final, t->kx, t->vTx, t->ki, t->vTi));
    t->have_forward = true;
    return 0;
}

extern "C" int mi355_wan_forward_train(mi355_wan_plan* p, void* stream, const void* latents, int lat_dtype, const float* t_in, const void* enc_a,
                                       const void* enc_b, void* v_out) {
    return wan_forward_train(p, stream, latents, lat_dtype, t_in, enc_a, enc_b, v_out, false, nullptr, 0, nullptr);
}
// arguments as mi355_wan_forward_i2v; mi355_wan_backward serves both plan kinds (no gradient flows to the condition)
extern "C" int mi355_wan_forward_train_i2v(mi355_wan_plan* p, void* stream, const void* latents, int lat_dtype, const float* t_in, const void* enc_a,
                                           const void* enc_b, const void* condition, int cond_dtype, const void* image_embeds, void* v_out) {
    return wan_forward_train(p, stream, latents, lat_dtype, t_in, enc_a, enc_b, v_out, true, condition, cond_dtype, image_embeds);
}
// arguments as mi355_wan_forward_ff; mi355_wan_backward reads the plan's head_rows (the stashed modulation table holds two rows per sample)
extern "C" int mi355_wan_forward_train_ff(mi355_wan_plan* p, void* stream, const void* latents, int lat_dtype, const float* t_in, const void* enc_a,
                                          const void* enc_b, const void* first_frame, int ff_dtype, void* v_out) {
    return wan_forward_train(p, stream, latents, lat_dtype, t_in, enc_a, enc_b, v_out, false, nullptr, 0, nullptr, true, first_frame, ff_dtype);
}

// d loss / d weights from dv = d loss / d v_out [Bp][C][T][h][w] fp32 (v_out = the prediction of the LAST mi355_wan_forward_train on this plan)
extern "C" int mi355_wan_backward(mi355_wan_plan* p, void* stream, const float* dv) {
    if (!p || !dv) return errorf("mi355_wan_backward: null argument");
    if (!p->train || !p->train->have_forward) return errorf("mi355_wan_backward: no training-mode forward has run on this plan");
    mi355_wan_train* t = static_cast<mi355_wan_train*>(p->train);
    mi355_wan* e = p->e;
    hipStream_t st = (hipStream_t)stream;
    CHK(wan_ensure_transposed(e, st));
    WanTrainState* ts = wan_train_state(e);
    const int D = e->D, F = e->F, NO = e->NO, M = p->M, Mc = p->Mc, S = p->S;
    const bf16_t* mod = t->mod;
    const long mld = p->mod_cols;
    const int64_t kx_el = (int64_t)p->Bp * e->H * p->Nt_pad * 128;
    TrainScratch& sc = t->sc;
    const AttnGeom ag_self{p->Bp, e->H, D, S, p->S_pad, p->cs, nullptr, 0, 0};
    const AttnGeom ag_cross{p->Bp, e->H, D, S, p->S_pad, nullptr, nullptr, p->Nt, p->Nt_pad};
    const AttnGeom ag_img{p->Bp, e->H, D, S, p->S_pad, nullptr, nullptr, p->Ni, p->Ni_pad};
    const int64_t ki_el = (int64_t)p->Bp * e->H * p->Ni_pad * 128, qk_el = (int64_t)p->Bp * e->H * p->S_pad * 128;
    const ModRows mr{mod, mld, e->cfg.eps, p->head_rows};
    const TrainChain ch{st, M, t->M_pad, S, sc.g1, sc.g2, sc.g3, sc.wide, sc.hid, false};
    auto G = [&](int i, const char* layer) { return ts->grads.linear("blocks." + std::to_string(i) + layer); };
    auto norm_back = [&](const bf16_t* y, const bf16_t* dy, const float* w_, const float* rstd, bool rope, float scale, bf16_t* out, long ld, int col, int rows,
                         int rps, int S_pad_) -> hipError_t {
        NormRopeFullBwdParams r{y, dy, w_, rstd, rope ? p->cs : nullptr, out, ld, col, rows, e->H, rps, 0, S_pad_, scale};
        return launch_norm_rope_full_bwd(r, st);
    };
    // ---- proj_out (un-patchify transposed) and the output modulation
    HIPCHK(launch_unpatch_bwd(dv, t->dproj, p->Bp, e->cfg.out_channels, p->T * p->hp, p->wp, 2, st));
    CHK(t_dgrad(sc, st, t->dproj, NO, NO, ts->projT, M, D, sc.g3, D, nullptr, 0));
    const int mo = e->L * 6 * D;
    CHK(t_ln_back(ch, mr, D, t->x_final, sc.g3, t->dx, mo, mo + D, 0));
    for (int i = e->L - 1; i >= 0; --i) {
        const WanBlockW& b = e->blk[i];
        const WTrainBlk& k = t->blk[i];
        const WBlkWT& w = ts->wt[i];
        const int m0 = i * 6 * D;
        // ---- feed-forward (gated residual)
        CHK(t_mlp_back(sc, ch, mr, m0, D, F, t->dx, k.x_mid2, k.xn3, k.pre, w.ff1, w.ff2, G(i, ".ffn.net.0.proj"), G(i, ".ffn.net.2")));
        // ---- cross-attention (x += attn2(norm2(x), text): no gate): d (projection output) = d x
        CHK(t_linear_back(sc, ch, t->dx, D, D, p->Ni ? k.o23 : k.o2, D, D, w.o2, G(i, ".attn2.to_out.0"), sc.g2, D));
        if (p->Ni) {
            // image branch: the same dO through the image softmax first (its own o and log-sum-exp: delta is per softmax); its dK / dV have no
            // consumer (add_k_proj / add_v_proj / norm_added_k are frozen) and are overwritten by the text pass, its dq~ is kept aside
            CHK(t_attention128_backward(sc, ag_img, st, k.q2, t->ki + i * ki_el, t->vTi + i * ki_el, k.lse3, k.o3, nullptr, sc.g2, nullptr, S));
            HIPCHK(copy_d2d(t->dq_img, sc.dq, (size_t)qk_el * 2, st));
        }
        CHK(t_attention128_backward(sc, ag_cross, st, k.q2, t->kx + i * kx_el, t->vTx + i * kx_el, k.lse2, k.o2, nullptr, sc.g2, nullptr, S));
        if (p->Ni) HIPCHK(launch_add_bf16(sc.dq, t->dq_img, sc.dq, (long)qk_el, st));      // dq~ = dq~_text + dq~_img: fp32 sum, one bf16 rounding
        // queries: full-row RMSNorm backward (no RoPE) -> d (to_q output) [M][D]
        HIPCHK(norm_back(k.q2, sc.dq, b.nq2, k.rstd_q2, false, kScale, sc.wide, D, 0, M, S, p->S_pad));
        CHK(t_linear_back(sc, ch, sc.wide, D, D, k.xn2, D, D, w.q2, G(i, ".attn2.to_q"), sc.g3, D));
        CHK(t_ln_back(ch, ModRows{b.ln2_mod, 0, e->cfg.eps}, D, k.x_mid1, sc.g3, t->dx, 0, D, 1));          // norm2: LayerNorm with affine = modulation rows (bias, weight - 1)
        // keys / values: the text tokens' k (RMSNorm across heads, no RoPE) and v of THIS block -> d (to_k | to_v outputs) [Mc][2D]
        const LinGrad gk2 = G(i, ".attn2.to_k"), gv2 = G(i, ".attn2.to_v");
        if (gk2.w || gk2.b || gv2.w || gv2.b) {
            HIPCHK(norm_back(t->kx + i * kx_el, sc.dk, b.nk2, t->rstd_kx + (int64_t)i * Mc, false, 1.0f, t->widec, 2 * D, 0, Mc, p->Nt, p->Nt_pad));
            HIPCHK(norm_back(nullptr, sc.dvh, nullptr, nullptr, false, 1.0f, t->widec, 2 * D, D, Mc, p->Nt, p->Nt_pad));
            const WgradSeg sg[2] = {{0, D, gk2.w, gk2.b}, {D, D, gv2.w, gv2.b}};
            const WgradX xc{t->ctx, D, D};
            CHK(t_wgrad_group(sc, st, t->widec, 2 * D, sg, 2, &xc, 1, Mc, t->Mc_pad));
        }
        // ---- self-attention (gated residual)
        HIPCHK(launch_gate_mul(t->dx, mod + m0 + 2 * D, mld, sc.g1, M, D, S, st, p->head_rows));
        CHK(t_linear_back(sc, ch, sc.g1, D, D, k.o1, D, D, w.o, G(i, ".attn1.to_out.0"), sc.g2, D));
        CHK(t_attention128_backward(sc, ag_self, st, k.q, k.k, k.vT, k.lse1, k.o1, nullptr, sc.g2, nullptr, S));
        HIPCHK(norm_back(k.q, sc.dq, b.nq, k.rstd_q, true, kScale, sc.wide, 3 * D, 0, M, S, p->S_pad));
        HIPCHK(norm_back(k.k, sc.dk, b.nk, k.rstd_k, true, 1.0f, sc.wide, 3 * D, D, M, S, p->S_pad));
        HIPCHK(norm_back(nullptr, sc.dvh, nullptr, nullptr, false, 1.0f, sc.wide, 3 * D, 2 * D, M, S, p->S_pad));
        {
            const LinGrad gq = G(i, ".attn1.to_q"), gk = G(i, ".attn1.to_k"), gv = G(i, ".attn1.to_v");
            const WgradSeg sg[3] = {{0, D, gq.w, gq.b}, {D, D, gk.w, gk.b}, {2 * D, D, gv.w, gv.b}};
            const WgradX xi{k.xn1, D, D};
            CHK(t_wgrad_group(sc, st, sc.wide, 3 * D, sg, 3, &xi, 1, M, t->M_pad));
        }
        CHK(t_dgrad(sc, st, sc.wide, 3 * D, 3 * D, w.qkv, M, D, sc.g3, D, nullptr, 0));
        CHK(t_ln_back(ch, mr, D, k.x_in, sc.g3, t->dx, m0, m0 + D, 1));
    }
    CHK(t_wgrad_join(sc, st));
    return 0;
}

// operator-level entry point (unit test of the new kernel): forward of the full-row RMSNorm [+ RoPE] producer with its 1 / rms output, then its
// backward: src [M][ld] (column `col`), weight [H*128], cos_sin [S][64] float2 or NULL, y [B][H][S_pad][128] (written), rstd [M] (written),
// dy [B][H][S_pad][128] -> dx [M][H*128]
extern "C" int mi355_op_norm_rope_full_fwd_bwd(void* stream, const void* src, int64_t src_ld, int col, const float* weight, const float* cos_sin, void* y,
                                               float* rstd, const void* dy, void* dx, int M, int H, int rows_per_sample, int S_pad, float eps, float out_scale) {
    if (!src || !weight || !y || !rstd || !dy || !dx) return errorf("mi355_op_norm_rope_full_fwd_bwd: null argument");
    NormRopeFullParams r;
    memset(&r, 0, sizeof(r));
    r.src = (const bf16_t*)src; r.src_ld = src_ld; r.col = col; r.weight = weight; r.cs = (const float2*)cos_sin; r.out = (bf16_t*)y; r.M = M; r.H = H;
    r.rows_per_sample = rows_per_sample; r.s_off = 0; r.S_pad = S_pad; r.eps = eps; r.out_scale = out_scale; r.rstd_out = rstd;
    HIPCHK(launch_norm_rope_full(r, (hipStream_t)stream));
    NormRopeFullBwdParams b{(const bf16_t*)y, (const bf16_t*)dy, weight, rstd, (const float2*)cos_sin, (bf16_t*)dx, (long)H * 128, 0, M, H, rows_per_sample, 0, S_pad,
                            out_scale};
    HIPCHK(launch_norm_rope_full_bwd(b, (hipStream_t)stream));
    return 0;
}

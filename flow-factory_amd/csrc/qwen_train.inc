// mi355_flow -- Qwen-Image differentiable transformer forward + native backward for the `optimize()` replay (SURVEY.md 8(f) N1 over N4;
// reference src/flow_factory/trainers/grpo.py:263, :326-330 and trainers/dgpo.py:352-364 (BASELINE.json configs[4]'s trainer: the matching loss
// on `noise_pred`) over models/qwen_image/qwen_image.py:476-600).  Textually included at the end of qwen_engine.hip.
//
//   mi355_qwen_forward_train : mi355_qwen_forward's own launch sequence (forward_core, text chain on the side stream included) -- the same kernel
//                              binaries on per-block activation buffers, true-CFG
//                              combine included: the prediction is bit-identical to the no-grad forward's -- keeping what the backward needs in
//                              the plan's training stash (ONE per plan, overwritten by every call);
//   mi355_qwen_backward      : d loss / d (combined prediction) [B][Ni][C] fp32 -> fp32 weight gradients into the buffers registered with
//                              mi355_qwen_set_grad.  With n_cfg == 2 the adjoint of the norm-rescaled combine (qwen_image.py:579-587) splits it
//                              into the two branches' raw-output gradients first.
// Gradient scope: weights and biases of every linear layer inside the 60 double-stream blocks -- attn.{to_q,to_k,to_v,to_out.0,add_q_proj,
// add_k_proj,add_v_proj,to_add_out}, img_mlp.net.{0.proj,2}, txt_mlp.net.{0.proj,2}: a superset of the reference's Qwen-Image default target
// modules (qwen_image.py:81-89).  img_mod / txt_mod, norm weights, img_in / txt_in / txt_norm, the timestep MLP, norm_out and proj_out: never.
// A block's backward is the FLUX.1 double-stream block's (flux_train.inc) with the image rows FIRST in the joint sequence and ragged text keys
// (`kv_len`): the head_dim-128 attention backward masks keys >= kv_len[b] exactly like the forward.

struct QBlkWT { bf16_t *qkv, *o, *cqkv, *co, *ff1, *ff2, *cff1, *cff2; };

struct QwenTrainState {      // per engine
    char* arenaT = nullptr; size_t bytes = 0;
    std::vector<QBlkWT> wt;
    bf16_t* projT = nullptr;
    bool dirty = true;
    GradRegistry grads;
};
struct mi355_qwen_train {    // per plan
    mi355_qwen_plan* p;
    char* ws = nullptr; size_t ws_bytes = 0;
    std::vector<QTrainBlk> blk;
    bf16_t *x_final, *mod, *vraw;        // this step's modulation rows and raw network outputs (the CFG adjoint needs both branches)
    int* kvlen;                          // this step's key lengths (the plan's copy may be overwritten by a no-grad forward before the backward)
    bool have_forward = false, ragged = false;
    float guidance = 1.f;
    bf16_t *dx, *dc, *dvb;
    TrainScratch sc;
    int Mi_pad, Mc_pad;
};

static QwenTrainState* qwen_train_state(mi355_qwen* e) {      // created on first use
    if (!e->train) e->train = new QwenTrainState();
    return e->train;
}
static void qwen_train_mark_dirty(mi355_qwen* e) {
    if (e->train) e->train->dirty = true;
}
static void qwen_train_release(mi355_qwen_plan* p) {
    if (!p->train) return;
    t_wgrad_streams_destroy(p->train->sc);
    if (p->train->ws) (void)hipFree(p->train->ws);
    delete p->train;
    p->train = nullptr;
}
static void qwen_train_release_engine(mi355_qwen* e) {
    if (!e->train) return;
    if (e->train->arenaT) (void)hipFree(e->train->arenaT);
    delete e->train;
    e->train = nullptr;
}

static bool qwen_trainable_name(const std::string& n) {
    static const char* ok[] = {".attn.to_q.", ".attn.to_k.", ".attn.to_v.", ".attn.to_out.0.", ".attn.add_q_proj.", ".attn.add_k_proj.",
                               ".attn.add_v_proj.", ".attn.to_add_out.", ".img_mlp.net.0.proj.", ".img_mlp.net.2.", ".txt_mlp.net.0.proj.",
                               ".txt_mlp.net.2."};
    if (n.rfind("transformer_blocks.", 0) != 0) return false;
    for (const char* k : ok)
        if (n.find(k) != std::string::npos) return true;
    return false;
}

extern "C" int mi355_qwen_set_grad(mi355_qwen* e, const char* name, float* grad) {
    if (!e || !name) return errorf("mi355_qwen_set_grad: null argument");
    if (e->slots.find(name) == e->slots.end()) return errorf("mi355_qwen_set_grad: unknown parameter '%s'", name);
    if (grad && !qwen_trainable_name(name))
        return errorf("mi355_qwen_set_grad: '%s' lies outside the native backward's scope (the linear layers inside the transformer blocks)", name);
    qwen_train_state(e)->grads.set(name, grad);
    return 0;
}
// the same with the buffer's dtype: MI355_F32, or MI355_BF16 for the weights / biases of the linear layers inside the transformer blocks (the
// kernels that finish those gradients round their fp32 sums to bf16 on the way out: the values of `fp32 buffer -> bf16`, minus the round trip)
extern "C" int mi355_qwen_set_grad_typed(mi355_qwen* e, const char* name, void* grad, int dtype) {
    if (dtype == DT_F32 || !grad) return mi355_qwen_set_grad(e, name, (float*)grad);
    if (dtype != DT_BF16) return errorf("mi355_qwen_set_grad_typed: gradient buffers are fp32 or bf16 (dtype %d)", dtype);
    if (!e || !name) return errorf("mi355_qwen_set_grad_typed: null argument");
    if (!qwen_trainable_name(name)) return errorf("mi355_qwen_set_grad_typed: bf16 gradient buffers are limited to the linear layers inside the transformer blocks ('%s')", name);
    const int rc = mi355_qwen_set_grad(e, name, (float*)grad);
    if (rc == 0) grad_buf_mark(grad, DT_BF16);
    return rc;
}
extern "C" int mi355_qwen_clear_grads(mi355_qwen* e) {
    if (!e) return errorf("null engine");
    qwen_train_state(e)->grads.clear();
    return 0;
}
// 0 = the native backward produces a gradient for `name`, 1 = it does not
extern "C" int mi355_qwen_grad_supported(mi355_qwen* e, const char* name) {
    if (!e || !name || !e->slots.count(name)) return 1;
    return qwen_trainable_name(name) ? 0 : 1;
}
extern "C" int64_t mi355_qwen_plan_training_bytes(mi355_qwen_plan* p) {
    return p && p->train ? (int64_t)p->train->ws_bytes : 0;
}

static float* qgrad_of(mi355_qwen* e, const std::string& name) { return qwen_train_state(e)->grads.find(name); }

// ---- transposed weights -------------------------------------------------------------------------------------------
static int qwen_ensure_transposed(mi355_qwen* e, hipStream_t st) {
    QwenTrainState* s = qwen_train_state(e);
    const int D = e->D, F = e->F, L = e->L, C = e->cfg.in_channels;
    if (!s->arenaT) {
        Carver c;
        s->wt.resize(L);
        for (QBlkWT& w : s->wt) {
            c.take(w.qkv, (int64_t)D * 3 * D); c.take(w.o, (int64_t)D * D); c.take(w.cqkv, (int64_t)D * 3 * D); c.take(w.co, (int64_t)D * D);
            c.take(w.ff1, (int64_t)D * F); c.take(w.ff2, (int64_t)F * D); c.take(w.cff1, (int64_t)D * F); c.take(w.cff2, (int64_t)F * D);
        }
        c.take(s->projT, (int64_t)D * C);
        CHK(c.alloc(&s->arenaT, &s->bytes, false, "qwen training", " for the transposed weights"));
        s->dirty = true;
    }
    if (!s->dirty) return 0;
    auto tr = [&](const bf16_t* w, int rows, int cols, bf16_t* out, long ld_out, int col0) {
        return launch_transpose(w, cols, 0, out + col0, ld_out, 0, rows, cols, rows, 1, st);
    };
    for (int i = 0; i < L; ++i) {
        const QBlockW& b = e->blk[i];
        QBlkWT& w = s->wt[i];
        HIPCHK(tr(b.w_qk, 2 * D, D, w.qkv, 3 * D, 0)); HIPCHK(tr(b.w_v, D, D, w.qkv, 3 * D, 2 * D));
        HIPCHK(tr(b.w_o, D, D, w.o, D, 0));
        HIPCHK(tr(b.w_cqk, 2 * D, D, w.cqkv, 3 * D, 0)); HIPCHK(tr(b.w_cv, D, D, w.cqkv, 3 * D, 2 * D));
        HIPCHK(tr(b.w_co, D, D, w.co, D, 0));
        HIPCHK(tr(b.w_ff1, F, D, w.ff1, F, 0)); HIPCHK(tr(b.w_ff2, D, F, w.ff2, D, 0));
        HIPCHK(tr(b.w_cff1, F, D, w.cff1, F, 0)); HIPCHK(tr(b.w_cff2, D, F, w.cff2, D, 0));
    }
    HIPCHK(tr(e->w_proj, C, D, s->projT, C, 0));          // [C][D] -> [D][C]
    s->dirty = false;
    return 0;
}

// ---- training workspace ----------------------------------------------------------------------------------------------
static int qwen_train_of(mi355_qwen_plan* p, mi355_qwen_train** out) {
    if (p->train) { *out = p->train; return 0; }
    mi355_qwen* e = p->e;
    const int D = e->D, F = e->F, L = e->L, H = e->H, C = e->cfg.in_channels;
    const int Mi = p->Mi, Mc = p->Mc;
    const int64_t qk_el = (int64_t)p->FB * H * p->S_pad * 128;
    mi355_qwen_train* t = new mi355_qwen_train();
    t->p = p;
    t->Mi_pad = (Mi + 63) / 64 * 64; t->Mc_pad = (Mc + 63) / 64 * 64;
    const int Mmax = Mi > Mc ? Mi : Mc, Mmax_pad = t->Mi_pad > t->Mc_pad ? t->Mi_pad : t->Mc_pad;
    TrainScratch& sc = t->sc;
    Carver c;
    t->blk.resize(L);
    for (QTrainBlk& k : t->blk) {
        c.take(k.x_in, (int64_t)Mi * D); c.take(k.xn, (int64_t)Mi * D); c.take(k.x_mid, (int64_t)Mi * D); c.take(k.xn_mlp, (int64_t)Mi * D);
        c.take(k.pre, (int64_t)Mi * F); c.take(k.o_img, (int64_t)Mi * D);
        c.take(k.c_in, (int64_t)Mc * D); c.take(k.cn, (int64_t)Mc * D); c.take(k.c_mid, (int64_t)Mc * D); c.take(k.cn_mlp, (int64_t)Mc * D);
        c.take(k.cpre, (int64_t)Mc * F); c.take(k.o_ctx, (int64_t)Mc * D);
        c.take(k.q, qk_el); c.take(k.k, qk_el); c.take(k.vT, qk_el);
        c.take(k.lse, (int64_t)p->FB * H * p->S_pad); c.take(k.rstd_img, (int64_t)Mi * 2 * H); c.take(k.rstd_ctx, (int64_t)Mc * 2 * H);
    }
    c.take(t->x_final, (int64_t)Mi * D); c.take(t->mod, (int64_t)p->FB * e->mod_cols); c.take(t->vraw, (int64_t)p->FB * p->n_lat); c.take(t->kvlen, p->FB);
    c.take(t->dx, (int64_t)Mi * D); c.take(t->dc, (int64_t)Mc * D); c.take(t->dvb, (int64_t)Mi * C);
    c.take(sc.g1, (int64_t)Mi * D); c.take(sc.g1c, (int64_t)Mc * D); c.take(sc.g2, (int64_t)Mi * D); c.take(sc.g2c, (int64_t)Mc * D);
    c.take(sc.g3, (int64_t)Mi * D); c.take(sc.g3c, (int64_t)Mc * D);
    c.take(sc.wide, (int64_t)Mi * (3 * D + F)); c.take(sc.widec, (int64_t)Mc * (3 * D + F)); c.take(sc.hid, (int64_t)Mmax * F);
    c.take(sc.doh, qk_el); c.take(sc.v, qk_el); c.take(sc.dq, qk_el); c.take(sc.dk, qk_el); c.take(sc.dvh, qk_el);
    c.take(sc.delta, (int64_t)p->FB * H * p->S_pad); c.take(sc.nld, (int64_t)p->FB * H * p->S_pad * 2);
    const int n_slots = get_wgrad_side() ? WG_SLOTS : 1;
    for (int i = 0; i < n_slots; ++i) { c.take(sc.slot[i].aT, (int64_t)F * Mmax_pad); c.take(sc.slot[i].xT, (int64_t)F * Mmax_pad); }
    sc.part_floats = (size_t)16 * D * D > (size_t)2 * F * D ? (size_t)16 * D * D : (size_t)2 * F * D;
    const int nrt = Mmax_pad / 64 > 64 ? Mmax_pad / 64 : 64;
    c.take(sc.part, (int64_t)sc.part_floats); c.take(sc.csum, (int64_t)nrt * F); c.take(sc.zero_bias, F > 3 * D ? F : 3 * D);
    c.take(sc.hid_c, (int64_t)Mc * F); c.take(sc.csum_c, (int64_t)(t->Mc_pad / 64 > 64 ? t->Mc_pad / 64 : 64) * F);
    if (c.alloc(&t->ws, &t->ws_bytes, true, "qwen training", " of activation stash + backward scratch") != 0) { delete t; return 1; }
    sc.aT_rows = F; sc.xT_rows = F;
    if (t_wgrad_streams_init(sc, n_slots > 1) != 0) { t_wgrad_streams_destroy(sc); (void)hipFree(t->ws); delete t; return 1; }
    p->train = t;
    *out = t;
    return 0;
}

// ---- training-mode forward: forward_core (qwen_engine.hip) on the per-block stash -- two-stream like the no-grad forward --------------------
// arguments as mi355_qwen_forward
extern "C" int mi355_qwen_forward_train(mi355_qwen_plan* p, void* stream, const void* latents, int lat_dtype, const float* t_model,
                                        const void* prompt_embeds, const int32_t* txt_lens_host, float guidance_scale, void* v_out, void* v_raw) {
    if (!p || !latents || !t_model || !prompt_embeds || !v_out) return errorf("mi355_qwen_forward_train: null argument");
    if (lat_dtype < 0 || lat_dtype > 2) return errorf("mi355_qwen_forward_train: bad latent dtype %d", lat_dtype);
    CHK(mi355_qwen_weights_ready(p->e));
    hipStream_t st = (hipStream_t)stream;
    CHK(update_score_bounds(p->e, st));
    mi355_qwen_train* t = nullptr;
    CHK(qwen_train_of(p, &t));
    for (int r = 0; r < p->ncfg; ++r)
        HIPCHK(copy_d2d(p->t_dev + (size_t)r * p->B, t_model, (size_t)p->B * 4, st));
    CHK(prepare_prompt(p, st, prompt_embeds, txt_lens_host));
    p->mod_ld = p->e->mod_cols;
    CHK(prepare_conditioning(p, st, p->FB));
    CHK(forward_core(p, st, latents, lat_dtype, p->mod_all, t->blk.data(), t->x_final));
    int rc = 0;
    const bf16_t* v = combine(p, st, guidance_scale, p->v, &rc);
    CHK(rc);
    HIPCHK(copy_d2d(v_out, v, (size_t)p->B * p->n_lat * 2, st));
    if (v_raw) HIPCHK(copy_d2d(v_raw, p->v2, (size_t)p->FB * p->n_lat * 2, st));
    // what the backward needs of this step besides the block stash (the plan's own copies may be overwritten by a no-grad forward first)
    HIPCHK(copy_d2d(t->mod, p->mod_all, (size_t)p->FB * p->e->mod_cols * 2, st));
    HIPCHK(copy_d2d(t->vraw, p->v2, (size_t)p->FB * p->n_lat * 2, st));
    HIPCHK(copy_d2d(t->kvlen, p->kvlen, (size_t)p->FB * 4, st));
    t->ragged = txt_lens_host != nullptr;
    t->guidance = guidance_scale;
    t->have_forward = true;
    return 0;
}

// d loss / d weights from dv = d loss / d v_out [B][Ni][C] fp32 (v_out = the prediction of the LAST mi355_qwen_forward_train on this plan)
extern "C" int mi355_qwen_backward(mi355_qwen_plan* p, void* stream, const float* dv) {
    if (!p || !dv) return errorf("mi355_qwen_backward: null argument");
    if (!p->train || !p->train->have_forward) return errorf("mi355_qwen_backward: no training-mode forward has run on this plan");
    mi355_qwen_train* t = p->train;
    mi355_qwen* e = p->e;
    hipStream_t st = (hipStream_t)stream;
    CHK(qwen_ensure_transposed(e, st));
    QwenTrainState* ts = qwen_train_state(e);
    const int D = e->D, F = e->F, C = e->cfg.in_channels;
    const int Ni = p->Ni, Nt = p->Nt, Mi = p->Mi, Mc = p->Mc;
    const bf16_t* mod = t->mod;
    const long mld = e->mod_cols;
    TrainScratch& sc = t->sc;
    const AttnGeom ag{p->FB, e->H, D, p->S, p->S_pad, p->cs, t->ragged ? t->kvlen : nullptr};
    auto G = [&](int i, const char* leaf) { return qgrad_of(e, "transformer_blocks." + std::to_string(i) + leaf); };
    auto ln_back = [&](hipStream_t s_, const bf16_t* x, const bf16_t* dy, bf16_t* dres, int Mr, int rps, int shift_off, int scale_off,
                       int accumulate) -> hipError_t {
        LnModBwdParams l{x, dy, nullptr, dres, mod, mld, scale_off, 0, Mr, D, rps, e->cfg.eps, accumulate, nullptr, shift_off, 0};
        return launch_ln_mod_bwd(l, s_);
    };
    // ---- adjoint of the true-CFG combine (n_cfg == 2): d v_out -> d [neg | pos]; n_cfg == 1: v_out IS the network output
    if (p->ncfg == 2) HIPCHK(launch_cfg_rescale_bwd(t->vraw, t->vraw + (int64_t)p->B * p->n_lat, t->guidance, dv, t->dvb, t->dvb + (int64_t)p->B * p->n_lat,
                                                    (long)p->B * Ni, C, st));
    else HIPCHK(launch_convert(dv, DT_F32, t->dvb, DT_BF16, (long)Mi * C, st));
    // ---- proj_out and norm_out (AdaLayerNormContinuous: scale first)
    CHK(t_dgrad(sc, st, t->dvb, C, C, ts->projT, Mi, D, sc.g3, D, nullptr, 0));
    HIPCHK(ln_back(st, t->x_final, sc.g3, t->dx, Mi, Ni, e->mod_out + D, e->mod_out, 0));
    // The text chain on the plan's side stream (the one that carries it in the forward: key 12's size rule; key 28): its GEMMs have FB * n_text rows
    // (128 at B = 1 with true CFG), a fraction of a round of workgroups each.  Join before the joint attention backward (it reads the text rows'
    // dO), fork after it (the text producer backward reads dq / dk / dv).  Scratch is per chain (g?c, widec, hid_c, csum_c); the weight-gradient
    // operand slots are shared through their events.
    // (without the weight-gradient stream the two chains would share ONE operand slot and the split-K partials with no event between them:
    // found by the key-26 bit-identity test -- the text chain then stays in line)
    const bool two = get_train_text_side() != 0 && qwen_two_stream_wanted(p) && sc.wside != nullptr;
    if (two) CHK(qwen_two_stream_init(p));
    hipStream_t cs = two ? p->side : st;
    bf16_t* hid_c = two ? sc.hid_c : sc.hid;
    if (two) {          // the stash, the transposed weights and d x are complete on `st`
        HIPCHK(ev_record(p->ev_fork[e->L], st));
        HIPCHK(ev_wait(cs, p->ev_fork[e->L]));
    }
    for (int i = e->L - 1; i >= 0; --i) {
        const QBlockW& b = e->blk[i];
        const QTrainBlk& k = t->blk[i];
        const QBlkWT& w = ts->wt[i];
        const int mi = b.mod_img, mc = b.mod_ctx;
        const bool last = i + 1 == e->L;            // its text stream has no MLP and no consumer: d c starts at this block's attention
        bf16_t* dpre = sc.wide + (size_t)Mi * 3 * D;
        bf16_t* dpre_c = sc.widec + (size_t)Mc * 3 * D;
        // ---- MLP, image stream
        HIPCHK(launch_gate_mul(t->dx, mod + mi + 5 * D, mld, sc.g1, Mi, D, Ni, st));
        if (G(i, ".img_mlp.net.2.weight") || G(i, ".img_mlp.net.2.bias")) {
            if (G(i, ".img_mlp.net.2.weight")) HIPCHK(launch_gelu_fwd(k.pre, sc.hid, (long)Mi * F, st));
            CHK(t_wgrad(sc, st, sc.g1, D, 0, D, sc.hid, F, F, Mi, t->Mi_pad, G(i, ".img_mlp.net.2.weight"), G(i, ".img_mlp.net.2.bias")));
        }
        CHK(t_dgrad(sc, st, sc.g1, D, D, w.ff2, Mi, F, dpre, F, k.pre, F));
        if (G(i, ".img_mlp.net.0.proj.weight") || G(i, ".img_mlp.net.0.proj.bias"))
            CHK(t_wgrad(sc, st, dpre, F, 0, F, k.xn_mlp, D, D, Mi, t->Mi_pad, G(i, ".img_mlp.net.0.proj.weight"), G(i, ".img_mlp.net.0.proj.bias")));
        CHK(t_dgrad(sc, st, dpre, F, F, w.ff1, Mi, D, sc.g3, D, nullptr, 0));
        HIPCHK(ln_back(st, k.x_mid, sc.g3, t->dx, Mi, Ni, mi + 3 * D, mi + 4 * D, 1));
        // ---- MLP, text stream
        if (!last) {
            HIPCHK(launch_gate_mul(t->dc, mod + mc + 5 * D, mld, sc.g1c, Mc, D, Nt, cs));
            if (G(i, ".txt_mlp.net.2.weight") || G(i, ".txt_mlp.net.2.bias")) {
                if (G(i, ".txt_mlp.net.2.weight")) HIPCHK(launch_gelu_fwd(k.cpre, hid_c, (long)Mc * F, cs));
                CHK(t_wgrad(sc, cs, sc.g1c, D, 0, D, hid_c, F, F, Mc, t->Mc_pad, G(i, ".txt_mlp.net.2.weight"), G(i, ".txt_mlp.net.2.bias"), two));
            }
            CHK(t_dgrad(sc, cs, sc.g1c, D, D, w.cff2, Mc, F, dpre_c, F, k.cpre, F));
            if (G(i, ".txt_mlp.net.0.proj.weight") || G(i, ".txt_mlp.net.0.proj.bias"))
                CHK(t_wgrad(sc, cs, dpre_c, F, 0, F, k.cn_mlp, D, D, Mc, t->Mc_pad, G(i, ".txt_mlp.net.0.proj.weight"), G(i, ".txt_mlp.net.0.proj.bias"), two));
            CHK(t_dgrad(sc, cs, dpre_c, F, F, w.cff1, Mc, D, sc.g3c, D, nullptr, 0));
            HIPCHK(ln_back(cs, k.c_mid, sc.g3c, t->dc, Mc, Nt, mc + 3 * D, mc + 4 * D, 1));
        }
        // ---- joint attention: out-projections of both streams (the last block's text out-projection has no consumer: its dO is zero)
        HIPCHK(launch_gate_mul(t->dx, mod + mi + 2 * D, mld, sc.g1, Mi, D, Ni, st));
        if (G(i, ".attn.to_out.0.weight") || G(i, ".attn.to_out.0.bias"))
            CHK(t_wgrad(sc, st, sc.g1, D, 0, D, k.o_img, D, D, Mi, t->Mi_pad, G(i, ".attn.to_out.0.weight"), G(i, ".attn.to_out.0.bias")));
        CHK(t_dgrad(sc, st, sc.g1, D, D, w.o, Mi, D, sc.g2, D, nullptr, 0));
        if (!last) {
            HIPCHK(launch_gate_mul(t->dc, mod + mc + 2 * D, mld, sc.g1c, Mc, D, Nt, cs));
            if (G(i, ".attn.to_add_out.weight") || G(i, ".attn.to_add_out.bias"))
                CHK(t_wgrad(sc, cs, sc.g1c, D, 0, D, k.o_ctx, D, D, Mc, t->Mc_pad, G(i, ".attn.to_add_out.weight"), G(i, ".attn.to_add_out.bias"), two));
            CHK(t_dgrad(sc, cs, sc.g1c, D, D, w.co, Mc, D, sc.g2c, D, nullptr, 0));
            if (two) {      // join: the attention backward reads the text rows' dO (and the previous block's text chain has read dq / dk / dv)
                HIPCHK(ev_record(p->ev_join[i], cs));
                HIPCHK(ev_wait(st, p->ev_join[i]));
            }
        } else {
            // (frozen by construction: the gradient of an unused output is exactly zero; registered buffers are still overwritten)
            for (const char* leaf : {".attn.to_add_out.weight", ".attn.to_add_out.bias", ".txt_mlp.net.0.proj.weight", ".txt_mlp.net.0.proj.bias",
                                     ".txt_mlp.net.2.weight", ".txt_mlp.net.2.bias"}) {
                float* g0 = G(i, leaf);
                if (g0) HIPCHK(hipMemsetAsync(g0, 0, (size_t)e->slots[std::string("transformer_blocks.") + std::to_string(i) + leaf].numel * grad_buf_esize(g0), st));
            }
        }
        // image rows first in the joint sequence: (o_first, do_first) = image, (o_rest, do_rest) = text
        CHK(t_attention128_backward(sc, ag, st, k.q, k.k, k.vT, k.lse, k.o_img, k.o_ctx, sc.g2, last ? nullptr : sc.g2c, Ni));
        if (two) {          // fork: dq / dk / dv are written
            HIPCHK(ev_record(p->ev_fork[i], st));
            HIPCHK(ev_wait(cs, p->ev_fork[i]));
        }
        CHK(t_rope_back(sc, ag, st, k.q, k.k, k.rstd_img, b.nq, b.nk, sc.wide, 3 * D, Mi, Ni, 0));
        CHK(t_rope_back(sc, ag, cs, k.q, k.k, k.rstd_ctx, b.ncq, b.nck, sc.widec, 3 * D, Mc, Nt, Ni));
        {
            const char* nm[3] = {".attn.to_q", ".attn.to_k", ".attn.to_v"};
            const char* cn[3] = {".attn.add_q_proj", ".attn.add_k_proj", ".attn.add_v_proj"};
            WgradSeg si[3], sx[3];
            for (int j = 0; j < 3; ++j) {
                si[j] = WgradSeg{j * D, D, G(i, (std::string(nm[j]) + ".weight").c_str()), G(i, (std::string(nm[j]) + ".bias").c_str())};
                sx[j] = WgradSeg{j * D, D, G(i, (std::string(cn[j]) + ".weight").c_str()), G(i, (std::string(cn[j]) + ".bias").c_str())};
            }
            const WgradX xi{k.xn, D, D}, xc{k.cn, D, D};
            CHK(t_wgrad_group(sc, st, sc.wide, 3 * D, si, 3, &xi, 1, Mi, t->Mi_pad));
            CHK(t_wgrad_group(sc, cs, sc.widec, 3 * D, sx, 3, &xc, 1, Mc, t->Mc_pad, two));
        }
        CHK(t_dgrad(sc, st, sc.wide, 3 * D, 3 * D, w.qkv, Mi, D, sc.g3, D, nullptr, 0));
        CHK(t_dgrad(sc, cs, sc.widec, 3 * D, 3 * D, w.cqkv, Mc, D, sc.g3c, D, nullptr, 0));
        HIPCHK(ln_back(st, k.x_in, sc.g3, t->dx, Mi, Ni, mi, mi + D, 1));
        HIPCHK(ln_back(cs, k.c_in, sc.g3c, t->dc, Mc, Nt, mc, mc + D, last ? 0 : 1));
    }
    if (two) {          // the caller's stream goes on only after the text chain
        HIPCHK(ev_record(p->ev_join[e->L], cs));
        HIPCHK(ev_wait(st, p->ev_join[e->L]));
    }
    CHK(t_wgrad_join(sc, st));
    return 0;
}

extern "C" int mi355_op_cfg_rescale_bwd(void* stream, const void* v_neg, const void* v_pos, float guidance_scale, const float* d_out, void* d_neg,
                                        void* d_pos, int64_t rows, int channels) {
    if (!v_neg || !v_pos || !d_out || !d_neg || !d_pos) return errorf("mi355_op_cfg_rescale_bwd: null argument");
    HIPCHK(launch_cfg_rescale_bwd((const bf16_t*)v_neg, (const bf16_t*)v_pos, guidance_scale, d_out, (bf16_t*)d_neg, (bf16_t*)d_pos, (long)rows, channels,
                                  (hipStream_t)stream));
    return 0;
}

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
// A block's backward is train_common.h's t_double_block_back (the one FLUX.1's double blocks run) with the image rows FIRST in the joint
// sequence, ragged text keys (`kv_len`: the head_dim-128 attention backward masks keys >= kv_len[b] exactly like the forward) and a last block
// whose text output has no consumer.  The training state's life cycle, the set_grad family and the scratch carving are train_common.h's too.

namespace {

struct QwenTrainState : EngineTrain {      // per engine
    std::vector<DoubleWT> wt;
};
struct mi355_qwen_train : PlanTrain {      // per plan
    std::vector<DoubleStash> blk;
    bf16_t *x_final, *mod, *vraw;        // this step's modulation rows and raw network outputs (the CFG adjoint needs both branches)
    int* kvlen;                          // this step's key lengths (the plan's copy may be overwritten by a no-grad forward before the backward)
    bool ragged = false;
    float guidance = 1.f;
    bf16_t *dx, *dc, *dvb;
    int Mi_pad, Mc_pad;
};

}  // namespace

static QwenTrainState* qwen_train_state(mi355_qwen* e) { return engine_train_state<QwenTrainState>(e->train); }
static const DoubleBackSched kQwenDouble{true, ".img_mlp", ".txt_mlp", true};     // (the last block's text stream has no MLP and no consumer)

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
    return t_set_grad<QwenTrainState>(e, "mi355_qwen", qwen_trainable_name, name, grad);
}
// the same with the buffer's dtype: MI355_F32, or MI355_BF16 for the weights / biases of the linear layers inside the transformer blocks (the
// kernels that finish those gradients round their fp32 sums to bf16 on the way out: the values of `fp32 buffer -> bf16`, minus the round trip)
extern "C" int mi355_qwen_set_grad_typed(mi355_qwen* e, const char* name, void* grad, int dtype) {
    return t_set_grad_typed<QwenTrainState>(e, "mi355_qwen", qwen_trainable_name, name, grad, dtype);
}
extern "C" int mi355_qwen_clear_grads(mi355_qwen* e) { return t_clear_grads<QwenTrainState>(e); }
// 0 = the native backward produces a gradient for `name`, 1 = it does not
extern "C" int mi355_qwen_grad_supported(mi355_qwen* e, const char* name) { return t_grad_supported(e, qwen_trainable_name, name); }
extern "C" int64_t mi355_qwen_plan_training_bytes(mi355_qwen_plan* p) { return p && p->train ? (int64_t)p->train->ws_bytes : 0; }

// ---- transposed weights -------------------------------------------------------------------------------------------
static int qwen_ensure_transposed(mi355_qwen* e, hipStream_t st) {
    QwenTrainState* s = qwen_train_state(e);
    const int D = e->D, F = e->F, L = e->L, C = e->cfg.in_channels;
    if (!s->arenaT) {
        Carver c;
        s->wt.resize(L);
        for (DoubleWT& w : s->wt) t_double_wt_take(c, w, D, F);
        c.take(s->projT, (int64_t)D * C);
        CHK(c.alloc(&s->arenaT, &s->bytes, false, "qwen training", " for the transposed weights"));
        s->dirty = true;
    }
    if (!s->dirty) return 0;
    for (int i = 0; i < L; ++i) CHK(t_double_wt_fill(e->blk[i], s->wt[i], D, F, st));
    HIPCHK(t_transpose_weight(e->w_proj, C, D, s->projT, C, 0, st));          // [C][D] -> [D][C]
    s->dirty = false;
    return 0;
}

// ---- training workspace ----------------------------------------------------------------------------------------------
static int qwen_train_of(mi355_qwen_plan* p, mi355_qwen_train** out) {
    if (p->train) { *out = static_cast<mi355_qwen_train*>(p->train); return 0; }
    mi355_qwen* e = p->e;
    const int D = e->D, F = e->F, L = e->L, H = e->H, C = e->cfg.in_channels;
    const int Mi = p->Mi, Mc = p->Mc;
    const int64_t qk_el = (int64_t)p->FB * H * p->S_pad * 128;
    const int64_t bhs = (int64_t)p->FB * H * p->S_pad;
    mi355_qwen_train* t = new mi355_qwen_train();
    t->Mi_pad = (Mi + 63) / 64 * 64; t->Mc_pad = (Mc + 63) / 64 * 64;
    const int Mmax = Mi > Mc ? Mi : Mc, Mmax_pad = t->Mi_pad > t->Mc_pad ? t->Mi_pad : t->Mc_pad;
    TrainScratch& sc = t->sc;
    Carver c;
    t->blk.resize(L);
    for (DoubleStash& k : t->blk) t_double_stash_take(c, k, Mi, Mc, D, F, H, qk_el, bhs);
    c.take(t->x_final, (int64_t)Mi * D); c.take(t->mod, (int64_t)p->FB * e->mod_cols); c.take(t->vraw, (int64_t)p->FB * p->n_lat); c.take(t->kvlen, p->FB);
    c.take(t->dx, (int64_t)Mi * D); c.take(t->dc, (int64_t)Mc * D); c.take(t->dvb, (int64_t)Mi * C);
    c.take(sc.g1, (int64_t)Mi * D); c.take(sc.g1c, (int64_t)Mc * D); c.take(sc.g2, (int64_t)Mi * D); c.take(sc.g2c, (int64_t)Mc * D);
    c.take(sc.g3, (int64_t)Mi * D); c.take(sc.g3c, (int64_t)Mc * D);
    c.take(sc.wide, (int64_t)Mi * (3 * D + F)); c.take(sc.widec, (int64_t)Mc * (3 * D + F)); c.take(sc.hid, (int64_t)Mmax * F);
    // operand slots: both streams' weight gradients go through them (rows = the longer of the two token counts); nothing is wider than [.][F]
    CHK(t_train_alloc(c, t, "qwen training", ScratchSizes{D, F, qk_el, qk_el, bhs, F, F, Mmax_pad, F > 3 * D ? F : 3 * D, Mc}));
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
    mi355_qwen_train* t = static_cast<mi355_qwen_train*>(p->train);
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
    const ModRows mr{mod, mld, e->cfg.eps};
    const TrainChain im{st, Mi, t->Mi_pad, Ni, sc.g1, sc.g2, sc.g3, sc.wide, sc.hid, false};
    // ---- adjoint of the true-CFG combine (n_cfg == 2): d v_out -> d [neg | pos]; n_cfg == 1: v_out IS the network output
    if (p->ncfg == 2) HIPCHK(launch_cfg_rescale_bwd(t->vraw, t->vraw + (int64_t)p->B * p->n_lat, t->guidance, dv, t->dvb, t->dvb + (int64_t)p->B * p->n_lat,
                                                    (long)p->B * Ni, C, st));
    else HIPCHK(launch_convert(dv, DT_F32, t->dvb, DT_BF16, (long)Mi * C, st));
    // ---- proj_out and norm_out (AdaLayerNormContinuous: scale first)
    CHK(t_dgrad(sc, st, t->dvb, C, C, ts->projT, Mi, D, sc.g3, D, nullptr, 0));
    CHK(t_ln_back(im, mr, D, t->x_final, sc.g3, t->dx, e->mod_out + D, e->mod_out, 0));
    // The text chain on the plan's side stream (the one that carries it in the forward: key 12's size rule; key 28): its GEMMs have FB * n_text rows
    // (128 at B = 1 with true CFG), a fraction of a round of workgroups each.  Scratch is per chain (g?c, widec, hid_c, csum_c); the weight-gradient
    // operand slots are shared through their events.
    // (without the weight-gradient stream the two chains would share ONE operand slot and the split-K partials with no event between them:
    // found by the key-26 bit-identity test -- the text chain then stays in line)
    const bool two = get_train_text_side() != 0 && qwen_two_stream_wanted(p) && sc.wside != nullptr;
    if (two) CHK(qwen_two_stream_init(p));
    const TrainChain tx{two ? p->side : st, Mc, t->Mc_pad, Nt, sc.g1c, sc.g2c, sc.g3c, sc.widec, two ? sc.hid_c : sc.hid, two};
    CHK(t_double_blocks_back(sc, kQwenDouble, ag, F, mr, e->L, e->blk.data(), t->blk.data(), ts->wt.data(), ts->grads, im, tx, t->dx, t->dc,
                             p->ev_join.data(), p->ev_fork.data()));
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

// mi355_flow -- FLUX.1 differentiable transformer forward + native backward for the `optimize()` replay (SURVEY.md 8(f) N1 over N3;
// reference src/flow_factory/trainers/grpo.py:263 (`adapter.forward` WITH autograd), :326-330 (backward) over
// models/flux/flux1.py:294-346).  Textually included at the end of flux_engine.hip (shares its engine / plan structs and launch helpers).
//
//   mi355_flux_forward_train : mi355_flux_forward on flux_engine.hip's forward_core with the plan's training stash (see there);
//   mi355_flux_backward      : d loss / d weights from d loss / d v (the scheduler step's adjoint is mi355_sde_step_bwd, one op for all families).
//
// Gradient scope: weights and biases of every linear layer INSIDE the transformer blocks --
//   transformer_blocks.N.attn.{to_q,to_k,to_v,to_out.0,add_q_proj,add_k_proj,add_v_proj,to_add_out}, .ff.net.{0.proj,2}, .ff_context.net.{0.proj,2}
//   single_transformer_blocks.N.attn.{to_q,to_k,to_v}, .proj_mlp, .proj_out
// -- a superset of the reference's FLUX.1 default target modules (flux1.py:76-84: the attention projections of every block and the MLPs of the
// double blocks).  The AdaLN modulation linears, q / k norm weights, embedders, conditioning MLPs and the final proj_out are outside it
// (mi355_flux_grad_supported says so; the host refuses or routes such a configuration elsewhere).  The data gradient runs through all blocks.
//
// Backward of a single-stream block (the 38 of FLUX.1-dev), y' = y + gate * proj_out([attn(LNmod(y)) | gelu(proj_mlp(LNmod(y)))]):
//   dyg   = gate * dy'                                         gate_mul
//   dO    = dyg . W_out[:, :D]      dpre = (dyg . W_out[:, D:]) * gelu'(pre)      two dgrad GEMMs on the transposed weight (EPI_DGELU)
//   (dq~, dk, dv) = attention'(q~, k, v, o, dO, L)             attn128_bwd_prep + transpose + attention128_bwd (two passes)
//   d[q|k|v]_pre  = (RMSNorm . RoPE)'(dq~, dk) | dv            rope_rms_bwd128 -> token-major, written BESIDE dpre in one [M][3D + F] buffer
//   dyn   = [dq_pre | dk_pre | dv | dpre] . [W_q; W_k; W_v; W_mlp]     ONE dgrad GEMM with K = 3D + F = 7D
//   dy    = dy' + LNmod'(y)(dyn)                               ln_mod_bwd (accumulating in place)
// Double-stream blocks: train_common.h's t_double_block_back (the one Qwen-Image runs) with context rows first in the joint sequence.  The
// training state's life cycle, the set_grad family, the scratch carving and the per-layer backward helpers are train_common.h's too; this file
// keeps FLUX.1's own program: the name scope, the single-stream block, the head and tail of the backward.  Weight gradients: dW = dY^T . X as
// split-K GEMMs on transposed operands, bias gradients as column sums taken by the dY transpose.

namespace {

struct FSglWT { bf16_t *cat, *out; };       // [D][3D + F] = [W_q; W_k; W_v; W_mlp]^T and [D + F][D] = W_out^T

struct FluxTrainState : EngineTrain {      // per engine
    std::vector<DoubleWT> dwt;
    std::vector<FSglWT> swt;
};
struct mi355_flux_train : PlanTrain {      // per plan
    std::vector<DoubleStash> dbl;
    std::vector<FTrainSgl> sgl;
    bf16_t *x_final, *mod;
    bf16_t *dyj, *dx, *dc, *dvb;            // backward: residual-stream gradients
    int M_pad, Mi_pad, Mx_pad, Mc_pad;      // Mi: the target rows (what the final layer sees), Mx: every image-stream row
};

}  // namespace

static FluxTrainState* flux_train_state(mi355_flux* e) { return engine_train_state<FluxTrainState>(e->train); }
static const DoubleBackSched kFluxDouble{false, ".ff", ".ff_context", false};

static bool flux_trainable_name(const std::string& n) {
    static const char* dbl_ok[] = {".attn.to_q.", ".attn.to_k.", ".attn.to_v.", ".attn.to_out.0.", ".attn.add_q_proj.", ".attn.add_k_proj.",
                                   ".attn.add_v_proj.", ".attn.to_add_out.", ".ff.net.0.proj.", ".ff.net.2.", ".ff_context.net.0.proj.",
                                   ".ff_context.net.2."};
    static const char* sgl_ok[] = {".attn.to_q.", ".attn.to_k.", ".attn.to_v.", ".proj_mlp.", ".proj_out."};
    if (n.rfind("transformer_blocks.", 0) == 0) {
        for (const char* k : dbl_ok)
            if (n.find(k) != std::string::npos) return true;
        return false;
    }
    if (n.rfind("single_transformer_blocks.", 0) == 0) {
        for (const char* k : sgl_ok)
            if (n.find(k) != std::string::npos) return true;
    }
    return false;
}

// fp32 gradient buffer (same shape as the parameter, caller-owned, OVERWRITTEN by every backward); NULL un-registers
extern "C" int mi355_flux_set_grad(mi355_flux* e, const char* name, float* grad) {
    return t_set_grad<FluxTrainState>(e, "mi355_flux", flux_trainable_name, name, grad);
}
// the same with the buffer's dtype: MI355_F32, or MI355_BF16 for the weights / biases of the linear layers inside the transformer blocks (the
// kernels that finish those gradients round their fp32 sums to bf16 on the way out: the values of `fp32 buffer -> bf16`, minus the round trip)
extern "C" int mi355_flux_set_grad_typed(mi355_flux* e, const char* name, void* grad, int dtype) {
    return t_set_grad_typed<FluxTrainState>(e, "mi355_flux", flux_trainable_name, name, grad, dtype);
}
extern "C" int mi355_flux_clear_grads(mi355_flux* e) { return t_clear_grads<FluxTrainState>(e); }
// 0 = the native backward produces a gradient for `name`, 1 = it does not
extern "C" int mi355_flux_grad_supported(mi355_flux* e, const char* name) { return t_grad_supported(e, flux_trainable_name, name); }
extern "C" int64_t mi355_flux_plan_training_bytes(mi355_flux_plan* p) { return p && p->train ? (int64_t)p->train->ws_bytes : 0; }

// ---- transposed weights -------------------------------------------------------------------------------------------
static int flux_ensure_transposed(mi355_flux* e, hipStream_t st) {
    FluxTrainState* s = flux_train_state(e);
    const int D = e->D, F = e->F, L = e->L, LS = e->LS, C = e->cfg.in_channels;
    if (!s->arenaT) {
        Carver c;
        s->dwt.resize(L); s->swt.resize(LS);
        for (DoubleWT& w : s->dwt) t_double_wt_take(c, w, D, F);
        for (FSglWT& w : s->swt) { c.take(w.cat, (int64_t)D * (3 * D + F)); c.take(w.out, (int64_t)(D + F) * D); }
        c.take(s->projT, (int64_t)D * C);
        CHK(c.alloc(&s->arenaT, &s->bytes, false, "flux training", " for the transposed weights"));
        s->dirty = true;
    }
    if (!s->dirty) return 0;
    auto tr = [&](const bf16_t* w, int rows, int cols, bf16_t* out, long ld_out, int col0) { return t_transpose_weight(w, rows, cols, out, ld_out, col0, st); };
    for (int i = 0; i < L; ++i) CHK(t_double_wt_fill(e->dbl[i], s->dwt[i], D, F, st));
    for (int i = 0; i < LS; ++i) {
        const SingleW& b = e->sgl[i];
        FSglWT& w = s->swt[i];
        const long ldc = 3L * D + F;
        HIPCHK(tr(b.w_qk, 2 * D, D, w.cat, ldc, 0)); HIPCHK(tr(b.w_v, D, D, w.cat, ldc, 2 * D)); HIPCHK(tr(b.w_mlp, F, D, w.cat, ldc, 3 * D));
        HIPCHK(tr(b.w_out, D, D + F, w.out, D, 0));       // [D][D + F] -> [D + F][D]
    }
    HIPCHK(tr(e->w_proj, C, D, s->projT, C, 0));          // [C][D] -> [D][C]
    s->dirty = false;
    return 0;
}

// ---- training workspace ----------------------------------------------------------------------------------------------
static int flux_train_of(mi355_flux_plan* p, mi355_flux_train** out) {
    if (p->train) { *out = static_cast<mi355_flux_train*>(p->train); return 0; }
    mi355_flux* e = p->e;
    const int D = e->D, F = e->F, L = e->L, LS = e->LS, H = e->H, C = e->cfg.in_channels;
    const int Mi = p->Mi, Mx = p->Mx, Mc = p->Mc, M = p->M;
    const int64_t qk_el = (int64_t)p->B * H * p->S_pad * 128;
    const int64_t bhs = (int64_t)p->B * H * p->S_pad;
    mi355_flux_train* t = new mi355_flux_train();
    t->M_pad = (M + 63) / 64 * 64; t->Mi_pad = (Mi + 63) / 64 * 64; t->Mx_pad = (Mx + 63) / 64 * 64; t->Mc_pad = (Mc + 63) / 64 * 64;
    TrainScratch& sc = t->sc;
    Carver c;
    t->dbl.resize(L); t->sgl.resize(LS);
    for (DoubleStash& k : t->dbl) t_double_stash_take(c, k, Mx, Mc, D, F, H, qk_el, bhs);
    for (FTrainSgl& k : t->sgl) {
        c.take(k.y_in, (int64_t)M * D); c.take(k.yn, (int64_t)M * D); c.take(k.pre, (int64_t)M * F); c.take(k.o, (int64_t)M * D);
        c.take(k.q, qk_el); c.take(k.k, qk_el); c.take(k.vT, qk_el);
        c.take(k.lse, bhs); c.take(k.rstd, (int64_t)M * 2 * H);
    }
    c.take(t->x_final, (int64_t)Mi * D); c.take(t->mod, (int64_t)p->B * e->mod_cols);
    c.take(t->dyj, (int64_t)M * D); c.take(t->dx, (int64_t)Mx * D); c.take(t->dc, (int64_t)Mc * D);
    c.take(sc.g1, (int64_t)M * D); c.take(sc.g1c, (int64_t)Mc * D); c.take(sc.g2, (int64_t)M * D); c.take(sc.g2c, (int64_t)Mc * D);
    c.take(sc.g3, (int64_t)M * D); c.take(sc.g3c, (int64_t)Mc * D);
    c.take(sc.wide, (int64_t)M * (3 * D + F)); c.take(sc.widec, (int64_t)Mc * (3 * D + F)); c.take(sc.hid, (int64_t)M * F);
    c.take(t->dvb, (int64_t)Mi * C);
    // operand slots: the widest dY group is [M][F], the widest layer input the single blocks' [o | gelu(pre)]
    CHK(t_train_alloc(c, t, "flux training", ScratchSizes{D, F, qk_el, qk_el, bhs, F, D + F, t->M_pad, 3 * D + F, Mc}));
    p->train = t;
    *out = t;
    return 0;
}

// ---- training-mode forward: forward_core (flux_engine.hip) on the per-block stash ------------------------------------------------------
// transformer only, training mode: arguments as mi355_flux_forward; the activations the backward needs stay in the plan's training stash
// (ONE stash per plan, overwritten by every call)
static int flux_forward_train(mi355_flux_plan* p, void* stream, const void* latents, int lat_dtype, const float* t_model, const float* guidance_model,
                              const void* prompt_embeds, const void* pooled, void* v_out, bool cond_entry, const void* image_latents, int image_dtype) {
    if (!p || !latents || !t_model || !prompt_embeds || !pooled || !v_out) return errorf("mi355_flux_forward_train: null argument");
    if (p->e->cfg.guidance_embeds && !guidance_model) return errorf("mi355_flux_forward_train: this model embeds guidance, guidance_model is NULL");
    if (lat_dtype < 0 || lat_dtype > 2) return errorf("mi355_flux_forward_train: bad latent dtype %d", lat_dtype);
    CHK(check_condition("mi355_flux_forward_train", p, cond_entry, image_latents, image_dtype));
    CHK(mi355_flux_weights_ready(p->e));
    hipStream_t st = (hipStream_t)stream;
    CHK(update_score_bounds(p->e, st));
    mi355_flux_train* t = nullptr;
    CHK(flux_train_of(p, &t));
    HIPCHK(copy_d2d(p->t_dev, t_model, (size_t)p->B * 4, st));
    if (guidance_model) HIPCHK(copy_d2d(p->g_dev, guidance_model, (size_t)p->B * 4, st));
    CHK(prepare_prompt(p, st, prompt_embeds, pooled));
    CHK(prepare_conditioning(p, st, 1));
    if (cond_entry) CHK(prepare_condition(p, st, image_latents, image_dtype));
    CHK(forward_core(p, st, latents, lat_dtype, p->mod_all, (bf16_t*)v_out, t->dbl.data(), t->sgl.data(), t->x_final));
    // this step's modulation rows: the plan's own copy may be overwritten by a no-grad forward (the KL reference pass) before the backward runs
    HIPCHK(copy_d2d(t->mod, p->mod_all, (size_t)p->B * p->e->mod_cols * 2, st));
    t->have_forward = true;
    return 0;
}
extern "C" int mi355_flux_forward_train(mi355_flux_plan* p, void* stream, const void* latents, int lat_dtype, const float* t_model,
                                        const float* guidance_model, const void* prompt_embeds, const void* pooled, void* v_out) {
    return flux_forward_train(p, stream, latents, lat_dtype, t_model, guidance_model, prompt_embeds, pooled, v_out, false, nullptr, 0);
}
// FLUX.1 Kontext: mi355_flux_forward_train on a condition plan (arguments as mi355_flux_forward_cond).  No gradient flows to image_latents:
// x_embedder is outside the native gradient scope.
extern "C" int mi355_flux_forward_train_cond(mi355_flux_plan* p, void* stream, const void* latents, int lat_dtype, const float* t_model,
                                             const float* guidance_model, const void* prompt_embeds, const void* pooled, void* v_out,
                                             const void* image_latents, int image_dtype) {
    return flux_forward_train(p, stream, latents, lat_dtype, t_model, guidance_model, prompt_embeds, pooled, v_out, true, image_latents, image_dtype);
}

// ---- backward (helpers: train_common.h) ------------------------------------------------------------------------------------------
// d loss / d weights (into the buffers registered with mi355_flux_set_grad) from dv = d loss / d v_out [B][Ni][C] fp32 of the LAST
// mi355_flux_forward_train on this plan
extern "C" int mi355_flux_backward(mi355_flux_plan* p, void* stream, const float* dv) {
    if (!p || !dv) return errorf("mi355_flux_backward: null argument");
    if (!p->train || !p->train->have_forward) return errorf("mi355_flux_backward: no training-mode forward has run on this plan");
    mi355_flux_train* t = static_cast<mi355_flux_train*>(p->train);
    mi355_flux* e = p->e;
    hipStream_t st = (hipStream_t)stream;
    CHK(flux_ensure_transposed(e, st));
    FluxTrainState* ts = flux_train_state(e);
    const int D = e->D, F = e->F, C = e->cfg.in_channels;
    const int Ni = p->Ni, Nx = p->Nx, Nt = p->Nt, S = p->S, Mi = p->Mi, Mx = p->Mx, Mc = p->Mc, M = p->M;
    const bf16_t* mod = t->mod;
    const long mld = e->mod_cols;
    const size_t rowb = (size_t)D * 2;
    TrainScratch& sc = t->sc;
    const AttnGeom ag{p->B, e->H, D, S, p->S_pad, p->cs, nullptr};
    const ModRows mr{mod, mld, e->cfg.eps};
    const TrainChain joint{st, M, t->M_pad, S, sc.g1, sc.g2, sc.g3, sc.wide, sc.hid, false};
    const TrainChain im{st, Mx, t->Mx_pad, Nx, sc.g1, sc.g2, sc.g3, sc.wide, sc.hid, false};       // the image stream of the double blocks
    const TrainChain fin{st, Mi, t->Mi_pad, Ni, sc.g1, sc.g2, sc.g3, sc.wide, sc.hid, false};      // the final layer: target rows only
    auto GS = [&](int i, const char* leaf) { return ts->grads.find("single_transformer_blocks." + std::to_string(i) + leaf); };
    // ---- proj_out and norm_out (AdaLayerNormContinuous: scale first)
    HIPCHK(launch_convert(dv, DT_F32, t->dvb, DT_BF16, (long)Mi * C, st));
    CHK(t_dgrad(sc, st, t->dvb, C, C, ts->projT, Mi, D, sc.g3, D, nullptr, 0));
    CHK(t_ln_back(fin, mr, D, t->x_final, sc.g3, t->dx, e->mod_out + D, e->mod_out, 0));
    // ---- joint stream gradient: the text rows (and a condition plan's condition rows) of the last single block's output have no consumer
    HIPCHK(hipMemsetAsync(t->dyj, 0, (size_t)M * rowb, st));
    HIPCHK(hipMemcpy2DAsync(t->dyj + (size_t)Nt * D, (size_t)S * rowb, t->dx, (size_t)Ni * rowb, (size_t)Ni * rowb, p->B, hipMemcpyDeviceToDevice, st));
    const long ldw = 3L * D + F;
    for (int i = e->LS - 1; i >= 0; --i) {
        const SingleW& b = e->sgl[i];
        const FTrainSgl& k = t->sgl[i];
        const FSglWT& w = ts->swt[i];
        const int m0 = b.mod;
        HIPCHK(launch_gate_mul(t->dyj, mod + m0 + 2 * D, mld, sc.g1, M, D, S, st));
        if (GS(i, ".proj_out.weight") || GS(i, ".proj_out.bias")) {
            if (GS(i, ".proj_out.weight")) HIPCHK(launch_gelu_fwd(k.pre, sc.hid, (long)M * F, st));      // X = [o | gelu(pre)]
            const WgradSeg sg{0, D, GS(i, ".proj_out.weight"), GS(i, ".proj_out.bias")};
            const WgradX xs[2] = {{k.o, D, D}, {sc.hid, F, F}};
            CHK(t_wgrad_group(sc, st, sc.g1, D, &sg, 1, xs, 2, M, t->M_pad));
        }
        CHK(t_dgrad(sc, st, sc.g1, D, D, w.out, M, D, sc.g2, D, nullptr, 0));                                       // dO
        CHK(t_dgrad(sc, st, sc.g1, D, D, w.out + (size_t)D * D, M, F, sc.wide + 3 * D, ldw, k.pre, F));             // dpre -> columns 3D.. of `wide`
        CHK(t_attention128_backward(sc, ag, st, k.q, k.k, k.vT, k.lse, k.o, nullptr, sc.g2, nullptr, S));
        CHK(t_rope_back(sc, ag, st, k.q, k.k, k.rstd, b.nq, b.nk, sc.wide, ldw, M, S, 0));
        {
            const char* nm[4] = {".attn.to_q", ".attn.to_k", ".attn.to_v", ".proj_mlp"};
            WgradSeg sg[4];
            for (int j = 0; j < 4; ++j)
                sg[j] = WgradSeg{j * D, j < 3 ? D : F, GS(i, (std::string(nm[j]) + ".weight").c_str()), GS(i, (std::string(nm[j]) + ".bias").c_str())};
            const WgradX xy{k.yn, D, D};
            CHK(t_wgrad_group(sc, st, sc.wide, ldw, sg, 4, &xy, 1, M, t->M_pad));
        }
        CHK(t_dgrad(sc, st, sc.wide, ldw, 3 * D + F, w.cat, M, D, sc.g3, D, nullptr, 0));
        CHK(t_ln_back(joint, mr, D, k.y_in, sc.g3, t->dyj, m0, m0 + D, 1));
    }
    // ---- split the joint gradient: context rows first
    HIPCHK(hipMemcpy2DAsync(t->dc, (size_t)Nt * rowb, t->dyj, (size_t)S * rowb, (size_t)Nt * rowb, p->B, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpy2DAsync(t->dx, (size_t)Nx * rowb, t->dyj + (size_t)Nt * D, (size_t)S * rowb, (size_t)Nx * rowb, p->B, hipMemcpyDeviceToDevice, st));
    // The text chain of the double blocks on the plan's side stream (key 28; the stream and events of the forward's text chain, key 14's size
    // rule; only with the weight-gradient stream, whose events order the shared operand slots).  Per-chain scratch: g?c, widec, hid_c, csum_c.
    const bool two = get_train_text_side() != 0 && flux_two_stream_wanted(p) && sc.wside != nullptr && e->L > 0;
    if (two) CHK(flux_two_stream_init(p));
    const TrainChain tx{two ? p->side : st, Mc, t->Mc_pad, Nt, sc.g1c, sc.g2c, sc.g3c, sc.widec, two ? sc.hid_c : sc.hid, two};
    CHK(t_double_blocks_back(sc, kFluxDouble, ag, F, mr, e->L, e->dbl.data(), t->dbl.data(), ts->dwt.data(), ts->grads, im, tx, t->dx, t->dc,
                             p->ev_join.data(), p->ev_fork.data()));
    CHK(t_wgrad_join(sc, st));
    return 0;
}

// ---- operator-level entry points (unit tests of the new kernels) -----------------------------------------------------------------------
// attention forward (with log-sum-exp) + backward, head_dim 128, for both entry points below (`who`, for the messages).  Scratch is allocated
// and freed inside (test helper, synchronises).
static int op_attention128_fwd_bwd(const char* who, hipStream_t st, const void* q, const void* k, const void* vT, const void* do_first, const void* do_rest,
                                   void* o_first, void* o_rest, int64_t ld_first, int64_t ld_rest, int n_first, void* dq, void* dk, void* dv, int B, int H,
                                   int S, int S_pad, int S_kv, int S_kv_pad, const void* kv_len, float score_bound, float* lse_out, float* delta_out) {
    const int Skp = S_kv > 0 ? S_kv_pad : S_pad;
    const size_t el = (size_t)B * H * S_pad * 128, elk = (size_t)B * H * Skp * 128, bhs = (size_t)B * H * S_pad;
    char* ws = nullptr;
    const size_t bytes = (el + elk) * 2 + bhs * 4 * 4;
    HIPCHK(hipMalloc((void**)&ws, bytes));
    hipError_t err = hipMemsetAsync(ws, 0, bytes, st);       // zero padding of doh / v / lse / delta, on the caller's stream
    bf16_t* doh = (bf16_t*)ws; bf16_t* v = doh + el;
    float* lse = (float*)(v + elk); float* delta = lse + bhs; float* nld = delta + bhs;
    Attn128Params a;
    memset(&a, 0, sizeof(a));
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.vT = (const bf16_t*)vT; a.o_first = (bf16_t*)o_first; a.ld_first = ld_first; a.n_first = n_first;
    a.o_rest = (bf16_t*)o_rest; a.ld_rest = ld_rest; a.B = B; a.H = H; a.S = S; a.S_pad = S_pad; a.q_prescaled = 1; a.score_bound = score_bound;
    a.S_kv = S_kv; a.S_kv_pad = S_kv_pad; a.kv_len = (const int*)kv_len; a.lse = lse;
    if (err == hipSuccess) err = launch_attention128(a, st);
    Attn128BwdPrepParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.o_first = (const bf16_t*)o_first; pp.ld_o_first = ld_first; pp.o_rest = (const bf16_t*)o_rest; pp.ld_o_rest = ld_rest;
    pp.do_first = (const bf16_t*)do_first; pp.ld_do_first = ld_first; pp.do_rest = (const bf16_t*)do_rest; pp.ld_do_rest = ld_rest; pp.n_first = n_first;
    pp.lse = lse; pp.doh = doh; pp.delta = delta; pp.nld = nld; pp.B = B; pp.H = H; pp.S = S; pp.S_pad = S_pad;
    if (err == hipSuccess) err = launch_attn128_bwd_prep(pp, st);
    const long hs = (long)Skp * 128;
    if (err == hipSuccess) err = launch_transpose((const bf16_t*)vT, Skp, hs, v, 128, hs, 128, Skp, 128, B * H, st);
    AttnBwdParams ab{(const bf16_t*)q, (const bf16_t*)k, v, doh, lse, delta, nld, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, B, H, S, S_pad};
    ab.kv_len = (const int*)kv_len; ab.S_kv = S_kv; ab.S_kv_pad = S_kv_pad;
    if (err == hipSuccess) err = launch_attention128_bwd(ab, st);
    if (err == hipSuccess && lse_out) err = hipMemcpyAsync(lse_out, lse, bhs * 4, hipMemcpyDeviceToDevice, st);
    if (err == hipSuccess && delta_out) err = hipMemcpyAsync(delta_out, delta, bhs * 4, hipMemcpyDeviceToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    (void)hipFree(ws);
    if (err != hipSuccess) return errorf("%s: %s", who, hipGetErrorString(err));
    return 0;
}

// q (already scaled by log2(e)/sqrt(128)), k [B][H][S_pad][128], vT [B][H][128][S_pad]; d_o token-major [B*S][H*128] -> o [B*S][H*128],
// dq, dk, dv [B][H][S_pad][128].  score_bound as mi355_op_attention128 (mi355_tune_set(21, .)).
extern "C" int mi355_op_attention128_fwd_bwd(void* stream, const void* q, const void* k, const void* vT, const void* d_o, void* o, void* dq, void* dk,
                                             void* dv, int B, int H, int S, int S_pad) {
    const char* who = "mi355_op_attention128_fwd_bwd";
    if (!q || !k || !vT || !d_o || !o || !dq || !dk || !dv) return errorf("%s: null argument", who);
    return op_attention128_fwd_bwd(who, (hipStream_t)stream, q, k, vT, d_o, nullptr, o, nullptr, (int64_t)H * 128, (int64_t)H * 128, S, dq, dk, dv, B, H, S, S_pad,
                                   0, 0, nullptr, (float)get_attn128_op_bound(), nullptr, nullptr);
}

// The same with the fields the entry point above pins exposed: cross-attention and ragged keys (as mi355_op_attention128_ex; k, vT, dk, dv are then
// [B][H][S_kv_pad][128] / [B][H][128][S_kv_pad]), the first / rest split of o and dO with their row strides (Attn128BwdPrepParams; do_rest may be
// NULL: that part of the output has no consumer), the |score| bound as an argument, and optional copies of the forward's log2-sum-exp and of the
// backward's delta = rowsum(dO * O), both [B][H][S_pad] fp32 (rows >= S: zero, as the zeroed scratch holds them).
extern "C" int mi355_op_attention128_fwd_bwd_ex(void* stream, const void* q, const void* k, const void* vT, const void* do_first, const void* do_rest,
                                                void* o_first, void* o_rest, int64_t ld_first, int64_t ld_rest, int n_first, void* dq, void* dk, void* dv,
                                                int B, int H, int S, int S_pad, int S_kv, int S_kv_pad, const void* kv_len, int kv_len_n,
                                                float score_bound, float* lse_out, float* delta_out) {
    const char* who = "mi355_op_attention128_fwd_bwd_ex";
    if (!q || !k || !vT || !dq || !dk || !dv) return errorf("%s: null argument", who);
    if (attn128_ex_check(who, B, H, S, S_pad, n_first, S_kv, S_kv_pad, kv_len, kv_len_n, score_bound)) return 1;
    if (n_first > 0 && (!o_first || !do_first || ld_first < (int64_t)H * 128)) return errorf("%s: o_first / do_first is NULL or ld_first < H * 128", who);
    if (n_first < S && (!o_rest || ld_rest < (int64_t)H * 128)) return errorf("%s: o_rest is NULL or ld_rest < H * 128", who);
    return op_attention128_fwd_bwd(who, (hipStream_t)stream, q, k, vT, do_first, do_rest, o_first, o_rest, ld_first, ld_rest, n_first, dq, dk, dv, B, H, S, S_pad,
                                   S_kv, S_kv_pad, kv_len, score_bound, lse_out, delta_out);
}

// q | k producer forward (mi355_op_rope_norm + the 1/rms side output) and its backward: dq / dk / dv [B][H][S_pad][128] (dq w.r.t. the stored,
// scaled q) -> out [M][3 H 128] = [dq_pre | dk_pre | dv]; rstd [M][2H] fp32 scratch / output
extern "C" int mi355_op_rope_norm_fwd_bwd(void* stream, const void* src, int64_t src_ld, int q_col, int k_col, const float* nw_q, const float* nw_k,
                                          const float* cos_sin, void* q_out, void* k_out, float* rstd, const void* dq, const void* dk, const void* dv,
                                          void* out, int M, int H, int rows_per_sample, int s_off, int S_pad, float eps, float q_scale) {
    if (!src || !nw_q || !nw_k || !cos_sin || !q_out || !k_out || !rstd || !dq || !dk || !dv || !out) return errorf("mi355_op_rope_norm_fwd_bwd: null argument");
    RopeNormParams r;
    memset(&r, 0, sizeof(r));
    r.src = (const bf16_t*)src; r.src_ld = src_ld; r.q_col = q_col; r.k_col = k_col; r.nw_q = nw_q; r.nw_k = nw_k;
    r.cs = (const float2*)cos_sin; r.q_out = (bf16_t*)q_out; r.k_out = (bf16_t*)k_out; r.M = M; r.H = H;
    r.rows_per_sample = rows_per_sample; r.s_off = s_off; r.S_pad = S_pad; r.eps = eps; r.q_scale = q_scale; r.rstd_out = rstd;
    HIPCHK(launch_rope_norm(r, (hipStream_t)stream));
    RopeRmsBwdParams b;
    memset(&b, 0, sizeof(b));
    b.q = (const bf16_t*)q_out; b.k = (const bf16_t*)k_out; b.dq = (const bf16_t*)dq; b.dk = (const bf16_t*)dk; b.dv = (const bf16_t*)dv;
    b.rstd = rstd; b.nw_q = nw_q; b.nw_k = nw_k; b.cs = (const float2*)cos_sin; b.q_scale = q_scale; b.out = (bf16_t*)out; b.ld_out = 3L * H * 128;
    b.M = M; b.H = H; b.rows_per_sample = rows_per_sample; b.s_off = s_off; b.S_pad = S_pad;
    HIPCHK(launch_rope_rms_bwd128(b, (hipStream_t)stream));
    return 0;
}

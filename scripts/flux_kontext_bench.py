"""FLUX.1 Kontext on one MI355X at the FLUX.1-dev geometry (11.9 B parameters, synthetic weights / prompts / condition latents): the
condition-plan rollout and `optimize()` replay step at target 1024^2 with a 1024^2 condition image (Ni = Nc = 4096, Nt = 512, B = 1,
28 steps); the plain FLUX.1 rollout at 1024^2 runs in the same process on the same engine and weights (the plain `optimize()` step:
scripts/flux_train_bench.py).

    python scripts/flux_kontext_bench.py [--size 1024] [--cond-size 1024] [--denoise-steps 28] [--iters 2] [--no-train]

Fractions of peak use `flux_forward_flops(cfg, Ni + Nc, Nt)` (2 FLOP/MAC, matmuls only) against 2.5 PFLOP/s dense bf16; the step's
backward FLOPs as scripts/flux_train_bench.py counts them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flow-factory_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--cond-size", type=int, default=1024)
ap.add_argument("--n-text", type=int, default=512)
ap.add_argument("--denoise-steps", type=int, default=28)
ap.add_argument("--iters", type=int, default=2)
ap.add_argument("--layers", type=int, default=19)
ap.add_argument("--single-layers", type=int, default=38)
ap.add_argument("--no-train", action="store_true", help="rollouts only")
args = ap.parse_args()

from mi355_flow import flux  # noqa: E402
from mi355_flow.samples import Flux1Sample  # noqa: E402
from mi355_flow.scheduler import FlowMatchEulerDiscreteSDEScheduler, set_scheduler_timesteps  # noqa: E402
from mi355_flow.weights import flux_forward_flops, module_from_state_dict, synthetic_flux_state_dict  # noqa: E402

dev = torch.device("cuda")
cfg = flux.FluxConfig(num_layers=args.layers, num_single_layers=args.single_layers)
mod = module_from_state_dict(synthetic_flux_state_dict(cfg, device=dev), buffers=())
DEFAULT = ("attn.to_k.", "attn.to_q.", "attn.to_v.", "attn.to_out.0.", "attn.add_k_proj.", "attn.add_q_proj.", "attn.add_v_proj.", "attn.to_add_out.",
           "ff.net.0.proj.", "ff.net.2.", "ff_context.net.0.proj.", "ff_context.net.2.")
for n, p in mod.named_parameters():
    p.requires_grad_(any(k in n for k in DEFAULT))
sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, dynamics_type="Flow-SDE", shift=3.0,
                                           use_dynamic_shifting=True)
ad = flux.Flux1KontextNativeAdapter(mod, cfg, sched, latent_storage_dtype="fp16")
ad.rollout()
B, Nt, N = args.batch, args.n_text, args.denoise_steps
h = w = args.size // 8
hc = wc = args.cond_size // 8
Ni, Nc = (h // 2) * (w // 2), (hc // 2) * (wc // 2)
g = torch.Generator(device=dev).manual_seed(1)
mk = lambda *s: torch.randn(*s, device=dev, generator=g)
pe, pp = mk(B, Nt, cfg.joint_attention_dim).bfloat16(), mk(B, cfg.pooled_projection_dim).bfloat16()
il = mk(B, Nc, 64).bfloat16()
image_ids = flux.prepare_latent_image_ids(hc // 2, wc // 2, dev, torch.bfloat16)
image_ids[:, 0] = 1
latent_ids = torch.cat([flux.prepare_latent_image_ids(h // 2, w // 2, dev, torch.bfloat16), image_ids])


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    fn()                                    # (the second rollout of a configuration captures its graph)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


common = dict(prompt=None, height=args.size, width=args.size, num_inference_steps=N, guidance_scale=3.5, prompt_embeds=pe, pooled_prompt_embeds=pp,
              compute_log_prob=True, trajectory_indices="all")
t_cond = timed(lambda: ad.inference(**common, image_latents=il, image_ids=image_ids), args.iters)
ad._sample_cls = Flux1Sample            # the plain FLUX.1 rollout on the same engine and weights returns the plain sample class
t_plain = timed(lambda: flux.FluxRolloutMixin.inference(ad, **common), args.iters)
ad._sample_cls = flux.Flux1KontextSample
F_cond, F_plain = flux_forward_flops(cfg, Ni + Nc, Nt), flux_forward_flops(cfg, Ni, Nt)
out = {"what": "FLUX.1 Kontext rollout, FLUX.1 geometry, synthetic weights", "layers": [cfg.num_layers, cfg.num_single_layers], "batch": B,
       "size": args.size, "cond_size": args.cond_size, "tokens": {"Ni": Ni, "Nc": Nc, "Nt": Nt, "S": Nt + Ni + Nc}, "denoise_steps": N,
       "kontext": {"s_per_rollout": round(t_cond, 3), "denoise_steps_per_s": round(B * N / t_cond, 2),
                   "forward_tflops": round(F_cond * B * N / t_cond / 1e12, 1), "frac_of_2.5PF": round(F_cond * B * N / t_cond / 2.5e15, 4)},
       "plain_flux1_same_process": {"s_per_rollout": round(t_plain, 3), "denoise_steps_per_s": round(B * N / t_plain, 2),
                                    "forward_tflops": round(F_plain * B * N / t_plain / 1e12, 1),
                                    "frac_of_2.5PF": round(F_plain * B * N / t_plain / 2.5e15, 4)},
       "workspace_gib": round(ad.engine.plan(B, h, w, Nt, N, cond=(hc, wc)).workspace_bytes / 2 ** 30, 2)}
print(json.dumps(out), flush=True)
if args.no_train:
    sys.exit(0)

ts = set_scheduler_timesteps(sched, 28, seq_len=Ni, device=dev)      # dynamic shifting: mu from the target's Ni
step = dict(t=ts[2].expand(B), t_next=ts[3].expand(B), latents=mk(B, Ni, 64).half(), next_latents=mk(B, Ni, 64).half(), prompt_embeds=pe,
            pooled_prompt_embeds=pp, guidance_scale=3.5, noise_level=0.7, compute_log_prob=True, return_kwargs=["log_prob", "dt"])


def fwd_bwd():
    ad.forward(**step, image_latents=il, latent_ids=latent_ids).log_prob.sum().backward()
    for p in mod.parameters():
        p.grad = None


def step_flops(S):
    D, L, LS = cfg.dim, cfg.num_layers, cfg.num_single_layers
    lin = (L + LS) * S * 12 * D * D
    attn = (L + LS) * 2 * S * S * D
    lin_train = L * S * 12 * D * D + LS * S * 3 * D * D
    return 2.0 * (lin + attn) * B + 2.0 * (lin + 2.5 * attn + lin_train) * B


with torch.no_grad():
    lp0 = ad.forward(**step, image_latents=il, latent_ids=latent_ids).log_prob
t_fb = timed(fwd_bwd, args.iters)
lp1 = ad.forward(**step, image_latents=il, latent_ids=latent_ids).log_prob.detach()
S = Nt + Ni + Nc
plan = ad.engine.plan(B, h, w, Nt, 1, cond=(hc, wc))
print(json.dumps({"what": "FLUX.1 Kontext GRPO optimize() replay step, default target modules", "tokens": S, "ms_forward_backward": round(t_fb * 1e3, 2),
                  "tflops_step": round(step_flops(S) / t_fb / 1e12, 1), "frac_of_2500": round(step_flops(S) / t_fb / 2.5e15, 4),
                  "ratio_is_one": bool(torch.equal(lp0, lp1)), "stash_plus_scratch_GiB": round(plan.training_bytes / 2 ** 30, 2)}), flush=True)

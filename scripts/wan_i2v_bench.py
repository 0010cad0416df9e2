"""Wan image-to-video against plain text-to-video on one MI355X, in ONE process, three legs: `t2v`; `i2v` = the condition channels only
(Wan2.2-I2V-A14B's transformer input, `cat([latents, condition], 1)` into a 36-channel patch embedding); `i2v_img` = the same plus the image
cross-attention branch of Wan2.1-I2V with 257 CLIP tokens of width 1280.  The 1.3B-width synthetic geometry (30 blocks, D = 1536) at
480 x 832 x 49 frames (20 280 tokens), B = 1 with CFG.  Per leg: the fused rollout (denoise-steps/s) and the `optimize()` replay step on the
reference's default target modules (forward + backward ms).  The legs alternate `--rounds` times so that a drift of the clock shows as spread.

    python scripts/wan_i2v_bench.py [--denoise-steps 4] [--rounds 3] [--layers 30] [--no-train]

`--leg t2v|i2v|i2v_img --only-step`: 1 + iters training steps of one leg and nothing else (for a `rocprofv3 --kernel-trace --stats` run)."""
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
ap.add_argument("--frames", type=int, default=49)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=832)
ap.add_argument("--n-text", type=int, default=512)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--denoise-steps", type=int, default=4)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=1)
ap.add_argument("--layers", type=int, default=30)
ap.add_argument("--leg", choices=["all", "t2v", "i2v", "i2v_img"], default="all")
ap.add_argument("--no-train", action="store_true", help="rollouts only")
ap.add_argument("--only-step", action="store_true")
args = ap.parse_args()

from mi355_flow import wan  # noqa: E402
from mi355_flow.weights import module_from_state_dict, synthetic_wan_state_dict  # noqa: E402

dev = torch.device("cuda")
DEFAULT = (".attn1.to_q.", ".attn1.to_k.", ".attn1.to_v.", ".attn1.to_out.0.", ".attn2.to_q.", ".attn2.to_k.", ".attn2.to_v.", ".attn2.to_out.0.",
           ".ffn.net.0.proj.", ".ffn.net.2.")
B, Nt, N = args.batch, args.n_text, args.denoise_steps
T, h, w = (args.frames - 1) // 4 + 1, args.height // 8, args.width // 8
g = torch.Generator(device=dev).manual_seed(1)
mk = lambda *s: torch.randn(*s, device=dev, generator=g)      # noqa: E731
pe, ne = mk(B, Nt, 4096).bfloat16(), mk(B, Nt, 4096).bfloat16()
cond = torch.cat([torch.zeros(B, 4, T, h, w, device=dev), mk(B, 16, T, h, w)], 1)
cond[:, :4, 0] = 1.0
image_embeds = mk(B, 257, 1280).bfloat16()
x0, x1 = mk(B, 16, T, h, w).half(), mk(B, 16, T, h, w).half()


def make(kind):
    cfg = wan.WanConfig(num_layers=args.layers, cond_channels=0 if kind == "t2v" else 20, image_dim=1280 if kind == "i2v_img" else None)
    mod = module_from_state_dict(synthetic_wan_state_dict(cfg, device=dev), buffers=())
    for n, p in mod.named_parameters():
        p.requires_grad_(any(k in n for k in DEFAULT))
    sched = wan.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, dynamics_type="Flow-SDE")
    ad = (wan.Wan2T2VNativeAdapter if kind == "t2v" else wan.Wan2I2VNativeAdapter)(mod, cfg, sched, latent_storage_dtype="fp16")
    ad.rollout()
    extra = {} if kind == "t2v" else dict(condition=cond, **(dict(image_embeds=image_embeds) if kind == "i2v_img" else {}))
    roll = lambda: ad.inference(prompt=None, height=args.height, width=args.width, num_frames=args.frames, num_inference_steps=N,      # noqa: E731
                                guidance_scale=args.guidance, prompt_embeds=pe, negative_prompt_embeds=ne, compute_log_prob=True,
                                trajectory_indices="all", **extra)
    sched.set_timesteps(28)
    ts = sched.timesteps
    kw = dict(t=ts[2].float().expand(B), t_next=ts[3].float().expand(B), latents=x0, next_latents=x1, prompt_embeds=pe, negative_prompt_embeds=ne,
              guidance_scale=args.guidance, noise_level=0.7, compute_log_prob=True, return_kwargs=["log_prob", "dt"], **extra)

    def step():
        ad.forward(**kw).log_prob.sum().backward()
        for p in mod.parameters():
            p.grad = None

    return ad, roll, step


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


kinds = ["t2v", "i2v", "i2v_img"] if args.leg == "all" else [args.leg]
legs = {k: make(k) for k in kinds}
if args.only_step:
    _, _, step = legs[kinds[0]]
    step()
    print(json.dumps({"leg": kinds[0], "ms_forward_backward": round(timed(step, args.iters) * 1e3, 2), "steps_profiled": args.iters + 1}))
    sys.exit(0)
res = {k: {"denoise_steps_per_s": [], "ms_train_step": []} for k in kinds}
for k in kinds:                                     # warm-up: plans, training stash, transposed weights
    legs[k][1]()
    if not args.no_train:
        legs[k][2]()
for _ in range(args.rounds):
    for k in kinds:
        res[k]["denoise_steps_per_s"].append(round(B * N / timed(legs[k][1], args.iters), 4))
        if not args.no_train:
            res[k]["ms_train_step"].append(round(timed(legs[k][2], args.iters) * 1e3, 2))
med = lambda v: sorted(v)[len(v) // 2] if v else None      # noqa: E731
out = {"what": "Wan T2V vs I2V (condition channels) vs I2V with 257 image tokens, 1.3B-width synthetic geometry", "layers": args.layers, "batch": B, "n_cfg": 2 if args.guidance > 1 else 1,
       "clip": [args.frames, args.height, args.width], "tokens": T * (h // 2) * (w // 2), "denoise_steps": N, "runs": res,
       "median": {k: {m: med(v) for m, v in res[k].items()} for k in kinds}}
if "t2v" in kinds:
    a = out["median"]["t2v"]
    for k in kinds[1:]:
        b = out["median"][k]
        out[k + "_over_t2v"] = {"denoise_steps_per_s": round(b["denoise_steps_per_s"] / a["denoise_steps_per_s"], 4),
                                "ms_train_step": round(b["ms_train_step"] / a["ms_train_step"], 4) if a["ms_train_step"] else None}
print(json.dumps(out), flush=True)

"""Cost of the two-group modulation: the first-frame rollout of Wan2.2-TI2V-5B in image-to-video use against the text-to-video rollout of the
SAME build, weights and shape, alternating in ONE process.  TI2V-5B geometry (30 blocks, D = 3072, 24 heads, ffn 14336, 48 latent channels, drawn
weights) at 480 x 832 x 49 frames = a 13 x 30 x 52 latent grid = 5 070 tokens of which 390 are frame 0, B = 1 with CFG.  The extra work of the
`ff` leg is one frame's patch merge per step and twice the conditioning rows; its ln_mod / gated-residual launches run the split instantiations.

    python scripts/wan_ti2v_ab.py [--denoise-steps 8] [--rounds 3] [--layers 30]

Prints one JSON line: denoise-steps/s per leg and round, the medians, `ff_over_t2v` and the run-to-run spread of the T2V leg.
`--leg t2v|ff --only-rollout`: 1 + iters rollouts of one leg and nothing else (for a `rocprofv3 --kernel-trace --stats` run)."""
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
ap.add_argument("--denoise-steps", type=int, default=8)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=1)
ap.add_argument("--layers", type=int, default=30)
ap.add_argument("--leg", choices=["all", "t2v", "ff"], default="all")
ap.add_argument("--only-rollout", action="store_true")
args = ap.parse_args()

from mi355_flow import wan  # noqa: E402
from mi355_flow.weights import synthetic_wan_state_dict  # noqa: E402

dev = torch.device("cuda")
B, Nt, N = args.batch, args.n_text, args.denoise_steps
T, h, w = (args.frames - 1) // 4 + 1, args.height // 16, args.width // 16          # the TI2V VAE compresses 4 x 16 x 16
g = torch.Generator(device=dev).manual_seed(1)
mk = lambda *s: torch.randn(*s, device=dev, generator=g)      # noqa: E731
pe, ne = mk(B, Nt, 4096).bfloat16(), mk(B, Nt, 4096).bfloat16()
first_frame = mk(B, 48, 1, h, w)

cfg = wan.WanConfig(in_channels=48, out_channels=48, num_layers=args.layers, num_attention_heads=24, ffn_dim=14336)
sd = synthetic_wan_state_dict(cfg, device=dev)


def make(kind):
    sched = wan.UniPCMultistepSDEScheduler(flow_shift=3.0, noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, dynamics_type="Flow-SDE")
    ad = (wan.Wan2T2VNativeAdapter if kind == "t2v" else wan.Wan2TI2VNativeAdapter)(sd, cfg, sched, latent_storage_dtype="fp16")
    ad.vae_scale_spatial = 16
    ad.rollout()
    extra = {} if kind == "t2v" else dict(condition=first_frame)
    return lambda: ad.inference(prompt=None, height=args.height, width=args.width, num_frames=args.frames, num_inference_steps=N,
                                guidance_scale=args.guidance, prompt_embeds=pe, negative_prompt_embeds=ne, compute_log_prob=True,
                                trajectory_indices="all", **extra)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


kinds = ["t2v", "ff"] if args.leg == "all" else [args.leg]
legs = {k: make(k) for k in kinds}
for k in kinds:                                     # warm-up: plans
    legs[k]()
if args.only_rollout:
    print(json.dumps({"leg": kinds[0], "denoise_steps_per_s": round(B * N / timed(legs[kinds[0]], args.iters), 4), "rollouts_profiled": args.iters + 1}))
    sys.exit(0)
res = {k: [] for k in kinds}
for _ in range(args.rounds):
    for k in kinds:
        res[k].append(round(B * N / timed(legs[k], args.iters), 4))
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
out = {"what": "Wan2.2-TI2V-5B geometry: first-frame rollout (two-group modulation) vs text-to-video rollout, same build and shape",
       "layers": args.layers, "batch": B, "n_cfg": 2 if args.guidance > 1 else 1, "clip": [args.frames, args.height, args.width],
       "tokens": T * (h // 2) * (w // 2), "head_tokens": (h // 2) * (w // 2), "denoise_steps": N, "denoise_steps_per_s": res,
       "median": {k: med(v) for k, v in res.items()}}
if len(kinds) == 2:
    out["ff_over_t2v"] = round(out["median"]["ff"] / out["median"]["t2v"], 4)
    out["t2v_spread"] = round((max(res["t2v"]) - min(res["t2v"])) / out["median"]["t2v"], 4)
print(json.dumps(out), flush=True)

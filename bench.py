#!/usr/bin/env python
"""bench.py -- denoise-steps/sec of the SD3.5-medium 1024^2 GRPO rollout on MI355X.

    python bench.py --gpus N --steps K --warmup W      (N > 1: re-executes itself under torch.distributed.run, one rank per GPU;
                                                        when already launched that way -- RANK / WORLD_SIZE set -- it just runs its rank)

One bench "step" = ONE rollout micro-batch through the drop-in API (`SD3_5NativeAdapter.inference`):
`--batch` samples x 28 SDE/ODE denoise steps at 1024x1024 (latents 16x128x128, 4096 image + 333 text
tokens), RNG draws + collectors + sample building included, VAE decode / rewards excluded
(SURVEY.md 8(d)).  value = samples x 28 x K x N / wall-time  [denoise-steps/sec, whole job].
Synthetic prompts (random prompt embeddings) and random-init weights of the SD3.5-medium
architecture: no checkpoints / datasets exist in this environment.

A plain run does what the headline figure needs and nothing else: set-up, the warm-up steps, the timed steps, `--dump-outputs`, the line.
Rank 0 prints ONE JSON line; besides the contract keys it carries
  roofline     : the dominant kernel (attention, v_mfma_f32_32x32x16_bf16) -- algorithmic FLOPs per
                 launch / mean launch duration from hipEvents recorded on the launch stream over the
                 timed region, vs the 2.5 PFLOP/s dense bf16 MFMA peak; plus the whole-forward figure
                 the north star asks for (`forward.frac`, target 0.40) and a per-class breakdown.

`--full` adds everything else this file measures or checks (each leg keeps its own `--no-...` switch): the kernel-variant cross-check of
one rollout before the timed steps and, after them, the roofline figures that take rollouts of their own (`attention_dynamic`,
`guaranteed_floor`, `gemm`, `delivered_clock_mhz`), `power`, `graph_vs_eager`, `small_batch`, `vae_decode`, the `optimize_step*` and
`families` subprocess legs, `optimize_step_ddp` (N > 1) and
  cpu_baseline : the oracle (fp32 PyTorch restatement of the reference path) timed on the host
                 cores on a bounded sample; a reported baseline, not the optimisation target.

`--dump-outputs DIR` writes the samples of the last timed step as DIR/<field>.npy (`dump_outputs`), for comparing two builds on the same inputs.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "flow-factory_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (MI355X_MICROARCH.md; AMD's 5 PF figure is 2:1 sparse)
N_TEXT = 333               # 77 CLIP + 256 T5 tokens


def forward_flops(cfg, Ni, Nt):
    """algorithmic matmul FLOPs per transformer forward per sample (2 FLOP/MAC)."""
    D, F, L, Ld = cfg.dim, cfg.ff_mult * cfg.dim, cfg.num_layers, len(cfg.dual_layers)
    mac = (L * Ni * (4 * D * D + 2 * D * F) + ((L - 1) * Nt * (4 * D * D + 2 * D * F) + Nt * 3 * D * D)
           + Ld * Ni * 4 * D * D + L * 2 * (Ni + Nt) ** 2 * D + Ld * 2 * Ni * Ni * D
           + Nt * cfg.joint_attention_dim * D + 2 * Ni * cfg.patch_size ** 2 * cfg.in_channels * D)
    return 2.0 * mac


def attention_flops(cfg, Ni, Nt):
    L, Ld, D = cfg.num_layers, len(cfg.dual_layers), cfg.dim
    return 2.0 * (L * 2 * (Ni + Nt) ** 2 * D + Ld * 2 * Ni * Ni * D), L + Ld  # flops / forward / sample, launches


def _stream_mode_at_start():
    """mi355_tune_set key 8 (stream mode of the SD3.5 forward) as THIS process was started: MI355_TUNE's entry, else the library default 2.
    The per-class legs switch to single stream for their own measurement and must hand back what the run asked for -- a run under
    MI355_TUNE="8=0" (the single-stream rocprof table) stays single-stream."""
    for kv in filter(None, os.environ.get("MI355_TUNE", "").split(",")):
        k, _, v = kv.partition("=")
        if k.strip() == "8":
            return int(v)
    return 2


def cpu_baseline(budget_s=150.0):
    """Oracle on the host cores: ONE measured fp32 MMDiT-X forward (= one denoise step, n_cfg = 1) of one sample at the bench
    shape (1024^2: 4096 + 333 tokens, 11.25 TFLOP).  A 256^2 forward is timed first; only if its FLOP-scaled estimate exceeds
    `budget_s` is the 1024^2 figure extrapolated (and labelled so) instead of measured."""
    from oracle import mmditx_ref as M
    cfg = M.SD35_MEDIUM
    cores = torch.get_num_threads()      # torch's default = the physical cores (one thread per SMT sibling is 40x SLOWER here: measured)
    # timing only: draw the 2.5 B fp32 weights on the GPU and copy them down (the CPU generator needs ~1 min)
    from mi355_flow.engine import TransformerConfig
    from mi355_flow.weights import synthetic_state_dict
    sd = {k: v.float().cpu() for k, v in synthetic_state_dict(TransformerConfig(), device="cuda", dtype=torch.float32).items()}
    g = torch.Generator().manual_seed(4321)
    enc = torch.randn(1, N_TEXT, 4096, generator=g)
    pooled = torch.randn(1, 2048, generator=g)
    t = torch.tensor([900.0])

    def run(hw):
        x = torch.randn(1, 16, hw, hw, generator=g)
        t0 = time.perf_counter()
        with torch.no_grad():
            M.mmdit_forward(sd, cfg, x, t, enc, pooled)
        return time.perf_counter() - t0

    run(32)  # warm the thread pool / allocator
    t256 = min(run(32), run(32))         # (one probe of the final round-4 evidence run took 14.9 s against the usual 5.6 s: a transient)
    f256, f1024 = M.forward_flops(cfg, 256, N_TEXT), M.forward_flops(cfg, 4096, N_TEXT)
    # the 256^2 forward is bound by streaming the 10 GB of fp32 weights, not by FLOPs: the measured 1024^2 / 256^2 time ratio is 4.3 ... 4.8
    # (24.0 / 5.70 s, 27.1 / 5.60 s on two boxes) against a FLOP ratio of 12.4 -- predict with 5.5, keep the FLOP ratio as the ceiling
    est = t256 * min(f1024 / f256, 5.5)
    if est <= budget_s:
        t1024 = run(128)
        return dict(value=round(1.0 / t1024, 5), unit="denoise-steps/sec", cores=cores, kind="port", measured=True,
                    sample=f"1 fp32 oracle forward (= 1 denoise step, n_cfg=1) of 1 sample at 1024^2: {t1024:.2f} s MEASURED on {cores} threads "
                           f"({f1024 / t1024 / 1e12:.2f} TFLOP/s); 256^2 forward {t256:.2f} s")
    return dict(value=round(1.0 / est, 5), unit="denoise-steps/sec", cores=cores, kind="port", measured=False,
                sample=f"1 fp32 oracle forward at 256^2 ({t256:.2f} s measured) EXTRAPOLATED x5.5 (measured time ratio 4.3-4.8) to 1024^2 "
                       f"(estimate {est:.0f} s > budget {budget_s:.0f} s)")


def skip_rollout_draws(adapter, batch, size, n_steps, device):
    """Advance the device's global generator by what one `inference()` call draws from it, without running the rollout: the initial
    latents in the transformer dtype, then one fp32 tensor per denoise step (none under ODE dynamics) -- `NativeRolloutMixin.inference`."""
    shape = (batch, adapter.engine.cfg.in_channels, size // 8, size // 8)
    torch.randn(shape, device=device, dtype=adapter.transformer_dtype)
    if adapter.scheduler.dynamics_type != "ODE":
        for _ in range(n_steps):
            torch.randn(shape, device=device, dtype=torch.float32)


DUMP_BUDGET_BYTES = 64 * 10**6   # `--dump-outputs` writes at most this much in all
DUMP_FIELDS = ("timesteps", "all_latents", "latent_index_map", "log_probs", "log_prob_index_map", "image")


def dump_outputs(out_dir, samples):
    """`--dump-outputs`: what `inference()` returned in the last timed step, as `<out_dir>/<field>.npy` (float32, batch first) -- the fields a
    rollout produces, not the prompt embeddings handed in.  The weights, the prompts and the RNG seeds are fixed, so two builds run with
    the same arguments can be compared file by file.  The budget goes to the smallest arrays first; one that does not fit into an even share
    of what is left is written as a sample of its flattened elements at fixed seeded positions (the same positions for the same shape)."""
    import numpy as np
    stacked = type(samples[0]).stack(samples)
    arrays = {k: stacked[k].detach().float().cpu().numpy() for k in DUMP_FIELDS if isinstance(stacked.get(k), torch.Tensor)}
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_BUDGET_BYTES
    for n, (name, a) in enumerate(sorted(arrays.items(), key=lambda kv: kv[1].size)):
        share = (left // (len(arrays) - n) - 1024) // 4    # float32 elements, the .npy header left room for
        if a.size > share:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).integers(0, a.size, share))]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.nbytes + 1024


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` typed by hand: re-execute under torch.distributed.run (one rank per GPU, RCCL rendezvous on
    127.0.0.1) with the same arguments; the ranks see RANK / WORLD_SIZE and take the normal path."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


DDP_LEG_DEADLINE_S = 420      # wall-clock budget of the optional `optimize_step_ddp` leg (normally ~30 s) before the headline line goes out without it


def ddp_optimize_leg(ddp, microstep, params, world, rank, device, iters=3, backend="nccl (RCCL)"):
    """The policy-update collective of the north star, measured (world > 1 only): one `optimize()` micro-step -- grad-mode replay forward +
    backward -- under `DistributedDataParallel` (reference: the trainable component is DDP-wrapped by `accelerator.prepare`,
    trainers/loader.py:33, and the loss goes through `accelerator.backward`, trainers/grpo.py:326-330), timed twice per rank:
    synchronising (the reducer all-reduces every bucket on the process group while the backward still produces the later gradients) and
    inside `no_sync()` (the same backward, no collective).  Their difference is the all-reduce time the backward does NOT hide.  MAX over
    ranks for both; the bytes are what one micro-step hands to the collective.  Every rank runs this; rank 0 gets the dict."""
    import contextlib

    def timed(ctx):
        with ctx():
            microstep()                                   # warm-up (first synchronising step also builds the buckets)
        if device is not None:
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(iters):
            with ctx():
                microstep()
        if device is not None:
            torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
        for q in params:
            q.grad = None
        return dt
    t_sync = timed(contextlib.nullcontext)
    t_sync = timed(contextlib.nullcontext)                # (second pass: on the rebuilt, gradient-ready-ordered buckets)
    t_nosync = timed(ddp.no_sync)
    both = torch.tensor([t_sync, t_nosync], dtype=torch.float64, device=device if device is not None else "cpu")
    allb = [torch.zeros_like(both) for _ in range(world)]
    if world > 1:
        dist.all_gather(allb, both)
    else:
        allb = [both]
    per_rank = [[float(v) for v in b.tolist()] for b in allb]
    n_bytes = sum(q.numel() * q.element_size() for q in params)
    ms_sync, ms_nosync = max(r[0] for r in per_rank) * 1e3, max(r[1] for r in per_rank) * 1e3
    return {"ms_per_microstep_allreduce": round(ms_sync, 3), "ms_per_microstep_no_sync": round(ms_nosync, 3),
            "ms_exposed_allreduce": round(ms_sync - ms_nosync, 3), "bytes_reduced_per_microstep": int(n_bytes),
            "trainable_tensors": len(params), "world_size": world, "backend": backend,
            "per_rank_ms": [[round(v * 1e3, 3) for v in r] for r in per_rank],
            "note": "one optimize() micro-step (grad-mode replay forward + native backward) under DistributedDataParallel; MAX over ranks; "
                    "exposed = synchronising - no_sync() on the same backward; untimed w.r.t. `value`"}


def dry_run(args, world, rank):
    """Launcher / aggregation self-test WITHOUT a GPU (tests/test_dist_gloo.py): same rendezvous, barriers, MAX-over-ranks timing,
    per-rank gather and JSON assembly as the real path, on the gloo backend with the rollout replaced by a sleep.  Not a measurement."""
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    B, N = args.batch, args.denoise_steps

    def fence():
        if world > 1:
            dist.barrier()

    for _ in range(args.warmup):
        time.sleep(0.01)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.05 * (1 + rank))          # rank r is slower: MAX over ranks must pick the last rank
    fence()
    elapsed = time.perf_counter() - t0
    per_rank = [elapsed]
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64)
        allt = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(allt, tt)
        per_rank = [float(x.item()) for x in allt]
        elapsed = max(per_rank)
    ddp_leg = None
    if args.full and world > 1 and not args.no_ddp_step:
        # the assembly of the `optimize_step_ddp` leg (wrapper, sync / no_sync timing, MAX over ranks, byte count) on gloo with a stand-in
        # module -- what the real path runs around the engine's autograd node
        from torch.nn.parallel import DistributedDataParallel as DDP
        torch.manual_seed(0)
        net = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.Tanh(), torch.nn.Linear(128, 64))
        wrapped = DDP(net)
        xin = torch.randn(8, 64)

        def microstep():
            wrapped(xin).square().mean().backward()
        ddp_leg = ddp_optimize_leg(wrapped, microstep, list(net.parameters()), world, rank, None, iters=2, backend="gloo")
    if rank == 0:
        print(json.dumps({
            **({"optimize_step_ddp": ddp_leg} if ddp_leg is not None else {}),
            "metric": "denoise-steps/sec (whole node), SD3.5-medium 1024^2 GRPO rollout", "value": round(B * N * args.steps * world / elapsed, 3),
            "unit": "denoise-steps/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "dry-run", "config": {"workload": "launcher self-test (no GPU work)", "global_batch": B * world},
            "world": {"backend": "gloo", "world_size": world,
                      "per_rank_denoise_steps_per_s": [round(B * N * args.steps / t, 3) for t in per_rank]}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8, help="samples per rollout micro-batch per GPU")
    ap.add_argument("--guidance", type=float, default=1.0, help="> 1 enables CFG (2 forwards per denoise step)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--denoise-steps", type=int, default=28)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure, run everything else this file measures or checks (all untimed w.r.t. `value`): the "
                         "kernel-variant cross-check, the roofline figures that take rollouts of their own, power, graph vs eager, small batches, "
                         "VAE decode, the optimize() steps, the other families, the DDP step (--gpus > 1) and the CPU baseline; the --no-... "
                         "switches below take single legs out again")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-selfcheck", action="store_true", help="skip the untimed kernel-variant cross-check of one rollout")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--kernel-timing", choices=["attention", "all"], default="attention",
                    help="hipEvent brackets in the timed region: the dominant kernel only (default) or every class")
    ap.add_argument("--pp-min-tiles", type=int, default=None, help="(tuning) smallest 256x256-tile grid that uses the ping-pong GEMM")
    ap.add_argument("--model", choices=["sd3_5", "flux1"], default="sd3_5",
                    help="sd3_5 = BASELINE.json configs[1] (the metric's config); flux1 = FLUX.1-dev geometry (configs[2], SURVEY 8(f) N3)")
    ap.add_argument("--no-vae", action="store_true", help="skip the (untimed w.r.t. `value`) VAE-decode leg")
    ap.add_argument("--no-small-batch", action="store_true",
                    help="skip the (untimed w.r.t. `value`) small-batch legs: B = 2 at 1024^2 and the reference's 512^2 B = 2 CFG example shape")
    ap.add_argument("--no-clock-probe", action="store_true", help="skip the delivered-core-clock probe of one extra (untimed) rollout")
    ap.add_argument("--no-train-step", action="store_true",
                    help="skip the optimize()-replay leg (SURVEY.md 8(f) N1; scripts/train_bench.py in a subprocess, untimed w.r.t. `value`)")
    ap.add_argument("--no-families", action="store_true",
                    help="skip the (untimed w.r.t. `value`) FLUX.1-dev / Wan2.1 / Qwen-Image rollout legs (BASELINE.json configs[2..4]; subprocesses)")
    ap.add_argument("--no-ddp-step", action="store_true",
                    help="(--gpus > 1) skip the `optimize_step_ddp` leg: one optimize() micro-step under DistributedDataParallel on the RCCL group, "
                         "synchronising vs no_sync() (the exposed gradient all-reduce time of the policy update)")
    ap.add_argument("--ddp-step-world1", action="store_true",
                    help="(--gpus 1) run the `optimize_step_ddp` leg on a world-size-1 RCCL group: communicator, reducer buckets and all-reduce "
                         "kernels without a second peer -- a self-test of the leg on a 1-GPU box, not a scaling number")
    ap.add_argument("--no-graph", action="store_true", help="launch the rollout eagerly instead of replaying the hipGraph")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher self-test without a GPU: gloo backend, the rollout replaced by a fixed sleep per micro-batch "
                         "(tests/test_dist_gloo.py); the JSON line is marked \"data\": \"dry-run\" and is NOT a measurement")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them returned (rank 0's samples) as DIR/<field>.npy, float32, at most "
                         "64 MB in all: the same arguments give the same inputs, so two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.dry_run:
        ap.error("--dump-outputs: a dry run computes nothing")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if args.dry_run:
        return dry_run(args, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the rollout engine has no CPU path")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI; the rollout itself needs no collective
    elif args.ddp_step_world1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)

    from mi355_flow import _lib
    from mi355_flow.adapter import SD3_5NativeAdapter
    from mi355_flow.engine import TransformerConfig
    from mi355_flow.scheduler import FlowMatchEulerDiscreteSDEScheduler
    from mi355_flow.trajectory import compute_trajectory_indices
    from mi355_flow.weights import synthetic_state_dict

    flux_mode = args.model == "flux1"
    B, N = args.batch, args.denoise_steps
    g = torch.Generator(device=dev).manual_seed(4321 + rank)
    torch.manual_seed(42 + rank)  # reference: set_seed(seed, device_specific=True) (trainers/loader.py:70)
    if flux_mode:
        from mi355_flow.flux import Flux1NativeAdapter, FluxConfig
        from mi355_flow.weights import flux_forward_flops, synthetic_flux_state_dict
        cfg = FluxConfig()  # FLUX.1-dev
        n_text = 512
        sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42,
                                                   dynamics_type="Flow-SDE", shift=3.0, use_dynamic_shifting=True)
        adapter = Flux1NativeAdapter(synthetic_flux_state_dict(cfg, device=dev, seed=1234), cfg, sched, latent_storage_dtype="fp16", device=dev)
        torch.cuda.empty_cache()
        cfg_on = False
        if args.guidance == 1.0:
            args.guidance = 3.5   # embedded guidance (examples/grpo/full/flux1/default.yaml); no second forward
        pe = torch.randn(B, n_text, cfg.joint_attention_dim, device=dev, generator=g).bfloat16()
        pp = torch.randn(B, cfg.pooled_projection_dim, device=dev, generator=g).bfloat16()
        adapter.rollout()
        traj = compute_trajectory_indices(sched.train_timesteps, N)

        def one_rollout():
            return adapter.inference(prompt=None, height=args.size, width=args.size, num_inference_steps=N, guidance_scale=args.guidance,
                                     prompt_embeds=pe, pooled_prompt_embeds=pp, compute_log_prob=True, trajectory_indices=traj)
    else:
        cfg = TransformerConfig()  # SD3.5-medium
        n_text = N_TEXT
        sched = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42,
                                                   dynamics_type="Flow-SDE", shift=3.0)
        adapter = SD3_5NativeAdapter(synthetic_state_dict(cfg, device=dev, seed=1234), cfg, sched, latent_storage_dtype="fp16",
                                     device=dev)
        cfg_on = args.guidance > 1.0
        pe = torch.randn(B, N_TEXT, cfg.joint_attention_dim, device=dev, generator=g).bfloat16()
        pp = torch.randn(B, cfg.pooled_projection_dim, device=dev, generator=g).bfloat16()
        ne = torch.randn(B, N_TEXT, cfg.joint_attention_dim, device=dev, generator=g).bfloat16() if cfg_on else None
        npl = torch.randn(B, cfg.pooled_projection_dim, device=dev, generator=g).bfloat16() if cfg_on else None
        adapter.rollout()
        traj = compute_trajectory_indices(sched.train_timesteps, N)

        def one_rollout():
            return adapter.inference(prompt=None, height=args.size, width=args.size, num_inference_steps=N,
                                     guidance_scale=args.guidance, prompt_embeds=pe, pooled_prompt_embeds=pp,
                                     negative_prompt_embeds=ne, negative_pooled_prompt_embeds=npl, compute_log_prob=True,
                                     trajectory_indices=traj)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    lib = _lib.load()
    if args.pp_min_tiles is not None:
        lib.mi355_tune_set(3, args.pp_min_tiles)
    if os.environ.get("MI355_ATTN_STATIC") == "0":     # A/B: keep the running-max softmax even where the static bound holds
        lib.mi355_tune_set(6, 0)
    # (MI355_TUNE="key=value,..." -- A/B of kernel / launch variants -- is applied by _lib.load() itself)
    for _ in range(args.warmup):
        samples = one_rollout()
    if not args.full and not args.no_selfcheck and not flux_mode:
        # a plain run leaves the cross-check below out, but not what it does to the inputs of the timed steps: they have always drawn their
        # noise from where the check's seeded rollout leaves the global generator, and go on doing so (same samples, same `--dump-outputs`)
        torch.cuda.manual_seed(1234 + rank)
        skip_rollout_draws(adapter, B, args.size, N, dev)
    if args.full and not args.no_selfcheck and not flux_mode:
        # untimed sanity net: the same seeded rollout through the first-correct-path kernels (simple GEMM schedule,
        # plain online softmax, eager launches) must reproduce the shipped kernels' trajectory
        def seeded():
            torch.cuda.manual_seed(1234 + rank)
            out = one_rollout()
            return torch.stack([o.all_latents for o in out]).float(), torch.stack([o.log_probs for o in out])
        lat_a, lp_a = seeded()
        for k, v in ((0, 0), (1, 0), (2, 0)):
            lib.mi355_tune_set(k, v)
        lat_b, lp_b = seeded()
        for k, v in ((0, 1), (1, 1), (2, 0 if args.no_graph else 1)):
            lib.mi355_tune_set(k, v)
        rel = float((lat_a - lat_b).norm() / lat_b.norm())
        if not (rel < 2e-2 and torch.allclose(lp_a, lp_b, rtol=1e-3)):
            raise SystemExit(f"bench selfcheck failed: kernel variants disagree (latents rel-L2 {rel:.3e}, log-probs {lp_a.tolist()} vs {lp_b.tolist()})")
    timing = not args.no_kernel_timing and not flux_mode   # (per-class hipEvent brackets exist in the SD3.5 engine only)
    fence()
    if args.no_graph:
        lib.mi355_tune_set(2, 0)
    if args.pp_min_tiles is not None:
        lib.mi355_tune_set(3, args.pp_min_tiles)
    if timing and args.kernel_timing == "all":
        # per-class brackets only mean something when one kernel runs at a time: with the text chain on its side stream the small
        # text-stream kernels overlap the image-stream ones and their durations are concurrency stretch, not cost
        lib.mi355_tune_set(8, 0)
    if timing:
        lib.mi355_profile_enable(1 if args.kernel_timing == "all" else 2)  # brackets force eager launches
    t0 = time.perf_counter()
    for _ in range(args.steps):
        samples = one_rollout()
    fence()
    elapsed = time.perf_counter() - t0
    import ctypes as C
    ms = (C.c_double * 5)()
    cnt = (C.c_int64 * 5)()
    if timing:
        _lib.check(lib.mi355_profile_collect(ms, cnt), "profile_collect")
        lib.mi355_profile_enable(0)
    per_rank = [elapsed]
    if world > 1:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        allt = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(allt, tt)
        per_rank = [float(x.item()) for x in allt]
        elapsed = max(per_rank)                      # MAX over ranks
    assert len(samples) == B and samples[0].all_latents.shape[0] == len(traj) and torch.isfinite(samples[0].log_probs).all()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, samples)

    n_cfg = 2 if cfg_on else 1
    lat = args.size // 8
    Ni = (lat // 2) ** 2
    denoise_steps_total = B * N * args.steps * world
    value = denoise_steps_total / elapsed
    F = flux_forward_flops(cfg, Ni, n_text) if flux_mode else forward_flops(cfg, Ni, N_TEXT)
    fwd_tflops = n_cfg * F * (B * N * args.steps) / elapsed / 1e12  # per GPU
    out = {
        "metric": ("denoise-steps/sec (whole node), FLUX.1-dev 1024^2 GRPO rollout" if flux_mode else
                   "denoise-steps/sec (whole node), SD3.5-medium 1024^2 GRPO rollout"), "value": round(value, 3),
        "unit": "denoise-steps/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"{'FLUX.1-dev (11.9 B parameters, embedded guidance)' if flux_mode else 'SD3.5-medium'} T2I GRPO rollout, "
                               f"{args.size}x{args.size}, {N} denoise steps (Flow-SDE, 1 SDE step, "
                               f"log-prob fused), batch {B}/GPU, n_cfg={n_cfg}, fp16 latent storage; 1 bench step = 1 rollout micro-batch",
                   "global_batch": B * world, "tokens_per_sample": Ni + n_text, "n_cfg": n_cfg, "denoise_steps": N,
                   "parallelism": f"dp{world} (rollout shards by prompt group, no data-path collective)"},
        "world": {"backend": "nccl (RCCL)" if world > 1 else None, "world_size": world,
                  "per_rank_denoise_steps_per_s": [round(B * N * args.steps / t, 3) for t in per_rank]},
    }
    if os.environ.get("MI355_TUNE"):
        out["tune"] = os.environ["MI355_TUNE"]          # non-default kernel / launch variants of this run (mi355_tune_set keys)
    if timing and args.kernel_timing == "all":
        out["tune"] = (out.get("tune", "") + ",8=0 (single stream: --kernel-timing all)").lstrip(",")
        lib.mi355_tune_set(8, _stream_mode_at_start())
    if timing and rank == 0:
        attn_fl, attn_launches = attention_flops(cfg, Ni, N_TEXT)
        fwd_per_timed = n_cfg * N * args.steps  # transformer forwards (batch B each) in the timed region on this rank
        names = ["attention", "gemm", "ln_modulate", "sde_step", "misc"]
        by_class = {names[i]: {"ms": round(ms[i], 3), "launches": int(cnt[i])} for i in range(5) if cnt[i] > 0}
        a_ms = ms[0] / max(cnt[0], 1)                       # mean duration of one attention launch
        a_flop = attn_fl * B * n_cfg / attn_launches        # mean algorithmic FLOPs of one attention launch (forward batch B*n_cfg)
        achieved = a_flop / (a_ms * 1e-3) / 1e12 if a_ms > 0 else 0.0
        gemm_fl = (F - attn_fl) * B * fwd_per_timed        # fwd_per_timed already counts the n_cfg forwards
        # HBM bytes per launch come from a rocprofv3 --pmc pass (counters cannot be read from inside the process): the committed
        # summary names the commit it was collected at; `traffic` is null when there is none
        traffic, traffic_src, mfma_busy = None, None, None
        pmc = os.path.join(ROOT, "profiles", "pmc_attention.json")
        if os.path.isfile(pmc):
            pj = json.load(open(pmc))
            traffic = pj.get("hbm_bytes_per_launch")
            mfma_busy = pj.get("mfma_busy")
            traffic_src = f"profiles/pmc_attention.json@{pj.get('commit', 'round-' + str(pj.get('round')))} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes)"
        ainfo = adapter.engine.attention_info()
        out["roofline"] = {
            "bound": "mfma", "kernel": "attn_kernel (joint S=4429 x24, dual S=4096 x13 per forward)",
            "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
            "traffic": traffic, "traffic_source": traffic_src, "mfma_busy": mfma_busy, "flops_per_launch": a_flop, "ms_per_launch": round(a_ms, 4),
            "static_softmax": ainfo["static"] == ainfo["total"] and os.environ.get("MI355_ATTN_STATIC") != "0",
            "static_softmax_launches": f"{ainfo['static']}/{ainfo['total']} (proven |score| bound {ainfo['max_bound']:.1f} <= 60 selects it per layer: "
                                       "weight-dependent -- see attention_dynamic for the kernel every checkpoint can run)",
            **({"gemm": {"achieved": round(gemm_fl / (ms[1] * 1e-3) / 1e12, 1),
                         "frac": round(gemm_fl / (ms[1] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)}} if ms[1] > 0 else {}),
            "forward": {"achieved": round(fwd_tflops, 1), "frac": round(fwd_tflops / PEAK_BF16_TFLOPS, 4),
                        "flops_per_forward_per_sample": F, "note": "wall-clock of the whole rollout incl. host glue; north-star target 0.40"},
            "by_class": by_class,
        }
    if args.full and timing and rank == 0 and world == 1:
        # (a) the running-max ("dynamic") attention kernel on the same rollout: what a checkpoint whose q/k norm weights do not
        #     prove the static bound would run;  (b) graph-replay vs eager wall clock of one rollout (the timed region above runs
        #     eagerly because the event brackets cannot live inside a captured graph)
        def timed_rollout():
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            one_rollout()
            torch.cuda.synchronize()
            return time.perf_counter() - t1
        lib.mi355_tune_set(6, 0)
        one_rollout()                                   # re-capture / warm with the dynamic kernel
        lib.mi355_profile_enable(2)
        dyn_wall = timed_rollout()
        _lib.check(lib.mi355_profile_collect(ms, cnt), "profile_collect")
        lib.mi355_profile_enable(0)
        d_ms = ms[0] / max(cnt[0], 1)
        lib.mi355_tune_set(6, 0 if os.environ.get("MI355_ATTN_STATIC") == "0" else 1)
        out["roofline"]["attention_dynamic"] = {"achieved": round(a_flop / (d_ms * 1e-3) / 1e12, 1), "ms_per_launch": round(d_ms, 4),
                                                "frac": round(a_flop / (d_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                                                "rollout_denoise_steps_per_s": round(B * N / dyn_wall, 3)}
        # the floor that holds for ANY checkpoint (the static-softmax kernel is selected per layer from the q/k norm weights): `frac` above is
        # the timed region's kernel; these two are the same rollout on the running-max kernel
        dyn_fwd = n_cfg * F * B * N / dyn_wall / 1e12
        out["roofline"]["guaranteed_floor"] = {"attention_frac": out["roofline"]["attention_dynamic"]["frac"],
                                               "forward_frac": round(dyn_fwd / PEAK_BF16_TFLOPS, 4), "forward_achieved": round(dyn_fwd, 1),
                                               "note": "running-max softmax on every layer (what a checkpoint whose norm weights prove no score "
                                                       "bound runs); one untimed eager rollout with event brackets"}
        # the GEMM class (51 % of the kernel time) in the driver's own record: one more untimed eager rollout with EVERY class bracketed -- on a
        # single stream, because beside a side stream the small text GEMMs' durations are concurrency stretch, not cost
        if args.kernel_timing != "all":
            try:
                lib.mi355_tune_set(8, 0)
                one_rollout()
                lib.mi355_profile_enable(1)
                one_rollout()
                torch.cuda.synchronize()
                _lib.check(lib.mi355_profile_collect(ms, cnt), "profile_collect")
                lib.mi355_profile_enable(0)
                g_fl = (F - attn_fl) * B * n_cfg * N
                names5 = ["attention", "gemm", "ln_modulate", "sde_step", "misc"]
                out["roofline"]["gemm"] = {"achieved": round(g_fl / (ms[1] * 1e-3) / 1e12, 1), "frac": round(g_fl / (ms[1] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                                           "ms_per_rollout": round(ms[1], 2), "launches": int(cnt[1]),
                                           "note": "all GEMM launches of one untimed single-stream eager rollout, event-bracketed; algorithmic FLOPs = forward minus attention"}
                out["roofline"]["by_class_single_stream"] = {names5[i]: {"ms": round(ms[i], 3), "launches": int(cnt[i])} for i in range(5) if cnt[i] > 0}
            except Exception as e:  # noqa: BLE001
                out["roofline"]["gemm"] = {"error": repr(e)}
            lib.mi355_tune_set(8, _stream_mode_at_start())
        lib.mi355_tune_set(2, 1)
        one_rollout(); one_rollout()                    # eager warm-up + capture
        # package power and energy of the rollout (ROCm SMI, in-process): the round-3 finding that the rollout runs at the power cap had clock
        # evidence only.  Two graph-replayed rollouts inside the sampling window; energy from the device's accumulator.
        try:
            sys.path.insert(0, os.path.join(ROOT, "scripts"))
            from power_meter import PowerMeter
            one_rollout()
            torch.cuda.synchronize()
            with PowerMeter(device=local) as pm:
                one_rollout(); one_rollout()
                torch.cuda.synchronize()
            ps = pm.summary()
            if ps.get("energy_j"):
                ps["joules_per_rollout"] = round(ps["energy_j"] / 2, 1)
                ps["joules_per_denoise_step"] = round(ps["energy_j"] / 2 / (B * N), 2)
                ps["algorithmic_tflop_per_joule"] = round(n_cfg * F * B * N * 2 / ps["energy_j"] / 1e12, 3)
            ps["note"] = "socket power sampled every 20 ms (rsmi_dev_power_get) over two graph-replayed rollouts; energy = rsmi_dev_energy_count_get delta"
            out["power"] = ps
        except Exception as e:  # noqa: BLE001
            out["power"] = {"error": repr(e)}
        if not args.no_clock_probe:
            # core clock DELIVERED under the package power cap while the rollout runs: one probe wave on a side stream samples
            # {s_memtime, s_memrealtime (100 MHz)} pairs beside one more (untimed) graph-replayed rollout
            try:
                import numpy as np
                n_s = 2000
                buf = torch.zeros(2 * n_s, device=dev, dtype=torch.int64)
                side = torch.cuda.Stream()
                span_s = (elapsed / args.steps) * 0.6
                torch.cuda.synchronize()
                one_rollout()                                               # load is running before the probe starts
                _lib.check(lib.mi355_clock_probe(side.cuda_stream, buf.data_ptr(), n_s, max(1, int(span_s * 1.8e9 / 8128 / n_s))), "clock_probe")
                one_rollout(); one_rollout()
                torch.cuda.synchronize()
                a = buf.cpu().numpy().reshape(n_s, 2).astype(np.float64)
                dc, dw = np.diff(a[:, 0]), np.diff(a[:, 1])
                mhz = dc[dw > 0] / dw[dw > 0] * 100.0
                med = float(np.median(mhz))
                out["roofline"]["delivered_clock_mhz"] = {"median": round(med, 0), "p10": round(float(np.percentile(mhz, 10)), 0),
                                                          "p90": round(float(np.percentile(mhz, 90)), 0), "nominal": 2400,
                                                          "span_ms": round((a[-1, 1] - a[0, 1]) / 100.0 * 1e-3, 1),
                                                          "forward_frac_at_delivered_clock": round(fwd_tflops / (PEAK_BF16_TFLOPS * med / 2400.0), 4),
                                                          "note": "s_memtime / s_memrealtime of a probe wave beside the rollout (mi355_clock_probe); the peaks "
                                                                  "are quoted at 2400 MHz"}
            except Exception as e:  # noqa: BLE001
                out["roofline"]["delivered_clock_mhz"] = {"error": repr(e)}
        g_s = min(timed_rollout() for _ in range(2))
        lib.mi355_tune_set(2, 0)
        e_s = min(timed_rollout() for _ in range(2))
        lib.mi355_tune_set(2, 0 if args.no_graph else 1)
        out["graph_vs_eager"] = {"graph_ms_per_rollout": round(g_s * 1e3, 2), "eager_ms_per_rollout": round(e_s * 1e3, 2),
                                 "graph_denoise_steps_per_s": round(B * N / g_s, 3), "eager_denoise_steps_per_s": round(B * N / e_s, 3),
                                 "note": "untimed w.r.t. `value`; one hipGraph launch replays the whole N-step loop (~7 850 kernels)"}
    if args.full and rank == 0 and world == 1 and not flux_mode and not args.no_small_batch:
        # Small-batch configurations of the same engine (hipGraph replay; the text-stream chain of every block on a second stream): the
        # reference's own example shape (examples/grpo/full/sd3_5: 512^2, N = 10, B = 2 with CFG) and B = 2 at the bench resolution.
        # Reported beside the metric, never inside `value`; a failure here is recorded, not raised.
        try:
            legs = {}
            lib.mi355_tune_set(2, 1)
            for tag, (b2, size2, gs2, n2) in (("b2_1024_nocfg_28", (2, 1024, 1.0, 28)), ("b2_512_cfg4.5_10", (2, 512, 4.5, 10))):
                cfg2 = gs2 > 1.0
                pe2 = torch.randn(b2, N_TEXT, cfg.joint_attention_dim, device=dev, generator=g).bfloat16()
                pp2 = torch.randn(b2, cfg.pooled_projection_dim, device=dev, generator=g).bfloat16()
                ne2 = torch.randn(b2, N_TEXT, cfg.joint_attention_dim, device=dev, generator=g).bfloat16() if cfg2 else None
                np2 = torch.randn(b2, cfg.pooled_projection_dim, device=dev, generator=g).bfloat16() if cfg2 else None
                traj2 = compute_trajectory_indices(sched.train_timesteps, n2)

                def roll2():
                    return adapter.inference(prompt=None, height=size2, width=size2, num_inference_steps=n2, guidance_scale=gs2,
                                             prompt_embeds=pe2, pooled_prompt_embeds=pp2, negative_prompt_embeds=ne2,
                                             negative_pooled_prompt_embeds=np2, compute_log_prob=True, trajectory_indices=traj2)
                roll2(); roll2()                                  # eager warm-up of the new plan, then capture
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(3):
                    s2 = roll2()
                torch.cuda.synchronize()
                dt2 = (time.perf_counter() - t1) / 3
                assert len(s2) == b2 and torch.isfinite(s2[0].log_probs).all()
                n_cfg2 = 2 if cfg2 else 1
                F2 = forward_flops(cfg, (size2 // 16) ** 2, N_TEXT)
                tf2 = n_cfg2 * F2 * b2 * n2 / dt2 / 1e12
                legs[tag] = {"batch": b2, "size": size2, "guidance": gs2, "denoise_steps": n2, "ms_per_rollout": round(dt2 * 1e3, 2),
                             "denoise_steps_per_s": round(b2 * n2 / dt2, 2), "forward_tflops": round(tf2, 1),
                             "forward_frac": round(tf2 / PEAK_BF16_TFLOPS, 4)}
            out["small_batch"] = {**legs, "note": "hipGraph replay, two-stream forward; untimed w.r.t. `value`"}
        except Exception as e:  # noqa: BLE001 -- never let an extra leg take the headline line down
            out["small_batch"] = {"error": repr(e)}
        lib.mi355_tune_set(2, 0 if args.no_graph else 1)
    if flux_mode and rank == 0:
        out["roofline"] = {"bound": "mfma", "kernel": "whole FLUX.1 forward (MFMA GEMMs + head_dim-128 attention), wall-clock of the rollout",
                           "achieved": round(fwd_tflops, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(fwd_tflops / PEAK_BF16_TFLOPS, 4),
                           "traffic": None, "flops_per_forward_per_sample": F}
    if args.full and rank == 0 and not args.no_vae:
        # image decode that closes the reference's rollout (sd3_5.py:307): reported beside the metric,
        # not inside it -- `value` counts denoise steps, the decode is once per sample
        from mi355_flow.vae import VAEConfig, VAEDecoder
        from mi355_flow.weights import synthetic_vae_state_dict, vae_decode_flops
        vcfg = VAEConfig(scaling_factor=0.3611, shift_factor=0.1159) if flux_mode else VAEConfig()
        dec = VAEDecoder(vcfg)
        dec.bind_state_dict(synthetic_vae_state_dict(vcfg, device=dev))
        dec.ready()
        zl = torch.randn(B, 16, lat, lat, device=dev, generator=g).half()
        vb = min(4, B)
        dec.decode(zl, max_batch=vb)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            img = dec.decode(zl, max_batch=vb)
        e1.record()
        torch.cuda.synchronize()
        v_ms = e0.elapsed_time(e1) / 3 / B
        v_tf = vae_decode_flops(vcfg, lat, lat) / (v_ms * 1e-3) / 1e12
        out["vae_decode"] = {"ms_per_image": round(v_ms, 3), "achieved": round(v_tf, 1), "unit": "TFLOP/s", "frac": round(v_tf / PEAK_BF16_TFLOPS, 4),
                             "flops_per_image": vae_decode_flops(vcfg, lat, lat), "micro_batch": vb,
                             "share_of_rollout": round(v_ms * B / (elapsed / args.steps * 1e3), 4),
                             "note": "SD3 AutoencoderKL decoder, synthetic weights; outside the timed region"}
        assert bool(torch.isfinite(img.float()).all())
        dec.close()
    if args.full and rank == 0 and world == 1 and not flux_mode and not args.no_train_step:
        # the optimize() replay step with gradients (reference trainers/grpo.py:185-342) at B = 2, 1024^2, the reference's
        # default target modules: forward with stash + native backward.  Its own process (its stash and scratch are ~10 GiB; nothing of
        # this process's state is touched), reported beside the metric, never inside it; any failure is recorded, not raised.
        try:
            import subprocess
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_bench.py"), "--batch", "2", "--size", "1024", "--train", "default",
                                "--iters", "3"], capture_output=True, text=True, timeout=300)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            tb = json.loads(line)
            out["optimize_step"] = {"ms_forward_backward": tb["ms_forward_backward"], "ms_forward_train": tb["ms_forward_train"],
                                    "ms_forward_nograd": tb["ms_forward_nograd"], "achieved": tb["tflops_step"], "unit": "TFLOP/s",
                                    "frac": tb["frac_of_2500"], "trainable_params": tb["trainable_params"], "ratio_is_one": tb["ratio_is_one"],
                                    "trainable": tb["trainable"],
                                    "note": "B = 2, 1024^2, SD3_5Adapter.default_target_modules (reference sd3_5.py:75-80: the eight attn.* "
                                            "projections, image and text side; attn2 frozen); grad-mode log-prob torch.equal the no-grad "
                                            "replay's; untimed w.r.t. `value`"}
        except Exception as e:  # noqa: BLE001
            out["optimize_step"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not flux_mode and not args.no_train_step:
        # the same for FLUX.1 (round 4: native backward, SURVEY.md 8(f) N1 over N3): FLUX.1-dev geometry, B = 1, 1024^2 (4608 joint tokens),
        # the reference's default FLUX.1 target modules (5.4 B trainable parameters); own process (~110 GB of HBM), recorded, never raised
        try:
            import subprocess
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "flux_train_bench.py"), "--batch", "1", "--size", "1024", "--iters", "2"],
                               capture_output=True, text=True, timeout=300)
            tb = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            out["optimize_step_flux1"] = {"ms_forward_backward": tb["ms_forward_backward"], "ms_forward_train": tb["ms_forward_train"],
                                          "ms_forward_nograd": tb["ms_forward_nograd"], "achieved": tb["tflops_step"], "unit": "TFLOP/s",
                                          "frac": tb["frac_of_2500"], "trainable_params": tb["trainable_params"], "ratio_is_one": tb["ratio_is_one"],
                                          "stash_plus_scratch_GiB": tb["stash_plus_scratch_GiB"],
                                          "note": "FLUX.1-dev geometry, B = 1, 1024^2, default target modules (flux1.py:76-84); grad-mode log-prob "
                                                  "torch.equal the no-grad replay's; untimed w.r.t. `value`"}
        except Exception as e:  # noqa: BLE001
            out["optimize_step_flux1"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not flux_mode and not args.no_train_step:
        # ... and for Qwen-Image (round 4: native backward, SURVEY.md 8(f) N1 over N4; BASELINE.json configs[4]'s family): 60 layers, B = 1, 1024^2,
        # true CFG (forward batch [negative | positive]), the reference's default target modules (6.8 B trainable parameters); own process
        # (~150 GB of HBM: 41 GB masters + 41 GB engine copy + transposed weights + 37 GB stash), recorded, never raised
        try:
            import subprocess
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "qwen_train_bench.py"), "--batch", "1", "--size", "1024", "--iters", "2"],
                               capture_output=True, text=True, timeout=420)
            tb = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            out["optimize_step_qwen_image"] = {"ms_forward_backward": tb["ms_forward_backward"], "ms_forward_train": tb["ms_forward_train"],
                                               "ms_forward_nograd": tb["ms_forward_nograd"], "achieved": tb["tflops_step"], "unit": "TFLOP/s",
                                               "frac": tb["frac_of_2500"], "trainable_params": tb["trainable_params"], "ratio_is_one": tb["ratio_is_one"],
                                               "stash_plus_scratch_GiB": tb["stash_plus_scratch_GiB"], "n_cfg": tb["n_cfg"],
                                               "note": "Qwen-Image geometry (60 layers), B = 1, 1024^2, true CFG, default target modules "
                                                       "(qwen_image.py:81-89); grad-mode log-prob torch.equal the no-grad replay's; untimed w.r.t. `value`"}
        except Exception as e:  # noqa: BLE001
            out["optimize_step_qwen_image"] = {"error": repr(e)}
    if args.full and rank == 0 and world == 1 and not flux_mode and not args.no_train_step:
        # ... and for Wan2.1-T2V-1.3B at BASELINE.json configs[3]'s OWN shape: 480 x 832 x 49 frames (20 280 video tokens), B = 1, CFG, all 30 blocks,
        # the reference's default Wan target modules (first timed in round 5's first GPU call: 1092.8 ms, profiles/r05a_wan_train_b1_480p49.json);
        # own process (~83 GiB of HBM), recorded, never raised
        try:
            import subprocess
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "wan_train_bench.py"), "--batch", "1", "--frames", "49", "--iters", "2"],
                               capture_output=True, text=True, timeout=150)
            tb = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            out["optimize_step_wan21"] = {"ms_forward_backward": tb["ms_forward_backward"], "ms_forward_train": tb["ms_forward_train"],
                                          "ms_forward_nograd": tb["ms_forward_nograd"], "achieved": tb["tflops_step"], "unit": "TFLOP/s",
                                          "frac": tb["frac_of_2500"], "trainable_params": tb["trainable_params"], "ratio_is_one": tb["ratio_is_one"],
                                          "stash_plus_scratch_GiB": tb["stash_plus_scratch_GiB"], "tokens": tb["tokens"], "n_cfg": tb["n_cfg"],
                                          "note": "Wan2.1-T2V-1.3B geometry (30 layers), B = 1, 480 x 832 x 49 frames (config D's own shape), CFG, default target modules "
                                                  "(wan2_t2v.py:74-85); untimed w.r.t. `value`"}
        except Exception as e:  # noqa: BLE001
            out["optimize_step_wan21"] = {"error": repr(e), "stderr_tail": (r.stderr[-400:] if "r" in dir() and hasattr(r, "stderr") else "")}
    if args.full and rank == 0 and world == 1 and not flux_mode and not args.no_families:
        # BASELINE.json configs[2..4] on the driver's box: the other engines' rollouts at their own geometries, 2 denoise
        # steps each (the per-step cost does not depend on the step count), each in its own process (24 / 3 / 41 GB of weights), untimed w.r.t.
        # `value`; a failure is recorded under its key, never raised.
        import subprocess
        fam = {}
        for tag, cmd in (("flux1_dev_b8_1024", ["flux_bench.py", "--batch", "8", "--size", "1024", "--denoise-steps", "2", "--iters", "2"]),
                         ("wan21_t2v_1p3b_b2_cfg_480x832x49", ["wan_bench.py", "--batch", "2", "--denoise-steps", "2", "--iters", "2"]),
                         ("qwen_image_b2_cfg_1328", ["qwen_bench.py", "--batch", "2", "--size", "1328", "--denoise-steps", "2", "--iters", "2"])):
            try:
                t1 = time.perf_counter()
                r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", cmd[0])] + cmd[1:], capture_output=True, text=True, timeout=300)
                fb = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                fam[tag] = {"denoise_steps_per_s": fb["denoise_steps_per_s"], "forward_tflops": fb["forward_tflops"], "forward_frac": fb["frac_of_2.5PF"],
                            "batch": fb.get("batch"), "n_cfg": fb.get("n_cfg", 1), "denoise_steps": fb.get("denoise_steps"), "finite": fb.get("finite"),
                            "leg_wall_s": round(time.perf_counter() - t1, 1)}
            except Exception as e:  # noqa: BLE001
                fam[tag] = {"error": repr(e)}
        fam["note"] = ("real geometries (FLUX.1-dev 11.9 B, Wan2.1-T2V-1.3B, Qwen-Image 60 layers), synthetic weights / prompts, hipGraph / eager as each "
                       "engine ships; denoise-steps/s = samples x steps / wall; forward_frac vs 2.5 PFLOP/s on algorithmic matmul FLOPs")
        out["families"] = fam
    if ((args.full and world > 1) or args.ddp_step_world1) and not flux_mode and not args.no_ddp_step:
        # north star: "gradient all-reduce on RCCL over xGMI for the policy update" -- every rank takes part; a failure on any rank is
        # recorded (and keeps the headline line), never raised
        # This leg is the only part of the file where a rank can wait for another rank that is not coming (one rank failing between two
        # collectives).  Two guards keep the headline line safe: (1) everything local -- building the module -- happens first and the ranks
        # agree (MIN of a success flag on the group they already used) before the first DDP collective; (2) a deadline: if the leg has not
        # finished after DDP_LEG_DEADLINE_S seconds, rank 0 prints the line without it and every rank leaves.
        import threading
        print_lock, state = threading.Lock(), {"printed": False}

        def abandon():
            with print_lock:
                if state["printed"]:
                    return
                state["printed"] = True
                if rank == 0:
                    out["optimize_step_ddp"] = {"error": f"the leg did not finish within {DDP_LEG_DEADLINE_S} s on some rank: abandoned"}
                    print(json.dumps(out), flush=True)
            os._exit(0)
        timer = threading.Timer(DDP_LEG_DEADLINE_S, abandon)
        timer.daemon = True
        timer.start()
        leg = None
        try:
            from torch.nn.parallel import DistributedDataParallel as DDP
            from mi355_flow.weights import module_from_state_dict
            del samples
            torch.cuda.empty_cache()
            ok_local, err_local = 1, None
            try:
                mod = module_from_state_dict(synthetic_state_dict(cfg, device=dev, seed=1234))
            except Exception as e:  # noqa: BLE001
                ok_local, err_local = 0, repr(e)
            flag = torch.tensor([ok_local], device=dev, dtype=torch.int32)
            if dist.is_initialized():
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                raise RuntimeError(f"module construction failed on some rank (this rank: {err_local}); leg skipped on every rank")
            targets = ("attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj", "attn.to_add_out",      # SD3_5Adapter.default_target_modules
                       "attn.to_q", "attn.to_k", "attn.to_v", "attn.to_out.0")                           # (reference sd3_5.py:75-80)
            for n_, q_ in mod.named_parameters():
                q_.requires_grad_(any(k_ in n_ for k_ in targets))
            wrapped = DDP(mod, device_ids=[local], broadcast_buffers=False)          # default 25 MiB buckets, like accelerate's
            sched2 = FlowMatchEulerDiscreteSDEScheduler(noise_level=0.7, sde_steps=[1, 2, 3], num_sde_steps=1, seed=42, shift=3.0)
            ad2 = SD3_5NativeAdapter(wrapped, cfg, sched2, latent_storage_dtype="fp16", device=dev)      # bound to the WRAPPED module, like the plugin
            ad2.rollout()
            sched2.set_timesteps(28)
            b2, lat2 = 2, 1024 // 8
            mk = lambda *sh: torch.randn(*sh, device=dev, generator=g)      # noqa: E731
            kw2 = dict(t=sched2.timesteps[2].expand(b2), t_next=sched2.timesteps[3].expand(b2), latents=mk(b2, 16, lat2, lat2).half(),
                       next_latents=mk(b2, 16, lat2, lat2).half(), prompt_embeds=mk(b2, N_TEXT, 4096).bfloat16(),
                       pooled_prompt_embeds=mk(b2, 2048).bfloat16(), guidance_scale=1.0, noise_level=0.7, compute_log_prob=True,
                       return_kwargs=["log_prob", "dt"])
            ad2.train()

            def microstep():
                ad2.forward(**kw2).log_prob.sum().backward()
            leg = ddp_optimize_leg(wrapped, microstep, [q_ for q_ in mod.parameters() if q_.requires_grad], world, rank, dev)
            leg["shape"] = "SD3.5-medium, B = 2 per rank, 1024^2, the reference's default target modules"
            ad2.engine.close()
        except Exception as e:  # noqa: BLE001
            leg = {"error": repr(e)}
        with print_lock:
            if state["printed"]:          # (the deadline fired while this thread was finishing: the line is out, leave)
                os._exit(0)
            state["printed"] = True       # from here on the deadline thread does nothing; the line is printed below
        timer.cancel()
        if rank == 0:
            out["optimize_step_ddp"] = leg
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline and not flux_mode:
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    if world > 1 or (args.ddp_step_world1 and dist.is_initialized()):
        import threading
        bye = threading.Timer(60, lambda: os._exit(0))      # the line is out: never sit in the farewell barrier for a rank that is gone
        bye.daemon = True
        bye.start()
        dist.barrier()
        dist.destroy_process_group()
        bye.cancel()


if __name__ == "__main__":
    main()

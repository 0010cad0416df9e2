"""Operator A/B of tune key 46 (tile-uniform GEMM epilogues, csrc/gemm.hip) at the image-stream shapes of the SD3.5 B = 8, 1024^2 rollout
(32768 rows, rows_per_sample 4096) through mi355_op_gemm_epi under the default dispatch: key 46 = 0 | 1 alternating in one process, five rounds
of 20 launches each (device events), the fastest round of each, bit identity of every output buffer between the two keys, and which kernel
family / epilogue build ran.  Key 46 = 0 runs the general epilogue kernels (the code from before the tile-uniform builds).
usage: python scripts/gemm_epilogue_ab.py [qk]        (qk: the q|k norm launch only)"""
import math, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flow-factory_amd"))
from mi355_flow import engine, _lib
lib = _lib.load()
BIAS, GELU, GATE, QK, VT = 0, 2, 5, 6, 7
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(1)
def rnd(*s, scale=1.0): return (torch.randn(*s, device=dev, generator=g) * scale).bfloat16()
def timeit(fn, iters=20, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3
# (name, epi, M, N, K, tune key 0 value): w4 = 2 forces the 4-wave kernel, 3 the ping-pong kernel; default dispatch = what the model runs
CASES = [("bias_gelu 32768x6144x1536", GELU, 32768, 6144, 1536), ("qk_norm 32768x3072x1536", QK, 32768, 3072, 1536),
         ("gate_res 32768x1536x1536", GATE, 32768, 1536, 1536), ("gate_res 32768x1536x6144", GATE, 32768, 1536, 6144),
         ("vT 1536x32768x1536", VT, 1536, 32768, 1536), ("bias 32768x1536x1536", BIAS, 32768, 1536, 1536),
         ("bias 32768x3072x1536", BIAS, 32768, 3072, 1536)]
if len(sys.argv) > 1 and sys.argv[1] == "qk":
    CASES = [c for c in CASES if c[1] == QK]
RPS = 4096
for name, epi, M, N, K in CASES:
    A = rnd(M, K); W = rnd(N, K, scale=1 / math.sqrt(K))
    bias = torch.randn(M if epi == VT else N, device=dev, generator=g)
    kw = dict(rows_per_sample=RPS)
    bufs = {}
    if epi == QK:
        H = N // 128; S_pad = 4432; B = M // RPS
        bufs["q"] = torch.zeros(B * H * S_pad * 64, device=dev, dtype=torch.bfloat16); bufs["k"] = torch.zeros_like(bufs["q"])
        nw = torch.ones(64, device=dev)
        kw.update(q=bufs["q"], k=bufs["k"], nw_q=nw, nw_k=nw, H=H, S_pad=S_pad, s_off=336, q_scale=0.18)
    elif epi == VT:
        H = M // 64; S_pad = 4432; B = N // RPS
        bufs["q"] = torch.zeros(B * H * 64 * S_pad, device=dev, dtype=torch.bfloat16)
        kw.update(q=bufs["q"], H=H, S_pad=S_pad, s_off=336)
    else:
        bufs["out"] = rnd(M, N)
        kw.update(out=bufs["out"], ldo=N)
        if epi == GATE:
            kw.update(aux=rnd(M // RPS, N), ld_aux=N)
    fam = {}
    def run(key):
        lib.mi355_tune_set(46, key)
        fam[key] = engine.op_gemm_epi(epi, A, K, W, K, M, N, K, bias, **kw) + (",tile-uniform" if lib.mi355_gemm_last_epilogue_tile_uniform() else "")
    # bit identity (gate_res is in place: restore x first)
    outs = {}
    for key in (0, 1):
        for b in bufs.values():          # (the gated residual is in place: both keys start from the same x)
            b.zero_()
        run(key); torch.cuda.synchronize()
        outs[key] = {k: v.clone() for k, v in bufs.items()}
    same = all(torch.equal(outs[0][k], outs[1][k]) for k in bufs)
    t = {0: [], 1: []}
    for rnd_i in range(5):
        for key in (0, 1):
            t[key].append(timeit(lambda: run(key)))
    fl = 2.0 * M * N * K
    m0, m1 = min(t[0]), min(t[1])
    print(f"{name:28s} {fam[1]:21s} key0 {m0:7.1f} us ({fl / m0 / 1e6:6.0f} TF/s) [{' '.join(f'{v:.1f}' for v in t[0])}] | key1 {m1:7.1f} us ({fl / m1 / 1e6:6.0f} TF/s) "
          f"[{' '.join(f'{v:.1f}' for v in t[1])}] | {100 * (m1 / m0 - 1):+.1f} % | bit-identical {same}", flush=True)
lib.mi355_tune_set(46, 1)

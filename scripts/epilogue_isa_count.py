"""Static instruction count of the fused GEMM epilogues (no GPU needed).

Compiles csrc/gemm.hip to gfx950 assembly the way the Makefile compiles it (plus -S --cuda-device-only) and prints
  * for every gemm_w4_kernel<EPI, 0[, FAST]> the mnemonic histogram of the code BEHIND the hand-scheduled main loop -- one output tile's epilogue
    of one wave, straight-line code (v_accvgpr_read statements included) plus the few instructions that close the tile loop;
  * the ScratchSize / NumVgprs / NumAgprs lines of every GEMM kernel.

    python scripts/epilogue_isa_count.py [--src DIR] [--asm FILE] [--top N]

--src: a csrc directory other than this tree's (e.g. an export of the parent commit); --asm: an assembly file made earlier (skips the compile).
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI = ["bias", "bias_silu", "bias_gelu", "posadd", "addsrc_silu", "gate_res", "qk_norm", "vT", "unpatch", "bias_row", "f32", "img", "dgelu",
       "qk_norm_rstd", "gate_res_split"]
GROUPS = (("slow-rate integer multiplies", ("v_mul_lo_u32", "v_mad_u64_u32", "v_mad_i64_i32", "v_mul_hi_u32")),
          ("cross-lane through LDS", ("ds_bpermute_b32",)),
          ("cross-lane on the VALU", ("v_permlane16_swap_b32", "v_permlane32_swap_b32")),
          ("waits", ("s_waitcnt", "s_nop")))


def compile_asm(src_dir, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-S", "--cuda-device-only",
           os.path.join(src_dir, "gemm.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"hipcc failed ({r.returncode}): {' '.join(cmd)}")


def kernels(lines):
    """{mangled name: (first, last) line index of the body}"""
    out, cur = {}, None
    for i, l in enumerate(lines):
        m = re.match(r"(_ZN5mi355\S*gemm_\w*kernel\S*):", l)
        if m:
            cur = (m.group(1), i)
        elif cur and l.startswith(".Lfunc_end"):
            out[cur[0]] = (cur[1], i)
            cur = None
    return out


def is_inst(l):
    s = l.strip()
    return bool(s) and s[0] not in ".;" and not s.endswith(":") and not s.startswith("//")


def w4_label(name):
    m = re.search(r"gemm_w4_kernelILi(\d+)ELi0E(?:Lb([01])E)?E", name)
    if not m:
        return None
    e = int(m.group(1))
    return (EPI[e] if e < len(EPI) else f"epi{e}") + (", tile-uniform" if m.group(2) == "1" else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "flow-factory_amd", "csrc"))
    ap.add_argument("--asm", default=None)
    ap.add_argument("--top", type=int, default=24)
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            compile_asm(args.src, os.path.join(d, "gemm.s"))
            text = open(os.path.join(d, "gemm.s")).read()
    lines = text.split("\n")
    ks = kernels(lines)
    print("== epilogue of gemm_w4_kernel<EPI, 0>: instructions behind the main loop, per output tile and wave")
    for name, (a, b) in ks.items():
        label = w4_label(name)
        if label is None:
            continue
        # the main loop is the inline-asm block that holds the MFMAs; everything after its end belongs to the epilogue
        last_mfma = max((i for i in range(a, b) if "v_mfma" in lines[i]), default=None)
        if last_mfma is None:
            continue
        end = next(i for i in range(last_mfma, b) if "#ASMEND" in lines[i])
        hist = collections.Counter(l.split()[0] for l in lines[end + 1:b] if is_inst(l))
        total = sum(hist.values())
        print(f"-- w4<{label}>: {total} instructions")
        for title, names in GROUPS:
            print(f"   {title}: " + ", ".join(f"{n} {hist.get(n, 0)}" for n in names))
        print("   " + ", ".join(f"{n} {c}" for n, c in hist.most_common(args.top)))
    print("== resources of every GEMM kernel (name: NumVgprs NumAgprs ScratchSize)")
    for name, (a, b) in ks.items():
        tail = "\n".join(lines[b:b + 60])
        v, ag, sc = (re.search(rf"; {k}: (\d+)", tail) for k in ("NumVgprs", "NumAgprs", "ScratchSize"))
        short = re.sub(r"^_ZN5mi35512_GLOBAL__N_1\d+", "", name).replace("EvNS_10GemmParamsE", "")
        print(f"   {short:44s} {v.group(1) if v else '?':>4s} {ag.group(1) if ag else '?':>4s} {sc.group(1) if sc else '?':>4s}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

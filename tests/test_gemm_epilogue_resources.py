"""Register and scratch budgets of the GEMM kernels (csrc/gemm.hip), read from the kernel descriptors of the built library with
`llvm-readelf --notes` (no GPU): the fused epilogues run with one or two waves per SIMD and nothing to hide a scratch reload behind, and the
hand-scheduled 4-wave loops own v120-v247 and every AGPR, so a register count that moves is a performance bug before it is anything else.

Budgets (`.vgpr_count` is the unified total: arch VGPRs rounded up to the accumulator offset, plus AGPRs):
  * gemm_w4_kernel / gemm_w6_kernel: one wave per SIMD, 512 unified registers (256 AGPR accumulators + at most 256 arch VGPRs); no scratch;
  * gemm_pp_kernel: 512 threads, two waves per SIMD: at most 256 unified registers; the tile-uniform epilogue builds (third template
    argument true, tune key 46) use no scratch and stay below the general builds' counts;
  * gemm_mid_kernel: __launch_bounds__(256, 2): at most 256; no scratch;
  * six general builds have spilled a few registers since before this test (GENERAL_SCRATCH: the ping-pong q / k and V^T scatters, which
    "sit at their register limit" (gemm.hip), and the 4-wave posadd / addsrc_silu / dgelu builds, which no shipped dispatch selects): their
    private segment may not grow beyond the recorded figures.  Every other production build -- the tile-uniform ones that replace the
    ping-pong scatters on the image grids among them -- is held to zero.  The ablation and trace builds (second template argument != 0:
    measurement only, some with deliberately broken code) are not production code and are left out.
"""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flow-factory_amd", "libmi355flow.so")

# general builds with a recorded spill: mangled-name fragment -> largest private segment (bytes per lane)
GENERAL_SCRATCH = {"gemm_pp_kernelILi6ELi0ELb0E": 12, "gemm_pp_kernelILi13ELi0ELb0E": 48, "gemm_pp_kernelILi7ELi0ELb0E": 8,
                   "gemm_w4_kernelILi3ELi0ELb0E": 12, "gemm_w4_kernelILi4ELi0ELb0E": 12, "gemm_w4_kernelILi12ELi0ELb0E": 28}
FAST_EPIS = (0, 1, 2, 5, 6, 7, 13)          # bias, bias_silu, bias_gelu, gate_res, qk_norm, vT, qk_norm_rstd


def _code_objects(path):
    """the gfx950 code objects of every offload bundle inside the shared library"""
    b = open(path, "rb").read()
    magic, out, i = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (i := b.find(magic, i)) >= 0:
        n, = struct.unpack_from("<Q", b, i + 24)
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", b, p)
            triple = b[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(b[i + off:i + off + size])
        i += len(magic)
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: (agpr, unified vgpr, spilled vgprs, private segment bytes)} of every gemm_*_kernel of gemm.hip"""
    readelf = shutil.which("llvm-readelf") or next((p for p in ("/opt/rocm/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-readelf") if os.path.exists(p)), None)
    if readelf is None:
        pytest.skip("no llvm-readelf")
    assert os.path.exists(LIB), "build() has not run"
    tmp = tmp_path_factory.mktemp("co")
    found = {}
    for n, co in enumerate(_code_objects(LIB)):
        f = tmp / f"co{n}.elf"
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if re.search(r"gemm_(w4|w6|pp|mid)_kernel", name):
                found[name] = (int(blk.split()[0]), int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                               int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return found


def _of(kernels, family):
    return {k: v for k, v in kernels.items() if f"gemm_{family}_kernel" in k}


def test_every_family_is_in_the_library(kernels):
    for fam, least in (("w4", 10), ("w6", 8), ("pp", 10), ("mid", 8)):
        assert len(_of(kernels, fam)) >= least, (fam, sorted(_of(kernels, fam)))
    # the tile-uniform builds of both 256x256 families, for every epilogue that has one
    # (the 4-wave kernel: only where the epilogue looks at the sample -- its bias / SiLU / GELU builds were measured and dropped)
    for fam, epis in (("w4", (5, 6, 7, 13)), ("pp", FAST_EPIS)):
        for e in epis:
            assert any(f"gemm_{fam}_kernelILi{e}ELi0ELb1E" in k for k in kernels), (fam, e)


def _production(name):
    """not one of the ablation / trace builds of the ping-pong and 4-wave kernels (second template argument != 0: measurement only)"""
    m = re.search(r"gemm_(?:pp|w4)_kernelILi\d+ELi(\d+)E", name)
    return m is None or m.group(1) == "0"


def test_no_scratch(kernels):
    for name, (agpr, vgpr, spill, priv) in kernels.items():
        if not _production(name):
            continue
        allowed = next((v for frag, v in GENERAL_SCRATCH.items() if frag in name), 0)
        assert priv <= allowed and (spill == 0 or allowed), (name, agpr, vgpr, spill, priv)


def test_register_budgets(kernels):
    for name, (agpr, vgpr, spill, priv) in _of(kernels, "w4").items():
        assert agpr == 256 and vgpr - agpr <= 256, (name, agpr, vgpr)          # the asm loop's clobber list names v247 and a255
    for name, (agpr, vgpr, spill, priv) in _of(kernels, "w6").items():
        assert vgpr <= 512, (name, agpr, vgpr)
    for fam in ("pp", "mid"):
        for name, (agpr, vgpr, spill, priv) in _of(kernels, fam).items():
            assert vgpr <= 256, (name, agpr, vgpr)          # two waves per SIMD


def test_tile_uniform_builds_need_fewer_registers_than_the_general_ones(kernels):
    """gemm_pp<gate_res> is at 253 of 256: the tile-uniform builds drop the per-row 64-bit addresses and must not climb back to the limit"""
    pp = _of(kernels, "pp")
    for e in FAST_EPIS:
        fast = next(v for k, v in pp.items() if f"gemm_pp_kernelILi{e}ELi0ELb1E" in k)
        gen = next(v for k, v in pp.items() if f"gemm_pp_kernelILi{e}ELi0ELb0E" in k)
        assert fast[1] <= gen[1] and fast[1] <= 253 and fast[2] == 0 and fast[3] == 0, (e, fast, gen)

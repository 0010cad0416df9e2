"""csrc/attn64_w4_asm.inc (the hand-scheduled key loop of attn64_w4_kernel) against its generator csrc/gen_attn64_w4.py: the committed file is
what the generator prints, the generator's structural checks pass, every register the loop names is declared to the compiler, and the built
kernels' descriptors allocate them."""
import contextlib
import importlib
import io
import os
import re
import shutil
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flow-factory_amd", "csrc")
INC = os.path.join(CSRC, "attn64_w4_asm.inc")


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, CSRC)
    try:
        return importlib.import_module("gen_attn64_w4")
    finally:
        sys.path.remove(CSRC)


def test_committed_inc_is_what_the_generator_emits(gen):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        gen.main()
    with open(INC) as f:
        assert f.read() == buf.getvalue(), "attn64_w4_asm.inc is stale: python3 gen_attn64_w4.py > attn64_w4_asm.inc"


def test_structural_checks_pass(gen):
    gen.check_all()
    # and they do catch what they are for: a wait that leaves the awaited fragment in flight, a read moved in front of its buffer's last MFMA
    body = gen.body_multi(unroll=2)
    i = next(n for n, ins in enumerate(body) if ins.startswith("s_waitcnt lgkmcnt(7)"))
    bad = list(body)
    bad[i] = gen.I("s_waitcnt lgkmcnt(8)", **body[i].meta)
    with pytest.raises(AssertionError):
        gen.check_stream(bad, 5)
    j = next(n for n, ins in enumerate(body) if ins.startswith("ds_read_b128") and getattr(ins, "meta", {}).get("tag", ("", 0))[0] == "V")
    m = max(n for n in range(j) if body[n].startswith("v_mfma") and body[n].meta["expect"][0] == "K")
    bad = list(body)
    bad.insert(m - 12, bad.pop(j))
    with pytest.raises(AssertionError):
        gen.check_stream(bad, 5)
    k = next(n for n, ins in enumerate(body) if ins.startswith("s_waitcnt vmcnt(4)"))
    bad = list(body)
    bad[k] = gen.I("s_waitcnt vmcnt(5)", **body[k].meta)
    with pytest.raises(AssertionError):
        gen.check_stream(bad, 5)


def test_registers_stay_inside_the_declared_budget(gen):
    text = open(INC).read()
    clob = set(re.findall(r'"([avs]\d+)"', next(ln for ln in text.splitlines() if ln.startswith("#define A64_CLOBBERS"))))
    assert clob == {f"a{i}" for i in range(gen.A_END)} | {f"v{i}" for i in range(gen.S_BASE, gen.V_END)} | {f"s{i}" for i in range(gen.S_LO, gen.S_HI)}
    named = set()
    for ln in text.splitlines():
        m = re.match(r'\s+"(.*)\\n" \\$', ln)
        if not m or m.group(1).startswith(("s_nop", "s_waitcnt", "L_", "s_cbranch")):
            continue
        for kind, lo, hi in re.findall(r"\b([vas])\[?(\d+)(?::(\d+))?\]?", m.group(1)):
            named |= {f"{kind}{i}" for i in range(int(lo), int(hi or lo) + 1)}
    assert named and named <= clob, sorted(named - clob)
    assert {f"a{gen.A_END - 1}", f"v{gen.V_END - 1}", f"v{gen.S_BASE}"} <= named


def _code_objects(path):
    """the gfx950 code objects of every offload bundle inside a host object / shared library"""
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


def test_kernel_descriptors_allocate_the_named_registers(gen, tmp_path):
    readelf = shutil.which("llvm-readelf") or next((p for p in ("/opt/rocm/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-readelf") if os.path.exists(p)), None)
    if readelf is None:
        pytest.skip("no llvm-readelf")
    lib = os.path.join(ROOT, "flow-factory_amd", "libmi355flow.so")
    assert os.path.exists(lib), "build() has not run"
    found = {}
    for n, co in enumerate(_code_objects(lib)):
        f = tmp_path / f"co{n}.elf"
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "attn64_w4_kernel" in name:
                found[name] = (int(blk.split()[0]), int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    assert len(found) >= 2, found            # the LSE and the rollout instantiation
    for name, (agpr, vgpr, spill) in found.items():
        # gfx90a and later: .vgpr_count is the unified total (arch VGPRs rounded up to the accumulator offset, + AGPRs)
        assert agpr >= gen.A_END and vgpr - agpr >= gen.V_END and spill == 0, (name, agpr, vgpr, spill)

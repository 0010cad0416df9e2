"""What every generator of a hand-scheduled loop (csrc/gen_*.py -> *_asm.inc) repeats: register names, the macro printers and the
MFMA / filler interleaver.  A generator builds a list of instructions and prints it as one C macro of string literals; the C++ shell wraps
the macro in an asm statement with the matching clobber list."""


def vr(b, n=1):
    return f"v[{b}:{b + n - 1}]" if n > 1 else f"v{b}"


def ar(b, n=1):
    return f"a[{b}:{b + n - 1}]" if n > 1 else f"a{b}"


def sr(b):
    return f"s[{b}:{b + 1}]"


def interleave(mfmas, fill):
    """one MFMA, then the instructions listed for its gap (fill: {MFMA index: [instructions]}), then the next MFMA ..."""
    out = []
    for i, m in enumerate(mfmas):
        out.append(m)
        out += fill.get(i, [])
    return out


def emit(name, lines):
    """`name` as one macro of string literals, an instruction each (an entry may hold several, joined by a literal backslash-n: they share a gap)"""
    print(f"#define {name} \\")
    for ln in lines:
        for part in ln.split("\\n"):
            print(f'    "{part}\\n" \\')
    print('    ""')
    print()


def regs(kind, lo, hi):
    return [f"{kind}{i}" for i in range(lo, hi)]


def clobbers(*names):
    """the clobber list of an asm statement: clobbers(*regs("v", 16, 160), "scc", "memory")"""
    return ", ".join(f'"{r}"' for r in names)


def read_acc_macros(prefix, bases):
    """accumulator read-out behind a loop: PREFIX_READ_ACC_<base>(d) fills f32x16 d from a[base : base + 16)"""
    for base in bases:
        rd = " ".join(f"v_accvgpr_read_b32 %{i}, a{base + i}\\n" for i in range(16))
        outs = ", ".join(f'"=v"(t_[{i}])' for i in range(16))
        print(f"#define {prefix}_READ_ACC_{base}(d) {{ float t_[16]; asm volatile(\"{rd}\" : {outs}); _Pragma(\"unroll\") for (int i_ = 0; i_ < 16; ++i_) d[i_] = t_[i_]; }}")

"""Lab: how long a kernel's prologue is, instruction by class, in a hipcc assembly listing (-S --cuda-device-only).

    python tools/isa_prologue.py LISTING.s KERNEL [--until PATTERN] [--list]

KERNEL selects the kernels whose (mangled) name contains it; for the v3 decode GEMV a template-argument tuple works too:
    --v3 NW,D,OUTL,MODE,BITS,MB,RSC,FL,XG[,KCT]     (gemv_v3_kernel<...>; without KCT: the run-time-K instance)
The prologue ends at the first instruction that contains PATTERN: v_mfma by default (the question the tool was first written for:
where the integer divisions of an attention prologue sit), global_load_dwordx4 for the first weight load of the decode GEMV's ring.
Per kernel one line: instructions ahead of that instruction (the kernarg-preload compatibility preamble included, as the listing
has it), of them LDS-DMA, branches, scalar / vector ALU, scalar loads, divisions (v_rcp_iflag), and the kernel's register counts
from its metadata.  --list prints the prologue itself."""
import argparse
import re


def kernels(text):
    """name -> instruction lines of every kernel of the listing."""
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        ins = [l.strip() for l in m.group(2).split("\n")]
        out[m.group(1)] = [l for l in ins if l and not l.startswith((";", ".")) and not l.endswith(":")]
    return out


def registers(text, name):
    """(vgpr, sgpr, agpr) of the kernel's `.set NAME.num_vgpr, N` lines (sgpr: the numbered ones, without VCC and the like)."""
    got = [re.search(r"\.set " + re.escape(name) + r"\." + f + r", (\d+)", text) for f in ("num_vgpr", "numbered_sgpr", "num_agpr")]
    return tuple(int(m.group(1)) for m in got) if all(got) else None


def v3_name(tup):
    """The mangled template-argument list of gemv_v3_kernel for NW,D,OUTL,MODE,BITS,MB,RSC,FL,XG[,KCT]."""
    v = [int(x) for x in tup.split(",")]
    assert len(v) in (9, 10), "NW,D,OUTL,MODE,BITS,MB,RSC,FL,XG[,KCT]"
    s = "".join(("Lb%dE" if i in (2, 7, 8) else "Li%dE") % x for i, x in enumerate(v[:9]))
    return "gemv_v3_kernelI" + s + ("Li%dEEEv" % v[9] if len(v) == 10 else "")


def prologue(ins, pattern):
    first = next((k for k, l in enumerate(ins) if pattern in l), len(ins))
    head = ins[:first]
    count = lambda f: sum(1 for l in head if f(l))
    return first, head, {
        "lds_dma": count(lambda l: "_load_lds_" in l or (l.startswith("buffer_load") and l.endswith(" lds"))),
        "branch": count(lambda l: l.startswith(("s_cbranch", "s_branch"))),
        "salu": count(lambda l: l.startswith("s_") and not l.startswith(("s_cbranch", "s_branch", "s_load", "s_waitcnt", "s_nop", "s_barrier"))),
        "valu": count(lambda l: l.startswith("v_")),
        "s_load": count(lambda l: l.startswith("s_load")),
        "s_nop": count(lambda l: l.startswith("s_nop")),
        "div": count(lambda l: "v_rcp_iflag" in l),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernel", nargs="?", default="")
    ap.add_argument("--v3", action="append", default=[], help="template arguments of a gemv_v3_kernel instance (repeatable)")
    ap.add_argument("--until", default="v_mfma", help="the instruction that ends the prologue (substring)")
    ap.add_argument("--list", action="store_true", help="print the prologue")
    a = ap.parse_args()
    text = open(a.listing).read()
    ks = kernels(text)
    keys = [v3_name(t) for t in a.v3] or [a.kernel]
    for key in keys:
        # (a run-time-K instance's argument list is a prefix of its compile-time-K siblings': end it where the list ends)
        hit = [n for n in ks if key in n and (key.endswith("EEEv") or not key.startswith("gemv_v3_kernelI") or (key + "EEv") in n or (key + "Li0EEEv") in n)]
        if not hit:
            print("no kernel matches", key)
        for n in hit:
            first, head, c = prologue(ks[n], a.until)
            regs = registers(text, n)
            print(f"{n[:110]}\n  before the first {a.until}: {first} of {len(ks[n])} instructions  "
                  + "  ".join(f"{k}={v}" for k, v in c.items())
                  + (f"  vgpr={regs[0]} sgpr={regs[1]} agpr={regs[2]}" if regs else ""))
            if a.list:
                print("\n".join("    " + l for l in head))


if __name__ == "__main__":
    main()

"""profiles/antithetic_isa.txt from two directories of AMDGPU listings (tools/isa_digests.py says how they are made: one unit.s per
translation unit, every -DMCP_NB for mcp_paths_inst.hip), the parent tree's and this tree's:
   python tools/antithetic_isa.py BEFORE AFTER > profiles/antithetic_isa.txt
Section 1 is tools/isa_digests.py's comparison per unit; section 2 lists every mc_paths_anti_kernel at NB = 4 and 16 next to its
twin without pairs: the compiler's figures, the scratch_ instructions of the kernel and of its loops, and the step loop's VALU."""
import os
import re
import sys
import textwrap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_digests import kernels, units  # noqa: E402

HEADER = [
    "Device listings (hipcc -S --cuda-device-only -O3 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function, gfx950) of "
    "mcp_paths_inst.hip at every -DMCP_NB=1..16, mcp_sweep_paths.hip parts 0..3, mcp_stats_kernels.hip and mcp_sweep_kernels.hip, of "
    "the parent tree and of this tree with the antithetic kernels (SPEC.md 2.3 / 5.10) added; written by tools/antithetic_isa.py.",
    "1. tools/isa_digests.py BEFORE AFTER per unit: the kernel symbols of the parent's listing, of this tree's, and how many of the "
    "parent's this tree keeps in all five figures (code digest, NumVgprs, ScratchSize, Occupancy, LDS).  The symbols this tree adds "
    "are the 18 mc_paths_anti_kernel instantiations per unit (isa_digests.py itself exits with status 1 for that reason).",
    "2. mc_paths_anti_kernel<NB, KT, 1, LOGC, A> at NB = 4 and NB = 16: registers, the private segment the compiler reserves "
    "(ScratchSize: on this compiler also the home of SGPRs parked in VGPR lanes, so it is not a count of accesses), occupancy as the "
    "compiler reports it, LDS, the scratch_ instructions of the whole kernel and of its loops (every span of a backward branch: the "
    "step loops and what encloses them), and the VGPRs / occupancy of the twin without pairs (A's base: the plain, drawdown or "
    "horizon kernel, or its GARCH twin).  The line below: the innermost loop with the most VALU (tools/isa_mix.py's step loop; for "
    "the GARCH walks the Gaussian side of the nu branch, see profiles/garch_isa.txt) of the kernel and of its twin, the ratio per "
    "pair and per path, and the packed fmas of that loop that carry a neg_lo / neg_hi source modifier (the second member's chain: "
    "fma(L, -z, r) costs no instruction of its own).  Where the compiler made the chi-block loop the innermost loop with the most "
    "VALU, on either side, the line reads `t loop`: the smallest loop that holds the Philox rounds, chi-block body and both sides "
    "of the nu branch included, on both sides.  No kernel has a scratch_ instruction in its step or t loop; where the whole kernel "
    "has some they sit in the epilogue, which the loop over the tiles encloses.",
]
# A of mc_paths_anti_kernel -> its twin without pairs: kernel name and the end of its mangled name ({lg}: the LOGC argument)
TWINS = {"PathArgsA": ("mc_paths_kernel", "Lb0ELb0E{lg}EEEvNS_8PathArgsE"), "PathArgsADD": ("mc_paths_dd_kernel", "{lg}EEEvNS_10PathArgsDDE"),
         "PathArgsAHZ": ("mc_paths_hz_kernel", "{lg}EEEvNS_10PathArgsHZE"), "PathArgsGA": ("mc_paths_g_kernel", "EEvNS_9PathArgsGE"),
         "PathArgsGADD": ("mc_paths_g_dd_kernel", "EEvNS_11PathArgsGDDE"), "PathArgsGAHZ": ("mc_paths_g_hz_kernel", "EEvNS_11PathArgsGHZE")}


def body(lines, sym):
    i = next(j for j, l in enumerate(lines) if l.startswith(sym + ":"))
    k = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
    return lines[i:k]


def is_scratch(line):
    return "scratch_" in line.split(";")[0] and not line.startswith(".")


def loops(bl):
    """every (first, last) line span of a backward branch"""
    labels = {l.split(":")[0]: i for i, l in enumerate(bl) if l.startswith(".LBB")}
    res = []
    for i, l in enumerate(bl):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\w+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            res.append((labels[m.group(1)], i))
    return res


def spans(bl):
    """(step, t): the innermost loop with the most VALU (tools/isa_mix.py's step loop) and the smallest loop that holds the Philox
    rounds (the loop over t with whatever the compiler rotated around it)"""
    lp = [(a, b) for a, b in loops(bl) if "s_cbranch" in bl[b]]
    inner = [(a, b) for a, b in lp if not any(a2 >= a and b2 <= b and (a2, b2) != (a, b) for a2, b2 in lp)]
    ph = [i for i, l in enumerate(bl) if "v_bitop3_b32" in l]          # the Philox rounds' three-way xors
    holds = lambda a, b: sum(1 for i in ph if a <= i <= b) >= 0.95 * len(ph)   # noqa: E731
    t = min(((a, b) for a, b in loops(bl) if holds(a, b)), key=lambda s: s[1] - s[0])
    return max(inner, key=lambda s: count(bl, s)[0]), t


def count(bl, span):
    """(VALU, packed fmas with a neg modifier, scratch_ instructions) of a span"""
    seg = bl[span[0]:span[1] + 1]
    return (sum(1 for l in seg if l.strip().startswith("v_")),
            sum(1 for l in seg if "v_pk_fma_f32" in l and ("neg_lo" in l or "neg_hi" in l)), sum(1 for l in seg if is_scratch(l)))


def main(before, after):
    out = []
    for para in HEADER:
        first, rest = ("# " + para[:3], para[3:]) if para[0].isdigit() else ("# ", para)
        out += textwrap.wrap(rest, 132, initial_indent=first, subsequent_indent="#    " if para[0].isdigit() else "# ")
    tot = [0, 0, 0]
    for u in units(after):
        b, a = kernels(os.path.join(before, u + ".s")), kernels(os.path.join(after, u + ".s"))
        keep = sum(1 for s in b if s in a and a[s] == b[s])
        out.append(f"## {u}.s: {len(b)} kernel symbols in the parent's listing, {len(a)} in this tree's; equal to the parent's in all five "
                   f"figures: {keep} of {len(b)}")
        tot = [tot[0] + len(b), tot[1] + len(a), tot[2] + keep]
    out.append(f"## all units: {tot[2]} of {tot[0]} parent kernels keep code digest, NumVgprs, ScratchSize, Occupancy and LDS; "
               f"{tot[1] - tot[0]} new symbols")
    out.append("## antithetic kernels: A LOGC NB KT | VGPRs | ScratchSize | occupancy | LDS B | scratch_ instructions: whole kernel, "
               "inside loops || twin: VGPRs occupancy")
    for nb in (4, 16):
        path = os.path.join(after, f"paths_nb{nb}.s")
        lines = open(path).read().split("\n")
        ks = kernels(path)
        for kt in (1, 8):
            for arg, (name, tail) in TWINS.items():
                for lg in (0, 1):
                    sym = next((s for s in ks if f"mc_paths_anti_kernelILi{nb}ELi{kt}ELi1ELb{lg}ENS_" in s
                                and s.endswith(f"{len(arg)}{arg}EEEvT3_")), None)
                    if sym is None:                      # the GARCH walks compound simply only
                        continue
                    tsym = next(s for s in ks if s.startswith(f"_ZN3mcp{len(name)}{name}ILi{nb}ELi{kt}ELi1E")
                                and s.endswith(tail.format(lg=f"Lb{lg}")))
                    d, td, bl, tb = ks[sym], ks[tsym], body(lines, sym), body(lines, tsym)
                    in_loops = {i for a, b in loops(bl) for i in range(a, b + 1) if is_scratch(bl[i])}
                    out.append(f"{arg:13s} {lg} {nb:2d} {kt} | {d[2]:3d} | {d[3]:3d} | {d[4]} | {d[5]:5d} | {sum(map(is_scratch, bl)):2d} "
                               f"{len(in_loops):2d} || {td[2]:3d} {td[4]}   digest {d[0]} ({d[1]} instructions)")
                    (sa, ta), (st, tt) = spans(bl), spans(tb)
                    # the step loop, unless on either side the compiler made the chi-block loop the innermost loop with the most VALU
                    # (it then holds less than half of the t loop's VALU): then the t loop on both sides
                    whole = count(bl, sa)[0] < count(bl, ta)[0] / 2 or count(tb, st)[0] < count(tb, tt)[0] / 2
                    va, neg, scl = count(bl, ta if whole else sa)
                    vt = count(tb, tt if whole else st)[0]
                    out.append(f"    {'t loop' if whole else 'step loop'}: VALU {va}  scratch_ {scl}  v_pk_fma_f32 with neg_lo/neg_hi {neg} "
                               f"|| twin: VALU {vt}  (per pair x{va / vt:.3f}, per path x{va / vt / 2:.3f})")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

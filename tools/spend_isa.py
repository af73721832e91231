"""profiles/spend_isa.txt from two directories of AMDGPU listings (tools/isa_digests.py says how they are made: one unit.s per
translation unit; mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16), the parent tree's and this tree's:
   python tools/spend_isa.py BEFORE AFTER > profiles/spend_isa.txt
Section 1 is tools/isa_digests.py's comparison per unit; section 2 lists mc_paths_spend_kernel at those NB, KT = 1 and 8 and its four
draw variants next to the mc_paths_cf_kernel twin of the same template arguments: the compiler's figures, the scratch_ instructions of
the kernel and of its walk, and the step loop's instruction mix."""
import os
import re
import sys
import textwrap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from antithetic_isa import body, count, is_scratch, spans  # noqa: E402
from isa_digests import kernels, units  # noqa: E402

HEADER = [
    "Device listings (hipcc -S --cuda-device-only -O3 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function, gfx950) of "
    "mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16, mcp_sweep_paths.hip parts 0..3, mcp_stats_kernels.hip and mcp_sweep_kernels.hip, of "
    "the parent tree and of this tree with the spending kernels (SPEC.md 4.16) added; written by tools/spend_isa.py.",
    "1. tools/isa_digests.py BEFORE AFTER per unit: the kernel symbols of the parent's listing, of this tree's, and how many of the "
    "parent's this tree keeps in all five figures (code digest, NumVgprs, ScratchSize, Occupancy, LDS).  The symbols this tree adds "
    "are the 8 spending instantiations per unit (four draw variants, KT = 1 and 8).",
    "2. mc_paths_spend_kernel<NB, KT, 1, BOOT, BLDS, STT> (gauss: 0 0 0, t: 0 0 1, boot in LDS: 1 1 0, boot in global memory: 1 0 0): "
    "SGPRs, VGPRs, the private segment the compiler reserves (ScratchSize: on this compiler also the home of SGPRs parked in VGPR "
    "lanes, so it is not a count of accesses), occupancy as the compiler reports it, the scratch_ instructions of the whole kernel and "
    "of the walk (the smallest loop that holds the Philox rounds: the loop over t), and the SGPRs / VGPRs / ScratchSize / occupancy of "
    "the mc_paths_cf_kernel twin.  The line below: the innermost loop with the most VALU (tools/isa_mix.py's step loop; `t loop` where "
    "on either side that is the Student-t chi-block loop: then the smallest loop that holds the Philox rounds, on both sides) of the "
    "kernel and of its twin -- VALU, SALU (s_ without the waits, branches and loads), scalar loads (s_load / s_buffer_load), "
    "scratch_ -- and the VALU ratio, the yardstick of tools/spend_probe.py.  The spans are ranges of lines of the listing: where the "
    "compiler lays the code between two segments of the walk (the horizon store, the review) inside the range its step loop's backward "
    "branch covers, that code is counted with the loop.  The walk column (the loop over t) has no scratch_ instruction in any kernel: "
    "at NB <= 4 the kernels are bounded at 6 waves per SIMD (KT = 1, MCP_MIN_WAVES_SP) and at 4 (KT = 8, MCP_MIN_WAVES_SP8; the twin "
    "runs 5 there, the 16 registers of w and Y do not fit 96).  The rule's step is, per (path, portfolio), a subtract, one compare, a "
    "max (with the v_max that quiets a NaN in front of it), two selects and an add where the twin has an add, two compares and a "
    "select: +3 VALU at KT = 1 in every kernel at NB <= 4; the schedule's two scalar loads per step are gone.  At KT = 8 the counts "
    "also hold the v_readlane / v_writelane of scalars the compiler parks in VGPR lanes (48 per step in the Gaussian kernel at NB = 4, "
    "12 in its twin; 84 in the bootstrap kernels, whose twins park almost none), and at NB = 13, 16 register allocation moves them "
    "both ways.",
]
VARIANTS = (("gauss", "Lb0ELb0ELb0E"), ("t", "Lb0ELb0ELb1E"), ("boot_lds", "Lb1ELb1ELb0E"), ("boot_global", "Lb1ELb0ELb0E"))


def sgprs(lines, sym):
    i = next(j for j, l in enumerate(lines) if l.startswith(sym + ":"))
    k = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
    for x in lines[k:k + 200]:
        m = re.match(r"\s*; (?:TotalNumSgprs|NumSgprs): (\d+)", x)
        if m:
            return int(m.group(1))
    return -1


def mix(bl, span):
    """(VALU, SALU, scalar loads, scratch_) of a span"""
    seg = [l.split(";")[0].strip() for l in bl[span[0]:span[1] + 1]]
    sload = sum(1 for l in seg if l.startswith(("s_load", "s_buffer_load")))
    salu = sum(1 for l in seg if l.startswith("s_") and not l.startswith(("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_branch",
                                                                          "s_cbranch", "s_barrier")))
    return count(bl, span)[0], salu, sload, count(bl, span)[2]


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
    out.append("## spending kernels: variant NB KT | SGPRs VGPRs | ScratchSize | occupancy | scratch_ instructions: whole kernel, walk "
               "|| mc_paths_cf_kernel twin: SGPRs VGPRs ScratchSize occupancy")
    for nb in (1, 4, 13, 16):
        path = os.path.join(after, f"paths_nb{nb}.s")
        lines = open(path).read().split("\n")
        ks = kernels(path)
        for name, args in VARIANTS:
            for kt in (1, 8):
                sym = f"_ZN3mcp21mc_paths_spend_kernelILi{nb}ELi{kt}ELi1E{args}EEvNS_10PathArgsSPE"
                tsym = f"_ZN3mcp18mc_paths_cf_kernelILi{nb}ELi{kt}ELi1E{args}EEvNS_10PathArgsCFE"
                d, td, bl, tb = ks[sym], ks[tsym], body(lines, sym), body(lines, tsym)
                (sa, ta), (st, tt) = spans(bl), spans(tb)
                out.append(f"{name:11s} {nb:2d} {kt} | {sgprs(lines, sym):3d} {d[2]:3d} | {d[3]:3d} | {d[4]} | {sum(map(is_scratch, bl)):2d} "
                           f"{count(bl, ta)[2]:2d} || {sgprs(lines, tsym):3d} {td[2]:3d} {td[3]:3d} {td[4]}   digest {d[0]} ({d[1]} instructions)")
                whole = count(bl, sa)[0] < count(bl, ta)[0] / 2 or count(tb, st)[0] < count(tb, tt)[0] / 2
                ma, mt = mix(bl, ta if whole else sa), mix(tb, tt if whole else st)
                out.append(f"    {'t loop' if whole else 'step loop'}: VALU {ma[0]}  SALU {ma[1]}  scalar loads {ma[2]}  scratch_ {ma[3]} || twin: "
                           f"VALU {mt[0]}  SALU {mt[1]}  scalar loads {mt[2]}  scratch_ {mt[3]}  (VALU ratio {ma[0] / mt[0]:.3f}, {ma[0] - mt[0]:+d})")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

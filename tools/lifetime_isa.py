"""profiles/lifetime_isa.txt from two directories of AMDGPU listings (tools/isa_digests.py says how they are made: one unit.s per
translation unit; mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16, and mcp_stats_kernels.hip), the parent tree's and this tree's:
   python tools/lifetime_isa.py BEFORE AFTER > profiles/lifetime_isa.txt
Section 1 is tools/isa_digests.py's comparison per unit; section 2 lists the lifetime twins (mc_paths_glide_life_kernel,
mc_paths_spend_life_kernel) at those NB, KT = 1 and 8 and their four draw variants next to the kernel each is the twin of: the
compiler's figures, the scratch_ instructions of the kernel and of its walk, and the step loop's instruction mix."""
import os
import sys
import textwrap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from antithetic_isa import body, count, is_scratch, spans  # noqa: E402
from isa_digests import kernels, units  # noqa: E402
from spend_isa import VARIANTS, mix, sgprs  # noqa: E402

HEADER = [
    "Device listings (hipcc -S --cuda-device-only -O3 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function, gfx950) of "
    "mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16 and of mcp_stats_kernels.hip, of the parent tree and of this tree with the lifetime "
    "twins (SPEC.md 4.17) and the lifetime histogram (SPEC.md 5.17) added; written by tools/lifetime_isa.py.",
    "1. tools/isa_digests.py BEFORE AFTER per unit: the kernel symbols of the parent's listing, of this tree's, and how many of the "
    "parent's this tree keeps in all five figures (code digest, NumVgprs, ScratchSize, Occupancy, LDS).  The symbols this tree adds "
    "are the 16 twins per unit (two walks, four draw variants, KT = 1 and 8) and the two instances of life_hist_kernel.",
    "2. The twins <NB, KT, 1, BOOT, BLDS, STT> (gauss: 0 0 0, t: 0 0 1, boot in LDS: 1 1 0, boot in global memory: 1 0 0): SGPRs, VGPRs, "
    "the private segment the compiler reserves (ScratchSize: on this compiler also the home of SGPRs parked in VGPR lanes, so it is "
    "not a count of accesses), occupancy as the compiler reports it, the scratch_ instructions of the whole kernel and of the walk "
    "(the smallest loop that holds the Philox rounds: the loop over t), and the same figures of the original.  The line below: the "
    "innermost loop with the most VALU (tools/isa_mix.py's step loop; `t loop` where on either side that is the Student-t chi-block "
    "loop: then the smallest loop that holds the Philox rounds, on both sides) of the twin and of its original -- VALU, SALU, scalar "
    "loads, scratch_ -- and the VALU ratio, the expectation tools/lifetime_probe.py's measured ratios are held against.  The counter "
    "costs, per (path, portfolio) and step, one VALU add on the mask the step's select already uses (v_addc_co_u32 with a zero "
    "addend, or v_cndmask + v_add where the compiler keeps the mask in a VGPR) and one register: +1 VALU per step at KT = 1 and +8 in "
    "the Gaussian glide twin at KT = 8, NB <= 4; elsewhere at KT = 8 register allocation moves the v_readlane / v_writelane of parked "
    "scalars both ways.  Both twins keep their originals' launch bounds, so the occupancy columns differ only where the compiler's own "
    "register count crosses a step.  The one scratch_ instruction in the step-loop line of the Student-t glide twin at NB = 4, KT = 1 is "
    "the original's (profiles/glide_isa.txt: a reload the compiler lays between two segments of the walk, inside the range the step "
    "loop's backward branch covers); the walk column (the loop over t) has no scratch_ instruction in any twin.",
]
PAIRS = (("glide", "_ZN3mcp26mc_paths_glide_life_kernelILi{nb}ELi{kt}ELi1E{a}EEvNS_11PathArgsGPLE", "_ZN3mcp21mc_paths_glide_kernelILi{nb}ELi{kt}ELi1E{a}EEvNS_10PathArgsGPE"),
         ("spend", "_ZN3mcp26mc_paths_spend_life_kernelILi{nb}ELi{kt}ELi1E{a}EEvNS_11PathArgsSPLE", "_ZN3mcp21mc_paths_spend_kernelILi{nb}ELi{kt}ELi1E{a}EEvNS_10PathArgsSPE"))


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
    ks = kernels(os.path.join(after, "stats_kernels.s"))
    for sym in sorted(s for s in ks if "life_hist" in s):
        d = ks[sym]
        out.append(f"## {sym}: {d[1]} instructions, NumVgprs {d[2]}, ScratchSize {d[3]}, Occupancy {d[4]}, LDS {d[5]} B")
    out.append("## lifetime twins: walk variant NB KT | SGPRs VGPRs | ScratchSize | occupancy | scratch_ instructions: whole kernel, walk "
               "|| the original: SGPRs VGPRs ScratchSize occupancy, scratch_ in its walk")
    worst = 0
    for nb in (1, 4, 13, 16):
        path = os.path.join(after, f"paths_nb{nb}.s")
        lines = open(path).read().split("\n")
        ks = kernels(path)
        for walk, fsym, ftwin in PAIRS:
            for name, args in VARIANTS:
                for kt in (1, 8):
                    sym, tsym = fsym.format(nb=nb, kt=kt, a=args), ftwin.format(nb=nb, kt=kt, a=args)
                    d, td, bl, tb = ks[sym], ks[tsym], body(lines, sym), body(lines, tsym)
                    (sa, ta), (st, tt) = spans(bl), spans(tb)
                    worst = max(worst, count(bl, ta)[2])
                    out.append(f"{walk} {name:11s} {nb:2d} {kt} | {sgprs(lines, sym):3d} {d[2]:3d} | {d[3]:3d} | {d[4]} | {sum(map(is_scratch, bl)):2d} "
                               f"{count(bl, ta)[2]:2d} || {sgprs(lines, tsym):3d} {td[2]:3d} {td[3]:3d} {td[4]} {count(tb, tt)[2]:2d}   digest {d[0]} "
                               f"({d[1]} instructions)")
                    whole = count(bl, sa)[0] < count(bl, ta)[0] / 2 or count(tb, st)[0] < count(tb, tt)[0] / 2
                    ma, mt = mix(bl, ta if whole else sa), mix(tb, tt if whole else st)
                    out.append(f"    {'t loop' if whole else 'step loop'}: VALU {ma[0]}  SALU {ma[1]}  scalar loads {ma[2]}  scratch_ {ma[3]} || original: "
                               f"VALU {mt[0]}  SALU {mt[1]}  scalar loads {mt[2]}  scratch_ {mt[3]}  (VALU ratio {ma[0] / mt[0]:.3f}, {ma[0] - mt[0]:+d})")
    out.append(f"## the most scratch_ instructions in the walk of any twin listed: {worst}")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

"""profiles/band_isa.txt from two directories of AMDGPU listings (tools/isa_digests.py says how they are made: one unit.s per
translation unit; mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16), the parent tree's and this tree's:
   python tools/band_isa.py BEFORE AFTER > profiles/band_isa.txt
Section 1 is tools/isa_digests.py's comparison per unit; section 2 lists mc_paths_band_kernel at those NB and its three draw variants
next to the mc_paths_reb_kernel<NB, 1, 1, ...> of the same draws: the compiler's figures, the scratch_ instructions of the kernel and
of its walk, and the step loop's instruction mix."""
import os
import sys
import textwrap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from antithetic_isa import body, count, is_scratch, loops, spans  # noqa: E402
from isa_digests import kernels, units  # noqa: E402
from spend_isa import mix, sgprs  # noqa: E402

HEADER = [
    "Device listings (hipcc -S --cuda-device-only -O3 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function, gfx950) of "
    "mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16, of the parent tree and of this tree with the tolerance-band kernel (SPEC.md 4.18) "
    "added; written by tools/band_isa.py.",
    "1. tools/isa_digests.py BEFORE AFTER per unit: the kernel symbols of the parent's listing, of this tree's, and how many of the "
    "parent's this tree keeps in all five figures (code digest, NumVgprs, ScratchSize, Occupancy, LDS).  The symbols this tree adds "
    "are the 3 instances of mc_paths_band_kernel per unit (Gaussian draws, bootstrap rows in LDS and in global memory; one portfolio).",
    "2. mc_paths_band_kernel<NB, 1, 1, BOOT, BLDS> (gauss: 0 0, boot in LDS: 1 1, boot in global memory: 1 0): SGPRs, VGPRs, the private "
    "segment the compiler reserves (ScratchSize: on this compiler also the home of SGPRs parked in VGPR lanes, so it is not a count of "
    "accesses), occupancy as the compiler reports it, the scratch_ instructions of the whole kernel, of the walk (the smallest loop "
    "that holds the Philox rounds: the loop over t) and, in brackets, of every loop around that one, the smallest first (the loops over "
    "the events of the segmented walk -- the reviews, the horizon stores -- then the back edges of the loop over the grid-stride "
    "tiles), and the same figures of mc_paths_reb_kernel<NB, 1, 1, BOOT, BLDS>.  The line below: the innermost "
    "loop with the most VALU (tools/isa_mix.py's step loop) of the kernel and of the rebalancing kernel -- VALU, SALU, scalar loads, "
    "scratch_ -- and the VALU ratio; where the compiler rotates the segmented walk into one loop (the bootstrap kernels at NB >= 4, the "
    "Gaussian kernel at NB = 16) that span holds the event arms too, the review's unrolled compares with them, and the ratio says "
    "nothing about a step.  The step between events is the rebalancing kernel's: the review lives in the event arm, outside "
    "the step loop: at NB = 4 the Gaussian step loop is the rebalancing kernel's 403 VALU instruction for instruction.  Where "
    "ScratchSize is not 0 at NB <= 4 (the Gaussian kernel: two dwords more than the rebalancing kernel) the two reloads sit in the loop over "
    "the tiles, one in front of the walk and one behind it, once per tile: the loops over the events show 0.  The band kernel keeps the rebalancing kernel's launch "
    "bounds (MCP_MIN_WAVES_REB at NB <= 4).",
]


def around(bl, t):
    """the scratch_ instructions of every loop around the loop over t, the smallest loop first: the segmented walk's loops over the
    events, then the back edges of the loop over the grid-stride tiles"""
    spans_ = sorted(((a, b) for a, b in loops(bl) if a <= t[0] and b >= t[1] and (a, b) != t), key=lambda s: s[1] - s[0])
    return [count(bl, s)[2] for s in spans_]


VARIANTS = (("gauss", "Lb0ELb0E"), ("boot_lds", "Lb1ELb1E"), ("boot_global", "Lb1ELb0E"))


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
    out.append("## band kernels: variant NB | SGPRs VGPRs | ScratchSize | occupancy | scratch_ instructions: whole kernel, walk, [loops around the walk] "
               "|| mc_paths_reb_kernel: SGPRs VGPRs ScratchSize occupancy, scratch_ in its walk")
    worst = 0
    for nb in (1, 4, 13, 16):
        path = os.path.join(after, f"paths_nb{nb}.s")
        lines = open(path).read().split("\n")
        ks = kernels(path)
        for name, args in VARIANTS:
            sym = f"_ZN3mcp20mc_paths_band_kernelILi{nb}ELi1ELi1E{args}EEvNS_10PathArgsTBE"
            tsym = f"_ZN3mcp19mc_paths_reb_kernelILi{nb}ELi1ELi1E{args}EEvNS_10PathArgsRBE"
            d, td, bl, tb = ks[sym], ks[tsym], body(lines, sym), body(lines, tsym)
            (sa, ta), (st, tt) = spans(bl), spans(tb)
            worst = max(worst, count(bl, ta)[2])
            out.append(f"{name:11s} {nb:2d} | {sgprs(lines, sym):3d} {d[2]:3d} | {d[3]:3d} | {d[4]} | {sum(map(is_scratch, bl)):2d} "
                       f"{count(bl, ta)[2]:2d} {around(bl, ta)} || {sgprs(lines, tsym):3d} {td[2]:3d} {td[3]:3d} {td[4]} {count(tb, tt)[2]:2d}   digest {d[0]} "
                       f"({d[1]} instructions; the rebalancing kernel {td[1]})")
            ma, mt = mix(bl, sa), mix(tb, st)
            out.append(f"    step loop: VALU {ma[0]}  SALU {ma[1]}  scalar loads {ma[2]}  scratch_ {ma[3]} || rebalancing kernel: "
                       f"VALU {mt[0]}  SALU {mt[1]}  scalar loads {mt[2]}  scratch_ {mt[3]}  (VALU ratio {ma[0] / mt[0]:.3f}, {ma[0] - mt[0]:+d})")
    out.append(f"## the most scratch_ instructions in the walk of any band kernel listed: {worst}")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

"""profiles/underwater_isa.txt from two directories of AMDGPU listings (tools/isa_digests.py says how they are made: one unit.s per
translation unit; mcp_paths_inst.hip at -DMCP_NB=1, 4 and 16), the parent tree's and this tree's:
   python tools/underwater_isa.py BEFORE AFTER > profiles/underwater_isa.txt
Section 1 is tools/isa_digests.py's comparison per unit; section 2 lists the four under-water twins at those NB, KT = 1 and 8 --
mc_paths_uw_kernel (simple and log), mc_paths_g_uw_kernel, mc_paths_j_uw_kernel -- next to the drawdown kernel each one is the twin
of: the compiler's figures, the scratch_ instructions of the kernel and of its walk, and the step loop's instruction mix.  Symbol
digests and resource figures only."""
import os
import sys
import textwrap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from antithetic_isa import body, count, is_scratch, spans  # noqa: E402
from glide_isa import mix, sgprs  # noqa: E402
from isa_digests import kernels, units  # noqa: E402

HEADER = [
    "Device listings (hipcc -S --cuda-device-only -O3 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function, gfx950) of "
    "mcp_paths_inst.hip at -DMCP_NB=1, 4 and 16, mcp_sweep_paths.hip parts 0..3, mcp_stats_kernels.hip and mcp_sweep_kernels.hip, of the "
    "parent tree and of this tree with the under-water twins of the drawdown kernels (SPEC.md 4.20) added; written by "
    "tools/underwater_isa.py.",
    "1. tools/isa_digests.py BEFORE AFTER per unit: the kernel symbols of the parent's listing, of this tree's, and how many of the "
    "parent's this tree keeps in all five figures (code digest, NumVgprs, ScratchSize, Occupancy, LDS).  The symbols this tree adds "
    "are the 8 under-water instantiations per path unit (Gaussian simple, Gaussian log, GARCH walk, jump walk; KT = 1 and 8).",
    "2. The twins (uw: mc_paths_uw_kernel<.., false>; uw log: <.., true>; g uw: mc_paths_g_uw_kernel, the GARCH walk, which also serves "
    "Student-t requests; j uw: mc_paths_j_uw_kernel): SGPRs, VGPRs, the private segment the compiler reserves (ScratchSize: on this "
    "compiler also the home of SGPRs parked in VGPR lanes, so it is not a count of accesses), occupancy as the compiler reports it "
    "(waves per SIMD), the scratch_ instructions of the whole kernel and of the walk (the smallest loop that holds the Philox rounds: "
    "the loop over t), and the SGPRs / VGPRs / ScratchSize / occupancy of the parent (mc_paths_dd_kernel, mc_paths_g_dd_kernel, "
    "mc_paths_j_dd_kernel of the same NB, KT and compounding).  A twin at fewer waves per SIMD than its parent is marked `-1 wave` "
    "(or more) at the end of its line.  The line below: the innermost loop with the most VALU (tools/isa_mix.py's step loop; `t loop` "
    "where on either side that is the Student-t chi-block loop: then the smallest loop that holds the Philox rounds, on both sides) of "
    "the twin and of its parent -- VALU, SALU (s_ without the waits, branches and loads), scalar loads (s_load / s_buffer_load), "
    "scratch_ -- and the VALU ratio and difference.  The rule of SPEC.md 4.20 adds, behind the update of the peak, one compare against "
    "the peak just written, one add, one select and one integer max per path and portfolio; KT = 8 multiplies that by eight, and the "
    "counters take 2 KT VGPRs.  A scratch_ instruction inside a walk is listed here, not hidden.",
]
VARIANTS = (("uw", "_ZN3mcp18mc_paths_uw_kernelILi{nb}ELi{kt}ELi1ELb0EEE", "_ZN3mcp18mc_paths_dd_kernelILi{nb}ELi{kt}ELi1ELb0EEEvNS_10PathArgsDDE"),
            ("uw log", "_ZN3mcp18mc_paths_uw_kernelILi{nb}ELi{kt}ELi1ELb1EEE", "_ZN3mcp18mc_paths_dd_kernelILi{nb}ELi{kt}ELi1ELb1EEEvNS_10PathArgsDDE"),
            ("g uw", "_ZN3mcp20mc_paths_g_uw_kernelILi{nb}ELi{kt}ELi1EEE", "_ZN3mcp20mc_paths_g_dd_kernelILi{nb}ELi{kt}ELi1EEEvNS_11PathArgsGDDE"),
            ("j uw", "_ZN3mcp20mc_paths_j_uw_kernelILi{nb}ELi{kt}ELi1EEE", "_ZN3mcp20mc_paths_j_dd_kernelILi{nb}ELi{kt}ELi1EEEvNS_11PathArgsJDDE"))


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
    out.append("## under-water twins: variant NB KT | SGPRs VGPRs | ScratchSize | occupancy | scratch_ instructions: whole kernel, walk "
               "|| parent: SGPRs VGPRs ScratchSize occupancy")
    for nb in (1, 4, 16):
        path = os.path.join(after, f"paths_nb{nb}.s")
        lines = open(path).read().split("\n")
        ks = kernels(path)
        for name, pat, tpat in VARIANTS:
            for kt in (1, 8):
                sym = next(s for s in ks if s.startswith(pat.format(nb=nb, kt=kt)))
                tsym = tpat.format(nb=nb, kt=kt)
                d, td, bl, tb = ks[sym], ks[tsym], body(lines, sym), body(lines, tsym)
                (sa, ta), (st, tt) = spans(bl), spans(tb)
                lost = f"   {d[4] - td[4]:+d} wave{'s' if td[4] - d[4] > 1 else ''} per SIMD" if d[4] < td[4] else ""
                out.append(f"{name:6s} {nb:2d} {kt} | {sgprs(lines, sym):3d} {d[2]:3d} | {d[3]:3d} | {d[4]} | {sum(map(is_scratch, bl)):2d} "
                           f"{count(bl, ta)[2]:2d} || {sgprs(lines, tsym):3d} {td[2]:3d} {td[3]:3d} {td[4]}   digest {d[0]} ({d[1]} instructions){lost}")
                whole = count(bl, sa)[0] < count(bl, ta)[0] / 2 or count(tb, st)[0] < count(tb, tt)[0] / 2
                ma, mt = mix(bl, ta if whole else sa), mix(tb, tt if whole else st)
                out.append(f"    {'t loop' if whole else 'step loop'}: VALU {ma[0]}  SALU {ma[1]}  scalar loads {ma[2]}  scratch_ {ma[3]} || parent: "
                           f"VALU {mt[0]}  SALU {mt[1]}  scalar loads {mt[2]}  scratch_ {mt[3]}  (VALU ratio {ma[0] / mt[0]:.3f}, {ma[0] - mt[0]:+d})")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

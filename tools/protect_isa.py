"""profiles/protect_isa.txt from two directories of AMDGPU listings (tools/isa_digests.py says how they are made: one unit.s per
translation unit; mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16), the parent tree's and this tree's:
   python tools/protect_isa.py BEFORE AFTER > profiles/protect_isa.txt
Section 1 is tools/isa_digests.py's comparison per unit; section 2 lists mc_paths_pi_kernel at those NB, KT = 1 and 8 and its four
variants (GARCH or jump walk, with or without the drawdown) next to the twin without protection -- mc_paths_g_hz_kernel,
mc_paths_g_dd_kernel, mc_paths_j_hz_kernel, mc_paths_j_dd_kernel of the same NB and KT: the compiler's figures, the scratch_
instructions of the kernel and of its walk, and the step loop's instruction mix; section 3 is count_kernel<BelowPair> next to
count_kernel<RuinedShort>."""
import os
import sys
import textwrap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from antithetic_isa import body, count, is_scratch, spans  # noqa: E402
from glide_isa import mix, sgprs  # noqa: E402
from isa_digests import kernels, units  # noqa: E402

HEADER = [
    "Device listings (hipcc -S --cuda-device-only -O3 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function, gfx950) of "
    "mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16, mcp_sweep_paths.hip parts 0..3, mcp_stats_kernels.hip and mcp_sweep_kernels.hip, of "
    "the parent tree and of this tree with the floor-protection kernels (SPEC.md 4.15) added; written by tools/protect_isa.py.",
    "1. tools/isa_digests.py BEFORE AFTER per unit: the kernel symbols of the parent's listing, of this tree's, and how many of the "
    "parent's this tree keeps in all five figures (code digest, NumVgprs, ScratchSize, Occupancy, LDS).  The symbols this tree adds "
    "are the 8 mc_paths_pi_kernel instantiations per path unit (GARCH or jump walk, with or without the drawdown, KT = 1 and 8) and "
    "count_kernel<BelowPair> in mcp_stats_kernels.hip.",
    "2. mc_paths_pi_kernel<NB, KT, 1, JP, DD> (g: the GARCH walk, which also serves Gaussian and Student-t requests; j: the jump walk; "
    "dd: with the drawdown state): SGPRs, VGPRs, the private segment the compiler reserves (ScratchSize: on this compiler also the home "
    "of SGPRs parked in VGPR lanes, so it is not a count of accesses), occupancy as the compiler reports it, the scratch_ instructions "
    "of the whole kernel and of the walk (the smallest loop that holds the Philox rounds: the loop over t), and the SGPRs / VGPRs / "
    "ScratchSize / occupancy of the twin without protection (mc_paths_g_hz_kernel, mc_paths_g_dd_kernel, mc_paths_j_hz_kernel, "
    "mc_paths_j_dd_kernel).  The line below: the innermost loop with the most VALU (tools/isa_mix.py's step loop; `t loop` where on "
    "either side that is the Student-t chi-block loop: then the smallest loop that holds the Philox rounds, on both sides) of the "
    "kernel and of its twin -- VALU, SALU (s_ without the waits, branches and loads), scalar loads (s_load / s_buffer_load), "
    "scratch_ -- and the VALU ratio and difference.  The rule of SPEC.md 4.15 replaces the twin's one fma per path and portfolio by: "
    "mul (theta M), max (F), sub (C), mul (m C), mul (b V), min, max (E), sub (V - E), fma (u), fma (V'), max (M') -- 11 VALU where "
    "the twin has 1, so +10 per portfolio of the pass plus what the compiler adds to quiet a NaN in front of a min or max "
    "(v_max_f32 x, x, x) and the moves around the scalar operands; KT = 8 multiplies the difference by eight.  One more VGPR per "
    "portfolio of the pass carries M.  The rule's scalar loads (S_t and the four constants) sit behind a scheduling barrier, after the "
    "weight dot: issued earlier they were live across the step's SGPR peak and the KT = 8 jump kernels parked scalars in VGPR lanes "
    "(about 130 v_readlane / v_writelane per step at NB = 4).  At NB <= 4, KT = 1 the jump-walk kernels take MCP_MIN_WAVES_PI = 5 "
    "(87 to 95 VGPRs, occupancy 5 where the twin has 6): at 6 waves they reloaded one spilled pair inside the step loop.  No kernel "
    "has a scratch_ instruction in its step loop or walk.",
    "3. count_kernel<BelowPair> next to count_kernel<RuinedShort> (mcp_stats_kernels.hip): the same ballot-and-popcount loop with two compares "
    "against the row's own thresholds.",
]
VARIANTS = (("g", 0, 0, "mc_paths_g_hz_kernel", "PathArgsGHZ"), ("g dd", 0, 1, "mc_paths_g_dd_kernel", "PathArgsGDD"),
            ("j", 1, 0, "mc_paths_j_hz_kernel", "PathArgsJHZ"), ("j dd", 1, 1, "mc_paths_j_dd_kernel", "PathArgsJDD"))


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
    out.append("## floor-protection kernels: variant NB KT | SGPRs VGPRs | ScratchSize | occupancy | scratch_ instructions: whole kernel, walk "
               "|| twin: SGPRs VGPRs ScratchSize occupancy")
    for nb in (1, 4, 13, 16):
        path = os.path.join(after, f"paths_nb{nb}.s")
        lines = open(path).read().split("\n")
        ks = kernels(path)
        for name, jp, dd, twin, targ in VARIANTS:
            for kt in (1, 8):
                sym = next(s for s in ks if s.startswith(f"_ZN3mcp18mc_paths_pi_kernelILi{nb}ELi{kt}ELi1ELb{jp}ELb{dd}EEE"))
                tsym = f"_ZN3mcp{len(twin)}{twin}ILi{nb}ELi{kt}ELi1EEEvNS_{len(targ)}{targ}E"
                d, td, bl, tb = ks[sym], ks[tsym], body(lines, sym), body(lines, tsym)
                (sa, ta), (st, tt) = spans(bl), spans(tb)
                out.append(f"{name:5s} {nb:2d} {kt} | {sgprs(lines, sym):3d} {d[2]:3d} | {d[3]:3d} | {d[4]} | {sum(map(is_scratch, bl)):2d} "
                           f"{count(bl, ta)[2]:2d} || {sgprs(lines, tsym):3d} {td[2]:3d} {td[3]:3d} {td[4]}   digest {d[0]} ({d[1]} instructions)")
                whole = count(bl, sa)[0] < count(bl, ta)[0] / 2 or count(tb, st)[0] < count(tb, tt)[0] / 2
                ma, mt = mix(bl, ta if whole else sa), mix(tb, tt if whole else st)
                out.append(f"    {'t loop' if whole else 'step loop'}: VALU {ma[0]}  SALU {ma[1]}  scalar loads {ma[2]}  scratch_ {ma[3]} || twin: "
                           f"VALU {mt[0]}  SALU {mt[1]}  scalar loads {mt[2]}  scratch_ {mt[3]}  (VALU ratio {ma[0] / mt[0]:.3f}, {ma[0] - mt[0]:+d})")
    path = os.path.join(after, "stats_kernels.s")
    ks = kernels(path)
    out.append("## count kernels: symbol | digest (instructions) NumVgprs ScratchSize Occupancy LDS")
    for s in sorted(ks):
        if "count_kernel" in s:                               # count_kernel<RuinedShort>, count_kernel<BelowPair>
            d = ks[s]
            out.append(f"{s} | {d[0]} ({d[1]}) {d[2]} {d[3]} {d[4]} {d[5]}")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

"""profiles/jump_isa.txt from two directories of AMDGPU listings (tools/isa_digests.py says how they are made: one unit.s per
translation unit; mcp_paths_inst.hip at -DMCP_NB=1, 4, 13 and 16), the parent tree's and this tree's:
   python tools/jump_isa.py BEFORE AFTER > profiles/jump_isa.txt
Section 1 is tools/isa_digests.py's comparison per unit; section 2 lists mc_paths_j_kernel, mc_paths_j_dd_kernel and
mc_paths_j_hz_kernel at those NB and KT = 1, 8 next to their twins without jumps: the compiler's figures, the scratch_ instructions
of the kernel and of its walk, and the step loop's VALU."""
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
    "the parent tree and of this tree with the jump-diffusion kernels (SPEC.md 2.5 / 4.12) added; written by tools/jump_isa.py.",
    "1. tools/isa_digests.py BEFORE AFTER per unit: the kernel symbols of the parent's listing, of this tree's, and how many of the "
    "parent's this tree keeps in all five figures (code digest, NumVgprs, ScratchSize, Occupancy, LDS).  The symbols this tree adds "
    "are the 6 jump-diffusion instantiations per unit (three kernels, KT = 1 and 8).",
    "2. mc_paths_j_kernel / mc_paths_j_dd_kernel / mc_paths_j_hz_kernel<NB, KT, 1>: SGPRs, VGPRs, the private segment the compiler "
    "reserves (ScratchSize: on this compiler also the home of SGPRs parked in VGPR lanes, so it is not a count of accesses), "
    "occupancy as the compiler reports it, the scratch_ instructions of the whole kernel and of the walk (the smallest loop that holds "
    "the Philox rounds: the loop over t), and the VGPRs / occupancy of the plain twin (mc_paths_kernel, mc_paths_dd_kernel, "
    "mc_paths_hz_kernel, simple compounding).  The line below: the innermost loop with the most VALU (tools/isa_mix.py's step loop) of "
    "the kernel and of its twin, and the ratio.",
]
KERNELS = {"mc_paths_j_kernel": ("9PathArgsJE", "mc_paths_kernel", "Lb0ELb0ELb0EEEvNS_8PathArgsE"),
           "mc_paths_j_dd_kernel": ("11PathArgsJDDE", "mc_paths_dd_kernel", "Lb0EEEvNS_10PathArgsDDE"),
           "mc_paths_j_hz_kernel": ("11PathArgsJHZE", "mc_paths_hz_kernel", "Lb0EEEvNS_10PathArgsHZE")}


def sgprs(lines, sym):
    i = next(j for j, l in enumerate(lines) if l.startswith(sym + ":"))
    k = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
    for x in lines[k:k + 200]:
        m = re.match(r"\s*; (?:TotalNumSgprs|NumSgprs): (\d+)", x)
        if m:
            return int(m.group(1))
    return -1


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
    out.append("## jump-diffusion kernels: kernel NB KT | SGPRs VGPRs | ScratchSize | occupancy | scratch_ instructions: whole kernel, "
               "walk || plain twin: VGPRs occupancy")
    for nb in (1, 4, 13, 16):
        path = os.path.join(after, f"paths_nb{nb}.s")
        lines = open(path).read().split("\n")
        ks = kernels(path)
        for name, (tail, twin, twin_tail) in KERNELS.items():
            for kt in (1, 8):
                sym = f"_ZN3mcp{len(name)}{name}ILi{nb}ELi{kt}ELi1EEEvNS_{tail}"
                tsym = next(s for s in ks if s.startswith(f"_ZN3mcp{len(twin)}{twin}ILi{nb}ELi{kt}ELi1E") and s.endswith(twin_tail))
                d, td, bl, tb = ks[sym], ks[tsym], body(lines, sym), body(lines, tsym)
                (sa, ta), (st, tt) = spans(bl), spans(tb)
                out.append(f"{name:21s} {nb:2d} {kt} | {sgprs(lines, sym):3d} {d[2]:3d} | {d[3]:3d} | {d[4]} | {sum(map(is_scratch, bl)):2d} "
                           f"{count(bl, ta)[2]:2d} || {td[2]:3d} {td[4]}   digest {d[0]} ({d[1]} instructions)")
                va, vt = count(bl, sa)[0], count(tb, st)[0]
                out.append(f"    step loop: VALU {va}  scratch_ {count(bl, sa)[2]} || twin: VALU {vt}  scratch_ {count(tb, st)[2]}  "
                           f"(ratio {va / vt:.3f}, {va - vt:+d})")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

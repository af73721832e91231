"""profiles/uncertain_isa.txt from two directories of AMDGPU listings (tools/isa_digests.py says how they are made: one unit.s per
translation unit; mcp_paths_inst.hip at -DMCP_NB=1, 4 and 16), the parent tree's and this tree's:
   python tools/uncertain_isa.py BEFORE AFTER > profiles/uncertain_isa.txt
Section 1 is tools/isa_digests.py's comparison per unit; section 2 lists the seven drift-uncertainty kernels at those NB, KT = 1 and 8 --
mc_paths_pu_kernel, mc_paths_pu_dd_kernel, mc_paths_pu_hz_kernel (simple and log) and mc_paths_pu_cf_kernel -- next to the kernel each
one is the twin of: the compiler's figures, the scratch_ instructions of the kernel and of its walk, and the step loop's instruction
mix.  Symbol digests and resource figures only."""
import os
import sys
import textwrap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from antithetic_isa import body, count, is_scratch, loops, spans  # noqa: E402
from glide_isa import mix, sgprs  # noqa: E402
from isa_digests import kernels, units  # noqa: E402

HEADER = [
    "Device listings (hipcc -S --cuda-device-only -O3 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function, gfx950) of "
    "mcp_paths_inst.hip at -DMCP_NB=1, 4 and 16, mcp_sweep_paths.hip parts 0..3, mcp_stats_kernels.hip and mcp_sweep_kernels.hip, of the "
    "parent tree and of this tree with the drift-uncertainty kernels (SPEC.md 2.7 / 4.21) added; written by tools/uncertain_isa.py.",
    "1. tools/isa_digests.py BEFORE AFTER per unit: the kernel symbols of the parent's listing, of this tree's, and how many of the "
    "parent's this tree keeps in all five figures (code digest, NumVgprs, ScratchSize, Occupancy, LDS).  The symbols this tree adds "
    "are the 14 drift-uncertainty instantiations per path unit (plain, drawdown and horizon walk, each simple and log, and the "
    "cash-flow walk; KT = 1 and 8).",
    "2. The kernels (pu: mc_paths_pu_kernel<.., false>; pu log: <.., true>; likewise pu dd, pu hz; pu cf: mc_paths_pu_cf_kernel): "
    "SGPRs, VGPRs, the private segment the compiler reserves (ScratchSize: on this compiler also the home of SGPRs parked in VGPR "
    "lanes, so it is not a count of accesses), occupancy as the compiler reports it (waves per SIMD), the scratch_ instructions of the "
    "whole kernel and of the walk (the largest loop inside the tile loop that holds the step loop: the loop over t, or over the "
    "horizons' segments around it), and the SGPRs / VGPRs "
    "/ ScratchSize / occupancy of the twin without the feature (mc_paths_kernel, mc_paths_dd_kernel, mc_paths_hz_kernel, "
    "mc_paths_cf_kernel on Gaussian draws, of the same NB, KT and compounding).  A kernel at fewer waves per SIMD than its twin is "
    "marked `-1 wave` (or more) at the end of its line.  The line below: the innermost loop with the most VALU (tools/isa_mix.py's "
    "step loop) of the kernel and of its twin -- VALU, SALU (s_ without the waits, branches and loads), scalar loads (s_load / "
    "s_buffer_load), scratch_ -- and the VALU ratio and difference.  The step itself gains nothing: the row pair starts from a register "
    "pair instead of an LDS read.  The setup (nb Philox blocks, 4 nb normals and one triangular chain per path) runs once per tile, "
    "outside every loop over t.  A scratch_ instruction inside a walk is listed here, not hidden.",
]
VARIANTS = (("pu", "_ZN3mcp18mc_paths_pu_kernelILi{nb}ELi{kt}ELi1ELb0EEE", "_ZN3mcp15mc_paths_kernelILi{nb}ELi{kt}ELi1ELb0ELb0ELb0EEE"),
            ("pu log", "_ZN3mcp18mc_paths_pu_kernelILi{nb}ELi{kt}ELi1ELb1EEE", "_ZN3mcp15mc_paths_kernelILi{nb}ELi{kt}ELi1ELb0ELb0ELb1EEE"),
            ("pu dd", "_ZN3mcp21mc_paths_pu_dd_kernelILi{nb}ELi{kt}ELi1ELb0EEE", "_ZN3mcp18mc_paths_dd_kernelILi{nb}ELi{kt}ELi1ELb0EEE"),
            ("pu dd log", "_ZN3mcp21mc_paths_pu_dd_kernelILi{nb}ELi{kt}ELi1ELb1EEE", "_ZN3mcp18mc_paths_dd_kernelILi{nb}ELi{kt}ELi1ELb1EEE"),
            ("pu hz", "_ZN3mcp21mc_paths_pu_hz_kernelILi{nb}ELi{kt}ELi1ELb0EEE", "_ZN3mcp18mc_paths_hz_kernelILi{nb}ELi{kt}ELi1ELb0EEE"),
            ("pu hz log", "_ZN3mcp21mc_paths_pu_hz_kernelILi{nb}ELi{kt}ELi1ELb1EEE", "_ZN3mcp18mc_paths_hz_kernelILi{nb}ELi{kt}ELi1ELb1EEE"),
            ("pu cf", "_ZN3mcp21mc_paths_pu_cf_kernelILi{nb}ELi{kt}ELi1EEE", "_ZN3mcp18mc_paths_cf_kernelILi{nb}ELi{kt}ELi1ELb0ELb0ELb0EEE"))


def walk_scratch(bl):
    """scratch_ instructions inside the walk.  These kernels draw Philox blocks outside the loop over t too (the setup), so the smallest
    loop that holds the Philox rounds is the tile loop, setup and epilogue included; the walk is the largest loop strictly inside it
    that holds the step loop -- the loop over t, or the loop over the horizons' segments around it."""
    step, tile = spans(bl)
    inside = [(a, b) for a, b in loops(bl) if a <= step[0] and b >= step[1] and a >= tile[0] and b <= tile[1] and (a, b) != tile]
    walk = max(inside, key=lambda s: s[1] - s[0]) if inside else step
    return count(bl, walk)[2]


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
    out.append("## drift-uncertainty kernels: variant NB KT | SGPRs VGPRs | ScratchSize | occupancy | scratch_ instructions: whole kernel, walk "
               "|| twin: SGPRs VGPRs ScratchSize occupancy")
    in_walk = 0
    for nb in (1, 4, 16):
        path = os.path.join(after, f"paths_nb{nb}.s")
        lines = open(path).read().split("\n")
        ks = kernels(path)
        for name, pat, tpat in VARIANTS:
            for kt in (1, 8):
                sym = next(s for s in ks if s.startswith(pat.format(nb=nb, kt=kt)))
                tsym = next(s for s in ks if s.startswith(tpat.format(nb=nb, kt=kt)))
                d, td, bl, tb = ks[sym], ks[tsym], body(lines, sym), body(lines, tsym)
                (sa, ta), (st, tt) = spans(bl), spans(tb)
                lost = f"   {d[4] - td[4]:+d} wave{'s' if td[4] - d[4] > 1 else ''} per SIMD" if d[4] < td[4] else ""
                in_walk += walk_scratch(bl)
                out.append(f"{name:9s} {nb:2d} {kt} | {sgprs(lines, sym):3d} {d[2]:3d} | {d[3]:4d} | {d[4]} | {sum(map(is_scratch, bl)):3d} "
                           f"{walk_scratch(bl):2d} || {sgprs(lines, tsym):3d} {td[2]:3d} {td[3]:4d} {td[4]}   digest {d[0]} ({d[1]} instructions){lost}")
                ma, mt = mix(bl, sa), mix(tb, st)
                out.append(f"    step loop: VALU {ma[0]}  SALU {ma[1]}  scalar loads {ma[2]}  scratch_ {ma[3]} || twin: "
                           f"VALU {mt[0]}  SALU {mt[1]}  scalar loads {mt[2]}  scratch_ {mt[3]}  (VALU ratio {ma[0] / mt[0]:.3f}, {ma[0] - mt[0]:+d})")
    out.append(f"## scratch_ instructions inside a walk, all {3 * 2 * len(VARIANTS)} listed kernels: {in_walk}")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

"""profiles/lean_probe.json from the two measurements of the lean Gaussian kernel (mc_paths_lean_kernel) against the kernel it
leaves in place:

  lab    python tools/kernel_lab.py run nolean lean nolean2 --rounds 8 > lab.txt      one process, interleaved rounds at the bench
         shape (10^6 paths x 16 assets x 252 steps, fused statistics epilogue); `nolean` and `nolean2` are two builds of the same
         flags, the A/A repeat
  bench  python bench.py --gpus 1 --steps 20 --warmup 3, two fresh processes of the parent tree and two of this tree, alternated;
         one file of JSON result lines per tree, in run order

  python tools/lean_probe.py lab.txt parent_bench.jsonl branch_bench.jsonl -o profiles/lean_probe.json

The bar (the gain must clear the noise): |1 - lean/nolean| of the lab medians at least three times the A/A spread
|1 - nolean2/nolean|."""
import argparse, json, re, statistics, sys


def lab_rounds(path):
    out = {}
    for line in open(path):
        m = re.match(r"\s*(\w+)\s+rounds \(ms\): (.*)", line)
        if m:
            out[m.group(1)] = [float(x) for x in m.group(2).split()]
    return out


def bench_lines(path):
    return [json.loads(l) for l in open(path) if l.lstrip().startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lab"); ap.add_argument("parent_bench"); ap.add_argument("branch_bench")
    ap.add_argument("--base", default="nolean"); ap.add_argument("--arm", default="lean"); ap.add_argument("--repeat", default="nolean2")
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    rounds = lab_rounds(a.lab)
    med = {n: statistics.median(t) for n, t in rounds.items()}
    ratio = med[a.arm] / med[a.base]
    aa = med[a.repeat] / med[a.base]
    parent, branch = bench_lines(a.parent_bench), bench_lines(a.branch_bench)
    pv, bv = [x["value"] for x in parent], [x["value"] for x in branch]
    out = {
        "what": "mc_paths_lean_kernel<4, false> against mc_paths_kernel<4,1,1,false,false,false> at the bench shape (10^6 paths x 16 "
                "assets x 252 steps, one portfolio, fused statistics epilogue), MI355X",
        "lab": {"command": f"python tools/kernel_lab.py run {a.base} {a.arm} {a.repeat} --rounds {len(rounds[a.base])}",
                "note": "one process, interleaved rounds, ms per launch (two launches per timed pair); the arms differ in the host's "
                        "routing alone (-DMCP_EXP_LEAN), the retained kernel's code is the parent's instruction for instruction "
                        "(profiles/lean_isa.txt)",
                "rounds_ms": rounds, "median_ms": med, "min_ms": {n: min(t) for n, t in rounds.items()},
                "ratio_arm_over_base": ratio, "aa_ratio_repeat_over_base": aa,
                "gain": 1.0 - ratio, "aa_spread": abs(1.0 - aa),
                "gain_over_aa_spread": (1.0 - ratio) / abs(1.0 - aa) if aa != 1.0 else None,
                "clears_three_times_the_aa_spread": (1.0 - ratio) >= 3.0 * abs(1.0 - aa)},
        "bench": {"command": "python bench.py --gpus 1 --steps 20 --warmup 3 (fresh processes, parent and branch alternated)",
                  "parent_paths_per_s": pv, "branch_paths_per_s": bv,
                  "parent_spread": max(pv) / min(pv) - 1.0, "branch_spread": max(bv) / min(bv) - 1.0,
                  "ratio_branch_over_parent_of_means": statistics.mean(bv) / statistics.mean(pv)},
    }
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

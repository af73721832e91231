"""profiles/icdf_centred_probe.json from the three measurements of the lean kernel's centred normal transform
(normal_icdf_centred on the binade-scaled table, MCP_EXP_ICDF_CENTRED) against the transform it replaces, by the protocol of
tools/lean_probe.py:

  lab      python tools/kernel_lab.py run base centred base2 --rounds 8 > lab.txt     one process, interleaved rounds at the bench
           shape; `base` and `base2` are two loads of the -DMCP_EXP_ICDF_CENTRED=0 build, the A/A repeat
  bench    python bench.py --gpus 1 --steps 20 --warmup 3, fresh processes of the parent tree and of this tree, alternated; one file
           of JSON result lines per tree, in run order; one --session per visit to a GPU (boxes differ by a few percent, so runs
           of different sessions are not pooled)
  profiled rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 3 --serial, one run
           per tree, no counters; the *_kernel_stats.csv of each (compared with each other only)

  python tools/icdf_centred_probe.py lab.txt parent_kernel_stats.csv branch_kernel_stats.csv --session parent.jsonl branch.jsonl
         [--session ...] -o profiles/icdf_centred_probe.json

The bars: the lab gain at least three times the A/A spread; the branch's bench mean above the parent's by more than three times
the parent's own run-to-run spread."""
import argparse, csv, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lean_probe import bench_lines, lab_rounds


def lean_row(path):
    for r in csv.DictReader(open(path)):
        if "mc_paths_lean_kernel" in r["Name"]:
            return {"name": r["Name"], "calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]),
                    "max_ns": float(r["MaxNs"])}
    raise SystemExit(f"no mc_paths_lean_kernel row in {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lab"); ap.add_argument("parent_stats"); ap.add_argument("branch_stats")
    ap.add_argument("--session", nargs=2, action="append", required=True, metavar=("PARENT_JSONL", "BRANCH_JSONL"))
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    rounds = lab_rounds(a.lab)
    med = {n: statistics.median(t) for n, t in rounds.items()}
    ratio, aa = med["centred"] / med["base"], med["base2"] / med["base"]
    sessions = []
    for parent_bench, branch_bench in a.session:
        pv, bv = [x["value"] for x in bench_lines(parent_bench)], [x["value"] for x in bench_lines(branch_bench)]
        p_spread = max(pv) / min(pv) - 1.0
        b_gain = statistics.mean(bv) / statistics.mean(pv) - 1.0
        sessions.append({"parent_paths_per_s": pv, "branch_paths_per_s": bv, "parent_spread": p_spread,
                         "branch_spread": max(bv) / min(bv) - 1.0, "gain_of_means": b_gain,
                         "every_branch_run_above_every_parent_run": min(bv) > max(pv),
                         "clears_three_times_the_parent_spread": b_gain > 3.0 * p_spread})
    pk, bk = lean_row(a.parent_stats), lean_row(a.branch_stats)
    out = {
        "what": "mc_paths_lean_kernel<4, false> on normal_icdf_centred and the binade-scaled LDS table (377 VALU per wave-step) against "
                "the same kernel on normal_icdf (393) at the bench shape (10^6 paths x 16 assets x 252 steps, one portfolio, fused "
                "statistics epilogue), MI355X",
        "lab": {"command": f"python tools/kernel_lab.py run base centred base2 --rounds {len(rounds['base'])}",
                "note": "one process, interleaved rounds, ms per launch (two launches per timed pair); the arms differ in "
                        "-DMCP_EXP_ICDF_CENTRED alone",
                "rounds_ms": rounds, "median_ms": med, "min_ms": {n: min(t) for n, t in rounds.items()},
                "ratio_centred_over_base": ratio, "aa_ratio_base2_over_base": aa, "gain": 1.0 - ratio, "aa_spread": abs(1.0 - aa),
                "gain_over_aa_spread": (1.0 - ratio) / abs(1.0 - aa) if aa != 1.0 else None,
                "clears_three_times_the_aa_spread": (1.0 - ratio) >= 3.0 * abs(1.0 - aa)},
        "bench": {"command": "python bench.py --gpus 1 --steps 20 --warmup 3 (fresh processes, parent and branch alternated)",
                  "spread": "max / min - 1 over a tree's runs of one session", "sessions": sessions},
        "profiled": {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 3 --serial "
                                "(one run per tree, no counters; profiled figures are compared with each other only)",
                     "parent": pk, "branch": bk, "ratio_branch_over_parent_average": bk["average_ns"] / pk["average_ns"]},
    }
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

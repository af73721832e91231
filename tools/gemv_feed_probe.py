"""profiles/gemv_feed_probe.json from the measurements of the lean kernel's factor feed (two row pairs in flight, MCP_EXP_GEMV2;
the lab arms that were tried beside it) against the parent tree, by the protocol of tools/lean_probe.py:

  lab      python tools/kernel_lab.py run feed_base ARM ... feed_base2 --rounds 8 > lab.txt      one process, interleaved rounds at
           the bench shape; `feed_base` and `feed_base2` are two loads of the parent's step loop, the A/A repeat
  bench    python bench.py --gpus 1 --steps 20 --warmup 3, fresh processes of the parent tree and of this tree, alternated, at least
           4 + 4; one file of JSON result lines per tree, in run order
  outputs  python bench.py ... --dump-outputs DIR of each tree; `cmp` of every file, its verdict passed as --outputs-equal yes|no
  profiled rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 3 --serial, one run
           per tree, no counters; the *_kernel_stats.csv of each (compared with each other only)
  counters rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_BUSY_CYCLES --output-format csv -- python
           tools/profile_paths.py, one run per tree, nothing traced; the *_counter_collection.csv of each

  python tools/gemv_feed_probe.py --lab lab.txt [--lab lab2.txt ...] parent.jsonl branch.jsonl parent_kernel_stats.csv
         branch_kernel_stats.csv parent_counter_collection.csv branch_counter_collection.csv --outputs-equal yes
         -o profiles/gemv_feed_probe.json                 (one --lab per visit to a GPU: boxes differ by a few percent, sessions are not pooled)

The bars: an arm's lab gain over feed_base at least three times the A/A spread, and more than that spread above the arm below it;
every bench run of this tree above every run of the parent's."""
import argparse, collections, csv, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icdf_centred_probe import lean_row
from lean_probe import bench_lines, lab_rounds

COUNTERS = ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_WAVE_CYCLES", "SQ_INSTS_VALU", "SQ_BUSY_CYCLES")


def counters(path):
    """Mean over the lean kernel's dispatches of every counter of one counter-only run, and the two wait shares."""
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        if "mc_paths_lean_kernel" in r["Kernel_Name"]:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
    out = {k: sum(v) / len(v) for k, v in agg.items()}
    out["dispatches"] = max((len(v) for v in agg.values()), default=0)
    if out.get("SQ_WAVE_CYCLES"):
        out["wait_any_share"] = out.get("SQ_WAIT_ANY", 0.0) / out["SQ_WAVE_CYCLES"]
        out["wait_inst_any_share"] = out.get("SQ_WAIT_INST_ANY", 0.0) / out["SQ_WAVE_CYCLES"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lab", action="append", required=True); ap.add_argument("parent_bench"); ap.add_argument("branch_bench")
    ap.add_argument("parent_stats"); ap.add_argument("branch_stats"); ap.add_argument("parent_pmc"); ap.add_argument("branch_pmc")
    ap.add_argument("--outputs-equal", choices=["yes", "no"], required=True)
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    labs = []
    for path in a.lab:
        rounds = lab_rounds(path)
        med = {n: statistics.median(t) for n, t in rounds.items()}
        spread = abs(1.0 - med["feed_base2"] / med["feed_base"])
        arms = {n: {"gain_over_feed_base": 1.0 - med[n] / med["feed_base"],
                    "clears_three_times_the_aa_spread": 1.0 - med[n] / med["feed_base"] >= 3.0 * spread}
                for n in rounds if n not in ("feed_base", "feed_base2")}
        labs.append({"command": "python tools/kernel_lab.py run " + " ".join(rounds) + f" --rounds {len(rounds['feed_base'])}",
                     "rounds_ms": rounds, "median_ms": med, "min_ms": {n: min(t) for n, t in rounds.items()}, "aa_spread": spread, "arms": arms})
    pv, bv = [x["value"] for x in bench_lines(a.parent_bench)], [x["value"] for x in bench_lines(a.branch_bench)]
    pk, bk = lean_row(a.parent_stats), lean_row(a.branch_stats)
    out = {
        "what": "mc_paths_lean_kernel<4, false> at the bench shape (10^6 paths x 16 assets x 252 steps, one portfolio, fused statistics "
                "epilogue), MI355X: the step loop's factor feed against the parent tree's",
        "lab": {"note": "one process per session, interleaved rounds, ms per launch (two launches per timed pair); the arms differ in the lean step "
                        "loop alone; feed_base is the parent's step loop instruction for instruction.  gemv2: two row pairs in flight "
                        "(MCP_EXP_GEMV2); prio_gemv: gemv2 and the priority raised over the factor (MCP_EXP_PRIO), the product build; prio_only: "
                        "the priority without gemv2.  Tried and taken out of the source again: gemv2_lpre / prio_gemv_lpre (the first row-pair "
                        "group's factor entries, the weights and its drift loaded ahead of the step's last Philox block) and prio_philox "
                        "(the priority raised over Philox and the normals instead)",
                "sessions": labs},
        "bench": {"command": "python bench.py --gpus 1 --steps 20 --warmup 3 (fresh processes, parent and branch alternated)",
                  "parent_paths_per_s": pv, "branch_paths_per_s": bv, "parent_spread": max(pv) / min(pv) - 1.0,
                  "branch_spread": max(bv) / min(bv) - 1.0, "gain_of_means": statistics.mean(bv) / statistics.mean(pv) - 1.0,
                  "every_branch_run_above_every_parent_run": min(bv) > max(pv)},
        "outputs": {"command": "python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR per tree, cmp of every file",
                    "byte_equal": a.outputs_equal == "yes"},
        "profiled": {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 3 --serial "
                                "(one run per tree, no counters; profiled figures are compared with each other only)",
                     "parent": pk, "branch": bk, "ratio_branch_over_parent_average": bk["average_ns"] / pk["average_ns"]},
        "counters": {"command": "rocprofv3 --pmc " + " ".join(COUNTERS) + " --output-format csv -- python tools/profile_paths.py "
                                "(one run per tree, nothing traced)",
                     "parent": counters(a.parent_pmc), "branch": counters(a.branch_pmc)},
    }
    text = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

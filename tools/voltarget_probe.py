"""profiles/voltarget_probe.json: one mcp_simulate_vol_target call at N = 16, T = 252, 10^6 paths, K = 1 on GARCH draws beside the
parent commit's mcp_simulate_garch call of the same shape and draws, whole-call wall clock, fresh processes alternated.
   python tools/voltarget_probe.py --parent DIR [--rounds 4] [--out profiles/voltarget_probe.json]
DIR is a checkout of the parent commit with its library built.  Every process warms up (3 calls) and reports the median of 7 timed
calls; the driver starts parent and branch processes in turn, `rounds` of each, and writes both medians of the process medians and
the parent's run-to-run range.
   python tools/voltarget_probe.py --one garch|vol_target      one process: prints its median in ms (the package of the current directory)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

N, T, PATHS, GARCH = 16, 252, 1_000_000, (0.1, 0.85, 1.0)


def one(which):
    sys.path.insert(0, os.getcwd())
    import numpy as np
    from monte_carlo_portfolio_amd import simulate_paths, synthetic
    mu, cov = synthetic.synthetic_market(N)
    w = np.full(N, 1.0 / N)
    kw = dict(n_steps=T, n_paths=PATHS, seed=12345, garch=GARCH)
    if which == "vol_target":
        kw["vol_target"] = (float(np.sqrt(w @ cov @ w)), 0.94, 1.5, 0.0001, 0.00005)
    ms = []
    for i in range(10):
        t0 = time.perf_counter()
        simulate_paths(mu, cov, w, **kw)
        if i >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"which": which, "median_ms": statistics.median(ms), "all_ms": ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="profiles/voltarget_probe.json")
    a = ap.parse_args()
    if a.one:
        return one(a.one)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {"parent_garch": [], "vol_target": [], "branch_garch": []}
    for _ in range(a.rounds):
        for name, cwd, which in (("parent_garch", a.parent, "garch"), ("vol_target", here, "vol_target"), ("branch_garch", here, "garch")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", which], cwd=cwd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"{name} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["median_ms"])
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {"what": f"whole-call wall clock of simulate_paths at N = {N}, T = {T}, {PATHS} paths, K = 1, garch = {GARCH}: the parent commit's "
                   "mcp_simulate_garch call, this tree's mcp_simulate_vol_target call on the same draws (target: the portfolio's step volatility, "
                   "decay 0.94, cap 1.5) and this tree's mcp_simulate_garch call; fresh processes alternated, each the median of 7 calls after 3 "
                   "warm-up calls; the medians of the process medians and the parent's run-to-run range",
           "generated_by": "tools/voltarget_probe.py", "rounds": a.rounds,
           "parent_garch_median_ms": med["parent_garch"], "parent_garch_range_ms": [min(runs["parent_garch"]), max(runs["parent_garch"])],
           "vol_target_median_ms": med["vol_target"], "vol_target_range_ms": [min(runs["vol_target"]), max(runs["vol_target"])],
           "branch_garch_median_ms": med["branch_garch"], "branch_garch_range_ms": [min(runs["branch_garch"]), max(runs["branch_garch"])],
           "vol_target_over_parent_garch": med["vol_target"] / med["parent_garch"], "process_medians_ms": runs}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "what"}))


if __name__ == "__main__":
    main()

"""profiles/underwater_probe.json: one mcp_simulate_underwater call at N = 16, T = 252, 10^6 paths, K = 1 on Gaussian draws beside the
parent commit's mcp_simulate_drawdown call of the same shape, whole-call wall clock, fresh processes alternated.
   python tools/underwater_probe.py --parent DIR [--rounds 4] [--out profiles/underwater_probe.json]
DIR is a checkout of the parent commit with its library built.  Every process warms up (3 calls) and reports the median of 7 timed
calls; the driver starts parent and branch processes in turn, `rounds` of each, and writes the medians of the process medians and
every run-to-run range.
   python tools/underwater_probe.py --one drawdown|underwater      one process: prints its median in ms (the package of the current directory)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

N, T, PATHS = 16, 252, 1_000_000


def one(which):
    sys.path.insert(0, os.getcwd())
    import numpy as np
    from monte_carlo_portfolio_amd import simulate_paths, synthetic
    mu, cov = synthetic.synthetic_market(N)
    w = np.full(N, 1.0 / N)
    kw = dict(n_steps=T, n_paths=PATHS, seed=12345, drawdown=True)
    if which == "underwater":
        kw["underwater"] = True
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
    ap.add_argument("--out", default="profiles/underwater_probe.json")
    a = ap.parse_args()
    if a.one:
        return one(a.one)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {"parent_drawdown": [], "underwater": [], "branch_drawdown": []}
    for _ in range(a.rounds):
        for name, cwd, which in (("parent_drawdown", a.parent, "drawdown"), ("underwater", here, "underwater"), ("branch_drawdown", here, "drawdown")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", which], cwd=cwd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"{name} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["median_ms"])
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {"what": f"whole-call wall clock of simulate_paths(drawdown=True) at N = {N}, T = {T}, {PATHS} paths, K = 1, Gaussian draws, simple "
                   "compounding: the parent commit's mcp_simulate_drawdown call, this tree's mcp_simulate_underwater call on the same draws "
                   "(underwater=True: two counters per path, two histogram launches, two summaries) and this tree's mcp_simulate_drawdown call; "
                   "fresh processes alternated, each the median of 7 calls after 3 warm-up calls; the medians of the process medians and "
                   "every run-to-run range",
           "generated_by": "tools/underwater_probe.py", "rounds": a.rounds,
           "parent_drawdown_median_ms": med["parent_drawdown"], "parent_drawdown_range_ms": [min(runs["parent_drawdown"]), max(runs["parent_drawdown"])],
           "underwater_median_ms": med["underwater"], "underwater_range_ms": [min(runs["underwater"]), max(runs["underwater"])],
           "branch_drawdown_median_ms": med["branch_drawdown"], "branch_drawdown_range_ms": [min(runs["branch_drawdown"]), max(runs["branch_drawdown"])],
           "underwater_over_parent_drawdown": med["underwater"] / med["parent_drawdown"], "process_medians_ms": runs}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "what"}))


if __name__ == "__main__":
    main()

"""profiles/uncertain_probe.json: one simulate_paths call at N = 16, T = 252, 10^6 paths with drift_uncertainty beside the same call
without it, at K = 1 (where the call without it runs the lean kernel: the difference is the user's real price) and at K = 8,
whole-call wall clock, fresh processes alternated.
   python tools/uncertain_probe.py [--rounds 3] [--out profiles/uncertain_probe.json]
Every process warms up (3 calls) and reports the median of 7 timed calls; the driver starts the four kinds of process in turn,
`rounds` of each, and writes the medians of the process medians and their run-to-run ranges.
   python tools/uncertain_probe.py --one plain|uncertain --k 1|8      one process: prints its median in ms"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

N, T, PATHS, N_OBS = 16, 252, 1_000_000, 84


def one(which, k):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    from monte_carlo_portfolio_amd import simulate_paths, synthetic
    mu, cov = synthetic.synthetic_market(N)
    w = np.full(N, 1.0 / N) if k == 1 else synthetic.dirichlet_weights(N, k)
    kw = dict(n_steps=T, n_paths=PATHS, seed=12345)
    if which == "uncertain":
        kw["drift_uncertainty"] = N_OBS
    ms = []
    for i in range(10):
        t0 = time.perf_counter()
        simulate_paths(mu, cov, w, **kw)
        if i >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"which": which, "k": k, "median_ms": statistics.median(ms), "all_ms": ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/uncertain_probe.json")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.k)
    arms = [(f"{which}_k{k}", which, k) for k in (1, 8) for which in ("plain", "uncertain")]
    runs = {name: [] for name, _, _ in arms}
    for _ in range(a.rounds):
        for name, which, k in arms:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", which, "--k", str(k)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"{name} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["median_ms"])
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {"what": f"whole-call wall clock of simulate_paths at N = {N}, T = {T}, {PATHS} paths, K = 1 and K = 8: the call without the keyword "
                   f"(K = 1: the lean kernel) and the call with drift_uncertainty = {N_OBS}; fresh processes alternated, each the median of 7 "
                   "calls after 3 warm-up calls; the medians of the process medians and their run-to-run ranges",
           "generated_by": "tools/uncertain_probe.py", "rounds": a.rounds}
    for name in runs:
        out[f"{name}_median_ms"] = med[name]
        out[f"{name}_range_ms"] = [min(runs[name]), max(runs[name])]
    for k in (1, 8):
        out[f"uncertain_over_plain_k{k}"] = med[f"uncertain_k{k}"] / med[f"plain_k{k}"]
    out["process_medians_ms"] = runs
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "what"}))


if __name__ == "__main__":
    main()

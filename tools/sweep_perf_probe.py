"""Timing probe for the sweep's series statistics (mcp_sweep_historical_perf, SPEC.md 5.24) beside mcp_sweep_historical on the same
inputs, both as whole host calls (uploads, kernel, download, finish): rows x assets x portfolios, the median of 25 calls after 3
warm-up calls each, alternating so that both see the same clocks.  One process, one run -> profiles/sweep_perf.json.

    python tools/sweep_perf_probe.py [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from monte_carlo_portfolio_amd import sweep  # noqa: E402

SHAPES = ((13, 3, 2500), (252, 16, 10_000), (4096, 16, 2500))
WARMUP, CALLS = 3, 25


def main(out_path):
    rows = []
    for R, N, P in SHAPES:
        rng = np.random.default_rng(R + N)
        Rc, mean, cov = sweep.sweep_inputs(rng.normal(0.0004, 0.02, (R, N)), 252)
        W = np.random.RandomState(7).dirichlet(np.ones(N), P)
        calls = {"mcp_sweep_historical": lambda: sweep.score_portfolios(Rc, mean, cov, W, 0.03),
                 "mcp_sweep_historical_perf": lambda: sweep.score_performance(Rc, W, 0.03, 252)}
        ts = {k: [] for k in calls}
        for it in range(WARMUP + CALLS):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                if it >= WARMUP:
                    ts[k].append(time.perf_counter() - t0)
        row = {"rows": R, "assets": N, "portfolios": P, "calls": CALLS, "warmup": WARMUP}
        for k, t in ts.items():
            row[k] = {"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}
        row["ratio_of_medians"] = row["mcp_sweep_historical_perf"]["median_ms"] / row["mcp_sweep_historical"]["median_ms"]
        rows.append(row)
        print(f"rows {R:5d} x assets {N:2d} x portfolios {P:6d}: perf {row['mcp_sweep_historical_perf']['median_ms']:8.3f} ms  "
              f"historical {row['mcp_sweep_historical']['median_ms']:8.3f} ms  ratio {row['ratio_of_medians']:.2f}")
    doc = {"what": "whole host calls, wall clock, one process on one MI355X; a single-box number", "shapes": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                             "sweep_perf.json"))

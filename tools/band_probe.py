"""Cost of tolerance-band rebalancing (SPEC.md 4.18 / 5.18) at N = 16, T = 252, 10^6 paths, K = 1, Gaussian draws: mc_paths_band_kernel
against mc_paths_reb_kernel<4, 1, 1, ...> at the same period, in the same process.  The rebalancing kernel is the parent commit's by
code digest (profiles/band_isa.txt), so its call is the parent's.  Per period (e = 21 and e = 1) three legs: every tolerance 0 (every
lane trades at every review), nothing watched (no lane trades: every review takes the wave-level skip) and one band for all assets
that trades in about half of the reviews (found by bisection on 20 000 paths before anything is timed).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/band_probe.py --rounds 5 -o run.json
                                                            (kernel times in DIR; the run's own call times and the bands found in run.json)
  python tools/band_probe.py --summarize DIR --rounds 5 --run-json run.json -o profiles/band_probe.json

After the bisection (CAL calls per period, each one path-kernel dispatch) every configuration is warmed up with --warm calls; then
--rounds rounds each run every configuration once, so the legs alternate through the whole timed window; *_again repeats the
rebalancing call (an A/A pair: the noise of a ratio).  Calls are synchronous and each has exactly one path-kernel dispatch, so the
kernel trace is cut at the path kernels.  Medians over the rounds; ratios of the medians."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monte_carlo_portfolio_amd import simulate_paths, synthetic  # noqa: E402

N, T, P = 16, 252, 1_000_000
COST = 1e-3
PERIODS = (21, 1)
CAL, CAL_PATHS = 12, 20_000
LEGS = ("reb", "band_all", "band_none", "band_half", "reb_again")


def _call(mu, cov, w, e, n, tol=None):
    kw = {} if tol is None else {"tolerance": tol}
    return simulate_paths(mu, cov, w, n_steps=T, n_paths=n, seed=synthetic.BENCH_SEED, rebalance=e, rebalance_cost=COST, **kw)


def half_band(mu, cov, w, e):
    """The tolerance (one number for every asset) at which about half of the reviews trade: CAL bisection steps on CAL_PATHS paths."""
    lo, hi = 0.0, 0.5
    share = None
    for _ in range(CAL):
        mid = 0.5 * (lo + hi)
        tb = _call(mu, cov, w, e, CAL_PATHS, mid)["tolerance"]
        share = tb["trades"]["mean"] / tb["n_reviews"]
        lo, hi = (mid, hi) if share > 0.5 else (lo, mid)
    return 0.5 * (lo + hi), share


def configs():
    """[(name, kernel-name substring, call)] in the order the probe runs them; the bisections run here"""
    mu, cov = synthetic.synthetic_market(N)
    w = synthetic.equal_weights(N)
    out, found = [], {}
    for e in PERIODS:
        tol, share = half_band(mu, cov, w, e)
        found[f"e{e}"] = {"tolerance": tol, "share_of_reviews_trading": share}
        legs = {"reb": None, "reb_again": None, "band_all": 0.0, "band_none": np.inf, "band_half": tol}
        for name in LEGS:
            pat = "mc_paths_band_kernel<" if name.startswith("band") else "mc_paths_reb_kernel<"
            out.append((f"e{e}_{name}", pat, lambda e=e, t=legs[name]: _call(mu, cov, w, e, P, t)))
    return out, found


def run(rounds, warm):
    cfg, found = configs()
    for _ in range(warm):
        for _, _, f in cfg:
            f()
    ts = {name: [] for name, _, _ in cfg}
    for _ in range(rounds):
        for name, _, f in cfg:
            t0 = time.perf_counter()
            f()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    res = {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v} for name, v in ts.items()}
    for name, v in res.items():
        print(f"call {name:16s} {v['median_ms']:9.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})")
    print("half bands:", json.dumps(found))
    return {"calls": res, "half_bands": found}


def summarize(d, rounds, warm, run_json):
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    rows = sorted(csv.DictReader(open(paths[0])), key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6   # noqa: E731
    calls = []                                                                  # [[path-kernel row, the rows up to the next one]]
    for r in rows:
        if "mc_paths_" in r["Kernel_Name"]:
            calls.append([r])
        elif calls:
            calls[-1].append(r)
    names = [(f"e{e}_{leg}", "mc_paths_band_kernel<" if leg.startswith("band") else "mc_paths_reb_kernel<") for e in PERIODS for leg in LEGS]
    C, skip = len(names), CAL * len(PERIODS)
    if len(calls) != skip + C * (warm + rounds):
        raise SystemExit(f"{len(calls)} path-kernel dispatches, expected {skip + C * (warm + rounds)}")
    calls = calls[skip:]
    k = {}
    med = statistics.median
    for i, (name, pat) in enumerate(names):
        mine = [calls[C * (warm + r) + i] for r in range(rounds)]
        assert all(pat in c[0]["Kernel_Name"] for c in mine), (name, mine[0][0]["Kernel_Name"])
        t = [ms(c[0]) for c in mine]
        k[name] = {"kernel": mine[0][0]["Kernel_Name"].split("(")[0], "median_ms": med(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t,
                   "all_dispatches_ms": med([sum(ms(r) for r in c) for c in mine])}
    res = {
        "what": f"Tolerance bands (SPEC.md 4.18 / 5.18) at N = {N}, T = {T}, {P} paths, K = 1, Gaussian draws, cost {COST}: kernel times of "
                "mc_paths_band_kernel against mc_paths_reb_kernel at the same period -- the parent commit's kernel by code digest -- from one "
                f"rocprofv3 --kernel-trace --stats process; every configuration warmed up ({warm} calls), then {rounds} rounds that each run "
                "every configuration once; medians over the rounds and ratios of the medians; *_again is the A/A pair.  band_all: every "
                "tolerance 0; band_none: nothing watched; band_half: one band that trades in about half of the reviews.  all_dispatches_ms "
                "adds the statistics kernels of the call (the banded call also reduces the trade counts and the turnover)",
        "generated_by": "tools/band_probe.py",
        "kernels": k,
        "ratios_vs_rebalancing_kernel": {name: v["median_ms"] / k[name.split("_")[0] + "_reb"]["median_ms"] for name, v in k.items()
                                         if not name.endswith("_reb")},
    }
    if run_json:
        res.update(json.load(open(run_json)))
    for name, v in k.items():
        r = res["ratios_vs_rebalancing_kernel"].get(name)
        print(f"kernel {name:16s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]  all dispatches {v['all_dispatches_ms']:.4f} ms"
              + (f"  x{r:.4f}" if r else ""))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds; each runs every configuration once")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls of every configuration before the rounds")
    ap.add_argument("--summarize", default=None, help="rocprofv3 output directory of a run with the same --rounds / --warm")
    ap.add_argument("--run-json", default=None, help="the -o file of the profiled run: its call times and half bands go into the summary")
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    res = summarize(a.summarize, a.rounds, a.warm, a.run_json) if a.summarize else run(a.rounds, a.warm)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Cost of buy-and-hold and periodic rebalancing (SPEC.md 4.5) at BASELINE configs[1]'s shape (16 assets, 10^6 paths, 252 steps),
K = 1 and K = 8: the rebalancing kernel for periods 1, 21 and never (buy-and-hold) without and with a cost of 10 bp, against the
constant-weight kernel of the same draws -- Gaussian (mc_paths_kernel) and bootstrap with R = 252 rows in LDS
(mc_paths_boot_kernel) -- in the same process, and the whole calls.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rebalance_probe.py --rounds 9    (kernel times)
  python tools/rebalance_probe.py --rounds 9 --time -o calls_a.json                                           (call times)
  python tools/rebalance_probe.py --rounds 9 --time -o calls_b.json                      (the same command again: the spread)
  python tools/rebalance_probe.py --summarize DIR --rounds 9 --calls-json calls_a.json calls_b.json -o profiles/rebalance_probe.json

Every configuration is first warmed up with --warm calls; then --rounds rounds each run every configuration once, so the
constant-weight baselines and the variants alternate through the whole timed window.  Calls are synchronous, so the path-kernel
dispatches of the kernel trace fall to the configurations in that order (one dispatch per call: K = 8 is one pass of the
8-portfolio kernel).  Kernel and call times are medians over the rounds; the ratios are those of the medians."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from monte_carlo_portfolio_amd import simulate_bootstrap, simulate_paths, synthetic  # noqa: E402

N, T, P = 16, 252, 1_000_000
REB = [(1, 0.0), (1, 1e-3), (21, 0.0), (21, 1e-3), ("never", 0.0), ("never", 1e-3)]


def configs():
    """[(name, kernel-name substring, call)] in the order the probe runs them; *_again repeats the constant-weight baseline
    after the variants of its group (an A/A pair: the noise of a ratio)"""
    mu, cov = synthetic.synthetic_market(N)
    rng = np.random.default_rng(20240601)
    rows = mu + rng.standard_normal((252, N)) @ np.linalg.cholesky(cov).T
    out = []
    for K in (1, 8):
        w = synthetic.dirichlet_weights(N, K) if K > 1 else synthetic.equal_weights(N)
        kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED)
        out.append((f"K{K}_gauss_constant", "mc_paths_kernel<", lambda w=w, kw=kw: simulate_paths(mu, cov, w, **kw)))
        for m, c in REB:
            out.append((f"K{K}_gauss_m{m}_cost{c:g}", "mc_paths_reb_kernel<",
                        lambda w=w, kw=kw, m=m, c=c: simulate_paths(mu, cov, w, rebalance=m, rebalance_cost=c, **kw)))
        out.append((f"K{K}_gauss_again", "mc_paths_kernel<", lambda w=w, kw=kw: simulate_paths(mu, cov, w, **kw)))   # A/A
        out.append((f"K{K}_boot_constant", "mc_paths_boot_kernel<",
                    lambda w=w, kw=kw: simulate_bootstrap(rows, w, block=3.0, **kw)))
        for m, c in REB:
            out.append((f"K{K}_boot_m{m}_cost{c:g}", "mc_paths_reb_kernel<",
                        lambda w=w, kw=kw, m=m, c=c: simulate_bootstrap(rows, w, block=3.0, rebalance=m, rebalance_cost=c, **kw)))
        out.append((f"K{K}_boot_again", "mc_paths_boot_kernel<", lambda w=w, kw=kw: simulate_bootstrap(rows, w, block=3.0, **kw)))
    return out


def run(rounds, warm, timed):
    cfg = configs()
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
    if timed:
        for name, v in res.items():
            print(f"call {name:28s} {v['median_ms']:9.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})")
    return res


def base(name):
    """the constant-weight configuration of the same K and draws: K8_boot_m21_cost0 -> K8_boot_constant"""
    return "_".join(name.split("_")[:2]) + "_constant"


def summarize(d, rounds, warm, calls_json):
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    rows = [r for r in csv.DictReader(open(paths[0])) if "mc_paths_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cfg = configs()
    C = len(cfg)
    if len(rows) != C * (warm + rounds):
        raise SystemExit(f"{len(rows)} path-kernel dispatches, expected {C * (warm + rounds)}")
    k = {}
    for i, (name, pat, _) in enumerate(cfg):
        mine = [rows[C * (warm + r) + i] for r in range(rounds)]
        assert all(pat in r["Kernel_Name"] for r in mine), (name, mine[0]["Kernel_Name"])
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in mine]
        k[name] = {"kernel": mine[0]["Kernel_Name"].split("(")[0], "median_ms": statistics.median(ms), "min_ms": min(ms),
                   "max_ms": max(ms)}
    res = {
        "what": "buy-and-hold / periodic rebalancing (SPEC.md 4.5) at configs[1]'s shape (N = 16, T = 252, 10^6 paths), K = 1 and 8: "
                "kernel times of mc_paths_reb_kernel per period m and cost, and of the constant-weight kernel of the same draws "
                "(mc_paths_kernel, mc_paths_boot_kernel with R = 252 rows in LDS), from one rocprofv3 --kernel-trace --stats process; "
                f"every configuration warmed up ({warm} calls), then {rounds} rounds that each run every configuration once "
                "(baselines and variants alternate); medians over the rounds and ratios of the medians.  Whole-call wall-clock "
                "medians from two more processes without the profiler (the same command twice: the spread between processes)",
        "generated_by": "tools/rebalance_probe.py",
        "kernels": k,
        "ratios_vs_constant": {name: v["median_ms"] / k[base(name)]["median_ms"] for name, v in k.items() if "_constant" not in name},
    }
    for j, cj in enumerate(calls_json or []):
        c = json.load(open(cj))
        res[f"calls_{j}"] = c
        res[f"call_ratios_vs_constant_{j}"] = {name: v["median_ms"] / c[base(name)]["median_ms"] for name, v in c.items()
                                               if "_constant" not in name}
    for name, v in k.items():
        r = res["ratios_vs_constant"].get(name)
        calls = "  ".join(f"call x{res[f'call_ratios_vs_constant_{j}'][name]:.3f}" for j in range(len(calls_json or []))
                          if name in res[f"call_ratios_vs_constant_{j}"])
        print(f"kernel {name:28s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]" + (f"  x{r:.3f}  {calls}" if r else ""))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9, help="timed rounds; each runs every configuration once")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls of every configuration before the rounds")
    ap.add_argument("--time", action="store_true", help="print and save the call times")
    ap.add_argument("--summarize", default=None, help="rocprofv3 output directory of a run with the same --rounds / --warm")
    ap.add_argument("--calls-json", nargs="*", default=None)
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    res = summarize(a.summarize, a.rounds, a.warm, a.calls_json) if a.summarize else run(a.rounds, a.warm, a.time)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

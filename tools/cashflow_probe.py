"""Cost of cash flows and ruin (SPEC.md 4.7 / 5.6) at BASELINE configs[1]'s shape (16 assets, 10^6 paths, 252 steps, four horizons),
K = 1 and K = 8: mc_paths_cf_kernel on Gaussian, bootstrap (row table in LDS and in global memory) and Student-t (nu = 5) draws,
each against its twin without cash flows (mc_paths_hz_kernel, mc_paths_boot_hz_kernel, mc_paths_t_hz_kernel) in the same process,
the counting kernel, and the whole calls.  Two more configurations time what a mass of ruined paths costs the streaming select:
synthetic_market(3), equal weights, T = 60, five horizons, 10^6 paths with 0.0165 taken out per step (close to half of the paths
end at exactly +0) against an all-zero schedule of the same shape, with the hist_kernel dispatches of each call summed.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cashflow_probe.py --rounds 5     (kernel times)
  python tools/cashflow_probe.py --rounds 5 --time -o calls_a.json                                            (call times)
  python tools/cashflow_probe.py --rounds 5 --time -o calls_b.json                       (the same command again: the spread)
  python tools/cashflow_probe.py --summarize DIR --rounds 5 --calls-json calls_a.json calls_b.json -o profiles/cashflow_probe.json

Every configuration is first warmed up with --warm calls; then --rounds rounds each run every configuration once, so the twins
and the cash-flow kernels alternate through the whole timed window.  Calls are synchronous and each has exactly one path-kernel
dispatch (K = 8 is one pass of the 8-portfolio kernel), so the kernel trace is cut at the path kernels: a call's dispatches are
its path kernel and everything up to the next one.  Kernel and call times are medians over the rounds; ratios of the medians."""
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

COUNT_ROWS = "count_kernel<mcp::RuinedShort>"      # launch_count_rows' kernel as the trace names it

N, T, P = 16, 252, 1_000_000
HZ = dict(horizons=[21, 63, 126, 252], bands=(5.0, 50.0, 95.0))
FLOW = 0.001                       # a contribution: no path is ruined, the statistics passes see what the twin's see
TIES = dict(n_steps=60, n_paths=P, horizons=[12, 24, 36, 48, 60], bands=(5.0, 50.0, 95.0))


def configs():
    """[(name, kernel-name substring, call)] in the order the probe runs them; hz_gauss_again repeats the first twin after the
    variants of its group (an A/A pair: the noise of a ratio)"""
    mu, cov = synthetic.synthetic_market(N)
    rng = np.random.default_rng(7)
    L = np.linalg.cholesky(cov)
    rows = {"boot": mu + rng.standard_normal((250, N)) @ L.T, "bootg": mu + rng.standard_normal((400, N)) @ L.T}   # 250 rows fit LDS
    out = []
    for K in (1, 8):
        w = synthetic.dirichlet_weights(N, K) if K > 1 else synthetic.equal_weights(N)
        kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED, **HZ)
        draws = [("gauss", "mc_paths_hz_kernel<", lambda c, w=w, kw=kw: simulate_paths(mu, cov, w, cashflow=c, **kw))]
        for b in ("boot", "bootg"):
            draws.append((b, "mc_paths_boot_hz_kernel<", lambda c, w=w, kw=kw, b=b: simulate_bootstrap(rows[b], w, block=5.0, cashflow=c, **kw)))
        draws.append(("t5", "mc_paths_t_hz_kernel<", lambda c, w=w, kw=kw: simulate_paths(mu, cov, w, dof=5, cashflow=c, **kw)))
        for name, twin, f in draws:
            out.append((f"K{K}_hz_{name}", twin, lambda f=f: f(None)))
            out.append((f"K{K}_cf_{name}", "mc_paths_cf_kernel<", lambda f=f: f(FLOW)))
        out.append((f"K{K}_hz_gauss_again", "mc_paths_hz_kernel<", lambda f=draws[0][2]: f(None)))
    mu3, cov3 = synthetic.synthetic_market(3)
    for name, c in (("ties_zero", 0.0), ("ties_ruin", -0.0165)):
        out.append((f"K1_cf_{name}", "mc_paths_cf_kernel<",
                    lambda c=c: simulate_paths(mu3, cov3, np.ones(3) / 3, seed=synthetic.BENCH_SEED, cashflow=c, **TIES)))
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
    """the configuration a ratio is taken against: K8_cf_t5 -> K8_hz_t5, K1_hz_gauss_again -> K1_hz_gauss, ties_ruin -> ties_zero"""
    if name.endswith("ties_ruin"):
        return name.replace("ties_ruin", "ties_zero")
    return name.replace("_again", "").replace("_cf_", "_hz_")


def has_ratio(name):
    return "_cf_" in name and not name.endswith("ties_zero") or name.endswith("_again")


def summarize(d, rounds, warm, calls_json):
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
    cfg = configs()
    C = len(cfg)
    if len(calls) != C * (warm + rounds):
        raise SystemExit(f"{len(calls)} path-kernel dispatches, expected {C * (warm + rounds)}")
    k = {}
    med = statistics.median
    for i, (name, pat, _) in enumerate(cfg):
        mine = [calls[C * (warm + r) + i] for r in range(rounds)]
        assert all(pat in c[0]["Kernel_Name"] for c in mine), (name, mine[0][0]["Kernel_Name"])
        t = [ms(c[0]) for c in mine]
        part = lambda sub: [sum(ms(r) for r in c[1:] if sub in r["Kernel_Name"]) for c in mine]   # noqa: E731
        k[name] = {"kernel": mine[0][0]["Kernel_Name"].split("(")[0], "median_ms": med(t), "min_ms": min(t), "max_ms": max(t),
                   "hist_kernel_ms": med(part("hist_kernel")), "hist_kernel_dispatches": sum("hist_kernel" in r["Kernel_Name"] for r in mine[0]),
                   "count_rows_kernel_ms": med(part(COUNT_ROWS)),
                   "count_rows_kernel_dispatches": sum(COUNT_ROWS in r["Kernel_Name"] for r in mine[0]),
                   "all_dispatches_ms": med([sum(ms(r) for r in c) for c in mine])}
    res = {
        "what": "Cash flows and ruin (SPEC.md 4.7 / 5.6) at configs[1]'s shape (N = 16, T = 252, 10^6 paths, horizons 21 / 63 / 126 / 252), "
                "K = 1 and 8: kernel times of mc_paths_cf_kernel on Gaussian, bootstrap (LDS: 250 rows; global: 400 rows) and Student-t "
                "(nu = 5) draws with 0.001 paid in per step (no ruin) against the twin without cash flows (mc_paths_hz_kernel, "
                "mc_paths_boot_hz_kernel, mc_paths_t_hz_kernel), from one rocprofv3 --kernel-trace --stats process; every configuration "
                f"warmed up ({warm} calls), then {rounds} rounds that each run every configuration once (twins and variants alternate); "
                "medians over the rounds and ratios of the medians; *_again is the A/A pair.  hist_kernel_ms / count_rows_kernel_ms (count_kernel<RuinedShort>, the kernel behind launch_count_rows): the "
                "dispatches of those kernels summed per call.  ties_ruin / ties_zero: synthetic_market(3), equal weights, T = 60, "
                "horizons 12 .. 60, 10^6 paths, 0.0165 taken out per step (about 45 % of the paths end at +0) against an all-zero "
                "schedule.  Whole-call wall-clock medians from two more processes without the profiler (the same command twice: the "
                "spread between processes)",
        "generated_by": "tools/cashflow_probe.py",
        "kernels": k,
        "ratios_vs_twin": {name: v["median_ms"] / k[base(name)]["median_ms"] for name, v in k.items() if has_ratio(name)},
        "hist_kernel_ratio_ties": k["K1_cf_ties_ruin"]["hist_kernel_ms"] / k["K1_cf_ties_zero"]["hist_kernel_ms"],
    }
    for j, cj in enumerate(calls_json or []):
        c = json.load(open(cj))
        res[f"calls_{j}"] = c
        res[f"call_ratios_vs_twin_{j}"] = {name: v["median_ms"] / c[base(name)]["median_ms"] for name, v in c.items() if has_ratio(name)}
    for name, v in k.items():
        r = res["ratios_vs_twin"].get(name)
        cr = "  ".join(f"call x{res[f'call_ratios_vs_twin_{j}'][name]:.3f}" for j in range(len(calls_json or []))
                       if name in res[f"call_ratios_vs_twin_{j}"])
        print(f"kernel {name:22s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]  hist {v['hist_kernel_ms']:.4f}  "
              f"count {v['count_rows_kernel_ms']:.4f}" + (f"  x{r:.3f}  {cr}" if r else ""))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds; each runs every configuration once")
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

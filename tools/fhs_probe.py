"""Cost of filtered historical simulation (SPEC.md 2.4 / 4.11) at BASELINE configs[1]'s shape (16 assets, 10^6 paths, 252 steps, one
portfolio, R = 252 rows in LDS, mean block 1): mc_paths_fhs_kernel against mc_paths_boot_kernel on the same rows and against
mc_paths_g_kernel on the rows' mean and covariance, in the same process, and the whole calls.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fhs_probe.py --rounds 7        (kernel times)
  python tools/fhs_probe.py --rounds 7 --time -o calls.json                                                 (call times)
  python tools/fhs_probe.py --summarize DIR --rounds 7 --calls-json calls.json -o profiles/fhs_probe.json

Every configuration is first warmed up with --warm calls; then --rounds rounds each run every configuration once, in the order
FHS, bootstrap, GARCH, FHS again, so the kernels alternate through the whole timed window and FHS has an A/A repeat (the noise a
ratio is read against).  Calls are synchronous, so the path-kernel dispatches of the kernel trace fall to the configurations in that
order (one dispatch per call).  Kernel and call times are medians over the rounds; the ratios are those of the medians."""
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

from monte_carlo_portfolio_amd import filter_rows, simulate_bootstrap, simulate_filtered, simulate_paths, synthetic  # noqa: E402

N, T, P, R = 16, 252, 1_000_000, 252
AB = (0.10, 0.85)


def configs():
    """[(name, kernel-name substring, call)] in the order the probe runs them"""
    rng = np.random.default_rng(20240601)
    mu, cov = synthetic.synthetic_market(N)
    rows = mu + rng.standard_normal((R, N)) @ np.linalg.cholesky(cov).T
    f = filter_rows(rows, AB)
    g = (f.alpha, f.beta, f.h0)
    w = synthetic.equal_weights(N)
    kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED)
    fhs = lambda: simulate_filtered(f, w, block=1.0, **kw)                                           # noqa: E731
    boot = lambda: simulate_bootstrap(rows, w, block=1.0, **kw)                                      # noqa: E731
    garch = lambda: simulate_paths(rows.mean(axis=0), np.cov(rows.T), w, garch=g, **kw)              # noqa: E731
    return [("fhs", "mc_paths_fhs_kernel<4, 1, 1, true>", fhs), ("boot", "mc_paths_boot_kernel<4, 1, 1, false, true>", boot),
            ("garch", "mc_paths_g_kernel<4, 1, 1>", garch), ("fhs_again", "mc_paths_fhs_kernel<4, 1, 1, true>", fhs)]


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
            print(f"call {name:12s} {v['median_ms']:9.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})")
    return res


def ratios(k):
    return {"fhs_vs_boot": k["fhs"]["median_ms"] / k["boot"]["median_ms"], "fhs_vs_garch": k["fhs"]["median_ms"] / k["garch"]["median_ms"],
            "fhs_again_vs_fhs": k["fhs_again"]["median_ms"] / k["fhs"]["median_ms"]}


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
        k[name] = {"kernel": mine[0]["Kernel_Name"].split("(")[0], "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
    res = {
        "what": "filtered historical simulation (SPEC.md 2.4 / 4.11) at configs[1]'s shape (N = 16, T = 252, 10^6 paths, K = 1, R = 252 "
                "rows in LDS, mean block 1): kernel times of mc_paths_fhs_kernel, of mc_paths_boot_kernel on the same rows and of "
                "mc_paths_g_kernel on their mean and covariance, and of the FHS kernel's A/A repeat, from one rocprofv3 --kernel-trace "
                f"--stats process; every configuration warmed up ({warm} calls), then {rounds} rounds that each run every configuration "
                "once (the kernels alternate); medians over the rounds and ratios of the medians.  Whole-call wall-clock medians from "
                "one more process without the profiler",
        "generated_by": "tools/fhs_probe.py",
        "kernels": k,
        "kernel_ratios": ratios(k),
    }
    res["fixed_bar_faster_than_garch"] = res["kernel_ratios"]["fhs_vs_garch"] < 1.0
    if calls_json:
        c = json.load(open(calls_json))
        res["calls"] = c
        res["call_ratios"] = ratios(c)
    for name, v in k.items():
        print(f"kernel {name:12s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]")
    for name, v in res["kernel_ratios"].items():
        print(f"kernel ratio {name:18s} {v:.4f}" + (f"   call ratio {res['call_ratios'][name]:.4f}" if calls_json else ""))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="timed rounds; each runs every configuration once")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls of every configuration before the rounds")
    ap.add_argument("--time", action="store_true", help="print and save the call times")
    ap.add_argument("--summarize", default=None, help="rocprofv3 output directory of a run with the same --rounds / --warm")
    ap.add_argument("--calls-json", default=None)
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    res = summarize(a.summarize, a.rounds, a.warm, a.calls_json) if a.summarize else run(a.rounds, a.warm, a.time)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

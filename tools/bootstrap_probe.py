"""Cost of the stationary block bootstrap (SPEC.md 2.1 / 4.4) at BASELINE configs[1]'s shape (16 assets, 10^6 paths, 252 steps,
one portfolio): the bootstrap kernel against the plain Gaussian kernel in the same process, with the row table in LDS (R = 252)
and in global memory (R = 100,000), the horizons variant (12 monthly horizons, 3 levels), and the whole calls.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bootstrap_probe.py --calls 5    (kernel times)
  python tools/bootstrap_probe.py --calls 7 --time -o calls.json                                             (call times)
  rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU SQ_INSTS_LDS --output-format csv -d PMC -- \
      python tools/bootstrap_probe.py --calls 1               (counters only; again with MCP_LIB_PATH = an unswizzled lab build)
  python tools/bootstrap_probe.py --summarize DIR --calls-json calls.json --pmc PMC PMC_NOSWZ -o profiles/bootstrap_probe.json

The kernel times are the kernel trace's per-kernel averages over the calls of one process (the mangled names tell the plain,
LDS-table, global-table and horizon kernels apart).  Call times are wall-clock medians of synchronous calls, A / B interleaved,
in a process without the profiler."""
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
HORIZONS = list(range(21, 253, 21))
LEVELS = (2.5, 50.0, 97.5)


def tables():
    rng = np.random.default_rng(20240601)
    mu, cov = synthetic.synthetic_market(N)
    L = np.linalg.cholesky(cov)
    return {R: (mu + rng.standard_normal((R, N)) @ L.T) for R in (252, 100_000)}, mu, cov


def calls(n, timed):
    tab, mu, cov = tables()
    w = synthetic.equal_weights(N)
    kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED)
    runs = {
        "gauss": lambda: simulate_paths(mu, cov, w, **kw),
        "boot_lds": lambda: simulate_bootstrap(tab[252], w, block=3.0, **kw),
        "boot_global": lambda: simulate_bootstrap(tab[100_000], w, block=3.0, **kw),
        "boot_lds_hz": lambda: simulate_bootstrap(tab[252], w, block=3.0, horizons=HORIZONS, bands=LEVELS, **kw),
        "gauss_hz": lambda: simulate_paths(mu, cov, w, horizons=HORIZONS, bands=LEVELS, **kw),
    }
    for f in runs.values():
        f()
    out = {k: [] for k in runs}
    for _ in range(n):
        for k, f in runs.items():
            t0 = time.perf_counter()
            f()
            out[k].append((time.perf_counter() - t0) * 1e3)
    res = {k: {"median_ms": statistics.median(v), "all_ms": v} for k, v in out.items()}
    if timed:
        for k, v in res.items():
            print(f"call {k:12s} {v['median_ms']:9.3f} ms")
    return res


KERNELS = {  # key: substring of the demangled kernel name (<NB, KT, PPT, ..., LOGC[, BLDS]>)
    "gauss": "mc_paths_kernel<4, 1, 1, false, false, false>",
    "boot_lds": "mc_paths_boot_kernel<4, 1, 1, false, true>",
    "boot_global": "mc_paths_boot_kernel<4, 1, 1, false, false>",
    "boot_lds_hz": "mc_paths_boot_hz_kernel<4, 1, 1, false, true>",
    "gauss_hz": "mc_paths_hz_kernel<4, 1, 1, false>",
}


def counters(d):
    """per-kernel sums of a counter-only run's counter_collection.csv (every dispatch of the process)"""
    paths = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no counter_collection.csv under {d}")
    out = {}
    for r in csv.DictReader(open(paths[0])):
        for key, pat in KERNELS.items():
            if pat in r["Kernel_Name"]:
                out.setdefault(key, {}).setdefault(r["Counter_Name"], 0.0)
                out[key][r["Counter_Name"]] += float(r["Counter_Value"])
    return out


def summarize(d, calls_json, pmc=None):
    paths = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no kernel_stats.csv under {d}")
    rows = list(csv.DictReader(open(paths[0])))
    k = {}
    for key, pat in KERNELS.items():
        hit = [r for r in rows if pat in r["Name"]]
        if hit:
            k[key] = {"name": hit[0]["Name"], "calls": int(hit[0]["Calls"]), "avg_ms": float(hit[0]["AverageNs"]) / 1e6,
                      "min_ms": float(hit[0]["MinNs"]) / 1e6}
    g = k["gauss"]["avg_ms"]
    res = {
        "what": "stationary block bootstrap (SPEC.md 2.1 / 4.4) cost at configs[1]'s shape (N = 16, T = 252, 10^6 paths, K = 1, "
                "mean block 3): kernel times from one rocprofv3 --kernel-trace --stats process, ratios against the plain Gaussian "
                "kernel; whole-call wall-clock medians from a process without the profiler",
        "generated_by": "tools/bootstrap_probe.py",
        "kernels": k,
        "ratio_boot_lds_vs_gauss": k["boot_lds"]["avg_ms"] / g,
        "ratio_boot_global_vs_gauss": k["boot_global"]["avg_ms"] / g,
        "ratio_boot_lds_hz_vs_boot_lds": k["boot_lds_hz"]["avg_ms"] / k["boot_lds"]["avg_ms"],
        "hard_bar_no_slower": k["boot_lds"]["avg_ms"] <= g,
        "target_0_6": k["boot_lds"]["avg_ms"] <= 0.6 * g,
    }
    if calls_json:
        c = json.load(open(calls_json))
        res["calls"] = c
        res["call_ratio_boot_lds_vs_gauss"] = c["boot_lds"]["median_ms"] / c["gauss"]["median_ms"]
        res["call_ratio_boot_global_vs_gauss"] = c["boot_global"]["median_ms"] / c["gauss"]["median_ms"]
    if pmc:
        sw, nosw = counters(pmc[0]), counters(pmc[1])
        res["lds_counters"] = {
            "what": "counter-only runs (rocprofv3 --pmc, one process per arm, all dispatches of a --calls 1 run summed): the LDS "
                    "row table XOR-swizzled (this build) and unswizzled (lab build -DMCP_EXP_BOOT_SWIZZLE=0)",
            "swizzled": sw, "unswizzled": nosw,
            "bank_conflict_ratio_boot_lds": sw["boot_lds"]["SQ_LDS_BANK_CONFLICT"] / nosw["boot_lds"]["SQ_LDS_BANK_CONFLICT"],
            "lds_idx_active_ratio_boot_lds": sw["boot_lds"]["SQ_LDS_IDX_ACTIVE"] / nosw["boot_lds"]["SQ_LDS_IDX_ACTIVE"],
        }
        print(f"swizzle: SQ_LDS_BANK_CONFLICT x{res['lds_counters']['bank_conflict_ratio_boot_lds']:.3f}, "
              f"SQ_LDS_IDX_ACTIVE x{res['lds_counters']['lds_idx_active_ratio_boot_lds']:.3f}")
    for key in ("ratio_boot_lds_vs_gauss", "ratio_boot_global_vs_gauss", "ratio_boot_lds_hz_vs_boot_lds"):
        print(f"{key:32s} {res[key]:.4f}")
    for key, v in k.items():
        print(f"kernel {key:12s} {v['avg_ms']:.4f} ms  ({v['calls']} calls)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--time", action="store_true", help="print and save the call times")
    ap.add_argument("--summarize", default=None, help="rocprofv3 output directory of a --calls run")
    ap.add_argument("--calls-json", default=None)
    ap.add_argument("--pmc", nargs=2, default=None, metavar=("SWIZZLED_DIR", "UNSWIZZLED_DIR"),
                    help="with --summarize: the two counter-only run directories")
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    res = summarize(a.summarize, a.calls_json, a.pmc) if a.summarize else calls(a.calls, a.time)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Cost of a spending rule (SPEC.md 4.16 / 5.16) at BASELINE configs[1]'s shape (16 assets, 10^6 paths, 252 steps, four horizons), K = 1
and K = 8, Gaussian draws: mc_paths_spend_kernel under a floor-and-ceiling rule reviewed every 21 steps and under the constant rule
(no review: the twin's walk) against its twin, mc_paths_cf_kernel of the same build, on the same withdrawal in the same process, and
the whole calls.  The twin is the parent commit's kernel by code digest (profiles/spend_isa.txt), whose VALU ratio of the two step
loops is the yardstick for the kernel-time ratio.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/spend_probe.py --rounds 5      (kernel times)
  python tools/spend_probe.py --rounds 5 --time -o calls_a.json                                              (call times)
  python tools/spend_probe.py --rounds 5 --time -o calls_b.json                          (the same command again: the spread)
  python tools/spend_probe.py --summarize DIR --rounds 5 --calls-json calls_a.json calls_b.json -o profiles/spend_probe.json

Every configuration is first warmed up with --warm calls; then --rounds rounds each run every configuration once, so the twin and the
spending kernels alternate through the whole timed window; cf_again repeats the twin after its variants (an A/A pair: the noise of a
ratio).  Calls are synchronous and each has exactly one path-kernel dispatch (K = 8 is one pass of the 8-portfolio kernel), so the
kernel trace is cut at the path kernels.  A spending call reduces one more array than its twin (the total paid out: a pass 0 and a
select), which shows in the call times and in all_dispatches_ms, not in the kernel times.  Kernel and call times are medians over the
rounds; ratios of the medians."""
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

from monte_carlo_portfolio_amd import simulate_paths, spending_rule, synthetic  # noqa: E402

N, T, P = 16, 252, 1_000_000
HZ = dict(horizons=[21, 63, 126, 252], bands=(5.0, 50.0, 95.0))
TAKE = 0.001                       # taken out per step, a quarter of v0 over the walk: no path is ruined, the statistics passes of both calls
                                   # see the same kind of values
RULES = {"spend": spending_rule("floor_ceiling", TAKE, every=21, down=0.025, up=0.05, inflation=0.002, first=TAKE),
         "spend_const": spending_rule("constant", TAKE, every=0, first=TAKE)}


def configs():
    """[(name, kernel-name substring, call)] in the order the probe runs them"""
    mu, cov = synthetic.synthetic_market(N)
    out = []
    for K in (1, 8):
        w = synthetic.dirichlet_weights(N, K) if K > 1 else synthetic.equal_weights(N)
        kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED, **HZ)
        out.append((f"K{K}_cf", "mc_paths_cf_kernel<", lambda w=w, kw=kw: simulate_paths(mu, cov, w, cashflow=-TAKE, **kw)))
        for name, rule in RULES.items():
            out.append((f"K{K}_{name}", "mc_paths_spend_kernel<", lambda w=w, kw=kw, rule=rule: simulate_paths(mu, cov, w, spending=rule, **kw)))
        out.append((f"K{K}_cf_again", "mc_paths_cf_kernel<", lambda w=w, kw=kw: simulate_paths(mu, cov, w, cashflow=-TAKE, **kw)))
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
            print(f"call {name:16s} {v['median_ms']:9.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})")
    return res


def base(name):
    """the configuration a ratio is taken against: K8_spend -> K8_cf, K1_cf_again -> K1_cf"""
    return name.split("_")[0] + "_cf"


def has_ratio(name):
    return "_spend" in name or name.endswith("_again")


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
        k[name] = {"kernel": mine[0][0]["Kernel_Name"].split("(")[0], "median_ms": med(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t,
                   "all_dispatches_ms": med([sum(ms(r) for r in c) for c in mine])}
    res = {
        "what": "Spending rules (SPEC.md 4.16 / 5.16) at configs[1]'s shape (N = 16, T = 252, 10^6 paths, horizons 21 / 63 / 126 / 252), K = 1 "
                "and 8, Gaussian draws, 0.001 v0 taken out per step (no ruin): kernel times of mc_paths_spend_kernel under a floor-and-ceiling "
                "rule reviewed every 21 steps and under the constant rule (no review) against the twin mc_paths_cf_kernel of the same build "
                f"on the same withdrawal, from one rocprofv3 --kernel-trace --stats process; every configuration warmed up ({warm} calls), "
                f"then {rounds} rounds that each run every configuration once (twin and variants alternate); medians over the rounds and "
                "ratios of the medians; *_cf_again is the A/A pair of the twin.  Whole-call wall-clock medians from two more processes "
                "without the profiler (the same command twice: the spread between processes); a spending call reduces one more array, "
                "the total paid out",
        "generated_by": "tools/spend_probe.py",
        "kernels": k,
        "ratios_vs_twin": {name: v["median_ms"] / k[base(name)]["median_ms"] for name, v in k.items() if has_ratio(name)},
    }
    for j, cj in enumerate(calls_json or []):
        c = json.load(open(cj))
        res[f"calls_{j}"] = c
        res[f"call_ratios_vs_twin_{j}"] = {name: v["median_ms"] / c[base(name)]["median_ms"] for name, v in c.items() if has_ratio(name)}
    for name, v in k.items():
        r = res["ratios_vs_twin"].get(name)
        cr = "  ".join(f"call x{res[f'call_ratios_vs_twin_{j}'][name]:.3f}" for j in range(len(calls_json or []))
                       if name in res[f"call_ratios_vs_twin_{j}"])
        print(f"kernel {name:16s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]" + (f"  x{r:.4f}  {cr}" if r else ""))
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

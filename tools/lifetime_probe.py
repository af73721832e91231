"""Cost of the lifetime (SPEC.md 4.17 / 5.17) at N = 16, T = 252, 10^6 paths, K = 1 and K = 8, Gaussian draws: the cash-flow and the
spending call with lifetime=True against the same call without it, in the same process.  The call without it runs the parent commit's
kernels by code digest (profiles/lifetime_isa.txt), so it is the parent's call; the VALU ratio of the two step loops in that file is
the expectation the kernel-time ratio is held against.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/lifetime_probe.py --rounds 5      (kernel times)
  python tools/lifetime_probe.py --rounds 5 --time -o calls_a.json                                              (call times)
  python tools/lifetime_probe.py --rounds 5 --time -o calls_b.json                          (the same command again: the spread)
  python tools/lifetime_probe.py --summarize DIR --rounds 5 --calls-json calls_a.json calls_b.json -o profiles/lifetime_probe.json

Every configuration is first warmed up with --warm calls; then --rounds rounds each run every configuration once, so the calls with
and without the lifetime alternate through the whole timed window; *_again repeats the call without it (an A/A pair: the noise of a
ratio).  Calls are synchronous and each has exactly one path-kernel dispatch, so the kernel trace is cut at the path kernels; the
lifetime's histogram pass is the life_hist_kernel dispatch of the call.  Medians over the rounds; ratios of the medians."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monte_carlo_portfolio_amd import simulate_paths, spending_rule, synthetic  # noqa: E402

N, T, P = 16, 252, 1_000_000
TAKE = 0.0045                      # taken out per step: more than v0 over the walk, so that a good share of the paths is ruined inside it and the
                                   # histogram has mass on many bins
RULE = spending_rule("floor_ceiling", TAKE, every=21, down=0.025, up=0.05, inflation=0.002, first=TAKE)
KERNELS = {"cf": "mc_paths_cf_kernel<", "cf_life": "mc_paths_glide_life_kernel<", "spend": "mc_paths_spend_kernel<",
           "spend_life": "mc_paths_spend_life_kernel<", "cf_again": "mc_paths_cf_kernel<", "spend_again": "mc_paths_spend_kernel<"}


def configs():
    """[(name, kernel-name substring, call)] in the order the probe runs them"""
    mu, cov = synthetic.synthetic_market(N)
    out = []
    for K in (1, 8):
        w = synthetic.dirichlet_weights(N, K) if K > 1 else synthetic.equal_weights(N)
        kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED)
        for name in ("cf", "cf_life", "cf_again", "spend", "spend_life", "spend_again"):
            how = dict(cashflow=-TAKE) if name.startswith("cf") else dict(spending=RULE)
            if name.endswith("_life"):
                how["lifetime"] = True
            out.append((f"K{K}_{name}", KERNELS[name], lambda w=w, kw=kw, how=how: simulate_paths(mu, cov, w, **how, **kw)))
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
    """the configuration a ratio is taken against: K8_spend_life -> K8_spend, K1_cf_again -> K1_cf"""
    return name.rsplit("_", 1)[0]


def has_ratio(name):
    return name.endswith(("_life", "_again"))


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
                   "all_dispatches_ms": med([sum(ms(r) for r in c) for c in mine]),
                   "life_hist_ms": med([sum(ms(r) for r in c if "life_hist" in r["Kernel_Name"]) for c in mine])}
    res = {
        "what": f"The lifetime (SPEC.md 4.17 / 5.17) at N = {N}, T = {T}, {P} paths, K = 1 and 8, Gaussian draws, {TAKE} v0 taken out per "
                "step (a share of the paths is ruined inside the walk): kernel times of the lifetime twins against the kernels of the same "
                "call without the lifetime -- the parent commit's kernels by code digest -- from one rocprofv3 --kernel-trace --stats "
                f"process; every configuration warmed up ({warm} calls), then {rounds} rounds that each run every configuration once; medians "
                "over the rounds and ratios of the medians; *_again is the A/A pair.  life_hist_ms is the histogram pass of the call.  "
                "Whole-call wall-clock medians from two more processes without the profiler (the same command twice: the spread between "
                "processes)",
        "generated_by": "tools/lifetime_probe.py",
        "kernels": k,
        "ratios_vs_call_without": {name: v["median_ms"] / k[base(name)]["median_ms"] for name, v in k.items() if has_ratio(name)},
    }
    for j, cj in enumerate(calls_json or []):
        c = json.load(open(cj))
        res[f"calls_{j}"] = c
        res[f"call_ratios_vs_call_without_{j}"] = {name: v["median_ms"] / c[base(name)]["median_ms"] for name, v in c.items() if has_ratio(name)}
    for name, v in k.items():
        r = res["ratios_vs_call_without"].get(name)
        cr = "  ".join(f"call x{res[f'call_ratios_vs_call_without_{j}'][name]:.3f}" for j in range(len(calls_json or []))
                       if name in res[f"call_ratios_vs_call_without_{j}"])
        print(f"kernel {name:16s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]  hist {v['life_hist_ms']:.4f} ms"
              + (f"  x{r:.4f}  {cr}" if r else ""))
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

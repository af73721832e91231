"""Cost of the two regimes of the Markov switching (SPEC.md 2.6 / 4.13) at BASELINE configs[1]'s shape (16 assets, 10^6 paths, 252
steps), K = 1 and K = 8: mc_paths_r_kernel, mc_paths_r_dd_kernel and mc_paths_r_hz_kernel, each against its Gaussian twin (what the
same call without `regimes` runs: mc_paths_lean_kernel for K = 1 and mc_paths_kernel for K = 8, mc_paths_dd_kernel,
mc_paths_hz_kernel -- kernels whose code the regime kernels' commit leaves as the parent commit has it, profiles/regime_isa.txt) in
the same process, and the whole calls.  Two variants per twin: `mixed` (p01 = 0.05, p10 = 0.2, the stationary start: most waves hold
paths of both regimes and walk both chains) and `calm` (start = 0, p01 = 0: every wave sits in regime 0 and skips regime 1's chain).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/regime_probe.py --rounds 5      (kernel times)
  python tools/regime_probe.py --rounds 5 --time -o calls_a.json                                             (call times)
  python tools/regime_probe.py --rounds 5 --time -o calls_b.json                        (the same command again: the spread)
  python tools/regime_probe.py --summarize DIR --rounds 5 --calls-json calls_a.json calls_b.json -o profiles/regime_probe.json

Every configuration is first warmed up with --warm calls; then --rounds rounds each run every configuration once, in the order
twin, mixed, calm, twin again, so twins and variants alternate through the whole timed window and every twin has an A/A repeat
(the noise a ratio is read against).  Calls are synchronous, so the path-kernel dispatches of the kernel trace fall to the
configurations in that order (one dispatch per call: K = 8 is one pass of the 8-portfolio kernel).  Kernel and call times are
medians over the rounds; the ratios are those of the medians."""
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

from monte_carlo_portfolio_amd import simulate_paths, synthetic  # noqa: E402

N, T, P = 16, 252, 1_000_000
MIXED, CALM = (0.05, 0.2), (0.0, 0.2, 0.0)          # (p01, p10[, start]); no start: the stationary one
HZ = dict(horizons=[21, 63, 126, 252], bands=(5.0, 50.0, 95.0))
FAMILIES = (("plain", {}, ""), ("dd", {"drawdown": True}, "dd_"), ("hz", HZ, "hz_"))


def configs():
    """[(name, kernel-name substrings, call)] in the order the probe runs them: per K and family the twin, the two regime variants
    and the twin again (an A/A pair: the noise of a ratio).  Regime 1 is the market with every mean 1 % lower and every volatility
    doubled; the factors are passed as they are, so the twin and regime 0 walk on the same L."""
    mu, cov = (np.asarray(a, np.float64) for a in synthetic.synthetic_market(N))
    L = np.linalg.cholesky(cov)
    mu1, L1 = mu - 0.01, 2.0 * L
    out = []
    for K in (1, 8):
        w = synthetic.dirichlet_weights(N, K) if K > 1 else synthetic.equal_weights(N)
        kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED, chol=L)
        for fam, fkw, fk in FAMILIES:
            twin = lambda w=w, kw=kw, fkw=fkw: simulate_paths(mu, cov, w, **fkw, **kw)                  # noqa: E731
            mixed = lambda w=w, kw=kw, fkw=fkw: simulate_paths(mu, cov, w, regimes=MIXED[:2] + (mu1, L1), **fkw, **kw)             # noqa: E731
            calm = lambda w=w, kw=kw, fkw=fkw: simulate_paths(mu, cov, w, regimes=CALM[:2] + (mu1, L1, CALM[2]), **fkw, **kw)      # noqa: E731
            tpat = (f"mc_paths_{fk}kernel<", "mc_paths_lean_kernel<") if fam == "plain" else (f"mc_paths_{fk}kernel<",)
            out.append((f"K{K}_{fam}_twin", tpat, twin))
            out.append((f"K{K}_{fam}_mixed", (f"mc_paths_r_{fk}kernel<",), mixed))
            out.append((f"K{K}_{fam}_calm", (f"mc_paths_r_{fk}kernel<",), calm))
            out.append((f"K{K}_{fam}_again", tpat, twin))
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
    """the twin of a configuration: K8_dd_mixed -> K8_dd_twin"""
    return name.rsplit("_", 1)[0] + "_twin"


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
        assert all(any(p in r["Kernel_Name"] for p in pat) for r in mine), (name, mine[0]["Kernel_Name"])
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in mine]
        k[name] = {"kernel": mine[0]["Kernel_Name"].split("(")[0], "median_ms": statistics.median(ms), "min_ms": min(ms),
                   "max_ms": max(ms)}
    res = {
        "what": "the two regimes of the Markov switching (SPEC.md 2.6 / 4.13) at configs[1]'s shape (N = 16, T = 252, 10^6 paths), K = 1 "
                "and 8: kernel times of mc_paths_r_kernel / mc_paths_r_dd_kernel / mc_paths_r_hz_kernel, mixed (p01 = 0.05, p10 = 0.2) and "
                "all calm (start = 0, p01 = 0), each against its Gaussian twin (the kernel the same call without `regimes` runs, code "
                "as in the parent commit) and the twin's A/A repeat, from one rocprofv3 --kernel-trace --stats "
                f"process; every configuration warmed up ({warm} calls), then {rounds} rounds that each run every configuration once "
                "(twins and variants alternate); medians over the rounds and ratios of the medians.  Whole-call wall-clock "
                "medians from two more processes without the profiler (the same command twice: the spread between processes)",
        "regimes": {"mixed": list(MIXED), "calm": list(CALM)},
        "generated_by": "tools/regime_probe.py",
        "kernels": k,
        "ratios_vs_twin": {name: v["median_ms"] / k[base(name)]["median_ms"] for name, v in k.items() if not name.endswith("_twin")},
    }
    for j, cj in enumerate(calls_json or []):
        c = json.load(open(cj))
        res[f"calls_{j}"] = c
        res[f"call_ratios_vs_twin_{j}"] = {name: v["median_ms"] / c[base(name)]["median_ms"] for name, v in c.items()
                                           if not name.endswith("_twin")}
    for name, v in k.items():
        r = res["ratios_vs_twin"].get(name)
        calls = "  ".join(f"call x{res[f'call_ratios_vs_twin_{j}'][name]:.3f}" for j in range(len(calls_json or []))
                          if name in res[f"call_ratios_vs_twin_{j}"])
        print(f"kernel {name:28s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]" + (f"  x{r:.3f}  {calls}" if r else ""))
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

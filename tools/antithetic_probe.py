"""Cost of antithetic pairs (SPEC.md 2.3) at BASELINE configs[1]'s shape (16 assets, 10^6 paths, 252 steps), K = 1 and K = 8:
mc_paths_anti_kernel on the Gaussian plain, drawdown and horizon walks and on Student-t draws with nu = 5, each at 10^6 paths (5 10^5
lanes) against its twin without pairs at 10^6 paths (mc_paths_kernel / mc_paths_dd_kernel / mc_paths_hz_kernel / mc_paths_t_kernel) in
the same process.  The twins' code is the parent commit's (tools/isa_digests.py: every existing symbol keeps its digest).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/antithetic_probe.py --rounds 5     (kernel times)
  python tools/antithetic_probe.py --summarize DIR --rounds 5 -o profiles/antithetic_probe.json

Every configuration is first warmed up with --warm calls; then --rounds rounds each run every configuration once, in the order
twin, antithetic variant, twin again, so twins and variants alternate through the whole timed window and every twin has an A/A
repeat (the noise a ratio is read against).  Calls are synchronous, so the path-kernel dispatches of the kernel trace fall to the
configurations in that order (one dispatch per call: K = 8 is one pass of the 8-portfolio kernel).  Kernel times are medians over
the rounds; the ratios are those of the medians."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monte_carlo_portfolio_amd import simulate_paths, synthetic  # noqa: E402

N, T, P = 16, 252, 1_000_000
NU = 5
HZ = dict(horizons=[21, 63, 126, 252], bands=(5.0, 50.0, 95.0))
WALKS = (("gauss_plain", {}, "mc_paths_kernel<"), ("gauss_dd", {"drawdown": True}, "mc_paths_dd_kernel<"),
         ("gauss_hz", HZ, "mc_paths_hz_kernel<"), (f"t{NU}_plain", {"dof": NU}, "mc_paths_t_kernel<"))


def configs():
    """[(name, kernel-name substring, call)] in the order the probe runs them: per K and walk the twin, the antithetic variant and
    the twin again (an A/A pair: the noise of a ratio)"""
    mu, cov = synthetic.synthetic_market(N)
    out = []
    for K in (1, 8):
        w = synthetic.dirichlet_weights(N, K) if K > 1 else synthetic.equal_weights(N)
        kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED)
        for walk, wkw, twin_kernel in WALKS:
            twin = lambda w=w, kw=kw, wkw=wkw: simulate_paths(mu, cov, w, **wkw, **kw)                       # noqa: E731
            anti = lambda w=w, kw=kw, wkw=wkw: simulate_paths(mu, cov, w, antithetic=True, **wkw, **kw)      # noqa: E731
            out.append((f"K{K}_{walk}_twin", twin_kernel, twin))
            out.append((f"K{K}_{walk}_anti", "mc_paths_anti_kernel<", anti))
            out.append((f"K{K}_{walk}_again", twin_kernel, twin))
    return out


def run(rounds, warm):
    cfg = configs()
    for _ in range(warm + rounds):
        for _, _, f in cfg:
            f()


def summarize(d, rounds, warm):
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
    twin = lambda name: name.rsplit("_", 1)[0] + "_twin"   # noqa: E731
    res = {
        "what": "antithetic pairs (SPEC.md 2.3) at configs[1]'s shape (N = 16, T = 252, 10^6 paths), K = 1 and 8: kernel time of "
                "mc_paths_anti_kernel at 10^6 paths (5 10^5 pairs, one lane each) over its twin's at 10^6 paths -- the Gaussian plain, "
                "drawdown and horizon kernels and the Student-t kernel at nu = 5 -- and the twin's A/A repeat, from one rocprofv3 "
                f"--kernel-trace --stats process; every configuration warmed up ({warm} calls), then {rounds} rounds that each run "
                "every configuration once (twins and variants alternate); medians over the rounds and ratios of the medians",
        "generated_by": "tools/antithetic_probe.py",
        "kernels": k,
        "ratios_vs_twin": {name: v["median_ms"] / k[twin(name)]["median_ms"] for name, v in k.items() if not name.endswith("_twin")},
    }
    for name, v in k.items():
        r = res["ratios_vs_twin"].get(name)
        print(f"kernel {name:24s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]" + (f"  x{r:.3f}" if r else ""))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds; each runs every configuration once")
    ap.add_argument("--warm", type=int, default=2, help="warm-up calls of every configuration before the rounds")
    ap.add_argument("--summarize", default=None, help="rocprofv3 output directory of a run with the same --rounds / --warm")
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    if not a.summarize:
        run(a.rounds, a.warm)
        return 0
    res = summarize(a.summarize, a.rounds, a.warm)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

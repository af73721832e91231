"""Cost of the risk attribution (SPEC.md 4.10 / 5.9) at BASELINE configs[1]'s shape (16 assets, 10^6 paths, 252 steps):
mc_paths_attr_kernel<4, 1, 1> against its twin mc_paths_g_kernel<4, 1, 1> (the same draws without the contributions) on Gaussian
draws and on Student-t draws with nu = 5, in one process, and the whole attribution=True call against the plain call for K = 1 and
K = 8.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/attribution_probe.py --rounds 5      (kernel times)
  python tools/attribution_probe.py --rounds 5 --time -o calls_a.json                                             (call times)
  python tools/attribution_probe.py --rounds 5 --time -o calls_b.json                        (the same command again: the spread)
  python tools/attribution_probe.py --summarize DIR --rounds 5 --calls-json calls_a.json calls_b.json -o profiles/attribution_probe.json

Every configuration is first warmed up with --warm calls; then --rounds rounds each run every configuration once, in the order
twin, attribution, twin again, so twins and variants alternate through the whole timed window and every twin has an A/A repeat (the
noise a ratio is read against).  Calls are synchronous, so the path-kernel dispatches of the kernel trace fall to the configurations
in that order: one dispatch for a twin (alpha = beta = 0, h0 = 1 on mc_paths_g_kernel), and for an attribution call the first
walk's kernel and then K dispatches of mc_paths_attr_kernel.  Kernel and call times are medians over the rounds; the ratios are
those of the medians."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monte_carlo_portfolio_amd import simulate_paths, synthetic  # noqa: E402

N, T, P = 16, 252, 1_000_000
NU = 5
UNIT_GARCH = (0.0, 0.0, 1.0)            # the GARCH kernel on the Gaussian / Student-t call's own values (SPEC.md 4.9)


def configs(timed):
    """[(name, [kernel-name substrings of the call's path dispatches, in order], call)] in the order the probe runs them.  Kernel
    mode (K = 1): per draw source the twin on mc_paths_g_kernel, the attribution call, the twin again.  Call mode (`timed`): per K
    the plain call, the attribution call, the plain call again."""
    mu, cov = synthetic.synthetic_market(N)
    kw = dict(n_steps=T, n_paths=P, seed=synthetic.BENCH_SEED)
    out = []
    if timed:
        for K in (1, 8):
            w = synthetic.dirichlet_weights(N, K) if K > 1 else synthetic.equal_weights(N)
            plain = lambda w=w: simulate_paths(mu, cov, w, **kw)                        # noqa: E731
            attr = lambda w=w: simulate_paths(mu, cov, w, attribution=True, **kw)       # noqa: E731
            out += [(f"K{K}_gauss_twin", [], plain), (f"K{K}_gauss_attr", [], attr), (f"K{K}_gauss_again", [], plain)]
        return out
    w = synthetic.equal_weights(N)
    for draws, dkw, first in (("gauss", {}, "mc_paths_kernel<"), (f"t{NU}", {"dof": NU}, "mc_paths_t_kernel<")):
        twin = lambda dkw=dkw: simulate_paths(mu, cov, w, garch=UNIT_GARCH, **dkw, **kw)        # noqa: E731
        attr = lambda dkw=dkw: simulate_paths(mu, cov, w, attribution=True, **dkw, **kw)        # noqa: E731
        out += [(f"K1_{draws}_twin", ["mc_paths_g_kernel<"], twin), (f"K1_{draws}_attr", [first, "mc_paths_attr_kernel<"], attr),
                (f"K1_{draws}_again", ["mc_paths_g_kernel<"], twin)]
    return out


def run(rounds, warm, timed):
    cfg = configs(timed)
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
            print(f"call {name:20s} {v['median_ms']:9.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})")
    return res


def base(name):
    """the twin of a configuration: K1_t5_attr -> K1_t5_twin"""
    return name.rsplit("_", 1)[0] + "_twin"


def summarize(d, rounds, warm, calls_json):
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    rows = [r for r in csv.DictReader(open(paths[0])) if "mc_paths_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cfg = configs(False)
    per_round = sum(len(pats) for _, pats, _ in cfg)
    if len(rows) != per_round * (warm + rounds):
        raise SystemExit(f"{len(rows)} path-kernel dispatches, expected {per_round * (warm + rounds)}")
    k = {}
    off = 0
    for name, pats, _ in cfg:
        at = off + len(pats) - 1                         # the last dispatch of the call: the twin's kernel, or the attribution kernel
        mine = [rows[per_round * (warm + r) + at] for r in range(rounds)]
        assert all(pats[-1] in r["Kernel_Name"] for r in mine), (name, mine[0]["Kernel_Name"])
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in mine]
        k[name] = {"kernel": mine[0]["Kernel_Name"].split("(")[0], "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
        off += len(pats)
    res = {
        "what": "risk attribution (SPEC.md 4.10 / 5.9) at configs[1]'s shape (N = 16, T = 252, 10^6 paths): kernel times of "
                "mc_paths_attr_kernel<4, 1, 1> on Gaussian draws and at nu = 5 against its twin mc_paths_g_kernel<4, 1, 1> (alpha = beta = "
                "0, h0 = 1: the same draws and values without the contributions) and the twin's A/A repeat, from one rocprofv3 "
                f"--kernel-trace --stats process; every configuration warmed up ({warm} calls), then {rounds} rounds that each run every "
                "configuration once (twins and variants alternate); medians over the rounds and ratios of the medians.  Whole-call "
                "wall-clock medians of simulate_paths(attribution=True) against the plain call (whose kernels are the parent commit's, "
                "profiles/attribution_isa.txt) for K = 1 and K = 8 from two more processes without the profiler (the same command "
                "twice: the spread between processes)",
        "generated_by": "tools/attribution_probe.py",
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
        print(f"kernel {name:20s} {v['median_ms']:8.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]" + (f"  x{r:.3f}" if r else ""))
    for j in range(len(calls_json or [])):
        for name, r in res[f"call_ratios_vs_twin_{j}"].items():
            print(f"call   {name:20s} process {j}: x{r:.3f}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds; each runs every configuration once")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls of every configuration before the rounds")
    ap.add_argument("--time", action="store_true", help="time the whole calls (K = 1 and 8) instead of running the kernel configurations")
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

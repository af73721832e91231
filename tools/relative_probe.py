"""profiles/relative_probe.json: what the benchmark-relative statistics (SPEC.md 5.23) cost, three figures from one process on one box.
   python tools/relative_probe.py [--rounds 3] [--out profiles/relative_probe.json]
1. mcp_launch_relative (kernel and merge kernel, Y written) and mcp_launch_downside over the same [8][10^6] binary32 array on one
   stream: device events around 50 back-to-back launches after 10 warm-up launches, so that the figure is the launch's steady-state
   period, not one launch's latency; `rounds` repeats, alternated.  The relative pass reads 8 B and writes 4 B per element and row
   where the downside pass reads 4 B, and it reads the benchmark's row once per portfolio.
2. The walk that produces such values: one simulate_paths call at N = 16, T = 252, K = 8, 10^6 paths without the keyword (the walk
   and its select), and the same call with benchmark=0; whole-call wall clock, the median of 7 calls after 3 warm-up calls, the two
   alternated per round."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

N, T, PATHS, K = 16, 252, 1_000_000, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(rounds):
    import numpy as np
    import torch
    from monte_carlo_portfolio_amd import _ffi
    lib = _ffi.lib()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    prm = _ffi.make_params(N, T, K)
    vals = torch.from_numpy((1.0 + 0.2 * np.random.default_rng(K).standard_normal((K, PATHS))).astype(np.float32)).to(dev)
    active = torch.zeros((K, PATHS), dtype=torch.float32, device=dev)
    pivot = torch.zeros(K, dtype=torch.float64, device=dev)
    rl_partials = torch.zeros((lib.mcp_relative_ws_bytes(K, PATHS) + 7) // 8, dtype=torch.int64, device=dev)
    ds_partials = torch.zeros((lib.mcp_downside_ws_bytes(K, PATHS) + 7) // 8, dtype=torch.int64, device=dev)
    sums = torch.zeros(K * 18, dtype=torch.int64, device=dev)
    V, C, S = ctypes.c_void_p(vals.data_ptr()), ctypes.c_void_p(pivot.data_ptr()), ctypes.c_void_p(sums.data_ptr())

    def relative():
        _ffi.check(lib.mcp_launch_relative(ctypes.byref(prm), V, PATHS, PATHS, K, K, 0, C, ctypes.c_void_p(rl_partials.data_ptr()), S,
                                           ctypes.c_void_p(active.data_ptr()), st))

    def downside():
        _ffi.check(lib.mcp_launch_downside(ctypes.byref(prm), V, PATHS, PATHS, K, C, 0.0, ctypes.c_void_p(ds_partials.data_ptr()), S, st))

    def period(fn, reps=50):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return 1e3 * a.elapsed_time(b) / reps            # microseconds per launch

    runs = {"relative": [], "downside": []}
    for _ in range(rounds):
        for name, fn in (("relative", relative), ("downside", downside)):
            runs[name].append(period(fn))
    med = {k: statistics.median(v) for k, v in runs.items()}
    return {"relative_us": med["relative"], "relative_range_us": [min(runs["relative"]), max(runs["relative"])],
            "downside_us": med["downside"], "downside_range_us": [min(runs["downside"]), max(runs["downside"])],
            "relative_over_downside": med["relative"] / med["downside"], "relative_bytes": 12 * K * PATHS,
            "relative_gb_per_s": 12 * K * PATHS / med["relative"] / 1e3}


def calls(rounds):
    from monte_carlo_portfolio_amd import simulate_paths, synthetic
    mu, cov = synthetic.synthetic_market(N)
    w = synthetic.dirichlet_weights(N, K)
    runs = {"plain": [], "benchmark": []}
    for _ in range(rounds):
        for name, kw in (("plain", {}), ("benchmark", dict(benchmark=0))):
            ms = []
            for i in range(10):
                t0 = time.perf_counter()
                simulate_paths(mu, cov, w, n_steps=T, n_paths=PATHS, seed=12345, **kw)
                if i >= 3:
                    ms.append(1e3 * (time.perf_counter() - t0))
            runs[name].append(statistics.median(ms))
    med = {k: statistics.median(v) for k, v in runs.items()}
    return {"call_plain_ms": med["plain"], "call_plain_range_ms": [min(runs["plain"]), max(runs["plain"])],
            "call_benchmark_ms": med["benchmark"], "call_benchmark_range_ms": [min(runs["benchmark"]), max(runs["benchmark"])],
            "benchmark_over_plain": med["benchmark"] / med["plain"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/relative_probe.json")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    out = {"what": f"1. microseconds per launch of mcp_launch_relative (kernel and merge kernel, Y written) and of mcp_launch_downside over "
                   f"the same [{K}][{PATHS}] binary32 array, device events around 50 back-to-back launches, medians and ranges of the "
                   f"rounds.  2. whole-call wall clock of simulate_paths at N = {N}, T = {T}, K = {K}, {PATHS} paths without the keyword "
                   "(the walk and its select) and with benchmark=0: medians of 7 calls after 3 warm-up calls, medians and ranges of the "
                   "rounds.  One process, one box, one run.",
           "generated_by": "tools/relative_probe.py", "rounds": a.rounds}
    out.update(kernels(a.rounds))
    out.update(calls(a.rounds))
    out["relative_us_over_plain_call_us"] = out["relative_us"] / (1e3 * out["call_plain_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "what"}))


if __name__ == "__main__":
    main()

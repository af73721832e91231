"""profiles/downside_probe.json: what the downside statistics (SPEC.md 5.22) cost.
   python tools/downside_probe.py [--rounds 3] [--out profiles/downside_probe.json]
1. One simulate_paths call at N = 16, T = 252, 10^6 paths with downside=0.0 beside the same call without it, at K = 1 (the lean
   kernel) and K = 8: whole-call wall clock, fresh processes alternated; every process warms up (3 calls) and reports the median of 7
   timed calls; the driver writes the medians of the process medians and their run-to-run ranges.
2. mcp_launch_downside alone against mcp_launch_pass0 alone over the same [K][10^6] binary32 array (K = 1 and 8), on one stream:
   device events around 50 back-to-back launches after 10 warm-up launches, so that the figure is the launch's steady-state period (the
   kernel and its merge kernel, or pass0 alone, whose histogram simply keeps counting), not one launch's latency; `rounds` repeats,
   alternated.
   Both stream the same 4 B per value; the downside pass forms x by a binary64 division and keeps eleven binary64 sums where pass0
   keeps two and a histogram.
   python tools/downside_probe.py --one plain|downside --k 1|8      one process of part 1: prints its median in ms
   python tools/downside_probe.py --kernels                         part 2 alone: prints its figures"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

N, T, PATHS = 16, 252, 1_000_000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(which, k):
    sys.path.insert(0, ROOT)
    import numpy as np
    from monte_carlo_portfolio_amd import simulate_paths, synthetic
    mu, cov = synthetic.synthetic_market(N)
    w = np.full(N, 1.0 / N) if k == 1 else synthetic.dirichlet_weights(N, k)
    kw = dict(n_steps=T, n_paths=PATHS, seed=12345)
    if which == "downside":
        kw["downside"] = 0.0
    ms = []
    for i in range(10):
        t0 = time.perf_counter()
        simulate_paths(mu, cov, w, **kw)
        if i >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"which": which, "k": k, "median_ms": statistics.median(ms), "all_ms": ms}))


def kernels(rounds):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from monte_carlo_portfolio_amd import _ffi
    lib = _ffi.lib()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for K in (1, 8):
        prm = _ffi.make_params(N, T, K)
        vals = torch.from_numpy((1.0 + 0.2 * np.random.default_rng(K).standard_normal((K, PATHS))).astype(np.float32)).to(dev)
        pivot = torch.zeros(K, dtype=torch.float64, device=dev)
        ws = [torch.zeros((lib.mcp_ws_bytes(w, K, PATHS) + 7) // 8, dtype=torch.int64, device=dev) for w in range(_ffi.WS_COUNT)]
        partials = torch.zeros((lib.mcp_downside_ws_bytes(K, PATHS) + 7) // 8, dtype=torch.int64, device=dev)
        sums = torch.zeros(K * 12, dtype=torch.int64, device=dev)
        V, C = ctypes.c_void_p(vals.data_ptr()), ctypes.c_void_p(pivot.data_ptr())

        def downside():
            _ffi.check(lib.mcp_launch_downside(ctypes.byref(prm), V, PATHS, PATHS, K, C, 0.0, ctypes.c_void_p(partials.data_ptr()),
                                               ctypes.c_void_p(sums.data_ptr()), st))

        def pass0():
            _ffi.check(lib.mcp_launch_pass0(ctypes.byref(prm), V, PATHS, PATHS, C, ctypes.c_void_p(ws[_ffi.WS_PARTIALS].data_ptr()),
                                            ctypes.c_void_p(ws[_ffi.WS_HIST].data_ptr()), st))

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

        runs = {"downside": [], "pass0": []}
        for _ in range(rounds):
            for name, fn in (("downside", downside), ("pass0", pass0)):
                runs[name].append(period(fn))
        med = {k: statistics.median(v) for k, v in runs.items()}
        out[f"k{K}"] = {"downside_us": med["downside"], "downside_range_us": [min(runs["downside"]), max(runs["downside"])],
                        "pass0_us": med["pass0"], "pass0_range_us": [min(runs["pass0"]), max(runs["pass0"])],
                        "downside_over_pass0": med["downside"] / med["pass0"], "bytes": 4 * K * PATHS,
                        "downside_gb_per_s": 4 * K * PATHS / med["downside"] / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/downside_probe.json")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.k)
    if a.kernels:
        return print(json.dumps(kernels(a.rounds)))
    arms = [(f"{which}_k{k}", which, k) for k in (1, 8) for which in ("plain", "downside")]
    runs = {name: [] for name, _, _ in arms}
    for _ in range(a.rounds):
        for name, which, k in arms:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", which, "--k", str(k)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"{name} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["median_ms"])
    k = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels", "--rounds", str(max(a.rounds, 3))], capture_output=True, text=True, timeout=300)
    if k.returncode != 0:
        sys.exit(f"kernels failed ({k.returncode}):\n{k.stdout[-2000:]}{k.stderr[-2000:]}")
    med = {name: statistics.median(v) for name, v in runs.items()}
    out = {"what": f"1. whole-call wall clock of simulate_paths at N = {N}, T = {T}, {PATHS} paths, K = 1 and K = 8: the call without the keyword "
                   "and the call with downside = 0.0; fresh processes alternated, each the median of 7 calls after 3 warm-up calls; the "
                   "medians of the process medians and their run-to-run ranges.  2. `kernels`: microseconds per launch of "
                   "mcp_launch_downside (kernel and merge kernel) and of mcp_launch_pass0 (one kernel) over the same "
                   f"[K][{PATHS}] binary32 array, device events around 50 back-to-back launches, medians and ranges of the rounds",
           "generated_by": "tools/downside_probe.py", "rounds": a.rounds}
    for name in runs:
        out[f"{name}_median_ms"] = med[name]
        out[f"{name}_range_ms"] = [min(runs[name]), max(runs[name])]
    for kk in (1, 8):
        out[f"downside_over_plain_k{kk}"] = med[f"downside_k{kk}"] / med[f"plain_k{kk}"]
    out["kernels"] = json.loads(k.stdout.strip().splitlines()[-1])
    out["process_medians_ms"] = runs
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k_: v for k_, v in out.items() if k_ != "what"}))


if __name__ == "__main__":
    main()

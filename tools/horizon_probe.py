"""Cost of the values at intermediate horizons (SPEC.md 4.3 / 5.2) at BASELINE configs[1] (16 assets, 10^6 paths, 252 steps,
one portfolio) with 12 monthly horizons and 3 band levels: the path kernel with and without the horizon stores, and the whole
simulate_paths(horizons=..., bands=...) call against the plain call.

  python tools/horizon_probe.py [--reps 7] [-o profiles/horizon_probe.json]

Kernel times are HIP-event times of back-to-back launches (mcp_launch_paths vs mcp_launch_paths_horizons, statistics epilogue
on, as a call runs them), A and B interleaved, median of the repetitions.  Call times are wall-clock medians of synchronous
simulate_paths calls (the default context, store=False)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from monte_carlo_portfolio_amd import _ffi, simulate_paths, synthetic  # noqa: E402
from monte_carlo_portfolio_amd.simulate import prepare_inputs  # noqa: E402

HORIZONS = list(range(21, 253, 21))          # 12 monthly horizons of a 252-step year, T itself the last
LEVELS = (2.5, 50.0, 97.5)


def kernel_ms(n_assets, n_steps, n_paths, reps, launches):
    lib = _ffi.lib()
    mu, cov = synthetic.synthetic_market(n_assets)
    mu32, L, W32 = prepare_inputs(mu, cov, synthetic.equal_weights(n_assets))
    prm = _ffi.make_params(n_assets, n_steps, 1)
    dev = torch.device("cuda", 0)
    packed = torch.from_numpy(_ffi.pack_params(mu32, L, W32)).to(dev)
    pivot = torch.from_numpy(_ffi.pivots(prm, mu32, L, W32)).to(dev)
    term = torch.empty(n_paths, dtype=torch.float32, device=dev)
    hz = torch.empty(len(HORIZONS) * n_paths, dtype=torch.float32, device=dev)
    steps = np.asarray(HORIZONS, np.int32)
    part = torch.zeros(lib.mcp_ws_bytes(_ffi.WS_PARTIALS, 1, n_paths), dtype=torch.uint8, device=dev)
    hist = torch.zeros(lib.mcp_ws_bytes(_ffi.WS_HIST, 1, n_paths), dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = ctypes.byref(prm)

    def plain():
        _ffi.check(lib.mcp_launch_paths(p, packed.data_ptr(), pivot.data_ptr(), synthetic.BENCH_SEED, 0, n_paths, term.data_ptr(),
                                        n_paths, part.data_ptr(), hist.data_ptr(), stream))

    def horizons():
        _ffi.check(lib.mcp_launch_paths_horizons(p, packed.data_ptr(), pivot.data_ptr(), synthetic.BENCH_SEED, 0, n_paths,
                                                 term.data_ptr(), n_paths, len(HORIZONS), steps.ctypes.data_as(ctypes.c_void_p),
                                                 hz.data_ptr(), n_paths, part.data_ptr(), hist.data_ptr(), stream))

    out = {"plain": [], "hz": []}
    for f in (plain, horizons):
        f()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, f in (("plain", plain), ("hz", horizons)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / launches)
    a, b = statistics.median(out["plain"]), statistics.median(out["hz"])
    return {"assets": n_assets, "steps": n_steps, "paths": n_paths, "horizons": len(HORIZONS), "plain_ms": a, "hz_ms": b,
            "ratio": b / a, "plain_ms_all": out["plain"], "hz_ms_all": out["hz"]}


def call_ms(n_paths, reps):
    mu, cov = synthetic.synthetic_market(16)
    w = synthetic.equal_weights(16)
    kw = dict(n_steps=252, n_paths=n_paths, seed=synthetic.BENCH_SEED)
    hk = dict(horizons=HORIZONS, bands=LEVELS)
    simulate_paths(mu, cov, w, **kw)
    simulate_paths(mu, cov, w, **kw, **hk)
    out = {"plain": [], "hz": []}
    for _ in range(reps):
        for name, extra in (("plain", {}), ("hz", hk)):
            t0 = time.perf_counter()
            simulate_paths(mu, cov, w, **kw, **extra)
            out[name].append((time.perf_counter() - t0) * 1e3)
    a, b = statistics.median(out["plain"]), statistics.median(out["hz"])
    return {"assets": 16, "steps": 252, "paths": n_paths, "horizons": len(HORIZONS), "levels": len(LEVELS), "plain_ms": a,
            "hz_ms": b, "ratio": b / a, "plain_ms_all": out["plain"], "hz_ms_all": out["hz"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    res = {
        "what": "values at intermediate horizons (SPEC.md 4.3 / 5.2) cost: path kernel with / without the horizon stores, and "
                "the whole call with 12 horizons and 3 levels",
        "generated_by": "tools/horizon_probe.py",
        "device": torch.cuda.get_device_name(0),
        "horizon_steps": HORIZONS,
        "levels": list(LEVELS),
        "kernel_configs1": kernel_ms(16, 252, 1_000_000, a.reps, 10),
        "call_1e6": call_ms(1_000_000, a.reps),
    }
    for key in ("kernel_configs1", "call_1e6"):
        r = res[key]
        print(f"{key:16s} N={r['assets']:2d} T={r['steps']:4d} n={r['paths']:.0e} H={r['horizons']}: plain {r['plain_ms']:.3f} ms, "
              f"horizons {r['hz_ms']:.3f} ms, ratio {r['ratio']:.4f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

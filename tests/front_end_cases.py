"""What the Python front end does with its keywords, recorded without a GPU: which mcp_simulate* entry point a call reaches and
the kind of every positional argument it passes, or the exception it raises.  The library's mcp_simulate* functions are replaced
by a recorder that returns 0; nothing is launched.  tests/golden/make_front_end_cases.py runs this on a checkout of the parent
commit to write tests/golden/front_end_cases.json; tests/test_front_end_cpu.py runs it on the tree under test and compares."""
import contextlib
import ctypes
import itertools

import numpy as np

N, K, PATHS = 3, 1, 8
CALL_KEYWORDS = ("rows", "dof", "period", "drawdown", "horizons", "flows", "overlay", "garch", "attribution", "antithetic", "filtered",
                 "jumps", "regimes", "glide")


def kind(v):
    """NULL, an integer's value, an array's dtype and shape (`ptr` in front where only its address is passed), a struct's name."""
    if v is None:
        return "NULL"
    if isinstance(v, (bool, int, np.integer)):
        return int(v)
    if isinstance(v, np.ndarray):
        return f"{v.dtype.name}{list(v.shape)}"
    if isinstance(v, ctypes.c_void_p):
        arr = getattr(v, "_arr", None)                     # ndarray.ctypes.data_as keeps its array there
        return "NULL" if not v.value else "ptr" if arr is None else f"ptr {arr.dtype.name}{list(arr.shape)}"
    if isinstance(v, ctypes.Structure):
        return type(v).__name__
    if hasattr(v, "_obj"):                                 # ctypes.byref(struct)
        return type(v._obj).__name__
    return f"?{type(v).__name__}"


class Recorder:
    """Stands in for the loaded library: mcp_simulate* note their arguments, set the path count `n` of every mcp_stats record they
    are handed (the front end divides by it) and return 0; everything else is `real`'s."""

    def __init__(self, real=None):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if not name.startswith("mcp_simulate"):
            return getattr(self.real, name)

        def entry(*args):
            self.calls.append([name, [kind(a) for a in args]])
            for arr in (getattr(a, "_arr", None) for a in args):
                if arr is not None and "n" in (arr.dtype.names or ()):
                    arr["n"] = PATHS
            return 0
        return entry


@contextlib.contextmanager
def recording(real=None):
    """-> (Recorder, Context with a NULL handle): _ffi.lib and simulate.default_context are replaced inside the block."""
    from monte_carlo_portfolio_amd import _ffi, simulate
    rec = Recorder(real)
    ctx = simulate.Context.__new__(simulate.Context)
    ctx._h, ctx.device, ctx.devices = ctypes.c_void_p(), 0, (0,)
    saved = _ffi.lib, simulate.default_context
    _ffi.lib, simulate.default_context = (lambda: rec), (lambda device=0: ctx)
    try:
        yield rec, ctx
    finally:
        _ffi.lib, simulate.default_context = saved


def record(rec, fn):
    """One case: {"raises": [type, text]} or {"calls": [[entry, [kinds]]], "keys": sorted keys of the dict returned, if any}."""
    del rec.calls[:]
    try:
        res = fn()
    except Exception as e:                                 # noqa: BLE001 -- the type is what is recorded
        return {"raises": [type(e).__name__, str(e)]}
    if isinstance(res, list) and res and isinstance(res[0], dict):
        res = res[0]
    out = {"calls": [list(c) for c in rec.calls]}
    if isinstance(res, dict):
        out["keys"] = sorted(res)
    return out


def subsets(names):
    """The empty set, every single name and every pair."""
    return [()] + [(a,) for a in names] + list(itertools.combinations(names, 2))


def call_cases():
    """Context._call at N = 3, T = 5, K = 1, 8 paths, store=True for the empty set, every single and every pair of CALL_KEYWORDS."""
    from monte_carlo_portfolio_amd import _ffi
    f32 = np.float32
    mu, chol, W = np.full(N, 1e-3, f32), (0.01 * np.eye(N)).astype(f32), np.full((K, N), 1 / N, f32)
    table = np.array([(_ffi.MCP_OVERLAY_PUT, 0.9, 0.01, 1.0)], _ffi.OVERLAY_ROW_DTYPE)
    values = {
        "rows": dict(rows=np.full((6, N), 1e-3, f32), block=2.0), "dof": dict(dof=5), "period": dict(period=2, cost=1e-3),
        "drawdown": dict(drawdown=True), "horizons": dict(horizons=np.array([2, 5], np.int32), levels=np.array([5.0, 50.0])),
        "flows": dict(flows=np.full(5, 0.01, f32), target=1.0),
        "overlay": dict(overlay=(table, np.array([0, 1, 1, 1], np.int32), np.ones(N, f32))), "garch": dict(garch=(0.05, 0.9, 1.0)),
        "attribution": dict(attribution=True), "antithetic": dict(antithetic=True),
        "filtered": dict(filtered=(np.zeros(N, f32), np.full((6, N), 1e-3, f32), np.ones(6, f32))),
        "jumps": dict(jumps=(0.1, -0.01, 0.01, None)), "regimes": dict(regimes=(0.05, 0.2, 0.1, mu.copy(), chol.copy())),
        "glide": dict(glide=(np.array([2], np.int32), np.full((1, K, N), 1 / N, f32))),
    }
    out = {}
    with recording() as (rec, ctx):
        prm = _ffi.make_params(N, 5, K)
        for names in subsets(CALL_KEYWORDS):
            kw = {} if "rows" in names or "filtered" in names else dict(mu=mu, chol=chol)      # rows bring their own draws
            for n in names:
                kw.update(values[n])
            out["+".join(names)] = record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, True, **kw))
    return out


def public_cases(real):
    """simulate_paths, simulate_bootstrap, simulate_filtered and simulate_sweep at N = 3, n_steps=6, n_paths=8 over the recorder
    wrapped around the loaded library `real` (the host helpers behind the 'jumps' and 'regimes' blocks are its own)."""
    from monte_carlo_portfolio_amd import options, simulate as sim
    mu, cov, w = np.full(N, 1e-3), 1e-4 * np.eye(N), np.full(N, 1 / N)
    paths = {
        "drawdown": dict(drawdown=True), "horizons": dict(horizons=[2, 6], bands=(5.0, 50.0)), "rebalance": dict(rebalance=2),
        "dof": dict(dof=5), "cashflow": dict(cashflow=0.01, target=1.0),
        "overlay": dict(overlay={0: [(options.LONG_PUT, 90.0, 1.0, 1.0)]}, spot=[100.0, 100.0, 100.0]), "garch": dict(garch=(0.05, 0.9)),
        "attribution": dict(attribution=True), "antithetic": dict(antithetic=True), "jumps": dict(jumps=(0.1, -0.01, 0.01)),
        "regimes": dict(regimes=(0.05, 0.2, np.full(N, -1e-3), 4e-4 * np.eye(N))), "glide": dict(glide=([2], [[0.5, 0.25, 0.25]])),
        "fold": dict(fold=True), "native_math": dict(native_math=True), "log": dict(compounding="log"), "shard": dict(shard="portfolios"),
    }
    returns = np.linspace(-0.02, 0.02, 10 * N).reshape(10, N)
    boot = {k: paths[k] for k in ("horizons", "rebalance", "cashflow", "glide", "log", "shard")}
    boot.update(block=dict(block=3.0), cost=dict(rebalance_cost=1e-3))
    boot_refused = {k: paths[k] for k in ("overlay", "attribution", "antithetic", "garch", "dof", "fold", "native_math", "drawdown")}
    boot_refused.update(spot=dict(spot=[1.0] * N), chol=dict(chol=np.eye(N)), overlay_none=dict(overlay=None),
                        attribution_off=dict(attribution=False), antithetic_off=dict(antithetic=False), jumps=paths["jumps"],
                        regimes=paths["regimes"])
    triple = (np.zeros(N), returns, np.ones(10))
    filt_refused = {k: paths[k] for k in ("log", "dof", "fold", "native_math", "drawdown", "rebalance", "cashflow", "overlay", "attribution",
                                          "antithetic", "jumps", "regimes", "glide")}
    sweep = {"plain": {}, "drawdown": paths["drawdown"], "horizons": dict(horizons=[2, 6]), "bands": dict(bands=(5.0,)),
             "cashflow": dict(cashflow=0.01), "target": dict(target=1.0), "glide": paths["glide"], "attribution": paths["attribution"],
             "antithetic": paths["antithetic"], "attribution_off": dict(attribution=False), "antithetic_off": dict(antithetic=False)}
    W2 = np.array([[0.5, 0.25, 0.25], [0.2, 0.3, 0.5]])

    def merged(table, names):
        kw = {}
        for n in names:
            kw.update(table[n])
        return kw
    out = {}
    with recording(real) as (rec, _):
        for names in subsets(sorted(paths)):
            kw = merged(paths, names)
            out["paths:" + "+".join(names)] = record(rec, lambda: sim.simulate_paths(mu, cov, w, n_steps=6, n_paths=PATHS, **kw))
        for names in subsets(sorted(boot)):
            kw = merged(boot, names)
            out["bootstrap:" + "+".join(names)] = record(rec, lambda: sim.simulate_bootstrap(returns, w, n_steps=6, n_paths=PATHS, **kw))
        for name, kw in boot_refused.items():
            out["bootstrap:" + name] = record(rec, lambda: sim.simulate_bootstrap(returns, w, n_steps=6, n_paths=PATHS, **kw))
        for name, kw in [("", {}), ("horizons", dict(horizons=[2, 6], levels=(5.0,)))] + list(filt_refused.items()):
            out["filtered:" + name] = record(rec, lambda: sim.simulate_filtered(triple, w, n_steps=6, n_paths=PATHS, garch=(0.05, 0.9), **kw))
        out["filtered:no garch"] = record(rec, lambda: sim.simulate_filtered(triple, w, n_steps=6, n_paths=PATHS))
        for name, kw in sweep.items():
            out["sweep:" + name] = record(rec, lambda: sim.simulate_sweep(mu, cov, weights=W2, n_steps=6, n_paths=PATHS, **kw))
    return out


def argtypes():
    """The argument types of every row of _ffi.SIGNATURES, by name."""
    from monte_carlo_portfolio_amd import _ffi
    return {name: [t.__name__ for t in args] for name, (_, args) in sorted(_ffi.SIGNATURES.items())}

"""GPU checks of filtered historical simulation (SPEC.md 2.4 / 4.11 / 5.11): every path bit-equal to the NumPy restatement
(fhs_ref.py) over widths, portfolio counts, block lengths and both placements of the row and shock tables, each of the four
mc_paths_fhs_kernel instances of every NB used; the bootstrap at alpha = 0, h0 = 1; horizon rows, bands and records against NumPy
on the stored values; shards and tiles; the variance law from the kernel's stored rows; recovery after a refused call."""
import contextlib
import ctypes
import io
import math
import os
import runpy
import sys

import numpy as np
import pytest

from bootstrap_ref import simulate_boot
from fhs_ref import law_check, law_inputs, simulate_fhs
from horizons_ref import x_of
from oracle import ref_stats
from monte_carlo_portfolio_amd import _ffi, simulate_bootstrap, simulate_filtered, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xF11_7E12
N_PATHS = 2 * 256 + 37            # two full workgroups and a ragged third
GARCH = (0.25, 0.6, 2.0)
Q_ALPHA = (1 - 0.95) * 100


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(R, N, K, seed=0):
    rng = np.random.default_rng(seed + 1000 * N + R)
    mu = (rng.standard_normal(N) * 0.002).astype(np.float32)
    resid = (rng.standard_t(4, size=(R, N)) * 0.015).astype(np.float32)
    shock = (rng.chisquare(3, size=R) / 3.0).astype(np.float32)
    W = rng.dirichlet(np.ones(N), size=K).astype(np.float32)
    return mu, resid, shock, W


CASES = [  # N, K, T, block, R: the tables sit in LDS while R ceil(N/4) + ceil(R/4) <= 1088; K = 1 is the KT = 1 kernel, K >= 2 KT = 8
    (1, 1, 7, 1.0, 40),            # NB = 1: LDS, KT = 1
    (1, 1, 7, math.inf, 5000),     #         global, KT = 1
    (3, 3, 60, 2.5, 40),           #         LDS, KT = 8
    (3, 3, 60, 1.0, 5000),         #         global, KT = 8
    (16, 1, 60, 1.0, 256),         # NB = 4: the last size in LDS, KT = 1
    (16, 1, 60, 2.5, 257),         #         the first size in global memory, KT = 1
    (16, 9, 7, math.inf, 256),     #         LDS, KT = 8, two passes
    (16, 9, 7, 1.0, 257),          #         global, KT = 8
    (17, 1, 7, 1.0, 207),          # NB = 5: the last size in LDS, KT = 1
    (17, 1, 7, 2.5, 208),          #         global, KT = 1
    (17, 20, 7, 2.5, 40),          #         LDS, KT = 8, three passes
    (17, 20, 7, math.inf, 5000),   #         global, KT = 8
    (64, 1, 7, math.inf, 66),      # NB = 16: the last size in LDS, KT = 1
    (64, 1, 7, 1.0, 67),           #          global, KT = 1
    (64, 3, 7, 1.0, 40),           #          LDS, KT = 8
    (64, 3, 7, 2.5, 5000),         #          global, KT = 8
]


@pytest.mark.parametrize("N,K,T,b,R", CASES)
def test_every_path_equals_the_restatement(N, K, T, b, R, gpu_ctx):
    mu, resid, shock, W = _inputs(R, N, K)
    begin = (1 << 32) - 300                                   # the path ids cross 2^32
    hz = sorted({1, (T + 1) // 2, T})
    prm = _ffi.make_params(N, T, K, v0=2.0)
    plain = gpu_ctx.simulate_filtered(prm, (mu, resid, shock), GARCH, W, b, SEED, begin, N_PATHS, True)
    out = gpu_ctx.simulate_filtered(prm, (mu, resid, shock), GARCH, W, b, SEED, begin, N_PATHS, True, horizons=hz, levels=(50.0,))
    ref = simulate_fhs(mu, resid, shock, W, T, SEED, (begin + np.arange(N_PATHS)).astype(np.uint64), b, GARCH, v0=2.0, horizons=hz)
    assert len(np.unique(ref["h"][-1])) > 1                   # the variance ratio moved
    assert np.array_equal(_bits(plain.terminal), _bits(ref["V_T"]))
    assert np.array_equal(_bits(out.terminal), _bits(ref["V_T"]))
    assert np.array_equal(_bits(out.horizon_terminal), _bits(ref["V_h"]))


@pytest.mark.parametrize("K", [1, 9])
@pytest.mark.parametrize("R", [100, 5000])
def test_without_dynamics_it_is_the_bootstrap_on_the_shifted_rows(R, K, gpu_ctx):
    N, T, b = 16, 24, 2.5
    mu, resid, shock, W = _inputs(R, N, K, seed=3)
    rows = (resid.astype(np.float64) + mu.astype(np.float64)).astype(np.float32)
    hz = [1, 7, 24]
    prm = _ffi.make_params(N, T, K)
    got = gpu_ctx.simulate_filtered(prm, (mu, resid, shock), (0.0, 0.7, 1.0), W, b, SEED, 5, N_PATHS, True, horizons=hz)
    _, _, _, term, hzt = gpu_ctx.simulate_bootstrap_horizons(prm, rows, W, b, SEED, 5, N_PATHS, hz, (), True)
    assert np.array_equal(_bits(got.terminal), _bits(term)) and np.array_equal(_bits(got.horizon_terminal), _bits(hzt))
    plain = gpu_ctx.simulate_filtered(prm, (mu, resid, shock), (0.0, 0.7, 1.0), W, b, SEED, 5, N_PATHS, True)
    _, term1 = gpu_ctx.simulate_bootstrap(prm, rows, W, b, SEED, 5, N_PATHS, True)
    assert np.array_equal(_bits(plain.terminal), _bits(term1))
    moved = gpu_ctx.simulate_filtered(prm, (mu, resid, shock), (0.2, 0.7, 1.0), W, b, SEED, 5, N_PATHS, True)
    assert not np.array_equal(_bits(moved.terminal), _bits(term1))


def _order_stats(x, q):
    lo, hi, g = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double()
    _ffi.check(_ffi.lib().mcp_percentile_rank_q(x.size, q, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(g)))
    xs = np.sort(x)
    return xs[lo.value], xs[hi.value]


@pytest.mark.parametrize("R", [40, 5000])
def test_horizon_rows_bands_and_records_on_the_stored_values(R, gpu_ctx):
    N, K, T, b = 16, 3, 24, 2.5
    mu, resid, shock, W = _inputs(R, N, K, seed=7)
    hz, levels = [1, 5, 12, 24], (2.5, 50.0, 97.5)
    n = 20_011
    tri = (mu, resid, shock)
    out = gpu_ctx.simulate_filtered(_ffi.make_params(N, T, K), tri, GARCH, W, b, SEED, 3, n, True, horizons=hz, levels=levels)
    assert np.array_equal(out.horizon_terminal[-1], out.terminal)
    for i, h in enumerate(hz):
        short = gpu_ctx.simulate_filtered(_ffi.make_params(N, h, K), tri, GARCH, W, b, SEED, 3, n, True)
        assert np.array_equal(_bits(out.horizon_terminal[i]), _bits(short.terminal)), h
        for k in range(K):
            x = x_of(out.horizon_terminal[i, k])
            hs = out.hz_stats[i, k]
            assert hs["var"] == short.stats[k]["var"] == np.percentile(x, Q_ALPHA) and hs["n_tail"] == short.stats[k]["n_tail"]
            assert hs["min"] == x.min() and hs["max"] == x.max()
            for j, q in enumerate(levels):
                assert out.bands[i, k, j] == np.percentile(x, q), (h, k, q)
    for k in range(K):                                         # the records of the call against the reference's definitions
        want = ref_stats.path_stats(out.terminal[k])
        st = out.stats[k]
        x = x_of(out.terminal[k])
        lo, hi = _order_stats(x, Q_ALPHA)
        assert st["n"] == n and st["var"] == want["var"] and st["n_tail"] == want["n_tail"]
        assert st["x_lo"] == lo and st["x_hi"] == hi and st["min"] == want["min"] and st["max"] == want["max"]
        assert abs(st["mean"] - want["mean"]) <= 1e-12 * max(1.0, abs(want["mean"]))
        assert abs(st["std"] - want["std"]) <= 1e-12 * max(1e-3, want["std"])
        assert abs(st["cvar"] - want["cvar"]) <= 1e-12 * max(1.0, abs(want["cvar"]))


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_logical_shards_and_portfolio_shards_equal_one_shard(devices, gpu_ctx):
    N, K, T = 16, 20, 30
    mu, resid, shock, W = _inputs(5000, N, K, seed=9)
    tri, prm = (mu, resid, shock), _ffi.make_params(N, T, K)
    one = gpu_ctx.simulate_filtered(prm, tri, GARCH, W, 4.0, SEED, 11, 30_001, True)
    c = Context(devices)
    try:
        sh = c.simulate_filtered(prm, tri, GARCH, W, 4.0, SEED, 11, 30_001, True)
        sp = c.simulate_filtered(_ffi.make_params(N, T, K, shard_portfolios=True), tri, GARCH, W, 4.0, SEED, 11, 30_001, True)
        hz = c.simulate_filtered(prm, tri, GARCH, W, 4.0, SEED, 11, 30_001, True, horizons=[10, 30], levels=(50.0,))
    finally:
        c.close()
    assert np.array_equal(one.terminal, sh.terminal) and np.array_equal(one.terminal, sp.terminal)
    assert np.array_equal(one.terminal, hz.terminal) and np.array_equal(hz.horizon_terminal[-1], one.terminal)
    for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi", "cvar"):
        assert np.array_equal(one.stats[f], sh.stats[f]) and np.array_equal(one.stats[f], sp.stats[f]), f
        assert np.array_equal(one.stats[f], hz.stats[f]), f
    assert np.allclose(one.stats["mean"], sh.stats["mean"], rtol=1e-12) and np.allclose(one.stats["std"], sp.stats["std"], rtol=1e-12)


def test_small_terminal_budget_tiles_the_portfolios(gpu_ctx):
    N, K, T = 4, 20, 12
    mu, resid, shock, W = _inputs(2000, N, K, seed=2)
    tri, prm = (mu, resid, shock), _ffi.make_params(N, T, K)
    want = gpu_ctx.simulate_filtered(prm, tri, GARCH, W, 2.5, SEED, 0, 10_000, True)
    c = Context(0, terminal_budget=3 * 10_000 * 4)
    try:
        got = c.simulate_filtered(prm, tri, GARCH, W, 2.5, SEED, 0, 10_000, True)
        ghz = c.simulate_filtered(prm, tri, GARCH, W, 2.5, SEED, 0, 10_000, True, horizons=[4, 12], levels=(5.0, 95.0))
    finally:
        c.close()
    assert np.array_equal(want.terminal, got.terminal) and np.array_equal(want.terminal, ghz.terminal)
    for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi"):
        assert np.array_equal(want.stats[f], got.stats[f]) and np.array_equal(want.stats[f], ghz.stats[f]), f


def test_variance_law_from_the_stored_horizon_rows(gpu_ctx):
    """SPEC.md 4.11 at b = 1, the inputs and the bound of the CPU test: at every step |mean((rho_t - w.mu)^2) - E[h_t] M| is within 5
    standard errors, rho_t = V_t / V_{t-1} - 1 in binary64 from the binary32 rows (their rounding is under 1e-5 of the level)."""
    f, w, g = law_inputs()
    res = simulate_filtered(f, w, n_steps=6, n_paths=1_000_000, garch=g, block=1.0, seed=2024, horizons=[1, 2, 3, 4, 5, 6], store=True,
                            context=gpu_ctx)
    V = np.concatenate([np.ones((1, 1_000_000)), res["horizon_terminal"].astype(np.float64)])
    rho = V[1:] / V[:-1] - 1.0
    z, rel, Eh = law_check(rho, f, w, g)
    print("z", z, "relative standard error", rel, "E[h]", Eh)
    assert np.all(np.abs(z) <= 5.0), z


def test_refused_calls_leave_the_staging_buffers_intact(gpu_ctx):
    N, K, T, n = 16, 3, 40, 50_000
    mu_g, cov = synthetic.synthetic_market(N)
    mu32, L, W32 = prepare_inputs(mu_g, cov, synthetic.dirichlet_weights(N, K))
    mu, resid, shock, _ = _inputs(100, N, K, seed=4)
    rows = (resid + mu).astype(np.float32)
    prm = _ffi.make_params(N, T, K)
    g0 = gpu_ctx.simulate(prm, mu32, L, W32, 77, 0, n, True)
    b0 = gpu_ctx.simulate_bootstrap(prm, rows, W32, 2.0, SEED, 0, n, True)
    with pytest.raises(_ffi.McpError):
        gpu_ctx.simulate_filtered(_ffi.make_params(N, T, K, compounding="log"), (mu, resid, shock), GARCH, W32, 2.0, SEED, 0, 1000, False)
    with pytest.raises(ValueError):
        simulate_filtered((mu, resid, shock), W32, n_steps=T, n_paths=1000, garch=GARCH, dof=5, context=gpu_ctx)
    bad = shock.copy()
    bad[50] = -1.0
    with pytest.raises(_ffi.McpError):
        gpu_ctx.simulate_filtered(prm, (mu, resid, bad), GARCH, W32, 2.0, SEED, 0, 1000, False)
    f1 = gpu_ctx.simulate_filtered(prm, (mu, resid, shock), GARCH, W32, 2.0, SEED, 0, n, True)
    ids = np.arange(0, n, 997, dtype=np.uint64)
    assert np.array_equal(_bits(f1.terminal[:, ::997]), _bits(simulate_fhs(mu, resid, shock, W32, T, SEED, ids, 2.0, GARCH)["V_T"]))
    b1 = gpu_ctx.simulate_bootstrap(prm, rows, W32, 2.0, SEED, 0, n, True)
    g1 = gpu_ctx.simulate(prm, mu32, L, W32, 77, 0, n, True)
    assert np.array_equal(b0[1], b1[1]) and np.array_equal(b0[0], b1[0])
    assert np.array_equal(g0[1], g1[1]) and np.array_equal(g0[0], g1[0])
    assert np.array_equal(_bits(b1[1][:, ::997]), _bits(simulate_boot(rows, W32, T, SEED, ids, 2.0)["V_T"]))


def test_simulate_filtered_returns_simulate_bootstrap_shapes(gpu_ctx):
    f, w, _ = law_inputs()
    one = simulate_filtered(f, w, n_steps=12, n_paths=5000, block=3.0, store=True, horizons=[1, 6, 12], levels=(5.0, 95.0), context=gpu_ctx)
    assert one["n"] == 5000 and one["terminal"].shape == (5000,) and one["horizons"]["bands"].shape == (3, 2)
    assert one["horizon_terminal"].shape == (3, 5000)
    same = simulate_filtered((f.mu, f.resid, f.shock), w, n_steps=12, n_paths=5000, garch=(f.alpha, f.beta, f.h0), block=3.0,
                             context=gpu_ctx)
    assert same["var"] == one["var"] and same["mean"] == one["mean"]
    many = simulate_filtered(f, np.eye(5), n_steps=12, n_paths=5000, context=gpu_ctx)
    assert isinstance(many, list) and len(many) == 5
    arr = simulate_filtered(f, np.eye(5), n_steps=12, n_paths=5000, as_array=True, context=gpu_ctx)
    assert arr.shape == (5,) and arr.dtype == _ffi.STATS_DTYPE
    boot = simulate_bootstrap(f.resid.astype(np.float64) + f.mu.astype(np.float64), w, n_steps=12, n_paths=5000, block=3.0, context=gpu_ctx)
    flat = simulate_filtered(f, w, n_steps=12, n_paths=5000, garch=(0.0, 0.0, 1.0), block=3.0, context=gpu_ctx)
    assert flat["var"] == boot["var"] and flat["cvar"] == boot["cvar"]


def test_pipeline_prints_the_filtered_fan(gpu_ctx):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        mod = runpy.run_path(os.path.join(ROOT, "examples", "pipeline.py"), run_name="pipeline_test")
    finally:
        sys.path.pop(0)
    data = os.path.join(ROOT, "tests", "golden", "data")
    files = [os.path.join(data, f) for f in ("Avalanche Historical Data.csv", "Cardano Historical Data.csv",
                                             "NEAR_USD Binance Historical Data.csv")]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mod["main"](files, n_paths=20_000)
    text = out.getvalue()
    assert text.count("filtered-rows fan after") == 3 and text.count("GARCH fan after") == 3
    assert text.count("bootstrap fan after") == 3 and text.count("forecast fan after") == 3

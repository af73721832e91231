"""GPU checks of the GARCH(1,1) variance ratio (SPEC.md 4.9 / 5.8): terminal, drawdown and horizon values bit-equal to the NumPy
restatement (garch_ref.py) over widths, portfolio counts, step counts, Gaussian and Student-t draws, starts at and away from 1 and
a path range across 2^32; the anchors against the calls without GARCH; the records and bands against NumPy on the stored values;
the law of the variance at 10^6 paths; the shards, the tiles, recovery after a rejected call; and the examples' lines."""
import contextlib
import ctypes
import io
import os
import runpy
import sys

import numpy as np
import pytest

from garch_ref import LAW_GARCH, law_checks, law_market, simulate_garch
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, metrics, simulate_paths, simulate_sweep, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs
from oracle import ref_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x6A_4C11


def _market(N, K, seed=0):
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(seed + 31 * N + K).dirichlet(np.ones(N), size=K)
    if K > 1:
        W[-1] *= 0.9                                     # 10 % cash in one portfolio
    return prepare_inputs(mu, cov, W)


def _pick(n_paths, begin, count=12):
    ids = {0, 1, n_paths - 1, n_paths // 2}
    ids.update(np.linspace(0, n_paths - 1, count).astype(int).tolist())
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 3)))
    return np.array(sorted(ids), np.int64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(ctx, prm, g, mu, L, W, begin, n, store=True, **kw):
    return ctx.simulate_garch(prm, g, mu, L, W, SEED, begin, n, store, **kw)


def _gauss(ctx, prm, mu, L, W, begin, n):
    """(stats, terminal) of the Gaussian call on the path kernels: mcp_simulate, or for K >= 17 -- where mcp_simulate runs the MFMA
    sweep kernels, whose moment partials are laid out differently -- the terminal block of mcp_simulate_drawdown."""
    if prm.n_portfolios <= 16:
        return ctx.simulate(prm, mu, L, W, SEED, begin, n, True)
    st, _, term, _ = ctx.simulate_drawdown(prm, mu, L, W, SEED, begin, n, True)
    return st, term


CASES = [  # N, dof, K, T, path_begin, n_paths, (alpha, beta, h0)
    (1, None, 1, 7, 0, 3000, (0.10, 0.85, 1.0)),
    (1, 3, 1, 30, 0, 3000, (0.10, 0.85, 2.5)),
    (3, None, 3, 60, (1 << 32) - 1500, 3000, (0.08, 0.80, 2.5)),
    (3, 4, 3, 60, (1 << 32) - 1500, 3000, (0.20, 0.70, 0.4)),
    (13, 5, 8, 1, 17, 5000, (0.15, 0.80, 1.0)),
    (13, None, 8, 12, 17, 5000, (0.15, 0.80, 3.0)),
    (16, None, 1, 60, 0, 4096, (0.05, 0.90, 1.0)),
    (16, 8, 1, 60, 0, 4096, (0.05, 0.90, 0.25)),
    (16, 32, 3, 0, 0, 1000, (0.10, 0.85, 2.0)),
    (17, None, 20, 7, 5, 2000, (0.30, 0.60, 1.5)),
    (17, 9, 20, 7, 5, 2000, (0.10, 0.85, 1.0)),
    (64, None, 3, 7, (1 << 32) - 7, 300, (0.10, 0.85, 4.0)),
    (64, 32, 3, 7, (1 << 32) - 7, 300, (0.50, 0.45, 1.0)),
    (3, None, 1, 12, 0, 1_000_003, (0.10, 0.85, 2.5)),
    (3, 9, 1, 12, 0, 1_000_003, (0.10, 0.85, 1.0)),
]


@pytest.mark.parametrize("N,dof,K,T,begin,n,g", CASES)
def test_terminal_values_equal_the_restatement(N, dof, K, T, begin, n, g, gpu_ctx):
    mu, L, W = _market(N, K, 3)
    out = _run(gpu_ctx, _ffi.make_params(N, T, K), g, mu, L, W, begin, n, dof=dof)
    st, term = out.stats, out.terminal
    ids = _pick(n, begin, 6 if N >= 16 and T > 7 else 12)
    ref = simulate_garch(mu, L, W, T, SEED, (begin + ids).astype(np.uint64), g, dof=dof)
    assert np.array_equal(_bits(term[:, ids]), _bits(ref["V_T"]))
    for k in (0, K - 1):
        want = ref_stats.path_stats(term[k])
        assert st[k]["var"] == want["var"] and st[k]["n_tail"] == want["n_tail"]
        assert st[k]["min"] == want["min"] and st[k]["max"] == want["max"] and st[k]["n"] == n
        for f in ("mean", "std", "sharpe", "cvar"):
            assert abs(st[k][f] - want[f]) <= 1e-12 * max(1.0, abs(want[f])), f


@pytest.mark.parametrize("N,dof,K,g", [(3, None, 1, (0.10, 0.85, 2.5)), (3, 5, 1, (0.10, 0.85, 1.0)), (16, None, 3, (0.08, 0.80, 0.5)),
                                       (16, 9, 3, (0.08, 0.80, 2.5)), (5, None, 20, (0.2, 0.7, 1.0)), (5, 32, 20, (0.2, 0.7, 3.0)),
                                       (64, None, 8, (0.10, 0.85, 2.5))])
def test_horizon_rows_are_the_n_steps_h_calls_and_the_bands_np_percentile(N, dof, K, g, gpu_ctx):
    T, n, hz, lv = 24, 20_000, [1, 5, 12, 24], (2.5, 50.0, 97.5)
    mu, L, W = _market(N, K, 5)
    out = _run(gpu_ctx, _ffi.make_params(N, T, K), g, mu, L, W, 3, n, dof=dof, horizons=hz, levels=lv)
    for i, h in enumerate(hz):
        oh = _run(gpu_ctx, _ffi.make_params(N, h, K), g, mu, L, W, 3, n, dof=dof)
        assert np.array_equal(_bits(out.horizon_terminal[i]), _bits(oh.terminal))
        for k in range(K):
            x = x_of(out.horizon_terminal[i, k])
            assert out.hz_stats[i, k]["var"] == np.percentile(x, (1 - 0.95) * 100) == oh.stats[k]["var"]
            for j, q in enumerate(lv):
                assert out.bands[i, k, j] == np.percentile(x, q)
    plain = _run(gpu_ctx, _ffi.make_params(N, T, K), g, mu, L, W, 3, n, dof=dof)
    assert np.array_equal(_bits(out.terminal), _bits(plain.terminal)) and plain.stats.tobytes() == out.stats.tobytes()
    ids = _pick(n, 3, 6)
    ref = simulate_garch(mu, L, W, T, SEED, (3 + ids).astype(np.uint64), g, dof=dof, horizons=hz)
    assert np.array_equal(_bits(out.horizon_terminal[:, :, ids]), _bits(ref["V_h"]))


@pytest.mark.parametrize("N,dof,K,T,g", [(1, None, 1, 30, (0.10, 0.85, 2.5)), (3, 4, 1, 30, (0.10, 0.85, 1.0)),
                                         (16, None, 3, 12, (0.08, 0.80, 2.5)), (16, 5, 3, 12, (0.08, 0.80, 0.5)),
                                         (17, None, 20, 5, (0.2, 0.7, 1.0)), (17, 32, 20, 5, (0.2, 0.7, 3.0)),
                                         (13, None, 8, 9, (0.3, 0.6, 2.0))])
def test_drawdown_equals_the_restatement(N, dof, K, T, g, gpu_ctx):
    n = 30_000
    mu, L, W = _market(N, K, 7)
    out = _run(gpu_ctx, _ffi.make_params(N, T, K), g, mu, L, W, 9, n, dof=dof, drawdown=True)
    plain = _run(gpu_ctx, _ffi.make_params(N, T, K), g, mu, L, W, 9, n, dof=dof)
    assert np.array_equal(_bits(out.terminal), _bits(plain.terminal)) and plain.stats.tobytes() == out.stats.tobytes()
    ids = _pick(n, 9, 6)
    ref = simulate_garch(mu, L, W, T, SEED, (9 + ids).astype(np.uint64), g, dof=dof)
    assert np.array_equal(_bits(out.qd[:, ids]), _bits(ref["q"]))
    assert np.array_equal(_bits(out.terminal[:, ids]), _bits(ref["V_T"]))
    for k in range(K):
        mdd = out.qd[k].astype(np.float64) - 1.0
        dar = metrics.var(mdd, 0.95)
        dd = out.dd_stats
        assert dd[k]["var"] == dar and int(dd[k]["n_tail"]) == int(np.count_nonzero(mdd <= dar))
        assert dd[k]["min"] == mdd.min() and dd[k]["max"] == mdd.max() and dd[k]["sharpe"] == 0.0
        assert abs(dd[k]["cvar"] - metrics.cvar(mdd, 0.95)) <= 1e-12
        assert abs(dd[k]["mean"] - mdd.mean()) <= 1e-12


@pytest.mark.parametrize("N,K,T", [(1, 1, 30), (3, 3, 12), (16, 1, 40), (16, 8, 12), (17, 20, 6), (64, 3, 5)])
@pytest.mark.parametrize("beta", [0.0, 0.85, 0.9990000128746033])
def test_alpha_zero_from_one_is_the_call_without_garch(N, K, T, beta, gpu_ctx):
    n, prm = 20_000, _ffi.make_params(N, T, K)
    mu, L, W = _market(N, K, 1)
    g = (0.0, beta, 1.0)
    st, term = _gauss(gpu_ctx, prm, mu, L, W, 7, n)
    out = _run(gpu_ctx, prm, g, mu, L, W, 7, n)
    assert np.array_equal(_bits(out.terminal), _bits(term)) and out.stats.tobytes() == st.tobytes()
    t = gpu_ctx.simulate_student_t(prm, 5, mu, L, W, SEED, 7, n, True)
    out = _run(gpu_ctx, prm, g, mu, L, W, 7, n, dof=5)
    assert np.array_equal(_bits(out.terminal), _bits(t[4])) and out.stats.tobytes() == t[0].tobytes()
    hz = sorted({1, max(1, T // 2), T})
    h = gpu_ctx.simulate_horizons(prm, mu, L, W, SEED, 7, n, hz, (5.0, 95.0), True)
    out = _run(gpu_ctx, prm, g, mu, L, W, 7, n, horizons=hz, levels=(5.0, 95.0))
    assert np.array_equal(_bits(out.horizon_terminal), _bits(h[4])) and out.hz_stats.tobytes() == h[1].tobytes()
    assert np.array_equal(out.bands, h[2]) and out.stats.tobytes() == h[0].tobytes()
    d = gpu_ctx.simulate_student_t(prm, 7, mu, L, W, SEED, 7, n, True, drawdown=True)
    out = _run(gpu_ctx, prm, g, mu, L, W, 7, n, dof=7, drawdown=True)
    assert np.array_equal(_bits(out.qd), _bits(d[5])) and out.dd_stats.tobytes() == d[1].tobytes()
    d = gpu_ctx.simulate_drawdown(prm, mu, L, W, SEED, 7, n, True)
    out = _run(gpu_ctx, prm, g, mu, L, W, 7, n, drawdown=True)
    assert np.array_equal(_bits(out.qd), _bits(d[3])) and out.dd_stats.tobytes() == d[1].tobytes()


@pytest.mark.parametrize("N,K,dof", [(1, 1, None), (3, 3, 4), (16, 1, None), (16, 8, 9), (17, 20, None)])
def test_from_one_the_first_step_is_the_call_without_garch(N, K, dof, gpu_ctx):
    n, g = 20_000, (0.3, 0.6, 1.0)
    mu, L, W = _market(N, K, 2)
    prm1 = _ffi.make_params(N, 1, K)
    if dof is None:
        st, term = _gauss(gpu_ctx, prm1, mu, L, W, 0, n)
    else:
        r = gpu_ctx.simulate_student_t(prm1, dof, mu, L, W, SEED, 0, n, True)
        st, term = r[0], r[4]
    one = _run(gpu_ctx, prm1, g, mu, L, W, 0, n, dof=dof)
    assert np.array_equal(_bits(one.terminal), _bits(term)) and one.stats.tobytes() == st.tobytes()
    out = _run(gpu_ctx, _ffi.make_params(N, 9, K), g, mu, L, W, 0, n, dof=dof, horizons=[1, 9], levels=())
    assert np.array_equal(_bits(out.horizon_terminal[0]), _bits(term))
    far = _run(gpu_ctx, prm1, (0.3, 0.6, 2.0), mu, L, W, 0, n, dof=dof)
    assert not np.array_equal(_bits(far.terminal), _bits(term))


def test_records_are_numpy_on_the_stored_values(gpu_ctx):
    N, K, T, n = 16, 3, 12, 200_001
    mu, L, W = _market(N, K, 3)
    prm = _ffi.make_params(N, T, K, v0=10_000.0, alpha=0.99, rf=0.01)
    for dof in (None, 5):
        out = _run(gpu_ctx, prm, (0.10, 0.85, 2.5), mu, L, W, 0, n, dof=dof)
        for k in range(K):
            want = ref_stats.path_stats(out.terminal[k], v0=10_000.0, alpha=0.99, rf=0.01)
            x = x_of(out.terminal[k], v0=10_000.0)
            st = out.stats
            assert st[k]["var"] == np.percentile(x, (1 - 0.99) * 100) == want["var"]
            assert st[k]["n_tail"] == want["n_tail"] and st[k]["min"] == x.min() and st[k]["max"] == x.max()
            for f in ("mean", "std", "sharpe", "cvar"):
                assert abs(st[k][f] - want[f]) <= 1e-12 * max(1.0, abs(want[f])), f


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("h0", [1.0, 2.5])
def test_the_variance_term_structure_the_mean_and_the_clustering(N, h0, gpu_ctx):
    """10^6 paths, horizons 1 .. 24 stored: the assertions of garch_ref.law_checks, which the binary64 twin passes on the CPU
    (test_garch_cpu.test_the_twin_passes_the_law_assertions_at_the_gpu_tests_size)."""
    n, T = 1_000_000, 24
    mu, cov, w = law_market(N)
    mu32, L, W = prepare_inputs(mu, cov, w)
    g = LAW_GARCH + (h0,)
    prm = _ffi.make_params(N, T, 1)
    out = _run(gpu_ctx, prm, g, mu32, L, W, 0, n, horizons=list(range(1, T + 1)), levels=())
    S = L.astype(np.float64) @ L.astype(np.float64).T
    w64 = W[0].astype(np.float64)
    mean_w, var_w = float(w64 @ mu32.astype(np.float64)), float(w64 @ S @ w64)
    print(N, h0, law_checks(out.horizon_terminal[:, 0, :], 1.0, mean_w, var_w, g))
    piv = _ffi.pivots(prm, mu32, L, W)
    assert abs(out.stats[0]["mean"] - piv[0]) < 5 * out.stats[0]["std"] / np.sqrt(n), (out.stats[0]["mean"], piv[0])
    assert piv[0] == pytest.approx((1.0 + mean_w) ** T - 1.0, rel=1e-9)


@pytest.mark.parametrize("N", [1, 3])
def test_the_gaussian_call_shows_no_clustering(N, gpu_ctx):
    n, T = 1_000_000, 24
    mu, cov, w = law_market(N)
    mu32, L, W = prepare_inputs(mu, cov, w)
    h = gpu_ctx.simulate_horizons(_ffi.make_params(N, T, 1), mu32, L, W, SEED, 0, n, list(range(1, T + 1)), (), True)
    S = L.astype(np.float64) @ L.astype(np.float64).T
    w64 = W[0].astype(np.float64)
    print(N, law_checks(h[4][:, 0, :], 1.0, float(w64 @ mu32.astype(np.float64)), float(w64 @ S @ w64), (0.0, 0.0, 1.0), clustered=False))


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_logical_shards_and_portfolio_shards_equal_one_shard(devices, gpu_ctx):
    N, K, T, g = 16, 20, 30, (0.10, 0.85, 2.5)
    mu, L, W = _market(N, K, 9)
    prm = _ffi.make_params(N, T, K)
    hz = dict(horizons=[10, 30], levels=(50.0,))
    one = _run(gpu_ctx, prm, g, mu, L, W, 11, 30_001, **hz)
    one_t = _run(gpu_ctx, prm, g, mu, L, W, 11, 30_001, dof=5, **hz)
    one_dd = _run(gpu_ctx, prm, g, mu, L, W, 11, 30_001, dof=7, drawdown=True)
    c = Context(devices)
    try:
        sh = _run(c, prm, g, mu, L, W, 11, 30_001, **hz)
        sh_t = _run(c, prm, g, mu, L, W, 11, 30_001, dof=5, **hz)
        sp = _run(c, _ffi.make_params(N, T, K, shard_portfolios=True), g, mu, L, W, 11, 30_001, **hz)
        sd = _run(c, prm, g, mu, L, W, 11, 30_001, dof=7, drawdown=True)
    finally:
        c.close()
    for want, other in ((one, sh), (one, sp), (one_t, sh_t)):
        assert np.array_equal(want.terminal, other.terminal) and np.array_equal(want.horizon_terminal, other.horizon_terminal)
        assert np.array_equal(want.bands, other.bands)
        for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi", "cvar"):
            assert np.array_equal(want.stats[f], other.stats[f]) and np.array_equal(want.hz_stats[f], other.hz_stats[f]), f
        assert np.allclose(want.stats["mean"], other.stats["mean"], rtol=1e-12)
        assert np.allclose(want.stats["std"], other.stats["std"], rtol=1e-12)
    assert np.array_equal(one_dd.terminal, sd.terminal) and np.array_equal(one_dd.qd, sd.qd)
    for f in ("var", "n_tail", "min", "max"):
        assert np.array_equal(one_dd.dd_stats[f], sd.dd_stats[f]) and np.array_equal(one_dd.stats[f], sd.stats[f]), f


def test_small_terminal_budget_tiles_the_portfolios(gpu_ctx):
    N, K, T, g = 4, 20, 12, (0.10, 0.85, 0.5)
    mu, L, W = _market(N, K, 2)
    prm = _ffi.make_params(N, T, K)
    kw = dict(dof=6, horizons=[4, 12], levels=(5.0, 95.0))
    want = _run(gpu_ctx, prm, g, mu, L, W, 0, 10_000, **kw)
    c = Context(0, terminal_budget=3 * 3 * 10_000 * 4)
    try:
        got = _run(c, prm, g, mu, L, W, 0, 10_000, **kw)
    finally:
        c.close()
    assert np.array_equal(want.terminal, got.terminal) and np.array_equal(want.horizon_terminal, got.horizon_terminal)
    assert np.array_equal(want.bands, got.bands)
    for f in ("var", "n_tail", "min", "max"):
        assert np.array_equal(want.stats[f], got.stats[f]) and np.array_equal(want.hz_stats[f], got.hz_stats[f])


def test_rejected_call_then_a_correct_one_then_a_gaussian_call(gpu_ctx):
    mu, L, W = _market(16, 3, 1)
    prm = _ffi.make_params(16, 40, 3)
    g = (0.10, 0.85, 2.5)
    g0, gt0 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    fresh = Context(0)
    try:
        want = _run(fresh, prm, g, mu, L, W, 0, 50_000)
    finally:
        fresh.close()
    fn = _ffi.lib().mcp_simulate_garch
    st = np.zeros(3, _ffi.STATS_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    for bad in (_ffi.McpGarch(0.5, 0.5, 1.0, 0), _ffi.McpGarch(0.1, 0.85, 0.0, 0), _ffi.McpGarch(0.1, 0.85, 1.0, 1)):
        assert fn(gpu_ctx._h, ctypes.byref(prm), ctypes.byref(bad), None, vp(mu), vp(L), vp(W), SEED, 0, 50_000, 0, None, 0, None, None,
                  vp(st), None, None, None, None, None) == _ffi.MCP_E_ARG
    with pytest.raises(_ffi.McpError):
        _run(gpu_ctx, _ffi.make_params(16, 40, 3, compounding="log"), g, mu, L, W, 0, 1000, store=False)
    got = _run(gpu_ctx, prm, g, mu, L, W, 0, 50_000)
    assert np.array_equal(want.terminal, got.terminal) and want.stats.tobytes() == got.stats.tobytes()
    g1, gt1 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    assert np.array_equal(gt0, gt1) and g0.tobytes() == g1.tobytes()


def test_simulate_paths_returns_its_shapes(gpu_ctx):
    mu, cov = synthetic.synthetic_market(3)
    one = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, garch=(0.1, 0.85, 2.5), store=True, horizons=[1, 6, 12],
                         bands=(5.0, 95.0), context=gpu_ctx)
    assert one["n"] == 5000 and one["terminal"].shape == (5000,) and one["horizons"]["bands"].shape == (3, 2)
    assert one["horizon_terminal"].shape == (3, 5000)
    dd = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, garch=[0.1, 0.85], dof=np.int64(4), drawdown=True, store=True,
                        context=gpu_ctx)
    assert isinstance(dd, list) and len(dd) == 3 and dd[0]["max_drawdown"].shape == (5000,) and "cdar" in dd[0]["drawdown"]
    arr = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, garch=np.array([0.1, 0.85, 0.5]), as_array=True, context=gpu_ctx)
    assert arr.shape == (3,) and arr.dtype == _ffi.STATS_DTYPE
    s, d = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, garch=(0.1, 0.85), dof=8, drawdown=True, as_array=True,
                          context=gpu_ctx)
    assert s.shape == d.shape == (3,)
    g = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, store=True, context=gpu_ctx)
    assert not np.array_equal(g["terminal"], one["terminal"])
    same = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, garch=(0.0, 0.5), store=True, context=gpu_ctx)
    assert np.array_equal(g["terminal"], same["terminal"]) and g["var"] == same["var"]
    hi = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, garch=(0.1, 0.85, 4.0), context=gpu_ctx)
    assert hi["std"] > 1.3 * g["std"]
    sw = simulate_sweep(mu, cov, weights=np.eye(3), n_steps=12, n_paths=5000, garch=(0.1, 0.85, 2.5), context=gpu_ctx)
    assert np.array_equal(sw["stats"]["var"], simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, garch=(0.1, 0.85, 2.5),
                                                             as_array=True, context=gpu_ctx)["var"])


def test_pipeline_prints_the_garch_lines(gpu_ctx):
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
    assert text.count("GARCH(1,1) fit: alpha = ") == 1 and text.count("GARCH fan after") == 3
    assert text.count("Student-t fan after") == 3 and text.count("bootstrap fan after") == 3 and text.count("forecast fan after") == 3


def test_streamlit_forecast_tab_shows_the_garch_fan(gpu_ctx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_shim import fake_streamlit
    record = []
    sys.modules["streamlit"] = fake_streamlit(record, 50_000)
    try:
        np.random.seed(4242)
        runpy.run_path(os.path.join(ROOT, "examples", "streamlit_app.py"), run_name="__main__")
    finally:
        del sys.modules["streamlit"]
    shown = [r[1][0] for r in record if r[0] == "write" and isinstance(r[1][0], dict) and "GARCH(1,1)" in r[1][0]]
    assert len(shown) == 1
    fit = shown[0]["GARCH(1,1)"]
    assert fit["alpha"] >= 0 and fit["beta"] >= 0 and fit["alpha"] + fit["beta"] < 1 and fit["h0"] > 0
    assert shown[0]["step"] == [1, 3, 6] and all(np.all(np.isfinite(shown[0][f"{q} %"])) for q in (2.5, 50.0, 97.5))
    assert np.all(np.asarray(shown[0]["2.5 %"]) < np.asarray(shown[0]["97.5 %"]))
    charts = [r[1][0] for r in record if r[0] == "line_chart" and isinstance(r[1][0], dict) and "step" in r[1][0]]
    assert len(charts) == 1
    side = [r[1][0] for r in record if r[0] == "write" and isinstance(r[1][0], dict) and "bootstrap of the observed rows" in r[1][0]]
    assert len(side) == 1

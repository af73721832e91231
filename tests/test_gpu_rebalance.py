"""GPU checks of buy-and-hold and periodic rebalancing (SPEC.md 4.5 / 5.4): terminal and horizon values bit-equal to the NumPy
restatement (rebalance_ref.py) over widths, portfolio counts, step counts, periods, costs and draw sources (Gaussian, bootstrap
rows in LDS and in global memory); period 1 against the constant-weight calls; the records against NumPy on the stored values;
the analytic law of buy-and-hold and rebalanced values; the cost; the shards, the tiles, recovery after a rejected call; and the
examples' lines."""
import contextlib
import io
import os
import runpy
import sys

import numpy as np
import pytest

from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, simulate_bootstrap, simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs
from rebalance_ref import boot_returns, gauss_returns, rebalanced

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EB_A1A2CE
Q_ALPHA = (1 - 0.95) * 100


def _market(N, K, seed=0, scale=1.0):
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(seed + 31 * N + K).dirichlet(np.ones(N), size=K)
    if K > 1:
        W[-1] *= 0.9                                     # 10 % cash in one portfolio
    return prepare_inputs(np.asarray(mu) * scale, np.asarray(cov) * scale, W)


def _table(R, N, seed=0):
    return (np.random.default_rng(seed + 1000 * N + R).standard_t(3, size=(R, N)) * 0.02 + 0.001).astype(np.float32)


def _pick(n_paths, begin):
    ids = {0, 1, n_paths - 1, n_paths // 2}
    ids.update(np.linspace(0, n_paths - 1, 20).astype(int).tolist())
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 3)))
    return np.array(sorted(ids), np.int64)


def _hz(T):
    """horizons that end at T (even T) or before it (odd T)"""
    if T < 1:
        return []
    return sorted({1, max(1, T // 2), T if T % 2 == 0 else max(1, T - 1)})


CASES = [  # N, K, T, period (0: never), cost, source, R          (LDS holds the table when R * ceil(N/4) <= 1088)
    (1, 1, 7, 1, 0.0, "gauss", 0),
    (1, 3, 7, 2, 1e-3, "boot", 50),
    (3, 3, 60, 5, 1e-3, "gauss", 0),
    (3, 8, 60, 59, 0.0, "boot", 100_000),
    (3, 17, 60, 1, 0.0, "boot", 40),
    (16, 1, 60, 5, 1e-3, "gauss", 0),
    (16, 1, 60, 60, 1e-3, "boot", 272),
    (16, 8, 60, 1, 1e-3, "boot", 272),
    (16, 17, 7, 2, 1e-3, "gauss", 0),
    (16, 3, 60, 0, 1e-3, "boot", 5000),
    (16, 1, 60, 5, 1e-3, "boot", 5000),            # one portfolio, the table in global memory
    (17, 3, 1, 1, 1e-3, "gauss", 0),
    (17, 1, 0, 0, 0.0, "gauss", 0),
    (17, 8, 7, 6, 1e-3, "boot", 100),
    (64, 1, 7, 7, 1e-3, "gauss", 0),
    (64, 3, 7, 2, 1e-3, "boot", 68),
    (64, 17, 7, 5, 0.0, "boot", 69),
    (64, 8, 60, 21, 1e-3, "gauss", 0),
]


@pytest.mark.parametrize("N,K,T,m,cost,source,R", CASES)
def test_values_equal_the_restatement(N, K, T, m, cost, source, R, gpu_ctx):
    mu, L, W = _market(N, K, N + T)
    rows = _table(R, N) if source == "boot" else None
    begin, n = (1 << 32) - 700, 1337
    hz = _hz(T)
    prm = _ffi.make_params(N, T, K, v0=2.0)
    kw = dict(rows=rows, block=2.5) if rows is not None else dict(mu=mu, chol=L)
    stats, hs, bands, term, hzt = gpu_ctx.simulate_rebalanced(prm, m, cost, W, SEED, begin, n, True,
                                                              horizons=hz if hz else None, levels=(5.0, 50.0), **kw)
    ids = _pick(n, begin)
    paths = (begin + ids).astype(np.uint64)
    r = boot_returns(rows, T, SEED, paths, 2.5) if rows is not None else gauss_returns(mu, L, T, SEED, paths)
    if T == 0:
        r = np.zeros((0, ids.size, 4 * ((N + 3) // 4)), np.float32)
    ref = rebalanced(r, W, m, cost, v0=2.0, horizons=hz)
    assert np.array_equal(term[:, ids].view(np.uint32), ref["V_T"].view(np.uint32))
    if hz:
        assert np.array_equal(hzt[:, :, ids].view(np.uint32), ref["V_h"].view(np.uint32))
    for k in range(K):                                               # the records against NumPy on the stored values
        x = x_of(term[k], "simple", 2.0)
        st = stats[k]
        assert st["n"] == n and st["var"] == np.percentile(x, Q_ALPHA)
        assert st["min"] == x.min() and st["max"] == x.max() and st["n_tail"] == int(np.sum(x <= st["var"]))
        tail = x[x <= st["var"]]
        assert abs(st["cvar"] - tail.mean()) <= 1e-12 * max(1.0, abs(tail.mean()))
        assert abs(st["mean"] - x.mean()) <= 1e-12 * max(1.0, abs(x.mean()))
        assert abs(st["std"] - x.std(ddof=1)) <= 1e-12 * max(1e-3, x.std(ddof=1))
        for i in range(len(hz)):
            xh = x_of(hzt[i, k], "simple", 2.0)
            assert hs[i, k]["var"] == np.percentile(xh, Q_ALPHA)
            assert bands[i, k, 0] == np.percentile(xh, 5.0) and bands[i, k, 1] == np.percentile(xh, 50.0)


@pytest.mark.parametrize("source", ["gauss", "lds", "global"])
def test_period_one_without_cost_is_the_constant_weight_call(source, gpu_ctx):
    N, K, T, n = 16, 3, 24, 20_011
    mu, L, W = _market(N, K, 4)
    hz, levels = [1, 5, 12, 24], (2.5, 50.0, 97.5)
    if source == "gauss":
        call = lambda **kw: simulate_paths(mu, L @ L.T.astype(np.float64), W, n_steps=T, n_paths=n, seed=SEED, path_begin=9,   # noqa: E731
                                           chol=L, store=True, context=gpu_ctx, **kw)
    else:
        rows = _table(272 if source == "lds" else 4000, N, 4)
        call = lambda **kw: simulate_bootstrap(rows, W, n_steps=T, n_paths=n, block=3.0, seed=SEED, path_begin=9,   # noqa: E731
                                               store=True, context=gpu_ctx, **kw)
    for hkw in ({}, {"horizons": hz, "bands": levels}):
        want, got = call(**hkw), call(rebalance=1, **hkw)
        for a, b in zip(want, got):
            assert np.array_equal(a["terminal"].view(np.uint32), b["terminal"].view(np.uint32))
            for f in ("var", "n_tail", "min", "max", "cvar", "x_lo", "x_hi"):
                assert a[f] == b[f], f
            for f in ("mean", "std", "sharpe"):
                assert abs(a[f] - b[f]) <= 1e-12 * max(1e-300, abs(a[f])), f
            if hkw:
                assert np.array_equal(a["horizon_terminal"].view(np.uint32), b["horizon_terminal"].view(np.uint32))
                assert np.array_equal(a["horizons"]["bands"], b["horizons"]["bands"])
                assert np.array_equal(a["horizons"]["var"], b["horizons"]["var"])


@pytest.mark.parametrize("m", [0, 1, 21])
def test_analytic_law(m, gpu_ctx):
    """Gaussian draws, no cost: per segment of length l, with u = 1 - sum W and M_ij = (1+mu_i)(1+mu_j) + (L L^T)_ij,
    E[g] = u + sum_i W_i (1+mu_i)^l, E[g^2] = u^2 + 2u sum_i W_i (1+mu_i)^l + sum_ij W_i W_j M_ij^l; segments are independent."""
    N, K, T, n = 4, 2, 63, 1_000_000
    rng = np.random.default_rng(7)
    mu = rng.normal(0.004, 0.003, N).astype(np.float32)
    A = rng.normal(size=(N, N)) * 0.04
    cov = A @ A.T + 0.0004 * np.eye(N)
    W = np.array([[0.4, 0.3, 0.2, 0.1], [0.5, -0.2, 0.3, 0.2]], np.float64) * np.array([[1.0], [0.9]])
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    term = gpu_ctx.simulate_rebalanced(_ffi.make_params(N, T, K), m, 0.0, W32, SEED, 0, n, True, mu=mu32, chol=L)[3]
    m64, L64, W64 = mu32.astype(np.float64), L.astype(np.float64), W32.astype(np.float64)
    M = np.outer(1 + m64, 1 + m64) + L64 @ L64.T
    segs = [T] if m == 0 else [m] * ((T - 1) // m) + [T - m * ((T - 1) // m)]
    for k in range(K):
        w = W64[k]
        u = 1.0 - w.sum()
        e1 = e2 = 1.0
        for ln in segs:
            a = w @ (1 + m64) ** ln
            e1 *= u + a
            e2 *= u * u + 2 * u * a + w @ (M ** ln) @ w
        v = term[k].astype(np.float64)
        sd = np.sqrt(e2 - e1 * e1)
        mean, s = v.mean(), v.std(ddof=1)
        assert abs(mean - e1) <= 5 * s / np.sqrt(n), (m, k, mean, e1)
        m4 = np.mean((v - mean) ** 4)
        se_sd = np.sqrt(max(m4 - s ** 4, 0.0) / n) / (2 * s)
        assert abs(s - sd) <= 5 * se_sd, (m, k, s, sd, se_sd)


@pytest.mark.parametrize("source", ["gauss", "boot"])
def test_cost_lowers_every_path(source, gpu_ctx):
    N, K, T, n = 8, 3, 60, 50_000
    mu, L, W = _market(N, K, 2, scale=0.25)
    kw = dict(rows=_table(300, N, 2) * np.float32(0.5), block=2.0) if source == "boot" else dict(mu=mu, chol=L)
    prm = _ffi.make_params(N, T, K)
    for m in (1, 5):
        _, free = gpu_ctx.simulate_rebalanced(prm, m, 0.0, W, SEED, 5, n, True, **kw)[:4:3]
        _, paid = gpu_ctx.simulate_rebalanced(prm, m, 1e-3, W, SEED, 5, n, True, **kw)[:4:3]
        assert np.all(paid <= free) and np.all(paid.mean(axis=1) < free.mean(axis=1)), m
    _, free = gpu_ctx.simulate_rebalanced(prm, 0, 0.0, W, SEED, 5, n, True, **kw)[:4:3]
    _, paid = gpu_ctx.simulate_rebalanced(prm, 0, 1e-3, W, SEED, 5, n, True, **kw)[:4:3]
    assert np.array_equal(free.view(np.uint32), paid.view(np.uint32))


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_logical_shards_and_portfolio_shards_equal_one_shard(devices, gpu_ctx):
    N, K, T = 16, 20, 30
    mu, L, W = _market(N, K, 9)
    prm = _ffi.make_params(N, T, K)
    one = gpu_ctx.simulate_rebalanced(prm, 4, 1e-3, W, SEED, 11, 30_001, True, mu=mu, chol=L, horizons=[10, 30], levels=(50.0,))
    c = Context(devices)
    try:
        sh = c.simulate_rebalanced(prm, 4, 1e-3, W, SEED, 11, 30_001, True, mu=mu, chol=L, horizons=[10, 30], levels=(50.0,))
        sp = c.simulate_rebalanced(_ffi.make_params(N, T, K, shard_portfolios=True), 4, 1e-3, W, SEED, 11, 30_001, True, mu=mu,
                                   chol=L, horizons=[10, 30], levels=(50.0,))
        rows = _table(5000, N, 9)
        b1 = gpu_ctx.simulate_rebalanced(prm, 0, 0.0, W, SEED, 11, 30_001, True, rows=rows, block=4.0)
        bs = c.simulate_rebalanced(prm, 0, 0.0, W, SEED, 11, 30_001, True, rows=rows, block=4.0)
    finally:
        c.close()
    for other in (sh, sp):
        assert np.array_equal(one[3], other[3]) and np.array_equal(one[4], other[4]) and np.array_equal(one[2], other[2])
        for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi", "cvar"):
            assert np.array_equal(one[0][f], other[0][f]) and np.array_equal(one[1][f], other[1][f]), f
        assert np.allclose(one[0]["mean"], other[0]["mean"], rtol=1e-12) and np.allclose(one[0]["std"], other[0]["std"], rtol=1e-12)
    assert np.array_equal(b1[3], bs[3]) and np.array_equal(b1[0]["var"], bs[0]["var"])


def test_small_terminal_budget_tiles_the_portfolios(gpu_ctx):
    N, K, T = 4, 20, 12
    mu, L, W = _market(N, K, 2)
    prm = _ffi.make_params(N, T, K)
    want = gpu_ctx.simulate_rebalanced(prm, 3, 1e-3, W, SEED, 0, 10_000, True, mu=mu, chol=L, horizons=[4, 12], levels=(5.0, 95.0))
    c = Context(0, terminal_budget=3 * 3 * 10_000 * 4)
    try:
        got = c.simulate_rebalanced(prm, 3, 1e-3, W, SEED, 0, 10_000, True, mu=mu, chol=L, horizons=[4, 12], levels=(5.0, 95.0))
    finally:
        c.close()
    assert np.array_equal(want[3], got[3]) and np.array_equal(want[4], got[4]) and np.array_equal(want[2], got[2])
    for f in ("var", "n_tail", "min", "max"):
        assert np.array_equal(want[0][f], got[0][f]) and np.array_equal(want[1][f], got[1][f])


def test_rejected_call_then_a_correct_one_then_a_plain_call(gpu_ctx):
    mu, L, W = _market(16, 3, 1)
    prm = _ffi.make_params(16, 40, 3)
    g0, gt0 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    with pytest.raises(_ffi.McpError):
        gpu_ctx.simulate_rebalanced(prm, -1, 0.0, W, SEED, 0, 1000, False, mu=mu, chol=L)
    with pytest.raises(_ffi.McpError):
        gpu_ctx.simulate_rebalanced(_ffi.make_params(16, 40, 3, compounding="log"), 3, 0.0, W, SEED, 0, 1000, False, mu=mu, chol=L)
    st, _, _, term, _ = gpu_ctx.simulate_rebalanced(prm, 3, 1e-3, W, SEED, 0, 50_000, True, mu=mu, chol=L)
    ids = np.arange(0, 50_000, 2499)
    ref = rebalanced(gauss_returns(mu, L, 40, SEED, ids.astype(np.uint64)), W, 3, 1e-3)
    assert np.array_equal(term[:, ids], ref["V_T"])
    x = x_of(term[1])
    assert st[1]["var"] == np.percentile(x, Q_ALPHA)
    g1, gt1 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    assert np.array_equal(gt0, gt1) and np.array_equal(g0, g1)


def test_simulate_paths_and_bootstrap_return_their_shapes(gpu_ctx):
    mu, cov = synthetic.synthetic_market(3)
    one = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, rebalance="never", store=True, horizons=[1, 6, 12],
                         bands=(5.0, 95.0), context=gpu_ctx)
    assert one["n"] == 5000 and one["terminal"].shape == (5000,) and one["horizons"]["bands"].shape == (3, 2)
    many = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, rebalance=3, rebalance_cost=1e-3, context=gpu_ctx)
    assert isinstance(many, list) and len(many) == 3
    arr = simulate_bootstrap(_table(50, 3), np.eye(3), n_steps=12, n_paths=5000, rebalance=2, as_array=True, context=gpu_ctx)
    assert arr.shape == (3,) and arr.dtype == _ffi.STATS_DTYPE


def test_pipeline_prints_the_allocation_lines(gpu_ctx):
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
    assert "max-Sharpe allocation bought and held" in text and "max-Sharpe allocation rebalanced every 3 periods at 10 bp" in text
    assert text.count("bootstrap fan after") == 3 and text.count("forecast fan after") == 3


def test_streamlit_portfolio_tab_shows_the_held_allocation(gpu_ctx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_shim import fake_streamlit
    record = []
    sys.modules["streamlit"] = fake_streamlit(record, 50_000)
    try:
        np.random.seed(4242)
        runpy.run_path(os.path.join(ROOT, "examples", "streamlit_app.py"), run_name="__main__")
    finally:
        del sys.modules["streamlit"]
    held = [r[1][0] for r in record if r[0] == "write" and isinstance(r[1][0], dict) and "allocation held" in r[1][0]]
    assert len(held) == 1
    got = held[0]["allocation held"]
    assert got["rebalancing"] == "never (buy and hold)" and got["cost (bp)"] == 10.0 and np.isfinite(got["var"])

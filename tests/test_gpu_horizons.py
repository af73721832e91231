"""Values at intermediate horizons on the GPU (SPEC.md 4.3 / 5.2): every horizon row bit-equal to mcp_simulate at n_steps = h,
the horizon records against that call's records, terminal output unchanged, bands bit-equal to np.percentile, the analytic
law in log mode, sharded and tiled calls, recovery after a rejected call, and the forecast tab of the example app."""
import os
import runpy
import sys

import numpy as np
import pytest

from horizons_ref import simulate_horizons, x_of
from monte_carlo_portfolio_amd import _ffi, simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("n", "n_tail", "var", "min", "max")
LEVELS = (0.0, 2.5, 50.0, 97.5, 100.0)


def _assert_bands(got, x, levels, mode):
    """SPEC.md 5.2: bit-equal to np.percentile on the stored values.  In log mode the device's expm1 and the host's may differ
    by one ulp (as for the terminal VaR, tests/test_gpu_parity.py), so there the bands agree to that rounding."""
    want = np.percentile(x, levels)
    if mode == "simple":
        assert np.array_equal(got, want), (got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-15, atol=1e-17)


def _inputs(n, k):
    mu, cov = synthetic.synthetic_market(n)
    return mu, cov, synthetic.dirichlet_weights(n, k)


CASES = [  # (N, K, T, horizons, mode): N in {1,3,16,17,64}, K in {1,3,8,9,20}, both modes, horizon lists with and without T
    (1, 1, 30, [1, 7, 30], "simple"), (3, 3, 25, [2, 3, 24], "log"), (16, 8, 40, [1, 10, 20, 39, 40], "simple"),
    (16, 1, 40, [13], "log"), (17, 9, 12, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], "simple"), (64, 20, 10, [5, 10], "log"),
    (64, 1, 16, [1, 16], "simple"), (3, 20, 21, [7, 14], "simple"), (16, 9, 33, [32], "log"),
]


@pytest.mark.parametrize("n,K,T,hz,mode", CASES)
def test_horizon_rows_equal_the_n_steps_h_calls(n, K, T, hz, mode, gpu_ctx, oracle):
    mu, cov, W = _inputs(n, K)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    n_paths, begin, seed, v0 = 3001, (1 << 32) - 1000, 0x5EED0002, 2.0
    prm = _ffi.make_params(n, T, K, mode, v0=v0)
    stats, hs, bands, term, hzt = gpu_ctx.simulate_horizons(prm, mu32, L, W32, seed, begin, n_paths, hz, LEVELS, True)
    assert hzt.shape == (len(hz), K, n_paths) and hs.shape == (len(hz), K) and bands.shape == (len(hz), K, len(LEVELS))
    plain, term0 = gpu_ctx.simulate(_ffi.make_params(n, T, K, mode, v0=v0), mu32, L, W32, seed, begin, n_paths, True)
    assert np.array_equal(term.view(np.uint32), term0.view(np.uint32))
    for f in ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max", "cvar", "sum_tail"):
        assert np.array_equal(stats[f], plain[f]), f
    for f in ("mean", "std", "sharpe"):
        np.testing.assert_allclose(stats[f], plain[f], rtol=1e-13, atol=1e-15)
    for i, h in enumerate(hz):
        ref, ref_term = gpu_ctx.simulate(_ffi.make_params(n, h, K, mode, v0=v0), mu32, L, W32, seed, begin, n_paths, True)
        assert np.array_equal(hzt[i].view(np.uint32), ref_term.view(np.uint32)), h
        for f in EXACT:
            assert np.array_equal(hs[i][f], ref[f]), (h, f)
        for f in ("mean", "std", "cvar"):
            np.testing.assert_allclose(hs[i][f], ref[f], rtol=1e-12, atol=1e-15, err_msg=f"{h} {f}")
        assert np.all(hs[i]["sharpe"] == 0.0)
        for k in range(K):
            _assert_bands(bands[i, k], x_of(hzt[i, k], mode, v0), LEVELS, mode)
    idx = np.unique(np.r_[0, 1, 255, 256, 999, 1000, 1001, n_paths - 1, np.arange(0, n_paths, 131)])
    ref = simulate_horizons(mu32, L, W32, T, seed, (begin + idx).astype(np.uint64), hz, mode, v0)
    assert np.array_equal(hzt[:, :, idx].view(np.uint32), ref["V_h"].view(np.uint32))
    c_ref = oracle.simulate(mu32, L, W32, hz[0], 64, seed, path_begin=begin + 960, compounding=mode, v0=v0)
    assert np.array_equal(hzt[0, :, 960:1024].view(np.uint32), c_ref.view(np.uint32))


@pytest.mark.parametrize("n_paths", [1, 2, 3, 1000])
def test_bands_tiny_samples(n_paths, gpu_ctx):
    mu, cov, W = _inputs(5, 3)
    d = simulate_paths(mu, cov, W, n_steps=12, n_paths=n_paths, seed=9, horizons=[1, 6, 12], bands=LEVELS, store=True,
                       context=gpu_ctx)
    for k in range(3):
        hzd = d[k]["horizons"]
        assert hzd["bands"].shape == (3, len(LEVELS)) and list(hzd["steps"]) == [1, 6, 12]
        for i in range(3):
            x = x_of(d[k]["horizon_terminal"][i])
            assert np.array_equal(hzd["bands"][i], np.percentile(x, LEVELS))
            assert hzd["min"][i] == x.min() and hzd["max"][i] == x.max()


@pytest.mark.parametrize("mode", ["simple", "log"])
def test_bands_at_configs1_shape(mode, gpu_ctx):
    """10^6 paths x 252 steps, 16 assets, one portfolio, 12 monthly horizons."""
    mu, cov, W = _inputs(16, 1)
    hz = list(range(21, 253, 21))
    levels = (2.5, 5.0, 50.0, 95.0, 97.5)
    d = simulate_paths(mu, cov, W[0], n_steps=252, n_paths=1_000_000, seed=synthetic.BENCH_SEED, compounding=mode, horizons=hz,
                       bands=levels, store=True, context=gpu_ctx)
    plain = simulate_paths(mu, cov, W[0], n_steps=252, n_paths=1_000_000, seed=synthetic.BENCH_SEED, compounding=mode, store=True,
                           context=gpu_ctx)
    assert np.array_equal(d["terminal"].view(np.uint32), plain["terminal"].view(np.uint32))
    assert all(d[f] == plain[f] for f in ("n", "n_tail", "var", "cvar", "mean", "std", "sharpe", "min", "max"))
    assert np.array_equal(d["horizon_terminal"][-1].view(np.uint32), plain["terminal"].view(np.uint32))
    for i in range(len(hz)):
        x = x_of(d["horizon_terminal"][i], mode)
        _assert_bands(d["horizons"]["bands"][i], x, levels, mode)
        _assert_bands(d["horizons"]["var"][i], x, (1 - 0.95) * 100, mode)
        if mode == "simple":
            assert d["horizons"]["n_tail"][i] == np.count_nonzero(x <= d["horizons"]["var"][i])


def test_log_bands_follow_the_analytic_law(gpu_ctx):
    """log mode: S_h ~ N(h w.mu, h w'Sigma w); the 50 % and 5 % bands lie within 5 standard errors."""
    from statistics import NormalDist
    norm = NormalDist()
    mu, cov, W = _inputs(16, 1)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    n = 1_000_000
    hz = [1, 21, 63, 126, 252]
    _, _, bands = simulate_paths(mu, cov, W[0], n_steps=252, n_paths=n, seed=31, compounding="log", horizons=hz, bands=(5.0, 50.0),
                                 as_array=True, context=gpu_ctx)
    w = W32[0].astype(np.float64)
    m = w @ mu32.astype(np.float64)
    L64 = L.astype(np.float64)
    s2 = w @ (L64 @ L64.T) @ w
    for i, h in enumerate(hz):
        sd = np.sqrt(h * s2)
        for j, p in enumerate((0.05, 0.5)):
            zp = norm.inv_cdf(p)
            se = np.sqrt(p * (1 - p) / n) / (norm.pdf(zp) / sd)
            got = np.log1p(bands[i, 0, j])
            assert abs(got - (h * m + zp * sd)) < 5 * se, (h, p, got, h * m + zp * sd, se)


def _same(a, b):
    for f in EXACT:
        assert np.array_equal(a[f], b[f]), f
    for f in ("mean", "std", "cvar"):
        np.testing.assert_allclose(a[f], b[f], rtol=0, atol=1e-15, err_msg=f)


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
@pytest.mark.parametrize("n_paths", [100_003, 2])
def test_logical_shards_and_portfolio_shards_equal_one_shard(devices, n_paths, gpu_ctx):
    mu, cov, W = _inputs(16, 3)
    kw = dict(n_steps=60, n_paths=n_paths, seed=11, as_array=True, horizons=[1, 20, 59], bands=(2.5, 50.0, 97.5))
    s1, h1, b1 = simulate_paths(mu, cov, W, context=gpu_ctx, **kw)
    ctx = Context(devices)
    try:
        sn, hn, bn = simulate_paths(mu, cov, W, context=ctx, **kw)
        assert ctx.exchange()[0] == "kernel"
        sp, hp, bp = simulate_paths(mu, cov, W, context=ctx, shard="portfolios", devices=devices, **kw)
    finally:
        ctx.close()
    _same(s1, sn)
    _same(h1, hn)
    _same(h1, hp)
    assert np.array_equal(b1, bn) and np.array_equal(b1, bp)


def test_small_terminal_budget_tiles_the_portfolios(gpu_ctx):
    mu, cov, W = _inputs(8, 5)
    n, hz = 20_000, [3, 10, 25]
    kw = dict(n_steps=50, n_paths=n, seed=12, store=True, as_array=True, horizons=hz, bands=(5.0, 95.0))
    s1, h1, b1, t1, z1 = simulate_paths(mu, cov, W, context=gpu_ctx, **kw)
    ctx = Context(0, terminal_budget=2 * 4 * (1 + len(hz)) * n)      # 4 (1 + H) B per path and portfolio: two per tile
    try:
        s2, h2, b2, t2, z2 = simulate_paths(mu, cov, W, context=ctx, **kw)
    finally:
        ctx.close()
    assert np.array_equal(t1, t2) and np.array_equal(z1, z2) and np.array_equal(b1, b2)
    _same(s1, s2)
    _same(h1, h2)


def test_rejected_call_then_a_correct_one(gpu_ctx):
    mu, cov, W = _inputs(4, 2)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    with pytest.raises(ValueError):
        simulate_paths(mu, cov, W, n_steps=20, n_paths=1000, horizons=[5, 30], context=gpu_ctx)
    with pytest.raises(_ffi.McpError, match="horizons"):
        gpu_ctx.simulate_horizons(_ffi.make_params(4, 20, 2, native_math=True), mu32, L, W32, 1, 0, 1000, [5, 10], (50.0,), False)
    with pytest.raises(_ffi.McpError, match="horizon"):
        gpu_ctx.simulate_horizons(_ffi.make_params(4, 20, 2), mu32, L, W32, 1, 0, 1000, [10, 5], (50.0,), False)
    stats, hs, bands, term, hzt = gpu_ctx.simulate_horizons(_ffi.make_params(4, 20, 2), mu32, L, W32, 1, 0, 1000, [5, 20], (50.0,),
                                                            True)
    for i, h in enumerate((5, 20)):
        ref, ref_term = gpu_ctx.simulate(_ffi.make_params(4, h, 2), mu32, L, W32, 1, 0, 1000, True)
        assert np.array_equal(hzt[i], ref_term) and np.array_equal(hs[i]["var"], ref["var"])
        for k in range(2):
            assert bands[i, k, 0] == np.percentile(x_of(hzt[i, k]), 50.0)


def test_forecast_tab_shows_the_simulated_fan(gpu_ctx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_shim import fake_streamlit
    import monte_carlo_portfolio_amd as mcp
    record = []
    n_paths = 100_000
    sys.modules["streamlit"] = fake_streamlit(record, n_paths)
    try:
        np.random.seed(4242)
        runpy.run_path(os.path.join(ROOT, "examples", "streamlit_app.py"), run_name="__main__")
    finally:
        del sys.modules["streamlit"]
    kinds = [r[0] for r in record]
    assert kinds.count("dataframe") == 1 and kinds.count("scatter_chart") == 5 and "error" not in kinds
    fans = [r[1][0] for r in record if r[0] == "write" and isinstance(r[1][0], dict) and "horizon" in r[1][0]]
    charts = [r[1][0] for r in record if r[0] == "line_chart" and isinstance(r[1][0], dict) and "horizon" in r[1][0]]
    assert len(fans) == 4 and len(charts) == 4                       # three assets and the Monte Carlo optimum
    # the same flow by hand
    files = []
    import io
    from test_gpu_shim import DATA, FILES
    for f in FILES:
        b = io.BytesIO(open(os.path.join(DATA, f), "rb").read())
        b.name = f
        files.append(b)
    names, prices, res = mcp.load_prices(files, resample_rule="M")
    rets = mcp.returns_matrix(res)
    np.random.seed(4242)
    want = mcp.run_all_methods(rets, min_weights=np.zeros(3), max_weights=np.ones(3), user_rf=3.0, annual_factor=12,
                               investment_amount=10000.0)
    mu_step, cov_step = rets.mean().values, rets.cov().values
    levels = (2.5, 50.0, 97.5)
    _, _, bands = mcp.simulate_paths(mu_step, cov_step, np.eye(3), n_steps=6, n_paths=n_paths, seed=12345, horizons=[1, 3, 6],
                                     bands=levels, as_array=True)
    opt = mcp.simulate_paths(mu_step, cov_step, want["Monte Carlo"]["weights"], n_steps=6, n_paths=n_paths, seed=12345,
                             v0=10000.0, horizons=[1, 3, 6], bands=levels)
    for a, name in enumerate(names):
        fan = next(f for f in fans if f["asset"] == name)
        last = float(res[name].iloc[-1])
        for j, q in enumerate(levels):
            assert fan[f"{q} %"] == (last * (1.0 + bands[:, a, j])).tolist()
    fan = next(f for f in fans if f["asset"] == "Monte Carlo optimum")
    for j, q in enumerate(levels):
        assert fan[f"{q} %"] == (10000.0 * (1.0 + opt["horizons"]["bands"][:, j])).tolist()

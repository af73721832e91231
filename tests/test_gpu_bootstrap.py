"""GPU checks of the stationary block bootstrap (SPEC.md 2.1 / 4.4 / 5.3): terminal and horizon values bit-equal to the NumPy
restatement (bootstrap_ref.py) over widths, portfolio counts, step counts, block lengths, both compounding modes and both row
table placements (LDS and global memory); the records against NumPy on the stored values; the shards, the tiles, recovery after
a rejected call; the reference-made collar matrix; and the examples' bootstrap lines."""
import contextlib
import io
import math
import os
import runpy
import sys

import numpy as np
import pytest

from bootstrap_ref import boot_indices, row_returns, simulate_boot
from horizons_ref import x_of
from oracle.np_oracle import _fma32
from monte_carlo_portfolio_amd import _ffi, simulate_bootstrap, simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_script_arrays.npz")
SEED = 0xB007_5EED


def _table(R, N, seed=0):
    rng = np.random.default_rng(seed + 1000 * N + R)
    return (rng.standard_t(3, size=(R, N)) * 0.02 + 0.001).astype(np.float32)


def _weights(N, K, seed=0):
    return np.random.default_rng(seed + N * 31 + K).dirichlet(np.ones(N), size=K).astype(np.float32)


Q_ALPHA = (1 - 0.95) * 100          # the reference's percentile level of VaR at alpha = 0.95 (app.py:259): 5.000000000000004


def _same(a, b, mode):
    """bit-equal in simple compounding; in log compounding x = expm1(S), and the device's expm1 and the host's may differ by
    one ulp (SPEC.md 5)"""
    return a == b if mode == "simple" else abs(a - b) <= 2.3e-16 * abs(b)


def _pick(n_paths, begin):
    """path ids (relative) to compare: both ends, a spread, and, when the range crosses 2^32, both sides of it"""
    ids = {0, 1, n_paths - 1, n_paths // 2}
    ids.update(np.linspace(0, n_paths - 1, 24).astype(int).tolist())
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 3)))
    return np.array(sorted(ids), np.int64)


CASES = [  # N, K, T, block, compounding, R        (LDS holds the table when R * ceil(N/4) <= 1088)
    (1, 1, 7, 1.0, "simple", 50),
    (3, 3, 252, 2.5, "log", 40),
    (4, 8, 1, 12.0, "simple", 300),
    (5, 9, 7, math.inf, "log", 17),
    (16, 1, 252, 1.0, "simple", 272),              # just inside the LDS slot
    (16, 1, 252, 2.5, "log", 273),                 # just outside: global memory
    (16, 20, 7, 12.0, "simple", 272),
    (16, 3, 7, 2.5, "log", 100_000),               # global
    (17, 3, 0, 1.0, "simple", 10),
    (33, 1, 7, math.inf, "simple", 100_000),
    (64, 9, 1, 2.5, "log", 5),
    (64, 1, 7, 1.0, "simple", 68),                 # N = 64: 68 rows fill the slot
    (64, 3, 7, math.inf, "log", 69),
]


@pytest.mark.parametrize("N,K,T,b,mode,R", CASES)
def test_terminal_values_equal_the_restatement(N, K, T, b, mode, R, gpu_ctx):
    rows, W = _table(R, N), _weights(N, K)
    begin, n = (1 << 32) - 700, 1337
    prm = _ffi.make_params(N, T, K, compounding=mode, v0=2.0)
    stats, term = gpu_ctx.simulate_bootstrap(prm, rows, W, b, SEED, begin, n, True)
    ids = _pick(n, begin)
    ref = simulate_boot(rows, W, T, SEED, (begin + ids).astype(np.uint64), b, mode, v0=2.0)
    assert np.array_equal(term[:, ids].view(np.uint32), ref["V_T"].view(np.uint32))
    for k in range(K):                                               # the records against NumPy on the stored values
        x = x_of(term[k], mode, 2.0)
        st = stats[k]
        assert st["n"] == n and _same(st["var"], np.percentile(x, Q_ALPHA), mode)
        assert _same(st["min"], x.min(), mode) and _same(st["max"], x.max(), mode)
        if mode == "simple":
            assert st["n_tail"] == int(np.sum(x <= st["var"]))
        assert abs(st["mean"] - x.mean()) <= 1e-12 * max(1.0, abs(x.mean()))
        assert abs(st["std"] - x.std(ddof=1)) <= 1e-12 * max(1e-3, x.std(ddof=1))


@pytest.mark.parametrize("mode", ["simple", "log"])
@pytest.mark.parametrize("R,b", [(40, 2.5), (272, 1.0), (5000, 12.0)])
def test_horizon_rows_equal_the_n_steps_h_calls_and_the_bands_np_percentile(mode, R, b, gpu_ctx):
    N, K, T = 16, 3, 24
    rows, W = _table(R, N, 7), _weights(N, K, 7)
    hz, levels = [1, 5, 12, 24], (2.5, 50.0, 97.5)
    n = 20_011
    prm = _ffi.make_params(N, T, K, compounding=mode)
    stats, hs, bands, term, hzt = gpu_ctx.simulate_bootstrap_horizons(prm, rows, W, b, SEED, 3, n, hz, levels, True)
    ids = _pick(n, 3)
    ref = simulate_boot(rows, W, T, SEED, (3 + ids).astype(np.uint64), b, mode, horizons=hz)
    assert np.array_equal(hzt[:, :, ids].view(np.uint32), ref["V_h"].view(np.uint32))
    assert np.array_equal(hzt[-1], term)
    for i, h in enumerate(hz):
        st_h, term_h = gpu_ctx.simulate_bootstrap(_ffi.make_params(N, h, K, compounding=mode), rows, W, b, SEED, 3, n, True)
        assert np.array_equal(hzt[i].view(np.uint32), term_h.view(np.uint32)), h
        for k in range(K):
            x = x_of(hzt[i, k], mode)
            assert hs[i, k]["var"] == st_h[k]["var"] and _same(hs[i, k]["var"], np.percentile(x, Q_ALPHA), mode)
            assert hs[i, k]["n_tail"] == st_h[k]["n_tail"] and _same(hs[i, k]["min"], x.min(), mode)
            for j, q in enumerate(levels):
                assert _same(bands[i, k, j], np.percentile(x, q), mode), (h, k, q)


ONE_PORTFOLIO = [  # call, compounding, R: the one-portfolio (K = 1) kernels that no case above launches
    ("terminal", "log", 7),
    ("horizons", "simple", 7), ("horizons", "log", 7),
    ("horizons", "simple", 1088 // 2 + 1), ("horizons", "log", 1088 // 2 + 1),
]


@pytest.mark.parametrize("call,mode,R", ONE_PORTFOLIO)
def test_one_portfolio_kernels_equal_the_restatement_on_every_path(call, mode, R, gpu_ctx):
    """N = 5 is two asset blocks with three padding assets, 300 paths are two workgroups with the second one ragged; at two
    asset blocks 7 rows sit in LDS and 545 are one more than it holds."""
    N, T, n, begin, b = 5, 6, 300, 3, 2.5
    rows, W = _table(R, N, 11), _weights(N, 1, 11)
    prm = _ffi.make_params(N, T, 1, compounding=mode, v0=2.0)
    paths = (begin + np.arange(n)).astype(np.uint64)
    if call == "terminal":
        _, term = gpu_ctx.simulate_bootstrap(prm, rows, W, b, SEED, begin, n, True)
        ref = simulate_boot(rows, W, T, SEED, paths, b, mode, v0=2.0)
    else:
        hz = [1, 4, 6]
        _, _, _, term, hzt = gpu_ctx.simulate_bootstrap_horizons(prm, rows, W, b, SEED, begin, n, hz, (50.0,), True)
        ref = simulate_boot(rows, W, T, SEED, paths, b, mode, v0=2.0, horizons=hz)
        assert np.array_equal(hzt.view(np.uint32), ref["V_h"].view(np.uint32))
    assert np.array_equal(term.view(np.uint32), ref["V_T"].view(np.uint32))


@pytest.mark.parametrize("mode", ["simple", "log"])
@pytest.mark.parametrize("N,R", [(16, 250), (16, 300), (5, 64)])
def test_b_inf_with_T_equal_R_visits_every_row_once(mode, N, R, gpu_ctx):
    rows, W = _table(R, N, 3), _weights(N, 2, 3)
    n = 3000
    _, term = gpu_ctx.simulate_bootstrap(_ffi.make_params(N, R, 2, compounding=mode), rows, W, math.inf, SEED, 0, n, True)
    ids = _pick(n, 0)
    idx = boot_indices(SEED, ids.astype(np.uint64), R, R, math.inf)
    rr = row_returns(rows, W)
    for c, p in enumerate(ids):
        start = idx[0, c]
        assert sorted(idx[:, c]) == list(range(R))
        for k in range(2):
            v = np.float32(0.0) if mode == "log" else np.float32(1.0)
            for t in range(R):                                         # the rotated sum / product of the row returns
                r = rr[k, (start + t) % R]
                v = np.float32(v + r) if mode == "log" else _fma32(np.array([v]), np.array([r]), np.array([v]))[0]
            assert term[k, p] == v, (p, k)


def test_collar_bootstrap_never_goes_below_the_worst_historical_row(gpu_ctx):
    """The reference-made collar returns: a one-step bootstrap stays inside the observed portfolio rows (the hedge's floor);
    the normal model on the same matrix's mean / cov does not."""
    ret = np.load(GOLDEN)["monthly_collar_seed12345__returns_df"].astype(np.float64)
    w = np.array([0.5, 0.3, 0.2])
    worst = float(np.float32(1.0) + row_returns(ret.astype(np.float32), w.astype(np.float32))[0].min()) - 1.0
    boot = simulate_bootstrap(ret, w, n_steps=1, n_paths=200_000, block=1.0, seed=5, store=True, context=gpu_ctx)
    gauss = simulate_paths(ret.mean(axis=0), np.cov(ret.T), w, n_steps=1, n_paths=200_000, seed=5, context=gpu_ctx)
    assert boot["min"] == worst and boot["var"] >= worst
    assert gauss["min"] < worst
    assert boot["min"] >= (ret @ w).min() - 1e-6


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_logical_shards_and_portfolio_shards_equal_one_shard(devices, gpu_ctx):
    N, K, T = 16, 20, 30
    rows, W = _table(5000, N, 9), _weights(N, K, 9)
    prm = _ffi.make_params(N, T, K)
    one, t1 = gpu_ctx.simulate_bootstrap(prm, rows, W, 4.0, SEED, 11, 30_001, True)
    c = Context(devices)
    try:
        sh, ts = c.simulate_bootstrap(prm, rows, W, 4.0, SEED, 11, 30_001, True)
        prm_p = _ffi.make_params(N, T, K, shard_portfolios=True)
        sp, tp = c.simulate_bootstrap(prm_p, rows, W, 4.0, SEED, 11, 30_001, True)
        hz = c.simulate_bootstrap_horizons(prm, rows, W, 4.0, SEED, 11, 30_001, [10, 30], (50.0,), True)
    finally:
        c.close()
    assert np.array_equal(t1, ts) and np.array_equal(t1, tp) and np.array_equal(t1, hz[3])
    for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi", "cvar"):
        assert np.array_equal(one[f], sh[f]) and np.array_equal(one[f], sp[f]), f
    assert np.allclose(one["mean"], sh["mean"], rtol=1e-12) and np.allclose(one["std"], sp["std"], rtol=1e-12)


def test_small_terminal_budget_tiles_the_portfolios(gpu_ctx):
    N, K, T = 4, 20, 12
    rows, W = _table(2000, N, 2), _weights(N, K, 2)
    prm = _ffi.make_params(N, T, K, compounding="log")
    want, tw = gpu_ctx.simulate_bootstrap(prm, rows, W, 2.5, SEED, 0, 10_000, True)
    c = Context(0, terminal_budget=3 * 10_000 * 4)
    try:
        got, tg = c.simulate_bootstrap(prm, rows, W, 2.5, SEED, 0, 10_000, True)
        ghz = c.simulate_bootstrap_horizons(prm, rows, W, 2.5, SEED, 0, 10_000, [4, 12], (5.0, 95.0), True)
    finally:
        c.close()
    assert np.array_equal(tw, tg) and np.array_equal(tw, ghz[3])
    for f in ("var", "n_tail", "min", "max"):
        assert np.array_equal(want[f], got[f]) and np.array_equal(want[f], ghz[0][f])


def test_rejected_call_then_a_correct_one_and_the_gaussian_buffers_are_left_intact(gpu_ctx):
    mu, cov = synthetic.synthetic_market(16)
    mu32, L, W32 = prepare_inputs(mu, cov, synthetic.dirichlet_weights(16, 3))
    prm = _ffi.make_params(16, 40, 3)
    g0, gt0 = gpu_ctx.simulate(prm, mu32, L, W32, 77, 0, 50_000, True)
    rows = _table(100, 16)
    bad = rows.copy()
    bad[50, 3] = np.nan
    with pytest.raises(_ffi.McpError):
        gpu_ctx.simulate_bootstrap(prm, bad, W32, 2.0, SEED, 0, 1000, False)
    with pytest.raises(_ffi.McpError):
        gpu_ctx.simulate_bootstrap(_ffi.make_params(16, 40, 3, native_math=True), rows, W32, 2.0, SEED, 0, 1000, False)
    b1, bt1 = gpu_ctx.simulate_bootstrap(prm, rows, W32, 2.0, SEED, 0, 50_000, True)
    ref = simulate_boot(rows, W32, 40, SEED, np.arange(0, 50_000, 997, dtype=np.uint64), 2.0)
    assert np.array_equal(bt1[:, ::997], ref["V_T"])
    g1, gt1 = gpu_ctx.simulate(prm, mu32, L, W32, 77, 0, 50_000, True)
    assert np.array_equal(gt0, gt1) and np.array_equal(g0, g1)


def test_simulate_bootstrap_returns_simulate_paths_shapes(gpu_ctx):
    pd = pytest.importorskip("pandas")
    ret = pd.DataFrame(_table(120, 3, 5).astype(np.float64), columns=["a", "b", "c"])
    one = simulate_bootstrap(ret, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, block=3.0, store=True, horizons=[1, 6, 12],
                             bands=(5.0, 95.0), context=gpu_ctx)
    assert one["n"] == 5000 and one["terminal"].shape == (5000,) and one["horizons"]["bands"].shape == (3, 2)
    assert one["horizon_terminal"].shape == (3, 5000)
    many = simulate_bootstrap(ret.values, np.eye(3), n_steps=12, n_paths=5000, block=3.0, context=gpu_ctx)
    assert isinstance(many, list) and len(many) == 3
    arr = simulate_bootstrap(ret.values, np.eye(3), n_steps=12, n_paths=5000, as_array=True, context=gpu_ctx)
    assert arr.shape == (3,) and arr.dtype == _ffi.STATS_DTYPE


def test_pipeline_prints_the_bootstrap_lines(gpu_ctx):
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
    assert "bootstrap (mean block 3)" in text and "VaR95" in text
    assert text.count("bootstrap fan after") == 3 and text.count("forecast fan after") == 3


def test_streamlit_portfolio_tab_shows_both_records(gpu_ctx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_shim import DATA, FILES, fake_streamlit
    import monte_carlo_portfolio_amd as mcp
    record = []
    n_paths = 100_000
    sys.modules["streamlit"] = fake_streamlit(record, n_paths)
    try:
        np.random.seed(4242)
        runpy.run_path(os.path.join(ROOT, "examples", "streamlit_app.py"), run_name="__main__")
    finally:
        del sys.modules["streamlit"]
    side = [r[1][0] for r in record if r[0] == "write" and isinstance(r[1][0], dict) and "bootstrap of the observed rows" in r[1][0]]
    assert len(side) == 1
    files = []
    for f in FILES:
        b = io.BytesIO(open(os.path.join(DATA, f), "rb").read())
        b.name = f
        files.append(b)
    names, prices, res = mcp.load_prices(files, resample_rule="M")
    rets = mcp.returns_matrix(res)
    np.random.seed(4242)
    want = mcp.run_all_methods(rets, min_weights=np.zeros(3), max_weights=np.ones(3), user_rf=3.0, annual_factor=12,
                               investment_amount=10000.0)
    boot = mcp.simulate_bootstrap(rets, want["Monte Carlo"]["weights"], n_steps=12, n_paths=n_paths, block=3.0, seed=12345,
                                  v0=10000.0, rf=0.03)
    got = side[0]["bootstrap of the observed rows"]
    assert got["var"] == boot["var"] and got["cvar"] == boot["cvar"] and got["sharpe"] == boot["sharpe"]
    assert side[0]["normal model (mean / cov)"]["var"] != got["var"]

"""Max drawdown of simulated paths on the GPU (SPEC.md 4.2 / 5.1): per-path q / d bit-equal to the NumPy restatement,
terminal values and statistics unchanged, DaR / CDaR against NumPy on the stored sample, sharded and tiled calls."""
import numpy as np
import pytest

from drawdown_ref import mdd_of, simulate_paths_dd
from monte_carlo_portfolio_amd import _ffi, metrics, simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs

pytestmark = pytest.mark.gpu

EXACT = ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max")


def _inputs(n, k, scale=1.0):
    mu, cov = synthetic.synthetic_market(n)
    return mu, np.asarray(cov) * scale, synthetic.dirichlet_weights(n, k)


def _sample(n_paths, rng, count=512):
    head, tail = np.arange(min(64, n_paths)), np.arange(max(0, n_paths - 64), n_paths)
    ragged = np.arange((n_paths // 256) * 256, n_paths)
    rest = rng.choice(n_paths, size=min(n_paths, count), replace=False)
    return np.unique(np.concatenate([head, tail, ragged, rest]))[:count + 200]


CASES = [  # (N, T, K, compounding): every N of {1,3,4,5,16,17,33,64}, T of {0,1,2,252}, K of {1,3,8,9,20}, both modes
    (1, 252, 1, "simple"), (3, 252, 3, "log"), (4, 2, 8, "simple"), (5, 252, 9, "log"), (16, 252, 1, "simple"),
    (16, 252, 1, "log"), (16, 252, 8, "log"), (17, 1, 20, "simple"), (33, 0, 3, "log"), (64, 252, 1, "simple"),
    (64, 2, 20, "log"), (3, 1, 9, "simple"), (5, 0, 1, "simple"), (4, 252, 20, "simple"), (1, 2, 9, "log"),
]


@pytest.mark.parametrize("n,T,K,mode", CASES)
def test_per_path_state_bit_equal_to_the_spec(n, T, K, mode, gpu_ctx):
    mu, cov, W = _inputs(n, K)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    n_paths, begin, seed = 3000, (1 << 32) - 1500, 0x5EED0001
    prm = _ffi.make_params(n, T, K, mode)
    stats, dd, term, qd = gpu_ctx.simulate_drawdown(prm, mu32, L, W32, seed, begin, n_paths, True)
    idx = _sample(n_paths, np.random.default_rng(n * 1000 + T + K), 256 if n >= 33 else 512)
    ref = simulate_paths_dd(mu32, L, W32, T, seed, (begin + idx).astype(np.uint64), mode)
    assert np.array_equal(term[:, idx].view(np.uint32), ref["V_T"].view(np.uint32))
    bad = np.argwhere(qd[:, idx].view(np.uint32) != ref["q"].view(np.uint32))
    assert bad.size == 0, f"{len(bad)} q/d differ, first (k, path) {bad[0][0]}, {idx[bad[0][1]]}: {qd[bad[0][0], idx[bad[0][1]]]!r} vs {ref['q'][bad[0][0], bad[0][1]]!r}"
    if T <= 1:
        assert np.all(mdd_of(qd, mode) == 0.0) and np.all(dd["var"] == 0.0) and np.all(dd["n_tail"] == n_paths)


@pytest.mark.parametrize("K", [1, 8, 20])
@pytest.mark.parametrize("mode", ["simple", "log"])
def test_terminal_values_and_stats_unchanged(K, mode, gpu_ctx):
    mu, cov, W = _inputs(16, K)
    kw = dict(n_steps=64, n_paths=50_003, seed=77, compounding=mode, store=True, as_array=True, context=gpu_ctx)
    plain, term0 = simulate_paths(mu, cov, W, **kw)
    stats, dd, term, mdd = simulate_paths(mu, cov, W, drawdown=True, **kw)
    assert np.array_equal(term.view(np.uint32), term0.view(np.uint32))
    if K <= 16:                      # the same kernel epilogue: every field bit for bit
        assert plain.tobytes() == stats.tobytes()
    else:                            # plain K >= 17 runs the MFMA sweep kernels: moments agree to fp64 association
        for f in EXACT + ("cvar", "sum_tail"):
            assert np.array_equal(plain[f], stats[f]), f
        for f in ("mean", "std", "sharpe"):
            np.testing.assert_allclose(stats[f], plain[f], rtol=1e-13, atol=1e-15)
    assert mdd.shape == term.shape and dd.shape == (K,) and np.all(dd["sharpe"] == 0.0)


def _check_against_numpy(dd, mdd, alpha):
    mdd = np.asarray(mdd, np.float64)
    dar = metrics.var(mdd, alpha)
    assert dd["var"] == dar, (dd["var"], dar)
    assert int(dd["n_tail"]) == int(np.count_nonzero(mdd <= dar))
    assert dd["min"] == mdd.min() and dd["max"] == mdd.max() and int(dd["n"]) == mdd.size
    scale = max(1.0, float(np.abs(mdd).max()))
    assert abs(dd["cvar"] - metrics.cvar(mdd, alpha)) <= 1e-12 * scale
    assert abs(dd["mean"] - mdd.mean()) <= 1e-12 * scale
    assert abs(dd["std"] - mdd.std(ddof=1)) <= 1e-12 * scale


@pytest.mark.parametrize("alpha,mode", [(0.9, "simple"), (0.95, "simple"), (0.99, "simple"), (0.95, "log")])
def test_dar_cdar_at_configs1_shape(alpha, mode, gpu_ctx):
    """10^6 paths x 252 steps, 16 assets, one portfolio (BASELINE configs[1]'s shape)."""
    mu, cov, W = _inputs(16, 1)
    d = simulate_paths(mu, cov, W[0], n_steps=252, n_paths=1_000_000, seed=synthetic.BENCH_SEED, alpha=alpha, compounding=mode,
                       store=True, drawdown=True, context=gpu_ctx)
    mdd = d["max_drawdown"]
    assert mdd.dtype == np.float64 and mdd.shape == (1_000_000,) and mdd.max() <= 0.0
    rec = np.zeros(1, _ffi.STATS_DTYPE)
    for key, f in (("mean", "mean"), ("std", "std"), ("dar", "var"), ("cdar", "cvar"), ("n_tail", "n_tail"), ("worst", "min"),
                   ("best", "max")):
        rec[f] = d["drawdown"][key]
    rec["n"] = mdd.size
    _check_against_numpy(rec[0], mdd, alpha)
    assert set(d["drawdown"]) == {"mean", "std", "dar", "cdar", "n_tail", "worst", "best", "x_lo", "x_hi"}


def test_all_ties_zero_volatility(gpu_ctx):
    mu = np.array([-0.002, 0.001, 0.0005])
    W = np.array([0.5, 0.3, 0.2])
    stats, dd, term, mdd = simulate_paths(mu, None, W, chol=np.zeros((3, 3)), n_steps=40, n_paths=200_001, seed=3, store=True,
                                          as_array=True, drawdown=True, context=gpu_ctx)
    assert np.all(mdd == mdd[0, 0]) and mdd[0, 0] < 0.0
    _check_against_numpy(dd[0], mdd[0], 0.95)


def test_all_zeros_one_step(gpu_ctx):
    mu, cov, W = _inputs(5, 3)
    stats, dd, term, mdd = simulate_paths(mu, cov, W, n_steps=1, n_paths=100_000, seed=4, store=True, as_array=True, drawdown=True,
                                          context=gpu_ctx)
    assert np.all(mdd == 0.0)
    for k in range(3):
        _check_against_numpy(dd[k], mdd[k], 0.95)


@pytest.mark.parametrize("mode", ["simple", "log"])
def test_huge_volatility(mode, gpu_ctx):
    mu, cov, W = _inputs(4, 2, scale=400.0)
    stats, dd, term, mdd = simulate_paths(mu, cov, W, n_steps=64, n_paths=300_000, seed=5, compounding=mode, store=True,
                                          as_array=True, drawdown=True, context=gpu_ctx)
    assert np.all(np.isfinite(mdd))
    if mode == "simple":
        assert mdd.min() < -1.0          # some paths cross zero
    for k in range(2):
        _check_against_numpy(dd[k], mdd[k], 0.95)


def _same(a, b, moments_tol=1e-15):
    for f in EXACT:
        assert np.array_equal(a[f], b[f]), f
    for f in ("mean", "std", "cvar"):
        np.testing.assert_allclose(a[f], b[f], rtol=0, atol=moments_tol, err_msg=f)


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
@pytest.mark.parametrize("n_paths", [100_003, 2])
def test_logical_shards_equal_one_shard(devices, n_paths, gpu_ctx):
    mu, cov, W = _inputs(16, 3)
    kw = dict(n_steps=100, n_paths=n_paths, seed=11, as_array=True, drawdown=True)
    s1, d1 = simulate_paths(mu, cov, W, context=gpu_ctx, **kw)
    ctx = Context(devices)
    try:
        sn, dn = simulate_paths(mu, cov, W, context=ctx, **kw)
        assert ctx.exchange()[0] == "kernel"
        sp, dp = simulate_paths(mu, cov, W, context=ctx, shard="portfolios", devices=devices, **kw)
    finally:
        ctx.close()
    _same(d1, dn)
    _same(s1, sn)
    _same(d1, dp)


def test_small_terminal_budget_tiles_the_portfolios(gpu_ctx):
    mu, cov, W = _inputs(8, 5)
    n = 20_000
    kw = dict(n_steps=50, n_paths=n, seed=12, store=True, as_array=True, drawdown=True)
    s1, d1, t1, m1 = simulate_paths(mu, cov, W, context=gpu_ctx, **kw)
    ctx = Context(0, terminal_budget=2 * 8 * n)        # 8 B per path and portfolio: two portfolios per tile
    try:
        s2, d2, t2, m2 = simulate_paths(mu, cov, W, context=ctx, **kw)
    finally:
        ctx.close()
    assert np.array_equal(t1, t2) and np.array_equal(m1, m2)
    _same(d1, d2)
    _same(s1, s2)


def test_rejected_call_then_a_correct_one(gpu_ctx):
    mu, cov, W = _inputs(4, 1)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    with pytest.raises(ValueError):
        simulate_paths(mu, cov, W[0], n_paths=1000, fold=True, drawdown=True, context=gpu_ctx)
    with pytest.raises(_ffi.McpError, match="drawdown"):
        gpu_ctx.simulate_drawdown(_ffi.make_params(4, 20, 1, fold=True), mu32, L, W32, 1, 0, 1000, False)
    stats, dd, term, qd = gpu_ctx.simulate_drawdown(_ffi.make_params(4, 20, 1), mu32, L, W32, 1, 0, 1000, True)
    _check_against_numpy(dd[0], mdd_of(qd[0]), 0.95)
    ref = simulate_paths_dd(mu32, L, W32, 20, 1, np.arange(0, 1000, 97, dtype=np.uint64))
    assert np.array_equal(qd[:, ::97].view(np.uint32), ref["q"].view(np.uint32))

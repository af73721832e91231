"""GPU checks of the two-regime Markov switching (SPEC.md 2.6 / 4.13 / 5.13): terminal, drawdown and horizon values bit-equal to the
NumPy restatement (regime_ref.py) over widths, portfolio counts, step counts and a path range across 2^32; the anchors against the
Gaussian calls; the records and bands against NumPy on the stored values; the chain read off exactly; the laws at 10^6 paths; the
shards, the tiles, split calls, recovery after a rejected call; and the example's lines."""
import contextlib
import ctypes
import io
import os
import runpy
import sys

import numpy as np
import pytest

import regime_ref as rr
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, metrics, regime_law, simulate_paths, simulate_sweep, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs
from oracle import ref_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5E_61BE
PROBS = (0.2, 0.3, 0.5)


def _market(N, K, seed=0):
    """(mu, L, mu1, L1, W): the synthetic market and a crisis twin of it -- every mean 1 % lower, every volatility doubled, every
    correlation moved halfway to 1."""
    mu, cov = (np.asarray(a, np.float64) for a in synthetic.synthetic_market(N))
    W = np.random.default_rng(seed + 31 * N + K).dirichlet(np.ones(N), size=K)
    if K > 1:
        W[-1] *= 0.9                                     # 10 % cash in one portfolio
    sd = np.sqrt(np.diag(cov))
    corr = cov / np.outer(sd, sd)
    cov1 = (0.5 * corr + 0.5) * np.outer(2.0 * sd, 2.0 * sd)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    mu1, L1, _ = prepare_inputs(mu - 0.01, cov1, W)
    return mu32, L, mu1, L1, W32


def _pick(n_paths, begin, count=12):
    ids = {0, 1, n_paths - 1, n_paths // 2}
    ids.update(np.linspace(0, n_paths - 1, count).astype(int).tolist())
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 3)))
    return np.array(sorted(ids), np.int64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(ctx, prm, probs, mu, L, mu1, L1, W, begin, n, store=True, **kw):
    return ctx.simulate_regimes(prm, (*probs, mu1, L1), mu, L, W, SEED, begin, n, store, **kw)


def _gauss(ctx, prm, mu, L, W, begin, n):
    """(stats, terminal) of the Gaussian call on the path kernels: mcp_simulate, or for K >= 17 -- where mcp_simulate runs the MFMA
    sweep kernels, whose moment partials are laid out differently -- the terminal block of mcp_simulate_drawdown."""
    if prm.n_portfolios <= 16:
        return ctx.simulate(prm, mu, L, W, SEED, begin, n, True)
    st, _, term, _ = ctx.simulate_drawdown(prm, mu, L, W, SEED, begin, n, True)
    return st, term


def _covers_both(ref, T):
    """So that parity cannot pass in one regime alone: the sampled (path, step) pairs hold both regimes and, from two steps on with
    enough of them, all four transitions."""
    if T >= 1:
        assert set(ref["s"].ravel().tolist()) == {0, 1}
    if T >= 7:
        assert rr.transitions_seen(ref["s"]) == {(0, 0), (0, 1), (1, 0), (1, 1)}


CASES = [  # N, K, T, path_begin, n_paths
    (1, 1, 7, 0, 3000),
    (1, 1, 60, 0, 3000),
    (3, 3, 60, (1 << 32) - 1500, 3000),
    (13, 8, 1, 17, 5000),
    (13, 8, 12, 17, 5000),
    (16, 1, 60, 0, 4096),
    (16, 3, 0, 0, 3000),
    (17, 20, 7, 5, 3000),
    (64, 3, 7, (1 << 32) - 7, 3000),
    (64, 1, 12, 0, 3000),
    (3, 1, 12, 0, 1_000_003),
]


@pytest.mark.parametrize("N,K,T,begin,n", CASES)
def test_terminal_values_equal_the_restatement(N, K, T, begin, n, gpu_ctx):
    mu, L, mu1, L1, W = _market(N, K, 3)
    out = _run(gpu_ctx, _ffi.make_params(N, T, K), PROBS, mu, L, mu1, L1, W, begin, n)
    st, term = out.stats, out.terminal
    ids = _pick(n, begin, 6 if N >= 16 and T > 7 else 12)
    ref = rr.simulate_regimes(mu, L, mu1, L1, W, T, SEED, (begin + ids).astype(np.uint64), PROBS)
    _covers_both(ref, T)
    assert np.array_equal(_bits(term[:, ids]), _bits(ref["V_T"]))
    for k in (0, K - 1):
        want = ref_stats.path_stats(term[k])
        assert st[k]["var"] == want["var"] and st[k]["n_tail"] == want["n_tail"]
        assert st[k]["min"] == want["min"] and st[k]["max"] == want["max"] and st[k]["n"] == n
        for f in ("mean", "std", "sharpe", "cvar"):
            assert abs(st[k][f] - want[f]) <= 1e-12 * max(1.0, abs(want[f])), f


@pytest.mark.parametrize("N,K", [(3, 1), (16, 3), (5, 20), (64, 8)])
def test_horizon_rows_are_the_n_steps_h_calls_and_the_bands_np_percentile(N, K, gpu_ctx):
    T, n, hz, lv = 24, 5000, [1, 5, 12, 24], (2.5, 50.0, 97.5)
    mu, L, mu1, L1, W = _market(N, K, 5)
    out = _run(gpu_ctx, _ffi.make_params(N, T, K), PROBS, mu, L, mu1, L1, W, 3, n, horizons=hz, levels=lv)
    for i, h in enumerate(hz):
        oh = _run(gpu_ctx, _ffi.make_params(N, h, K), PROBS, mu, L, mu1, L1, W, 3, n)
        assert np.array_equal(_bits(out.horizon_terminal[i]), _bits(oh.terminal))
        for k in range(K):
            x = x_of(out.horizon_terminal[i, k])
            assert out.hz_stats[i, k]["var"] == np.percentile(x, (1 - 0.95) * 100) == oh.stats[k]["var"]
            for jj, q in enumerate(lv):
                assert out.bands[i, k, jj] == np.percentile(x, q)
    plain = _run(gpu_ctx, _ffi.make_params(N, T, K), PROBS, mu, L, mu1, L1, W, 3, n)
    assert np.array_equal(_bits(out.terminal), _bits(plain.terminal)) and plain.stats.tobytes() == out.stats.tobytes()
    ids = _pick(n, 3, 6)
    ref = rr.simulate_regimes(mu, L, mu1, L1, W, T, SEED, (3 + ids).astype(np.uint64), PROBS, horizons=hz)
    _covers_both(ref, T)
    assert np.array_equal(_bits(out.horizon_terminal[:, :, ids]), _bits(ref["V_h"]))


@pytest.mark.parametrize("N,K,T", [(1, 1, 60), (16, 3, 12), (17, 20, 7), (13, 8, 12), (64, 1, 7)])
def test_drawdown_equals_the_restatement(N, K, T, gpu_ctx):
    n = 5000
    mu, L, mu1, L1, W = _market(N, K, 7)
    out = _run(gpu_ctx, _ffi.make_params(N, T, K), PROBS, mu, L, mu1, L1, W, 9, n, drawdown=True)
    plain = _run(gpu_ctx, _ffi.make_params(N, T, K), PROBS, mu, L, mu1, L1, W, 9, n)
    assert np.array_equal(_bits(out.terminal), _bits(plain.terminal)) and plain.stats.tobytes() == out.stats.tobytes()
    ids = _pick(n, 9, 6)
    ref = rr.simulate_regimes(mu, L, mu1, L1, W, T, SEED, (9 + ids).astype(np.uint64), PROBS)
    _covers_both(ref, T)
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


@pytest.mark.parametrize("N,K,T", [(1, 1, 12), (3, 3, 12), (16, 1, 60), (16, 8, 12), (17, 20, 7), (64, 3, 7)])
def test_the_anchors_are_the_gaussian_calls(N, K, T, gpu_ctx):
    """Identical regimes at (0.2, 0.3, 0.5), then all calm (start = 0, p01 = 0) against the Gaussian call on (mu, L), then all crisis
    (start = 1, p10 = 0) against the Gaussian call on (mu1, L1): terminal, horizon and drawdown rows and the statistics' bytes."""
    n, prm = 5000, _ffi.make_params(N, T, K)
    mu, L, mu1, L1, W = _market(N, K, 1)
    hz = sorted({1, max(1, T // 2), T})
    cases = ((PROBS, (mu, L, mu, L), (mu, L)),                         # identical regimes
             ((0.0, 0.3, 0.0), (mu, L, mu1, L1), (mu, L)),             # start = 0, p01 = 0: never in regime 1
             ((0.2, 0.0, 1.0), (mu, L, mu1, L1), (mu1, L1)))           # start = 1, p10 = 0: never in regime 0
    for probs, both, (m, f) in cases:
        st, term = _gauss(gpu_ctx, prm, m, f, W, 7, n)
        h = gpu_ctx.simulate_horizons(prm, m, f, W, SEED, 7, n, hz, (5.0, 95.0), True)
        d = gpu_ctx.simulate_drawdown(prm, m, f, W, SEED, 7, n, True)
        out = _run(gpu_ctx, prm, probs, *both, W, 7, n)
        assert np.array_equal(_bits(out.terminal), _bits(term)) and out.stats.tobytes() == st.tobytes()
        out = _run(gpu_ctx, prm, probs, *both, W, 7, n, horizons=hz, levels=(5.0, 95.0))
        assert np.array_equal(_bits(out.horizon_terminal), _bits(h[4])) and out.hz_stats.tobytes() == h[1].tobytes()
        assert np.array_equal(out.bands, h[2]) and out.stats.tobytes() == h[0].tobytes()
        out = _run(gpu_ctx, prm, probs, *both, W, 7, n, drawdown=True)
        assert np.array_equal(_bits(out.qd), _bits(d[3])) and out.dd_stats.tobytes() == d[1].tobytes()
    far = _run(gpu_ctx, prm, PROBS, mu, L, mu1, L1, W, 7, n)
    assert not np.array_equal(_bits(far.terminal), _bits(_gauss(gpu_ctx, prm, mu, L, W, 7, n)[1]))


def test_records_are_numpy_on_the_stored_values(gpu_ctx):
    N, K, T, n = 16, 3, 12, 200_001
    mu, L, mu1, L1, W = _market(N, K, 3)
    prm = _ffi.make_params(N, T, K, v0=10_000.0, alpha=0.99, rf=0.01)
    out = _run(gpu_ctx, prm, PROBS, mu, L, mu1, L1, W, 0, n)
    for k in range(K):
        want = ref_stats.path_stats(out.terminal[k], v0=10_000.0, alpha=0.99, rf=0.01)
        x = x_of(out.terminal[k], v0=10_000.0)
        st = out.stats
        assert st[k]["var"] == np.percentile(x, (1 - 0.99) * 100) == want["var"]
        assert st[k]["n_tail"] == want["n_tail"] and st[k]["min"] == x.min() and st[k]["max"] == x.max()
        for f in ("mean", "std", "sharpe", "cvar"):
            assert abs(st[k][f] - want[f]) <= 1e-12 * max(1.0, abs(want[f])), f


def test_the_chain_is_read_off_exactly(gpu_ctx):
    """N = 1, L = L1 = 0, mu = 0, mu1 = 1, v0 = 1: a step in regime 1 doubles the value and a step in regime 0 keeps it, so V_h =
    2^(steps so far in regime 1) exactly and s_{h-1} = V_h / V_{h-1} - 1.  The regime paths equal the restatement's on sampled ids;
    the occupancy of every step lies within 5 binomial standard errors of (pi P^t)_1 and both transition frequencies within 5
    binomial standard errors of p^01 and p^10."""
    n, T = 1_000_000, 24
    zero, one = np.zeros(1, np.float32), np.ones(1, np.float32)
    Z = np.zeros((1, 1), np.float32)
    out = _run(gpu_ctx, _ffi.make_params(1, T, 1), PROBS, zero, Z, one, Z, np.ones((1, 1), np.float32), 0, n,
               horizons=list(range(1, T + 1)), levels=())
    V = np.vstack([np.ones((1, n)), out.horizon_terminal[:, 0, :].astype(np.float64)])
    s = V[1:] / V[:-1] - 1.0
    assert np.all((s == 0.0) | (s == 1.0))
    s = s.astype(np.uint8)
    assert np.array_equal(V[1:], 2.0 ** np.cumsum(s, axis=0)) and np.array_equal(out.terminal[0].astype(np.float64), V[-1])
    ids = _pick(n, 0, 24)
    thr, p = rr.regime_consts(*PROBS)
    assert np.array_equal(s[:, ids], rr.regime_path(SEED, ids.astype(np.uint64), T, thr))
    occ, want = s.mean(axis=1), rr.occupancy_direct(*p, T)
    z_occ = (occ - want) / np.sqrt(want * (1.0 - want) / n)
    from0, from1 = s[:-1] == 0, s[:-1] == 1
    n0, n1 = int(from0.sum()), int(from1.sum())
    f01, f10 = float((from0 & (s[1:] == 1)).sum()) / n0, float((from1 & (s[1:] == 0)).sum()) / n1
    z01, z10 = (f01 - p[0]) / np.sqrt(p[0] * (1.0 - p[0]) / n0), (f10 - p[1]) / np.sqrt(p[1] * (1.0 - p[1]) / n1)
    print("occupancy z", np.round(z_occ, 2).tolist(), "p01", f01, z01, "p10", f10, z10)
    assert np.all(np.abs(z_occ) < 5.0) and abs(z01) < 5.0 and abs(z10) < 5.0


@pytest.mark.parametrize("persistent", [True, False])
def test_the_laws_of_the_step(persistent, gpu_ctx):
    """10^6 paths, N = 3, K = 3, T = 24, horizons every step: the assertions of regime_ref.law_checks, which the binary64 twin passes
    on the CPU (test_regimes_cpu.test_the_twin_passes_the_law_assertions_at_the_gpu_tests_size), for every portfolio -- the mean of
    x_h against the pivot of SPEC.md 5.13, Var rho_t against regime_law, and the lag-1 correlation of rho_t^2: above 0 with p01 =
    0.05, p10 = 0.2 and distinct regimes, at 0 with identical regimes."""
    n, T, N, K = 1_000_000, 24, 3, 3
    probs = (0.05, 0.2, 0.7)
    mu, L, mu1, L1, W = _market(N, K, 11)
    if not persistent:
        mu1, L1 = mu, L
    prm = _ffi.make_params(N, T, K)
    out = _run(gpu_ctx, prm, probs, mu, L, mu1, L1, W, 0, n, horizons=list(range(1, T + 1)), levels=())
    law = regime_law(probs, mu, L, mu1, L1, W, T)
    piv, hz = _ffi.regime_pivots(prm, probs, mu, mu1, W, list(range(1, T + 1)))
    assert np.array_equal(hz, law.pivots) and np.array_equal(piv, law.pivots[-1])
    for k in range(K):
        print(persistent, k, rr.law_checks(out.horizon_terminal[:, k, :], 1.0, law.pivots[:, k], law.mean[:, k], law.var[:, k], persistent))
        assert abs(out.stats[k]["mean"] - piv[k]) < 5 * out.stats[k]["std"] / np.sqrt(n)
        assert np.all(np.abs(out.hz_stats["mean"][:, k] - hz[:, k]) < 5 * out.hz_stats["std"][:, k] / np.sqrt(n))


def test_any_partition_of_the_paths_gives_the_same_values(gpu_ctx):
    N, K, T, n, begin = 16, 20, 12, 30_001, 11
    mu, L, mu1, L1, W = _market(N, K, 9)
    prm = _ffi.make_params(N, T, K)
    hz = dict(horizons=[5, 12], levels=(50.0,))
    one = _run(gpu_ctx, prm, PROBS, mu, L, mu1, L1, W, begin, n, **hz)
    one_dd = _run(gpu_ctx, prm, PROBS, mu, L, mu1, L1, W, begin, n, drawdown=True)
    cut = 12_345                                           # two calls split at an odd id
    a = _run(gpu_ctx, prm, PROBS, mu, L, mu1, L1, W, begin, cut, **hz)
    b = _run(gpu_ctx, prm, PROBS, mu, L, mu1, L1, W, begin + cut, n - cut, **hz)
    assert np.array_equal(_bits(np.concatenate([a.terminal, b.terminal], axis=1)), _bits(one.terminal))
    assert np.array_equal(_bits(np.concatenate([a.horizon_terminal, b.horizon_terminal], axis=2)), _bits(one.horizon_terminal))
    for devices in ((0, 0), (0, 0, 0)):
        c = Context(devices)
        try:
            sh = _run(c, prm, PROBS, mu, L, mu1, L1, W, begin, n, **hz)
            sp = _run(c, _ffi.make_params(N, T, K, shard_portfolios=True), PROBS, mu, L, mu1, L1, W, begin, n, **hz)
            sd = _run(c, prm, PROBS, mu, L, mu1, L1, W, begin, n, drawdown=True)
        finally:
            c.close()
        for other in (sh, sp):
            assert np.array_equal(one.terminal, other.terminal) and np.array_equal(one.horizon_terminal, other.horizon_terminal)
            assert np.array_equal(one.bands, other.bands)
            for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi", "cvar"):
                assert np.array_equal(one.stats[f], other.stats[f]) and np.array_equal(one.hz_stats[f], other.hz_stats[f]), f
            assert np.allclose(one.stats["mean"], other.stats["mean"], rtol=1e-12)
            assert np.allclose(one.stats["std"], other.stats["std"], rtol=1e-12)
        assert np.array_equal(one_dd.terminal, sd.terminal) and np.array_equal(one_dd.qd, sd.qd)
        for f in ("var", "n_tail", "min", "max"):
            assert np.array_equal(one_dd.dd_stats[f], sd.dd_stats[f]) and np.array_equal(one_dd.stats[f], sd.stats[f]), f


def test_small_terminal_budget_tiles_the_portfolios(gpu_ctx):
    N, K, T = 4, 20, 12
    mu, L, mu1, L1, W = _market(N, K, 2)
    prm = _ffi.make_params(N, T, K)
    kw = dict(horizons=[4, 12], levels=(5.0, 95.0))
    want = _run(gpu_ctx, prm, PROBS, mu, L, mu1, L1, W, 0, 10_000, **kw)
    c = Context(0, terminal_budget=3 * 3 * 10_000 * 4)
    try:
        got = _run(c, prm, PROBS, mu, L, mu1, L1, W, 0, 10_000, **kw)
    finally:
        c.close()
    assert np.array_equal(want.terminal, got.terminal) and np.array_equal(want.horizon_terminal, got.horizon_terminal)
    assert np.array_equal(want.bands, got.bands)
    for f in ("var", "n_tail", "min", "max"):
        assert np.array_equal(want.stats[f], got.stats[f]) and np.array_equal(want.hz_stats[f], got.hz_stats[f])


def test_rejected_call_then_a_correct_one_then_a_gaussian_call(gpu_ctx):
    mu, L, mu1, L1, W = _market(16, 3, 1)
    prm = _ffi.make_params(16, 40, 3)
    g0, gt0 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    fresh = Context(0)
    try:
        want = _run(fresh, prm, PROBS, mu, L, mu1, L1, W, 0, 50_000)
    finally:
        fresh.close()
    fn = _ffi.lib().mcp_simulate_regimes
    st = np.zeros(3, _ffi.STATS_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    bad_reserved = _ffi.make_regimes(*PROBS, mu1, L1)
    bad_reserved.reserved = 1
    for bad in (_ffi.make_regimes(1.5, 0.3, 0.5, mu1, L1), _ffi.make_regimes(0.2, 0.3, -0.5, mu1, L1), bad_reserved):
        assert fn(gpu_ctx._h, ctypes.byref(prm), ctypes.byref(bad), vp(mu), vp(L), vp(W), SEED, 0, 50_000, 0, None, 0, None, None,
                  vp(st), None, None, None, None, None) == _ffi.MCP_E_ARG
    with pytest.raises(_ffi.McpError):
        _run(gpu_ctx, _ffi.make_params(16, 40, 3, compounding="log"), PROBS, mu, L, mu1, L1, W, 0, 1000, store=False)
    got = _run(gpu_ctx, prm, PROBS, mu, L, mu1, L1, W, 0, 50_000)
    assert np.array_equal(want.terminal, got.terminal) and want.stats.tobytes() == got.stats.tobytes()
    g1, gt1 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    assert np.array_equal(gt0, gt1) and g0.tobytes() == g1.tobytes()


def test_simulate_paths_returns_its_shapes(gpu_ctx):
    mu, cov = (np.asarray(a, np.float64) for a in synthetic.synthetic_market(3))
    mu1, cov1 = mu - 0.01, 4.0 * cov
    r = (0.05, 0.2, mu1, cov1)
    w = [0.2, 0.3, 0.5]
    one = simulate_paths(mu, cov, w, n_steps=12, n_paths=5000, regimes=r, store=True, horizons=[1, 6, 12], bands=(5.0, 95.0),
                         context=gpu_ctx)
    assert one["n"] == 5000 and one["terminal"].shape == (5000,) and one["horizons"]["bands"].shape == (3, 2)
    assert one["horizon_terminal"].shape == (3, 5000)
    blk = one["regimes"]
    assert set(blk) == {"p01", "p10", "start", "stationary", "mean_duration", "occupancy"}
    p = rr.regime_consts(0.05, 0.2, 0.2)[1]
    assert (blk["p01"], blk["p10"], blk["start"]) == tuple(p) and blk["occupancy"].shape == (3,)
    assert blk["stationary"] == pytest.approx(0.2, abs=1e-9) and blk["mean_duration"] == pytest.approx((20.0, 5.0), rel=1e-8)
    dd = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, regimes=r + (0.9,), drawdown=True, store=True, context=gpu_ctx)
    assert isinstance(dd, list) and len(dd) == 3 and dd[0]["max_drawdown"].shape == (5000,) and "cdar" in dd[0]["drawdown"]
    assert dd[0]["regimes"]["start"] == rr.regime_consts(0.05, 0.2, 0.9)[1][2] and "occupancy" not in dd[0]["regimes"]
    arr = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, regimes=r, as_array=True, context=gpu_ctx)
    assert arr.shape == (3,) and arr.dtype == _ffi.STATS_DTYPE
    g = simulate_paths(mu, cov, w, n_steps=12, n_paths=5000, store=True, context=gpu_ctx)
    assert not np.array_equal(g["terminal"], one["terminal"]) and "regimes" not in g
    same = simulate_paths(mu, cov, w, n_steps=12, n_paths=5000, regimes=(0.0, 0.2, mu1, cov1, 0.0), store=True, context=gpu_ctx)
    assert np.array_equal(g["terminal"], same["terminal"]) and g["var"] == same["var"] and same["regimes"]["stationary"] == 0.0
    # an explicit chol= takes the fourth entry as regime 1's factor: the same call
    L, L1 = np.linalg.cholesky(cov), np.linalg.cholesky(cov1)
    fac = simulate_paths(mu, cov, w, n_steps=12, n_paths=5000, regimes=(0.05, 0.2, mu1, L1), chol=L, store=True, context=gpu_ctx)
    noh = simulate_paths(mu, cov, w, n_steps=12, n_paths=5000, regimes=r, store=True, context=gpu_ctx)
    assert np.array_equal(fac["terminal"], noh["terminal"]) and np.array_equal(noh["terminal"], one["terminal"])
    # a crisis regime fattens the left tail
    big = simulate_paths(mu, cov, w, n_steps=12, n_paths=200_000, regimes=r, context=gpu_ctx)
    ref = simulate_paths(mu, cov, w, n_steps=12, n_paths=200_000, context=gpu_ctx)
    assert big["var"] < ref["var"] and big["cvar"] < ref["cvar"] and big["std"] > ref["std"]
    sw = simulate_sweep(mu, cov, weights=np.eye(3), n_steps=12, n_paths=5000, regimes=r, context=gpu_ctx)
    assert np.array_equal(sw["stats"]["var"], arr["var"])


def test_pipeline_prints_the_regime_lines(gpu_ctx):
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
    assert text.count("regime fit: p01 = ") == 1
    assert text.count("optimum without regimes: VaR = ") == 1 and text.count("optimum with regimes:    VaR = ") == 1

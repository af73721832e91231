"""GPU checks of tolerance-band rebalancing (SPEC.md 4.18 / 5.18): values, trade counts and turnover bit-equal to the NumPy restatement
(band_ref.py) over widths, portfolio counts, step counts, review periods, costs and draw sources, the second grid-stride tile included;
the records, the histogram and its reductions against NumPy on the stored arrays; the anchors (every tolerance 0: the calendar call;
nothing watched: buy-and-hold); properties (c), (d), (e); recovery after a rejected call; the law of the one review; the cost; the
public functions' shapes and the example's line."""
import contextlib
import io
import os
import re
import runpy
import sys

import numpy as np
import pytest

import band_ref
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, band_law, simulate_bootstrap, simulate_paths, synthetic, tolerance_bands
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs
from rebalance_ref import boot_returns, gauss_returns

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x7B_A2D5
Q_ALPHA = (1 - 0.95) * 100
LEVELS = (0.0, 5.0, 50.0, 95.0, 100.0)
TILE2 = 8192 * 256                                       # paths of the first tile of every workgroup: ids from here on are walked second
_bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)   # noqa: E731


def _market(N, K, seed=0, scale=1.0):
    """Every portfolio of one asset holds cash beside it (a single asset at weight 1 never leaves a band); else 10 % cash in the last."""
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(seed + 31 * N + K).dirichlet(np.ones(N), size=K)
    if N == 1:
        W = W * np.linspace(0.5, 0.8, K)[:, None]
    elif K > 1:
        W[-1] *= 0.9
    return prepare_inputs(np.asarray(mu) * scale, np.asarray(cov) * scale, W)


def _table(R, N, seed=0):
    return (np.random.default_rng(seed + 1000 * N + R).standard_t(3, size=(R, N)) * 0.02 + 0.001).astype(np.float32)


def _pick(n_paths, begin):
    """Two whole waves (ids 0 .. 63 and 64 .. 127 of the launch), the ends, a spread, and both sides of a 2^32 crossing and of the
    second grid-stride tile."""
    ids = set(range(0, min(128, n_paths))) | {n_paths - 1, n_paths // 2}
    ids.update(np.linspace(0, n_paths - 1, 20).astype(int).tolist())
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 3)))
    if n_paths > TILE2:
        ids.update(range(TILE2 - 64, min(n_paths, TILE2 + 128)))
    return np.array(sorted(ids), np.int64)


def _bands(W, scale):
    """One asset not watched (the second, where there are two), bands of `scale` (wider from portfolio to portfolio) on the others."""
    K, N = W.shape
    tol = np.full((K, N), scale, np.float32) * (1.0 + 0.25 * np.arange(K, dtype=np.float32))[:, None]
    if N > 1:
        tol[:, 1] = np.inf
    return tol


def _choose_bands(r, W, e, cost, hz, waves):
    """Of a fixed ladder of scales, the one with the most trades among those at which the restatement shows, over the sampled paths, a
    review that trades, one that does not, and a whole wave (64 consecutive ids; `waves`: slices into the sample) with no trade at some
    review -> (tol, restatement)."""
    best = None
    for scale in 0.3 * 0.75 ** np.arange(32):
        tol = _bands(W, float(scale))
        ref = band_ref.banded(r, W, tol, e, cost, v0=2.0, horizons=hz)
        hits = ref["hits"]
        if hits.any() and not hits.all() and any(not hits[:, :, w].any(axis=2).all() for w in waves):
            if best is None or hits.mean() > best[1]["hits"].mean():
                best = (tol, ref)
    assert best is not None, "no scale of the ladder decides both ways on the sample"
    return best


def _hz(T):
    if T < 1:
        return []
    return sorted({1, max(1, T // 2), T if T % 2 == 0 else max(1, T - 1)})


def _check_records(out, K, n, n_rev, v0, hz):
    """The records, bands, histogram, sum, order statistics and the turnover record against NumPy on the stored arrays."""
    for k in range(K):
        x, st = x_of(out.terminal[k], "simple", v0), out.stats[k]
        assert st["n"] == n and st["var"] == np.percentile(x, Q_ALPHA) and st["min"] == x.min() and st["max"] == x.max()
        assert abs(st["mean"] - x.mean()) <= 1e-12 * max(1.0, abs(x.mean())) and abs(st["std"] - x.std(ddof=1)) <= 1e-12 * max(1e-3, x.std(ddof=1))
        for i in range(len(hz)):
            xh = x_of(out.horizon_terminal[i, k], "simple", v0)
            assert out.hz_stats[i, k]["var"] == np.percentile(xh, Q_ALPHA)
            assert out.bands[i, k, 0] == np.percentile(xh, 5.0) and out.bands[i, k, 1] == np.percentile(xh, 50.0)
        c = out.trades[k].astype(np.int64)
        assert out.trade_hist.shape == (K, n_rev + 1) and np.array_equal(out.trade_hist[k], np.bincount(c, minlength=n_rev + 1))
        assert out.trade_sum[k] == c.sum() and np.array_equal(out.trade_q[k], np.percentile(c, LEVELS, method="lower").astype(np.uint32))
        y, ts = out.turnover[k].astype(np.float64) - 1.0, out.turnover_stats[k]
        print(f"portfolio {k}: trades mean {c.mean():.3f} of {n_rev}, turnover mean {y.mean() + 1:.5f}  record mean {ts['mean'] + 1:.5f}")
        assert ts["n"] == n and ts["var"] == np.percentile(y, Q_ALPHA) and ts["min"] == y.min() and ts["max"] == y.max()
        assert ts["n_tail"] == int(np.sum(y <= ts["var"])) and ts["sharpe"] == 0.0
        tail = y[y <= ts["var"]]
        assert abs(ts["cvar"] - tail.mean()) <= 1e-12 * abs(tail.mean())
        assert abs(ts["mean"] - y.mean()) <= 1e-12 * abs(y.mean()) and abs(ts["std"] - y.std(ddof=1)) <= 1e-12 * max(1e-3, y.std(ddof=1))
        # (e) on every stored path
        assert c.max() <= n_rev and np.array_equal(_bits(out.turnover[k][c == 0]), np.zeros(int((c == 0).sum()), np.uint32))
        assert np.all(out.turnover[k][c > 0] > 0)


CASES = [  # N, K, T, e, cost, source, R, n          (LDS holds the table when R * ceil(N/4) <= 1088)
    (1, 1, 7, 1, 0.0, "gauss", 0, 1337),
    (1, 3, 7, 2, 1e-3, "boot", 50, 1337),
    (3, 3, 60, 5, 1e-3, "gauss", 0, 1337),
    (3, 2, 60, 59, 0.0, "boot", 100_000, 1337),
    (16, 1, 60, 1, 1e-3, "gauss", 0, 1337),
    (16, 3, 60, 5, 1e-3, "boot", 272, 1337),
    (16, 1, 60, 5, 1e-3, "boot", 5000, 1337),
    (17, 3, 1, 1, 1e-3, "gauss", 0, 1337),
    (17, 1, 0, 0, 0.0, "gauss", 0, 1337),
    (64, 1, 7, 2, 1e-3, "gauss", 0, 1337),
    (64, 2, 7, 3, 0.0, "boot", 68, 1337),
    (3, 1, 6, 2, 1e-3, "gauss", 0, TILE2 + 300),       # the second grid-stride tile: c and Y start from zero there too
    (3, 17, 7, 2, 1e-3, "gauss", 0, 1337),             # K >= 17: still one pass per portfolio, on the moment slots of the wide layout
]


@pytest.mark.parametrize("N,K,T,e,cost,source,R,n", CASES)
def test_values_counts_and_turnover_equal_the_restatement(N, K, T, e, cost, source, R, n, gpu_ctx):
    mu, L, W = _market(N, K, N + T, scale=4.0)
    rows = _table(R, N) if source == "boot" else None
    begin = 0 if n > TILE2 else (1 << 32) - 700
    hz, n_rev = _hz(T), band_ref.n_reviews(T, e)
    ids = _pick(n, begin)
    paths = (begin + ids).astype(np.uint64)
    r = boot_returns(rows, T, SEED, paths, 2.5) if rows is not None else gauss_returns(mu, L, T, SEED, paths)
    if T == 0:
        r = np.zeros((0, ids.size, 4 * ((N + 3) // 4)), np.float32)
    starts = [0, 64] + ([TILE2 - 64, TILE2, TILE2 + 64] if n > TILE2 else [])
    waves = [np.flatnonzero((ids >= s) & (ids < s + 64)) for s in starts]
    assert all(w.size == 64 for w in waves)
    if n_rev:
        tol, ref = _choose_bands(r, W, e, cost, hz, waves)
        print(f"bands {tol[0, 0]:.5f}: {ref['hits'].mean():.3f} of the sampled reviews trade")
    else:                                                   # T <= e: no review, nothing to decide
        tol = _bands(W, 0.01)
        ref = band_ref.banded(r, W, tol, e, cost, v0=2.0, horizons=hz)
    prm = _ffi.make_params(N, T, K, v0=2.0)
    kw = dict(rows=rows, block=2.5) if rows is not None else dict(mu=mu, chol=L)
    out = gpu_ctx.simulate_banded(prm, e, cost, tol, W, SEED, begin, n, True, levels=LEVELS, horizons=hz if hz else None, bands=(5.0, 50.0), **kw)
    assert np.array_equal(out.trades[:, ids], ref["c"])
    assert np.array_equal(_bits(out.turnover[:, ids]), _bits(ref["Y"]))
    assert np.array_equal(_bits(out.terminal[:, ids]), _bits(ref["V_T"]))
    if hz:
        assert np.array_equal(_bits(out.horizon_terminal[:, :, ids]), _bits(ref["V_h"]))
    _check_records(out, K, n, n_rev, 2.0, hz)


@pytest.mark.parametrize("source", ["gauss", "lds", "global"])
def test_anchors_zero_tolerance_and_nothing_watched(source, gpu_ctx):
    """(a): every tolerance 0 is simulate_paths(rebalance=e, rebalance_cost=kappa); (b): nothing watched, and e = 0, are rebalance=0."""
    N, K, T, n, e, kap = 16, 3, 24, 20_011, 4, 1e-3
    mu, L, W = _market(N, K, 4)
    hz, levels = [1, 5, 12, 24], (2.5, 50.0, 97.5)
    if source == "gauss":
        call = lambda **kw: simulate_paths(mu, L @ L.T.astype(np.float64), W, n_steps=T, n_paths=n, seed=SEED, path_begin=9,   # noqa: E731
                                           chol=L, store=True, context=gpu_ctx, horizons=hz, bands=levels, **kw)
    else:
        rows = _table(272 if source == "lds" else 4000, N, 4)
        call = lambda **kw: simulate_bootstrap(rows, W, n_steps=T, n_paths=n, block=3.0, seed=SEED, path_begin=9,   # noqa: E731
                                               store=True, context=gpu_ctx, horizons=hz, bands=levels, **kw)

    def same_values(a, b):
        assert np.array_equal(_bits(a["terminal"]), _bits(b["terminal"])) and np.array_equal(_bits(a["horizon_terminal"]), _bits(b["horizon_terminal"]))
        for f in ("var", "n_tail", "min", "max", "cvar", "x_lo", "x_hi"):
            assert a[f] == b[f], f
        for f in ("mean", "std", "sharpe"):
            assert abs(a[f] - b[f]) <= 1e-12 * max(1e-300, abs(a[f])), f
        assert np.array_equal(a["horizons"]["bands"], b["horizons"]["bands"]) and np.array_equal(a["horizons"]["var"], b["horizons"]["var"])
    n_rev = (T - 1) // e
    zero_weight = np.full((K, N), np.inf)
    Wz = W.copy()
    Wz[:, 3] = 0.0
    zero_weight[:, 3] = 0.0                                  # an asset of weight 0 at tolerance 0: 0 >= +0, every review trades
    for want, got in zip(call(rebalance=e, rebalance_cost=kap), call(rebalance=e, rebalance_cost=kap, tolerance=0.0)):
        same_values(want, got)
        tb = got["tolerance"]
        assert tb["n_reviews"] == n_rev and np.all(tb["trades"]["paths"] == n_rev) and tb["trades"]["mean"] == n_rev
        assert np.array_equal(tb["trades"]["hist"], [0] * n_rev + [n]) and np.count_nonzero(tb["trades"]["hist"]) == 1
        assert set(tb["trades"]["q"].values()) == {n_rev} and np.all(tb["turnover"]["paths"] > 0)
    for tol_kw in (dict(rebalance=e, tolerance=np.inf), dict(rebalance="never", tolerance=0.0), dict(rebalance=T, tolerance=0.0)):
        for want, got in zip(call(rebalance="never", rebalance_cost=kap), call(rebalance_cost=kap, **tol_kw)):
            same_values(want, got)
            tb = got["tolerance"]
            assert not tb["trades"]["paths"].any() and tb["trades"]["mean"] == 0.0 and tb["trades"]["hist"][0] == n
            assert np.array_equal(_bits(tb["turnover"]["paths"]), np.zeros(n, np.uint32)) and tb["turnover"]["mean"] == 0.0 == tb["turnover"]["max"]
    if source == "gauss":
        base = dict(n_steps=T, n_paths=n, seed=SEED, path_begin=9, chol=L, store=True, context=gpu_ctx, rebalance=e, rebalance_cost=kap)
        cov = L @ L.T.astype(np.float64)
        for want, got in zip(simulate_paths(mu, cov, Wz, **base), simulate_paths(mu, cov, Wz, tolerance=zero_weight, **base)):
            assert np.array_equal(_bits(want["terminal"]), _bits(got["terminal"])) and np.all(got["tolerance"]["trades"]["paths"] == n_rev)


def _mixed(gpu_ctx, N, K, T, e, n, hz=None, kap=1e-3, ctx=None, prm=None, scale=0.02, seed=60):
    mu, L, W = _market(N, K, seed, scale=4.0)
    tol = _bands(W, scale)
    prm = prm or _ffi.make_params(N, T, K)
    out = (ctx or gpu_ctx).simulate_banded(prm, e, kap, tol, W, SEED, 11, n, True, levels=LEVELS, horizons=hz, bands=(50.0,), mu=mu, chol=L)
    return out, (mu, L, W, tol)


def test_property_c_the_call_of_h_steps_gives_the_horizon(gpu_ctx):
    N, K, T, e, n, hz = 5, 2, 24, 3, 10_007, [3, 10, 23]
    full, (mu, L, W, tol) = _mixed(gpu_ctx, N, K, T, e, n, hz)
    assert 0.05 < full.trade_sum[0] / (n * 7) < 0.95
    ids = np.arange(256)
    r = gauss_returns(mu, L, T, SEED, (11 + ids).astype(np.uint64))
    hits = band_ref.banded(r, W, tol, e, 1e-3)["hits"]
    for i, h in enumerate(hz):
        cut = gpu_ctx.simulate_banded(_ffi.make_params(N, h, K), e, 1e-3, tol, W, SEED, 11, n, True, mu=mu, chol=L)
        assert np.array_equal(_bits(cut.terminal), _bits(full.horizon_terminal[i])), h
        assert np.array_equal(cut.trades[:, ids], hits[:band_ref.n_reviews(h, e)].sum(axis=0)), h      # the trades before step h
        assert np.all(cut.trades <= full.trades)
    _check_records(full, K, n, 7, 1.0, [])


def test_property_d_shards_and_tiles(gpu_ctx):
    """Two logical shards of one device, portfolio shards, and a budget that forces tiles of 2 of the 5 portfolios."""
    N, K, T, e, n, hz = 16, 5, 30, 4, 30_001, [10, 30]
    one, (mu, L, W, tol) = _mixed(gpu_ctx, N, K, T, e, n, hz)
    assert 0 < one.trade_sum[0] < 7 * n
    others = []
    c = Context((0, 0))
    try:
        others.append(_mixed(gpu_ctx, N, K, T, e, n, hz, ctx=c)[0])
        others.append(_mixed(gpu_ctx, N, K, T, e, n, hz, ctx=c, prm=_ffi.make_params(N, T, K, shard_portfolios=True))[0])
    finally:
        c.close()
    c = Context(0, terminal_budget=2 * n * (4 * (1 + len(hz)) + 12))
    try:
        others.append(_mixed(gpu_ctx, N, K, T, e, n, hz, ctx=c)[0])
    finally:
        c.close()
    for o in others:
        assert np.array_equal(o.trades, one.trades) and np.array_equal(_bits(o.turnover), _bits(one.turnover))
        assert np.array_equal(_bits(o.terminal), _bits(one.terminal)) and np.array_equal(_bits(o.horizon_terminal), _bits(one.horizon_terminal))
        assert np.array_equal(o.trade_hist, one.trade_hist) and np.array_equal(o.trade_sum, one.trade_sum) and np.array_equal(o.trade_q, one.trade_q)
        for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi"):
            assert np.array_equal(o.turnover_stats[f], one.turnover_stats[f]) and np.array_equal(o.stats[f], one.stats[f]), f


def test_rejected_call_then_a_correct_one_leaves_no_residue(gpu_ctx):
    N, K, T, e, n = 16, 3, 40, 4, 50_000
    fresh = Context(0)
    try:
        want, (mu, L, W, tol) = _mixed(gpu_ctx, N, K, T, e, n, ctx=fresh)
        plain_want = fresh.simulate(_ffi.make_params(N, T, K), mu, L, W, SEED, 0, n, True)
    finally:
        fresh.close()
    prm = _ffi.make_params(N, T, K)
    first = _mixed(gpu_ctx, N, K, T, e, n)[0]
    bad_tol = tol.copy()
    bad_tol[1, 2] = -0.5
    for args, msg in (((e, 1e-3, bad_tol), r"tol\[18\]"), ((e, 1.5, tol), "cost"), ((-1, 1e-3, tol), "every")):
        with pytest.raises(_ffi.McpError, match=msg):
            gpu_ctx.simulate_banded(prm, *args, W, SEED, 11, n, True, mu=mu, chol=L)
    with pytest.raises(_ffi.McpError, match="level"):
        gpu_ctx.simulate_banded(prm, e, 1e-3, tol, W, SEED, 11, n, True, levels=(101.0,), mu=mu, chol=L)
    with pytest.raises(_ffi.McpError, match="compound simply"):
        gpu_ctx.simulate_banded(_ffi.make_params(N, T, K, compounding="log"), e, 1e-3, tol, W, SEED, 11, 1000, False, mu=mu, chol=L)
    got = _mixed(gpu_ctx, N, K, T, e, n)[0]
    for o in (first, got):
        assert np.array_equal(o.trades, want.trades) and np.array_equal(o.trade_hist, want.trade_hist) and np.array_equal(o.trade_sum, want.trade_sum)
        assert np.array_equal(o.trade_q, want.trade_q) and np.array_equal(_bits(o.terminal), _bits(want.terminal))
        assert o.stats.tobytes() == want.stats.tobytes() and o.turnover_stats.tobytes() == want.turnover_stats.tobytes()
    assert np.all(got.trade_hist.sum(axis=1) == n) and 0 < got.trade_sum[0] < 9 * n
    stats, term = gpu_ctx.simulate(prm, mu, L, W, SEED, 0, n, True)
    assert np.array_equal(plain_want[1], term) and plain_want[0].tobytes() == stats.tobytes()


def test_the_one_review_trades_by_its_law(gpu_ctx):
    """N = 1, w = 0.5 beside cash, T = 2, e = 1, 10^6 Gaussian paths, r ~ N(0.01, 0.05^2), tol = 0.01: the one review trades with the
    probability band_law gives, about 0.43.  hist[1] is a binomial count, so the bound is five binomial standard errors,
    5 sqrt(p (1 - p) / n) = 2.5e-3; the binary32 roundings of the review move the thresholds by a few 1e-8 in r, below 1e-6 in
    probability."""
    n, w, tol = 1_000_000, 0.5, 0.01
    mu, cov = np.array([0.01]), np.array([[0.0025]])
    mu32, L, W32 = prepare_inputs(mu, cov, [w])
    d = simulate_paths(mu, cov, [w], n_steps=2, n_paths=n, seed=SEED, tolerance=tol, context=gpu_ctx)
    p = band_law(float(W32[0, 0]), float(mu32[0]), float(L[0, 0]), float(np.float32(tol)))
    hist = d["tolerance"]["trades"]["hist"]
    got, se = int(hist[1]) / n, np.sqrt(p * (1.0 - p) / n)
    print(f"P(trade) = {got:.6f}, law {p:.6f} ({abs(got - p) / se:.2f} se)")
    assert hist.shape == (2,) and int(hist.sum()) == n and 0.3 < p < 0.6 and abs(got - p) <= 5.0 * se
    assert d["tolerance"]["trades"]["mean"] == got


def test_the_cost_is_paid_by_the_paths_that_trade(gpu_ctx):
    N, K, e, n = 4, 1, 6, 40_000
    T = 2 * e
    mu, L, W = _market(N, K, 8, scale=4.0)
    tol = _bands(W, 0.02)
    prm = _ffi.make_params(N, T, K)
    paid = gpu_ctx.simulate_banded(prm, e, 2e-3, tol, W, SEED, 0, n, True, mu=mu, chol=L)
    free = gpu_ctx.simulate_banded(prm, e, 0.0, tol, W, SEED, 0, n, True, mu=mu, chol=L)
    traded = paid.trades[0] == 1
    assert 0.1 < traded.mean() < 0.9 and np.array_equal(paid.trades, free.trades) and np.array_equal(_bits(paid.turnover), _bits(free.turnover))
    assert np.array_equal(traded, paid.turnover[0] > 0)
    assert np.all(paid.terminal[0, traded] < free.terminal[0, traded])
    assert np.array_equal(_bits(paid.terminal[0, ~traded]), _bits(free.terminal[0, ~traded]))
    ids = np.flatnonzero(traded)[:200]
    ref = band_ref.banded(gauss_returns(mu, L, T, SEED, ids.astype(np.uint64)), W, tol, e, 2e-3)
    assert ref["hits"].all() and np.array_equal(_bits(paid.terminal[0, ids]), _bits(ref["V_T"][0]))
    assert np.array_equal(_bits(paid.turnover[0, ids]), _bits(ref["Y"][0]))


def test_simulate_paths_and_bootstrap_return_their_shapes(gpu_ctx):
    mu, cov = synthetic.synthetic_market(3)
    cov = cov * 20.0
    n, T, w = 5000, 12, [0.2, 0.3, 0.5]
    one = simulate_paths(mu, cov, w, n_steps=T, n_paths=n, rebalance=2, rebalance_cost=1e-3, tolerance=tolerance_bands(w, 0.05, 0.25), store=True,
                         horizons=[4, 12], context=gpu_ctx)
    cal = simulate_paths(mu, cov, w, n_steps=T, n_paths=n, rebalance=2, rebalance_cost=1e-3, store=True, horizons=[4, 12], context=gpu_ctx)
    assert sorted(set(one) - set(cal)) == ["tolerance"] and one["n"] == n
    tb = one["tolerance"]
    assert sorted(tb) == ["every", "n_reviews", "table", "trades", "turnover"] and tb["every"] == 2 and tb["n_reviews"] == 5
    assert np.allclose(tb["table"], [0.05, 0.05, 0.05]) and sorted(tb["trades"]) == ["hist", "mean", "paths", "q"]
    c, y = tb["trades"]["paths"], tb["turnover"]["paths"]
    assert c.shape == (n,) and c.dtype == np.uint32 and y.shape == (n,) and y.dtype == np.float32 and 0 < c.sum() < 5 * n
    assert np.array_equal(tb["trades"]["hist"], np.bincount(c, minlength=6)) and tb["trades"]["mean"] == c.astype(np.int64).sum() / n
    assert tb["trades"]["q"] == {q: int(np.percentile(c, q, method="lower")) for q in (5.0, 50.0, 95.0)}
    assert tb["turnover"]["var"] == np.percentile(y.astype(np.float64) - 1.0, Q_ALPHA) + 1.0
    assert tb["turnover"]["min"] == float(y.min()) and tb["turnover"]["max"] == float(y.max())
    assert abs(tb["turnover"]["mean"] - y.astype(np.float64).mean()) <= 1e-12
    many = simulate_paths(mu, cov, np.eye(3) * 0.5, n_steps=T, n_paths=n, tolerance=0.02, tolerance_levels=(50,), context=gpu_ctx)
    assert isinstance(many, list) and len(many) == 3 and "paths" not in many[0]["tolerance"]["trades"] and many[0]["tolerance"]["every"] == 1
    assert list(many[2]["tolerance"]["trades"]["q"]) == [50.0] and many[2]["tolerance"]["n_reviews"] == T - 1
    tup = simulate_paths(mu, cov, np.eye(3) * 0.5, n_steps=T, n_paths=n, tolerance=0.02, rebalance=3, as_array=True, store=True, context=gpu_ctx)
    hist, total, q, ts, trades, turn = tup[-6:]
    assert hist.shape == (3, 4) and total.shape == (3,) and q.shape == (3, 3) and ts.shape == (3,) and trades.shape == (3, n) and turn.shape == (3, n)
    rows = np.random.default_rng(5).normal(0.002, 0.03, size=(120, 3))
    b = simulate_bootstrap(rows, w, n_steps=T, n_paths=n, block=4.0, tolerance=[0.03, np.inf, 0.03], rebalance=3, store=True, context=gpu_ctx)
    tb = b["tolerance"]
    assert tb["n_reviews"] == 3 and np.array_equal(tb["trades"]["hist"], np.bincount(tb["trades"]["paths"], minlength=4)) and np.isinf(tb["table"][1])
    assert 0 < tb["trades"]["paths"].sum() < 3 * n


def test_pipeline_prints_the_rebalancing_lines(gpu_ctx):
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
    found = re.findall(r"rebalancing by (quarterly calendar|5/25 bands): mean trades ([0-9.]+) of (\d+) reviews  median turnover ([0-9.]+)  "
                       r"VaR = ([-+0-9.]+)  CVaR = ([-+0-9.]+)", out.getvalue())
    assert [f[0] for f in found] == ["quarterly calendar", "5/25 bands"], out.getvalue()
    (_, ct, cr, cy, _, _), (_, bt, br, by, _, _) = found
    assert float(ct) == int(cr) and 0 <= float(bt) <= int(br) and int(br) > int(cr) and float(cy) > 0 and float(by) >= 0

"""GPU checks of spending rules (SPEC.md 4.16 / 5.16): V_T, V_h and Y_T bit-equal to the NumPy restatement (spend_ref.py) on sampled
path ids for Gaussian, Student-t and bootstrap (row table in LDS and in global memory) draws, over the shapes at which one thing each
can break -- one asset, a width that is no multiple of 4, passes of 8 portfolios with k_begin > 0, a path range across 2^32, no
steps, no review, a period longer than the walk, a review on a horizon step and on step T, a grid-stride loop with a second tile --
with a coverage condition asserted on the restatement (every clamp outcome taken, paths ruined, a remainder paid); the anchors (a
constant withdrawal is the cash-flow call, no withdrawal is the plain call, V_h is the truncated call); tiles, shards and recovery
after a rejected call; the records; the law of the percentage rule; the public functions and the example's lines."""
import contextlib
import io
import os
import re
import runpy
import sys

import numpy as np
import pytest

import spend_ref
from cashflow_ref import counts_of
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, simulate_bootstrap, simulate_paths, spending_law, spending_rule, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs
from oracle import ref_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5BE2D
VARIANTS = ["gauss", "t", "boot_lds", "boot_global"]
EXACT = ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max")
CLOSE = ("mean", "std", "sharpe", "cvar")
TILE2 = 8192 * 256                                       # paths of the first tile of every workgroup: ids from here on are walked second


def _market(N, K, T, scale=None):
    """The synthetic market with every drift set to 0.05 (T <= 7) or 0.01 per step and its covariance scaled (x400 at T <= 7, x16 at
    N <= 3 and x81 above at T = 60) so that a portfolio's step volatility is about 0.15-0.2 or about 0.08: withdrawals of 12 % or 2 %
    of v0 per step then ruin some paths and leave most alive."""
    _, cov = synthetic.synthetic_market(N)
    short = T <= 7
    mu = np.full(N, 0.05 if short else 0.01)
    cov = cov * (scale if scale is not None else 400.0 if short else 16.0 if N <= 3 else 81.0)
    W = np.random.default_rng(31 * N + K + T).dirichlet(np.ones(N), size=K)
    if K > 1:
        W[-1] *= 0.9                                     # 10 % cash in one portfolio
    return prepare_inputs(mu, cov, W)


def _draws(variant, N, mu, L):
    """The draw arguments of Context.simulate_spending / spend_ref.simulate_sp for a kernel variant.  The bootstrap's row table is read
    from LDS while R ceil(N/4) <= 1088 float4 slots and from global memory beyond."""
    if variant == "gauss":
        return {"mu": mu, "chol": L}
    if variant == "t":
        return {"mu": mu, "chol": L, "dof": 5}
    nb = (N + 3) // 4
    R = 40 if variant == "boot_lds" and 40 * nb <= 1088 else (1088 // nb if variant == "boot_lds" else 1088 // nb + 50)
    z = np.random.default_rng(7 * N + R).standard_normal((R, N))
    rows = (mu.astype(np.float64) + z @ L.astype(np.float64).T).astype(np.float32)
    return {"rows": np.ascontiguousarray(rows), "block": 3.0}


def _rule(T, v0=1.0):
    """(rate, every-less tuple pieces): down = up = 0.1, inflation 0.015, rate = first / v0 = 0.12 at T <= 7 and 0.02 above."""
    rate = 0.12 if T <= 7 else 0.02
    return rate, 0.1, 0.1, 0.015, rate * v0


def _pick(n_paths, begin, count, at_least=0):
    """The first and last ids, `count` ids in a block from the first on (the sample the coverage condition is asserted on), and the ids
    around a 2^32 crossing."""
    ids = set(range(at_least, min(n_paths, at_least + count))) | {n_paths - 1, n_paths - 2}
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 3)))
    return np.array(sorted(ids), np.int64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_numpy_record(rec, values, v0=1.0, alpha=0.95):
    want = ref_stats.path_stats(values, v0=v0, alpha=alpha, rf=0.0)
    x = x_of(values, v0=v0)
    assert rec["n"] == values.size and rec["var"] == want["var"] == np.percentile(x, (1 - alpha) * 100)
    assert rec["n_tail"] == want["n_tail"] and rec["min"] == want["min"] and rec["max"] == want["max"]
    for f in ("mean", "std", "cvar"):
        assert abs(rec[f] - want[f]) <= 1e-12 * max(1.0, abs(want[f])), (f, rec[f], want[f])


def _assert_same(got, want, withdrawn=False):
    """Values, counts and bands bit-equal; the record fields EXACT equal and CLOSE within the project's 1e-12 max(1, |want|)."""
    assert np.array_equal(_bits(got.terminal), _bits(want.terminal))
    if want.horizon_terminal is not None:
        assert np.array_equal(_bits(got.horizon_terminal), _bits(want.horizon_terminal)) and np.array_equal(got.bands, want.bands)
    if want.counts is not None:
        assert np.array_equal(got.counts, want.counts)
        assert (want.hz_counts is None and got.hz_counts is None) or np.array_equal(got.hz_counts, want.hz_counts)
    pairs = [(got.stats, want.stats), (got.hz_stats, want.hz_stats)]
    if withdrawn:
        assert np.array_equal(_bits(got.withdrawn), _bits(want.withdrawn))
        pairs.append((got.wd_stats, want.wd_stats))
    for g, w in pairs:
        if w is None:
            continue
        for f in EXACT:
            assert np.array_equal(g[f], w[f]), f
        for f in CLOSE:
            assert np.all(np.abs(g[f] - w[f]) <= 1e-12 * np.maximum(1.0, np.abs(w[f]))), f


CASES = [  # N, K, T, path_begin, n_paths, every, horizons, v0, covered
    (1, 1, 7, 0, 3000, 2, (2, 3, 7), 1.0, True),                         # a review on a horizon step (2)
    (3, 3, 60, (1 << 32) - 1500, 3000, 12, (30, 60), 1.0, True),         # a review on step T, stored as a horizon too
    (13, 8, 7, 17, 1500, 3, (), 100.0, True),
    (16, 1, 60, 0, 4096, 12, (24, 30), 1.0, True),
    (17, 20, 7, 5, 2000, 2, (3, 7), 250.0, True),
    (64, 3, 7, (1 << 32) - 7, 300, 1, (), 1.0, False),
    (16, 20, 0, 0, 1000, 4, (), 1.0, False),                              # no steps
    (5, 2, 7, 0, 1200, 0, (4,), 1.0, False),                              # no review
    (5, 2, 7, 3, 1200, 9, (4,), 1.0, False),                              # a period longer than the walk
    (3, 1, 6, 0, TILE2 + 300, 2, (), 1.0, False),                         # a second grid-stride tile
]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N,K,T,begin,n,every,hz,v0,covered", CASES)
def test_values_equal_the_restatement(N, K, T, begin, n, every, hz, v0, covered, variant, gpu_ctx):
    mu, L, W = _market(N, K, T)
    draws = _draws(variant, N, mu, L)
    rate, down, up, infl, first = _rule(T, v0)
    prm = _ffi.make_params(N, T, K, v0=v0)
    second_tile = n > TILE2
    ids = _pick(n, begin, 256 if covered else 24, at_least=TILE2 if second_tile else 0)
    if second_tile:
        assert ids.min() >= TILE2
        ids = np.r_[[0, TILE2 - 1], ids]                  # and the ends of the first tile
    out = gpu_ctx.simulate_spending(prm, (rate, every, down, up, infl, first), W, SEED, begin, n, True, horizons=list(hz) or None,
                                    levels=(50.0,) if hz else (), target=0.5 * v0, **draws)
    c = spend_ref.consts(rate, down, up, infl, first, v0)
    assert np.array_equal(_bits(_ffi.spending_consts(_ffi.make_spending(rate, every, down, up, infl, first), v0)), _bits(c))
    ref = spend_ref.simulate_sp(c, every, W, T, SEED, (begin + ids).astype(np.uint64), v0=v0, horizons=hz, **draws)
    if covered:                                            # on the restatement, not on the kernel
        shares = spend_ref.outcome_shares(ref["outcome"])
        ruined = float(np.mean(ref["V_T"] == 0))
        print(f"outcomes neither / floor / ceiling {shares}, ruined {ruined:.3f}, remainders {int(ref['remainder'].sum())}")
        assert min(shares) >= 0.05, shares
        assert 0.02 <= ruined <= 0.60, ruined
        assert np.any(ref["remainder"])
    assert np.array_equal(_bits(out.terminal[:, ids]), _bits(ref["V_T"]))
    assert np.array_equal(_bits(out.withdrawn[:, ids]), _bits(ref["Y_T"]))
    if hz:
        assert np.array_equal(_bits(out.horizon_terminal[:, :, ids]), _bits(ref["V_h"]))
        assert np.array_equal(out.hz_counts, counts_of(out.horizon_terminal, 0.5 * v0))
        if hz[-1] == T:
            assert np.array_equal(_bits(out.horizon_terminal[-1]), _bits(out.terminal))
    else:
        assert out.hz_counts is None and out.hz_stats is None
    assert np.array_equal(out.counts, counts_of(out.terminal, 0.5 * v0))
    for a in (out.terminal, out.withdrawn):                # every stored value is +0 or > 0
        assert not np.any(np.signbit(a)) and not np.any(np.isnan(a))
    if T == 0:
        assert np.all(out.terminal == np.float32(v0)) and not out.withdrawn.any()
    for k in (0, K - 1):
        _assert_numpy_record(out.stats[k], out.terminal[k], v0=v0)
        _assert_numpy_record(out.wd_stats[k], out.withdrawn[k], v0=v0)
        assert out.wd_stats[k]["sharpe"] == 0.0


# ---- anchors --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N,K", [(3, 1), (16, 3), (5, 20)])
def test_a_constant_withdrawal_is_the_cashflow_call(N, K, variant, gpu_ctx):
    """(a): every = 0, and down = up = inflation = 0 with every = 1 -- values, horizon rows, counts, records and bands."""
    T, n, hz, lv, v0 = 24, 20_000, [1, 5, 12, 24], (2.5, 50.0, 97.5), 50.0
    mu, L, W = _market(N, K, 60)
    draws = _draws(variant, N, mu, L)
    prm = _ffi.make_params(N, T, K, v0=v0, rf=0.01)
    w0 = spend_ref.consts(0.03, 0.0, 0.0, 0.0, None, v0)[4]
    flows = np.full(T, -w0, np.float32)
    want = gpu_ctx.simulate_cashflow(prm, flows, W, SEED, 3, n, True, horizons=hz, levels=lv, target=40.0, **draws)
    assert 0 < want.counts[:, 0].sum() < K * n
    for sp in ((0.03, 0, 0.3, 0.2, 0.05), (0.03, 1, 0.0, 0.0, 0.0), (0.5, 0, 0.0, 0.0, 0.0, float(w0))):
        got = gpu_ctx.simulate_spending(prm, sp, W, SEED, 3, n, True, horizons=hz, levels=lv, target=40.0, **draws)
        _assert_same(got, want)
        # what the constant plan pays: w0 per live step and the remainder
        alive = got.terminal > 0
        assert np.all(got.withdrawn[alive] == np.float32(0) + np.cumsum(np.full(T, w0, np.float32), dtype=np.float32)[-1])
    solo_want = gpu_ctx.simulate_cashflow(prm, flows, W, SEED, 3, n, True, **draws)
    solo = gpu_ctx.simulate_spending(prm, (0.03, 0, 0.1, 0.1), W, SEED, 3, n, True, **draws)
    _assert_same(solo, solo_want)
    assert solo.hz_stats is None and solo.hz_counts is None


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N,K", [(3, 1), (16, 3), (5, 20)])
def test_no_withdrawal_is_the_plain_call(N, K, variant, gpu_ctx):
    """(b): rate = 0 and first = 0 pay nothing, with or without reviews."""
    T, n, hz, lv = 24, 20_000, [1, 5, 12, 24], (2.5, 50.0, 97.5)
    mu, L, W = _market(N, K, 60, scale=1.0)                # the market's own volatility: no path of the plain call reaches zero
    draws = _draws(variant, N, mu, L)
    prm = _ffi.make_params(N, T, K, v0=50.0, rf=0.01)
    kw = {"rows": draws["rows"], "block": draws["block"]} if "rows" in draws else dict(draws)
    for horizons in (hz, None):                              # the horizon call, then the plain / Student-t / bootstrap call
        want = gpu_ctx._call(prm, W, SEED, 3, n, True, horizons=np.asarray(hz, np.int32) if horizons else None,
                             levels=lv if horizons else (), **kw)
        for sp in ((0.0, 3, 0.1, 0.1, 0.02, 0.0), (0.0, 0, 0.0, np.inf, 0.0, 0.0)):
            got = gpu_ctx.simulate_spending(prm, sp, W, SEED, 3, n, True, horizons=horizons, levels=lv if horizons else (), **draws)
            assert want.counts is None and np.all(want.terminal > 0) and not got.counts.any()
            _assert_same(got, want)
            assert not got.withdrawn.any() and not np.any(np.signbit(got.withdrawn))
            assert np.all(got.wd_stats["mean"] == -1.0) and np.all(got.wd_stats["std"] == 0.0) and np.all(got.wd_stats["var"] == -1.0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_horizon_rows_are_the_truncated_calls(variant, gpu_ctx):
    """(d): V_h is the terminal value of the same call with T = h."""
    N, K, T, n, every = 16, 3, 30, 10_000, 4
    hz = [3, 4, 8, 17, 30]
    mu, L, W = _market(N, K, 60)
    draws = _draws(variant, N, mu, L)
    sp = (0.03, every, 0.1, 0.1, 0.01)
    full = gpu_ctx.simulate_spending(_ffi.make_params(N, T, K), sp, W, SEED, 11, n, True, horizons=hz, levels=(5.0, 95.0), **draws)
    assert 0 < full.counts[:, 0].sum()
    for i, h in enumerate(hz):
        part = gpu_ctx.simulate_spending(_ffi.make_params(N, h, K), sp, W, SEED, 11, n, True, **draws)
        assert np.array_equal(_bits(full.horizon_terminal[i]), _bits(part.terminal)), h
        assert np.array_equal(full.hz_counts[i], part.counts)
        for f in EXACT:
            assert np.array_equal(full.hz_stats[i][f], part.stats[f]), (h, f)
        for f in ("mean", "std", "cvar"):
            assert np.all(np.abs(full.hz_stats[i][f] - part.stats[f]) <= 1e-12 * np.maximum(1.0, np.abs(part.stats[f]))), (h, f)
    assert np.array_equal(_bits(full.horizon_terminal[-1]), _bits(full.terminal))
    assert np.array_equal(_bits(part.withdrawn), _bits(full.withdrawn))


# ---- the host side ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["gauss", "boot_global", "t"])
def test_shards_tiles_and_twenty_portfolios(variant, gpu_ctx):
    N, K, T, n, hz, lv = 16, 20, 30, 30_001, [10, 20, 30], (50.0,)
    mu, L, W = _market(N, K, 60)
    draws = _draws(variant, N, mu, L)
    sp = (0.03, 5, 0.1, 0.1, 0.01)
    prm = _ffi.make_params(N, T, K)
    call = lambda c, p=prm: c.simulate_spending(p, sp, W, SEED, 11, n, True, horizons=hz, levels=lv, target=0.4, **draws)   # noqa: E731
    one = call(gpu_ctx)
    assert np.array_equal(one.counts, counts_of(one.terminal, 0.4)) and np.array_equal(one.hz_counts, counts_of(one.horizon_terminal, 0.4))
    assert 0 < one.counts[0, 0] < n
    ids = np.r_[0:6, n - 3:n]
    ref = spend_ref.simulate_sp(spend_ref.consts(*sp[:1], *sp[2:]), sp[1], W, T, SEED, (11 + ids).astype(np.uint64), horizons=hz, **draws)
    assert np.array_equal(_bits(one.terminal[:, ids]), _bits(ref["V_T"])) and np.array_equal(_bits(one.withdrawn[:, ids]), _bits(ref["Y_T"]))
    others = []
    c = Context((0, 0))                                      # two path shards on one device
    try:
        others.append(call(c))
        others.append(call(c, _ffi.make_params(N, T, K, shard_portfolios=True)))
    finally:
        c.close()
    c = Context(0, terminal_budget=3 * 5 * n * 4)            # tiles of 3 portfolios (5 rows of n binary32 values each)
    try:
        others.append(call(c))
    finally:
        c.close()
    for o in others:
        _assert_same(o, one, withdrawn=True)


def test_records_with_a_large_mass_at_zero(gpu_ctx):
    """The V records and bands against NumPy where most paths are ruined (ties at x = -1), the Y record against NumPy on the stored
    Y, the counts against counts_of."""
    N, K, T, n, hz, lv = 3, 2, 30, 40_000, [10, 30], (5.0, 50.0, 95.0)
    mu, L, W = _market(N, K, 7)
    out = gpu_ctx.simulate_spending(_ffi.make_params(N, T, K, v0=10.0, alpha=0.9), (0.08, 5, 0.1, 0.1, 0.01), W, SEED, 0, n, True,
                                    horizons=hz, levels=lv, target=5.0, mu=mu, chol=L)
    assert np.all(out.counts[:, 0] > 0.6 * n) and np.all(out.counts[:, 0] < n)
    assert np.array_equal(out.counts, counts_of(out.terminal, 5.0)) and np.array_equal(out.hz_counts, counts_of(out.horizon_terminal, 5.0))
    for k in range(K):
        _assert_numpy_record(out.stats[k], out.terminal[k], v0=10.0, alpha=0.9)
        _assert_numpy_record(out.wd_stats[k], out.withdrawn[k], v0=10.0, alpha=0.9)
        assert out.wd_stats[k]["var"] == np.percentile(out.withdrawn[k].astype(np.float64) / 10.0 - 1.0, 10.0)
        for i in range(len(hz)):
            _assert_numpy_record(out.hz_stats[i, k], out.horizon_terminal[i, k], v0=10.0, alpha=0.9)
            assert np.array_equal(out.bands[i, k], np.percentile(x_of(out.horizon_terminal[i, k], v0=10.0), lv))


def test_rejected_call_then_a_correct_one_then_a_plain_one(gpu_ctx):
    N, K, T, n = 16, 3, 40, 50_000
    mu, L, W = _market(N, K, 60)
    prm = _ffi.make_params(N, T, K)
    sp = (0.03, 4, 0.1, 0.1, 0.01)
    fresh = Context(0)
    try:
        want = fresh.simulate_spending(prm, sp, W, SEED, 0, n, True, mu=mu, chol=L)
        plain_want = fresh.simulate(prm, mu, L, W, SEED, 0, n, True)
    finally:
        fresh.close()
    for bad, msg in (((-0.1, 4, 0.1, 0.1), "rate"), ((0.03, 4, 1.5, 0.1), "down"), ((0.03, 4, 0.1, -1.0), "up"),
                     ((0.03, 4, 0.1, 0.1, -1.0), "inflation"), ((0.03, 4, 0.1, 0.1, 0.0, np.nan), "first")):
        with pytest.raises(_ffi.McpError, match=msg):
            gpu_ctx.simulate_spending(prm, bad, W, SEED, 0, n, True, mu=mu, chol=L)
    with pytest.raises(_ffi.McpError, match="compound simply"):
        gpu_ctx.simulate_spending(_ffi.make_params(N, T, K, compounding="log"), sp, W, SEED, 0, 1000, False, mu=mu, chol=L)
    got = gpu_ctx.simulate_spending(prm, sp, W, SEED, 0, n, True, mu=mu, chol=L)
    assert np.array_equal(want.terminal, got.terminal) and want.stats.tobytes() == got.stats.tobytes()
    assert np.array_equal(want.withdrawn, got.withdrawn) and want.wd_stats.tobytes() == got.wd_stats.tobytes()
    assert np.array_equal(want.counts, got.counts) and got.counts[0, 0] > 0
    stats, term = gpu_ctx.simulate(prm, mu, L, W, SEED, 0, n, True)
    assert np.array_equal(plain_want[1], term) and plain_want[0].tobytes() == stats.tobytes()


def test_simulate_paths_and_bootstrap_return_their_shapes(gpu_ctx):
    mu, cov = synthetic.synthetic_market(3)
    cov = cov * 100.0
    rule = spending_rule("floor_ceiling", 0.05, every=4, down=0.025, up=0.05, inflation=0.01)
    one = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, spending=rule, store=True, horizons=[4, 12], bands=(5.0, 95.0),
                         context=gpu_ctx)
    assert one["n"] == 5000 and one["terminal"].shape == (5000,) and one["withdrawn"].shape == (5000,) and "cashflow" not in one
    sp = one["spending"]
    assert sp["every"] == 4 and sp["rate"] == float(np.float32(0.05)) and sp["lo"] == float(np.float32(0.975)) and sp["hi"] == float(np.float32(1.05))
    assert sp["growth"] == float(np.float32(1.01)) and sp["first"] == float(np.float32(0.05)) and sp["target"] is None
    assert sp["n_ruined"] == np.count_nonzero(one["terminal"] == 0) and sp["horizons"]["n_ruined"].shape == (2,) and "n_short" not in sp
    wd = sp["withdrawn"]
    assert wd["n"] == 5000 and wd["mean_v0"] == wd["mean"] + 1.0 and wd["var_v0"] == wd["var"] + 1.0 and wd["cvar_v0"] == wd["cvar"] + 1.0
    assert wd["var"] == np.percentile(x_of(one["withdrawn"]), (1 - 0.95) * 100)
    many = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, spending=spending_rule("percentage", 0.04), target=0.8, dof=4,
                          context=gpu_ctx)
    assert isinstance(many, list) and len(many) == 3 and "horizons" not in many[0]
    assert 0.0 <= many[0]["spending"]["shortfall_probability"] <= 1.0 and many[0]["spending"]["hi"] == float("inf")
    tup = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, spending=spending_rule("constant", 0.1, every=4, inflation=0.02),
                         as_array=True, store=True, context=gpu_ctx)
    s, t, c, ws, y = tup
    assert t.shape == (3, 5000) and y.shape == (3, 5000) and np.array_equal(c, counts_of(t)) and ws.shape == (3,) and c[:, 0].sum() > 0
    arr = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, spending=(0.02, 3, 0.1, 0.1), as_array=True, horizons=[6], context=gpu_ctx)
    assert len(arr) == 6 and arr[3].shape == (3, 2) and arr[4].shape == (1, 3, 2) and arr[5].shape == (3,)
    rows = np.random.default_rng(5).normal(0.002, 0.03, size=(120, 3))
    b = simulate_bootstrap(rows, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, block=4.0, spending=(0.09, 3, 0.1, 0.1), target=0.3, store=True,
                           horizons=[6, 12], context=gpu_ctx)
    assert b["spending"]["n_ruined"] == np.count_nonzero(b["terminal"] == 0) and b["spending"]["horizons"]["n_short"].shape == (2,)
    assert b["withdrawn"].dtype == np.float32 and "n_ruined" not in b["horizons"]      # the counts are the 'spending' block's


def test_pipeline_prints_the_spending_lines(gpu_ctx):
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
    m = re.search(r"floor-and-ceiling spending \(reviewed yearly, cut <= 2\.5 %, raise <= 5 %\): ruin probability ([0-9.]+) against ([0-9.]+) fixed  "
                  r"5 % / median payout ([0-9.,]+) / ([0-9.,]+) against ([0-9.,]+) / ([0-9.,]+)", out.getvalue())
    assert m, out.getvalue()
    assert 0.0 <= float(m.group(1)) <= 1.0 and 0.0 <= float(m.group(2)) <= 1.0
    held = re.search(r"withdrawal plan .* ruin probability at the end ([0-9.]+)", out.getvalue())
    assert held and float(held.group(1)) == float(m.group(2))


# ---- the law ------------------------------------------------------------------------------------------------------------------------------

def test_the_percentage_rule_follows_its_law(gpu_ctx):
    """(c): N = 3, T = 12, 10^6 Gaussian paths, every = 1, down = 1, up = inf, p = 0.02.  The means of V_T and Y_T within 5 standard
    errors, the variance of V_T within 5 standard errors from the sample's fourth moment; the bounds are the model's."""
    n, N, T, p = 1_000_000, 3, 12, 0.02
    mu, cov = synthetic.synthetic_market(N)
    mu, cov = mu * 252.0 / 12.0, cov * 252.0 / 12.0                                        # monthly steps
    w = [0.5, 0.3, 0.2]
    mu32, L, W = prepare_inputs(mu, cov, w)
    d = simulate_paths(mu, cov, w, n_steps=T, n_paths=n, seed=SEED, spending=spending_rule("percentage", p), store=True, context=gpu_ctx)
    cov_used = np.tril(L).astype(np.float64) @ np.tril(L).astype(np.float64).T
    law_mean, law_var, law_paid = spending_law(mu32, cov_used, w, T, p)
    v, y = d["terminal"].astype(np.float64), d["withdrawn"].astype(np.float64)
    assert d["spending"]["n_ruined"] == 0
    mean, var = v.mean(), v.var(ddof=1)
    c = v - mean
    m2, m4 = np.mean(c ** 2), np.mean(c ** 4)
    se_mean, se_var, se_paid = v.std(ddof=1) / np.sqrt(n), np.sqrt((m4 - m2 * m2) / n), y.std(ddof=1) / np.sqrt(n)
    print(f"V mean {mean:.9f} law {law_mean:.9f} ({abs(mean - law_mean) / se_mean:.2f} se) | var {var:.9e} law {law_var:.9e} "
          f"({abs(var - law_var) / se_var:.2f} se) | Y mean {y.mean():.9f} law {law_paid:.9f} ({abs(y.mean() - law_paid) / se_paid:.2f} se)")
    assert abs(mean - law_mean) <= 5 * se_mean and abs(var - law_var) <= 5 * se_var and abs(y.mean() - law_paid) <= 5 * se_paid
    assert abs(d["mean"] + 1.0 - mean) <= 1e-12 and abs(d["spending"]["withdrawn"]["mean_v0"] - y.mean()) <= 1e-12

"""GPU checks of drift uncertainty (SPEC.md 2.7 / 4.21 / 5.21): terminal values, the drawdown q / d, the horizon rows and the cash-flow
walk bit-equal to the NumPy restatement (uncertain_ref.py) on each of the seven kernel rows, over widths, portfolio counts, a path range
across 2^32 on stream 5 and a second grid-stride tile, on a dense factor and on one with a zero row and a zero column; the anchors (a)
M = 0 against the call without the keyword, (b) V_h against the call with T = h, (c) tiles, logical shards and portfolio shards against
the unsplit call; the records, bands and counts against NumPy on the stored values; the law of S_h at 10^6 paths, which the call
without the feature and a redraw per step both miss; the public surface."""
import math

import numpy as np
import pytest

import uncertain_ref as ref_
from cashflow_ref import counts_of
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, drift_law, simulate_paths
from monte_carlo_portfolio_amd.simulate import Context
from oracle import ref_stats

CASES, ROWS, SEED, market, pick = ref_.CASES, ref_.ROWS, ref_.SEED, ref_.market, ref_.pick

pytestmark = pytest.mark.gpu
FACTORS = {"dense": ref_.dense_factor, "holed": ref_.holed_factor}
EXACT = ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _row_kw(family, T, v0=1.0):
    """The keywords of Context.simulate_uncertain and of uncertain_ref.simulate for one kernel family."""
    hz = ref_.horizons_of(T) if family in ("hz", "cf") else None
    call = dict(drawdown=family == "dd", horizons=hz, levels=(5.0, 50.0) if hz else (),
                flows=ref_.flows_of(T, v0) if family == "cf" else None, target=0.02 * v0 if family == "cf" else None)
    ref = dict(drawdown=family == "dd", horizons=hz or (), flows=call["flows"])
    return call, ref


@pytest.mark.parametrize("factor", sorted(FACTORS))
@pytest.mark.parametrize("family,compounding", ROWS)
@pytest.mark.parametrize("N,K,T,begin,n", CASES)
def test_values_equal_the_restatement(N, K, T, begin, n, family, compounding, factor, gpu_ctx):
    mu, L, W = market(N, K)
    M = FACTORS[factor](N)
    prm = _ffi.make_params(N, T, K, compounding)
    call, rkw = _row_kw(family, T)
    ids = pick(n, begin)
    ref = ref_.simulate(mu, L, M, W, T, SEED, (begin + ids).astype(np.uint64), compounding, **rkw)
    if factor == "dense":                                  # the drift differs from path to path and from the launch's: parity is not mu's
        assert np.all(ref["m"].std(axis=0) > 0) and not np.any(ref["m"] == mu)
    out = gpu_ctx.simulate_uncertain(prm, M, mu, L, W, SEED, begin, n, True, **call)
    assert np.array_equal(_bits(out.terminal[:, ids]), _bits(ref["V_T"]))
    if family == "dd":
        assert np.array_equal(_bits(out.qd[:, ids]), _bits(ref["q"]))
    if call["horizons"]:
        assert np.array_equal(_bits(out.horizon_terminal[:, :, ids]), _bits(ref["V_h"]))
        assert np.array_equal(_bits(out.horizon_terminal[-1]), _bits(out.terminal))          # the last horizon is T
    if family == "cf":
        ruined = ref["V_T"] == 0
        assert 0.02 < ruined.mean() < 0.98, ruined.mean()  # the schedule ruins some paths and not others, on the restatement
        assert np.array_equal(out.counts, counts_of(out.terminal, call["target"]))
        assert np.array_equal(out.hz_counts, counts_of(out.horizon_terminal, call["target"]))
        assert not np.any(np.signbit(out.terminal)) and not np.any(np.isnan(out.terminal))
    else:
        assert out.counts is None and out.hz_counts is None


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("family,compounding", ROWS)
def test_anchor_a_a_zero_factor_is_the_call_without_the_keyword(family, compounding, K, gpu_ctx):
    """M = 0: every stored value, count and exact statistic is the call's without uncertainty.  At K = 1 the plain call runs the lean
    kernel, another kernel: equality holds all the same."""
    N, T, n, begin = 5, 12, 20_000, 7
    mu, L, W = market(N, K)
    prm = _ffi.make_params(N, T, K, compounding)
    call, _ = _row_kw(family, T)
    zero = np.zeros((N, N), np.float32)
    zero[2, 1] = -0.0                                      # -0 is +0 on the way in
    got = gpu_ctx.simulate_uncertain(prm, zero, mu, L, W, SEED, begin, n, True, **call)
    want = gpu_ctx._call(prm, W, SEED, begin, n, True, mu=mu, chol=L, **call)
    assert np.array_equal(_bits(got.terminal), _bits(want.terminal))
    for f in EXACT:
        assert np.array_equal(got.stats[f], want.stats[f]), f
    if family == "dd":
        assert np.array_equal(_bits(got.qd), _bits(want.qd)) and np.array_equal(got.dd_stats["var"], want.dd_stats["var"])
    if call["horizons"]:
        assert np.array_equal(_bits(got.horizon_terminal), _bits(want.horizon_terminal)) and np.array_equal(got.bands, want.bands)
    if family == "cf":
        assert np.array_equal(got.counts, want.counts) and np.array_equal(got.hz_counts, want.hz_counts) and 0 < got.counts[:, 0].min() < n
    moved = gpu_ctx.simulate_uncertain(prm, ref_.dense_factor(N), mu, L, W, SEED, begin, n, True, **call)
    live = (moved.terminal != 0) | (want.terminal != 0)     # a path ruined in both calls stores +0 in both
    assert np.mean(_bits(moved.terminal)[live] != _bits(want.terminal)[live]) > 0.9     # and a factor that is not zero moves the values


@pytest.mark.parametrize("family,compounding", [r for r in ROWS if r[0] in ("hz", "cf")])
def test_anchor_b_a_horizon_row_is_the_terminal_row_of_the_call_with_t_equal_h(family, compounding, gpu_ctx):
    N, K, T, n, begin = 6, 9, 13, 5000, (1 << 32) - 2000
    mu, L, W = market(N, K)
    M = ref_.dense_factor(N)
    call, _ = _row_kw(family, T)
    full = gpu_ctx.simulate_uncertain(_ffi.make_params(N, T, K, compounding), M, mu, L, W, SEED, begin, n, True, **call)
    for i, h in enumerate(call["horizons"]):
        kw = dict(call, horizons=None, levels=(), flows=None if call["flows"] is None else call["flows"][:h])
        part = gpu_ctx.simulate_uncertain(_ffi.make_params(N, h, K, compounding), M, mu, L, W, SEED, begin, n, True, **kw)
        assert np.array_equal(_bits(full.horizon_terminal[i]), _bits(part.terminal)), h
        if family == "cf":
            assert np.array_equal(full.hz_counts[i], part.counts)


@pytest.mark.parametrize("family,compounding", [("plain", "log"), ("dd", "simple"), ("hz", "simple"), ("cf", "simple")])
def test_anchor_c_tiles_and_shards_equal_the_unsplit_call(family, compounding, gpu_ctx):
    N, K, T, n, begin = 5, 3, 6, 30_001, (1 << 32) - 10_000
    mu, L, W = market(N, K)
    M = ref_.holed_factor(N)
    prm = _ffi.make_params(N, T, K, compounding)
    call, _ = _row_kw(family, T)
    one = gpu_ctx.simulate_uncertain(prm, M, mu, L, W, SEED, begin, n, True, **call)
    per_path = 4 * (1 + (1 if family == "dd" else 0) + (len(call["horizons"]) if call["horizons"] else 0))
    for make in (lambda: Context((0, 0)), lambda: Context((0, 0, 0)), lambda: Context(0, terminal_budget=2 * n * per_path)):
        c = make()
        try:
            got = c.simulate_uncertain(prm, M, mu, L, W, SEED, begin, n, True, **call)
        finally:
            c.close()
        assert np.array_equal(_bits(one.terminal), _bits(got.terminal))
        for f in EXACT:
            assert np.array_equal(one.stats[f], got.stats[f]), f
        if family == "dd":
            assert np.array_equal(_bits(one.qd), _bits(got.qd))
        if call["horizons"]:
            assert np.array_equal(_bits(one.horizon_terminal), _bits(got.horizon_terminal)) and np.array_equal(one.bands, got.bands)
        if family == "cf":
            assert np.array_equal(one.counts, got.counts) and np.array_equal(one.hz_counts, got.hz_counts)


def test_anchor_c_portfolio_shards_and_the_public_block(gpu_ctx):
    """simulate_paths(drift_uncertainty=...): two portfolio shards against one call, the three forms of the keyword, the block."""
    N, K, T, n = 4, 4, 12, 20_000
    mu, L, W = market(N, K)
    cov = (L.astype(np.float64) @ L.astype(np.float64).T)
    kw = dict(n_steps=T, n_paths=n, seed=SEED, horizons=[1, 4, 12], bands=(5, 95), store=True, cashflow=-0.01, target=0.5)
    one = simulate_paths(mu, cov, W, context=gpu_ctx, drift_uncertainty=84, **kw)
    c = Context((0, 0))
    try:
        two = simulate_paths(mu, cov, W, context=c, devices=[0, 0], shard="portfolios", drift_uncertainty=84, **kw)
    finally:
        c.close()
    plain = simulate_paths(mu, cov, W, context=gpu_ctx, **kw)
    as_cov = simulate_paths(mu, cov, W, context=gpu_ctx, drift_uncertainty=cov / 84, **kw)
    Mf = (np.linalg.cholesky(cov) / math.sqrt(84)).astype(np.float32)
    as_factor = simulate_paths(mu, cov, W, context=gpu_ctx, drift_uncertainty=("factor", Mf), **kw)
    for k, (a, b, p) in enumerate(zip(one, two, plain)):
        assert np.array_equal(a["terminal"], b["terminal"]) and np.array_equal(a["horizon_terminal"], b["horizon_terminal"])
        assert a["var"] == b["var"] and a["cashflow"] == b["cashflow"] and np.array_equal(a["horizons"]["bands"], b["horizons"]["bands"])
        assert np.array_equal(a["terminal"], as_factor[k]["terminal"])
        blk = a["drift_uncertainty"]
        law = drift_law(mu, L, Mf, W[k], T)
        assert blk["drift_std"] == law["drift_std"] > 0                            # from the binary32 M alone
        assert abs(blk["log_variance_share"] / law["log_variance_share"] - 1) < 1e-6   # a_k: the call factors cov again, a last-bit matter
        assert np.allclose(blk["horizon_log_variance_share"], [h * law["b"] / (law["a"] + h * law["b"]) for h in (1, 4, 12)], rtol=1e-6)
        assert "drift_uncertainty" not in p and not np.array_equal(a["terminal"], p["terminal"])
        assert a["horizons"]["std"][-1] > p["horizons"]["std"][-1]                 # the fan is wider at T
        assert abs(as_cov[k]["horizons"]["std"][-1] / a["horizons"]["std"][-1] - 1) < 1e-3   # cov / n_obs is the same law (the factor rounds apart)


@pytest.mark.parametrize("compounding", ["simple", "log"])
def test_records_bands_and_counts_are_numpy_on_the_stored_values(compounding, gpu_ctx):
    """The statistics, bands and counts of the underlying call (SPEC.md 5.21), held to the tolerances tests/test_gpu_horizons.py and
    tests/test_gpu_cashflow.py hold them to: var, n_tail, min and max exact, the bands np.percentile's bits (log: its rounding, rtol
    1e-15), mean, std and cvar within 1e-12 relative."""
    N, K, T, n, v0, lv = 5, 3, 12, 20_001, 2.0, (2.5, 50.0, 97.5)
    mu, L, W = market(N, K)
    M = ref_.dense_factor(N)
    prm = _ffi.make_params(N, T, K, compounding, v0=v0)
    hz = [1, 4, 12]
    cash = compounding == "simple"
    flows = ref_.flows_of(T, v0) if cash else None
    out = gpu_ctx.simulate_uncertain(prm, M, mu, L, W, SEED, 3, n, True, horizons=hz, levels=lv, flows=flows, target=0.02 * v0 if cash else None)
    rows = [(out.stats[k], out.terminal[k]) for k in range(K)] + [(out.hz_stats[i][k], out.horizon_terminal[i, k]) for i in range(3) for k in range(K)]
    for rec, values in rows:
        want = ref_stats.path_stats(values, v0=v0, compounding=compounding, alpha=0.95, rf=0.0)
        assert rec["n"] == n
        if cash:
            assert rec["var"] == want["var"] and rec["n_tail"] == want["n_tail"] and rec["min"] == want["min"] and rec["max"] == want["max"]
        else:
            np.testing.assert_allclose(rec["var"], want["var"], rtol=1e-15, atol=1e-17)
        for f in ("mean", "std", "cvar"):
            assert abs(rec[f] - want[f]) <= 1e-12 * max(1.0, abs(want[f])), (f, rec[f], want[f])
    for i in range(3):
        for k in range(K):
            want = np.percentile(x_of(out.horizon_terminal[i, k], compounding, v0), lv)
            if cash:
                assert np.array_equal(out.bands[i, k], want)
            else:
                np.testing.assert_allclose(out.bands[i, k], want, rtol=1e-15, atol=1e-17)
    if cash:
        assert np.array_equal(out.counts, counts_of(out.terminal, 0.02 * v0)) and np.array_equal(out.hz_counts, counts_of(out.horizon_terminal, 0.02 * v0))
        assert 0 < out.counts[:, 0].min() and out.counts[:, 0].max() < n and np.all(out.hz_counts[0, :, 0] < out.counts[:, 0])


def _law_inputs():
    """N = 3, T = 12, one portfolio; a dense M scaled so that T b = 3 a: three quarters of the variance of S_T is estimation risk."""
    N, T = 3, 12
    mu, L, W = market(N, 1)
    M0 = ref_.dense_factor(N, 1.0)
    law0 = drift_law(mu, L, M0, W[0], T)
    M = (M0.astype(np.float64) * math.sqrt(3.0 * law0["a"] / (T * law0["b"]))).astype(np.float32)
    return mu, L, M, W, T


def law_checks(S, hz, law, n):
    """At every horizon the mean of S_h within 5 sigma_h / sqrt(n) of h c and its variance within 5 sqrt(2 / n) relative of h a + h^2 b
    (the standard error of a normal sample's variance): two-sided normal bounds at a false-alarm rate below 1e-5, from the binary32
    inputs through drift_law, not fitted to any run.  -> the figures in standard errors, for printing."""
    out = []
    for i, h in enumerate(hz):
        s = np.asarray(S[i], np.float64)
        var_h = h * law["a"] + h * h * law["b"]
        z_mean = (s.mean() - h * law["c"]) / math.sqrt(var_h / n)
        z_var = (s.var() / var_h - 1.0) / math.sqrt(2.0 / n)
        out.append((h, z_mean, z_var))
        print("law: h", h, "mean", z_mean, "variance", z_var)
    return out


def test_the_law_of_the_log_value_at_a_million_paths(gpu_ctx):
    """S_h ~ N(h c, h a + h^2 b).  The binary64 twin is asserted first, so that a failure of the formula shows as such; then the
    kernel's rows; the call without the feature misses the variance at T by a factor of 4; one redraw per step instead of one draw per
    path would give h (a + b), outside the bound at h = 4 and h = 12."""
    mu, L, M, W, T = _law_inputs()
    n, hz = 1_000_000, [1, 4, 12]
    law = drift_law(mu, L, M, W[0], T)
    assert abs(T * law["b"] / (3.0 * law["a"]) - 1.0) < 1e-6
    bound = 5.0
    rng = np.random.default_rng(2024)
    w64, mu64, L64, M64 = W[0].astype(np.float64), mu.astype(np.float64), L.astype(np.float64), M.astype(np.float64)
    drift = (mu64 + rng.standard_normal((n, 3)) @ M64.T) @ w64
    S, twin = np.zeros(n), []
    for t in range(1, T + 1):
        S = S + drift + (rng.standard_normal((n, 3)) @ L64.T) @ w64
        if t in hz:
            twin.append(S.copy())
    for h, z_mean, z_var in law_checks(twin, hz, law, n):
        assert abs(z_mean) < bound and abs(z_var) < bound, ("twin", h, z_mean, z_var)
    prm = _ffi.make_params(3, T, 1, "log")
    out = gpu_ctx.simulate_uncertain(prm, M, mu, L, W, SEED, 0, n, True, horizons=np.array(hz, np.int32), levels=())
    for h, z_mean, z_var in law_checks(out.horizon_terminal[:, 0], hz, law, n):
        assert abs(z_mean) < bound and abs(z_var) < bound, ("kernel", h, z_mean, z_var)
    plain = gpu_ctx._call(prm, W, SEED, 0, n, True, mu=mu, chol=L, horizons=np.array(hz, np.int32), levels=())
    z_plain = law_checks(plain.horizon_terminal[:, 0], hz, law, n)
    assert abs(z_plain[-1][2]) > bound and abs(np.var(plain.horizon_terminal[-1, 0], dtype=np.float64) / law["log_var"] - 0.25) < 0.01
    for h in (4, 12):                                      # a redraw per step: h (a + b) against h a + h^2 b
        assert abs(h * (law["a"] + law["b"]) / (h * law["a"] + h * h * law["b"]) - 1.0) > bound * math.sqrt(2.0 / n)


def test_a_rejected_call_leaves_no_residue(gpu_ctx):
    N, K, T, n = 3, 3, 12, 5000
    mu, L, W = market(N, K)
    M = ref_.dense_factor(N)
    prm = _ffi.make_params(N, T, K)
    want = gpu_ctx.simulate_uncertain(prm, M, mu, L, W, SEED, 5, n, True)
    bad = M.copy()
    bad[1, 0] = np.inf
    for bad_prm, m, kw in ((_ffi.make_params(N, T, K, native_math=True), M, {}), (prm, bad, {}),
                           (prm, M, dict(drawdown=True, horizons=np.array([3], np.int32)))):
        with pytest.raises(_ffi.McpError):
            gpu_ctx.simulate_uncertain(bad_prm, m, mu, L, W, SEED, 5, n, True, **kw)
        got = gpu_ctx.simulate_uncertain(prm, M, mu, L, W, SEED, 5, n, True)
        assert np.array_equal(_bits(got.terminal), _bits(want.terminal)) and got.stats.tobytes() == want.stats.tobytes()

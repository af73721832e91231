"""GPU checks of the time under water (SPEC.md 4.20 / 5.20): terminal values, the drawdown q / d and the two counters m and c_T bit-equal
to the NumPy restatement (underwater_ref.py) on each of the four kernel rows -- Gaussian simple, Gaussian log, the GARCH walk on
Student-t and on GARCH draws, the jump walk -- over widths, portfolio counts, step counts, a path range across 2^32 and a second
grid-stride tile, on inputs whose coverage is asserted on the restatement; property (a) against the call without the option; (b) and
(c) on every stored path, the counters recomputed from the values a horizon call stores; the anchors (e); histograms, sums and order
statistics against NumPy on either side of the LDS limit of the histogram kernel; partitions (d); a rejected call; the two laws at 10^6
paths; the public surface."""
import contextlib
import io
import os
import re
import runpy
import sys

import numpy as np
import pytest

import underwater_ref as ref_
from monte_carlo_portfolio_amd import _ffi, simulate_paths
from monte_carlo_portfolio_amd.simulate import Context

CASES, DRAWS, ROWS, SEED, market, pick = ref_.CASES, ref_.DRAWS, ref_.ROWS, ref_.SEED, ref_.market, ref_.pick

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0.0, 5.0, 50.0, 95.0, 100.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _kw(draw):
    kw = dict(DRAWS[draw])
    if "jumps" in kw:
        kw["jumps"] = tuple(float(v) for v in kw["jumps"]) + (None,)
    return kw


def _run(ctx, prm, mu, L, W, begin, n, draw="gauss", store=True, levels=LEVELS):
    return ctx.simulate_underwater(prm, mu, L, W, SEED, begin, n, store, levels=levels, **_kw(draw))


def _integers_are_numpy(out, T, n, levels=LEVELS):
    """SPEC.md 5.20 on the stored counters: the histograms are np.bincount, the sums the integers' sums, the order statistics
    np.percentile(method="lower")."""
    for r, (per_path, hist) in enumerate(((out.uw_longest, out.uw_longest_hist), (out.uw_current, out.uw_current_hist))):
        assert hist.shape == (per_path.shape[0], T + 1) and np.all(hist[:, T] == 0) and np.all(hist.sum(axis=1) == n)
        for k in range(per_path.shape[0]):
            assert np.array_equal(hist[k], np.bincount(per_path[k], minlength=T + 1).astype(np.uint64)), (r, k)
            assert int(out.uw_sums[k, r]) == int(per_path[k].astype(np.uint64).sum())
            assert np.array_equal(out.uw_q[k, r], np.percentile(per_path[k], levels, method="lower").astype(np.uint32)), (r, k)


@pytest.mark.parametrize("draw,compounding", ROWS)
@pytest.mark.parametrize("N,K,T,begin,n", CASES)
def test_values_and_counters_equal_the_restatement(N, K, T, begin, n, draw, compounding, gpu_ctx):
    prm = _ffi.make_params(N, T, K, compounding)
    mu, L, W = market(N, K)
    ids = np.arange(n) if n <= 1037 else pick(n, begin)
    ref = ref_.simulate(mu, L, W, T, SEED, (begin + ids).astype(np.uint64), compounding, **DRAWS[draw])
    print(ref_.covers(ref, T))
    out = _run(gpu_ctx, prm, mu, L, W, begin, n, draw)
    assert np.array_equal(_bits(out.terminal[:, ids]), _bits(ref["V_T"]))
    assert np.array_equal(_bits(out.qd[:, ids]), _bits(ref["q"]))
    assert out.uw_longest.dtype == np.uint32 and np.array_equal(out.uw_longest[:, ids], ref["m"])
    assert np.array_equal(out.uw_current[:, ids], ref["c"])
    _integers_are_numpy(out, T, n)
    if T == 1:
        assert not out.uw_longest.any() and not out.uw_current.any()


@pytest.mark.parametrize("draw,compounding", ROWS)
def test_properties_a_b_c_against_the_calls_without_the_option(draw, compounding, gpu_ctx):
    """(a): everything the drawdown call returns is the call's with the option, bit for bit.  (b), (c): on every stored path, with the
    running peak and both counters recomputed from the values that the horizon call of the same walk stores after every step."""
    N, K, T, n, begin = 5, 9, 12, 20_000, 7
    prm = _ffi.make_params(N, T, K, compounding)
    mu, L, W = market(N, K)
    plain = gpu_ctx._call(prm, W, SEED, begin, n, True, mu=mu, chol=L, drawdown=True, **_kw(draw))
    out = _run(gpu_ctx, prm, mu, L, W, begin, n, draw)
    assert np.array_equal(_bits(out.terminal), _bits(plain.terminal)) and np.array_equal(_bits(out.qd), _bits(plain.qd))
    assert out.stats.tobytes() == plain.stats.tobytes() and out.dd_stats.tobytes() == plain.dd_stats.tobytes()
    lean = _run(gpu_ctx, prm, mu, L, W, begin, n, draw, store=False)                       # nothing stored: the same records and integers
    assert lean.terminal is None and lean.uw_longest is None and lean.stats.tobytes() == out.stats.tobytes()
    assert np.array_equal(lean.uw_longest_hist, out.uw_longest_hist) and np.array_equal(lean.uw_q, out.uw_q) and np.array_equal(lean.uw_sums, out.uw_sums)
    X = gpu_ctx._call(prm, W, SEED, begin, n, True, mu=mu, chol=L, horizons=np.arange(1, T + 1, dtype=np.int32), **_kw(draw)).horizon_terminal
    assert np.array_equal(_bits(X[-1]), _bits(out.terminal))
    P = np.maximum.accumulate(X, axis=0)
    under = X < P
    c = np.zeros(X.shape[1:], np.uint32)
    m = np.zeros(X.shape[1:], np.uint32)
    for t in range(T):
        c = np.where(under[t], c + np.uint32(1), np.uint32(0)).astype(np.uint32)
        m = np.maximum(m, c)
    assert np.array_equal(out.uw_longest, m) and np.array_equal(out.uw_current, c)
    assert np.array_equal(out.uw_current > 0, X[-1] < P[-1])                              # (b)
    ref_.properties({"m": out.uw_longest, "c": out.uw_current, "q": out.qd}, T, compounding)   # (b), (c)
    assert np.array_equal(np.unique(out.uw_longest), np.arange(T))


@pytest.mark.parametrize("draw,compounding", ROWS[:4])
def test_property_e_the_deterministic_anchors(draw, compounding, gpu_ctx):
    T, N, K, n = 12, 5, 9, 3000
    _, _, W = market(N, K)
    prm = _ffi.make_params(N, T, K, compounding)
    L = np.zeros((N, N), np.float32)
    for sign, want in ((1.0, 0), (-1.0, T - 1)):
        mu = (sign * np.linspace(0.01, 0.05, N)).astype(np.float32)
        out = _run(gpu_ctx, prm, mu, L, W, 11, n, draw, levels=(50.0,))
        assert np.all(out.uw_longest == want) and np.all(out.uw_current == want), (sign, draw)
        assert np.all(out.uw_longest_hist[:, want] == n) and np.all(out.uw_current_hist[:, want] == n)
        assert np.all(out.uw_sums == n * want) and np.all(out.uw_q == want)


@pytest.mark.parametrize("T", [8191, 8192])
def test_histograms_on_either_side_of_the_lds_limit(T, gpu_ctx):
    """T + 1 bins = LIFE_LDS_BINS = 8192 (the LDS path of life_hist_kernel) and 8193 (its global path); a strongly negative drift, so
    that the top bins are hit."""
    n, K = 2000, 2
    prm = _ffi.make_params(1, T, K)
    mu, L, W = np.array([-0.002], np.float32), np.array([[0.01]], np.float32), np.array([[1.0], [0.5]], np.float32)
    for draw in ("gauss", "jumps"):
        out = _run(gpu_ctx, prm, mu, L, W, 3, n, draw)
        _integers_are_numpy(out, T, n)
        assert out.uw_longest.max() == T - 1 and out.uw_current.max() == T - 1 and np.all(out.uw_longest_hist[:, T - 1] > 0)
        assert np.all(out.terminal > 0) and np.unique(out.uw_longest).size > 50


def test_two_logical_shards_and_two_tiles_equal_one_call(gpu_ctx):
    """Property (d): two logical shards of one device, and a terminal budget that forces two tiles of portfolios (16 bytes per path and
    portfolio: V_T, q, m, c_T), give the one call's values, counters, histograms and order statistics."""
    N, K, T, n = 5, 3, 12, 30_001
    mu, L, W = market(N, K)
    prm = _ffi.make_params(N, T, K)
    ones = {draw: _run(gpu_ctx, prm, mu, L, W, 11, n, draw) for draw in ("t", "jumps")}
    for make in (lambda: Context((0, 0)), lambda: Context(0, terminal_budget=2 * n * 16)):
        c = make()
        try:
            got = {draw: _run(c, prm, mu, L, W, 11, n, draw) for draw in ones}
        finally:
            c.close()
        for draw, one in ones.items():
            sh = got[draw]
            assert np.array_equal(one.terminal, sh.terminal) and np.array_equal(one.qd, sh.qd)
            assert np.array_equal(one.uw_longest, sh.uw_longest) and np.array_equal(one.uw_current, sh.uw_current)
            assert np.array_equal(one.uw_longest_hist, sh.uw_longest_hist) and np.array_equal(one.uw_current_hist, sh.uw_current_hist)
            assert np.array_equal(one.uw_sums, sh.uw_sums) and np.array_equal(one.uw_q, sh.uw_q)
            for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi", "cvar"):
                assert np.array_equal(one.stats[f], sh.stats[f]) and np.array_equal(one.dd_stats[f], sh.dd_stats[f]), f


def test_a_rejected_call_leaves_no_residue(gpu_ctx):
    N, K, T, n = 3, 3, 12, 5000
    mu, L, W = market(N, K)
    prm = _ffi.make_params(N, T, K)
    want = _run(gpu_ctx, prm, mu, L, W, 5, n)
    for bad_prm, kw in ((_ffi.make_params(N, T, K, native_math=True), {}), (prm, {"levels": (101.0,)}),
                        (_ffi.make_params(N, T, K, "log"), {"draw": "garch"})):
        with pytest.raises(_ffi.McpError):
            _run(gpu_ctx, bad_prm, mu, L, W, 5, n, **kw)
        got = _run(gpu_ctx, prm, mu, L, W, 5, n)
        assert np.array_equal(got.uw_longest_hist, want.uw_longest_hist) and np.array_equal(got.uw_current_hist, want.uw_current_hist)
        assert np.array_equal(got.uw_longest, want.uw_longest) and np.array_equal(got.uw_q, want.uw_q) and got.stats.tobytes() == want.stats.tobytes()


def test_the_two_laws_at_a_million_paths(gpu_ctx):
    """One asset, mu = 0, log compounding, T = 5, from the kernel's histograms: P(m = 0) = 2^-4 and P(c_T = 0) = 70 / 256
    (underwater.spell_law), each count within 5 binomial standard deviations."""
    T, n = 5, 1_000_000
    mu, L, W = np.zeros(1, np.float32), np.full((1, 1), 0.05, np.float32), np.ones((1, 1), np.float32)
    out = _run(gpu_ctx, _ffi.make_params(1, T, 1, "log"), mu, L, W, 0, n, store=False)
    print(ref_.law_checks(out.uw_longest_hist[0], out.uw_current_hist[0], T))


def test_public_call_blocks_and_portfolio_shards(gpu_ctx):
    """simulate_paths(drawdown=True, underwater=True): the 'underwater' block against the stored arrays, and two portfolio shards against
    one call."""
    N, K, T, n = 4, 3, 12, 20_000
    mu, L, W = market(N, K)
    kw = dict(n_steps=T, n_paths=n, seed=SEED, chol=L, drawdown=True, underwater=True, underwater_levels=(50, 95), store=True, dof=5)
    res = simulate_paths(mu, None, W, context=gpu_ctx, **kw)
    plain = simulate_paths(mu, None, W, n_steps=T, n_paths=n, seed=SEED, chol=L, drawdown=True, store=True, dof=5, context=gpu_ctx)
    for d, p in zip(res, plain):
        blk = d["underwater"]
        assert np.array_equal(d["terminal"], p["terminal"]) and np.array_equal(d["max_drawdown"], p["max_drawdown"]) and d["drawdown"] == p["drawdown"]
        for name in ("longest", "current"):
            steps = blk[name]["steps"]
            assert steps.shape == (n,) and steps.dtype == np.uint32 and blk[name]["hist"].shape == (T + 1,)
            assert np.array_equal(blk[name]["hist"], np.bincount(steps, minlength=T + 1).astype(np.uint64))
            assert blk[name]["mean"] == steps.astype(np.uint64).sum() / n
            assert blk[name]["levels"] == {q: int(np.percentile(steps, q, method="lower")) for q in (50.0, 95.0)}
        assert blk["p_under_water_at_end"] == 1.0 - np.count_nonzero(blk["current"]["steps"] == 0) / n and 0.0 < blk["p_under_water_at_end"] < 1.0
    c = Context((0, 0))
    try:
        two = simulate_paths(mu, None, W, context=c, devices=[0, 0], shard="portfolios", **kw)
    finally:
        c.close()
    for a, b in zip(res, two):
        assert np.array_equal(a["terminal"], b["terminal"]) and a["var"] == b["var"]
        for name in ("longest", "current"):
            assert np.array_equal(a["underwater"][name]["steps"], b["underwater"][name]["steps"])
            assert np.array_equal(a["underwater"][name]["hist"], b["underwater"][name]["hist"]) and a["underwater"][name]["levels"] == b["underwater"][name]["levels"]


def test_pipeline_prints_the_time_under_water(gpu_ctx):
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
    line = re.search(r"time under water: longest spell median (\d+) / 95 % (\d+) of (\d+) period\(s\), P\(under water at the end\) = ([0-9.]+)",
                     out.getvalue())
    assert line, out.getvalue()
    med, hi, af, p = int(line.group(1)), int(line.group(2)), int(line.group(3)), float(line.group(4))
    assert 0 <= med <= hi <= af - 1 and 0.0 <= p <= 1.0

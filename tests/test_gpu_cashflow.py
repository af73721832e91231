"""GPU checks of contributions, withdrawals and ruin (SPEC.md 4.7 / 5.6): terminal and horizon values bit-equal to the NumPy
restatement (cashflow_ref.py) for Gaussian, bootstrap (row table in LDS and in global memory) and Student-t draws over widths,
portfolio counts, step counts, schedules and a path range across 2^32; an all-zero schedule against the plain calls; V_h against
the T = h calls; the records and bands against NumPy on stored values with a large mass at zero; the counts; the shards, the
tiles and K = 20; the mean law without ruin; recovery after a rejected call; and the examples' lines."""
import contextlib
import ctypes
import io
import os
import runpy
import sys

import numpy as np
import pytest

from cashflow_ref import counts_of, simulate_cf
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, simulate_bootstrap, simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs
from oracle import ref_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xCA5_F10
VARIANTS = ["gauss", "boot_lds", "boot_global", "t"]
EXACT = ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max")
CLOSE = ("mean", "std", "sharpe", "cvar")


def _market(N, K, seed=0):
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(seed + 31 * N + K).dirichlet(np.ones(N), size=K)
    if K > 1:
        W[-1] *= 0.9                                     # 10 % cash in one portfolio
    return prepare_inputs(mu, cov, W)


def _draws(variant, N, mu, L):
    """The draw arguments of Context.simulate_cashflow / cashflow_ref.simulate_cf for a kernel variant.  The bootstrap's row table
    is read from LDS while R ceil(N/4) <= 1088 float4 slots and from global memory beyond."""
    if variant == "gauss":
        return {"mu": mu, "chol": L}
    if variant == "t":
        return {"mu": mu, "chol": L, "dof": 5}
    nb = (N + 3) // 4
    R = 40 if variant == "boot_lds" and 40 * nb <= 1088 else (1088 // nb if variant == "boot_lds" else 1088 // nb + 50)
    z = np.random.default_rng(7 * N + R).standard_normal((R, N))
    rows = (mu.astype(np.float64) + z @ L.astype(np.float64).T).astype(np.float32)
    return {"rows": np.ascontiguousarray(rows), "block": 3.0}


def _schedule(kind, T, v0=1.0):
    c = {"zero": np.zeros(T), "pay": np.full(T, 0.03), "take": np.full(T, -1.2 / max(T, 1)),
         "both": np.where(np.arange(T) % 2 == 0, 0.02, -0.06)}[kind]
    return (c * v0).astype(np.float32)


def _pick(n_paths, begin, count=12):
    ids = {0, 1, n_paths - 1, n_paths // 2}
    ids.update(np.linspace(0, n_paths - 1, count).astype(int).tolist())
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 3)))
    return np.array(sorted(ids), np.int64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _close(got, want, f):
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (f, got, want)


def _assert_numpy_record(rec, values, v0=1.0, alpha=0.95, rf=0.0, sharpe=True):
    want = ref_stats.path_stats(values, v0=v0, alpha=alpha, rf=rf)
    x = x_of(values, v0=v0)
    assert rec["n"] == values.size and rec["var"] == want["var"] == np.percentile(x, (1 - alpha) * 100)
    assert rec["n_tail"] == want["n_tail"] and rec["min"] == want["min"] and rec["max"] == want["max"]
    for f in ("mean", "std", "cvar") + (("sharpe",) if sharpe else ()):
        _close(rec[f], want[f], f)
    return want


CASES = [  # N, K, T, path_begin, n_paths, schedule, v0
    (1, 1, 7, 0, 3000, "take", 1.0),
    (3, 3, 60, (1 << 32) - 1500, 3000, "both", 1.0),
    (13, 8, 1, 17, 5000, "pay", 100.0),
    (16, 1, 60, 0, 4096, "both", 1.0),
    (16, 20, 0, 0, 1000, "zero", 1.0),
    (17, 20, 7, 5, 2000, "take", 250.0),
    (64, 3, 7, (1 << 32) - 7, 300, "zero", 1.0),
    (3, 8, 60, 0, 2000, "zero", 1.0),
    (16, 3, 60, 9, 2000, "take", 1.0),
]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N,K,T,begin,n,kind,v0", CASES)
def test_values_equal_the_restatement(N, K, T, begin, n, kind, v0, variant, gpu_ctx):
    mu, L, W = _market(N, K, T)
    draws = _draws(variant, N, mu, L)
    flows = _schedule(kind, T, v0)
    hz = sorted({1, max(1, T // 2), T}) if T >= 1 else None
    prm = _ffi.make_params(N, T, K, v0=v0)
    out = gpu_ctx.simulate_cashflow(prm, flows, W, SEED, begin, n, True, horizons=hz, levels=(50.0,) if hz else (), target=0.5 * v0,
                                    **draws)
    ids = _pick(n, begin, 6 if N >= 16 and T > 7 else 12)
    ref = simulate_cf(flows, W, T, SEED, (begin + ids).astype(np.uint64), v0=v0, horizons=hz or (), **draws)
    assert np.array_equal(_bits(out.terminal[:, ids]), _bits(ref["V_T"]))
    if hz:
        assert np.array_equal(_bits(out.horizon_terminal[:, :, ids]), _bits(ref["V_h"]))
        assert np.array_equal(_bits(out.horizon_terminal[-1]), _bits(out.terminal))
        assert np.array_equal(out.hz_counts, counts_of(out.horizon_terminal, 0.5 * v0))
    else:
        assert out.hz_counts is None and np.all(out.terminal == np.float32(v0))
    assert np.array_equal(out.counts, counts_of(out.terminal, 0.5 * v0))
    assert not np.any(np.signbit(out.terminal)) and not np.any(np.isnan(out.terminal))     # every stored value is +0 or > 0
    if kind == "take" and T >= 7:
        assert out.counts[:, 0].sum() > 0                                                  # the case does ruin paths
    for k in (0, K - 1):
        _assert_numpy_record(out.stats[k], out.terminal[k], v0=v0)


@pytest.mark.parametrize("variant", ["gauss", "boot_lds", "t"])
@pytest.mark.parametrize("N,K", [(3, 1), (16, 3), (5, 20)])
def test_zero_schedule_is_the_plain_call(N, K, variant, gpu_ctx):
    T, n, hz, lv = 24, 20_000, [1, 5, 12, 24], (2.5, 50.0, 97.5)
    mu, L, W = _market(N, K, 5)
    draws = _draws(variant, N, mu, L)
    prm = _ffi.make_params(N, T, K, v0=50.0, rf=0.01)
    got = gpu_ctx.simulate_cashflow(prm, np.zeros(T, np.float32), W, SEED, 3, n, True, horizons=hz, levels=lv, target=50.0, **draws)
    if variant == "t":
        want = gpu_ctx._call(prm, W, SEED, 3, n, True, mu=mu, chol=L, dof=5, horizons=np.asarray(hz, np.int32), levels=lv)
    elif variant == "gauss":
        want = gpu_ctx._call(prm, W, SEED, 3, n, True, mu=mu, chol=L, horizons=np.asarray(hz, np.int32), levels=lv)
    else:
        want = gpu_ctx._call(prm, W, SEED, 3, n, True, rows=draws["rows"], block=draws["block"], horizons=np.asarray(hz, np.int32),
                             levels=lv)
    assert np.array_equal(_bits(got.terminal), _bits(want.terminal))
    assert np.array_equal(_bits(got.horizon_terminal), _bits(want.horizon_terminal))
    assert np.array_equal(got.bands, want.bands)
    for g, w in ((got.stats, want.stats), (got.hz_stats, want.hz_stats)):
        for f in EXACT:
            assert np.array_equal(g[f], w[f]), f
        for f in CLOSE:
            assert np.all(np.abs(g[f] - w[f]) <= 1e-12 * np.maximum(1.0, np.abs(w[f]))), f
    assert np.all(got.counts[:, 0] == 0) and np.all(got.hz_counts[:, :, 0] == 0)
    assert np.array_equal(got.counts, counts_of(got.terminal, 50.0)) and got.counts[:, 1].sum() > 0
    # without horizons the same kernel walks one segment: the same terminal values and records
    solo = gpu_ctx.simulate_cashflow(prm, np.zeros(T, np.float32), W, SEED, 3, n, True, **draws)
    assert np.array_equal(_bits(solo.terminal), _bits(want.terminal)) and solo.stats.tobytes() == got.stats.tobytes()
    assert solo.hz_stats is None and solo.hz_counts is None and np.all(solo.counts == 0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_horizon_rows_are_the_truncated_calls(variant, gpu_ctx):
    N, K, T, n, hz = 16, 3, 30, 10_000, [1, 7, 18, 30]
    mu, L, W = _market(N, K, 2)
    draws = _draws(variant, N, mu, L)
    flows = np.r_[np.where(np.arange(20) % 2 == 0, 0.02, -0.1), np.full(10, -0.03)].astype(np.float32)   # 1.1 taken out in all
    full = gpu_ctx.simulate_cashflow(_ffi.make_params(N, T, K), flows, W, SEED, 11, n, True, horizons=hz, levels=(5.0, 95.0), **draws)
    assert full.counts[0, 0] > 0 and full.hz_counts[1, 0, 0] == 0    # ruin sets in between the horizons
    for i, h in enumerate(hz):
        part = gpu_ctx.simulate_cashflow(_ffi.make_params(N, h, K), flows[:h].copy(), W, SEED, 11, n, True, **draws)
        assert np.array_equal(_bits(full.horizon_terminal[i]), _bits(part.terminal))
        assert np.array_equal(full.hz_counts[i], part.counts)
        for f in EXACT:
            assert np.array_equal(full.hz_stats[i][f], part.stats[f]), (h, f)
        for f in ("mean", "std", "cvar"):
            assert np.all(np.abs(full.hz_stats[i][f] - part.stats[f]) <= 1e-12 * np.maximum(1.0, np.abs(part.stats[f]))), (h, f)


def test_records_and_bands_with_a_mass_at_zero(gpu_ctx):
    """synthetic_market(3), equal weights, v0 = 1, T = 60, 0.0165 taken out per step: close to half of the paths are ruined at T
    (VaR, x_lo, x_hi and CVaR sit on the ties at x = -1) and a few at h = 48 (ties at the bottom of the tail)."""
    n, T, hz, lv = 200_001, 60, [12, 24, 36, 48, 60], (1.0, 5.0, 25.0, 50.0, 75.0, 99.0)
    mu, cov = synthetic.synthetic_market(3)
    d = simulate_paths(mu, cov, np.ones(3) / 3, n_steps=T, n_paths=n, seed=SEED, cashflow=-0.0165, target=0.25, horizons=hz, bands=lv,
                       store=True, context=gpu_ctx)
    term, hterm = d["terminal"], d["horizon_terminal"]
    share_T = np.count_nonzero(term == 0) / n
    share_48 = np.count_nonzero(hterm[3] == 0) / n
    print(f"ruined share at T: {share_T:.4f}, at h = 48: {share_48:.5f}")
    assert 0.2 < share_T < 0.8 and 0.0 < share_48 < 0.05             # the shares this test relies on
    want = _assert_numpy_record(d, term)
    assert d["var"] == d["x_lo"] == d["x_hi"] == -1.0 and abs(d["cvar"] + 1.0) <= 1e-12
    assert d["n_tail"] == want["n_tail"] == d["cashflow"]["n_ruined"] == np.count_nonzero(term == 0) and d["min"] == -1.0
    assert d["cashflow"]["ruin_probability"] == d["cashflow"]["n_ruined"] / n
    assert d["cashflow"]["n_short"] == np.count_nonzero(term < np.float32(0.25))
    assert d["cashflow"]["shortfall_probability"] == d["cashflow"]["n_short"] / n
    assert d["cashflow"]["contributed"] == float(np.float64(np.float32(-0.0165)) * T)
    h = d["horizons"]
    for i in range(len(hz)):
        x = x_of(hterm[i])
        rec = {f: h[f][i] for f in ("mean", "std", "var", "cvar", "min", "max", "n_tail")}
        rec["n"] = n
        _assert_numpy_record(rec, hterm[i], sharpe=False)
        for j, q in enumerate(lv):
            assert h["bands"][i, j] == np.percentile(x, q), (hz[i], q)
        assert h["n_ruined"][i] == np.count_nonzero(hterm[i] == 0) and h["ruin_probability"][i] == h["n_ruined"][i] / n
        assert h["n_short"][i] == np.count_nonzero(hterm[i] < np.float32(0.25))
    assert np.all(np.diff(h["n_ruined"]) >= 0) and h["n_ruined"][-1] == d["cashflow"]["n_ruined"]
    assert np.all(h["n_short"] >= h["n_ruined"])
    assert h["bands"][-1, 0] == h["bands"][-1, 2] == -1.0 and h["bands"][-1, 4] > -1.0    # 1 % .. 25 % of x_T are the ties
    # an alpha whose rank falls in the ties at h = 48 (0 < share < 1 - alpha is not given there: take the rank from the share)
    a48 = 1.0 - share_48 / 2
    d2 = simulate_paths(mu, cov, np.ones(3) / 3, n_steps=48, n_paths=n, seed=SEED, cashflow=-0.0165, alpha=a48, store=True, context=gpu_ctx)
    assert np.array_equal(_bits(d2["terminal"]), _bits(hterm[3]))
    _assert_numpy_record(d2, d2["terminal"], alpha=a48)
    assert d2["var"] == -1.0 and d2["n_tail"] == np.count_nonzero(hterm[3] == 0)


def test_less_is_ruined_when_less_is_taken(gpu_ctx):
    mu, cov = synthetic.synthetic_market(3)
    kw = dict(n_steps=60, n_paths=200_001, seed=SEED, context=gpu_ctx)
    lo = simulate_paths(mu, cov, np.ones(3) / 3, cashflow=-0.015, **kw)["cashflow"]
    hi = simulate_paths(mu, cov, np.ones(3) / 3, cashflow=-0.0165, **kw)["cashflow"]
    assert 0 < lo["n_ruined"] < hi["n_ruined"] and "n_short" not in lo


@pytest.mark.parametrize("variant", ["gauss", "boot_global", "t"])
def test_shards_tiles_and_twenty_portfolios(variant, gpu_ctx):
    N, K, T, n, hz, lv = 16, 20, 30, 30_001, [10, 20, 30], (50.0,)
    mu, L, W = _market(N, K, 9)
    draws = _draws(variant, N, mu, L)
    flows = np.full(T, -1.0 / T, np.float32)             # the initial value taken out in all: the noise decides who is ruined
    prm = _ffi.make_params(N, T, K)
    one = gpu_ctx.simulate_cashflow(prm, flows, W, SEED, 11, n, True, horizons=hz, levels=lv, target=0.4, **draws)
    assert np.array_equal(one.counts, counts_of(one.terminal, 0.4)) and np.array_equal(one.hz_counts, counts_of(one.horizon_terminal, 0.4))
    assert np.all(np.diff(one.hz_counts[:, :, 0].astype(np.int64), axis=0) >= 0) and 0 < one.counts[0, 0] < n
    assert np.all((one.horizon_terminal == 0) | (one.horizon_terminal > 0)) and not np.any(np.signbit(one.horizon_terminal))
    others = []
    c = Context((0, 0))
    try:
        others.append(c.simulate_cashflow(prm, flows, W, SEED, 11, n, True, horizons=hz, levels=lv, target=0.4, **draws))
        others.append(c.simulate_cashflow(_ffi.make_params(N, T, K, shard_portfolios=True), flows, W, SEED, 11, n, True, horizons=hz,
                                          levels=lv, target=0.4, **draws))
    finally:
        c.close()
    c = Context(0, terminal_budget=3 * 4 * n * 4)        # tiles of 3 portfolios (4 rows of n binary32 values each)
    try:
        others.append(c.simulate_cashflow(prm, flows, W, SEED, 11, n, True, horizons=hz, levels=lv, target=0.4, **draws))
    finally:
        c.close()
    for o in others:
        assert np.array_equal(_bits(one.terminal), _bits(o.terminal)) and np.array_equal(_bits(one.horizon_terminal), _bits(o.horizon_terminal))
        assert np.array_equal(one.counts, o.counts) and np.array_equal(one.hz_counts, o.hz_counts) and np.array_equal(one.bands, o.bands)
        for g, w in ((o.stats, one.stats), (o.hz_stats, one.hz_stats)):
            for f in EXACT:
                assert np.array_equal(g[f], w[f]), f
            for f in ("mean", "std", "cvar"):
                assert np.all(np.abs(g[f] - w[f]) <= 1e-12 * np.maximum(1.0, np.abs(w[f]))), f


@pytest.mark.parametrize("dof", [None, 5])
def test_mean_is_the_pivot_without_ruin(dof, gpu_ctx):
    n, N, K, T = 1_000_000, 8, 2, 12
    mu, L, W = _market(N, K, 1)
    flows = np.linspace(0.01, 0.05, T).astype(np.float32)             # contributions only: no path is ruined
    prm = _ffi.make_params(N, T, K)
    out = gpu_ctx.simulate_cashflow(prm, flows, W, SEED, 0, n, True, mu=mu, chol=L, dof=dof)
    piv = _ffi.cashflow_pivots(prm, flows, W, mu=mu)
    assert np.all(out.counts == 0) and np.all(out.terminal > 0)
    for k in range(K):
        std = x_of(out.terminal[k]).std(ddof=1)
        print(f"dof {dof} k {k}: mean {out.stats[k]['mean']:.9f} pivot {piv[k]:.9f} 5 se {5 * std / np.sqrt(n):.3e}")
        assert abs(out.stats[k]["mean"] - piv[k]) < 5 * std / np.sqrt(n), (out.stats[k]["mean"], piv[k])


def test_rejected_call_then_a_correct_one_then_a_plain_call(gpu_ctx):
    mu, L, W = _market(16, 3, 1)
    prm = _ffi.make_params(16, 40, 3)
    flows = _schedule("take", 40)
    g0, gt0 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    fresh = Context(0)
    try:
        want = fresh.simulate_cashflow(prm, flows, W, SEED, 0, 50_000, True, mu=mu, chol=L)
    finally:
        fresh.close()
    bad = flows.copy()
    bad[7] = np.nan
    for f in (bad, flows[:39].copy()):
        with pytest.raises(_ffi.McpError, match="cash flow 8 is not finite|n_flows"):
            gpu_ctx.simulate_cashflow(prm, f, W, SEED, 0, 50_000, True, mu=mu, chol=L)
    with pytest.raises(_ffi.McpError, match="compound simply"):
        gpu_ctx.simulate_cashflow(_ffi.make_params(16, 40, 3, compounding="log"), flows, W, SEED, 0, 1000, False, mu=mu, chol=L)
    fn = _ffi.lib().mcp_simulate_cashflow
    st = np.zeros(3, _ffi.STATS_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    cf = _ffi.make_cashflow(flows)
    assert fn(gpu_ctx._h, ctypes.byref(prm), ctypes.byref(cf), vp(mu), vp(L), None, None, vp(W), SEED, 0, 50_000, 0, None, 0, None, None,
              vp(st), None, None, None, None, None) == _ffi.MCP_E_ARG               # counts_out is NULL
    got = gpu_ctx.simulate_cashflow(prm, flows, W, SEED, 0, 50_000, True, mu=mu, chol=L)
    assert np.array_equal(want.terminal, got.terminal) and want.stats.tobytes() == got.stats.tobytes()
    assert np.array_equal(want.counts, got.counts) and got.counts[0, 0] > 0
    g1, gt1 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    assert np.array_equal(gt0, gt1) and g0.tobytes() == g1.tobytes()


def test_simulate_paths_and_bootstrap_return_their_shapes(gpu_ctx):
    mu, cov = synthetic.synthetic_market(3)
    one = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, cashflow=-0.05, store=True, horizons=[1, 6, 12],
                         bands=(5.0, 95.0), context=gpu_ctx)
    assert one["n"] == 5000 and one["terminal"].shape == (5000,) and one["horizons"]["bands"].shape == (3, 2)
    assert set(one["cashflow"]) == {"contributed", "n_ruined", "ruin_probability"} and one["horizons"]["n_ruined"].shape == (3,)
    assert "n_short" not in one["horizons"] and one["horizons"]["ruin_probability"].dtype == np.float64
    sched = np.r_[np.full(6, 0.1), np.full(6, -0.2)]
    many = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, cashflow=sched, target=1.0, dof=4, context=gpu_ctx)
    assert isinstance(many, list) and len(many) == 3 and "horizons" not in many[0]
    assert abs(many[0]["cashflow"]["contributed"] - float(np.sum(sched.astype(np.float32).astype(np.float64)))) == 0.0
    assert 0.0 <= many[0]["cashflow"]["shortfall_probability"] <= 1.0 and isinstance(many[0]["cashflow"]["n_short"], int)
    arr = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, cashflow=0, as_array=True, context=gpu_ctx)
    plain = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, as_array=True, context=gpu_ctx)
    assert isinstance(arr, tuple) and len(arr) == 2 and arr[1].shape == (3, 2) and arr[1].dtype == np.uint64 and not arr[1].any()
    assert np.array_equal(arr[0]["var"], plain["var"]) and np.array_equal(arr[0]["n_tail"], plain["n_tail"])
    s, t, c = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, cashflow=-0.05, as_array=True, store=True, context=gpu_ctx)
    assert t.shape == (3, 5000) and np.array_equal(c, counts_of(t))
    got = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, cashflow=-0.05, target=0.5, as_array=True, store=True,
                         horizons=[6, 12], bands=(50.0,), context=gpu_ctx)
    assert len(got) == 7 and got[5].shape == (3, 2) and got[6].shape == (2, 3, 2) and np.array_equal(got[6], counts_of(got[4], 0.5))
    rows = np.random.default_rng(5).normal(0.002, 0.03, size=(120, 3))
    b = simulate_bootstrap(rows, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, block=4.0, cashflow=-0.08, target=0.3, store=True,
                           horizons=[6, 12], context=gpu_ctx)
    assert b["cashflow"]["n_ruined"] == np.count_nonzero(b["terminal"] == 0) and b["horizons"]["n_short"].shape == (2,)
    assert b["horizons"]["n_ruined"][-1] == b["cashflow"]["n_ruined"]


def test_pipeline_prints_the_withdrawal_lines(gpu_ctx):
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
    assert "withdrawal plan" in text and "ruin probability at the end" in text and text.count("ruined after") == 3
    assert text.count("forecast fan after") == 3 and text.count("Student-t fan after") == 3


def test_streamlit_forecast_tab_shows_the_ruin_probabilities(gpu_ctx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_shim import fake_streamlit
    record = []
    sys.modules["streamlit"] = fake_streamlit(record, 50_000)
    try:
        np.random.seed(4242)
        runpy.run_path(os.path.join(ROOT, "examples", "streamlit_app.py"), run_name="__main__")
    finally:
        del sys.modules["streamlit"]
    plans = [r[1][0] for r in record if r[0] == "write" and isinstance(r[1][0], dict) and "ruin probability per horizon" in r[1][0]]
    assert len(plans) == 1
    ruin = plans[0]["ruin probability per horizon"]
    assert len(ruin) >= 1 and all(0.0 <= float(v) <= 1.0 for v in ruin.values())
    assert list(ruin.values()) == sorted(ruin.values()) and "shortfall probability at the end" in plans[0]

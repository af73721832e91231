"""GPU checks of the risk attribution (SPEC.md 4.10 / 5.9): the stored contributions bit-equal to the NumPy restatement
(attribution_ref.py) on every path of every shape; statistics and terminal values bit-identical to the call without attribution;
the counts of the second walk equal to the statistics' own; the sums against NumPy binary64 on the stored device contributions; the
three identities inside the bounds of SPEC.md 6; a zero weight; the shards; the one-step law at 10^6 paths; every rejected
combination, recovery after it, and the examples' lines."""
import contextlib
import ctypes
import functools
import io
import os
import runpy
import sys

import numpy as np
import pytest

import attribution_ref as ar
from monte_carlo_portfolio_amd import _ffi, simulate_bootstrap, simulate_paths, simulate_sweep
from monte_carlo_portfolio_amd.simulate import Context, default_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = range(len(ar.CASES))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _prm(idx, alpha=ar.ALPHA):
    N, _, _, K, T, _, _ = ar.CASES[idx]
    return _ffi.make_params(N, T, K, alpha=alpha)


@functools.lru_cache(maxsize=None)
def _dev(idx):
    """The attribution call of CASES[idx] on the default context, with everything stored: run once, shared by the tests."""
    _, dof, garch, _, _, begin, n = ar.CASES[idx]
    ref = ar.case_ref(idx)
    return default_context(0).simulate_attribution(_prm(idx), ref["mu"], ref["L"], ref["W"], ar.SEED, begin, n, True, dof=dof, garch=garch)


def _plain(ctx, idx, prm=None):
    """(stats, terminal) of the same call without attribution."""
    _, dof, garch, _, _, begin, n = ar.CASES[idx]
    ref = ar.case_ref(idx)
    prm = prm or _prm(idx)
    if garch is not None:
        o = ctx.simulate_garch(prm, garch, ref["mu"], ref["L"], ref["W"], ar.SEED, begin, n, True, dof=dof)
        return o.stats, o.terminal
    if dof is not None:
        o = ctx.simulate_student_t(prm, dof, ref["mu"], ref["L"], ref["W"], ar.SEED, begin, n, True)
        return o[0], o[4]
    return ctx.simulate(prm, ref["mu"], ref["L"], ref["W"], ar.SEED, begin, n, True)


# 1. stored values
@pytest.mark.parametrize("idx", IDX, ids=ar.CASE_IDS)
def test_stored_contributions_equal_the_restatement_on_every_path(idx, gpu_ctx):
    N, _, _, K, _, _, n = ar.CASES[idx]
    got, ref = _dev(idx), ar.case_ref(idx)
    assert got.contributions.shape == (K, N, n) and got.contributions.dtype == np.float32
    diff = _bits(got.contributions) != _bits(ref["A"])
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5])
    assert np.array_equal(_bits(got.terminal), _bits(ref["V_T"]))


# 2. anchor
@pytest.mark.parametrize("idx", IDX, ids=ar.CASE_IDS)
def test_statistics_and_terminal_values_are_those_of_the_call_without_attribution(idx, gpu_ctx):
    got = _dev(idx)
    st, term = _plain(gpu_ctx, idx)
    assert got.stats.tobytes() == st.tobytes()
    assert np.array_equal(_bits(got.terminal), _bits(term))
    _, dof, garch, _, _, begin, n = ar.CASES[idx]
    ref = ar.case_ref(idx)
    lean = gpu_ctx.simulate_attribution(_prm(idx), ref["mu"], ref["L"], ref["W"], ar.SEED, begin, n, False, dof=dof, garch=garch)
    assert lean.terminal is None and lean.contributions is None
    assert lean.stats.tobytes() == st.tobytes() and lean.attr.tobytes() == got.attr.tobytes()      # run-to-run deterministic
    assert np.array_equal(lean.attr_counts, got.attr_counts)


# 3. counts
@pytest.mark.parametrize("idx", IDX, ids=ar.CASE_IDS)
def test_counts_equal_the_statistics_own(idx, gpu_ctx):
    got = _dev(idx)
    n = ar.CASES[idx][6]
    assert np.array_equal(got.attr_counts[:, 0], got.stats["n"]) and np.all(got.attr_counts[:, 0] == n)
    assert np.array_equal(got.attr_counts[:, 1], got.stats["n_tail"])
    if ar.CASES[idx][4] == 0:                          # T = 0: every terminal value ties at the VaR, every path is in the tail
        assert np.all(got.attr_counts[:, 1] == n) and np.all(got.stats["var"] == 0.0)


@pytest.mark.parametrize("idx", [1, 2, 7], ids=[ar.CASE_IDS[i] for i in (1, 2, 7)])
def test_a_tail_of_a_single_path(idx, gpu_ctx):
    """alpha = 1 - 1 / (2 n): the percentile falls between the two lowest order statistics."""
    _, dof, garch, K, _, begin, n = ar.CASES[idx]
    ref = ar.case_ref(idx)
    prm = _prm(idx, alpha=1.0 - 0.5 / n)
    got = gpu_ctx.simulate_attribution(prm, ref["mu"], ref["L"], ref["W"], ar.SEED, begin, n, True, dof=dof, garch=garch)
    assert np.all(got.stats["n_tail"] == 1) and np.array_equal(got.attr_counts[:, 1], got.stats["n_tail"])
    for k in range(K):
        worst = int(np.argmin(got.terminal[k]))
        assert np.array_equal(got.attr["sum_tail"][k], got.contributions[k, :, worst].astype(np.float64))
        assert np.array_equal(got.attr["cvar"][k], got.attr["sum_tail"][k] / 1.0)            # v0 = 1, n_tail = 1


# 4. sums
@pytest.mark.parametrize("idx", IDX, ids=ar.CASE_IDS)
def test_sums_against_numpy_on_the_stored_contributions(idx, gpu_ctx):
    N, _, _, K, _, _, n = ar.CASES[idx]
    got, ref = _dev(idx), ar.case_ref(idx)
    c = _ffi.pivots(_prm(idx), ref["mu"], ref["L"], ref["W"])
    for k in range(K):
        A = got.contributions[k].astype(np.float64)
        x = got.terminal[k].astype(np.float64) / 1.0 - 1.0
        tail = x <= got.stats["var"][k]
        d = x - c[k]
        assert int(tail.sum()) == int(got.stats["n_tail"][k])
        want = {"sum": A.sum(axis=1), "sum_tail": A[:, tail].sum(axis=1), "sum_xc": (A * d).sum(axis=1)}
        scale = {"sum": np.abs(A).sum(axis=1), "sum_tail": np.abs(A[:, tail]).sum(axis=1), "sum_xc": np.abs(A * d).sum(axis=1)}
        for f in want:                                 # association only (SPEC.md 6)
            err = np.abs(got.attr[f][k] - want[f])
            print(f"{ar.CASE_IDS[idx]} k={k} {f}: worst |error| / sum |summand| = {np.max(err / np.maximum(scale[f], 1e-300)):.2e}")
            assert np.all(err <= 1e-12 * scale[f]), (f, k, err, scale[f])
        # mean, cvar and vol are the formulas of SPEC.md 5.9 on those sums (v0 = 1)
        n_tail, sd = float(got.stats["n_tail"][k]), float(got.stats["std"][k])
        assert np.array_equal(got.attr["mean"][k], got.attr["sum"][k] / (1.0 * n))
        assert np.array_equal(got.attr["cvar"][k], got.attr["sum_tail"][k] / (1.0 * n_tail))
        if sd > 0:
            S1 = float(d.sum())
            vol = (got.attr["sum_xc"][k] - got.attr["sum"][k] * S1 / n) / (1.0 * (n - 1.0)) / sd
            tol = 1e-12 * (scale["sum_xc"] + scale["sum"] * np.abs(d).sum() / n) / ((n - 1.0) * sd)
            assert np.all(np.abs(got.attr["vol"][k] - vol) <= tol), (k, got.attr["vol"][k], vol)
        else:
            assert not got.attr["vol"][k].any()


# 5. residual
@pytest.mark.parametrize("idx", IDX, ids=ar.CASE_IDS)
def test_the_three_residuals_lie_inside_their_bounds(idx, gpu_ctx):
    K = ar.CASES[idx][3]
    got, ref = _dev(idx), ar.case_ref(idx)
    for k in range(K):
        x = got.terminal[k].astype(np.float64) - 1.0
        lim = ar.identity_bounds(ref["residual"][k], ref["bound"][k], x <= got.stats["var"][k])
        res = {"mean": got.stats["mean"][k] - got.attr["mean"][k].sum(), "cvar": got.stats["cvar"][k] - got.attr["cvar"][k].sum(),
               "vol": got.stats["std"][k] - got.attr["vol"][k].sum()}
        print(f"{ar.CASE_IDS[idx]} k={k}: " + ", ".join(f"{f} {res[f]:+.3e} (bound {lim[f]:.3e})" for f in res))
        for f in res:
            assert abs(res[f]) <= lim[f], (f, k, res[f], lim[f])


# 6. zero weight
def test_an_asset_with_weight_zero_reports_zero(gpu_ctx):
    seen = 0
    for idx, c in enumerate(ar.CASES):
        if c[0] > 2:
            got, ref = _dev(idx), ar.case_ref(idx)
            assert ref["W"][0, 1] == 0
            rec = got.attr[0, 1]
            assert rec["mean"] == 0 and rec["cvar"] == 0 and rec["vol"] == 0 and rec["sum"] == 0 and rec["sum_xc"] == 0
            assert not _bits(got.contributions[0, 1]).any()
            seen += 1
    assert seen >= 6


# 7. shards
@pytest.fixture(scope="module")
def two_shards():
    ctx = Context((0, 0))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("idx", [1, 2, 4, 7, 8], ids=[ar.CASE_IDS[i] for i in (1, 2, 4, 7, 8)])
def test_two_shards_against_one(idx, two_shards, gpu_ctx):
    _, dof, garch, K, _, begin, n = ar.CASES[idx]
    ref, one = ar.case_ref(idx), _dev(idx)
    two = two_shards.simulate_attribution(_prm(idx), ref["mu"], ref["L"], ref["W"], ar.SEED, begin, n, True, dof=dof, garch=garch)
    assert np.array_equal(two.attr_counts, one.attr_counts)
    assert np.array_equal(_bits(two.contributions), _bits(one.contributions))
    assert np.array_equal(_bits(two.terminal), _bits(one.terminal))
    c = _ffi.pivots(_prm(idx), ref["mu"], ref["L"], ref["W"])
    for k in range(K):
        A = one.contributions[k].astype(np.float64)
        x = one.terminal[k].astype(np.float64) - 1.0
        tail = x <= one.stats["var"][k]
        scale = {"sum": np.abs(A).sum(axis=1), "sum_tail": np.abs(A[:, tail]).sum(axis=1), "sum_xc": np.abs(A * (x - c[k])).sum(axis=1)}
        for f in scale:
            assert np.all(np.abs(two.attr[f][k] - one.attr[f][k]) <= 1e-12 * scale[f]), (f, k)


# 8. the one-step law
def test_one_step_law_at_a_million_paths(gpu_ctx):
    mu, cov, w = ar.law_market()
    d = simulate_paths(mu, cov, w, n_steps=1, n_paths=ar.LAW_PATHS, seed=ar.SEED, store=True, attribution=True, context=gpu_ctx)
    at = d["attribution"]
    assert d["contributions"].shape == (ar.LAW_N, ar.LAW_PATHS) and at["n_tail"] == d["n_tail"]
    x = d["terminal"].astype(np.float64) - 1.0
    print(ar.law_checks(d["contributions"], x, at["mean"], at["cvar"], at["vol"], d["mean"], d["cvar"], x <= d["var"], w, cov))
    assert abs(at["cvar_share"].sum() - 1.0) < 1e-12 and abs(at["vol_share"].sum() - 1.0) < 1e-12


# the public surface on top of the record arrays
def test_simulate_paths_blocks_and_as_array(gpu_ctx):
    idx = 2
    N, dof, garch, K, T, begin, n = ar.CASES[idx]
    ref, raw = ar.case_ref(idx), _dev(idx)
    kw = dict(n_steps=T, n_paths=n, seed=ar.SEED, path_begin=begin, chol=ref["L"], garch=garch, dof=dof, context=gpu_ctx, attribution=True)
    res = simulate_paths(ref["mu"], None, ref["W"], store=True, **kw)
    assert isinstance(res, list) and len(res) == K
    for k, d in enumerate(res):
        at = d["attribution"]
        assert sorted(at) == ["cvar", "cvar_share", "mean", "n_tail", "residual", "vol", "vol_share"]
        for f in ("mean", "cvar", "vol"):
            assert at[f].dtype == np.float64 and np.array_equal(at[f], raw.attr[f][k])
            assert at["residual"][f] == float(raw.stats["std" if f == "vol" else f][k]) - float(raw.attr[f][k].sum())
        assert np.array_equal(at["cvar_share"], at["cvar"] / at["cvar"].sum()) and at["n_tail"] == int(raw.stats["n_tail"][k])
        assert np.array_equal(_bits(d["contributions"]), _bits(raw.contributions[k])) and d["contributions"].shape == (N, n)
        assert np.array_equal(_bits(d["terminal"]), _bits(raw.terminal[k]))
    stats, term, attr, counts, contrib = simulate_paths(ref["mu"], None, ref["W"], store=True, as_array=True, **kw)
    assert attr.tobytes() == raw.attr.tobytes() and np.array_equal(counts, raw.attr_counts) and contrib.shape == (K, N, n)
    assert stats.tobytes() == raw.stats.tobytes() and term.shape == (K, n)
    lean = simulate_paths(ref["mu"], None, ref["W"], as_array=True, **kw)
    assert len(lean) == 3 and lean[1].tobytes() == raw.attr.tobytes()
    one = simulate_paths(ref["mu"], None, ref["W"][0], **kw)
    assert isinstance(one, dict) and "contributions" not in one and np.array_equal(one["attribution"]["vol"], raw.attr["vol"][0])
    shard = simulate_paths(ref["mu"], None, ref["W"], devices=[0, 0], as_array=True, **{**kw, "context": None})
    assert np.array_equal(shard[2], raw.attr_counts)


# 9. errors
def _raw_call(ctx, prm, ref, n, **kw):
    K, N = prm.n_portfolios, prm.n_assets
    st, at, cn = np.zeros(K, _ffi.STATS_DTYPE), np.zeros((K, N), _ffi.ATTR_DTYPE), np.zeros((K, 2), np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    gv, stt = kw.get("gv"), kw.get("st")
    return _ffi.lib().mcp_simulate_attribution(ctx._h, ctypes.byref(prm), ctypes.byref(gv) if gv is not None else None,
                                               ctypes.byref(stt) if stt is not None else None, vp(ref["mu"]), vp(ref["L"]), vp(ref["W"]),
                                               ar.SEED, 0, n, None, vp(st), None, vp(at) if kw.get("attr", True) else None,
                                               vp(cn) if kw.get("counts", True) else None)


def test_every_rejected_combination_returns_its_error_and_the_context_works_on(gpu_ctx):
    idx = 3
    N, _, _, K, T, begin, n = ar.CASES[idx]
    ref = ar.case_ref(idx)
    lib = _ffi.lib()
    for flags, code, what in (({"compounding": "log"}, _ffi.MCP_E_UNSUPPORTED, b"compounds simply"),
                              ({"fold": True}, _ffi.MCP_E_UNSUPPORTED, b"MCP_FLAG_FOLD"),
                              ({"native_math": True}, _ffi.MCP_E_UNSUPPORTED, b"MCP_FLAG_NATIVE_MATH"),
                              ({"shard_portfolios": True}, _ffi.MCP_E_UNSUPPORTED, b"MCP_FLAG_SHARD_PORTFOLIOS")):
        assert _raw_call(gpu_ctx, _ffi.make_params(N, T, K, **flags), ref, n) == code and what in lib.mcp_last_error()
    prm = _prm(idx)
    assert _raw_call(gpu_ctx, prm, ref, n, attr=False) == _ffi.MCP_E_ARG and b"attr_out" in lib.mcp_last_error()
    assert _raw_call(gpu_ctx, prm, ref, n, counts=False) == _ffi.MCP_E_ARG and b"attr_counts_out" in lib.mcp_last_error()
    assert _raw_call(gpu_ctx, prm, ref, n, st=_ffi.McpStudentT(2, 0)) == _ffi.MCP_E_ARG
    assert _raw_call(gpu_ctx, prm, ref, n, gv=_ffi.McpGarch(0.6, 0.6, 1.0, 0)) == _ffi.MCP_E_ARG
    W17 = {"mu": ref["mu"], "L": ref["L"], "W": np.ascontiguousarray(np.repeat(ref["W"], 17, axis=0))}
    assert _raw_call(gpu_ctx, _ffi.make_params(N, T, 17), W17, n) == _ffi.MCP_E_UNSUPPORTED and b"at most 16" in lib.mcp_last_error()
    mu, cov, w = ar.law_market()
    for kw in ({"drawdown": True}, {"horizons": [1]}, {"rebalance": 2}, {"cashflow": 1.0}, {"fold": True}, {"native_math": True},
               {"compounding": "log"}, {"shard": "portfolios"}, {"overlay": {0: [("Stock", 0.0, 0.0, 1.0)]}, "spot": [1.0] * 3}):
        with pytest.raises(ValueError, match="attribution needs"):
            simulate_paths(mu, cov, w, n_steps=2, n_paths=64, attribution=True, context=gpu_ctx, **kw)
    with pytest.raises(ValueError, match="call simulate_paths for the optimum"):
        simulate_sweep(mu, cov, weights=np.eye(3), n_steps=2, n_paths=64, attribution=True, context=gpu_ctx)
    with pytest.raises(ValueError, match="does not take attribution"):
        simulate_bootstrap(np.random.default_rng(0).normal(0, 0.02, (30, 3)), w, n_steps=2, n_paths=64, attribution=True, context=gpu_ctx)
    # the context works on the next call: the attribution again, then the plain call
    got, first = gpu_ctx.simulate_attribution(prm, ref["mu"], ref["L"], ref["W"], ar.SEED, begin, n, True), _dev(idx)
    assert got.attr.tobytes() == first.attr.tobytes() and np.array_equal(_bits(got.contributions), _bits(first.contributions))
    st, term = _plain(gpu_ctx, idx)
    assert st.tobytes() == first.stats.tobytes() and np.array_equal(_bits(term), _bits(first.terminal))


def test_pipeline_prints_the_attribution_lines(gpu_ctx):
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
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("  risk attribution ")]
    assert len(lines) == 3 and all("CVaR share" in ln and "volatility share" in ln and "weight" in ln for ln in lines)
    shares = np.array([[float(ln.split("CVaR share")[1].split("%")[0]), float(ln.split("volatility share")[1].split("%")[0])] for ln in lines])
    assert np.all(np.abs(shares.sum(axis=0) - 100.0) < 0.02)


def test_streamlit_sweep_tab_shows_the_risk_pie(gpu_ctx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_shim import fake_streamlit
    record = []
    sys.modules["streamlit"] = fake_streamlit(record, 50_000)
    try:
        np.random.seed(4242)
        runpy.run_path(os.path.join(ROOT, "examples", "streamlit_app.py"), run_name="__main__")
    finally:
        del sys.modules["streamlit"]
    shown = [r[1][0] for r in record if r[0] == "write" and isinstance(r[1][0], dict) and "risk attribution" in r[1][0]]
    assert len(shown) == 1
    pie = shown[0]["risk attribution"]
    assert sorted(pie) == ["CVaR share %", "volatility share %", "weight %"]
    assert list(pie["weight %"]) == list(pie["CVaR share %"]) == list(pie["volatility share %"])
    for f in ("CVaR share %", "volatility share %"):
        assert abs(sum(pie[f].values()) - 100.0) < 0.05

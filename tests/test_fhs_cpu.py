"""CPU checks of filtered historical simulation (SPEC.md 2.4 / 4.11 / 5.11): the host filter (garch.filter_rows), the NumPy
restatement against the bootstrap's at alpha = 0, h0 = 1 and across horizons, mcp_filtered_pivots, every argument rule of
mcp_simulate_filtered through the C ABI with a NULL context (no device is touched), and the variance law on a binary64 twin."""
import ctypes
import math

import numpy as np
import pytest

from bootstrap_ref import simulate_boot
from fhs_ref import clustered_rows, fhs_pivots, law_check, law_inputs, simulate_fhs, twin64
from monte_carlo_portfolio_amd import _ffi, filter_rows, fit_garch, simulate_filtered
from monte_carlo_portfolio_amd.garch import FilteredRows, _filter64

SEED = 0xF11_7E12


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _inputs(R, N, K, seed=0):
    rng = np.random.default_rng(seed + 100 * N + R)
    mu = (rng.standard_normal(N) * 0.002).astype(np.float32)
    resid = (rng.standard_t(4, size=(R, N)) * 0.015).astype(np.float32)
    shock = (rng.chisquare(3, size=R) / 3.0).astype(np.float32)
    W = rng.dirichlet(np.ones(N), size=K).astype(np.float32)
    return mu, resid, shock, W


# ---- the host filter ----

@pytest.mark.parametrize("ab", [(0.12, 0.8), (0.3, 0.3), (0.0, 0.5)])
def test_filter_reproduces_the_rows_the_shock_level_and_h0(ab):
    X = clustered_rows(400, 4, seed=3)
    m, resid, shock, h, h0 = _filter64(X, *ab)
    back = np.sqrt(h)[:, None] * resid + m
    assert np.all(np.abs(back - X) <= 1e-12 * np.maximum(np.abs(X), np.abs(m)))
    R = X.shape[0]
    assert abs(np.mean(shock * h) - (R - 1) / R) <= 1e-12
    ht = 1.0                                                   # the recurrence again, on the shocks it returned
    for t in range(R):
        assert ht == h[t]
        ht = (1.0 - ab[0] - ab[1]) + ab[0] * (shock[t] * ht) + ab[1] * ht
    assert ht == h0
    f = filter_rows(X, ab + (123.0,))                          # an h0 given is ignored
    assert isinstance(f, FilteredRows) and f.h0 == h0 and (f.alpha, f.beta) == ab
    assert f.mu.dtype == f.resid.dtype == f.shock.dtype == np.float32
    assert np.array_equal(f.resid, resid.astype(np.float32)) and np.array_equal(f.shock, shock.astype(np.float32))
    assert np.array_equal(f.mu, m.astype(np.float32)) and np.all(f.shock >= 0)


def test_filter_without_dynamics_centres_the_rows_and_fits_when_asked():
    X = clustered_rows(300, 3, seed=5)
    f = filter_rows(X, (0.0, 0.0))
    assert f.h0 == 1.0 and np.array_equal(f.resid, (X - X.mean(axis=0)).astype(np.float32))
    fit = fit_garch(X)
    g = filter_rows(X)
    assert (g.alpha, g.beta) == (fit.alpha, fit.beta) and abs(g.h0 - fit.h0) <= 1e-12 * fit.h0
    assert fit.alpha > 0.0                                     # the rows are clustered: the filter has something to remove
    for bad in [(0.5, 0.5), (-0.1, 0.2), (float("nan"), 0.1), (0.1,)]:
        with pytest.raises(ValueError):
            filter_rows(X, bad)


# ---- the restatement ----

@pytest.mark.parametrize("N,K,R,b", [(1, 1, 9, 1.0), (5, 3, 40, 2.5), (16, 2, 300, math.inf)])
def test_restatement_without_dynamics_is_the_bootstrap_on_the_shifted_rows(N, K, R, b):
    mu, resid, shock, W = _inputs(R, N, K)
    paths = np.array([0, 1, 255, 256, 1000, (1 << 32) - 1, 1 << 32, (1 << 40) + 7], np.uint64)
    hz = [1, 3, 12]
    got = simulate_fhs(mu, resid, shock, W, 12, SEED, paths, b, (0.0, 0.65, 1.0), v0=2.0, horizons=hz)
    assert np.all(got["h"] == 1.0)
    rows = (resid.astype(np.float64) + mu.astype(np.float64)).astype(np.float32)
    want = simulate_boot(rows, W, 12, SEED, paths, b, "simple", v0=2.0, horizons=hz)
    assert np.array_equal(got["idx"], want["idx"])
    assert np.array_equal(_bits(got["V_T"]), _bits(want["V_T"])) and np.array_equal(_bits(got["V_h"]), _bits(want["V_h"]))


def test_restatement_horizon_rows_are_the_shorter_calls_and_h_moves():
    mu, resid, shock, W = _inputs(60, 6, 2, seed=1)
    paths = np.arange(37, dtype=np.uint64) + np.uint64(5)
    g = (0.3, 0.3, 4.0)
    hz = [1, 2, 5, 9]
    full = simulate_fhs(mu, resid, shock, W, 9, SEED, paths, 2.5, g, horizons=hz)
    assert np.array_equal(_bits(full["V_h"][-1]), _bits(full["V_T"]))
    for i, h in enumerate(hz):
        assert np.array_equal(_bits(simulate_fhs(mu, resid, shock, W, h, SEED, paths, 2.5, g)["V_T"]), _bits(full["V_h"][i])), h
    assert np.all(full["h"][0] == np.float32(4.0)) and len(np.unique(full["h"][5])) > 1
    flat = simulate_fhs(mu, resid, shock, W, 9, SEED, paths, 2.5, (0.0, 0.6, 1.0))
    assert not np.array_equal(_bits(flat["V_T"]), _bits(full["V_T"]))


# ---- the C ABI ----

def _call(lib, prm, ft, gv=(0.1, 0.8, 1.5), hz=(), levels=(), W=True, stats=True, bands=None):
    K, N = prm.n_portfolios, prm.n_assets
    H, L = len(hz), len(levels)
    steps, lv = np.asarray(hz, np.int32), np.asarray(levels, np.float64)
    st = np.zeros(K, _ffi.STATS_DTYPE)
    Wm = np.full((K, N), 1.0 / N, np.float32)
    hst = np.zeros((max(H, 1), K), _ffi.STATS_DTYPE)
    bd = np.zeros((max(H, 1), K, max(L, 1)), np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                           # noqa: E731
    g = _ffi.McpGarch(*gv, 0) if gv is not None and not isinstance(gv, _ffi.McpGarch) else gv
    with_bands = L > 0 if bands is None else bands
    return lib.mcp_simulate_filtered(None, ctypes.byref(prm), ctypes.byref(ft) if ft is not None else None,
                                     ctypes.byref(g) if g is not None else None, vp(Wm) if W else None,
                                     1, 0, 100, H, vp(steps) if H else None, L, vp(lv) if L else None, None, vp(st) if stats else None,
                                     None, vp(hst) if H else None, vp(bd) if with_bands else None)


def test_a_valid_request_reaches_the_null_context(mcp_lib):
    mu, resid, shock, _ = _inputs(30, 4, 1)
    prm = _ffi.make_params(4, 10, 2)
    for b in (1.0, 2.5, math.inf):
        ft = _ffi.make_filtered(mu, resid, shock, b)
        assert _call(mcp_lib, prm, ft) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()
        assert _call(mcp_lib, prm, ft, hz=[2, 10], levels=[5.0, 95.0]) == _ffi.MCP_E_ARG
        assert b"ctx is NULL" in mcp_lib.mcp_last_error()
    zero = _ffi.make_filtered(mu, resid, np.zeros_like(shock), 1.0)            # s_j = 0 is allowed
    assert _call(mcp_lib, prm, zero, gv=(0.0, 0.0, 1.0)) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()


def _broken(what):
    mu, resid, shock, _ = _inputs(30, 4, 1)
    block, n_rows, reserved = 1.0, None, 0
    if what == "mu":
        mu[2] = np.inf
    elif what == "resid":
        resid[7, 3] = np.nan
        resid[9, 0] = np.nan
    elif what == "shock_nan":
        shock[11] = np.nan
    elif what == "shock_neg":
        shock[4] = -1e-30
    elif what == "block_low":
        block = 0.999
    elif what == "block_nan":
        block = float("nan")
    elif what == "rows_0":
        n_rows = 0
    elif what == "rows_big":
        n_rows = _ffi.MCP_MAX_BOOT_ROWS + 1
    elif what == "reserved":
        reserved = 1
    ft = _ffi.make_filtered(mu, resid, shock, block)
    if n_rows is not None:
        ft.n_rows = n_rows
    ft.reserved = reserved
    return ft, (mu, resid, shock)


BAD_FILTERED = [("mu", "filtered mu, asset 2"), ("resid", "filtered resid row 7, asset 3"), ("shock_nan", "filtered shock, row 11"),
                ("shock_neg", "filtered shock, row 4"), ("block_low", "mean_block"), ("block_nan", "mean_block"), ("rows_0", "n_rows"),
                ("rows_big", "n_rows"), ("reserved", "reserved")]


@pytest.mark.parametrize("what,msg", BAD_FILTERED)
def test_every_rule_of_the_rows_is_e_arg_and_names_the_first_offender(what, msg, mcp_lib):
    ft, keep = _broken(what)
    prm = _ffi.make_params(4, 10, 1)
    assert _call(mcp_lib, prm, ft) == _ffi.MCP_E_ARG
    assert msg.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    assert _call(mcp_lib, prm, ft, hz=[1, 5], levels=[50.0]) == _ffi.MCP_E_ARG
    assert msg.encode() in mcp_lib.mcp_last_error()
    piv = np.zeros(1, np.float64)
    assert mcp_lib.mcp_filtered_pivots(ctypes.byref(prm), ctypes.byref(ft), np.ones((1, 4), np.float32), piv) == _ffi.MCP_E_ARG
    assert msg.encode() in mcp_lib.mcp_last_error()


def test_null_structs_members_and_outputs(mcp_lib):
    mu, resid, shock, _ = _inputs(30, 4, 1)
    prm = _ffi.make_params(4, 10, 1)
    ft = _ffi.make_filtered(mu, resid, shock, 1.0)
    assert _call(mcp_lib, prm, None) == _ffi.MCP_E_ARG and b"filtered is NULL" in mcp_lib.mcp_last_error()
    for member in ("mu", "resid", "shock"):
        part = _ffi.make_filtered(mu, resid, shock, 1.0)
        setattr(part, member, None)
        assert _call(mcp_lib, prm, part) == _ffi.MCP_E_ARG
        assert f"filtered {member} is NULL".encode() in mcp_lib.mcp_last_error()
    assert _call(mcp_lib, prm, ft, gv=None) == _ffi.MCP_E_ARG and b"garch is NULL" in mcp_lib.mcp_last_error()
    assert _call(mcp_lib, prm, ft, W=False) == _ffi.MCP_E_ARG
    assert _call(mcp_lib, prm, ft, stats=False) == _ffi.MCP_E_ARG
    assert _call(mcp_lib, prm, ft, hz=[1, 5], levels=[50.0], bands=False) == _ffi.MCP_E_ARG and b"bands_out" in mcp_lib.mcp_last_error()
    assert _call(mcp_lib, prm, ft, hz=[3, 2]) == _ffi.MCP_E_ARG and b"increasing" in mcp_lib.mcp_last_error()
    assert _call(mcp_lib, _ffi.make_params(4, -1, 1), ft) == _ffi.MCP_E_ARG


BAD_GARCH = [(-0.1, 0.5, 1.0), (0.5, -0.1, 1.0), (0.6, 0.4, 1.0), (0.1, 0.8, 0.0), (0.1, 0.8, -1.0), (float("nan"), 0.5, 1.0),
             (0.1, float("inf"), 1.0), (0.1, 0.8, 1e39), (1.0 - 2.0 ** -26, 0.0, 1.0)]


@pytest.mark.parametrize("gv", BAD_GARCH)
def test_the_rules_of_the_garch_triple_hold(gv, mcp_lib):
    mu, resid, shock, _ = _inputs(30, 4, 1)
    ft = _ffi.make_filtered(mu, resid, shock, 1.0)
    assert _call(mcp_lib, _ffi.make_params(4, 10, 1), ft, gv=gv) == _ffi.MCP_E_ARG
    assert b"garch" in mcp_lib.mcp_last_error()
    assert _call(mcp_lib, _ffi.make_params(4, 10, 1), ft, gv=_ffi.McpGarch(0.1, 0.8, 1.0, 1)) == _ffi.MCP_E_ARG
    assert b"reserved" in mcp_lib.mcp_last_error()


def test_what_is_not_combined_is_unsupported_and_the_older_refusals_stand(mcp_lib):
    mu, resid, shock, _ = _inputs(30, 4, 1)
    ft = _ffi.make_filtered(mu, resid, shock, 1.0)
    for kw in ({"compounding": "log"}, {"fold": True}, {"native_math": True}):
        assert _call(mcp_lib, _ffi.make_params(4, 10, 1, **kw), ft) == _ffi.MCP_E_UNSUPPORTED, kw
    piv = np.zeros(1, np.float64)
    assert mcp_lib.mcp_filtered_pivots(ctypes.byref(_ffi.make_params(4, 10, 1, compounding="log")), ctypes.byref(ft),
                                       np.ones((1, 4), np.float32), piv) == _ffi.MCP_E_UNSUPPORTED
    bad, _keep = _broken("shock_neg")                          # an argument error is found before what is not combined
    assert _call(mcp_lib, _ffi.make_params(4, 10, 1, compounding="log"), bad) == _ffi.MCP_E_ARG
    for kw in ({"compounding": "log"}, {"dof": 5}, {"drawdown": True}, {"rebalance": 3}, {"antithetic": True}):
        with pytest.raises(ValueError):
            simulate_filtered((mu, resid, shock), np.ones(4) / 4, garch=(0.1, 0.8), **kw)
    with pytest.raises(ValueError):                            # a plain triple carries no (alpha, beta, h0)
        simulate_filtered((mu, resid, shock), np.ones(4) / 4)
    with pytest.raises(ValueError):
        simulate_filtered((mu, resid, -shock - 1), np.ones(4) / 4, garch=(0.1, 0.8))
    with pytest.raises(ValueError):
        simulate_filtered((mu, resid, shock), np.ones(4) / 4, garch=(0.1, 0.8), block=0.5)


@pytest.mark.parametrize("T", [0, 1, 12, 252])
def test_pivots_match_the_formula(T, mcp_lib):
    for R, N, K in [(1, 1, 1), (13, 3, 4), (300, 16, 3), (57, 33, 2)]:
        mu, resid, shock, W = _inputs(R, N, K, seed=T)
        got = _ffi.filtered_pivots(_ffi.make_params(N, T, K), mu + np.float32(0.003), resid, shock, W)
        want = fhs_pivots(mu + np.float32(0.003), resid, W, T)
        assert np.allclose(got, want, rtol=1e-15, atol=0.0), (R, N, K, got, want)
    mu, resid, shock, W = _inputs(5, 2, 1)
    assert _ffi.filtered_pivots(_ffi.make_params(2, 10, 1), mu - np.float32(3.0), resid, shock, W)[0] == 0.0   # m <= -1


# ---- the variance law (SPEC.md 4.11, b = 1) ----

def test_variance_law_on_the_binary64_twin():
    f, w, g = law_inputs()
    rho, _ = twin64(f.mu, f.resid, f.shock, w, 6, g, 1_000_000, np.random.default_rng(2024))
    z, rel, Eh = law_check(rho, f, w, g)
    print("z", z, "relative standard error", rel, "E[h]", Eh)
    assert np.all(np.abs(z) <= 5.0), z
    assert np.all(rel < 0.01) and np.all(Eh[:-1] / Eh[1:] > 1.05)     # a constant h is many standard errors away from step 1 on

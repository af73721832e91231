"""CPU checks of the Merton jump-diffusion (SPEC.md 2.5 / 4.12 / 5.12): the host constants of mcp_jump_consts against the pure-Python
restatement and the Poisson tail, the restatement in jump_ref.py against the Gaussian oracle at its anchors, the new C ABI symbols
and struct, argument errors and refused combinations with no device, the Python argument checks, jumps.diffusion_cov and
jumps.fit_jumps, and the binary64 twin against the assertions of the GPU law test."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from jump_ref import LAW_JUMPS, jump_consts, law_checks, law_market, law_of, simulate_jumps, twin_rows, twin_values
from monte_carlo_portfolio_amd import JumpFit, _ffi, diffusion_cov, fit_jumps, jump_law, synthetic
from monte_carlo_portfolio_amd.simulate import check_jumps, prepare_inputs
from oracle import np_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x3E_7A11
LAMBDAS = [0.0, 1e-9, 0.01, 0.15, 0.5, 1.0]


def _market(N, K):
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(17 * N + K).dirichlet(np.ones(N), size=K)
    return prepare_inputs(mu, cov, W)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the host constants ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", LAMBDAS)
def test_thresholds_and_drift_equal_the_restatement(lam, mcp_lib):
    rng = np.random.default_rng(5)
    for N, loading in ((1, None), (3, [1.5, 0.5, -0.25]), (16, None), (5, [0.0, 1.0, 2.0, 0.0, -1.0])):
        mu = rng.normal(4e-4, 2e-3, N).astype(np.float32)
        mu[0] = 0.0
        for m, s in ((-0.08, 0.05), (0.0, 0.0), (0.03, 0.0)):
            thr, mean_count, drift = _ffi.jump_consts(lam, m, s, loading, mu)
            want = jump_consts(lam, m, s, mu, loading)
            assert np.array_equal(thr, want[0]) and thr.dtype == np.uint32
            assert mean_count == want[1]
            assert np.array_equal(_bits(drift), _bits(want[4]))
            if loading is not None:                       # an asset with no loading keeps its drift
                assert all(drift[i] == mu[i] for i in range(N) if loading[i] == 0)
            if lam == 0.0 or m == 0.0:
                assert np.array_equal(_bits(drift), _bits(mu))


def test_known_thresholds(mcp_lib):
    assert int(_ffi.jump_consts(0.15, -0.08, 0.05)[0][0]) == 598254685 == int(jump_consts(0.15, -0.08, 0.05)[0][0])
    assert int(_ffi.jump_consts(1.0, -0.08, 0.05)[0][7]) == 44019 == int(jump_consts(1.0, -0.08, 0.05)[0][7])
    thr0 = _ffi.jump_consts(0.0, -0.08, 0.05)
    assert np.all(thr0[0] == 0) and thr0[1] == 0.0


@pytest.mark.parametrize("lam", LAMBDAS)
def test_thresholds_are_the_poisson_upper_tail(lam, mcp_lib):
    """thr_k within +-2 of 2^32 P(Poisson(lam) >= k), the tail summed from math.lgamma terms; E within 2^-30 of lam up to 0.15 (the
    tail beyond 8 jumps is below 1e-13 there, and 8 floors lose less than 8 2^-32)."""
    thr, mean_count, _ = _ffi.jump_consts(lam, 0.0, 0.0)
    for k in range(1, 9):
        tail = sum(math.exp(-lam + j * math.log(lam) - math.lgamma(j + 1)) for j in range(k, 60)) if lam > 0 else 0.0
        assert abs(int(thr[k - 1]) - tail * 2.0 ** 32) <= 2.0, (k, int(thr[k - 1]), tail * 2.0 ** 32)
    assert np.all(np.diff(thr.astype(np.int64)) <= 0)
    if lam <= 0.15:
        assert abs(mean_count - lam) <= 2.0 ** -30


def test_jump_law_reads_the_thresholds(mcp_lib):
    law, ref = jump_law((0.15, -0.08, 0.05)), law_of((0.15, -0.08, 0.05))
    assert np.array_equal(law.thresholds, ref["thr"]) and np.array_equal(law.pmf, ref["pmf"])
    assert law.pmf.shape == (9,) and abs(law.pmf.sum() - 1.0) < 1e-15 and np.all(law.pmf >= 0)
    assert law.mean_count == ref["mean_count"] and law.var_count == pytest.approx(ref["var_count"], rel=1e-14)
    assert law.k3_count == pytest.approx(ref["k3_count"], rel=1e-13) and law.var_jump == pytest.approx(ref["var_jump"], rel=1e-14)
    assert law.var_count == pytest.approx(0.15, rel=1e-6) and law.k3_count == pytest.approx(0.15, rel=1e-5)     # Poisson: all 0.15
    m, s = float(np.float32(-0.08)), float(np.float32(0.05))
    assert law.var_jump == pytest.approx(0.15 * (s * s + m * m), rel=1e-6)


# ---- the restatement at its anchors --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 3, 16])
@pytest.mark.parametrize("jumps", [(0.0, -0.08, 0.05), (0.5, 0.0, 0.0), (0.5, -0.08, 0.05, "zero")])
def test_the_anchors_are_the_gaussian_oracle_bit_for_bit(N, jumps):
    """lambda = 0, m = s = 0 and b = 0: J = +-0 or b J = +-0, the drift is not compensated, and fma(b, J, mu) = mu for mu != 0."""
    K, T, n, begin = 2, 5, 24, (1 << 32) - 12
    mu, L, W = _market(N, K)
    assert np.all(mu != 0)
    if len(jumps) == 4:
        jumps = jumps[:3] + (np.zeros(N, np.float32),)
    got = simulate_jumps(mu, L, W, T, SEED, np.arange(begin, begin + n, dtype=np.uint64), jumps)
    want = np_oracle.simulate(mu, L, W, T, n, SEED, path_begin=begin, exact=True)
    assert np.array_equal(_bits(got["V_T"]), _bits(want))
    if jumps[0] == 0.0:
        assert np.all(got["n"] == 0)
    else:
        assert got["n"].max() >= 1


def test_a_jump_moves_every_asset_and_the_restatement_partitions():
    mu, L, W = _market(3, 2)
    j = (0.5, -0.05, 0.03, [1.5, 0.5, -0.25])
    paths = np.arange(30, dtype=np.uint64) + np.uint64(100)
    full = simulate_jumps(mu, L, W, 9, SEED, paths, j, horizons=[2, 5, 9])
    assert not np.array_equal(_bits(full["V_T"]), _bits(np_oracle.simulate(mu, L, W, 9, 30, SEED, path_begin=100, exact=True)))
    assert {0, 1} <= set(full["n"].ravel().tolist()) and full["n"].max() >= 2
    assert np.all((full["J"] == 0) == (full["n"] == 0))
    for i, h in enumerate([2, 5, 9]):
        assert np.array_equal(_bits(full["V_h"][i]), _bits(simulate_jumps(mu, L, W, h, SEED, paths, j)["V_T"]))
    a, b = simulate_jumps(mu, L, W, 9, SEED, paths[:11], j), simulate_jumps(mu, L, W, 9, SEED, paths[11:], j)
    assert np.array_equal(_bits(np.concatenate([a["V_T"], b["V_T"]], axis=1)), _bits(full["V_T"]))
    one = simulate_jumps(mu, L, W[:1], 4, SEED, paths, j)
    assert np.array_equal(one["n"], full["n"][:4]) and np.array_equal(_bits(one["J"]), _bits(full["J"][:4]))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def test_struct_symbols_and_header(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcport.h")).read(), flags=re.S)
    assert re.search(r"\bmcp_simulate_jumps\s*\(", text) and re.search(r"\bmcp_jump_consts\s*\(", text)
    assert re.search(r"typedef struct \{\s*double intensity, mean, std;\s*const float \*loading;\s*int32_t reserved;\s*\} mcp_jumps;", text)
    for name in ("mcp_simulate_jumps", "mcp_jump_consts"):
        assert name in _ffi.SIGNATURES and hasattr(mcp_lib, name)
    assert ctypes.sizeof(_ffi.McpJumps) == 40 and _ffi.MCP_MAX_JUMPS == 8
    assert _ffi.MCP_ABI_VERSION == 4 == mcp_lib.mcp_abi_version()


def _raw():
    fn = ctypes.CDLL(_ffi.LIB_PATH).mcp_simulate_jumps
    fn.restype = ctypes.c_int
    return fn


def _call(prm, jp, hz=(), levels=(), dd=False, mdd=False, stats=True, mu=True, W=True):
    """mcp_simulate_jumps with a NULL context through an untyped handle: every rule of the request is checked before the context."""
    N, K = prm.n_assets, prm.n_portfolios
    m = np.full(N, 1e-3, np.float32)
    L = np.eye(N, dtype=np.float32) * 0.01
    Wm = np.full((K, N), 1.0 / N, np.float32)
    s = np.zeros(K, _ffi.STATS_DTYPE)
    ds = np.zeros(K, _ffi.STATS_DTYPE)
    md = np.zeros(K * 100, np.float32)
    h = np.asarray(hz, np.int32)
    lv = np.asarray(levels, np.float64)
    hs = np.zeros(max(1, h.size * K), _ffi.STATS_DTYPE)
    bb = np.zeros(max(1, h.size * K * lv.size), np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    return _raw()(None, ctypes.byref(prm), ctypes.byref(jp) if jp is not None else None, vp(m) if mu else None, vp(L),
                  vp(Wm) if W else None, ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100), h.size, vp(h) if h.size else None,
                  lv.size, vp(lv) if lv.size else None, None, vp(s) if stats else None, vp(md) if mdd else None, vp(ds) if dd else None,
                  None, vp(hs) if h.size else None, vp(bb) if lv.size else None)


NAN, INF = float("nan"), float("inf")
BAD = [(-1e-9, -0.08, 0.05, None, 0, "intensity"), (1.0 + 1e-9, -0.08, 0.05, None, 0, "intensity"), (NAN, -0.08, 0.05, None, 0, "finite"),
       (0.1, INF, 0.05, None, 0, "finite"), (0.1, -0.08, NAN, None, 0, "finite"), (0.1, 1e39, 0.05, None, 0, "binary32"),
       (0.1, -0.08, 1e39, None, 0, "binary32"), (0.1, -0.08, -1e-9, None, 0, "std"), (0.1, -0.08, 0.05, None, 1, "reserved"),
       (0.1, -0.08, 0.05, [1.0, NAN, 1.0, 1.0], 0, "loading"), (0.1, -0.08, 0.05, [1.0, 1.0, 1.0, -INF], 0, "loading")]


@pytest.mark.parametrize("lam,m,s,loading,reserved,what", BAD)
def test_bad_requests_return_e_arg_before_any_device(lam, m, s, loading, reserved, what, mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    ld = np.asarray(loading, np.float32) if loading is not None else None
    jp = _ffi.make_jumps(lam, m, s, ld)
    jp.reserved = reserved
    assert _call(prm, jp) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    assert _call(prm, jp, hz=[2, 5], levels=[50.0]) == _ffi.MCP_E_ARG
    assert _call(prm, jp, dd=True) == _ffi.MCP_E_ARG
    thr = np.zeros(8, np.uint32)
    e = ctypes.c_double()
    assert mcp_lib.mcp_jump_consts(ctypes.byref(jp), 4, None, thr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(e), None) == _ffi.MCP_E_ARG


def test_a_good_request_reaches_the_context_check_and_null_pointers_do_not(mcp_lib):
    prm = _ffi.make_params(4, 10, 2)
    ld = np.array([1.5, 0.0, -2.0, 1.0], np.float32)
    for jp in (_ffi.make_jumps(0.15, -0.08, 0.05), _ffi.make_jumps(0.0, 0.0, 0.0), _ffi.make_jumps(1.0, 3e38, 0.0, ld)):
        for kw in ({}, {"hz": [2, 5], "levels": [50.0]}, {"dd": True}):
            assert _call(prm, jp, **kw) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    ok = _ffi.make_jumps(0.15, -0.08, 0.05)
    assert _call(prm, None) == _ffi.MCP_E_ARG and b"jumps is NULL" in mcp_lib.mcp_last_error()
    for kw in ({"mu": False}, {"W": False}, {"stats": False}):
        assert _call(prm, ok, **kw) == _ffi.MCP_E_ARG and b"NULL pointer" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, mdd=True) == _ffi.MCP_E_ARG and b"mdd_out" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, hz=[3, 2]) == _ffi.MCP_E_ARG and b"increasing" in mcp_lib.mcp_last_error()
    e = ctypes.c_double()
    assert mcp_lib.mcp_jump_consts(ctypes.byref(ok), 4, None, None, ctypes.byref(e), None) == _ffi.MCP_E_ARG
    assert mcp_lib.mcp_jump_consts(ctypes.byref(ok), 0, None, None, ctypes.byref(e), None) == _ffi.MCP_E_ARG


@pytest.mark.parametrize("kw", [{"compounding": "log"}, {"fold": True}, {"native_math": True}])
def test_log_fold_and_native_math_are_unsupported(kw, mcp_lib):
    prm = _ffi.make_params(4, 10, 1, **kw)
    ok = _ffi.make_jumps(0.15, -0.08, 0.05)
    assert _call(prm, ok) == _ffi.MCP_E_UNSUPPORTED and b"jump" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, hz=[2, 5]) == _ffi.MCP_E_UNSUPPORTED
    assert _call(prm, ok, dd=True) == _ffi.MCP_E_UNSUPPORTED


def test_drawdown_with_horizons_is_unsupported(mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    assert _call(prm, _ffi.make_jumps(0.15, -0.08, 0.05), hz=[2, 5], dd=True) == _ffi.MCP_E_UNSUPPORTED
    assert b"horizons and the drawdown" in mcp_lib.mcp_last_error()


# ---- the Python rules ------------------------------------------------------------------------------------------------------

def test_check_jumps_accepts():
    assert check_jumps(None, 3) is None
    assert check_jumps((0.15, -0.08, 0.05), 3) == (0.15, -0.08, 0.05, None)
    assert check_jumps([np.float32(0.25), 0, np.int64(0)], 2)[:3] == (0.25, 0.0, 0.0)
    lam, m, s, b = check_jumps((1.0, 0.03, 0.0, [1.5, 0.5, -0.25]), 3)
    assert (lam, m, s) == (1.0, 0.03, 0.0) and b.dtype == np.float32 and b.tolist() == [1.5, 0.5, -0.25]
    assert check_jumps((0.1, 0.0, 0.0, None), 3)[3] is None
    fit = JumpFit(0.1, -0.05, 0.02, np.ones(3), 7)
    assert check_jumps(fit[:4], 3)[:3] == (0.1, -0.05, 0.02)


OV = {"overlay": {0: [("Stock", 0.0, 0.0, 1.0)]}, "spot": [1.0, 1.0, 1.0]}


@pytest.mark.parametrize("kw,match", [
    ({"jumps": True}, "jumps must be"), ({"jumps": "abc"}, "jumps must be"), ({"jumps": 0.1}, "jumps must be"),
    ({"jumps": (0.1, 0.2)}, "jumps must be"), ({"jumps": (0.1, 0.2, 0.3, None, 1)}, "jumps must be"),
    ({"jumps": (0.1, "0.8", 0.1)}, "jumps must be"), ({"jumps": (True, 0.0, 0.1)}, "jumps must be"), ({"jumps": (0.1, None, 0.1)}, "jumps must be"),
    ({"jumps": (NAN, 0.0, 0.1)}, "finite"), ({"jumps": (0.1, INF, 0.1)}, "finite"), ({"jumps": (0.1, 0.0, NAN)}, "finite"),
    ({"jumps": (0.1, 1e39, 0.1)}, "finite"), ({"jumps": (0.1, 0.0, 1e39)}, "finite"), ({"jumps": (-0.1, 0.0, 0.1)}, "intensity"),
    ({"jumps": (1.5, 0.0, 0.1)}, "intensity"), ({"jumps": (0.1, 0.0, -0.1)}, "std"),
    ({"jumps": (0.1, 0.0, 0.1, [1.0, 1.0])}, "loading"), ({"jumps": (0.1, 0.0, 0.1, [1.0, NAN, 1.0])}, "loading"),
    ({"jumps": (0.1, 0.0, 0.1, [1.0, 1e39, 1.0])}, "loading"),
    ({"jumps": (0.1, -0.01, 0.01), "compounding": "log"}, "log"), ({"jumps": (0.1, -0.01, 0.01), "fold": True}, "fold"),
    ({"jumps": (0.1, -0.01, 0.01), "native_math": True}, "native_math"), ({"jumps": (0.1, -0.01, 0.01), "rebalance": 3}, "rebalance"),
    ({"jumps": (0.1, -0.01, 0.01), "cashflow": 1.0}, "cashflow"), ({"jumps": (0.1, -0.01, 0.01), **OV}, "overlay"),
    ({"jumps": (0.1, -0.01, 0.01), "dof": 5}, "dof"), ({"jumps": (0.1, -0.01, 0.01), "garch": (0.1, 0.8)}, "garch"),
    ({"jumps": (0.1, -0.01, 0.01), "attribution": True}, "attribution"), ({"jumps": (0.1, -0.01, 0.01), "antithetic": True}, "antithetic"),
    ({"jumps": (0.1, -0.01, 0.01), "drawdown": True, "horizons": [2, 5]}, "horizons"),
    ({"jumps": (1.0, -0.5, 0.5)}, "positive definite"),
])
def test_python_rejects_bad_calls_without_a_context(kw, match, monkeypatch, mcp_lib):
    """The ValueError comes before any device is touched."""
    from monte_carlo_portfolio_amd import simulate as sim

    def boom(*a, **k):
        raise AssertionError("a context was requested")
    monkeypatch.setattr(sim, "default_context", boom)
    mu, cov = synthetic.synthetic_market(3)
    with pytest.raises(ValueError, match=match):
        sim.simulate_paths(mu, cov, np.ones(3) / 3, n_steps=20, n_paths=8, **kw)


def test_context_call_refuses_what_the_library_cannot_be_asked(monkeypatch):
    """Context._call with jumps and another draw model raises before the library is called (the C entry point has no such arguments)."""
    from monte_carlo_portfolio_amd.simulate import Context
    c = Context.__new__(Context)
    c._h = ctypes.c_void_p()
    prm = _ffi.make_params(3, 5, 1)
    mu, L, W = _market(3, 1)
    j = (0.1, -0.01, 0.01, None)
    for kw in ({"dof": 5}, {"garch": (0.1, 0.8, 1.0)}, {"period": 2}, {"flows": np.zeros(5, np.float32)}, {"rows": np.zeros((4, 3), np.float32)}):
        with pytest.raises(ValueError, match="jumps are not combined"):
            c._call(prm, W, 1, 0, 8, False, mu=mu, chol=L, jumps=j, **kw)


def test_simulate_sweep_passes_jumps_through(monkeypatch):
    from monte_carlo_portfolio_amd import simulate as sim
    seen = {}

    def fake(mu, cov, W, **kw):
        seen.update(kw)
        return np.zeros(W.shape[0], _ffi.STATS_DTYPE)
    monkeypatch.setattr(sim, "simulate_paths", fake)
    mu, cov = synthetic.synthetic_market(3)
    sim.simulate_sweep(mu, cov, weights=np.eye(3), jumps=(0.1, -0.02, 0.01))
    assert seen["jumps"] == (0.1, -0.02, 0.01)


def test_simulate_bootstrap_rejects_jumps(monkeypatch):
    from monte_carlo_portfolio_amd import simulate as sim
    monkeypatch.setattr(sim, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("context")))
    rows = np.random.default_rng(0).normal(0.0, 0.02, size=(30, 3))
    with pytest.raises(ValueError):
        sim.simulate_bootstrap(rows, np.ones(3) / 3, n_steps=20, n_paths=8, jumps=(0.1, -0.02, 0.01))


# ---- diffusion_cov and fit_jumps ---------------------------------------------------------------------------------------------

def test_diffusion_cov_round_trip_and_refusal(mcp_lib):
    mu, cov = synthetic.synthetic_market(3)
    j = (0.05, -0.02, 0.005, [0.5, 1.0, -1.5])
    b = np.array([0.5, 1.0, -1.5])
    d = diffusion_cov(cov, j, 3)
    vj = jump_law(j).var_jump
    np.testing.assert_allclose(d + vj * np.outer(b, b), cov, rtol=0, atol=1e-18)
    assert np.array_equal(diffusion_cov(cov, (0.0, -0.08, 0.05)), np.asarray(cov, np.float64))
    np.testing.assert_allclose(diffusion_cov(cov, (0.15, -0.02, 0.01)), cov - jump_law((0.15, -0.02, 0.01)).var_jump, rtol=0, atol=1e-18)
    with pytest.raises(ValueError, match="positive definite"):
        diffusion_cov(cov, (1.0, -0.5, 0.5))
    with pytest.raises(ValueError, match="entries"):
        diffusion_cov(cov, (0.1, -0.02, 0.01, [1.0, 1.0]))
    with pytest.raises(ValueError, match="cov must be"):
        diffusion_cov(cov, (0.1, -0.02, 0.01), 4)


def test_fit_jumps_recovers_the_intensity_and_the_mean():
    """20,000 twin rows at (0.1, -0.08, 0.03), loadings (1.5, 1, 0.5), on the three-asset market at 0.4 times its volatilities (0.4 to
    1.5 % a step; the equal-weight mean then has a diffusive standard deviation of 0.8 %).  A threshold rule only sees jumps that
    stand clear of the diffusion: here the cut, 3 robust standard deviations, is about 0.025, 1.8 standard deviations of the jump size
    inside its mean, so 96 % of the jumps pass it and the truncation moves the mean by a few per cent; 0.27 % of the diffusive rows
    pass it too, 2.4 % of the jump count.  (On the unscaled market the cut is 0.06 and a third of the jumps hide in the diffusion:
    the rule then reports 0.06, which is what it is documented to do.)"""
    mu, cov, _ = law_market(3)
    cov = 0.16 * cov
    b = [1.5, 1.0, 0.5]
    rows, n = twin_rows(mu, cov, (0.1, -0.08, 0.03, b), 20_000, 11)
    fit = fit_jumps(rows)
    print("fit_jumps:", fit, "true jump rows:", int(np.count_nonzero(n)))
    assert isinstance(fit, JumpFit) and fit.n_jump_rows == round(fit.intensity * 20_000)
    assert abs(fit.intensity - 0.1) <= 0.3 * 0.1
    assert fit.mean < 0 and abs(fit.mean - (-0.08)) <= 0.25 * 0.08
    assert fit.std > 0 and fit.loading.shape == (3,)
    assert fit.loading[0] > fit.loading[1] > fit.loading[2] > 0
    assert check_jumps(fit[:4], 3)[0] == fit.intensity


def test_fit_jumps_reports_no_jumps_on_gaussian_rows():
    mu, cov, _ = law_market(3)
    rows, n = twin_rows(mu, cov, (0.0, -0.08, 0.03), 20_000, 12)
    assert np.all(n == 0)
    fit = fit_jumps(rows)
    assert fit.intensity < 0.01 and fit.n_jump_rows == round(fit.intensity * 20_000)
    flat = fit_jumps(np.zeros((50, 2)))
    assert flat == JumpFit(0.0, 0.0, 0.0, flat.loading, 0) and np.all(flat.loading == 1.0)
    one = fit_jumps(np.r_[np.random.default_rng(1).normal(0, 0.01, 200), [-0.5]])
    assert one.n_jump_rows >= 1 and one.loading.shape == (1,) and one.mean < 0
    with pytest.raises(ValueError):
        fit_jumps(np.array([[0.1, np.nan]]))


# ---- the law: the binary64 twin against the assertions of the GPU law test ---------------------------------------------------

@pytest.mark.parametrize("N", [1, 3])
def test_the_twin_passes_the_law_assertions_at_the_gpu_tests_size(N):
    """The model itself, in binary64 on NumPy's generator, stays within the 5 standard errors the GPU law test allows."""
    mu, cov, w = law_market(N)
    V = twin_values(mu, cov, w, 12, 1_000_000, LAW_JUMPS, seed=40 + N)
    print(N, law_checks(V, 1.0, float(w @ mu), float(w @ cov @ w), float(w.sum()), LAW_JUMPS))

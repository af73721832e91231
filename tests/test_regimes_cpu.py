"""CPU checks of the two-regime Markov switching (SPEC.md 2.6 / 4.13 / 5.13): the host constants of mcp_regime_consts, the pivots of
mcp_regime_pivots against a direct binary64 matrix product, the restatement in regime_ref.py against the Gaussian oracle at its
anchors, the new C ABI symbols and struct, argument errors and refused combinations with no device, the Python argument checks,
regimes.regime_law, the binary64 twin against the assertions of the GPU law test, and regimes.fit_regimes."""
import ctypes
import os
import re

import numpy as np
import pytest

import regime_ref as rr
from monte_carlo_portfolio_amd import RegimeFit, _ffi, fit_regimes, regime_law, regimes, synthetic
from monte_carlo_portfolio_amd.simulate import _regime_block, check_regimes, prepare_inputs
from oracle import np_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5E_61BE
PROBS = (0.2, 0.3, 0.5)
NAN, INF = float("nan"), float("inf")


def _market(N, K, scale=1.0, shift=0.0):
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(17 * N + K).dirichlet(np.ones(N), size=K)
    return prepare_inputs(np.asarray(mu) + shift, np.asarray(cov) * scale, W)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the host constants ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p,thr", [(0.0, 0), (1.0, 1 << 32), (2.0 ** -33, 0), (0.5, 1 << 31), (1.0 - 2.0 ** -33, (1 << 32) - 1)])
def test_consts_at_the_edges(p, thr, mcp_lib):
    """thr = min(2^32, floor(p 2^32)): p = 0 never, p = 1 always (2^32 is above every 32-bit word), 2^-33 rounds down to never, and
    1 - 2^-33 to all but one word."""
    for slot in range(3):
        args = [0.25, 0.25, 0.25]
        args[slot] = p
        got_thr, got_p = _ffi.regime_consts(*args)
        want_thr, want_p = rr.regime_consts(*args)
        assert got_thr.dtype == np.uint64 and got_thr.tolist() == want_thr and int(got_thr[slot]) == thr
        assert got_p.tolist() == want_p and got_p[slot] == thr / 2.0 ** 32
    assert regimes.used_probabilities(p, p, p) == (thr / 2.0 ** 32,) * 3


def test_consts_of_ordinary_probabilities(mcp_lib):
    thr, p = _ffi.regime_consts(0.05, 0.2, 0.7)
    assert thr.tolist() == [214748364, 858993459, 3006477107]
    assert np.all(p <= [0.05, 0.2, 0.7]) and np.all(np.array([0.05, 0.2, 0.7]) - p < 2.0 ** -32)


# ---- the pivots ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probs", [PROBS, (0.05, 0.2, 0.7), (0.0, 0.0, 0.0), (0.0, 0.3, 1.0), (1.0, 1.0, 0.0), (0.3, 0.0, 0.25)])
def test_pivots_equal_a_direct_matrix_product(probs, mcp_lib):
    """mcp_regime_pivots' vector recursion against pi' D (P D)^(h-1) 1 - 1 by np.linalg.matrix_power: c + 1 is a product of at most 60
    factors near 1, each step four roundings of 2^-53 relative, in either order -- 60 * 4 * 2^-53 = 2.7e-14 of a value near 1; the
    subtraction of 1 is exact in both.  So the two agree to 1e-13 absolute."""
    mu, _, W = _market(3, 4)
    mu1 = (mu - np.float32(0.02)).astype(np.float32)
    T, hs = 60, [1, 2, 7, 12, 59, 60]
    prm = _ffi.make_params(3, T, 4)
    piv, hz = _ffi.regime_pivots(prm, probs, mu, mu1, W, hs)
    p = rr.regime_consts(*probs)[1]
    want = rr.pivots_direct(*p, mu, mu1, W, hs)
    np.testing.assert_allclose(hz, want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(piv, want[-1], rtol=0, atol=1e-13)
    law = regime_law(probs, mu, np.eye(3), mu1, np.eye(3), W, T)
    assert np.array_equal(law.pivots[[h - 1 for h in hs]], hz)           # the same recursion in NumPy: bit for bit
    if probs[0] == 0.0 and probs[2] == 0.0:                               # all calm: the Gaussian pivot (1 + m)^h - 1
        m = W.astype(np.float64) @ mu.astype(np.float64)
        np.testing.assert_allclose(hz, [(1.0 + m) ** h - 1.0 for h in hs], rtol=0, atol=1e-13)
    none, hz0 = _ffi.regime_pivots(_ffi.make_params(3, 0, 4), probs, mu, mu1, W)
    assert hz0 is None and np.all(none == 0.0)                            # T = 0


def test_regime_law_is_the_direct_law(mcp_lib):
    mu, L, W = _market(3, 2)
    mu1, L1 = (mu - np.float32(0.03)).astype(np.float32), (L * np.float32(2.5)).astype(np.float32)
    law = regime_law((0.05, 0.2, 0.7), mu, L, mu1, L1, W, 12)
    p = rr.regime_consts(0.05, 0.2, 0.7)[1]
    assert (law.p01, law.p10, law.start) == tuple(p)
    np.testing.assert_allclose(law.pi, rr.occupancy_direct(*p, 12), rtol=1e-13)
    for k in range(2):
        w = W[k].astype(np.float64)
        m = [float(w @ v.astype(np.float64)) for v in (mu, mu1)]
        s2 = [float(np.sum((f.astype(np.float64).T @ w) ** 2)) for f in (L, L1)]
        _, mean, var = rr.step_law(*p, m, s2, 12)
        np.testing.assert_allclose(law.mean[:, k], mean, rtol=1e-12)
        np.testing.assert_allclose(law.var[:, k], var, rtol=1e-12)
    assert np.all(law.var[:, 0] > 0) and law.pivots.shape == (12, 2)


# ---- the restatement at its anchors --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 3, 16])
@pytest.mark.parametrize("case", ["identical", "all calm", "all crisis"])
def test_the_anchors_are_the_gaussian_oracle_bit_for_bit(N, case):
    K, T, n, begin = 2, 5, 24, (1 << 32) - 12
    mu, L, W = _market(N, K)
    mu1, L1, _ = _market(N, K, scale=4.0, shift=-0.01)
    paths = np.arange(begin, begin + n, dtype=np.uint64)
    if case == "identical":
        got = rr.simulate_regimes(mu, L, mu, L, W, T, SEED, paths, PROBS)
        want = np_oracle.simulate(mu, L, W, T, n, SEED, path_begin=begin, exact=True)
        assert {0, 1} == set(got["s"].ravel().tolist())
    elif case == "all calm":
        got = rr.simulate_regimes(mu, L, mu1, L1, W, T, SEED, paths, (0.0, 0.3, 0.0))
        want = np_oracle.simulate(mu, L, W, T, n, SEED, path_begin=begin, exact=True)
        assert np.all(got["s"] == 0)
    else:
        got = rr.simulate_regimes(mu, L, mu1, L1, W, T, SEED, paths, (0.2, 0.0, 1.0))
        want = np_oracle.simulate(mu1, L1, W, T, n, SEED, path_begin=begin, exact=True)
        assert np.all(got["s"] == 1)
    assert np.array_equal(_bits(got["V_T"]), _bits(want))


def test_the_restatement_switches_and_partitions():
    mu, L, W = _market(3, 2)
    mu1, L1, _ = _market(3, 2, scale=4.0, shift=-0.01)
    paths = np.arange(40, dtype=np.uint64) + np.uint64(100)
    full = rr.simulate_regimes(mu, L, mu1, L1, W, 9, SEED, paths, PROBS, horizons=[2, 5, 9])
    assert rr.transitions_seen(full["s"]) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert not np.array_equal(_bits(full["V_T"]), _bits(np_oracle.simulate(mu, L, W, 9, 40, SEED, path_begin=100, exact=True)))
    for i, h in enumerate([2, 5, 9]):                         # the counter does not depend on T
        part = rr.simulate_regimes(mu, L, mu1, L1, W, h, SEED, paths, PROBS)
        assert np.array_equal(_bits(full["V_h"][i]), _bits(part["V_T"])) and np.array_equal(part["s"], full["s"][:h])
    a = rr.simulate_regimes(mu, L, mu1, L1, W, 9, SEED, paths[:11], PROBS)
    b = rr.simulate_regimes(mu, L, mu1, L1, W, 9, SEED, paths[11:], PROBS)
    assert np.array_equal(_bits(np.concatenate([a["V_T"], b["V_T"]], axis=1)), _bits(full["V_T"]))
    one = rr.simulate_regimes(mu, L, mu1, L1, W[:1], 4, SEED, paths, PROBS)      # all portfolios of a path share s_t
    assert np.array_equal(one["s"], full["s"][:4])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

def test_struct_symbols_and_header(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcport.h")).read(), flags=re.S)
    for name in ("mcp_simulate_regimes", "mcp_regime_consts", "mcp_regime_pivots"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _ffi.SIGNATURES and hasattr(mcp_lib, name)
    assert re.search(r"typedef struct \{\s*double p01, p10, start;\s*const float \*mu1;\s*const float \*chol1;\s*int32_t reserved;\s*\} "
                     r"mcp_regimes;", text)
    assert ctypes.sizeof(_ffi.McpRegimes) == 48
    assert _ffi.MCP_ABI_VERSION == 4 == mcp_lib.mcp_abi_version()


def _raw():
    fn = ctypes.CDLL(_ffi.LIB_PATH).mcp_simulate_regimes
    fn.restype = ctypes.c_int
    return fn


def _regime(N, p01=0.2, p10=0.3, start=0.5, mu1=True, chol1=True, reserved=0, poison_mu=None, poison_chol=None):
    m1 = np.full(N, -1e-3, np.float32)
    L1 = np.eye(N, dtype=np.float32) * 0.03
    if poison_mu is not None:
        m1[-1] = poison_mu
    if poison_chol is not None:
        L1[-1, 0] = poison_chol
    rs = _ffi.make_regimes(p01, p10, start, m1 if mu1 else None, L1 if chol1 else None)
    rs.reserved = reserved
    return rs, (m1, L1)


def _call(prm, rs, hz=(), levels=(), dd=False, mdd=False, stats=True, mu=True, chol=True, W=True, poison=None):
    """mcp_simulate_regimes with a NULL context through an untyped handle: every rule of the request is checked before the context."""
    N, K = prm.n_assets, prm.n_portfolios
    m = np.full(N, 1e-3, np.float32)
    L = np.eye(N, dtype=np.float32) * 0.01
    if poison == "mu":
        m[0] = NAN
    if poison == "chol":
        L[-1, -1] = INF
    Wm = np.full((K, N), 1.0 / N, np.float32)
    s = np.zeros(K, _ffi.STATS_DTYPE)
    ds = np.zeros(K, _ffi.STATS_DTYPE)
    md = np.zeros(K * 100, np.float32)
    h = np.asarray(hz, np.int32)
    lv = np.asarray(levels, np.float64)
    hs = np.zeros(max(1, h.size * K), _ffi.STATS_DTYPE)
    bb = np.zeros(max(1, h.size * K * lv.size), np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    return _raw()(None, ctypes.byref(prm), ctypes.byref(rs) if rs is not None else None, vp(m) if mu else None, vp(L) if chol else None,
                  vp(Wm) if W else None, ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100), h.size, vp(h) if h.size else None,
                  lv.size, vp(lv) if lv.size else None, None, vp(s) if stats else None, vp(md) if mdd else None, vp(ds) if dd else None,
                  None, vp(hs) if h.size else None, vp(bb) if lv.size else None)


BAD = [({"p01": -1e-9}, "outside"), ({"p01": 1.0 + 1e-9}, "outside"), ({"p10": -0.5}, "outside"), ({"p10": 1.5}, "outside"),
       ({"start": -1e-9}, "outside"), ({"start": 2.0}, "outside"), ({"p01": NAN}, "finite"), ({"p10": INF}, "finite"),
       ({"start": NAN}, "finite"), ({"reserved": 1}, "reserved"), ({"mu1": False}, "NULL"), ({"chol1": False}, "NULL"),
       ({"poison_mu": NAN}, "mu1"), ({"poison_mu": -INF}, "mu1"), ({"poison_chol": NAN}, "chol1"), ({"poison_chol": INF}, "chol1")]


@pytest.mark.parametrize("kw,what", BAD)
def test_bad_requests_return_e_arg_before_any_device(kw, what, mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    rs, keep = _regime(4, **kw)
    assert _call(prm, rs) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    assert _call(prm, rs, hz=[2, 5], levels=[50.0]) == _ffi.MCP_E_ARG
    assert _call(prm, rs, dd=True) == _ffi.MCP_E_ARG
    m = np.zeros(4, np.float32)
    Wm = np.full((1, 4), 0.25, np.float32)
    out = np.zeros(1)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    assert mcp_lib.mcp_regime_pivots(ctypes.byref(prm), ctypes.byref(rs), vp(m), vp(Wm), 0, None, vp(out), None) == _ffi.MCP_E_ARG
    if "poison_mu" not in kw and "poison_chol" not in kw and "mu1" not in kw and "chol1" not in kw:     # the consts read no array
        thr, p = np.zeros(3, np.uint64), np.zeros(3)
        assert mcp_lib.mcp_regime_consts(ctypes.byref(rs), vp(thr), vp(p)) == _ffi.MCP_E_ARG


def test_a_good_request_reaches_the_context_check_and_null_pointers_do_not(mcp_lib):
    prm = _ffi.make_params(4, 10, 2)
    for probs in (PROBS, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
        rs, keep = _regime(4, *probs)
        for kw in ({}, {"hz": [2, 5], "levels": [50.0]}, {"dd": True}):
            assert _call(prm, rs, **kw) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    ok, keep = _regime(4)
    assert _call(prm, None) == _ffi.MCP_E_ARG and b"regimes is NULL" in mcp_lib.mcp_last_error()
    for kw in ({"mu": False}, {"chol": False}, {"W": False}, {"stats": False}):
        assert _call(prm, ok, **kw) == _ffi.MCP_E_ARG and b"NULL pointer" in mcp_lib.mcp_last_error()
    for poison in ("mu", "chol"):
        assert _call(prm, ok, poison=poison) == _ffi.MCP_E_ARG and b"not finite" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, mdd=True) == _ffi.MCP_E_ARG and b"mdd_out" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, hz=[3, 2]) == _ffi.MCP_E_ARG and b"increasing" in mcp_lib.mcp_last_error()
    thr = np.zeros(3, np.uint64)
    assert mcp_lib.mcp_regime_consts(ctypes.byref(ok), thr.ctypes.data_as(ctypes.c_void_p), None) == _ffi.MCP_E_ARG
    assert mcp_lib.mcp_regime_consts(None, thr.ctypes.data_as(ctypes.c_void_p), None) == _ffi.MCP_E_ARG


@pytest.mark.parametrize("kw", [{"compounding": "log"}, {"fold": True}, {"native_math": True}])
def test_log_fold_and_native_math_are_unsupported(kw, mcp_lib):
    prm = _ffi.make_params(4, 10, 1, **kw)
    ok, keep = _regime(4)
    assert _call(prm, ok) == _ffi.MCP_E_UNSUPPORTED and b"regime" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, hz=[2, 5]) == _ffi.MCP_E_UNSUPPORTED
    assert _call(prm, ok, dd=True) == _ffi.MCP_E_UNSUPPORTED


def test_drawdown_with_horizons_is_unsupported(mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    ok, keep = _regime(4)
    assert _call(prm, ok, hz=[2, 5], dd=True) == _ffi.MCP_E_UNSUPPORTED
    assert b"horizons and the drawdown" in mcp_lib.mcp_last_error()


# ---- the Python rules ------------------------------------------------------------------------------------------------------

MU1 = [-0.01, -0.02, -0.03]
COV1 = (np.eye(3) * 0.01).tolist()


def test_check_regimes_accepts():
    assert check_regimes(None, 3) is None
    p01, p10, start, mu1, L1 = check_regimes((0.05, 0.2, MU1, COV1), 3)
    assert (p01, p10) == (0.05, 0.2) and start == 0.05 / 0.25 and mu1.dtype == np.float32 and L1.dtype == np.float32
    np.testing.assert_allclose(L1, np.eye(3) * 0.1, rtol=1e-7)
    assert check_regimes((0.0, 0.0, MU1, COV1), 3)[2] == 0.0                       # both 0: start 0
    assert check_regimes((0.05, 0.2, MU1, COV1, None), 3)[2] == 0.2
    assert check_regimes((np.float32(0.25), 1, MU1, COV1, np.int64(0)), 3)[:3] == (0.25, 1.0, 0.0)
    chol1 = np.array([[0.1, 9.0, 9.0], [0.01, 0.1, 9.0], [0.0, 0.02, 0.1]])
    L1 = check_regimes((0.05, 0.2, MU1, chol1, 0.7), 3, factor=True)[4]            # chol=: the factor, lower triangle, untouched
    assert np.array_equal(L1, np.tril(chol1).astype(np.float32))
    fit = RegimeFit(0.05, 0.2, np.zeros(3), np.eye(3), np.asarray(MU1), np.asarray(COV1), 0.9, 0.0, 0.0)
    assert check_regimes((fit.p01, fit.p10, fit.mu1, fit.cov1, fit.start), 3)[:3] == (0.05, 0.2, 0.9)


OV = {"overlay": {0: [("Stock", 0.0, 0.0, 1.0)]}, "spot": [1.0, 1.0, 1.0]}
OK = (0.05, 0.2, MU1, COV1)


@pytest.mark.parametrize("kw,match", [
    ({"regimes": True}, "regimes must be"), ({"regimes": "abcd"}, "regimes must be"), ({"regimes": 0.1}, "regimes must be"),
    ({"regimes": (0.1, 0.2, MU1)}, "regimes must be"), ({"regimes": (0.1, 0.2, MU1, COV1, 0.5, 1)}, "regimes must be"),
    ({"regimes": ("0.1", 0.2, MU1, COV1)}, "regimes must be"), ({"regimes": (True, 0.2, MU1, COV1)}, "regimes must be"),
    ({"regimes": (0.1, None, MU1, COV1)}, "regimes must be"), ({"regimes": (0.1, 0.2, MU1, COV1, "0.5")}, "regimes must be"),
    ({"regimes": (NAN, 0.2, MU1, COV1)}, "probabilities"), ({"regimes": (0.1, INF, MU1, COV1)}, "probabilities"),
    ({"regimes": (-0.1, 0.2, MU1, COV1)}, "probabilities"), ({"regimes": (0.1, 1.5, MU1, COV1)}, "probabilities"),
    ({"regimes": (0.1, 0.2, MU1, COV1, -0.1)}, "probabilities"), ({"regimes": (0.1, 0.2, MU1, COV1, NAN)}, "probabilities"),
    ({"regimes": (0.1, 0.2, MU1[:2], COV1)}, "mu1 must hold"), ({"regimes": (0.1, 0.2, MU1, np.eye(2))}, "mu1 must hold"),
    ({"regimes": (0.1, 0.2, [0.0, NAN, 0.0], COV1)}, "finite"), ({"regimes": (0.1, 0.2, [0.0, 1e39, 0.0], COV1)}, "finite"),
    ({"regimes": (0.1, 0.2, MU1, np.full((3, 3), INF))}, "finite"), ({"regimes": (0.1, 0.2, MU1, -np.eye(3))}, "positive definite"),
    ({"regimes": (0.1, 0.2, MU1, "cov")}, "regimes must be"),
    ({"regimes": OK, "compounding": "log"}, "log"), ({"regimes": OK, "fold": True}, "fold"), ({"regimes": OK, "native_math": True}, "native_math"),
    ({"regimes": OK, "rebalance": 3}, "rebalance"), ({"regimes": OK, "cashflow": 1.0}, "cashflow"), ({"regimes": OK, **OV}, "overlay"),
    ({"regimes": OK, "dof": 5}, "dof"), ({"regimes": OK, "garch": (0.1, 0.8)}, "garch"), ({"regimes": OK, "jumps": (0.1, -0.01, 0.01)}, "jumps"),
    ({"regimes": OK, "attribution": True}, "attribution"), ({"regimes": OK, "antithetic": True}, "antithetic"),
    ({"regimes": OK, "drawdown": True, "horizons": [2, 5]}, "horizons"),
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


def test_non_finite_regime_0_is_rejected_without_a_context(monkeypatch, mcp_lib):
    from monte_carlo_portfolio_amd import simulate as sim
    monkeypatch.setattr(sim, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("context")))
    mu, cov = synthetic.synthetic_market(3)
    with pytest.raises(ValueError, match="finite"):
        sim.simulate_paths([0.0, NAN, 0.0], cov, np.ones(3) / 3, n_steps=20, n_paths=8, regimes=OK)
    with pytest.raises(ValueError, match="finite"):
        sim.simulate_paths(mu, cov, np.ones(3) / 3, n_steps=20, n_paths=8, regimes=OK, chol=np.full((3, 3), INF))


def test_context_call_refuses_what_the_library_cannot_be_asked():
    """Context._call with regimes and another draw model raises before the library is called (the C entry point has no such
    arguments), and PathEngine has no regimes at all."""
    from monte_carlo_portfolio_amd.engine import PathEngine
    from monte_carlo_portfolio_amd.simulate import Context
    c = Context.__new__(Context)
    c._h = ctypes.c_void_p()
    prm = _ffi.make_params(3, 5, 1)
    mu, L, W = _market(3, 1)
    r = (0.05, 0.2, 0.5, mu, L)
    for kw in ({"dof": 5}, {"garch": (0.1, 0.8, 1.0)}, {"period": 2}, {"flows": np.zeros(5, np.float32)}, {"rows": np.zeros((4, 3), np.float32)},
               {"jumps": (0.1, -0.01, 0.01, None)}, {"attribution": True}, {"antithetic": True}):
        with pytest.raises(ValueError, match="regimes are not combined"):
            c._call(prm, W, 1, 0, 8, False, mu=mu, chol=L, regimes=r, **kw)
    import inspect
    assert not any("regimes" in inspect.signature(f).parameters for _, f in inspect.getmembers(PathEngine, inspect.isfunction))


def test_simulate_sweep_passes_regimes_through(monkeypatch):
    from monte_carlo_portfolio_amd import simulate as sim
    seen = {}

    def fake(mu, cov, W, **kw):
        seen.update(kw)
        return np.zeros(W.shape[0], _ffi.STATS_DTYPE)
    monkeypatch.setattr(sim, "simulate_paths", fake)
    mu, cov = synthetic.synthetic_market(3)
    sim.simulate_sweep(mu, cov, weights=np.eye(3), regimes=OK)
    assert seen["regimes"] is OK


def test_bootstrap_and_filtered_reject_regimes(monkeypatch):
    from monte_carlo_portfolio_amd import simulate as sim
    monkeypatch.setattr(sim, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("context")))
    rows = np.random.default_rng(0).normal(0.0, 0.02, size=(30, 3))
    with pytest.raises(ValueError):
        sim.simulate_bootstrap(rows, np.ones(3) / 3, n_steps=20, n_paths=8, regimes=OK)
    with pytest.raises(ValueError):
        sim.simulate_filtered((np.zeros(3), rows, np.ones(30)), np.ones(3) / 3, n_steps=20, n_paths=8, garch=(0.1, 0.8, 1.0), regimes=OK)


def test_the_result_block(mcp_lib):
    blk = _regime_block((0.05, 0.2, 0.7, None, None), np.array([1, 6, 12], np.int32))
    p = rr.regime_consts(0.05, 0.2, 0.7)[1]
    assert (blk["p01"], blk["p10"], blk["start"]) == tuple(p)
    assert blk["stationary"] == p[0] / (p[0] + p[1]) and blk["mean_duration"] == (1.0 / p[0], 1.0 / p[1])
    occ = rr.occupancy_direct(*p, 12)
    np.testing.assert_allclose(blk["occupancy"], [occ[:1].mean(), occ[:6].mean(), occ[:12].mean()], rtol=1e-13)
    calm = _regime_block((0.0, 0.0, 0.0, None, None), None)
    assert calm["stationary"] == 0.0 and calm["mean_duration"] == (INF, INF) and "occupancy" not in calm


# ---- the law: the binary64 twin against the assertions of the GPU law test ---------------------------------------------------

TWIN = dict(p01=0.05, p10=0.20, start=0.7, m=(0.01, -0.03), sd=(0.04, 0.10))


@pytest.mark.parametrize("persistent", [True, False])
def test_the_twin_passes_the_law_assertions_at_the_gpu_tests_size(persistent):
    """The model itself, in binary64 on NumPy's generator, stays within the 5 standard errors the GPU law test allows: T = 12, 10^6
    paths, one asset with (m, sigma) = (0.01, 0.04) in regime 0 and (-0.03, 0.10) in regime 1 -- or, for the null of the lag-1 test,
    regime 0's law in both."""
    m, sd = (TWIN["m"], TWIN["sd"]) if persistent else ((0.01, 0.01), (0.04, 0.04))
    p = rr.regime_consts(TWIN["p01"], TWIN["p10"], TWIN["start"])[1]
    V = rr.twin_values(*p, m, sd, 12, 1_000_000, seed=46 + persistent)
    mu, mu1 = np.array([m[0]], np.float64), np.array([m[1]], np.float64)
    piv = rr.pivots_direct(*p, mu, mu1, np.ones((1, 1)), list(range(1, 13)))[:, 0]
    _, mean, var = rr.step_law(*p, m, (sd[0] ** 2, sd[1] ** 2), 12)
    print(persistent, rr.law_checks(V, 1.0, piv, mean, var, persistent))


# ---- fit_regimes ---------------------------------------------------------------------------------------------------------------

def _series(R, p01, p10, ratio, seed, shift=0.0):
    """R rows of N = 3 from the two-regime model: regime 0 the synthetic market, regime 1 its volatilities times `ratio` and its
    means moved by `shift`; -> (rows, s, truth)."""
    mu0, cov0 = (np.asarray(a, np.float64) for a in synthetic.synthetic_market(3))
    mu1, cov1 = mu0 + shift, cov0 * ratio ** 2
    rng = np.random.default_rng(seed)
    s = np.zeros(R, np.int64)
    cur = int(rng.random() < regimes.stationary(p01, p10))
    for t in range(R):
        s[t] = cur
        cur = int(rng.random() < p01) if cur == 0 else int(rng.random() >= p10)
    z = rng.standard_normal((R, 3))
    L0, L1 = np.linalg.cholesky(cov0), np.linalg.cholesky(cov1)
    rows = np.where((s == 1)[:, None], mu1 + z @ L1.T, mu0 + z @ L0.T)
    return rows, s, (p01, p10, mu0, cov0, mu1, cov1)


@pytest.fixture(scope="module")
def two_regime_fit():
    rows, s, truth = _series(4000, 0.05, 0.10, 3.0, 7, shift=-0.002)
    fit, trace = regimes.baum_welch(rows)
    return rows, s, truth, fit, trace


def test_fit_regimes_climbs_and_beats_the_truth(two_regime_fit):
    """4000 rows, N = 3, volatility ratio 3, p01 = 0.05, p10 = 0.10.  An EM step cannot lower the likelihood; the trace is a sum of
    4000 binary64 logs of size ~10 each, so rounding alone moves it by at most 4000 * 10 * 2^-52 < 1e-11: the allowance below."""
    rows, s, truth, fit, trace = two_regime_fit
    print("fit:", fit.p01, fit.p10, fit.start, fit.loglik, fit.loglik_iid, len(trace))
    assert isinstance(fit, RegimeFit) and len(trace) <= regimes.MAX_ITER + 1
    assert np.all(np.diff(trace) >= -1e-9), np.diff(trace).min()
    assert fit.loglik == trace[-1] and fit.loglik >= fit.loglik_iid
    assert fit.loglik >= regimes.regime_loglik(rows, *truth)
    again = fit_regimes(rows)                                                     # deterministic
    assert all(np.array_equal(x, y) for x, y in zip(fit, again))


def test_fit_regimes_orders_and_recovers(two_regime_fit):
    rows, s, truth, fit, _ = two_regime_fit
    assert np.sum(fit.cov1) > np.sum(fit.cov0)                                    # regime 1: the larger equal-weight variance
    ratio = np.sqrt(np.diag(fit.cov1) / np.diag(fit.cov0))
    assert np.all(np.abs(ratio - 3.0) < 0.3), ratio
    assert abs(fit.p01 - 0.05) < 0.02 and abs(fit.p10 - 0.10) < 0.04
    assert 0.0 <= fit.start <= 1.0
    want = (1.0 - fit.p10) if s[-1] == 1 else fit.p01                             # today's regime, moved one step on
    assert abs(fit.start - want) < 0.15, (fit.start, want, s[-5:])
    assert not regimes.no_evidence(fit, 4000)
    p01, p10, start, mu1, L1 = check_regimes((fit.p01, fit.p10, fit.mu1, fit.cov1, fit.start), 3)
    assert start == fit.start


def test_fit_regimes_on_one_regime_finds_no_evidence():
    """The rule: loglik - loglik_iid <= (q / 2) log R with q = N + N (N + 1) / 2 + 3 extra parameters (Schwarz).  For N = 3 and
    R = 4000 that is 6 * 8.29 = 49.8 units of log-likelihood."""
    rows, _, _ = _series(4000, 0.0, 1.0, 1.0, 8)
    fit = fit_regimes(rows)
    print("one regime:", fit.loglik - fit.loglik_iid, fit.p01, fit.p10)
    assert regimes.extra_parameters(3) == 12
    assert fit.loglik >= fit.loglik_iid - 1e-9
    assert fit.loglik - fit.loglik_iid <= 0.5 * 12 * np.log(4000.0)
    assert regimes.no_evidence(fit, 4000)


def test_fit_regimes_rejects_bad_rows():
    with pytest.raises(ValueError):
        fit_regimes(np.array([[0.1, np.nan], [0.0, 0.0], [0.1, 0.2], [0.3, 0.1]]))
    with pytest.raises(ValueError):
        fit_regimes(np.zeros((3, 3)))

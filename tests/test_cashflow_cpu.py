"""CPU checks of contributions, withdrawals and ruin (SPEC.md 4.7 / 5.6): the NumPy restatement in cashflow_ref.py against the C
oracle (an all-zero schedule) and against a scalar binary32 annuity (a market without noise), mcp_cashflow_pivots against the
restatement's Horner walk and against the plain pivots, the new C ABI symbols and struct, every argument error with no device,
and the Python argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from bootstrap_ref import boot_pivots
from cashflow_ref import counts_of, horner_pivots, simulate_cf, step_means, walk
from monte_carlo_portfolio_amd import _ffi, synthetic
from monte_carlo_portfolio_amd.simulate import prepare_inputs
from oracle.np_oracle import _fma32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mcp_simulate_cashflow", "mcp_cashflow_pivots")
SEED = 0xCA5_F10


def _rows(R, N, seed=0):
    return np.random.default_rng(seed).normal(0.001, 0.02, size=(R, N)).astype(np.float32)


# ---- 1. the restatement with an all-zero schedule is the C oracle --------------------------------------------------------------

@pytest.mark.parametrize("N,K,T", [(3, 3, 9), (16, 2, 7)])
def test_zero_schedule_restatement_is_the_c_oracle(N, K, T, oracle):
    mu, cov = synthetic.synthetic_market(N)
    mu32, L, W32 = prepare_inputs(mu, cov, synthetic.dirichlet_weights(N, K))
    want = oracle.simulate(mu32, L, W32, T, 200, SEED)
    got = simulate_cf(np.zeros(T, np.float32), W32, T, SEED, np.arange(200, dtype=np.uint64), mu=mu32, chol=L, horizons=[1, T])
    assert np.all(got["rho"] > -1.0) and np.all(want > 0)           # the plain values stay positive: ruin never acts
    assert np.array_equal(got["V_T"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["V_h"][1].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["V_h"][0].view(np.uint32), oracle.simulate(mu32, L, W32, 1, 200, SEED).view(np.uint32))


# ---- 2. the pivots ------------------------------------------------------------------------------------------------------------

def _schedule(T, seed=3):
    c = np.random.default_rng(seed).normal(0.0, 0.02, T).astype(np.float32)
    if T >= 2:
        c[0], c[1] = np.float32(0.05), np.float32(-0.04)              # both signs, whatever the draw
    return c


@pytest.mark.parametrize("T", [0, 1, 60])
@pytest.mark.parametrize("v0", [1.0, 10_000.0, 0.1])
def test_pivots_equal_the_horner_walk(T, v0, mcp_lib):
    N, K = 5, 4
    mu, cov = synthetic.synthetic_market(N)
    mu32, _, W32 = prepare_inputs(mu, cov, synthetic.dirichlet_weights(N, K))
    rows = _rows(40, N)
    flows = (_schedule(T) * np.float32(v0)).astype(np.float32)
    prm = _ffi.make_params(N, T, K, v0=v0)
    for kw in ({"mu": mu32}, {"rows": rows}):
        got = _ffi.cashflow_pivots(prm, flows, W32, **kw)
        want, _ = horner_pivots(step_means(W32, **kw), flows, v0)
        assert np.all(np.abs(got - want) <= 1e-15 * np.maximum(1.0, np.abs(want))), (kw.keys(), got, want)
        if T == 0:
            assert np.all(got == 0.0)


@pytest.mark.parametrize("T", [0, 12, 252])
def test_zero_schedule_pivots_are_the_plain_pivots(T, mcp_lib):
    N, K = 6, 3
    mu, cov = synthetic.synthetic_market(N)
    mu32, L, W32 = prepare_inputs(mu, cov, synthetic.dirichlet_weights(N, K))
    rows = _rows(50, N, 1)
    prm = _ffi.make_params(N, T, K, v0=250.0)
    zero = np.zeros(T, np.float32)
    got = _ffi.cashflow_pivots(prm, zero, W32, mu=mu32)
    want = _ffi.pivots(prm, mu32, L, W32)
    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    got = _ffi.cashflow_pivots(prm, zero, W32, rows=rows)
    want = _ffi.bootstrap_pivots(prm, rows, W32)
    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    assert np.all(np.abs(want - boot_pivots(rows, W32, T)) <= 1e-12 * np.maximum(1.0, np.abs(want)))


def test_hopeless_plan_pivots_at_minus_one_and_horizons_share_the_walk(mcp_lib):
    mu32 = np.array([0.001], np.float32)
    W32 = np.ones((1, 1), np.float32)
    flows = np.full(30, -0.1, np.float32)
    assert _ffi.cashflow_pivots(_ffi.make_params(1, 30, 1), flows, W32, mu=mu32)[0] == -1.0
    at_T, at_h = horner_pivots(step_means(W32, mu=mu32), flows, 1.0, horizons=[3, 9, 30])
    assert at_T[0] == -1.0 and at_h[2, 0] == -1.0 and -1.0 < at_h[1, 0] < at_h[0, 0] < 0.0
    for i, h in enumerate([3, 9, 30]):                               # one walk gives every horizon: A_h is the T = h pivot
        assert at_h[i, 0] == _ffi.cashflow_pivots(_ffi.make_params(1, h, 1), flows[:h], W32, mu=mu32)[0]


# ---- 3. header / binding / library ----------------------------------------------------------------------------------------------

def test_new_symbols_in_header_binding_and_library(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcport.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text)
        assert name in _ffi.SIGNATURES and hasattr(mcp_lib, name)
    assert re.search(r"typedef struct \{\s*const float \*flows;\s*int32_t n_flows;\s*int32_t has_target;\s*double target;\s*\} mcp_cashflow;",
                     text)
    assert ctypes.sizeof(_ffi.McpCashflow) == 24
    assert re.search(r"#define MCP_ABI_VERSION 4\b", text)
    assert _ffi.MCP_ABI_VERSION == 4 == mcp_lib.mcp_abi_version()


# ---- 4. argument errors with a NULL context -------------------------------------------------------------------------------------

def _raw(name):
    fn = getattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    fn.restype = ctypes.c_int
    return fn


def _call(prm, cf="ok", source="gauss", st=None, hz=(), levels=(), counts=True, hz_counts=None, hz_stats=None, bands=None,
          stats=True, W=True, flows=None, has_target=0, target=0.0, n_flows=None):
    """mcp_simulate_cashflow with a NULL context through an untyped handle (NULL pointers anywhere)."""
    N, K, T = prm.n_assets, prm.n_portfolios, prm.n_steps
    mu = np.full(N, 1e-3, np.float32)
    L = np.eye(N, dtype=np.float32) * 0.01
    bt = _ffi.make_bootstrap(np.full((10, N), 0.01, np.float32), 2.0)
    Wm = np.full((K, N), 1.0 / N, np.float32)
    s = np.zeros(K, _ffi.STATS_DTYPE)
    cn = np.zeros((K, 2), np.uint64)
    h = np.asarray(hz, np.int32)
    lv = np.asarray(levels, np.float64)
    hs = np.zeros(max(1, h.size * K), _ffi.STATS_DTYPE)
    bb = np.zeros(max(1, h.size * K * lv.size), np.float64)
    hc = np.zeros((max(1, h.size), K, 2), np.uint64)
    fl = np.full(max(T, 0), -0.01, np.float32) if flows is None else np.asarray(flows, np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    hz_stats = h.size > 0 if hz_stats is None else hz_stats
    hz_counts = h.size > 0 if hz_counts is None else hz_counts
    bands = lv.size > 0 if bands is None else bands
    if cf == "ok":
        cf = _ffi.McpCashflow(vp(fl) if fl.size else None, fl.size if n_flows is None else n_flows, has_target, target)
    elif cf == "null_flows":
        cf = _ffi.McpCashflow(None, T, 0, 0.0)
    mu_p = vp(mu) if source in ("gauss", "both", "mu") else None
    L_p = vp(L) if source in ("gauss", "both") else None
    b_p = ctypes.byref(bt) if source in ("boot", "both", "mu") else None
    return _raw("mcp_simulate_cashflow")(
        None, ctypes.byref(prm), ctypes.byref(cf) if cf is not None else None, mu_p, L_p, b_p,
        ctypes.byref(st) if st is not None else None, vp(Wm) if W else None, ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100),
        h.size, vp(h) if h.size else None, lv.size, vp(lv) if lv.size else None, None, vp(s) if stats else None,
        vp(cn) if counts else None, None, vp(hs) if hz_stats else None, vp(bb) if bands else None, vp(hc) if hz_counts else None)


BAD = [  # (keywords of _call, what the error names)
    ({"cf": None}, "cashflow is NULL"), ({"cf": "null_flows"}, "flows is NULL"), ({"n_flows": 9}, "n_flows"), ({"n_flows": 11}, "n_flows"),
    ({"n_flows": 0}, "n_flows"), ({"flows": [0.1] * 9 + [float("nan")]}, "not finite"), ({"flows": [float("inf")] + [0.1] * 9}, "not finite"),
    ({"flows": [-float("inf")] * 10}, "not finite"), ({"has_target": 1, "target": float("nan")}, "target"),
    ({"has_target": 1, "target": float("inf")}, "target"), ({"has_target": 2}, "has_target"), ({"has_target": -1}, "has_target"),
    ({"counts": False}, "counts_out"), ({"hz": [2, 5], "hz_counts": False}, "hz_counts_out"), ({"hz_counts": True}, "hz_counts_out"),
]


@pytest.mark.parametrize("kw,what", BAD)
@pytest.mark.parametrize("source", ["gauss", "boot", "t"])
def test_bad_requests_return_e_arg_with_a_null_context(kw, what, source, mcp_lib):
    prm = _ffi.make_params(4, 10, 2)
    st = _ffi.McpStudentT(5, 0) if source == "t" else None
    src = "gauss" if source == "t" else source
    assert _call(prm, source=src, st=st, **kw) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    if "hz" not in kw and "hz_counts" not in kw:
        assert _call(prm, source=src, st=st, hz=[2, 5], levels=[50.0], **kw) == _ffi.MCP_E_ARG
        assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()


def test_v0_that_rounds_to_zero_is_e_arg(mcp_lib):
    assert _call(_ffi.make_params(4, 10, 1, v0=1e-60)) == _ffi.MCP_E_ARG and b"rounds to zero" in mcp_lib.mcp_last_error()
    assert _call(_ffi.make_params(4, 10, 1, v0=1e-40)) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()   # a subnormal is > 0
    piv = np.zeros(1, np.float64)
    prm = _ffi.make_params(1, 2, 1, v0=1e-60)
    with pytest.raises(_ffi.McpError, match="rounds to zero"):
        _ffi.cashflow_pivots(prm, np.zeros(2, np.float32), np.ones((1, 1), np.float32), mu=np.zeros(1, np.float32))
    assert piv[0] == 0.0


def test_draw_sources_null_pointers_and_a_null_context(mcp_lib):
    prm = _ffi.make_params(4, 10, 2)
    for src in ("both", "none", "mu"):
        assert _call(prm, source=src) == _ffi.MCP_E_ARG and b"exactly one draw source" in mcp_lib.mcp_last_error()
    assert _call(prm, source="boot", st=_ffi.McpStudentT(5, 0)) == _ffi.MCP_E_ARG and b"exactly one draw source" in mcp_lib.mcp_last_error()
    assert _call(prm, st=_ffi.McpStudentT(2, 0)) == _ffi.MCP_E_ARG and b"dof" in mcp_lib.mcp_last_error()
    for kw in ({"W": False}, {"stats": False}):
        assert _call(prm, **kw) == _ffi.MCP_E_ARG and b"NULL pointer" in mcp_lib.mcp_last_error()
    assert _call(prm, hz=[3, 2]) == _ffi.MCP_E_ARG and b"increasing" in mcp_lib.mcp_last_error()
    assert _call(prm, hz_stats=True) == _ffi.MCP_E_ARG and b"n_horizons = 0" in mcp_lib.mcp_last_error()
    # a call rejected for its cash flows leaves the next valid call working: every valid request reaches the (NULL) context
    assert _call(prm, n_flows=3) == _ffi.MCP_E_ARG and b"n_flows" in mcp_lib.mcp_last_error()
    valid = [{}, {"source": "boot"}, {"st": _ffi.McpStudentT(5, 0)}, {"hz": [1, 10], "levels": [5.0, 95.0]}, {"has_target": 1, "target": 1.5},
             {"has_target": 0, "target": float("nan")}, {"flows": np.zeros(10)}]
    for kw in valid:
        assert _call(prm, **kw) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error(), kw
    assert _call(_ffi.make_params(4, 0, 2)) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()      # T = 0: no flows, NULL is fine


@pytest.mark.parametrize("kw", [{"compounding": "log"}, {"fold": True}, {"native_math": True}])
@pytest.mark.parametrize("source", ["gauss", "boot", "t"])
def test_log_fold_and_native_math_are_unsupported(kw, source, mcp_lib):
    prm = _ffi.make_params(4, 10, 1, **kw)
    st = _ffi.McpStudentT(5, 0) if source == "t" else None
    src = "gauss" if source == "t" else source
    assert _call(prm, source=src, st=st) == _ffi.MCP_E_UNSUPPORTED
    assert _call(prm, source=src, st=st, hz=[2, 5]) == _ffi.MCP_E_UNSUPPORTED
    if "compounding" in kw:
        with pytest.raises(_ffi.McpError, match="compound simply"):
            _ffi.cashflow_pivots(prm, np.zeros(10, np.float32), np.full((1, 4), 0.25, np.float32), mu=np.zeros(4, np.float32))


def test_pivot_argument_errors(mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    W = np.full((1, 4), 0.25, np.float32)
    fn = _raw("mcp_cashflow_pivots")
    out = np.zeros(1, np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    fl = np.zeros(10, np.float32)
    mu = np.zeros(4, np.float32)
    bt = _ffi.make_bootstrap(np.zeros((5, 4), np.float32), 1.0)
    ok = _ffi.McpCashflow(vp(fl), 10, 0, 0.0)
    assert fn(ctypes.byref(prm), None, vp(mu), None, vp(W), vp(out)) == _ffi.MCP_E_ARG
    assert fn(ctypes.byref(prm), ctypes.byref(ok), vp(mu), ctypes.byref(bt), vp(W), vp(out)) == _ffi.MCP_E_ARG
    assert fn(ctypes.byref(prm), ctypes.byref(ok), None, None, vp(W), vp(out)) == _ffi.MCP_E_ARG
    assert fn(ctypes.byref(prm), ctypes.byref(ok), vp(mu), None, None, vp(out)) == _ffi.MCP_E_ARG
    assert fn(ctypes.byref(prm), ctypes.byref(_ffi.McpCashflow(vp(fl), 9, 0, 0.0)), vp(mu), None, vp(W), vp(out)) == _ffi.MCP_E_ARG
    assert fn(ctypes.byref(prm), ctypes.byref(ok), vp(mu), None, vp(W), vp(out)) == 0
    assert fn(ctypes.byref(prm), ctypes.byref(ok), None, ctypes.byref(bt), vp(W), vp(out)) == 0


# ---- the Python argument checks -------------------------------------------------------------------------------------------------

PY_BAD = [
    ({"cashflow": True}, "cashflow"), ({"cashflow": [0.1] * 19}, "n_steps"), ({"cashflow": [0.1] * 21}, "n_steps"),
    ({"cashflow": [[0.1] * 20]}, "n_steps"), ({"cashflow": float("nan")}, "finite"), ({"cashflow": [0.1] * 19 + [float("inf")]}, "finite"),
    ({"cashflow": 1e39}, "finite"), ({"cashflow": [0.1] * 19 + [True]}, "bools"), ({"cashflow": "0.1"}, "cashflow"),
    ({"target": 2.0}, "target needs cashflow"), ({"cashflow": 0.1, "target": float("nan")}, "target"),
    ({"cashflow": 0.1, "target": True}, "target"), ({"cashflow": 0.1, "drawdown": True}, "drawdown"),
    ({"cashflow": 0.1, "rebalance": 3}, "rebalance"), ({"cashflow": 0.1, "rebalance": "never"}, "rebalance"),
    ({"cashflow": 0.1, "fold": True}, "fold"), ({"cashflow": 0.1, "native_math": True}, "native_math"),
    ({"cashflow": 0.1, "compounding": "log"}, "log"),
]


def _no_context(monkeypatch):
    from monte_carlo_portfolio_amd import simulate as sim

    def boom(*a, **k):
        raise AssertionError("a context was requested")
    monkeypatch.setattr(sim, "default_context", boom)
    return sim


@pytest.mark.parametrize("kw,match", PY_BAD)
def test_simulate_paths_rejects_bad_calls_without_a_context(kw, match, monkeypatch):
    sim = _no_context(monkeypatch)
    mu, cov = synthetic.synthetic_market(3)
    with pytest.raises(ValueError, match=match):
        sim.simulate_paths(mu, cov, np.ones(3) / 3, n_steps=20, n_paths=8, **kw)


@pytest.mark.parametrize("kw,match", [c for c in PY_BAD if not ({"drawdown", "fold", "native_math"} & set(c[0]))])
def test_simulate_bootstrap_rejects_bad_calls_without_a_context(kw, match, monkeypatch):
    sim = _no_context(monkeypatch)
    with pytest.raises(ValueError, match=match):
        sim.simulate_bootstrap(_rows(30, 3), np.ones(3) / 3, n_steps=20, n_paths=8, **kw)


@pytest.mark.parametrize("kw", [{"cashflow": -0.01}, {"cashflow": 0.0, "target": 1.2}, {"target": 1.2}])
def test_simulate_sweep_refuses_cash_flows(kw, monkeypatch):
    sim = _no_context(monkeypatch)
    mu, cov = synthetic.synthetic_market(3)
    with pytest.raises(ValueError, match="simulate_sweep does not take cashflow or target"):
        sim.simulate_sweep(mu, cov, n_portfolios=20, n_steps=20, n_paths=100, **kw)


def test_check_cashflow_rounds_to_binary32():
    from monte_carlo_portfolio_amd.simulate import check_cashflow
    assert check_cashflow(None, None, 5) == (None, None)
    f, g = check_cashflow(0.1, 3, 4)
    assert f.dtype == np.float32 and f.tolist() == [float(np.float32(0.1))] * 4 and g == 3.0 and isinstance(g, float)
    f, _ = check_cashflow(np.array([1, -2, 3]), None, 3)
    assert f.tolist() == [1.0, -2.0, 3.0]
    f, _ = check_cashflow(-5, None, 0)
    assert f.shape == (0,)
    f, _ = check_cashflow([], None, 0)
    assert f.shape == (0,)


# ---- 5. a market without noise: every path is the same annuity ----------------------------------------------------------------

def _annuity(v0, rho, flows):
    """The scalar binary32 loop of SPEC.md 4.7 -> (values after every step, the step of ruin or None)."""
    one = lambda x: np.array([x], np.float32)   # noqa: E731
    V, out, ruin = np.float32(v0), [], None
    for s, c in enumerate(flows, 1):
        U = np.float32(_fma32(one(V), one(rho), one(V))[0] + np.float32(c))
        V = U if V > 0 and U > 0 else np.float32(0.0)
        if V == 0 and ruin is None:
            ruin = s
        out.append(V)
    return np.array(out, np.float32), ruin


@pytest.mark.parametrize("v0,c,want_ruin", [(1.0, -0.06, True), (1.0, 0.02, False), (100.0, -7.5, True), (1.0, -0.001, False)])
def test_degenerate_market_is_a_scalar_annuity(v0, c, want_ruin):
    N, T = 3, 40
    mu32 = np.array([0.004, 0.001, 0.002], np.float32)
    W32 = np.array([[0.5, 0.25, 0.25]], np.float32)
    flows = np.full(T, c, np.float32)
    flows[30] = np.float32(abs(c) * 50)                               # a late windfall must not revive a ruined path
    hz = list(range(1, T + 1))
    got = simulate_cf(flows, W32, T, SEED, np.arange(5, dtype=np.uint64), mu=mu32, chol=np.zeros((N, N), np.float32), v0=v0, horizons=hz)
    rho = got["rho"][0, 0, 0]
    assert np.all(got["rho"] == rho)                                  # no noise: one return, every step and path
    want, ruin = _annuity(v0, rho, flows)
    assert (ruin is not None) == want_ruin
    for p in range(5):
        assert np.array_equal(got["V_h"][:, 0, p].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["V_T"][0].view(np.uint32), np.repeat(want[-1:], 5).view(np.uint32))
    if want_ruin:
        assert ruin < 30 and np.all(want[:ruin - 1] > 0) and np.all(want[ruin - 1:] == 0) and not np.any(np.signbit(want))
        assert counts_of(got["V_h"][:, 0, :])[:, 0].tolist() == [0] * (ruin - 1) + [5] * (T - ruin + 1)
    else:
        assert np.all(want > 0) and counts_of(got["V_T"])[0, 0] == 0
    assert counts_of(got["V_T"], target=v0)[0, 1] == (5 if want[-1] < np.float32(v0) else 0)


def test_walk_rules_by_hand():
    rho = np.array([[[0.5, -2.0, np.nan, 0.1], [0.5, 0.5, 0.5, 0.1]]], np.float32).transpose(0, 2, 1)   # [K=1, T=4, n=2]
    VT, Vh = walk(rho, np.array([0.0, 0.0, 0.0, 1.0], np.float32), 1.0, horizons=[1, 2, 3, 4])
    assert Vh[:, 0, 0].tolist() == [1.5, 0.0, 0.0, 0.0]              # 1.5 (1 - 2) < 0: ruin; NaN and the deposit leave it at +0
    last = np.float32(_fma32(np.array([3.375], np.float32), np.array([0.1], np.float32), np.array([3.375], np.float32))[0] + np.float32(1.0))
    assert Vh[:, 0, 1].tolist() == [1.5, 2.25, 3.375, float(last)]
    assert VT[0, 0] == 0.0 and not np.signbit(VT[0, 0]) and VT[0, 1] > 4.7
    VT, _ = walk(np.full((1, 1, 1), np.nan, np.float32), np.zeros(1, np.float32), 1.0)
    assert VT[0, 0] == 0.0                                            # a NaN U is ruin
    VT, _ = walk(np.zeros((1, 1, 1), np.float32), np.array([-1.0], np.float32), 1.0)
    assert VT[0, 0] == 0.0                                            # U = 0 exactly is ruin (U > 0 fails)

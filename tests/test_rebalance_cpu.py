"""CPU checks of buy-and-hold and periodic rebalancing (SPEC.md 4.5 / 5.4): the new C ABI symbols, argument errors with no
device, the pivots against NumPy and against the constant-weight pivots at period 1, the rules of the NumPy restatement in
rebalance_ref.py (period 1 is the constant-weight recurrence, it equals tracking dollar holdings, the cost sometimes does
nothing) and the Python argument checks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bootstrap_ref import simulate_boot
from horizons_ref import simulate_horizons
from monte_carlo_portfolio_amd import _ffi, synthetic
from monte_carlo_portfolio_amd.simulate import prepare_inputs
from rebalance_ref import boot_returns, dollar_holdings, gauss_returns, reb_pivots, rebalanced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mcp_simulate_rebalanced", "mcp_rebalance_pivots")
SEED = 0x5EB_A1A2CE


def test_new_symbols_in_header_binding_and_library(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcport.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text)
        assert name in _ffi.SIGNATURES
        assert hasattr(mcp_lib, name)
    assert re.search(r"typedef struct \{\s*int32_t period;\s*int32_t reserved;\s*double cost;\s*\} mcp_rebalance;", text)
    assert ctypes.sizeof(_ffi.McpRebalance) == 16
    assert _ffi.MCP_ABI_VERSION == 4 == mcp_lib.mcp_abi_version()


def _raw(name):
    fn = getattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    fn.restype = ctypes.c_int
    return fn


def _call(prm, reb, source="gauss", hz=(), levels=(), hz_stats=None, bands=None, horizon_out=False, stats=True, W=True):
    """mcp_simulate_rebalanced with a NULL context through an untyped handle (NULL pointers anywhere)."""
    N, K = prm.n_assets, prm.n_portfolios
    mu = np.full(N, 1e-3, np.float32)
    L = np.eye(N, dtype=np.float32) * 0.01
    rows = np.full((10, N), 0.01, np.float32)
    bt = _ffi.make_bootstrap(rows, 2.0)
    Wm = np.full((K, N), 1.0 / N, np.float32)
    st = np.zeros(K, _ffi.STATS_DTYPE)
    h = np.asarray(hz, np.int32)
    lv = np.asarray(levels, np.float64)
    hs = np.zeros(max(1, h.size * K), _ffi.STATS_DTYPE)
    bb = np.zeros(max(1, h.size * K * lv.size), np.float64)
    ho = np.zeros(max(1, h.size * K * 100), np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    if hz_stats is None:
        hz_stats = h.size > 0
    if bands is None:
        bands = lv.size > 0
    mu_p = vp(mu) if source in ("gauss", "both", "mu") else None
    L_p = vp(L) if source in ("gauss", "both") else None
    b_p = ctypes.byref(bt) if source in ("boot", "both", "mu") else None
    return _raw("mcp_simulate_rebalanced")(
        None, ctypes.byref(prm), ctypes.byref(reb) if reb is not None else None, mu_p, L_p, b_p, vp(Wm) if W else None,
        ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100), h.size, vp(h) if h.size else None, lv.size,
        vp(lv) if lv.size else None, None, vp(st) if stats else None, vp(ho) if horizon_out else None,
        vp(hs) if hz_stats else None, vp(bb) if bands else None)


BAD_RULES = [  # (period, reserved, cost, what the error names)
    (-1, 0, 0.0, "period"), (-(2 ** 31), 0, 0.0, "period"), (3, 1, 0.0, "reserved"), (3, 0, float("nan"), "cost"),
    (3, 0, -1e-9, "cost"), (3, 0, 1.0, "cost"), (3, 0, float("inf"), "cost"), (0, 0, 2.5, "cost"),
]


@pytest.mark.parametrize("period,reserved,cost,what", BAD_RULES)
@pytest.mark.parametrize("source", ["gauss", "boot"])
def test_bad_rules_return_e_arg_with_a_null_context(period, reserved, cost, what, source, mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    assert _call(prm, _ffi.McpRebalance(period, reserved, cost), source) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    assert _call(prm, _ffi.McpRebalance(period, reserved, cost), source, hz=[2, 5], levels=[50.0]) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error()
    piv = np.zeros(1, np.float64)
    assert _raw("mcp_rebalance_pivots")(ctypes.byref(prm), ctypes.byref(_ffi.McpRebalance(period, reserved, cost)),
                                        np.ones(4, np.float32).ctypes.data_as(ctypes.c_void_p), None,
                                        np.ones(4, np.float32).ctypes.data_as(ctypes.c_void_p),
                                        piv.ctypes.data_as(ctypes.c_void_p)) == _ffi.MCP_E_ARG


def test_draw_source_null_pointers_and_a_null_context(mcp_lib):
    prm = _ffi.make_params(4, 10, 2)
    ok = _ffi.McpRebalance(3, 0, 1e-3)
    assert _call(prm, None) == _ffi.MCP_E_ARG and b"rebalance is NULL" in mcp_lib.mcp_last_error()
    for src in ("both", "none", "mu"):                  # mu + chol + boot; nothing; mu + boot without chol
        assert _call(prm, ok, src) == _ffi.MCP_E_ARG
        assert b"exactly one draw source" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, W=False) == _ffi.MCP_E_ARG and b"NULL pointer" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, stats=False) == _ffi.MCP_E_ARG and b"NULL pointer" in mcp_lib.mcp_last_error()
    for src in ("gauss", "boot"):                       # every argument valid: the context is NULL
        assert _call(prm, ok, src) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()
        assert _call(prm, _ffi.McpRebalance(0, 0, 0.0), src, hz=[1, 10], levels=[5.0, 95.0], horizon_out=True) == _ffi.MCP_E_ARG
        assert b"ctx is NULL" in mcp_lib.mcp_last_error()
    assert _call(_ffi.make_params(4, -1, 1), ok) == _ffi.MCP_E_ARG and b"n_steps" in mcp_lib.mcp_last_error()


@pytest.mark.parametrize("kw", [{"compounding": "log"}, {"fold": True}, {"native_math": True}])
@pytest.mark.parametrize("source", ["gauss", "boot"])
def test_log_fold_and_native_math_are_unsupported(kw, source, mcp_lib):
    prm = _ffi.make_params(4, 10, 1, **kw)
    assert _call(prm, _ffi.McpRebalance(3, 0, 0.0), source) == _ffi.MCP_E_UNSUPPORTED
    assert _call(prm, _ffi.McpRebalance(3, 0, 0.0), source, hz=[2, 5]) == _ffi.MCP_E_UNSUPPORTED


BAD_HZ = [  # (horizons, levels, hz_stats pointer, bands pointer, horizon_out, what)
    ([], [50.0], False, True, False, "n_horizons = 0"), ([], [], True, False, False, "n_horizons = 0"),
    ([], [], False, False, True, "n_horizons = 0"), ([3, 2], [], None, None, False, "increasing"),
    ([0, 3], [], None, None, False, "outside"), ([5, 11], [], None, None, False, "outside"),
    ([1, 2], [-1.0], None, None, False, "level"), ([1, 2], [50.0] * 17, None, None, False, "n_levels"),
    ([1, 2], [50.0], False, None, False, "hz_stats_out"), ([1, 2], [50.0], None, False, False, "bands_out"),
    ([1, 2], [], None, True, False, "bands_out"), (list(range(1, 66)), [], None, None, False, "n_horizons"),
]


@pytest.mark.parametrize("hz,levels,hs,bands,ho,what", BAD_HZ)
def test_bad_horizons_return_e_arg_with_a_null_context(hz, levels, hs, bands, ho, what, mcp_lib):
    prm = _ffi.make_params(4, 10 if len(hz) < 60 else 70, 1)
    assert _call(prm, _ffi.McpRebalance(2, 0, 0.0), hz=hz, levels=levels, hz_stats=hs, bands=bands, horizon_out=ho) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()


def _market(N, K, seed=0):
    rng = np.random.default_rng(seed + 17 * N + K)
    mu = rng.normal(4e-4, 3e-4, N).astype(np.float32)
    A = rng.normal(size=(N, N)) * 0.01
    L = np.linalg.cholesky(A @ A.T + 1e-5 * np.eye(N)).astype(np.float32)
    W = rng.dirichlet(np.ones(N), K).astype(np.float32)
    W[-1, 0] -= 0.3                                     # a short position and some cash
    return mu, L, W


def _rows(R, N, seed=0):
    return (np.random.default_rng(seed + R * 7 + N).standard_t(4, size=(R, N)) * 0.03 + 0.004).astype(np.float32)


@pytest.mark.parametrize("T", [0, 1, 7, 12, 60, 252])
@pytest.mark.parametrize("period", [0, 1, 2, 5, 21, 252, 1000])
def test_pivots_match_numpy(T, period, mcp_lib):
    for N, K in [(1, 1), (3, 4), (16, 3), (33, 2)]:
        mu, L, W = _market(N, K, T)
        got = _ffi.rebalance_pivots(_ffi.make_params(N, T, K), period, W, mu=mu)
        want = reb_pivots(W, T, period, mu=mu)
        assert np.allclose(got, want, rtol=1e-14, atol=0.0), (N, K, got, want)
        rows = _rows(57, N, T)
        got = _ffi.rebalance_pivots(_ffi.make_params(N, T, K), period, W, rows=rows, cost=0.5)   # the cost is ignored
        want = reb_pivots(W, T, period, rows=rows)
        assert np.allclose(got, want, rtol=1e-14, atol=0.0), (N, K, got, want)
        if T == 0:
            assert np.all(got == 0.0)


@pytest.mark.parametrize("T", [1, 7, 252])
def test_period_one_pivots_are_the_constant_weight_pivots(T, mcp_lib):
    """The formulas agree at m = 1; the evaluation order differs (per asset, then per portfolio)."""
    for N, K in [(1, 1), (5, 4), (16, 3), (64, 2)]:
        mu, L, W = _market(N, K, 1)
        prm = _ffi.make_params(N, T, K)
        got = _ffi.rebalance_pivots(prm, 1, W, mu=mu)
        want = _ffi.pivots(prm, mu, L, W)
        assert np.all(np.abs(got - want) <= np.maximum(1e-12 * np.abs(want), 1e-15)), (got, want)
        rows = _rows(300, N, 1)
        got = _ffi.rebalance_pivots(prm, 1, W, rows=rows)
        want = _ffi.bootstrap_pivots(prm, rows, W)
        assert np.all(np.abs(got - want) <= np.maximum(1e-12 * np.abs(want), 1e-15)), (got, want)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("N,K,T", [(1, 1, 7), (3, 3, 12), (16, 2, 30), (17, 1, 5)])
def test_period_one_without_cost_is_the_constant_weight_recurrence(N, K, T):
    """Property 1: with m = 1 and kappa = 0, B_i is r_i after every step and rho^ is SPEC.md 4's rho, bit for bit."""
    mu, L, W = _market(N, K, 5)
    paths = np.array([0, 1, 2, 77, (1 << 32) - 1, (1 << 32) + 5], np.uint64)
    hz = [1, T // 2, T] if T > 2 else [1, T]
    want = simulate_horizons(mu, L, W, T, SEED, paths, hz, v0=3.0)
    got = rebalanced(gauss_returns(mu, L, T, SEED, paths), W, 1, 0.0, v0=3.0, horizons=hz)
    assert np.array_equal(_bits(got["V_T"]), _bits(want["V_T"]))
    assert np.array_equal(_bits(got["V_h"]), _bits(want["V_h"]))
    rows = _rows(40, N, 5)
    want = simulate_boot(rows, W, T, SEED, paths, 2.5, v0=3.0, horizons=hz)
    got = rebalanced(boot_returns(rows, T, SEED, paths, 2.5), W, 1, 0.0, v0=3.0, horizons=hz)
    assert np.array_equal(_bits(got["V_T"]), _bits(want["V_T"]))
    assert np.array_equal(_bits(got["V_h"]), _bits(want["V_h"]))


@pytest.mark.parametrize("period,cost", [(0, 0.0), (1, 0.0), (21, 0.0), (1, 1e-3), (21, 1e-3), (5, 1e-2)])
def test_the_recurrence_equals_tracking_dollar_holdings(period, cost, capsys):
    """Property 3 at T = 252, N = 16: the binary32 recurrence against a binary64 evaluation of the same draws that tracks the
    dollar holdings of every asset."""
    mu, cov = synthetic.synthetic_market(16)
    mu32, L, W = prepare_inputs(mu, cov, synthetic.dirichlet_weights(16, 2))
    W = W.copy()
    W[1] *= 0.8                                         # 20 % cash
    paths = np.arange(0, 400, dtype=np.uint64)
    r = gauss_returns(mu32, L, 252, SEED, paths)
    got = rebalanced(r, W, period, cost)["V_T"].astype(np.float64)
    want = dollar_holdings(r, W, period, cost)
    rel = np.abs(got - want) / np.abs(want)
    with capsys.disabled():
        print(f"\n  m={period} kappa={cost}: relative difference to dollar holdings rms {np.sqrt(np.mean(rel ** 2)):.2e} "
              f"max {rel.max():.2e}")
    assert rel.max() <= 1e-5


def test_the_cost_sometimes_does_nothing():
    """Property 2: no effect without rebalance dates (m = 0, m >= T), and none for one asset of weight 1 (tau = 0)."""
    mu, L, W = _market(5, 3, 9)
    paths = np.arange(0, 64, dtype=np.uint64)
    r = gauss_returns(mu, L, 20, SEED, paths)
    for m in (0, 20, 25):
        assert np.array_equal(_bits(rebalanced(r, W, m, 0.0)["V_T"]), _bits(rebalanced(r, W, m, 0.2)["V_T"]))
    one = np.array([[0.0, 0.0, 1.0, 0.0, 0.0]], np.float32)
    for m in (1, 3):
        assert np.array_equal(_bits(rebalanced(r, one, m, 0.0)["V_T"]), _bits(rebalanced(r, one, m, 0.2)["V_T"]))
    lower = rebalanced(r, W, 3, 0.2)["V_T"]
    assert np.all(lower <= rebalanced(r, W, 3, 0.0)["V_T"]) and np.any(lower < rebalanced(r, W, 3, 0.0)["V_T"])


def test_horizon_values_are_the_terminal_values_of_shorter_calls():
    """SPEC.md 4.3's promise holds for rebalanced paths: V_h is taken before any trade of step h."""
    mu, L, W = _market(6, 2, 3)
    paths = np.arange(0, 32, dtype=np.uint64)
    r = gauss_returns(mu, L, 12, SEED, paths)
    got = rebalanced(r, W, 4, 1e-3, horizons=[3, 4, 8, 11, 12])
    for i, h in enumerate([3, 4, 8, 11, 12]):
        assert np.array_equal(_bits(got["V_h"][i]), _bits(rebalanced(r[:h], W, 4, 1e-3)["V_T"])), h


def test_c99_compile_and_link_of_the_new_prototypes(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "rb.c"
    src.write_text(r'''
        #include <math.h>
        #include <stdio.h>
        #include "mcport.h"
        int main(void) {
            mcp_params p = {3, 12, 2, MCP_COMPOUND_SIMPLE, 0, 0, 1.0, 0.95, 0.0};
            float mu[3] = {0.01f, 0.002f, -0.001f}, chol[9] = {0.05f, 0, 0, 0.01f, 0.04f, 0, 0, 0, 0.03f};
            float w[6] = {0.5f, 0.3f, 0.2f, 0.2f, 0.3f, 0.5f};
            mcp_rebalance rb = {3, 0, 1e-3};
            int32_t hz[2] = {1, 6};
            double levels[2] = {5.0, 95.0}, bands[8], piv[2];
            mcp_stats st[2], hst[4];
            if (sizeof(mcp_rebalance) != 16) return 1;
            if (mcp_simulate_rebalanced(NULL, &p, &rb, mu, chol, NULL, w, 1, 0, 8, 0, NULL, 0, NULL, NULL, st, NULL, NULL, NULL)
                != MCP_E_ARG) return 2;
            if (mcp_simulate_rebalanced(NULL, &p, &rb, mu, chol, NULL, w, 1, 0, 8, 2, hz, 2, levels, NULL, st, NULL, hst, bands)
                != MCP_E_ARG) return 3;
            if (mcp_rebalance_pivots(&p, &rb, mu, NULL, w, piv) != MCP_OK || !(fabs(piv[0]) < 1.0)) return 4;
            rb.cost = 1.0;
            if (mcp_rebalance_pivots(&p, &rb, mu, NULL, w, piv) != MCP_E_ARG) return 5;
            printf("%s\n", mcp_last_error());
            return 0;
        }''')
    exe = tmp_path / "rb"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64", "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("kw,match", [
    ({"rebalance": 3, "drawdown": True}, "drawdown"), ({"rebalance": 3, "fold": True}, "fold"),
    ({"rebalance": "never", "native_math": True}, "native_math"), ({"rebalance": 1, "compounding": "log"}, "log"),
    ({"rebalance_cost": 1e-3}, "needs rebalance"), ({"rebalance": True}, "whole number"), ({"rebalance": 2.0}, "whole number"),
    ({"rebalance": 0}, "whole number"), ({"rebalance": -3}, "whole number"), ({"rebalance": "monthly"}, "whole number"),
    ({"rebalance": 2 ** 31}, "whole number"), ({"rebalance": 3, "rebalance_cost": 1.0}, r"\[0, 1\)"),
    ({"rebalance": 3, "rebalance_cost": -1e-4}, r"\[0, 1\)"), ({"rebalance": 3, "rebalance_cost": float("nan")}, r"\[0, 1\)"),
    ({"rebalance": 3, "rebalance_cost": True}, "number"),
])
def test_python_rejects_bad_calls_without_a_context(kw, match, monkeypatch):
    """The ValueError comes before any device (or the library) is touched."""
    from monte_carlo_portfolio_amd import simulate as sim

    def boom(*a, **k):
        raise AssertionError("a context was requested")
    monkeypatch.setattr(sim, "default_context", boom)
    mu, cov = synthetic.synthetic_market(3)
    with pytest.raises(ValueError, match=match):
        sim.simulate_paths(mu, cov, np.ones(3) / 3, n_steps=20, n_paths=8, **kw)
    boot_kw = {k: v for k, v in kw.items() if k not in ("drawdown", "fold", "native_math")}
    if boot_kw != kw:
        boot_kw["drawdown" if "drawdown" in kw else "fold" if "fold" in kw else "native_math"] = True
    with pytest.raises(ValueError, match=match if boot_kw == kw else "does not take"):
        sim.simulate_bootstrap(_rows(30, 3), np.ones(3) / 3, n_steps=20, n_paths=8, **boot_kw)

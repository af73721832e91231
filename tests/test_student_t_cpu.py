"""CPU checks of the Student-t draws (SPEC.md 2.2 / 4.6): the NumPy restatement in student_t_ref.py against the C oracle (s = 1)
and against the chi-square law, the new C ABI symbol and struct, argument errors with no device, the Python argument checks and
fit_student_t_dof."""
import ctypes
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import stats as sps

from monte_carlo_portfolio_amd import _ffi, fit_student_t_dof, synthetic
from monte_carlo_portfolio_amd import student_t as stmod
from monte_carlo_portfolio_amd.simulate import prepare_inputs
from student_t_ref import chi_and_scale, simulate_t, t_rho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
SEED = 0x57_0DE7


def test_unit_scale_restatement_is_the_c_oracle(oracle):
    mu, cov = synthetic.synthetic_market(5)
    W = synthetic.dirichlet_weights(5, 3)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    want = oracle.simulate(mu32, L, W32, 9, 200, SEED)
    got = simulate_t(mu32, L, W32, 9, SEED, np.arange(200, dtype=np.uint64), dof=5, unit_scale=True)["V_T"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("dof", [3, 5, 32])
def test_chi_is_chi_square(dof):
    chi, s = chi_and_scale(SEED, np.arange(100_000, dtype=np.uint64), 3, dof)
    assert sps.kstest(chi.astype(np.float64), sps.chi2(dof).cdf).pvalue > 1e-4
    assert np.array_equal(s, np.sqrt(np.float32(dof - 2) / chi).astype(np.float32))


def test_chi_masks_the_surplus_words_of_the_last_block():
    """nu = 5 .. 8 share nt = 2 and so the same blocks: chi grows with nu, term by term (k ascending); nu = 4 (nt = 1) does not."""
    p = np.arange(64, dtype=np.uint64)
    c = {nu: chi_and_scale(SEED, p, 2, nu)[0] for nu in range(3, 9)}
    assert np.all(c[4] >= c[3]) and np.all(c[6] >= c[5]) and np.all(c[7] >= c[6]) and np.all(c[8] >= c[7])
    assert not np.array_equal(c[5], c[8]) and not np.all(c[5] >= c[4])


def test_one_step_covariance_matches_sigma_at_nu_10():
    mu, cov = synthetic.synthetic_market(3)
    mu32, L, _ = prepare_inputs(mu, cov, np.ones(3) / 3)
    n = 40_000
    r = t_rho(mu32, L, np.eye(3, dtype=np.float32), 1, SEED, np.arange(n, dtype=np.uint64), 10)[:, 0, :].astype(np.float64)
    S = L.astype(np.float64) @ L.astype(np.float64).T
    C = np.cov(r)
    d = r - r.mean(axis=1, keepdims=True)
    for i in range(3):
        for j in range(3):
            se = np.std(d[i] * d[j]) / np.sqrt(n)
            assert abs(C[i, j] - S[i, j]) < 5 * se, (i, j, C[i, j], S[i, j], se)
        se_m = np.sqrt(S[i, i] / n)
        assert abs(r[i].mean() - mu32[i]) < 5 * se_m


def test_struct_symbol_and_header(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcport.h")).read(), flags=re.S)
    assert re.search(r"\bmcp_simulate_student_t\s*\(", text)
    assert re.search(r"typedef struct \{\s*int32_t dof;\s*int32_t reserved;\s*\} mcp_student_t;", text)
    assert re.search(r"#define MCP_MAX_T_DOF 32\b", text)
    assert "mcp_simulate_student_t" in _ffi.SIGNATURES and hasattr(mcp_lib, "mcp_simulate_student_t")
    assert ctypes.sizeof(_ffi.McpStudentT) == 8 and _ffi.MCP_MAX_T_DOF == 32
    assert _ffi.MCP_ABI_VERSION == 4 == mcp_lib.mcp_abi_version()


def _raw():
    fn = ctypes.CDLL(_ffi.LIB_PATH).mcp_simulate_student_t
    fn.restype = ctypes.c_int
    return fn


def _call(prm, st, hz=(), levels=(), dd=False, mdd=False, hz_stats=None, bands=None, stats=True, mu=True, W=True):
    """mcp_simulate_student_t with a NULL context through an untyped handle (NULL pointers anywhere)."""
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
    hz_stats = h.size > 0 if hz_stats is None else hz_stats
    bands = lv.size > 0 if bands is None else bands
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    return _raw()(None, ctypes.byref(prm), ctypes.byref(st) if st is not None else None, vp(m) if mu else None, vp(L),
                  vp(Wm) if W else None, ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100), h.size,
                  vp(h) if h.size else None, lv.size, vp(lv) if lv.size else None, None, vp(s) if stats else None,
                  vp(md) if mdd else None, vp(ds) if dd else None, None, vp(hs) if hz_stats else None, vp(bb) if bands else None)


@pytest.mark.parametrize("dof,reserved,what", [(2, 0, "dof"), (33, 0, "dof"), (0, 0, "dof"), (-5, 0, "dof"), (5, 1, "reserved")])
def test_bad_requests_return_e_arg_with_a_null_context(dof, reserved, what, mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    assert _call(prm, _ffi.McpStudentT(dof, reserved)) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    assert _call(prm, _ffi.McpStudentT(dof, reserved), hz=[2, 5], levels=[50.0]) == _ffi.MCP_E_ARG
    assert _call(prm, _ffi.McpStudentT(dof, reserved), dd=True) == _ffi.MCP_E_ARG


@pytest.mark.parametrize("N", [1, 4])
def test_the_counter_bound_of_stream_two(N, mcp_lib):
    prm = _ffi.make_params(N, 2 ** 29, 1)                # T ceil(N/4) = 2^29 fits; T ceil(32/4) = 2^32 does not
    assert _call(prm, _ffi.McpStudentT(32, 0)) == _ffi.MCP_E_ARG
    assert b"stream 2" in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    assert _call(prm, _ffi.McpStudentT(28, 0)) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()


def test_null_pointers_and_a_null_context(mcp_lib):
    prm = _ffi.make_params(4, 10, 2)
    ok = _ffi.McpStudentT(5, 0)
    assert _call(prm, None) == _ffi.MCP_E_ARG and b"student_t is NULL" in mcp_lib.mcp_last_error()
    for kw in ({"mu": False}, {"W": False}, {"stats": False}):
        assert _call(prm, ok, **kw) == _ffi.MCP_E_ARG and b"NULL pointer" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, mdd=True) == _ffi.MCP_E_ARG and b"mdd_out" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, hz_stats=True) == _ffi.MCP_E_ARG and b"n_horizons = 0" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, hz=[3, 2]) == _ffi.MCP_E_ARG and b"increasing" in mcp_lib.mcp_last_error()
    assert _call(prm, ok, hz=[1, 2], levels=[50.0], hz_stats=False) == _ffi.MCP_E_ARG
    for kw in ({}, {"dd": True}, {"dd": True, "mdd": True}, {"hz": [1, 10], "levels": [5.0, 95.0]}):   # all valid: the context is NULL
        assert _call(prm, ok, **kw) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()


@pytest.mark.parametrize("kw", [{"compounding": "log"}, {"fold": True}, {"native_math": True}])
def test_log_fold_and_native_math_are_unsupported(kw, mcp_lib):
    prm = _ffi.make_params(4, 10, 1, **kw)
    assert _call(prm, _ffi.McpStudentT(5, 0)) == _ffi.MCP_E_UNSUPPORTED
    assert _call(prm, _ffi.McpStudentT(5, 0), hz=[2, 5]) == _ffi.MCP_E_UNSUPPORTED


def test_drawdown_with_horizons_is_unsupported(mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    assert _call(prm, _ffi.McpStudentT(5, 0), hz=[2, 5], dd=True) == _ffi.MCP_E_UNSUPPORTED
    assert b"horizons and the drawdown" in mcp_lib.mcp_last_error()


def test_c99_compile_and_link_of_the_new_prototype(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "st.c"
    src.write_text(r'''
        #include <stdio.h>
        #include "mcport.h"
        int main(void) {
            mcp_params p = {3, 12, 2, MCP_COMPOUND_SIMPLE, 0, 0, 1.0, 0.95, 0.0};
            float mu[3] = {0.01f, 0.002f, -0.001f}, chol[9] = {0.05f, 0, 0, 0.01f, 0.04f, 0, 0, 0, 0.03f};
            float w[6] = {0.5f, 0.3f, 0.2f, 0.2f, 0.3f, 0.5f};
            mcp_student_t st = {5, 0};
            mcp_stats s[2], d[2];
            if (sizeof(mcp_student_t) != 8 || MCP_MAX_T_DOF != 32) return 1;
            if (mcp_simulate_student_t(NULL, &p, &st, mu, chol, w, 1, 0, 8, 0, NULL, 0, NULL, NULL, s, NULL, d, NULL, NULL, NULL)
                != MCP_E_ARG) return 2;
            st.dof = 2;
            if (mcp_simulate_student_t(NULL, &p, &st, mu, chol, w, 1, 0, 8, 0, NULL, 0, NULL, NULL, s, NULL, NULL, NULL, NULL, NULL)
                != MCP_E_ARG) return 3;
            printf("%s\n", mcp_last_error());
            return 0;
        }''')
    exe = tmp_path / "st"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def _rows(R, N, seed=0):
    return np.random.default_rng(seed).normal(0.0, 0.02, size=(R, N))


@pytest.mark.parametrize("kw,match", [
    ({"dof": True}, "integer"), ({"dof": 5.5}, "integer"), ({"dof": "5"}, "integer"), ({"dof": 2}, "integer"),
    ({"dof": 33}, "integer"), ({"dof": float("nan")}, "integer"), ({"dof": 5, "compounding": "log"}, "log"),
    ({"dof": 5, "fold": True}, "fold"), ({"dof": 5, "native_math": True}, "native_math"), ({"dof": 5, "rebalance": 3}, "rebalance"),
    ({"dof": 5, "drawdown": True, "horizons": [2, 5]}, "horizons"),
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


def test_simulate_bootstrap_rejects_dof(monkeypatch):
    from monte_carlo_portfolio_amd import simulate as sim
    monkeypatch.setattr(sim, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("context")))
    with pytest.raises(ValueError, match=r"does not take \['dof'\].*simulate_paths\(dof="):
        sim.simulate_bootstrap(_rows(30, 3), np.ones(3) / 3, n_steps=20, n_paths=8, dof=5)


def _t_rows(nu, R, N, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(N, N))
    S = A @ A.T / N + 0.1 * np.eye(N)
    z = rng.standard_normal((R, N)) @ np.linalg.cholesky(S).T
    if nu is None:
        return 0.01 + z
    return 0.01 + z * np.sqrt((nu - 2) / rng.chisquare(nu, R))[:, None]


@pytest.mark.parametrize("nu", [3, 4, 6])
def test_fit_recovers_nu(nu):
    assert fit_student_t_dof(_t_rows(nu, 20_000, 3, nu)) == nu


def test_fit_gives_32_on_gaussian_rows():
    assert fit_student_t_dof(_t_rows(None, 20_000, 3, 7)) == 32


def test_fit_on_the_weekly_btc_and_eth_rows():
    import monte_carlo_portfolio_amd as mcp
    files = []
    for f in ("BTC_USD 7 Years Weekly.csv", "ETH_USD 7 Years Weekly.csv"):
        b = io.BytesIO(open(os.path.join(DATA, f), "rb").read())
        b.name = f
        files.append(b)
    _, _, res = mcp.load_prices(files, resample_rule="W", report=lambda m: None)
    rets = mcp.returns_matrix(res)
    assert rets.shape[0] > 300
    assert fit_student_t_dof(rets) <= 8
    for i in range(2):
        assert fit_student_t_dof(rets.iloc[:, i]) <= 8


def test_fit_input_errors():
    good = _rows(40, 3)
    bad = good.copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        fit_student_t_dof(bad)
    with pytest.raises(ValueError, match="N \\+ 2"):
        fit_student_t_dof(good[:4])
    with pytest.raises(ValueError, match="positive definite"):
        fit_student_t_dof(np.column_stack([good[:, 0], good[:, 0], good[:, 1]]))
    for dofs in ([2, 5], [5, 33], [True], [4.5], []):
        with pytest.raises(ValueError):
            fit_student_t_dof(good, dofs=dofs)


def test_fit_breaks_ties_toward_the_smaller_nu(monkeypatch):
    x = _t_rows(5, 2_000, 2, 3)
    assert fit_student_t_dof(x, dofs=[9, 4, 30, 4]) == fit_student_t_dof(x, dofs=[4, 9, 30])
    monkeypatch.setattr(stmod._Fit, "loglik", lambda self, nu: 0.0)
    assert fit_student_t_dof(x, dofs=[12, 7, 20]) == 7
    assert fit_student_t_dof(x) == 3


def test_fit_is_the_maximum_of_the_loglik():
    x = _t_rows(5, 3_000, 2, 11)
    ll = {nu: stmod.student_t_loglik(x, nu) for nu in range(3, 33)}
    assert fit_student_t_dof(x) == max(ll, key=lambda nu: (ll[nu], -nu))
    # the N = 1 log-likelihood is scipy's t with scale sqrt(Sigma_hat (nu - 2) / nu)
    y = x[:, 0]
    s = np.sqrt(np.var(y, ddof=1) * 3.0 / 5.0)
    assert stmod.student_t_loglik(y, 5) == pytest.approx(np.sum(sps.t.logpdf(y, 5, loc=y.mean(), scale=s)), rel=1e-10)

"""CPU checks of the stationary block bootstrap (SPEC.md 2.1 / 4.4 / 5.3): the new C ABI symbols, argument errors with no
device, the pivots against the formula, the rules of the NumPy restatement in bootstrap_ref.py (on the reference-made collar
matrix too) and the Python argument checks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bootstrap_ref import boot_indices, boot_pivots, row_returns, simulate_boot, start_index, step_words, threshold
from monte_carlo_portfolio_amd import _ffi

ROOT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(ROOT)
NEW_SYMBOLS = ("mcp_simulate_bootstrap", "mcp_simulate_bootstrap_horizons", "mcp_bootstrap_pivots")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_script_arrays.npz")


def collar_returns():
    """The reference's own returns matrix of a collar overlay (monthly, seed 12345): kinked, not Gaussian."""
    return np.load(GOLDEN)["monthly_collar_seed12345__returns_df"].astype(np.float64)


def test_new_symbols_in_header_binding_and_library(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcport.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text)
        assert name in _ffi.SIGNATURES
        assert hasattr(mcp_lib, name)
    assert re.search(r"#define MCP_MAX_BOOT_ROWS \(1 << 20\)", text)
    assert re.search(r"typedef struct \{\s*const float \*rows;\s*int32_t n_rows;\s*int32_t reserved;\s*double mean_block;\s*\} mcp_bootstrap;",
                     text)
    assert _ffi.MCP_MAX_BOOT_ROWS == 1 << 20
    assert ctypes.sizeof(_ffi.McpBootstrap) == 24
    assert _ffi.MCP_ABI_VERSION == 4 == mcp_lib.mcp_abi_version()


def _rows(R=10, N=4, fill=0.01):
    return np.full((R, N), fill, np.float32)


def _boot_call(lib, ctx, prm, boot, W=True, stats=True):
    Wm = np.full((prm.n_portfolios, prm.n_assets), 1.0 / prm.n_assets, np.float32)
    st = np.zeros(max(1, prm.n_portfolios), _ffi.STATS_DTYPE)
    bp = ctypes.byref(boot) if boot is not None else None
    if not W:                                   # the binding's W is an ndarray: a NULL W goes through an untyped handle
        raw = ctypes.CDLL(_ffi.LIB_PATH).mcp_simulate_bootstrap
        raw.restype = ctypes.c_int
        return raw(ctx, ctypes.byref(prm), bp, None, ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100), None,
                   st.ctypes.data_as(ctypes.c_void_p))
    return lib.mcp_simulate_bootstrap(ctx, ctypes.byref(prm), bp, Wm, 1, 0, 100, None,
                                      st.ctypes.data_as(ctypes.c_void_p) if stats else None)


def _hz_call(lib, ctx, prm, boot, hz, levels, bands=None):
    Wm = np.full((1, prm.n_assets), 1.0 / prm.n_assets, np.float32)
    st = np.zeros(1, _ffi.STATS_DTYPE)
    h = np.asarray(hz, np.int32)
    lv = np.asarray(levels, np.float64)
    hs = np.zeros(max(1, h.size), _ffi.STATS_DTYPE)
    b = np.zeros(max(1, h.size * lv.size), np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    if bands is None:
        bands = lv.size > 0
    return lib.mcp_simulate_bootstrap_horizons(ctx, ctypes.byref(prm), ctypes.byref(boot), Wm, 1, 0, 100, h.size,
                                               vp(h) if h.size else None, lv.size, vp(lv) if lv.size else None, None, vp(st),
                                               None, vp(hs), vp(b) if bands else None)


def _bad_tables():
    nan_rows = _rows()
    nan_rows[3, 2] = np.nan
    inf_rows = _rows()
    inf_rows[9, 0] = -np.inf
    ok = _rows()
    return [  # (rows or None, n_rows, mean_block, what the error names)
        (None, 10, 1.0, "rows is NULL"), (ok, 0, 1.0, "n_rows"), (ok, -3, 1.0, "n_rows"), (ok, (1 << 20) + 1, 1.0, "n_rows"),
        (nan_rows, 10, 1.0, "not finite"), (inf_rows, 10, 1.0, "not finite"), (ok, 10, 0.999, "mean_block"),
        (ok, 10, 0.0, "mean_block"), (ok, 10, -np.inf, "mean_block"), (ok, 10, float("nan"), "mean_block"),
    ]


@pytest.mark.parametrize("case", range(10))
def test_bad_tables_return_e_arg_with_a_null_context(case, mcp_lib):
    rows, R, b, what = _bad_tables()[case]
    bt = _ffi.McpBootstrap(rows.ctypes.data_as(ctypes.c_void_p) if rows is not None else None, R, 0, b)
    prm = _ffi.make_params(4, 10, 1)
    assert _boot_call(mcp_lib, None, prm, bt) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()
    assert _hz_call(mcp_lib, None, prm, bt, [2, 5], [50.0]) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error()
    piv = np.zeros(1, np.float64)
    assert mcp_lib.mcp_bootstrap_pivots(ctypes.byref(prm), ctypes.byref(bt), np.ones((1, 4), np.float32), piv) == _ffi.MCP_E_ARG


def test_null_pointers_flags_and_a_null_context(mcp_lib):
    rows = _rows()
    bt = _ffi.make_bootstrap(rows, 2.0)
    prm = _ffi.make_params(4, 10, 1)
    assert _boot_call(mcp_lib, None, prm, None) == _ffi.MCP_E_ARG
    assert b"bootstrap is NULL" in mcp_lib.mcp_last_error()
    assert _boot_call(mcp_lib, None, prm, bt, W=False) == _ffi.MCP_E_ARG
    assert _boot_call(mcp_lib, None, prm, bt, stats=False) == _ffi.MCP_E_ARG
    assert _boot_call(mcp_lib, None, prm, bt) == _ffi.MCP_E_ARG              # every argument valid: the context is NULL
    assert b"ctx is NULL" in mcp_lib.mcp_last_error()
    assert _boot_call(mcp_lib, None, _ffi.make_params(4, 10, 1, compounding="log"), _ffi.make_bootstrap(rows, np.inf)) == _ffi.MCP_E_ARG
    assert b"ctx is NULL" in mcp_lib.mcp_last_error()
    bad_prm = _ffi.make_params(4, -1, 1)
    assert _boot_call(mcp_lib, None, bad_prm, bt) == _ffi.MCP_E_ARG
    for flags in ({"fold": True}, {"native_math": True}):
        prm_f = _ffi.make_params(4, 10, 1, **flags)
        assert _boot_call(mcp_lib, None, prm_f, bt) == _ffi.MCP_E_UNSUPPORTED
        assert _hz_call(mcp_lib, None, prm_f, bt, [2, 5], []) == _ffi.MCP_E_UNSUPPORTED


BAD_HZ = [([], [50.0], "n_horizons"), ([3, 2], [], "increasing"), ([0, 3], [], "outside"), ([5, 11], [], "outside"),
          ([1, 2], [-1.0], "level"), ([1, 2], [float("nan")], "level"), ([1, 2], [50.0] * 17, "n_levels")]


@pytest.mark.parametrize("hz,levels,what", BAD_HZ)
def test_bad_horizons_return_e_arg_with_a_null_context(hz, levels, what, mcp_lib):
    rows = _rows()
    bt = _ffi.make_bootstrap(rows, 3.0)
    prm = _ffi.make_params(4, 10, 1)
    assert _hz_call(mcp_lib, None, prm, bt, hz, levels) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()


def test_bands_pointer_must_match_the_levels(mcp_lib):
    rows = _rows()
    bt = _ffi.make_bootstrap(rows, 3.0)
    prm = _ffi.make_params(4, 10, 1)
    assert _hz_call(mcp_lib, None, prm, bt, [1, 5], [50.0], bands=False) == _ffi.MCP_E_ARG
    assert b"bands_out" in mcp_lib.mcp_last_error()
    assert _hz_call(mcp_lib, None, prm, bt, [1, 5], [], bands=True) == _ffi.MCP_E_ARG
    assert _hz_call(mcp_lib, None, prm, bt, [1, 5], [2.5, 97.5]) == _ffi.MCP_E_ARG
    assert b"ctx is NULL" in mcp_lib.mcp_last_error()


@pytest.mark.parametrize("mode", ["simple", "log"])
@pytest.mark.parametrize("T", [0, 1, 12, 252])
def test_pivots_match_the_formula(mode, T, mcp_lib):
    rng = np.random.default_rng(T + (mode == "log"))
    for R, N, K in [(1, 1, 1), (13, 3, 4), (300, 16, 3), (57, 33, 2)]:
        rows = (rng.standard_t(4, size=(R, N)) * 0.03 + 0.004).astype(np.float32)
        W = rng.dirichlet(np.ones(N), size=K).astype(np.float32)
        got = _ffi.bootstrap_pivots(_ffi.make_params(N, T, K, compounding=mode), rows, W)
        want = boot_pivots(rows, W, T, mode)
        assert np.allclose(got, want, rtol=1e-15, atol=0.0), (R, N, K, got, want)
        if T == 0:
            assert np.all(got == 0.0)


def test_collar_pivot_is_the_compounded_mean_of_the_historical_portfolio_rows(mcp_lib):
    ret = collar_returns()
    rows = ret.astype(np.float32)
    w = np.array([[0.5, 0.3, 0.2]], np.float32)
    port = rows.astype(np.float64) @ w[0].astype(np.float64)
    got = _ffi.bootstrap_pivots(_ffi.make_params(3, 12, 1), rows, w)[0]
    assert abs(got - np.expm1(12 * np.log1p(port.mean()))) <= 1e-15 * abs(got)


def test_threshold():
    assert threshold(1.0) == 1 << 32
    assert threshold(2.0) == 1 << 31
    assert threshold(np.inf) == 0
    assert threshold(3.0) == int(2.0 ** 32 / 3.0)
    assert threshold(1e300) == 0


SEED = 0x1234_5678_9ABC


def test_b1_restarts_at_every_step_and_the_index_is_the_mulhi_of_x0():
    paths = np.arange((1 << 32) - 40, (1 << 32) + 40, dtype=np.uint64)
    for R in (1, 7, 272, 100_000, 1 << 20):
        idx = boot_indices(SEED, paths, 9, R, 1.0)
        for t in range(9):
            x0, _ = step_words(SEED, paths, t)
            want = (x0.astype(object) * R) // (1 << 32)
            assert np.array_equal(idx[t], np.array(want, np.int64)), (R, t)
        assert idx.min() >= 0 and idx.max() < R


def test_b_inf_walks_consecutive_rows_circularly():
    paths = np.arange(0, 500, dtype=np.uint64)
    R = 13
    idx = boot_indices(SEED, paths, 40, R, np.inf)
    x0, _ = step_words(SEED, paths, 0)
    assert np.array_equal(idx[0], start_index(x0, R))
    for t in range(1, 40):
        assert np.array_equal(idx[t], (idx[t - 1] + 1) % R)


def test_mean_block_sets_the_restart_rate():
    paths = np.arange(0, 20_000, dtype=np.uint64)
    for b in (2.5, 12.0):
        idx = boot_indices(SEED, paths, 30, 1000, b)
        cont = (idx[1:] == (idx[:-1] + 1) % 1000)
        # a restart may land on the next row by chance (1/R); the continuation rate is 1 - 1/b
        assert abs(cont.mean() - (1 - 1 / b)) < 0.01, (b, cont.mean())
        _, x1 = step_words(SEED, paths, 5)
        restart = x1.astype(np.int64) < threshold(b)
        assert np.array_equal(idx[5][~restart], (idx[4][~restart] + 1) % 1000)


def test_one_step_iid_values_are_the_historical_portfolio_rows_of_the_collar():
    """T = 1, b = 1: every path's return is one of the reference's port_series values `returns_df @ ws` (app.py:710), in
    binary32 (the fma chain of SPEC.md 4.4 against the binary64 product: a few ulp)."""
    ret = collar_returns()
    rows = ret.astype(np.float32)
    w = np.array([0.5, 0.3, 0.2])
    port_series = ret @ w
    paths = np.arange(0, 4096, dtype=np.uint64)
    got = simulate_boot(rows, w.astype(np.float32), 1, SEED, paths, 1.0, "log")
    rr = got["row_rho"][0]
    assert np.array_equal(got["V_T"][0].view(np.uint32), rr[got["idx"][0]].view(np.uint32))
    assert np.allclose(rr.astype(np.float64), port_series, rtol=0, atol=4 * np.finfo(np.float32).eps * np.abs(ret).sum(axis=1).max())
    assert set(np.unique(got["idx"][0])) == set(range(rows.shape[0]))        # 4096 draws visit all 13 rows
    simple = simulate_boot(rows, w.astype(np.float32), 1, SEED, paths, 1.0, "simple")
    x = simple["V_T"][0].astype(np.float64) - 1.0
    assert x.min() >= np.float32(1.0 + rr.min()) - 1.0 and x.min() == float(np.float32(1.0 + rr.min())) - 1.0


def test_c99_compile_and_link_of_the_new_prototypes(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "bt.c"
    src.write_text(r'''
        #include <math.h>
        #include <stdio.h>
        #include "mcport.h"
        int main(void) {
            mcp_params p = {3, 12, 2, MCP_COMPOUND_SIMPLE, 0, 0, 1.0, 0.95, 0.0};
            float rows[12] = {0.01f, 0.02f, -0.01f, 0.0f, 0.01f, 0.02f, -0.02f, 0.0f, 0.01f, 0.03f, 0.01f, -0.01f};
            float w[6] = {0.5f, 0.3f, 0.2f, 0.2f, 0.3f, 0.5f};
            mcp_bootstrap bt = {rows, 4, 0, 2.5};
            int32_t hz[2] = {1, 6};
            double levels[2] = {5.0, 95.0}, bands[8], piv[2];
            mcp_stats st[2], hst[4];
            if (MCP_MAX_BOOT_ROWS != 1048576 || sizeof(mcp_bootstrap) != 24) return 1;
            if (mcp_simulate_bootstrap(NULL, &p, &bt, w, 1, 0, 8, NULL, st) != MCP_E_ARG) return 2;
            if (mcp_simulate_bootstrap_horizons(NULL, &p, &bt, w, 1, 0, 8, 2, hz, 2, levels, NULL, st, NULL, hst, bands) != MCP_E_ARG)
                return 3;
            if (mcp_bootstrap_pivots(&p, &bt, w, piv) != MCP_OK || !(fabs(piv[0]) < 1.0)) return 4;
            bt.mean_block = 0.5;
            if (mcp_bootstrap_pivots(&p, &bt, w, piv) != MCP_E_ARG) return 5;
            printf("%s\n", mcp_last_error());
            return 0;
        }''')
    exe = tmp_path / "bt"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64", "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("kw,match", [
    ({"block": 0.5}, "block"), ({"block": float("nan")}, "block"), ({"fold": True}, "fold"),
    ({"native_math": True}, "native_math"), ({"drawdown": True}, "drawdown"), ({"horizons": [3, 2]}, "increasing"),
    ({"horizons": [2, 21]}, "n_steps"), ({"bands": (50.0,)}, "horizons"), ({"returns": "nan"}, "NaN"),
    ({"returns": "narrow"}, "columns"), ({"returns": "empty"}, "R >= 1"),
])
def test_python_rejects_bad_bootstrap_calls_without_a_context(kw, match, monkeypatch):
    """The ValueError comes before any device (or the library) is touched."""
    from monte_carlo_portfolio_amd import simulate as sim

    def boom(*a, **k):
        raise AssertionError("a context was requested")
    monkeypatch.setattr(sim, "default_context", boom)
    returns = collar_returns()
    kind = kw.pop("returns", None)
    if kind == "nan":
        returns = returns.copy()
        returns[4, 1] = np.nan
    elif kind == "narrow":
        returns = returns[:, :2]
    elif kind == "empty":
        returns = returns[:0]
    args = dict(n_steps=20, n_paths=8)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        sim.simulate_bootstrap(returns, np.ones(3) / 3, **args)


def test_python_takes_a_dataframe(monkeypatch):
    pd = pytest.importorskip("pandas")
    from monte_carlo_portfolio_amd import simulate as sim
    ret = collar_returns()
    rows, W = sim.bootstrap_inputs(pd.DataFrame(ret, columns=["a", "b", "c"]), [0.2, 0.3, 0.5])
    assert rows.dtype == np.float32 and rows.flags.c_contiguous and np.array_equal(rows, ret.astype(np.float32))
    assert W.shape == (1, 3)
    assert np.array_equal(row_returns(rows, W).shape, (1, 13))

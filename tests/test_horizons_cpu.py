"""CPU checks of the values at intermediate horizons (SPEC.md 4.3 / 5.2): the NumPy restatement in horizons_ref.py against the
C oracle, the percentile rank of a level against np.percentile, the new C ABI symbols, argument errors with no device and the
Python argument checks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from horizons_ref import lerp_rank, simulate_horizons
from monte_carlo_portfolio_amd import _ffi, synthetic
from monte_carlo_portfolio_amd.simulate import prepare_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mcp_simulate_horizons", "mcp_launch_paths_horizons", "mcp_percentile_rank_q")


def _inputs(n, k):
    mu, cov = synthetic.synthetic_market(n)
    return prepare_inputs(mu, cov, synthetic.dirichlet_weights(n, k))


@pytest.mark.parametrize("n,mode", [(1, "simple"), (5, "log"), (16, "simple"), (16, "log")])
def test_helper_horizon_values_equal_the_oracle_at_n_steps_h(n, mode, oracle):
    """SPEC.md 4.3: the value after step h of a T-step walk is the terminal value of the same call with n_steps = h."""
    mu, L, W = _inputs(n, 3)
    T, n_paths, seed, begin = 20, 48, 424242, (1 << 32) - 20
    horizons = [1, 2, 7, 19, 20]
    got = simulate_horizons(mu, L, W, T, seed, np.arange(begin, begin + n_paths, dtype=np.uint64), horizons, mode, v0=3.0)
    for i, h in enumerate(horizons):
        ref = oracle.simulate(mu, L, W, h, n_paths, seed, path_begin=begin, compounding=mode, v0=3.0)
        assert np.array_equal(got["V_h"][i].view(np.uint32), ref.view(np.uint32)), h
    assert np.array_equal(got["V_h"][-1].view(np.uint32), got["V_T"].view(np.uint32))


QS = [0.0, 2.5, 5.0, 10.0, 25.0, 33.3, 50.0, 66.7, 75.0, 90.0, 95.0, 97.5, 99.0, 99.9, 100.0]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 13, 100, 1000, 4097, 100_003])
def test_percentile_rank_q_reproduces_np_percentile(n):
    rng = np.random.default_rng(n)
    for rep in range(2 if n > 10_000 else 10):
        x = rng.normal(size=n).astype(np.float32).astype(np.float64)
        xs = np.sort(x)
        for q in QS + list(rng.uniform(0, 100, size=5)):
            lo, hi, g = _ffi.percentile_rank_q(n, q)
            assert 0 <= lo <= hi <= n - 1
            assert lerp_rank(xs, lo, hi, g) == np.percentile(x, q), (n, q)


def test_percentile_rank_q_edges(mcp_lib):
    assert _ffi.percentile_rank_q(1, 50.0) == (0, 0, 0.0)
    assert _ffi.percentile_rank_q(1000, 0.0) == (0, 1, 0.0)
    assert _ffi.percentile_rank_q(1000, 100.0) == (999, 999, 0.0)
    assert _ffi.percentile_rank_q(1_000_001, 5.0) == (50_000, 50_001, 0.0)
    out = (ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double())
    for q in (-0.1, 100.5, float("nan")):
        assert mcp_lib.mcp_percentile_rank_q(10, q, *map(ctypes.byref, out)) == _ffi.MCP_E_ARG
    assert mcp_lib.mcp_percentile_rank_q(0, 50.0, *map(ctypes.byref, out)) == _ffi.MCP_E_ARG


def test_new_symbols_in_header_binding_and_library(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcport.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text)
        assert name in _ffi.SIGNATURES
        assert hasattr(mcp_lib, name)
    assert re.search(r"#define MCP_MAX_HORIZONS 64\b", text) and re.search(r"#define MCP_MAX_LEVELS 16\b", text)
    assert _ffi.MCP_ABI_VERSION == 4 == mcp_lib.mcp_abi_version()
    assert (_ffi.MCP_MAX_HORIZONS, _ffi.MCP_MAX_LEVELS) == (64, 16)


def _call(lib, ctx, prm, hz, levels, hz_stats=True, bands=None):
    mu = np.zeros(4, np.float32)
    L = np.eye(4, dtype=np.float32) * 0.01
    W = np.ones((1, 4), np.float32) / 4
    st = np.zeros(1, _ffi.STATS_DTYPE)
    h = np.asarray(hz, np.int32)
    lv = np.asarray(levels, np.float64)
    hs = np.zeros(max(1, h.size), _ffi.STATS_DTYPE)
    b = np.zeros(max(1, h.size * lv.size), np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    if bands is None:
        bands = lv.size > 0
    return lib.mcp_simulate_horizons(ctx, ctypes.byref(prm), mu, L, W, 1, 0, 100, h.size, vp(h) if h.size else None, lv.size,
                                     vp(lv) if lv.size else None, None, vp(st), None, vp(hs) if hz_stats else None,
                                     vp(b) if bands else None)


BAD = [  # (horizons, levels, what the error names)
    ([], [50.0], "n_horizons"), ([3, 2], [50.0], "increasing"), ([2, 2], [], "increasing"), ([0, 3], [], "outside"),
    ([5, 11], [], "outside"), (list(range(1, 66)), [], "n_horizons"), ([1, 2], [-1.0], "level"),
    ([1, 2], [100.5], "level"), ([1, 2], [float("nan")], "level"), ([1, 2], [50.0] * 17, "n_levels"),
]


@pytest.mark.parametrize("hz,levels,what", BAD)
def test_bad_arguments_return_e_arg_without_a_device(hz, levels, what, mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    sentinel = ctypes.c_void_p(16)            # never dereferenced: the arguments are checked first
    assert _call(mcp_lib, sentinel, prm, hz, levels) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()


def test_null_context_and_output_pointers(mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    assert _call(mcp_lib, None, prm, [1, 5, 10], [2.5, 97.5]) == _ffi.MCP_E_ARG
    assert b"ctx is NULL" in mcp_lib.mcp_last_error()
    sentinel = ctypes.c_void_p(16)
    assert _call(mcp_lib, sentinel, prm, [1, 5], [50.0], hz_stats=False) == _ffi.MCP_E_ARG
    assert _call(mcp_lib, sentinel, prm, [1, 5], [50.0], bands=False) == _ffi.MCP_E_ARG
    assert _call(mcp_lib, sentinel, prm, [1, 5], [], bands=True) == _ffi.MCP_E_ARG
    assert b"bands_out" in mcp_lib.mcp_last_error()


def test_launch_rejects_fold_native_and_bad_horizons_before_the_device(mcp_lib):
    buf = ctypes.c_void_p(16)
    h = np.array([2, 5], np.int32)
    hp = h.ctypes.data_as(ctypes.c_void_p)
    for flags in ({"fold": True}, {"native_math": True}):
        prm = _ffi.make_params(4, 10, 1, **flags)
        assert mcp_lib.mcp_launch_paths_horizons(ctypes.byref(prm), buf, None, 0, 0, 100, buf, 100, 2, hp, buf, 100, None, None,
                                                 None) == _ffi.MCP_E_UNSUPPORTED
    prm = _ffi.make_params(4, 4, 1)                                  # h = 5 > T = 4
    assert mcp_lib.mcp_launch_paths_horizons(ctypes.byref(prm), buf, None, 0, 0, 100, buf, 100, 2, hp, buf, 100, None, None,
                                             None) == _ffi.MCP_E_ARG
    prm = _ffi.make_params(4, 10, 1)
    assert mcp_lib.mcp_launch_paths_horizons(ctypes.byref(prm), buf, None, 0, 0, 100, buf, 100, 2, hp, None, 100, None, None,
                                             None) == _ffi.MCP_E_ARG
    assert mcp_lib.mcp_launch_paths_horizons(ctypes.byref(prm), buf, None, 0, 0, 100, buf, 100, 2, hp, buf, 99, None, None,
                                             None) == _ffi.MCP_E_ARG


def test_c99_compile_and_link_of_the_new_prototypes(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "hz.c"
    src.write_text(r'''
        #include <stdio.h>
        #include "mcport.h"
        int main(void) {
            mcp_params p = {4, 12, 1, MCP_COMPOUND_SIMPLE, 0, 0, 1.0, 0.95, 0.0};
            float mu[4] = {0}, chol[16] = {0}, w[4] = {0.25f, 0.25f, 0.25f, 0.25f};
            int32_t hz[3] = {1, 3, 6};
            double levels[3] = {2.5, 50.0, 97.5}, bands[9];
            mcp_stats st, hst[3];
            uint64_t lo, hi;
            double g;
            if (MCP_ABI_VERSION != 4 || MCP_MAX_HORIZONS != 64 || MCP_MAX_LEVELS != 16) return 1;
            if (mcp_simulate_horizons(NULL, &p, mu, chol, w, 1, 0, 8, 3, hz, 3, levels, NULL, &st, NULL, hst, bands) != MCP_E_ARG)
                return 2;
            if (mcp_launch_paths_horizons(&p, NULL, NULL, 0, 0, 10, NULL, 10, 3, hz, NULL, 10, NULL, NULL, NULL) != MCP_E_ARG)
                return 3;
            if (mcp_percentile_rank_q(1001, 2.5, &lo, &hi, &g) != MCP_OK || lo != 25 || hi != 26) return 4;
            printf("%s\n", mcp_last_error());
            return 0;
        }''')
    exe = tmp_path / "hz"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("kw,match", [
    ({"drawdown": True}, "drawdown"), ({"fold": True}, "fold"), ({"native_math": True}, "native_math"),
    ({"horizons": []}, "horizons"), ({"horizons": [3, 2]}, "increasing"), ({"horizons": [0, 2]}, "increasing"),
    ({"horizons": [2, 21]}, "n_steps"), ({"horizons": [1.5]}, "whole"), ({"horizons": list(range(1, 66))}, "horizons"),
    ({"bands": (-1.0,)}, "percentages"), ({"bands": (100.5,)}, "percentages"), ({"bands": (float("nan"),)}, "percentages"),
    ({"bands": (50.0,) * 17}, "16"),
])
def test_python_rejects_bad_horizon_calls_without_a_context(kw, match, monkeypatch):
    """The ValueError comes before any device (or the library) is touched."""
    from monte_carlo_portfolio_amd import simulate as sim

    def boom(*a, **k):
        raise AssertionError("a context was requested")
    monkeypatch.setattr(sim, "default_context", boom)
    args = dict(n_steps=20, n_paths=8, horizons=[1, 5, 20], bands=(2.5, 97.5))
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        sim.simulate_paths(np.zeros(3), np.eye(3) * 1e-4, np.ones(3) / 3, **args)


def test_python_rejects_bands_without_horizons_and_sweeps_with_horizons(monkeypatch):
    from monte_carlo_portfolio_amd import simulate as sim

    def boom(*a, **k):
        raise AssertionError("a context was requested")
    monkeypatch.setattr(sim, "default_context", boom)
    with pytest.raises(ValueError, match="horizons"):
        sim.simulate_paths(np.zeros(3), np.eye(3) * 1e-4, np.ones(3) / 3, n_paths=8, bands=(50.0,))
    with pytest.raises(ValueError, match="horizons"):
        sim.simulate_sweep(np.zeros(3), np.eye(3) * 1e-4, weights=np.ones((2, 3)) / 3, n_paths=8, n_steps=12, horizons=[1, 3])

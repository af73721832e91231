"""CPU checks of the benchmark-relative statistics (SPEC.md 5.23): the extension header against its binding and the library; every
argument rule of mcp_ctx_request_relative and mcp_launch_relative with no device; mcp_relative_finish against relative.finish bit for
bit on random and degenerate records; the finished figures against independent two-pass NumPy evaluations; the front end's keyword
and its refusals with no device; the stand-alone selftest program; and the one-step law on a binary64 twin, at the standard-error
multiples the GPU test uses."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.stats

import front_end_cases
import relative_ref as ref_
from monte_carlo_portfolio_amd import _ffi, check_benchmark, relative, relative_law, simulate, simulate_bootstrap, simulate_filtered, simulate_paths, simulate_sweep, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcport_relative.h")
CSRC = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


# ---- 1. header / binding / library ----------------------------------------------------------------------------------------------

def test_extension_header_binding_and_library_agree(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    assert sorted(protos) == sorted(_ffi.RELATIVE_SIGNATURES) == ["mcp_ctx_request_relative", "mcp_launch_relative", "mcp_relative_finish",
                                                                  "mcp_relative_grid", "mcp_relative_trip_n", "mcp_relative_ws_bytes"]
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, params in protos.items():
        n_args = 0 if params.strip() == "void" else len(params.split(","))
        assert n_args == len(_ffi.RELATIVE_SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(mcp_lib, name).argtypes == _ffi.RELATIVE_SIGNATURES[name][1]
    names = [p.split()[-1].lstrip("*") for p in protos["mcp_launch_relative"].split(",")]
    assert names == ["prm", "d_values", "stride", "n", "rows", "group", "bench", "d_pivot", "d_partials", "d_sums", "d_active", "stream"]
    assert [p.split()[-1].lstrip("*") for p in protos["mcp_ctx_request_relative"].split(",")] == ["ctx", "req", "sums_out", "stats_out",
                                                                                                 "active_stats_out", "active_out", "hz_stats_out"]
    for table in (_ffi.SIGNATURES, _ffi.EXTENSION_SIGNATURES, _ffi.SPEND_SIGNATURES, _ffi.LIFE_SIGNATURES, _ffi.BAND_SIGNATURES,
                  _ffi.VOLTARGET_SIGNATURES, _ffi.UNDERWATER_SIGNATURES, _ffi.UNCERTAIN_SIGNATURES, _ffi.DOWNSIDE_SIGNATURES):
        assert not set(table) & set(protos)
    for struct, dtype_or_cls in (("mcp_relative_sums", _ffi.RELATIVE_SUMS_DTYPE), ("mcp_relative_stats", _ffi.RELATIVE_STATS_DTYPE),
                                 ("mcp_relative", _ffi.McpRelative)):
        fields = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        got = [n.strip().lstrip("*") for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        want = list(dtype_or_cls.names) if isinstance(dtype_or_cls, np.dtype) else [n for n, _ in dtype_or_cls._fields_]
        assert got == want, struct
    assert ctypes.sizeof(_ffi.McpRelative) == 8 and _ffi.RELATIVE_SUMS_DTYPE.itemsize == 144 and _ffi.RELATIVE_STATS_DTYPE.itemsize == 112
    assert all(_ffi.RELATIVE_SUMS_DTYPE[f] == np.uint64 for f in relative.COUNT_FIELDS) and relative.SUM_FIELDS[:5] == relative.COUNT_FIELDS
    assert '#include "mcport.h"' in text and 'extern "C"' in text and "MCP_ABI_VERSION" not in text
    assert mcp_lib.mcp_abi_version() == _ffi.MCP_ABI_VERSION == 4
    assert "mcp_relative" not in open(os.path.join(ROOT, "include", "mcport.h")).read()  # the main header is the parent's


def test_the_grid_is_the_downside_grid(mcp_lib):
    for n in (0, 1, 1024, 1025, 2048, 2049, 512 * 1024, 512 * 1024 + 1, 10 ** 9):
        assert mcp_lib.mcp_relative_grid(n) == mcp_lib.mcp_downside_grid(n)
    trip = mcp_lib.mcp_relative_trip_n()
    assert trip == 4 * (512 * 256 + 1) and mcp_lib.mcp_relative_grid(trip) == 512
    assert mcp_lib.mcp_relative_ws_bytes(3, 5000) == 3 * 5 * 144 and mcp_lib.mcp_relative_ws_bytes(0, 5000) == 0


def test_c99_compile_and_link_of_the_new_prototypes(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "rl.c"
    src.write_text(r'''
        #include <stdio.h>
        #include "mcport_relative.h"
        int main(void) {
            mcp_relative_sums s = {4, 1, 2, 2, 2, 0.625, 0.328125, 1.0, 0.375, 0.875, 0.890625, 0.71875, -0.125, 0.015625, 1.25, 1.0, -0.25, -0.625};
            mcp_relative_stats o;
            mcp_relative req = {0, 0};
            if (mcp_relative_finish(&s, 0.0, 0.0, &o) != MCP_OK || o.active_mean != 0.15625 || o.p_under != 0.25 || o.up_capture != 1.25) return 1;
            if (mcp_ctx_request_relative(NULL, &req, NULL, &o, NULL, NULL, NULL) != MCP_E_ARG) return 2;
            if (mcp_launch_relative(NULL, NULL, 0, 0, 1, 1, 0, NULL, NULL, NULL, NULL, NULL) != MCP_E_ARG) return 3;
            printf("%s %lu %lu\n", mcp_last_error(), (unsigned long)mcp_relative_grid(5000), (unsigned long)mcp_relative_ws_bytes(2, 5000));
            return 0;
        }''')
    exe = tmp_path / "rl"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[-2:] == ["5", "1440"], (out.returncode, out.stdout, out.stderr)


# ---- 2. the argument rules, without a device ---------------------------------------------------------------------------------------

def test_every_rule_of_the_request_and_the_launch_with_no_device(mcp_lib):
    stats = np.zeros(2, _ffi.RELATIVE_STATS_DTYPE)
    sums = np.zeros(2, _ffi.RELATIVE_SUMS_DTYPE)

    def ask(bench=1, reserved=0, req=True, stats_out=stats):
        r = ctypes.byref(_ffi.McpRelative(bench, reserved)) if req else None
        rc = mcp_lib.mcp_ctx_request_relative(None, r, vp(sums), None if stats_out is None else vp(stats_out), None, None, None)
        return rc, mcp_lib.mcp_last_error().decode()
    assert ask() == (_ffi.MCP_E_ARG, "ctx is NULL")                       # everything else in order: the context is looked at last
    assert ask(bench=0) == (_ffi.MCP_E_ARG, "ctx is NULL")
    assert ask(bench=10 ** 6) == (_ffi.MCP_E_ARG, "ctx is NULL")          # the upper end is the call's rule: K is not known here
    assert ask(req=False) == (_ffi.MCP_E_ARG, "ctx is NULL")              # a NULL request withdraws: only the context can be wrong
    rc, why = ask(stats_out=None)
    assert rc == _ffi.MCP_E_ARG and "stats_out is NULL" in why
    rc, why = ask(bench=-1)
    assert rc == _ffi.MCP_E_ARG and "bench=-1" in why
    rc, why = ask(reserved=7)
    assert rc == _ffi.MCP_E_ARG and "reserved=7" in why
    assert not stats.view(np.uint8).any() and not sums.view(np.uint8).any()
    # the launch: its own rules before any device
    prm = _ffi.make_params(1, 1, 1)
    one = np.zeros(64, np.float32)
    ok = dict(values=vp(one), stride=4, n=4, rows=6, group=3, bench=1, partials=vp(one), sums=vp(one))
    for change, text in ((dict(values=None), "bad argument"), (dict(partials=None), "bad argument"), (dict(sums=None), "bad argument"),
                         (dict(rows=0), "bad argument"), (dict(rows=-3), "bad argument"), (dict(stride=3), "bad argument"),
                         (dict(group=0), "multiple of group"), (dict(group=-3), "multiple of group"), (dict(group=4), "multiple of group"),
                         (dict(rows=7), "multiple of group"), (dict(bench=-1), "bench=-1"), (dict(bench=3), "bench=3"),
                         (dict(group=6, bench=6), "bench=6")):
        a = dict(ok, **change)
        rc = mcp_lib.mcp_launch_relative(ctypes.byref(prm), a["values"], a["stride"], a["n"], a["rows"], a["group"], a["bench"], None,
                                         a["partials"], a["sums"], None, None)
        assert rc == _ffi.MCP_E_ARG and text in mcp_lib.mcp_last_error().decode(), (change, mcp_lib.mcp_last_error())
    assert mcp_lib.mcp_launch_relative(None, vp(one), 4, 4, 1, 1, 0, None, vp(one), vp(one), None, None) == _ffi.MCP_E_ARG
    bad = _ffi.make_params(1, 1, 1)
    bad.v0 = -1.0                                                         # the rules of prm
    assert mcp_lib.mcp_launch_relative(ctypes.byref(bad), vp(one), 4, 4, 1, 1, 0, None, vp(one), vp(one), None, None) == _ffi.MCP_E_ARG
    assert mcp_lib.mcp_relative_finish(None, 0.0, 0.0, vp(stats)) == _ffi.MCP_E_ARG
    assert mcp_lib.mcp_relative_finish(vp(sums), 0.0, 0.0, None) == _ffi.MCP_E_ARG


def test_check_benchmark():
    assert check_benchmark(None, 3) is None and check_benchmark(0, 3) == 0 and check_benchmark(2, 3) == 2
    assert check_benchmark(np.int64(1), 3) == 1 and type(check_benchmark(np.int32(1), 3)) is int and check_benchmark(0, 1) == 0
    for bad in (True, False, np.bool_(True), 1.0, np.float32(0), "1", b"1", [1], (0,), np.zeros(1, int), {}, 1j):
        with pytest.raises(ValueError, match="benchmark must be"):
            check_benchmark(bad, 3)
    for bad, K in ((3, 3), (-1, 3), (1, 1), (10 ** 12, 5)):
        with pytest.raises(ValueError, match="is not a row"):
            check_benchmark(bad, K)


# ---- 3. mcp_relative_finish against relative.finish, bit for bit ----------------------------------------------------------------------

def _samples():
    """name -> (x_k, x_b, c_k, c_b): every branch of the finish."""
    rng = np.random.default_rng(23)
    xb = 0.04 + 0.1 * rng.standard_normal(997)
    xk = 0.01 + 0.7 * xb + 0.05 * rng.standard_normal(997)
    out = {"plain": (xk, xb, 0.038, 0.041), "own row": (xb, xb, 0.041, 0.041), "no pivots": (xk, xb, 0.0, 0.0)}
    ties = xk.copy()
    ties[::3] = xb[::3]
    out["ties"] = (ties, xb, 0.038, 0.041)
    out["always behind"] = (xb - np.abs(xk) - 1e-3, xb, 0.0, 0.041)
    out["never behind"] = (xb + np.abs(xk), xb, 0.1, 0.041)
    out["benchmark never up"] = (xk, -np.abs(xb) - 0.01, 0.038, -0.09)
    out["benchmark never down"] = (xk, np.abs(xb) + 0.01, 0.038, 0.09)
    zeros = xb.copy()
    zeros[::4] = 0.0
    out["benchmark at zero"] = (xk, zeros, 0.038, 0.03)
    out["flat benchmark"] = (xk, np.full(997, 0.25), 0.038, 0.25)
    out["flat benchmark off its pivot"] = (xk, np.full(997, 0.25), 0.038, 0.2)
    out["flat portfolio"] = (np.full(997, 0.125), xb, 0.125, 0.041)
    out["both flat"] = (np.full(64, 0.125), np.full(64, 0.25), 0.125, 0.25)
    out["anticorrelated"] = (-xb, xb, -0.041, 0.041)
    out["low volatility"] = (1.0 + 4e-4 * rng.standard_normal(5000), 1.0 + 4e-4 * rng.standard_normal(5000), 1.0 + 1e-5, 1.0 - 1e-5)
    out["n = 0"] = (np.zeros(0), np.zeros(0), 0.5, 0.25)
    out["n = 1"] = (np.array([0.3]), np.array([-0.1]), 0.2, 0.0)
    out["n = 2"] = (np.array([-0.3, 0.4]), np.array([0.1, 0.2]), 0.0, 0.1)
    return out


@pytest.mark.parametrize("name", sorted(_samples()))
def test_finish_in_c_and_in_python_agree_bit_for_bit(name, mcp_lib):
    xk, xb, ck, cb = _samples()[name]
    rec = ref_.raw_record(xk, xb, ck, cb)
    got, want = _ffi.relative_finish(rec, ck, cb), relative.finish(rec, ck, cb)
    assert set(want) == set(relative.STAT_FIELDS)
    for f in relative.STAT_FIELDS:
        assert np.float64(got[f]).view(np.uint64) == np.float64(want[f]).view(np.uint64), (f, got[f], want[f])
        assert math.isfinite(got[f]), f                       # every zero denominator has its value
    n = xk.size
    assert got["pivot"] == ck and got["bench_pivot"] == cb
    if n:
        assert got["p_under"] == np.mean(xk < xb) and got["p_over"] == np.mean(xk > xb)
    if name == "own row":
        assert got["tracking_error"] == 0.0 == got["information_ratio"] and got["beta"] == 1.0 == got["correlation"]
        assert got["up_capture"] == 1.0 == got["down_capture"] and got["active_mean"] == 0.0 == got["alpha"]
    if name == "ties":
        assert int(rec["n_under"]) + int(rec["n_over"]) == n - len(xk[::3])
    if name == "never behind":
        assert got["mean_underperformance"] == 0.0 == got["relative_downside_deviation"] and got["p_under"] == 0.0
    if name == "benchmark never up":
        assert got["up_capture"] == 0.0 and got["down_capture"] != 0.0
    if name == "benchmark never down":
        assert got["down_capture"] == 0.0 and got["up_capture"] != 0.0
    if name == "benchmark at zero":
        assert int(rec["n_up"]) + int(rec["n_down"]) == n - len(xb[::4])
    if name.startswith("flat benchmark") or name == "both flat":
        assert got["beta"] == 0.0 == got["correlation"] and got["down_capture"] == 0.0
    if name in ("flat portfolio", "both flat"):
        assert got["correlation"] == 0.0
    if name == "both flat":
        assert got["tracking_error"] == 0.0 == got["information_ratio"] and got["active_mean"] == -0.125
    if name == "anticorrelated":
        assert got["correlation"] == -1.0 and abs(got["beta"] + 1.0) < 1e-15
    if name == "n = 0":
        assert got["active_mean"] == 0.25 and got["alpha"] == 0.5 and all(got[f] == 0.0 for f in relative.STAT_FIELDS[1:8])
    if name == "n = 1":
        assert got["tracking_error"] == 0.0 == got["information_ratio"] and got["p_over"] == 1.0 and got["down_capture"] == 0.3 / -0.1


def test_finish_on_random_records_bit_for_bit(mcp_lib):
    rng = np.random.default_rng(24)
    for t in range(400):
        n = int(rng.integers(0, 40))
        xb = rng.normal(0.01, 0.1, n)
        xk = xb.copy() if t % 4 == 0 else rng.normal(0.02, 0.1, n)
        ck, cb = (0.01, 0.01) if t % 4 == 0 else rng.normal(0.0, 0.02, 2)
        rec = ref_.raw_record(xk, xb, ck, cb)
        got, want = _ffi.relative_finish(rec, ck, cb), relative.finish(rec, ck, cb)
        for f in relative.STAT_FIELDS:
            assert np.float64(got[f]).view(np.uint64) == np.float64(want[f]).view(np.uint64), (t, f, got[f], want[f])
        if t % 4 == 0 and n >= 2:
            assert got["beta"] == 1.0 == got["correlation"] and got["tracking_error"] == 0.0


# ---- 4. the finished figures against independent two-pass evaluations ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["plain", "no pivots", "ties", "always behind", "benchmark at zero", "low volatility", "n = 2"])
def test_finished_figures_against_two_pass_evaluations(name, mcp_lib):
    """The sums are exact (math.fsum), so the finish loses only in the conversion from shifted to central moments: a relative
    (delta / sigma)^2 2^-53 per moment, with delta the distance of the mean from the pivot.  |delta| <= sigma is asserted, not assumed,
    for d_k, d_b and e; then every moment is good to a few 2^-53 and 1e-10 is far above it.  The two-pass figures themselves carry
    n 2^-53 = 1e-13 at these sizes."""
    xk, xb, ck, cb = _samples()[name]
    rec = ref_.raw_record(xk, xb, ck, cb)
    got = _ffi.relative_finish(rec, ck, cb)
    n, a = xk.size, xk - xb
    assert abs(float(rec["k1"]) / n) <= np.std(xk) and abs(float(rec["b1"]) / n) <= np.std(xb) and abs(float(rec["e1"]) / n) <= np.std(a)
    close = lambda p, q: abs(p - q) <= 1e-10 * abs(q)     # noqa: E731
    assert close(got["active_mean"], np.mean(xk) - np.mean(xb))
    assert close(got["tracking_error"], np.std(a, ddof=1))
    assert close(got["information_ratio"], (np.mean(xk) - np.mean(xb)) / np.std(a, ddof=1))
    assert got["p_under"] == np.mean(a < 0) and got["p_over"] == np.mean(a > 0)
    if (a < 0).any():
        assert close(got["mean_underperformance"], np.mean(a[a < 0]))
    assert close(got["relative_downside_deviation"], math.sqrt(np.mean(np.minimum(a, 0.0) ** 2)))
    beta = np.cov(xk, xb)[0, 1] / np.var(xb, ddof=1)
    assert close(got["beta"], beta) and close(got["alpha"], np.mean(xk) - beta * np.mean(xb))
    assert abs(got["correlation"] - np.corrcoef(xk, xb)[0, 1]) <= 1e-10
    if (xb > 0).any():
        assert close(got["up_capture"], np.sum(xk[xb > 0]) / np.sum(xb[xb > 0]))
    if (xb < 0).any():
        assert close(got["down_capture"], np.sum(xk[xb < 0]) / np.sum(xb[xb < 0]))


# ---- 5. the law -----------------------------------------------------------------------------------------------------------------------

def test_relative_law_and_its_rules():
    mu, cov = np.array([0.01, 0.02]), np.array([[0.04, 0.01], [0.01, 0.09]])
    law = relative_law(mu, cov, [0.5, 0.5], [1.0, 0.0])
    assert abs(law["active_mean"] - 0.005) < 1e-17 and abs(law["tracking_error"] - math.sqrt(0.25 * 0.04 - 0.5 * 0.01 + 0.25 * 0.09)) < 1e-16
    assert abs(law["beta"] - 0.625) < 1e-15 and abs(law["alpha"] - (0.015 - 0.625 * 0.01)) < 1e-16
    assert abs(law["correlation"] - 0.025 / math.sqrt(0.0375 * 0.04)) < 1e-15
    assert law["information_ratio"] == law["active_mean"] / law["tracking_error"]
    assert abs(law["p_under"] - float(scipy.stats.norm.cdf(-law["information_ratio"]))) < 1e-15
    for w, wb in (([1.0, 0.0], [1.0, 0.0]), ([0.5, 0.5], [0.0, 0.0]), ([0.0, 0.0], [0.5, 0.5])):
        with pytest.raises(ValueError, match="positive variance"):
            relative_law(mu, cov, w, wb)


def test_a_binary64_twin_passes_the_law_assertions_at_the_gpu_tests_size(mcp_lib):
    """What tests/test_gpu_relative.py asserts of 10^6 simulated one-step paths, on NumPy's normals and the same market and weights:
    the standard-error multiples are the law's, not the kernel's."""
    n = 1_000_000
    mu, cov = synthetic.synthetic_market(4)
    W = np.array([[0.25, 0.25, 0.25, 0.25], [0.7, 0.1, 0.1, 0.1], [0.0, 0.2, 0.3, 0.5]])
    r = np.asarray(mu, np.float64) + np.random.default_rng(79).standard_normal((n, 4)) @ np.linalg.cholesky(np.asarray(cov, np.float64)).T
    x = r @ W.T
    for k in (1, 2):
        ck, cb = float(W[k] @ mu), float(W[0] @ mu)
        s, c = ref_.summands(x[:, k], x[:, 0], ck, cb)
        rec = np.zeros((), _ffi.RELATIVE_SUMS_DTYPE)
        for f in ref_.COUNTS:
            rec[f] = c[f]
        for f in ref_.SUMS:
            rec[f] = np.sum(s[f])
        ref_.law_assertions(_ffi.relative_finish(rec, ck, cb), relative_law(mu, cov, W[k], W[0]), n, f"twin k={k}")
    assert ref_.LAW_SE == 5.0


# ---- 6. the front end, without a device ---------------------------------------------------------------------------------------------

def test_the_keyword_rides_every_entry_point_and_is_refused_where_it_cannot(mcp_lib):
    assert simulate._PATHS_COMBINE["benchmark"][1] == ("shard='portfolios'",)
    mu, cov = synthetic.synthetic_market(3)
    w = synthetic.dirichlet_weights(3, 3)
    rows = np.full((30, 3), 0.01) + 0.01 * np.random.default_rng(1).standard_normal((30, 3))
    with front_end_cases.recording(mcp_lib) as (rec, ctx):
        # the funnel arms the context before the entry point is called: with the recorder's NULL context that is where it stops
        for kw in (dict(), dict(drawdown=True), dict(horizons=(2, 5)), dict(dof=5), dict(antithetic=True), dict(cashflow=-0.001),
                   dict(drift_uncertainty=60), dict(drawdown=True, underwater=True), dict(vol_target=(0.1, 0.9)), dict(tolerance=0.02)):
            got = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, benchmark=1, **kw))
            assert got == {"raises": ["McpError", "libmcport error -1: ctx is NULL"]}, (kw, got)
            same = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, **kw))
            assert "calls" in same, kw
        got = front_end_cases.record(rec, lambda: simulate_bootstrap(rows, w, n_steps=5, n_paths=64, benchmark=0))
        assert got == {"raises": ["McpError", "libmcport error -1: ctx is NULL"]}
        for bad in (True, 1.0, "0", [0]):
            for fn, first in ((simulate_paths, (mu, cov)), (simulate_bootstrap, (rows,))):
                got = front_end_cases.record(rec, lambda: fn(*first, w, n_steps=5, n_paths=64, benchmark=bad))
                assert got["raises"][0] == "ValueError" and got["raises"][1].startswith("benchmark must be"), (bad, got)
        for bad in (3, -1):
            got = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, benchmark=bad))
            assert got["raises"][0] == "ValueError" and "is not a row of the 3 portfolios" in got["raises"][1]
        got = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w[0], n_steps=5, n_paths=64, benchmark=1))
        assert got["raises"][0] == "ValueError" and "is not a row of the 1 portfolios" in got["raises"][1]
        got = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, benchmark=0, as_array=True))
        assert got == {"raises": ["ValueError", "benchmark fills the 'relative' block of the result dicts: not with as_array"]}
        got = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, benchmark=0, shard="portfolios"))
        assert got == {"raises": ["ValueError", simulate._PATHS_COMBINE["benchmark"][0] + ": not with shard='portfolios'"]}
        got = front_end_cases.record(rec, lambda: simulate_bootstrap(rows, w, n_steps=5, n_paths=64, benchmark=0, shard="portfolios"))
        assert got["raises"][0] == "ValueError" and got["raises"][1].endswith("not with shard='portfolios'")
        got = front_end_cases.record(rec, lambda: simulate_sweep(mu, cov, weights=w, n_steps=5, n_paths=64, benchmark=0))
        assert got["raises"][0] == "ValueError" and got["raises"][1].startswith("simulate_sweep does not take benchmark")
    with pytest.raises(ValueError, match="benchmark must be"):
        simulate_filtered(None, w, benchmark=0.5)


def test_the_result_block_from_the_calls_arrays():
    xk, xb, ck, cb = _samples()["plain"]
    rec = ref_.raw_record(xk, xb, ck, cb)
    sums = np.array([rec, rec], _ffi.RELATIVE_SUMS_DTYPE)
    stats = np.array([_ffi.relative_finish(rec, ck, cb)] * 2, _ffi.RELATIVE_STATS_DTYPE)
    hz = np.array([[stats[0], stats[1]]] * 3, _ffi.RELATIVE_STATS_DTYPE)
    act = np.zeros(2, _ffi.STATS_DTYPE)
    act["var"], act["min"], act["max"], act["n_tail"] = -0.1, -0.3, 0.2, 50
    y = np.ones((2, 997), np.float32)
    blocks = relative.relative_blocks(stats, sums, 1, act, hz, y)
    assert len(blocks) == 2 and set(blocks[0]) == set(relative.STAT_FIELDS) | {"benchmark", "sums", "active", "horizons"}
    assert blocks[1]["benchmark"] == 1 and blocks[1]["sums"]["n"] == xk.size and isinstance(blocks[1]["sums"]["n_under"], int)
    assert sorted(blocks[0]["active"]) == sorted(["mean", "std", "var", "cvar", "n_tail", "worst", "best", "y"])
    assert blocks[0]["active"]["worst"] == -0.3 and blocks[0]["active"]["best"] == 0.2 and blocks[0]["active"]["n_tail"] == 50
    assert len(blocks[0]["horizons"]) == 3 and blocks[0]["horizons"][2]["beta"] == blocks[0]["beta"] and blocks[0]["horizons"][0]["benchmark"] == 1
    assert relative.finish(blocks[0]["sums"], ck, cb)["information_ratio"] == blocks[0]["information_ratio"]
    plain = relative.relative_blocks(stats, sums, 1, act)[0]
    assert "horizons" not in plain and "y" not in plain["active"]


# ---- 7. the stand-alone selftest ---------------------------------------------------------------------------------------------------------

def test_the_relative_selftest_builds_and_runs_under_the_sanitizers(tmp_path):
    """`make relative-selftest`: csrc/relative_selftest.cpp with mcp_host.cpp, a plain C++ compiler, AddressSanitizer + UBSan, no
    device: the finish on hand-made records, the request's rules, arm / take / disarm, the one-tile rule against plan_tiles and the
    bytes the budget counts."""
    r = subprocess.run(["make", "-C", CSRC, "relative-selftest", f"BUILD={tmp_path}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "relative_selftest ok" in r.stdout
    text = open(os.path.join(CSRC, "relative_selftest.cpp")).read()
    main = text[text.index("int main()"):]
    assert all(f"{f}();" in main for f in ("run_finish", "run_request", "run_plan"))
    assert "const RelativeArm failing = arm.take();" in text and "const RelativeArm plain = arm.take();" in text
    api = open(os.path.join(CSRC, "mcp_api.cpp")).read()
    assert "const RelativeArm rl = c->relative.take();" in api and "check_relative_plan(plan, K, by_portfolio)" in api

"""CPU checks of the downside and shape statistics (SPEC.md 5.22): the extension header against its binding and the library; every
argument rule of mcp_ctx_request_downside with a context that touches no device, and of check_downside; mcp_downside_finish against
downside.finish bit for bit on exact sums; the finished figures against independent two-pass evaluations; the front end's keyword
with no device; the normal law on a binary64 twin; and that the host selftest carries the finish function and the arm / disarm rule."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.stats

import downside_ref as ref_
import front_end_cases
from monte_carlo_portfolio_amd import _ffi, check_downside, downside, metrics, normal_law, simulate, simulate_bootstrap, simulate_paths, simulate_sweep, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcport_downside.h")
CSRC = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


# ---- 1. header / binding / library ----------------------------------------------------------------------------------------------

def test_extension_header_binding_and_library_agree(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    assert sorted(protos) == sorted(_ffi.DOWNSIDE_SIGNATURES) == ["mcp_ctx_request_downside", "mcp_downside_finish", "mcp_downside_grid",
                                                                  "mcp_downside_trip_n", "mcp_downside_ws_bytes", "mcp_launch_downside"]
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, params in protos.items():
        n_args = 0 if params.strip() == "void" else len(params.split(","))
        assert n_args == len(_ffi.DOWNSIDE_SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(mcp_lib, name).argtypes == _ffi.DOWNSIDE_SIGNATURES[name][1]
    names = [p.split()[-1].lstrip("*") for p in protos["mcp_launch_downside"].split(",")]
    assert names == ["prm", "d_values", "stride", "n", "rows", "d_pivot", "tau", "d_partials", "d_sums", "stream"]
    assert [p.split()[-1].lstrip("*") for p in protos["mcp_ctx_request_downside"].split(",")] == ["ctx", "req", "sums_out", "stats_out", "hz_stats_out"]
    for table in (_ffi.SIGNATURES, _ffi.EXTENSION_SIGNATURES, _ffi.SPEND_SIGNATURES, _ffi.LIFE_SIGNATURES, _ffi.BAND_SIGNATURES,
                  _ffi.VOLTARGET_SIGNATURES, _ffi.UNDERWATER_SIGNATURES, _ffi.UNCERTAIN_SIGNATURES):
        assert not set(table) & set(protos)
    for struct, dtype_or_cls in (("mcp_downside_sums", _ffi.DOWNSIDE_SUMS_DTYPE), ("mcp_downside_stats", _ffi.DOWNSIDE_STATS_DTYPE),
                                 ("mcp_downside", _ffi.McpDownside)):
        fields = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        got = [n.strip().lstrip("*") for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        want = list(dtype_or_cls.names) if isinstance(dtype_or_cls, np.dtype) else [n for n, _ in dtype_or_cls._fields_]
        assert got == want, struct
    assert ctypes.sizeof(_ffi.McpDownside) == 16 and _ffi.DOWNSIDE_SUMS_DTYPE.itemsize == 96 and _ffi.DOWNSIDE_STATS_DTYPE.itemsize == 88
    assert '#include "mcport.h"' in text and 'extern "C"' in text and "MCP_ABI_VERSION" not in text
    assert mcp_lib.mcp_abi_version() == _ffi.MCP_ABI_VERSION == 4
    assert "downside" not in open(os.path.join(ROOT, "include", "mcport.h")).read()      # the main header is the parent's


def test_the_grid_is_a_function_of_n_alone(mcp_lib):
    assert [mcp_lib.mcp_downside_grid(n) for n in (0, 1, 1024, 1025, 2048, 2049, 512 * 1024, 512 * 1024 + 1, 10 ** 9)] == [1, 1, 1, 2, 2, 3, 512, 512, 512]
    trip = mcp_lib.mcp_downside_trip_n()
    assert trip == 4 * (512 * 256 + 1) and mcp_lib.mcp_downside_grid(trip) == 512
    assert mcp_lib.mcp_downside_ws_bytes(3, 5000) == 3 * 5 * 96 and mcp_lib.mcp_downside_ws_bytes(0, 5000) == 0


def test_c99_compile_and_link_of_the_new_prototypes(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "ds.c"
    src.write_text(r'''
        #include <stdio.h>
        #include "mcport_downside.h"
        int main(void) {
            mcp_downside_sums s = {4, 2, 2, 2.0, 22.0, 56.0, 274.0, -3.0, 5.0, -3.0, 5.0, 5.0};
            mcp_downside_stats o;
            mcp_downside req = {0.0, 0, 0};
            if (mcp_downside_finish(&s, 0.0, 0.0, &o) != MCP_OK || o.mean != 0.5 || o.p_below != 0.5) return 1;
            if (mcp_ctx_request_downside(NULL, &req, NULL, &o, NULL) != MCP_E_ARG) return 2;
            if (mcp_launch_downside(NULL, NULL, 0, 0, 1, NULL, 0.0, NULL, NULL, NULL) != MCP_E_ARG) return 3;
            printf("%s %lu %lu\n", mcp_last_error(), (unsigned long)mcp_downside_grid(5000), (unsigned long)mcp_downside_ws_bytes(2, 5000));
            return 0;
        }''')
    exe = tmp_path / "ds"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[-2:] == ["5", "960"], (out.returncode, out.stdout, out.stderr)


# ---- 2. the argument rules, without a device ---------------------------------------------------------------------------------------

def test_every_rule_of_the_request_with_a_null_context(mcp_lib):
    stats = np.zeros(2, _ffi.DOWNSIDE_STATS_DTYPE)
    sums = np.zeros(2, _ffi.DOWNSIDE_SUMS_DTYPE)

    def ask(tau=0.01, use_rf=0, reserved=0, req=True, stats_out=stats):
        r = ctypes.byref(_ffi.McpDownside(tau, use_rf, reserved)) if req else None
        rc = mcp_lib.mcp_ctx_request_downside(None, r, vp(sums), None if stats_out is None else vp(stats_out), None)
        return rc, mcp_lib.mcp_last_error().decode()
    assert ask() == (_ffi.MCP_E_ARG, "ctx is NULL")                       # everything else in order: the context is looked at last
    assert ask(use_rf=1) == (_ffi.MCP_E_ARG, "ctx is NULL")
    assert ask(req=False) == (_ffi.MCP_E_ARG, "ctx is NULL")              # a NULL request withdraws: only the context can be wrong
    rc, why = ask(stats_out=None)
    assert rc == _ffi.MCP_E_ARG and "stats_out is NULL" in why
    for bad in (math.nan, math.inf, -math.inf):
        rc, why = ask(tau=bad)
        assert rc == _ffi.MCP_E_ARG and "not finite" in why
        rc, why = ask(tau=bad, use_rf=1)                                  # tau is not read then, and must still be finite
        assert rc == _ffi.MCP_E_ARG and "not finite" in why
    rc, why = ask(reserved=7)
    assert rc == _ffi.MCP_E_ARG and "reserved=7" in why
    assert not stats.view(np.uint8).any() and not sums.view(np.uint8).any()
    # the launch: its own rules before any device
    prm = _ffi.make_params(1, 1, 1)
    one = np.zeros(16, np.float32)
    ok = dict(values=vp(one), stride=4, n=4, rows=1, tau=0.0, partials=vp(one), sums=vp(one))
    for change, text in ((dict(values=None), "bad argument"), (dict(partials=None), "bad argument"), (dict(sums=None), "bad argument"),
                         (dict(rows=0), "bad argument"), (dict(stride=3), "bad argument"), (dict(tau=math.nan), "not finite")):
        a = dict(ok, **change)
        rc = mcp_lib.mcp_launch_downside(ctypes.byref(prm), a["values"], a["stride"], a["n"], a["rows"], None, a["tau"], a["partials"], a["sums"], None)
        assert rc == _ffi.MCP_E_ARG and text in mcp_lib.mcp_last_error().decode(), change
    assert mcp_lib.mcp_launch_downside(None, vp(one), 4, 4, 1, None, 0.0, vp(one), vp(one), None) == _ffi.MCP_E_ARG
    assert mcp_lib.mcp_downside_finish(None, 0.0, 0.0, vp(stats)) == _ffi.MCP_E_ARG


def test_check_downside():
    assert check_downside(None) is None and check_downside(True) is True and check_downside(np.bool_(True)) is True
    assert check_downside(0) == 0.0 and check_downside(-0.02) == -0.02 and check_downside(np.float32(0.5)) == 0.5
    for bad in (False, math.nan, math.inf, -math.inf, "0.1", b"x", [0.1], (0.0, 0.1), np.zeros(2), {}, 1j):
        with pytest.raises(ValueError, match="downside must be"):
            check_downside(bad)


# ---- 3. mcp_downside_finish against downside.finish, bit for bit ----------------------------------------------------------------------

def _samples():
    """name -> (x, tau, pivot): every branch of the finish, on samples whose sums are exact (math.fsum)."""
    rng = np.random.default_rng(22)
    base = 0.05 + 0.1 * rng.standard_normal(997)
    out = {"plain": (base, 0.01, 0.049), "n_below = 0": (np.abs(base) + 0.02, 0.01, 0.1), "n_below = n": (-np.abs(base) - 0.02, 0.0, -0.1)}
    one = np.abs(base) + 0.02
    one[17] = -0.3
    out["n_below = 1"] = (one, 0.01, 0.1)
    two = one.copy()
    two[400] = -0.2
    out["n_below = 2"] = (two, 0.01, 0.1)
    at = base.copy()
    at[::3] = 0.01                                          # a third of the values equal tau: in neither set
    out["values equal to tau"] = (at, 0.01, 0.049)
    out["all at tau"] = (np.full(50, 0.25), 0.25, 0.2)
    out["constant"] = (np.full(64, 0.125), 0.0, 0.125)      # M2 = 0 exactly: d = 0
    out["constant off the pivot"] = (np.full(64, 0.1), 0.0, 0.125)
    out["low volatility"] = (1.0 + 4e-4 * rng.standard_normal(5000), 1.0, 1.0 + 1e-5)   # sigma / |mean| = 4e-4, tests/stats_cases.py's ratio
    out["n = 1"] = (np.array([0.3]), 0.1, 0.2)
    out["n = 2"] = (np.array([-0.3, 0.4]), 0.1, 0.0)
    return out


@pytest.mark.parametrize("name", sorted(_samples()))
def test_finish_in_c_and_in_python_agree_bit_for_bit(name, mcp_lib):
    x, tau, pivot = _samples()[name]
    rec = ref_.raw_record(x, pivot, tau)
    got, want = _ffi.downside_finish(rec, tau, pivot), downside.finish(rec, tau, pivot)
    for f in downside.STAT_FIELDS:
        assert np.float64(got[f]).view(np.uint64) == np.float64(want[f]).view(np.uint64) or (math.isnan(got[f]) and math.isnan(want[f])), (f, got[f], want[f])
    nb = int(rec["n_below"])
    assert math.isnan(got["downside_std"]) == (nb == 1) and (got["downside_std"] == 1e-4) == (nb == 0)
    assert (got["omega"] == math.inf) == (nb == 0) and got["p_below"] == nb / x.size
    if name == "constant":
        assert got["skewness"] == 0.0 and got["excess_kurtosis"] == 0.0 and got["mean"] == 0.125
    if name == "values equal to tau":
        assert int(rec["n_below"]) + int(rec["n_above"]) == x.size - len(x[::3])


# ---- 4. the finished figures against independent two-pass evaluations ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["plain", "values equal to tau", "low volatility", "n_below = 2", "n_below = n"])
def test_finished_figures_against_two_pass_evaluations(name, mcp_lib):
    """Exact sums leave the conversion from shifted to central moments as the only loss: (delta / sigma)^2 2^-53 with |delta| <= sigma,
    far below 1e-10 -- and |S1 / n| <= std is asserted, not assumed."""
    x, tau, pivot = _samples()[name]
    rec = ref_.raw_record(x, pivot, tau)
    got = _ffi.downside_finish(rec, tau, pivot)
    assert abs(float(rec["s1"]) / x.size) <= np.std(x)
    ex = x - tau
    close = lambda a, b: abs(a - b) <= 1e-10 * abs(b)     # noqa: E731
    assert close(got["sortino"], metrics.sortino_ratio(x, tau, 1))
    assert close(got["mean"], np.mean(x))
    if name != "n_below = n":                               # there skew and kurtosis are those of -|.|: fine, but keep the cases the issue names
        assert close(got["skewness"], scipy.stats.skew(x)) and close(got["excess_kurtosis"], scipy.stats.kurtosis(x))
    assert close(got["downside_deviation"], math.sqrt(np.mean(np.minimum(ex, 0.0) ** 2)))
    assert got["p_below"] == np.mean(x < tau)
    if (ex < 0).any():
        assert close(got["omega"], np.sum(ex[ex > 0]) / -np.sum(ex[ex < 0])) or not (ex > 0).any()
        assert close(got["mean_shortfall"], np.mean(ex[ex < 0]))
        assert close(got["sortino_target"], np.mean(ex) / math.sqrt(np.mean(np.minimum(ex, 0.0) ** 2)))
    if not (ex > 0).any():
        assert got["omega"] == 0.0


# ---- 5. the normal law ------------------------------------------------------------------------------------------------------------

def test_normal_law_against_quadrature_and_its_rules():
    mu, sigma, tau = 0.03, 0.2, -0.01
    law = normal_law(mu, sigma, tau)
    xs = np.linspace(mu - 12 * sigma, mu + 12 * sigma, 2_000_001)
    pdf = np.exp(-0.5 * ((xs - mu) / sigma) ** 2) / (sigma * math.sqrt(2 * math.pi))
    e = xs - tau
    quad = lambda f: float(np.sum(f * pdf) * (xs[1] - xs[0]))   # noqa: E731
    assert abs(law["p_below"] - quad(e < 0)) < 1e-5 and abs(law["l1"] - quad(np.minimum(e, 0))) < 1e-7
    assert abs(law["l2"] - quad(np.minimum(e, 0) ** 2)) < 1e-7 and abs(law["u1"] - quad(np.maximum(e, 0))) < 1e-7
    assert law["omega"] == law["u1"] / -law["l1"] and law["downside_deviation"] == math.sqrt(law["l2"])
    at_mean = normal_law(0.0, sigma, 0.0)
    assert at_mean["p_below"] == 0.5 and abs(at_mean["omega"] - 1) < 1e-15 and abs(at_mean["l2"] - sigma * sigma / 2) < 1e-18
    rng = np.random.default_rng(5)                          # the delta-method standard error against the spread of 400 sample Omegas
    draws = mu + sigma * rng.standard_normal((400, 20_000)) - tau
    om = np.maximum(draws, 0).sum(axis=1) / -np.minimum(draws, 0).sum(axis=1)
    assert abs(np.std(om) / (law["omega_se1"] / math.sqrt(20_000)) - 1) < 0.15
    with pytest.raises(ValueError):
        normal_law(0.0, 0.0, 0.0)


def test_a_binary64_twin_passes_the_law_assertions_at_the_gpu_tests_size(mcp_lib):
    """What tests/test_gpu_downside.py asserts of 10^6 simulated paths, on NumPy's normals: the assertions are not tighter than the law."""
    n, sigma = 1_000_000, 0.04
    x = 0.01 + sigma * np.random.default_rng(77).standard_normal(n)
    s, lo, hi = ref_.summands(x, 0.01, 0.01)
    rec = np.zeros((), _ffi.DOWNSIDE_SUMS_DTYPE)
    rec["n"], rec["n_below"], rec["n_above"] = n, lo.sum(), hi.sum()
    for f in ref_.SUMS:
        rec[f] = np.sum(s[f])
    ref_.law_assertions(_ffi.downside_finish(rec, 0.01, 0.01), sigma, n, "twin")
    t = 0.01 + sigma * math.sqrt(8 / 10) * np.random.default_rng(78).standard_t(10, n)
    assert scipy.stats.kurtosis(t) > 5 * math.sqrt(24.0 / n)    # 6 / (nu - 4) = 1 at nu = 10


# ---- 6. the front end, without a device ---------------------------------------------------------------------------------------------

def test_the_keyword_rides_every_entry_point_and_is_refused_where_it_cannot(mcp_lib):
    assert simulate._KEYWORD_GROUP["downside"] == "ctx" and simulate._PATHS_COMBINE["downside"][1] == ()
    for table in (_ffi.SIMULATE_ENTRIES, _ffi.EXTENSION_ENTRIES, _ffi.SPEND_ENTRIES, _ffi.LIFE_ENTRIES, _ffi.BAND_ENTRIES,
                  _ffi.VOLTARGET_ENTRIES, _ffi.UNDERWATER_ENTRIES, _ffi.UNCERTAIN_ENTRIES):
        for entry, groups in table.items():
            assert simulate._KEYWORD_GROUP["downside"] in groups, entry
    mu, cov = synthetic.synthetic_market(3)
    w = synthetic.dirichlet_weights(3, 2)
    with front_end_cases.recording(mcp_lib) as (rec, ctx):
        # the funnel arms the context before the entry point is called: with the recorder's NULL context that is where it stops
        for kw in (dict(), dict(drawdown=True), dict(horizons=(2, 5)), dict(dof=5), dict(antithetic=True), dict(cashflow=-0.001),
                   dict(drift_uncertainty=60), dict(drawdown=True, underwater=True), dict(vol_target=(0.1, 0.9))):
            got = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, downside=0.0, **kw))
            assert got == {"raises": ["McpError", "libmcport error -1: ctx is NULL"]}, (kw, got)
            same = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, **kw))
            assert "calls" in same and "downside" not in same.get("keys", []), kw
        got = front_end_cases.record(rec, lambda: simulate_bootstrap(np.full((30, 3), 0.01), w, n_steps=5, n_paths=64, downside=True))
        assert got == {"raises": ["McpError", "libmcport error -1: ctx is NULL"]}
        for bad in (False, math.nan, "rf"):
            got = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, downside=bad))
            assert got["raises"][0] == "ValueError" and got["raises"][1].startswith("downside must be")
        got = front_end_cases.record(rec, lambda: simulate_paths(mu, cov, w, n_steps=5, n_paths=64, downside=0.0, as_array=True))
        assert got == {"raises": ["ValueError", "downside fills the 'downside' block of the result dicts: not with as_array"]}
        got = front_end_cases.record(rec, lambda: simulate_sweep(mu, cov, weights=w, n_steps=5, n_paths=64, downside=0.0))
        assert got["raises"][0] == "ValueError" and got["raises"][1].startswith("simulate_sweep does not take downside")


def test_the_result_block_from_the_calls_arrays():
    x, tau, pivot = _samples()["plain"]
    rec = ref_.raw_record(x, pivot, tau)
    sums = np.array([rec, rec], _ffi.DOWNSIDE_SUMS_DTYPE)
    stats = np.array([_ffi.downside_finish(rec, tau, pivot)] * 2, _ffi.DOWNSIDE_STATS_DTYPE)
    hz = np.array([[stats[0], stats[1]]] * 3, _ffi.DOWNSIDE_STATS_DTYPE)
    blocks = downside.downside_blocks(stats, sums, tau, hz)
    assert len(blocks) == 2 and set(blocks[0]) == set(downside.STAT_FIELDS) | {"threshold", "sums", "horizons"}
    assert blocks[1]["threshold"] == tau and blocks[1]["sums"]["n"] == x.size and isinstance(blocks[1]["sums"]["n_below"], int)
    assert len(blocks[0]["horizons"]) == 3 and blocks[0]["horizons"][2]["p_below"] == blocks[0]["p_below"]
    assert downside.finish(blocks[0]["sums"], tau, pivot)["sortino"] == blocks[0]["sortino"]
    assert "horizons" not in downside.downside_blocks(stats, sums, tau)[0]


# ---- 7. the host selftest carries the finish function and the arm / disarm rule -----------------------------------------------------

def test_the_host_selftest_covers_finish_and_the_arm_disarm_rule():
    """tests/test_host_unit_cpu.py builds and runs the program under the sanitizers; here: that its main runs the downside cases and
    that they hold the rule -- armed, a failing call, then a plain call must not write."""
    text = open(os.path.join(CSRC, "host_selftest.cpp")).read()
    main = text[text.index("int main()"):]
    assert "run_downside();" in main
    body = text[text.index("static void run_downside()"):text.index("int main()")]
    assert "mcp_downside_finish(&four" in body and "std::isnan(o.downside_std)" in body and "o.downside_std == 1e-4" in body
    assert "const DownsideArm failing = arm.take();" in body and "const DownsideArm plain = arm.take();" in body
    assert "!plain.on && !plain.stats_out && !plain.sums_out && !plain.hz_stats_out" in body
    host = open(os.path.join(CSRC, "mcp_host.cpp")).read()
    assert "int mcp_downside_finish(" in host and "DownsideArm DownsideArm::take()" in host      # pure host code: the selftest links it
    api = open(os.path.join(CSRC, "mcp_api.cpp")).read()
    assert "const DownsideArm ds = c->downside.take();" in api

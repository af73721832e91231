"""CPU checks of the sweep's series statistics (SPEC.md 5.24): the NumPy restatement (tests/sweep_perf_ref.py) against numbers the
reference's own functions gave (tests/golden/ref_sweep_perf.npz) and against metrics.py; mcp_sweep_perf_finish against
sweep.performance_finish bit for bit on crafted records; every argument rule of mcp_sweep_historical_perf with no device; the
extension header against its binding; run_sweep / select_optimum with the extra methods on a patched scorer; the stand-alone
selftest program.

Bars (SPEC.md section 6), none of them measured: a sum of n <= 9000 binary64 terms in another association is within
1e-12 sum|summand| of ours (5.22 shows n u < 1e-12 there); a finished figure, the wealth product and the drawdown are within
1e-12 max(1, |.|) of the reference's; an optimum index is exact (the generator asserts the best and the runner-up are more than
1e-9 apart, three orders above that bar)."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import sweep_perf_ref as ref_
from sweep_perf_cases import CASES, FIGURES, TOL, assert_goldens, case_inputs, case_records, close, golden
from monte_carlo_portfolio_amd import _ffi, metrics, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcport_sweep_perf.h")
CSRC = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


# ---- 1. the restatement against the reference's numbers and against metrics.py ----------------------------------------------------------

@pytest.mark.parametrize("name,rf,ann", CASES)
def test_restatement_meets_the_reference(name, rf, ann):
    assert golden()["risk_free"] == [0.0, 0.03] and golden()["ann_factors"] == [12, 52]
    rec = case_records(name, rf, ann)
    assert_goldens(name, rf, ann, rec, sweep.performance_finish(rec, ann))
    # the sums against another association: NumPy's matrix product and pairwise sums over the same series
    returns, W = case_inputs(name)
    X = returns @ W.T                                    # [R, P]
    E = X - rf / ann
    neg = E < 0.0
    assert (rec["n"] == len(returns)).all() and (rec["n_neg"] == neg.sum(0)).all()     # no excess return is within an ulp of 0
    assert (np.abs(rec["S"] - E.sum(0)) <= TOL * np.abs(E).sum(0)).all()
    assert (np.abs(rec["S_neg"] - np.where(neg, E, 0.0).sum(0)) <= TOL * np.abs(E).sum(0)).all()
    D = (E - E.mean(0)) ** 2
    assert (np.abs(rec["M2"] - D.sum(0)) <= TOL * D.sum(0)).all()
    mean_neg = np.where(neg, E, 0.0).sum(0) / neg.sum(0)
    Dn = np.where(neg, (E - mean_neg) ** 2, 0.0)
    assert (np.abs(rec["M2_neg"] - Dn.sum(0)) <= TOL * Dn.sum(0)).all()
    # the rows of the drawdown: the trough is where the wealth curve is deepest below its running maximum, the peak is that maximum
    wealth = np.cumprod(1.0 + X, axis=0)
    peak = np.maximum.accumulate(wealth, axis=0)
    for p in range(0, W.shape[0], 17):
        t, k = int(rec["trough_row"][p]), int(rec["peak_row"][p])
        assert 0 <= k <= t < len(returns) and int(np.argmin((wealth[:, p] - peak[:, p]) / peak[:, p])) == t
        assert int(np.argmax(wealth[:t + 1, p])) == k


def test_restatement_agrees_with_metrics_on_single_series():
    """One asset at weight 1: x_r = 0.0 + r_r * 1.0 is the series itself, so metrics.py sees the very numbers the restatement walks."""
    rs = np.random.RandomState(7)
    for R, rf, ann in ((2, 0.0, 12), (13, 0.03, 12), (53, 0.03, 52), (252, 0.02, 252)):
        r = 0.03 * rs.standard_normal(R) + 0.004
        rec = ref_.raw_records(r[:, None], np.ones((1, 1)), rf, ann)
        fin = sweep.performance_finish(rec, ann)
        one = ref_.finish(rec[0], ann)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = {"sharpe_ratio": metrics.sharpe_ratio(r, rf, ann), "sortino_ratio": metrics.sortino_ratio(r, rf, ann),
                    "annual_volatility": metrics.annual_volatility(r, ann), "annual_return": metrics.annual_return(r, ann),
                    "max_drawdown": metrics.max_drawdown(r)}
            for k, v in want.items():
                if np.isnan(v):                              # one negative excess return: np.std of one value at ddof 1
                    assert rec["n_neg"][0] == 1 and np.isnan(fin[k][0]) and np.isnan(one[k])
                else:
                    close(fin[k], [v], (R, k))
                    close([one[k]], [v], (R, k))
        assert rec["prod"][0] == np.cumprod(1.0 + r)[-1] and rec["mdd"][0] == metrics.max_drawdown(r)   # the same sequential products


# ---- 2. the finish: the library against sweep.performance_finish ----------------------------------------------------------------------

def crafted_records():
    """Records through every branch of the finish: n_neg 0 / 1 / 2, a zero std, a zero drawdown, a NaN drawdown, a zero downside_std
    under a negative, a positive and a zero mean, and seeded random ones."""
    rows = [
        (4, 2, 1, 3, 1.0, -0.75, 0.75, 0.0625, 1.5, -0.25),
        (4, 0, 0, 0, 1.0, 0.0, 0.75, 0.0, 1.5, 0.0),                    # n_neg = 0 and mdd == 0
        (4, 1, 0, 1, 1.0, -0.25, 0.75, 0.0, 1.5, -0.5),                 # n_neg = 1: NaN
        (4, 4, 0, 3, -1.0, -1.0, 0.0, 0.0, 0.5, -0.5),                  # std == 0, downside_std == 0, mean < 0
        (4, 2, 0, 3, 1.0, -0.5, 0.75, 0.0, 1.5, -0.5),                  # downside_std == 0, mean > 0
        (4, 2, 0, 3, 0.0, -0.5, 0.75, 0.0, 1.5, -0.5),                  # downside_std == 0, mean == 0
        (4, 1, -1, -1, -0.5, -1.0, 0.75, 0.0, 0.0, math.nan),           # NaN mdd, wealth 0
        (13, 5, 2, 7, 0.0371, -0.0912, 0.0123, 0.0021, 1.0374, -0.0816),
        (4096, 2011, 100, 3000, 1.7, -16.2, 0.41, 0.13, 5.2, -0.31),
    ]
    rs = np.random.RandomState(11)
    for _ in range(40):
        n = int(rs.randint(2, 4097))
        nn = int(rs.randint(0, min(n, 6)))
        rows.append((n, nn, 0, n - 1, rs.normal(0, 1), -abs(rs.normal(0, 1)), abs(rs.normal(0, 1)), abs(rs.normal(0, 0.1)),
                     math.exp(rs.normal(0, 1)), -rs.uniform(0, 1)))
    return np.array(rows, _ffi.SWEEP_PERF_SUMS_DTYPE)


@pytest.mark.parametrize("ann", (12, 52, 252, 4.0, 0.5))
def test_library_finish_equals_the_python_finish(mcp_lib, ann):
    sums = crafted_records()
    got = np.zeros(len(sums), _ffi.SWEEP_PERF_STATS_DTYPE)
    for p in range(len(sums)):
        assert mcp_lib.mcp_sweep_perf_finish(vp(sums[p:p + 1]), float(ann), vp(got[p:p + 1])) == 0
    want = sweep.performance_finish(sums, ann)
    for k in ("sharpe_ratio", "sortino_ratio", "annual_volatility", "max_drawdown"):
        ok = ~np.isnan(want[k])                              # a NaN's sign and payload are the host's: only its place is compared
        assert np.array_equal(np.isnan(got[k]), ~ok), k
        assert np.array_equal(np.ascontiguousarray(got[k][ok]).view(np.uint64), want[k][ok].view(np.uint64)), k
    for k in ("annual_return", "calmar"):                    # through pow: the library's libm against NumPy's
        nan = np.isnan(want[k])
        assert np.array_equal(np.isnan(got[k]), nan), k
        close(got[k][~nan], want[k][~nan], k)
    assert np.array_equal(got["peak_row"], sums["peak_row"]) and np.array_equal(got["trough_row"], sums["trough_row"])
    # the stated values of the hand-made records
    assert want["sortino_ratio"][1] == sums["S"][1] / 4 / 1e-4 * np.sqrt(np.float64(ann)) and want["calmar"][1] == 0.0
    assert np.isnan(want["sortino_ratio"][2]) and np.isfinite(want["sharpe_ratio"][2])
    assert want["sharpe_ratio"][3] == 0.0 and want["annual_volatility"][3] == 0.0 and want["sortino_ratio"][3] == -np.inf
    assert want["sortino_ratio"][4] == np.inf and np.isnan(want["sortino_ratio"][5]) and want["sharpe_ratio"][5] == 0.0
    assert np.isnan(want["max_drawdown"][6]) and np.isnan(want["calmar"][6]) and want["annual_return"][6] == -1.0
    # and the scalar restatement agrees with the vector one
    for p in range(len(sums)):
        one = ref_.finish(sums[p], ann)
        for k in FIGURES:
            assert one[k] == want[k][p] or (math.isnan(one[k]) and np.isnan(want[k][p])) or \
                (k in ("annual_return", "calmar") and abs(one[k] - want[k][p]) <= TOL * max(1.0, abs(want[k][p]))), (p, k)


def test_finish_rules(mcp_lib):
    sums = crafted_records()[:1]
    out = np.zeros(1, _ffi.SWEEP_PERF_STATS_DTYPE)
    assert mcp_lib.mcp_sweep_perf_finish(None, 12.0, vp(out)) == _ffi.MCP_E_ARG
    assert mcp_lib.mcp_sweep_perf_finish(vp(sums), 12.0, None) == _ffi.MCP_E_ARG
    for ann in (0.0, -12.0, math.nan, math.inf):
        assert mcp_lib.mcp_sweep_perf_finish(vp(sums), ann, vp(out)) == _ffi.MCP_E_ARG and b"ann_factor" in mcp_lib.mcp_last_error()
        with pytest.raises(ValueError, match="ann_factor"):
            sweep.performance_finish(sums, ann)
    assert not out.view(np.uint8).any()


# ---- 3. the argument rules, without a device --------------------------------------------------------------------------------------------

def test_every_rule_of_the_call_with_no_device(mcp_lib):
    N, R, P = 3, 5, 4
    ret = np.full((R, N), 0.01)
    W = np.full((P, N), 0.25)
    stats = np.zeros(P, _ffi.SWEEP_PERF_STATS_DTYPE)
    sums = np.zeros(P, _ffi.SWEEP_PERF_SUMS_DTYPE)

    def call(N=N, R=R, P=P, returns=ret, W=W, rf=0.03, ann=12.0, sums_out=sums, stats_out=stats):
        rc = mcp_lib.mcp_sweep_historical_perf(None, N, R, P, None if returns is None else vp(returns), None if W is None else vp(W),
                                               rf, ann, None if sums_out is None else vp(sums_out),
                                               None if stats_out is None else vp(stats_out))
        return rc, mcp_lib.mcp_last_error().decode()
    assert call() == (_ffi.MCP_E_ARG, "ctx is NULL")                       # everything else in order: the context is looked at last
    assert call(sums_out=None) == (_ffi.MCP_E_ARG, "ctx is NULL")          # sums_out may be NULL
    assert call(P=0, W=None, stats_out=None) == (_ffi.MCP_E_ARG, "ctx is NULL")
    assert call(R=2) == (_ffi.MCP_E_ARG, "ctx is NULL") and call(N=1) == (_ffi.MCP_E_ARG, "ctx is NULL")
    for change, text in ((dict(N=0), "n_assets=0 outside [1,64]"), (dict(N=65), "n_assets=65 outside [1,64]"),
                         (dict(R=1), "n_rows=1 outside [2,4096]"), (dict(R=4097), "n_rows=4097 outside [2,4096]"),
                         (dict(R=0), "n_rows=0"), (dict(P=-1), "n_portfolios=-1 < 0"), (dict(ann=0.0), "ann_factor=0"),
                         (dict(ann=-12.0), "ann_factor=-12"), (dict(ann=math.inf), "ann_factor=inf"), (dict(ann=math.nan), "ann_factor="),
                         (dict(rf=math.nan), "risk_free="), (dict(rf=-math.inf), "risk_free=-inf"), (dict(returns=None), "returns is NULL"),
                         (dict(P=0, returns=None), "returns is NULL"), (dict(W=None), "W is NULL"), (dict(stats_out=None), "stats_out is NULL")):
        rc, why = call(**change)
        assert rc == _ffi.MCP_E_ARG and text in why, (change, why)
    for (r, i), bad in (((0, 0), math.nan), ((2, 1), math.inf), ((R - 1, N - 1), -math.inf)):
        a = ret.copy()
        a[r, i] = bad
        a[R - 1, N - 1] = bad                                              # a later one: the first is named
        rc, why = call(returns=a)
        assert rc == _ffi.MCP_E_ARG and f"returns[{r * N + i}] (row {r}, asset {i}) is not finite" == why
        w = W.copy()
        w[min(r, P - 1), i] = bad
        rc, why = call(W=w)
        assert rc == _ffi.MCP_E_ARG and f"W[{min(r, P - 1) * N + i}] (portfolio {min(r, P - 1)}, asset {i}) is not finite" == why
    rc, why = call(returns=np.full((R, N), math.nan), W=np.full((P, N), math.nan))
    assert "returns[0]" in why                                             # returns before W
    assert not stats.view(np.uint8).any() and not sums.view(np.uint8).any()


def test_front_end_refusals_are_worded_as_score_portfolios_words_them():
    R, W = np.full((5, 3), 0.01), np.full((4, 3), 0.25)
    for call in (lambda **k: sweep.score_performance(k.get("R", R), k.get("W", W)),
                 lambda **k: sweep.score_portfolios(k.get("R", R), np.zeros(3), np.eye(3), k.get("W", W), 0.0)):
        for kw, text in ((dict(W=np.zeros(3)), r"W must be a \[P, N\] matrix, got shape \(3,\)"),
                         (dict(R=np.zeros((5, 2))), r"returns must be an \[R, 3\] matrix like the 3 columns of W, got shape \(5, 2\)"),
                         (dict(R=np.where(np.arange(15).reshape(5, 3) >= 7, np.nan, 0.01)),
                          r"NaN or infinite values in returns \(first: row 2, asset 1\); 8 in all, drop them first"),
                         (dict(W=np.where(np.arange(12).reshape(4, 3) == 11, np.inf, 0.25)),
                          r"NaN or infinite values in W \(first: portfolio 3, asset 2\); 1 in all, drop them first")):
            with pytest.raises(ValueError, match=text):
                call(**kw)
    for kw, text in ((dict(R=R[:1]), "at least 2 rows"), (dict(ann_factor=0), "ann_factor=0"), (dict(ann_factor=math.inf), "ann_factor=inf"),
                     (dict(risk_free=math.nan), "risk_free=nan")):
        with pytest.raises(ValueError, match=text):
            sweep.score_performance(kw.pop("R", R), W, **kw)
    out = sweep.score_performance(R, np.empty((0, 3)), raw=True)          # P = 0: no device, empty arrays of the right types
    assert sorted(out) == sorted(sweep.PERFORMANCE_KEYS + ("n", "n_neg", "S", "S_neg", "M2", "M2_neg", "prod", "mdd"))
    assert all(v.shape == (0,) for v in out.values()) and out["peak_row"].dtype == np.int32 and out["calmar"].dtype == np.float64
    assert sorted(sweep.score_performance(R, np.empty((0, 3)))) == sorted(sweep.PERFORMANCE_KEYS)


# ---- 4. header / binding / library -------------------------------------------------------------------------------------------------------

def test_extension_header_binding_and_library_agree(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    assert sorted(protos) == sorted(_ffi.SWEEP_PERF_SIGNATURES) == ["mcp_sweep_historical_perf", "mcp_sweep_perf_finish"]
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, params in protos.items():
        assert len(params.split(",")) == len(_ffi.SWEEP_PERF_SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(mcp_lib, name).argtypes == _ffi.SWEEP_PERF_SIGNATURES[name][1]
    assert [p.split()[-1].lstrip("*") for p in protos["mcp_sweep_historical_perf"].split(",")] == [
        "ctx", "n_assets", "n_rows", "n_portfolios", "returns", "W", "risk_free", "ann_factor", "sums_out", "stats_out"]
    assert [p.split()[-1].lstrip("*") for p in protos["mcp_sweep_perf_finish"].split(",")] == ["sums", "ann_factor", "out"]
    for table in (_ffi.SIGNATURES, _ffi.EXTENSION_SIGNATURES, _ffi.SPEND_SIGNATURES, _ffi.LIFE_SIGNATURES, _ffi.BAND_SIGNATURES,
                  _ffi.VOLTARGET_SIGNATURES, _ffi.UNDERWATER_SIGNATURES, _ffi.UNCERTAIN_SIGNATURES, _ffi.DOWNSIDE_SIGNATURES,
                  _ffi.RELATIVE_SIGNATURES):
        assert not set(table) & set(protos)
    for struct, dtype in (("mcp_sweep_perf_sums", _ffi.SWEEP_PERF_SUMS_DTYPE), ("mcp_sweep_perf_stats", _ffi.SWEEP_PERF_STATS_DTYPE)):
        fields = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        got = [(decl.split()[0], n.strip()) for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert [n for _, n in got] == list(dtype.names), struct
        assert [{"int32_t": np.int32, "double": np.float64}[t] for t, _ in got] == [dtype[n] for n in dtype.names], struct
    assert _ffi.SWEEP_PERF_SUMS_DTYPE.itemsize == 64 and _ffi.SWEEP_PERF_STATS_DTYPE.itemsize == 56
    assert '#include "mcport.h"' in text and 'extern "C"' in text and "MCP_ABI_VERSION" not in text
    assert mcp_lib.mcp_abi_version() == _ffi.MCP_ABI_VERSION == 4
    assert "mcp_sweep_perf" not in open(os.path.join(ROOT, "include", "mcport.h")).read()   # the main header is the parent's


def test_c99_compile_and_link_of_the_new_prototypes(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "sp.c"
    src.write_text(r'''
        #include <stdio.h>
        #include "mcport_sweep_perf.h"
        int main(void) {
            mcp_sweep_perf_sums s = {4, 2, 1, 3, 1.0, -0.75, 0.75, 0.0625, 1.5, -0.25};
            mcp_sweep_perf_stats o;
            double r[4] = {0.01, 0.02, 0.03, 0.04}, w[2] = {0.5, 0.5};
            if (mcp_sweep_perf_finish(&s, 4.0, &o) != MCP_OK || o.sharpe_ratio != 1.0 || o.sortino_ratio != 2.0 || o.calmar != 2.0) return 1;
            if (mcp_sweep_historical_perf(NULL, 2, 2, 1, r, w, 0.0, 12.0, NULL, &o) != MCP_E_ARG) return 2;
            printf("%s|%d %d %d\n", mcp_last_error(), (int)sizeof s, (int)sizeof o, (int)o.trough_row);
            return 0;
        }''')
    exe = tmp_path / "sp"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ctx is NULL|64 56 3", (out.returncode, out.stdout, out.stderr)


# ---- 5. the extra methods of the sweep, on a patched scorer ----------------------------------------------------------------------------

def test_select_optimum_of_the_extra_methods():
    nan, inf = math.nan, math.inf
    assert sweep.EXTRA_METHODS == ("Sortino", "Max Drawdown", "Calmar") and not set(sweep.EXTRA_METHODS) & set(sweep.METHODS)
    assert sweep.METHODS == ("Monte Carlo", "VaR", "CVaR", "MPT", "Equal Weight")
    for m in sweep.EXTRA_METHODS:
        assert sweep.select_optimum(m, np.array([0.5, 2.0, 2.0, 1.0])) == 1                   # argmax, the first of a tie
        assert sweep.select_optimum(m, np.array([nan, inf, -3.0, -1.0, nan, -1.0])) == 3      # over the finite scores alone
        assert sweep.select_optimum(m, np.array([nan, -inf, -7.0])) == 2
        with pytest.raises(ValueError, match="no portfolio has a finite"):
            sweep.select_optimum(m, np.array([nan, inf, -inf]))
        with pytest.raises(ValueError, match="no portfolio satisfied"):
            sweep.select_optimum(m, np.array([]))
    assert sweep.select_optimum("Max Drawdown", np.array([-0.4, -0.1, -0.2])) == 1            # the drawdown closest to 0
    assert sweep.select_optimum("Monte Carlo", np.array([1.0, 3.0])) == 1 and sweep.select_optimum("VaR", np.array([1.0, 3.0])) == 0


def test_run_sweep_with_the_extra_methods(monkeypatch):
    rs = np.random.RandomState(3)
    returns = 0.02 * rs.standard_normal((13, 3))
    seen = []

    def fake_portfolios(R, mean, cov, W, rf, alpha=0.95, device=0):
        P = len(W)
        seen.append(("portfolios", rf))
        return {"port_return": W @ mean, "port_std": np.sqrt(np.einsum("pi,ij,pj->p", W, cov, W)), "sharpe": np.arange(P, dtype=float),
                "var_95": -np.arange(P, dtype=float), "cvar_95": -np.arange(P, dtype=float)}

    def fake_performance(R, W, risk_free=0.0, ann_factor=12, device=0, raw=False):
        seen.append(("performance", risk_free, ann_factor))
        rec = ref_.raw_records(R, W, risk_free, ann_factor)
        out = sweep.performance_finish(rec, ann_factor)
        out["sortino_ratio"][5] = np.nan                    # a NaN score in front of the optimum is skipped, not returned
        out["sortino_ratio"][6] = np.inf
        return out
    monkeypatch.setattr(sweep, "score_portfolios", fake_portfolios)
    monkeypatch.setattr(sweep, "score_performance", fake_performance)
    risks0, rets0, W0, metric0, _ = sweep.run_sweep(returns, "Monte Carlo", 40, seed=9)
    state0 = np.random.get_state()
    assert seen == [("portfolios", 3.0)]
    for method, key in (("Sortino", "sortino_ratio"), ("Max Drawdown", "max_drawdown"), ("Calmar", "calmar")):
        del seen[:]
        risks, rets, W, metric, opt = sweep.run_sweep(returns, method, 40, seed=9, risk_free=0.03, annual_factor=12)
        state = np.random.get_state()
        assert np.array_equal(W, W0) and np.array_equal(risks, risks0) and np.array_equal(rets, rets0)     # drawn as "Monte Carlo"
        assert state[2] == state0[2] and np.array_equal(state[1], state0[1])                               # and the stream left there
        assert seen == [("portfolios", 3.0), ("performance", 0.03, 12)]
        want = fake_performance(sweep.sweep_inputs(returns, 12)[0], W0, 0.03, 12)[key]
        assert np.array_equal(metric, want, equal_nan=True) and len(metric) == len(W)
        finite = np.where(np.isfinite(want), want, -np.inf)
        assert opt == int(np.argmax(finite)) and np.isfinite(metric[opt]) and opt not in ((5, 6) if method == "Sortino" else ())
    with pytest.raises(ValueError, match="unknown method"):
        sweep.run_sweep(returns, "Sterling", 40)
    # run_all_methods still walks METHODS alone, on one stream, and never asks for the series statistics
    del seen[:]
    out = sweep.run_all_methods(returns, 40, seed=9)
    assert tuple(out) == sweep.METHODS and all(s[0] == "portfolios" for s in seen) and len(seen) == 5
    assert np.array_equal(out["Monte Carlo"]["all_weights"], W0)
    np.random.seed(9)
    want_W = [sweep._draw_weights_loop(3, 40) for _ in range(4)]
    for m, w in zip(sweep.METHODS[:4], want_W):
        assert np.array_equal(out[m]["all_weights"], w), m


# ---- 6. the stand-alone program ------------------------------------------------------------------------------------------------------------

def test_the_selftest_program_builds_and_passes(tmp_path):
    """`make sweep-perf-selftest`: csrc/sweep_perf_selftest.cpp with mcp_host.cpp, a plain C++ compiler, AddressSanitizer + UBSan, no
    Python in the process."""
    r = subprocess.run(["make", "-C", CSRC, "sweep-perf-selftest", f"BUILD={tmp_path}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sweep_perf_selftest ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])

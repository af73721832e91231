"""CPU checks of the resampled historical sweep (SPEC.md 5.25): the NumPy restatement (tests/sweep_boot_ref.py) against NumPy's own
percentile of the materialised resample and against math.fsum; mcp_sweep_boot_counts against the bootstrap's restatement; every
argument rule of mcp_sweep_resampled with no device; the extension header against its binding; the front end's refusals, the summary
on hand-built scores, run_resampled_sweep on patched scorers; the stand-alone selftest program; the bootstrap law on the restatement.

Bars, none of them measured: an order statistic is exact; a sum of n binary64 terms taken in another association is within
gamma_n sum|terms| of ours, gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability, section 4.2), here with n = R + 2:
R - 1 additions, the rounding of a term's product and one to spare."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sweep_boot_ref as ref_
from bootstrap_ref import boot_indices
from monte_carlo_portfolio_amd import _ffi, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcport_sweep_boot.h")
CSRC = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
SEED = 0x1F2E3D4C5B6A7988
BEGIN = 2 ** 32 - 3
INF = math.inf


def market(R, N, P, seed):
    rs = np.random.RandomState(seed)
    return 0.02 * rs.standard_normal((R, N)) + 3e-4, rs.dirichlet(np.ones(N), size=P)


@pytest.fixture(scope="module")
def case():
    """One restatement shared by the tests of sections 1 to 3: 60 rows, 5 assets, 20 portfolios, 50 replicates per block length."""
    returns, W = market(60, 5, 20, 17)
    return returns, W, {b: ref_.resampled(returns, W, 0.03, 12, 0.95, SEED, BEGIN, 50, b, parts=True) for b in (1.0, 4.0, INF)}


# ---- 1. the order statistic ------------------------------------------------------------------------------------------------------------

def test_var_is_numpys_percentile_of_the_materialised_resample(case):
    returns, W, outs = case
    for block, out in outs.items():
        rows = ref_.replicate_rows(SEED, BEGIN, 50, 60, block)           # [R, B]
        for q in range(50):
            want = np.percentile(out["y"][:, rows[:, q]], (1 - 0.95) * 100, axis=1)
            assert want.tobytes() == np.ascontiguousarray(out["var_95"][:, q]).tobytes(), (block, q)
    for alpha in (0.5, 0.99, 0.9):                                        # gamma >= 0.5 takes the other branch of the lerp
        out = ref_.resampled(returns[:13], W[:4], 0.0, 12, alpha, SEED, 0, 30, 1.0, parts=True)
        rows = ref_.replicate_rows(SEED, 0, 30, 13, 1.0)
        for q in range(30):
            want = np.percentile(out["y"][:, rows[:, q]], (1 - alpha) * 100, axis=1)
            assert want.tobytes() == np.ascontiguousarray(out["var_95"][:, q]).tobytes(), (alpha, q)


# ---- 2. the moments against math.fsum ----------------------------------------------------------------------------------------------------

def test_moments_are_within_the_association_bound_of_fsum(case):
    returns, W, outs = case
    R = 60
    n = R + 2
    gamma_n = n * 2.0 ** -53 / (1.0 - n * 2.0 ** -53)                      # derived (module docstring), not measured
    for block, out in outs.items():
        c = out["counts"].astype(np.float64)
        for p in range(0, 20, 3):
            for q in range(0, 50, 7):
                terms = [float(c[q, r] * out["y"][p, r]) for r in range(R)]
                assert abs(out["S"][p, q] - math.fsum(terms)) <= gamma_n * math.fsum(abs(t) for t in terms), (block, p, q)
                m = out["S"][p, q] / np.float64(R)
                terms = [float(c[q, r] * ((out["y"][p, r] - m) * (out["y"][p, r] - m))) for r in range(R)]
                assert abs(out["M2"][p, q] - math.fsum(terms)) <= gamma_n * math.fsum(terms), (block, p, q)
                assert out["port_return"][p, q] == m * 12 and out["port_std"][p, q] == np.sqrt(out["M2"][p, q] / np.float64(R - 1) * 12)


# ---- 3. the clamp ----------------------------------------------------------------------------------------------------------------------------

def test_cvar_stays_between_the_smallest_value_and_var(case):
    for block, out in case[2].items():
        assert (out["cvar_95"] <= out["var_95"]).all() and (out["cvar_95"] >= out["lo"]).all(), block
        assert (out["tc"] >= 1).all() and (out["lo"] <= out["var_95"]).all()
    # a tail of one value repeated: three times 0.1 over 3 is above 0.1, the clamp brings it back
    out = ref_.score(np.full((4, 1), 0.1), np.ones((1, 1)), 0.0, 1, 0.5, np.array([[3, 1, 0, 0]], np.uint16), parts=True)
    assert out["ts"][0, 0] / 3 > 0.1 and out["cvar_95"][0, 0] == 0.1 == out["var_95"][0, 0]


# ---- 4. the host counts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,B,block,begin", ((2, 64, 1.0, 0), (13, 65, 4.0, BEGIN), (64, 10, INF, 7), (300, 5, 1.0, BEGIN), (4096, 2, 8.0, 1)))
def test_host_counts_are_the_bincount_of_the_bootstraps_rows(mcp_lib, R, B, block, begin):
    got = sweep.resample_counts(R, B, block, SEED, begin)
    rows = boot_indices(SEED, np.uint64(begin) + np.arange(B, dtype=np.uint64), R, R, block)
    assert got.dtype == np.uint16 and got.shape == (B, R)
    for q in range(B):
        assert np.array_equal(got[q], np.bincount(rows[:, q], minlength=R)), q
    assert (got.sum(axis=1) == R).all()
    if block == INF:
        assert (got == 1).all()
    assert np.array_equal(got, ref_.replicate_counts(SEED, begin, B, R, block))


# ---- 5. the argument rules, without a device ----------------------------------------------------------------------------------------------

def test_every_rule_of_the_call_with_no_device(mcp_lib):
    N, R, P, B = 3, 5, 4, 6
    ret, W = np.full((R, N), 0.01), np.full((P, N), 0.25)
    sc, opt, cnt = np.zeros((5, P, B)), np.zeros((3, B), np.int32), np.zeros((B, R), np.uint16)

    def call(N=N, R=R, P=P, returns=ret, W=W, rf=0.03, ann=12.0, alpha=0.95, seed=1, begin=0, B=B, block=1.0, scores=sc, opt_=opt, counts=cnt):
        rc = mcp_lib.mcp_sweep_resampled(None, N, R, P, None if returns is None else vp(returns), None if W is None else vp(W), rf, ann,
                                         alpha, seed, begin, B, block, None if scores is None else vp(scores),
                                         None if opt_ is None else vp(opt_), None if counts is None else vp(counts))
        return rc, mcp_lib.mcp_last_error().decode()
    assert call() == (_ffi.MCP_E_ARG, "ctx is NULL")                       # everything else in order: the context is looked at last
    assert call(counts=None) == (_ffi.MCP_E_ARG, "ctx is NULL")            # counts_out may be NULL
    assert call(P=0, W=None, scores=None, opt_=None) == (_ffi.MCP_E_ARG, "ctx is NULL")
    assert call(B=0, W=None, scores=None, opt_=None) == (_ffi.MCP_E_ARG, "ctx is NULL")
    assert call(R=2, block=INF, begin=2 ** 64 - 1 - B) == (_ffi.MCP_E_ARG, "ctx is NULL")
    for change, text in ((dict(N=0), "n_assets=0 outside [1,64]"), (dict(N=65), "n_assets=65 outside [1,64]"),
                         (dict(R=1), "n_rows=1 outside [2,4096]"), (dict(R=4097), "n_rows=4097 outside [2,4096]"),
                         (dict(P=-1), "n_portfolios=-1 < 0"), (dict(B=-1), "n_replicates=-1 outside [0,4096]"),
                         (dict(B=4097), "n_replicates=4097 outside [0,4096]"), (dict(P=2 ** 15 + 1, B=4096), "exceeds 2^27"),
                         (dict(block=0.5), "block=0.5 must be >= 1"), (dict(block=math.nan), "block="), (dict(block=-INF), "block=-inf"),
                         (dict(begin=2 ** 64 - B), "wraps"), (dict(begin=2 ** 64 - 1, B=1), "wraps"),
                         (dict(ann=0.0), "ann_factor=0"), (dict(ann=-12.0), "ann_factor=-12"), (dict(ann=INF), "ann_factor=inf"),
                         (dict(ann=math.nan), "ann_factor="), (dict(rf=math.nan), "rf="), (dict(rf=-INF), "rf=-inf"),
                         (dict(alpha=0.0), "alpha=0 outside (0,1)"), (dict(alpha=1.0), "alpha=1 outside (0,1)"), (dict(alpha=math.nan), "alpha="),
                         (dict(returns=None), "returns is NULL"), (dict(P=0, returns=None), "returns is NULL"), (dict(W=None), "W is NULL"),
                         (dict(scores=None), "scores_out is NULL"), (dict(opt_=None), "opt_out is NULL")):
        rc, why = call(**change)
        assert rc == _ffi.MCP_E_ARG and text in why, (change, why)
    for (r, i), bad in (((0, 0), math.nan), ((2, 1), INF), ((R - 1, N - 1), -INF)):
        a = ret.copy()
        a[r, i] = bad
        a[R - 1, N - 1] = bad                                              # a later one: the first is named
        rc, why = call(returns=a)
        assert rc == _ffi.MCP_E_ARG and f"returns[{r * N + i}] (row {r}, asset {i}) is not finite" == why   # the wording of 5.24's scan
        w = W.copy()
        w[min(r, P - 1), i] = bad
        rc, why = call(W=w)
        assert rc == _ffi.MCP_E_ARG and f"W[{min(r, P - 1) * N + i}] (portfolio {min(r, P - 1)}, asset {i}) is not finite" == why
    rc, why = call(returns=np.full((R, N), math.nan), W=np.full((P, N), math.nan))
    assert "returns[0]" in why                                             # returns before W
    assert not sc.any() and not opt.any() and not cnt.any()
    # the host function's own rules
    for args, text in (((1, 0, 2, 1, 1.0), "n_rows=1"), ((1, 0, 4097, 5, 1.0), "n_replicates=4097"), ((1, 0, 2, 5, 0.0), "block=0"),
                       ((1, 2 ** 64 - 1, 2, 5, 1.0), "wraps")):
        assert mcp_lib.mcp_sweep_boot_counts(*args, vp(cnt)) == _ffi.MCP_E_ARG and text in mcp_lib.mcp_last_error().decode(), args
    assert mcp_lib.mcp_sweep_boot_counts(1, 0, 2, 5, 1.0, None) == _ffi.MCP_E_ARG and b"counts_out is NULL" == mcp_lib.mcp_last_error()
    assert mcp_lib.mcp_sweep_boot_counts(1, 0, 0, 5, 1.0, None) == 0 and not cnt.any()


def test_front_end_refusals_are_worded_as_score_portfolios_words_them():
    R, W = np.full((5, 3), 0.01), np.full((4, 3), 0.25)
    for call in (lambda **k: sweep.score_resampled(k.get("R", R), k.get("W", W), 0.0),
                 lambda **k: sweep.score_portfolios(k.get("R", R), np.zeros(3), np.eye(3), k.get("W", W), 0.0)):
        for kw, text in ((dict(W=np.zeros(3)), r"W must be a \[P, N\] matrix, got shape \(3,\)"),
                         (dict(R=np.zeros((5, 2))), r"returns must be an \[R, 3\] matrix like the 3 columns of W, got shape \(5, 2\)"),
                         (dict(R=np.where(np.arange(15).reshape(5, 3) >= 7, np.nan, 0.01)),
                          r"NaN or infinite values in returns \(first: row 2, asset 1\); 8 in all, drop them first"),
                         (dict(W=np.where(np.arange(12).reshape(4, 3) == 11, np.inf, 0.25)),
                          r"NaN or infinite values in W \(first: portfolio 3, asset 2\); 1 in all, drop them first")):
            with pytest.raises(ValueError, match=text):
                call(**kw)
    for kw, text in ((dict(R=R[:1]), "at least 2 rows"), (dict(R=np.zeros((4097, 3))), "at most 4096"), (dict(annual_factor=0), "annual_factor=0"),
                     (dict(annual_factor=math.inf), "annual_factor=inf"), (dict(rf=math.nan), "rf=nan"), (dict(alpha=1.0), "alpha=1.0"),
                     (dict(n_replicates=-1), "n_replicates=-1"), (dict(n_replicates=4097), "n_replicates=4097"), (dict(block=0.5), "block=0.5"),
                     (dict(block=math.nan), "block=nan"), (dict(replicate_begin=-1), "replicate_begin=-1"),
                     (dict(replicate_begin=2 ** 64 - 3, n_replicates=4), "replicate_begin="),
                     (dict(W=np.full((2 ** 15 + 1, 3), 0.25), n_replicates=4096), "exceed 2\\^27")):
        kw = dict(kw)
        with pytest.raises(ValueError, match=text):
            sweep.score_resampled(kw.pop("R", R), kw.pop("W", W), kw.pop("rf", 0.0), **kw)
    for P, B in ((0, 7), (4, 0), (0, 0)):                                 # no work: no device, arrays of the right shapes and types
        out = sweep.score_resampled(R, W[:P], 0.0, n_replicates=B, counts=True)
        assert sorted(out) == sorted(sweep.RESAMPLED_KEYS + ("opt", "counts"))
        assert all(out[k].shape == (P, B) and out[k].dtype == np.float64 for k in sweep.RESAMPLED_KEYS)
        assert list(out["opt"]) == ["Monte Carlo", "VaR", "CVaR"] and all(v.shape == (B,) and v.dtype == np.int32 for v in out["opt"].values())
        assert out["counts"].shape == (B, 5) and out["counts"].dtype == np.uint16 and (out["counts"].sum(axis=1) == 5).all()
    assert "counts" not in sweep.score_resampled(R, W[:0], 0.0, n_replicates=3)


# ---- 6. header / binding / library ---------------------------------------------------------------------------------------------------------

def test_extension_header_binding_and_library_agree(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    assert sorted(protos) == sorted(_ffi.SWEEP_BOOT_SIGNATURES) == ["mcp_sweep_boot_counts", "mcp_sweep_resampled"]
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, params in protos.items():
        assert len(params.split(",")) == len(_ffi.SWEEP_BOOT_SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(mcp_lib, name).argtypes == _ffi.SWEEP_BOOT_SIGNATURES[name][1]
    assert [p.split()[-1].lstrip("*") for p in protos["mcp_sweep_resampled"].split(",")] == [
        "ctx", "n_assets", "n_rows", "n_portfolios", "returns", "W", "rf", "ann_factor", "alpha", "seed", "replicate_begin", "n_replicates",
        "block", "scores_out", "opt_out", "counts_out"]
    assert [p.split()[-1].lstrip("*") for p in protos["mcp_sweep_boot_counts"].split(",")] == [
        "seed", "replicate_begin", "n_replicates", "n_rows", "block", "counts_out"]
    kinds = {"double": ctypes.c_double, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
    for name, params in protos.items():
        for p, bound in zip(params.split(","), _ffi.SWEEP_BOOT_SIGNATURES[name][1]):
            assert bound == (ctypes.c_void_p if "*" in p else kinds[p.split()[-2]]), (name, p)
    for table in (_ffi.SIGNATURES, _ffi.EXTENSION_SIGNATURES, _ffi.SPEND_SIGNATURES, _ffi.LIFE_SIGNATURES, _ffi.BAND_SIGNATURES,
                  _ffi.VOLTARGET_SIGNATURES, _ffi.UNDERWATER_SIGNATURES, _ffi.UNCERTAIN_SIGNATURES, _ffi.DOWNSIDE_SIGNATURES,
                  _ffi.RELATIVE_SIGNATURES, _ffi.SWEEP_PERF_SIGNATURES):
        assert not set(table) & set(protos)
    assert int(re.search(r"#define MCP_SWEEP_MAX_REPLICATES (\d+)", text).group(1)) == _ffi.MCP_SWEEP_MAX_REPLICATES == 4096
    main = open(os.path.join(ROOT, "include", "mcport.h")).read()
    assert int(re.search(r"#define MCP_SWEEP_MAX_ROWS (\d+)", main).group(1)) == _ffi.MCP_SWEEP_MAX_ROWS
    assert '#include "mcport.h"' in text and 'extern "C"' in text and "MCP_ABI_VERSION" not in text
    assert mcp_lib.mcp_abi_version() == _ffi.MCP_ABI_VERSION == 4
    assert "mcp_sweep_resampled" not in main and "mcp_sweep_boot" not in main            # the main header is the parent's


def test_c99_compile_and_link_of_the_new_prototypes(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "sb.c"
    src.write_text(r'''
        #include <stdio.h>
        #include "mcport_sweep_boot.h"
        int main(void) {
            double r[4] = {0.01, 0.02, 0.03, 0.04}, w[2] = {0.5, 0.5}, s[5 * 3];
            int32_t o[3 * 3];
            uint16_t c[3 * 2];
            int q, sum = 0;
            if (mcp_sweep_boot_counts(7u, 0u, 3, 2, 1.0, c) != MCP_OK) return 1;
            for (q = 0; q < 6; q++) sum += c[q];
            if (sum != 6 || c[0] + c[1] != 2) return 2;
            if (mcp_sweep_resampled(NULL, 2, 2, 1, r, w, 0.0, 12.0, 0.95, 7u, 0u, 3, 1.0, s, o, c) != MCP_E_ARG) return 3;
            printf("%s|%d\n", mcp_last_error(), MCP_SWEEP_MAX_REPLICATES);
            return 0;
        }''')
    exe = tmp_path / "sb"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ctx is NULL|4096", (out.returncode, out.stdout, out.stderr)


# ---- 7. the summary and the resampled run, on hand-built scores and patched scorers ------------------------------------------------------

def test_resample_summary_of_hand_built_scores():
    W = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])
    sharpe = np.array([[1.0, 2.0, 0.0, 3.0],
                       [1.0, 2.0, 5.0, 1.0],
                       [0.0, 2.0, 5.0, 4.0]])
    scores = {k: sharpe * (i + 1) for i, k in enumerate(sweep.RESAMPLED_KEYS)}
    scores["sharpe"] = sharpe
    first = np.argmax(sharpe, axis=0).astype(np.int32)                    # ties go to the first index: 0, 0, 1, 2
    assert list(first) == [0, 0, 1, 2]
    scores["opt"] = {"Monte Carlo": first, "VaR": np.array([2, 2, 2, 2], np.int32), "CVaR": np.array([1, 1, 0, 0], np.int32)}
    out = sweep.resample_summary(scores, W, point=0)
    for k in sweep.RESAMPLED_KEYS:
        x = scores[k]
        assert np.array_equal(out[k]["mean"], x.mean(axis=1)) and np.array_equal(out[k]["se"], x.std(axis=1, ddof=1))
        assert out[k]["interval"].shape == (2, 3) and np.array_equal(out[k]["interval"], np.percentile(x, [2.5, 97.5], axis=1))
    mc = out["Monte Carlo"]
    assert list(mc["wins"]) == [2, 1, 1] and mc["wins"].sum() == 4 and np.array_equal(mc["win_share"], [0.5, 0.25, 0.25])
    assert np.array_equal(mc["resampled_weights"], [0.625, 0.375])        # (2 (1, 0) + (.5, .5) + (0, 1)) / 4
    assert mc["point"] == 0 and mc["point_win_share"] == 0.5
    assert mc["point_top5_share"] == 0.5                                   # ceil(3 / 20) = 1: nobody strictly above it in replicates 0 and 1
    assert list(out["VaR"]["wins"]) == [0, 0, 4] and np.array_equal(out["VaR"]["resampled_weights"], [0.0, 1.0])
    assert out["VaR"]["point_win_share"] == 0.0 and list(out["CVaR"]["wins"]) == [2, 2, 0]
    only = sweep.resample_summary(scores, W, point={"CVaR": 1}, levels=(5, 50, 95))
    assert "point" not in only["Monte Carlo"] and only["CVaR"]["point"] == 1 and only["sharpe"]["interval"].shape == (3, 3)
    assert "point" not in sweep.resample_summary(scores, W)["VaR"]
    one = {k: (v[:, :1] if k != "opt" else {m: o[:1] for m, o in v.items()}) for k, v in scores.items()}
    assert np.isnan(sweep.resample_summary(one, W)["sharpe"]["se"]).all()  # one replicate has no standard error
    with pytest.raises(ValueError, match=r"scores\['port_return'\] must be a \[2, B\] matrix"):
        sweep.resample_summary(scores, W[:2])


def test_run_resampled_sweep_draws_as_run_sweep_and_leaves_the_stream_there(monkeypatch):
    rs = np.random.RandomState(3)
    returns = 0.02 * rs.standard_normal((13, 3))
    seen = []

    def fake_portfolios(R, mean, cov, W, rf, alpha=0.95, device=0):
        P = len(W)
        return {"port_return": W @ mean, "port_std": np.sqrt(np.einsum("pi,ij,pj->p", W, cov, W)), "sharpe": np.arange(P, dtype=float),
                "var_95": -np.arange(P, dtype=float), "cvar_95": -np.arange(P, dtype=float)}

    def fake_resampled(R, W, rf, annual_factor=12, alpha=0.95, n_replicates=1000, block=1.0, seed=0, replicate_begin=0, device=0, counts=False):
        seen.append((rf, annual_factor, alpha, n_replicates, block, seed, replicate_begin))
        out = ref_.resampled(R, W, rf, annual_factor, alpha, seed, replicate_begin, n_replicates, block)
        return {k: out[k] for k in ref_.FIGURES + ("opt",)}
    monkeypatch.setattr(sweep, "score_portfolios", fake_portfolios)
    monkeypatch.setattr(sweep, "score_resampled", fake_resampled)
    plain = {}
    for method in ("Monte Carlo", "VaR", "CVaR", "MPT"):
        plain[method] = sweep.run_sweep(returns, method, 40, seed=9)
        state0 = np.random.get_state()
        del seen[:]
        got = sweep.run_resampled_sweep(returns, method, 40, seed=9, n_replicates=25, block=2.0, resample_seed=77)
        state = np.random.get_state()
        assert state[2] == state0[2] and np.array_equal(state[1], state0[1])                        # the stream is where run_sweep leaves it
        assert len(got) == 6 and all(np.array_equal(a, b) for a, b in zip(got[:5], plain[method]))   # the tuple of run_sweep first
        assert seen == [(3.0, 12, 0.95, 25, 2.0, 77, 0)]
        summ, crit = got[5], "Monte Carlo" if method == "MPT" else method
        assert summ[crit]["point"] == got[4] and summ[crit]["wins"].sum() == 25 and len(summ[crit]["wins"]) == len(got[2])
        assert all("point" not in summ[m] for m in ref_.CRITERIA if m != crit)
        want = ref_.resampled(sweep.sweep_inputs(returns, 12)[0], got[2], 3.0, 12, 0.95, 77, 0, 25, 2.0)
        assert np.array_equal(summ[crit]["wins"], np.bincount(want["opt"][crit], minlength=len(got[2])))
        assert np.allclose(summ[crit]["resampled_weights"].sum(), 1.0)
    for method in ("Equal Weight", "Sortino", "Sterling"):
        with pytest.raises(ValueError, match="unknown method"):
            sweep.run_resampled_sweep(returns, method, 40)


# ---- 8. the stand-alone program --------------------------------------------------------------------------------------------------------------

def test_the_selftest_program_builds_and_passes(tmp_path):
    """`make sweep-boot-selftest`: csrc/sweep_boot_selftest.cpp with mcp_host.cpp, a plain C++ compiler, AddressSanitizer + UBSan, no
    Python in the process."""
    r = subprocess.run(["make", "-C", CSRC, "sweep-boot-selftest", f"BUILD={tmp_path}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sweep_boot_selftest ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- 9. the bootstrap law ------------------------------------------------------------------------------------------------------------------------

def test_the_bootstrap_law_on_the_restatement():
    """block = 1, one asset at weight 1, R = 64, B = 4096, ann = 1: the standard deviation over the replicates of port_return is within
    5 / sqrt(2 B) = 5.5 % of sqrt((R - 1) / R) s / sqrt(R) (sweep_boot_ref.LAW says why)."""
    assert (ref_.LAW["R"], ref_.LAW["B"]) == (64, 4096) and ref_.LAW["margin"] == 5.0 / math.sqrt(2 * 4096) < 0.0553
    returns, W = ref_.law_input()
    out = ref_.resampled(returns, W, 0.0, 1, 0.95, ref_.LAW["seed"], 0, ref_.LAW["B"], 1.0)
    ratio = ref_.law_ratio(returns, out["port_return"][0])
    print("std over replicates / sqrt((R-1)/R) s / sqrt(R) =", ratio)
    assert abs(ratio - 1.0) <= ref_.LAW["margin"], ratio

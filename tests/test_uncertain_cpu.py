"""CPU checks of drift uncertainty (SPEC.md 2.7 / 4.21 / 5.21): the two statements of the rule in uncertain_ref.py against each other and,
at M = 0, against oracle.np_oracle.simulate; uncertainty.drift_factor's three forms, drift_cov and drift_law (against a binary64 Monte
Carlo twin); the extension header against its binding; every argument rule and refusal of mcp_simulate_uncertain through the C ABI
with a context that touches no device, and of simulate_paths(drift_uncertainty=...) with no context; the seven ladder rows, what the
host selftest proves about them, and that a request with uncertainty never runs the lean step loop."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import front_end_cases
import uncertain_ref as ref_
from monte_carlo_portfolio_amd import _ffi, check_drift_uncertainty, drift_cov, drift_factor, drift_law, simulate, simulate_paths, simulate_sweep
from oracle import np_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcport_uncertain.h")
CSRC = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
SEED, ROWS, market = ref_.SEED, ref_.ROWS, ref_.market


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _variants(T):
    for family, compounding in ROWS:
        yield family, compounding, dict(drawdown=family == "dd", horizons=ref_.horizons_of(T) if family in ("hz", "cf") else (),
                                        flows=ref_.flows_of(T) if family == "cf" else None)


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,T,begin", [(3, 1, 1, 0), (5, 3, 2, 0), (6, 2, 5, (1 << 32) - 3)])
def test_the_two_statements_agree_bit_for_bit(N, K, T, begin):
    mu, L, W = market(N, K)
    paths = np.arange(begin, begin + 8, dtype=np.uint64)
    for M in (ref_.dense_factor(N), ref_.holed_factor(N)):
        for family, compounding, kw in _variants(T):
            vec = ref_.simulate(mu, L, M, W, T, SEED, paths, compounding, **kw)
            for i, p in enumerate(paths):
                v, q, h = ref_.loop_one_path(mu, L, M, W, T, SEED, int(p), compounding, **kw)
                assert np.array_equal(_bits(v), _bits(vec["V_T"][:, i])), (family, compounding, int(p))
                if kw["drawdown"]:
                    assert np.array_equal(_bits(q), _bits(vec["q"][:, i]))
                if len(kw["horizons"]):
                    assert np.array_equal(_bits(h), _bits(vec["V_h"][:, :, i]))


@pytest.mark.parametrize("compounding", ["simple", "log"])
def test_a_zero_factor_is_the_oracle_and_a_factor_moves_every_path(compounding):
    N, K, T, begin, n = 5, 3, 4, (1 << 32) - 20, 64
    mu, L, W = market(N, K)
    paths = np.arange(begin, begin + n, dtype=np.uint64)
    want = np_oracle.simulate(mu, L, W, T, n, SEED, path_begin=begin, compounding=compounding, exact=True)
    zero = np.zeros((N, N), np.float32)
    zero[1, 0] = -0.0
    got = ref_.simulate(mu, L, zero, W, T, SEED, paths, compounding)
    assert np.array_equal(_bits(got["V_T"]), _bits(want)) and np.array_equal(got["m"], np.tile(mu, (n, 1)))
    assert np.array_equal(_bits(ref_.simulate(mu, L, None, W, T, SEED, paths, compounding)["V_T"]), _bits(want))
    moved = ref_.simulate(mu, L, ref_.dense_factor(N), W, T, SEED, paths, compounding)
    assert not np.any(_bits(moved["V_T"]) == _bits(want))
    # common random numbers: the step normals are stream 0's, the drift normals stream 5's and no step's
    g = ref_.drift_normals(SEED, paths, N)
    assert g.shape == (n, 8) and not any(np.array_equal(g, np_oracle.step_normals(SEED, paths, t, N)) for t in range(T))
    nb2 = ref_.drift_normals(SEED, paths[:4], 5)            # nb = 2: normal m of block q is asset m nb + q
    x0 = np_oracle.philox4x32_10(np.uint64(0), np.uint64(5), paths[:4] & np.uint64(0xFFFFFFFF), paths[:4] >> np.uint64(32), SEED & 0xFFFFFFFF, SEED >> 32)
    x1 = np_oracle.philox4x32_10(np.uint64(1), np.uint64(5), paths[:4] & np.uint64(0xFFFFFFFF), paths[:4] >> np.uint64(32), SEED & 0xFFFFFFFF, SEED >> 32)
    for m in range(4):
        assert np.array_equal(nb2[:, 2 * m], np_oracle.normals(x0[m])) and np.array_equal(nb2[:, 2 * m + 1], np_oracle.normals(x1[m]))


def test_the_gpu_tests_cash_flow_schedule_ruins_some_paths_and_not_others():
    for N, K, T, begin, n in ref_.CASES:
        mu, L, W = market(N, K)
        ids = ref_.pick(n, begin)[:300]
        for make in (ref_.dense_factor, ref_.holed_factor):
            V = ref_.simulate(mu, L, make(N), W, T, SEED, (begin + ids).astype(np.uint64), flows=ref_.flows_of(T))["V_T"]
            assert 0.02 < np.mean(V == 0) < 0.98, (N, K, T, np.mean(V == 0))
    big = ref_.pick(ref_.TILE + 257, 3)
    assert {0, 63, ref_.TILE - 3, ref_.TILE, ref_.TILE + 3, ref_.TILE + 256} <= set(big.tolist()) and big.size < 200
    assert {197, 200, 203} <= set(ref_.pick(5000, (1 << 32) - 200).tolist())


# ---- 2. uncertainty.py ------------------------------------------------------------------------------------------------------------

def test_drift_factor_takes_the_three_forms():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((4, 4))
    cov = A @ A.T / 100 + 0.01 * np.eye(4)
    low = np.linalg.cholesky(cov)
    M = drift_factor(84, cov)
    assert M.dtype == np.float32 and M.flags.c_contiguous and np.array_equal(M, (low / math.sqrt(84.0)).astype(np.float32))
    assert np.array_equal(drift_factor(84, None, chol=low.astype(np.float32)), (np.tril(low.astype(np.float32)).astype(np.float64) / math.sqrt(84.0)).astype(np.float32))
    assert np.array_equal(drift_factor(cov / 84, cov), np.linalg.cholesky(cov / 84).astype(np.float32))
    given = rng.standard_normal((4, 4))
    assert np.array_equal(drift_factor(("factor", given), cov), np.tril(given).astype(np.float32))
    assert not drift_factor(("factor", 0), cov).any() and drift_factor(("factor", np.zeros((4, 4))), cov).shape == (4, 4)
    assert check_drift_uncertainty(None, cov) is None and np.array_equal(check_drift_uncertainty(84, cov), M)
    singular = np.ones((4, 4))
    for bad in (0, -3, float("nan"), float("inf"), True, "84", singular, -cov, cov[:3, :3], ("factor", given[:3]), ("chol", given),
                ("factor", np.full((4, 4), np.inf)), ("factor", np.full((4, 4), 1e39)), [1.0, 2.0]):
        with pytest.raises(ValueError):
            drift_factor(bad, cov)
    with pytest.raises(ValueError, match="positive definite"):
        drift_factor(singular, cov)


def test_drift_cov_is_the_standard_error_of_the_sample_mean():
    rng = np.random.default_rng(5)
    rows = 0.05 * rng.standard_normal((84, 3))
    assert np.allclose(drift_cov(rows), np.cov(rows, rowvar=False, ddof=1) / 84, rtol=0, atol=0)
    assert drift_cov(rows[:, 0]).shape == (1, 1)
    for bad in (rows[:1], np.full((5, 2), np.nan), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            drift_cov(bad)


def test_drift_law_agrees_with_a_binary64_monte_carlo_twin():
    """10^6 draws of a NumPy generator: the mean and the variance of S_T (log) and the mean of V_T (simple) within 5 standard errors."""
    N, T, n = 3, 6, 1_000_000
    mu, L, W = market(N, 1, vol=0.08)
    M = ref_.dense_factor(N, 0.03)
    law = drift_law(mu, L, M, W[0], T, v0=2.0)
    assert law["drift_std"] == math.sqrt(law["b"]) and law["log_mean"] == T * law["c"] and law["log_var"] == T * law["a"] + T * T * law["b"]
    assert law["log_variance_share"] == T * law["b"] / (law["a"] + T * law["b"]) and 0.3 < law["log_variance_share"] < 0.99
    rng = np.random.default_rng(11)
    w, mu64, L64, M64 = W[0].astype(np.float64), mu.astype(np.float64), L.astype(np.float64), M.astype(np.float64)
    drift = (mu64 + rng.standard_normal((n, N)) @ M64.T) @ w
    S, V = np.zeros(n), np.full(n, 2.0)
    for _ in range(T):
        rho = drift + (rng.standard_normal((n, N)) @ L64.T) @ w
        S, V = S + rho, V * (1.0 + rho)
    assert abs(S.mean() - law["log_mean"]) < 5 * math.sqrt(law["log_var"] / n)
    assert abs(S.var() / law["log_var"] - 1) < 5 * math.sqrt(2.0 / n)
    assert abs(V.mean() - law["simple_mean"]) < 5 * V.std() / math.sqrt(n)
    known = drift_law(mu, L, np.zeros((N, N)), W[0], T, v0=2.0)
    assert known["b"] == 0 and known["log_variance_share"] == 0 and abs(known["simple_mean"] - 2.0 * (1 + known["c"]) ** T) < 1e-12
    assert law["simple_mean"] > known["simple_mean"]
    with pytest.raises(ValueError):
        drift_law(mu, L, M, W[0], 0)


# ---- 3. header / binding / library ----------------------------------------------------------------------------------------------

def test_extension_header_binding_and_library_agree(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    assert sorted(protos) == sorted(_ffi.UNCERTAIN_SIGNATURES) == ["mcp_simulate_uncertain"]
    params = [p.strip() for p in protos["mcp_simulate_uncertain"].split(",")]
    assert len(params) == len(_ffi.UNCERTAIN_SIGNATURES["mcp_simulate_uncertain"][1]) == 23
    assert [p.split()[-1].lstrip("*") for p in params[:4]] == ["ctx", "prm", "du", "cf"]
    assert [p.split()[-1].lstrip("*") for p in params[-9:]] == ["terminal_out", "stats_out", "mdd_out", "dd_stats_out", "counts_out", "horizon_out",
                                                                 "hz_stats_out", "bands_out", "hz_counts_out"]
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "mcp_simulate_uncertain") and hasattr(mcp_lib, "mcp_simulate_uncertain")
    for table in (_ffi.SIGNATURES, _ffi.SIMULATE_ENTRIES, _ffi.EXTENSION_SIGNATURES, _ffi.SPEND_SIGNATURES, _ffi.LIFE_SIGNATURES,
                  _ffi.BAND_SIGNATURES, _ffi.VOLTARGET_SIGNATURES, _ffi.UNDERWATER_SIGNATURES):
        assert "mcp_simulate_uncertain" not in table
    assert mcp_lib.mcp_simulate_uncertain.argtypes == _ffi.UNCERTAIN_SIGNATURES["mcp_simulate_uncertain"][1]
    assert _ffi.UNCERTAIN_ENTRIES == {"mcp_simulate_uncertain": ("ctx", "prm", "du", "cf", "mu", "chol", "W", "walk", "hz_in", "out", "dd", "counts",
                                                                 "hz_out", "hz_counts")}
    fields = re.search(r"typedef struct \{(.*?)\} mcp_drift_uncertainty;", text, flags=re.S).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()] == [n for n, _ in _ffi.McpDriftUncertainty._fields_] == ["factor", "reserved"]
    assert ctypes.sizeof(_ffi.McpDriftUncertainty) == 16
    assert '#include "mcport.h"' in text and 'extern "C"' in text and "MCP_ABI_VERSION" not in text
    assert mcp_lib.mcp_abi_version() == _ffi.MCP_ABI_VERSION == 4
    assert "uncertain" not in open(os.path.join(ROOT, "include", "mcport.h")).read()     # the main header is the parent's
    assert not [n for n in protos if n.startswith("mcp_launch")]                         # no enqueue-only entry point takes the factor


# ---- 4. the argument rules through the C ABI, without a device --------------------------------------------------------------------

def _raw(name):
    fn = getattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    fn.restype = ctypes.c_int
    return fn


def _call(prm, du=True, factor="ok", reserved=0, cf=False, mu=True, W=True, stats=True, dd=False, mdd=False, H=0, levels=(), counts=None,
          hz_counts=None, hz_stats=None, bad_flow=False, steps=None):
    """mcp_simulate_uncertain with a NULL context on valid arrays of prm's shape; the keywords break one thing each."""
    N, K, T = prm.n_assets, prm.n_portfolios, prm.n_steps
    mu_a, L, Wm = np.full(N, 1e-3, np.float32), (0.03 * np.eye(N)).astype(np.float32), np.full((K, N), 1.0 / N, np.float32)
    M = np.tril(np.full((N, N), 0.01, np.float32))
    if factor == "inf":
        M[N - 1, 0] = np.inf
    if factor == "nan":
        M[0, 0] = np.nan
    if factor == "upper_nan":
        M[0, N - 1] = np.nan
    if factor == "zero":
        M[:] = 0
    d = _ffi.McpDriftUncertainty(None if factor is None else M.ctypes.data, reserved)
    flows = np.full(T, -0.01, np.float32)
    if bad_flow:
        flows[0] = np.nan
    cfs = _ffi.make_cashflow(flows, 0.5) if cf else None
    lv = np.asarray(levels, np.float64)
    st = np.asarray(steps if steps is not None else [1, T][:H] if H else [], np.int32)
    s, ds, hs = np.zeros(K, _ffi.STATS_DTYPE), np.zeros(K, _ffi.STATS_DTYPE), np.zeros((max(H, 1), K), _ffi.STATS_DTYPE)
    qd, bands = np.zeros((K, 100), np.float32), np.zeros((max(H, 1), K, max(lv.size, 1)), np.float64)
    cn, hcn = np.zeros((K, 2), np.uint64), np.zeros((max(H, 1), K, 2), np.uint64)
    counts = cf if counts is None else counts
    hz_counts = (cf and H > 0) if hz_counts is None else hz_counts
    hz_stats = H > 0 if hz_stats is None else hz_stats
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    return _raw("mcp_simulate_uncertain")(
        None, ctypes.byref(prm), ref(d) if du else None, ref(cfs), vp(mu_a) if mu else None, vp(L), vp(Wm) if W else None,
        ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100), H, vp(st) if H else None, lv.size, vp(lv) if lv.size else None,
        None, vp(s) if stats else None, vp(qd) if mdd else None, vp(ds) if dd else None, vp(cn) if counts else None, None,
        vp(hs) if hz_stats else None, vp(bands) if lv.size else None, vp(hcn) if hz_counts else None)


BAD = [  # (keywords of _call, what the error names)
    ({"du": False}, "drift_uncertainty is NULL"), ({"factor": None}, "factor is NULL"), ({"reserved": 1}, "reserved"),
    ({"factor": "inf"}, "not finite"), ({"factor": "nan"}, "not finite"), ({"factor": "upper_nan"}, "not finite"),
    ({"mu": False}, "NULL pointer"), ({"W": False}, "NULL pointer"), ({"stats": False}, "NULL pointer"), ({"mdd": True}, "mdd_out"),
    ({"H": 2, "steps": [3, 2]}, "horizon"), ({"H": 2, "hz_stats": False}, "hz_stats_out"), ({"H": 2, "levels": (101.0,)}, "level"),
    ({"levels": (50.0,)}, "n_horizons = 0"), ({"cf": True, "bad_flow": True}, "flow"), ({"cf": True, "counts": False}, "counts_out"),
    ({"cf": True, "H": 2, "hz_counts": False}, "hz_counts_out"), ({"cf": True, "hz_counts": True}, "hz_counts_out"),
    ({"counts": True}, "without cash flows"), ({"H": 2, "hz_counts": True}, "without cash flows"),
]
UNSUPPORTED = [  # (keywords of make_params, keywords of _call, what the error names)
    ({"fold": True, "n_portfolios": 1}, {}, "MCP_FLAG_FOLD"), ({"native_math": True}, {}, "MCP_FLAG_NATIVE_MATH"),
    ({"native_math": True}, {"dd": True}, "MCP_FLAG_NATIVE_MATH"), ({}, {"dd": True, "H": 2}, "horizons and the drawdown"),
    ({}, {"dd": True, "cf": True}, "cash flows are not combined with the drawdown"), ({"compounding": "log"}, {"cf": True}, "log compounding"),
    ({"compounding": "log"}, {"cf": True, "H": 2}, "log compounding"),
]


def _prm(n_assets=4, n_steps=10, n_portfolios=2, **kw):
    return _ffi.make_params(n_assets, n_steps, n_portfolios, **kw)


@pytest.mark.parametrize("kw,what", BAD)
def test_bad_requests_return_e_arg_with_a_null_context(kw, what, mcp_lib):
    assert _call(_prm(), **kw) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()


@pytest.mark.parametrize("pkw,kw,what", UNSUPPORTED)
def test_refusals_return_e_unsupported_with_a_null_context(pkw, kw, what, mcp_lib):
    assert _call(_prm(**pkw), **kw) == _ffi.MCP_E_UNSUPPORTED
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()


def test_a_valid_request_gets_as_far_as_the_context(mcp_lib):
    """Every rule is checked before any device is touched: what is left to fail with a NULL context is the context."""
    for pkw, kw in (({}, {}), ({"compounding": "log"}, {}), ({}, {"factor": "zero"}), ({}, {"dd": True}), ({"compounding": "log"}, {"dd": True, "mdd": True}),
                    ({}, {"H": 2, "levels": (5.0, 95.0)}), ({"compounding": "log"}, {"H": 1}), ({}, {"cf": True}), ({}, {"cf": True, "H": 2}),
                    ({"n_portfolios": 20}, {}), ({"n_assets": 64, "n_portfolios": 1}, {"dd": True}), ({"n_assets": 1}, {})):
        assert _call(_prm(**pkw), **kw) == _ffi.MCP_E_ARG, (pkw, kw)
        assert b"ctx is NULL" in mcp_lib.mcp_last_error(), (pkw, kw, mcp_lib.mcp_last_error())


# ---- 5. the Python rules ----------------------------------------------------------------------------------------------------------

N, PATHS = front_end_cases.N, front_end_cases.PATHS
PUBLIC_REFUSED = {
    "underwater": dict(underwater=True, drawdown=True), "vol_target": dict(vol_target=(0.01, 0.7)), "tolerance": dict(tolerance=0.05),
    "spending": dict(spending=(0.02, 2, 0.1, 0.1)), "protect": dict(protect=0.8), "glide": dict(glide=([2], [[0.5, 0.25, 0.25]])),
    "regimes": dict(regimes=(0.05, 0.2, np.full(N, -1e-3), 4e-4 * np.eye(N))), "jumps": dict(jumps=(0.1, -0.01, 0.01)),
    "garch": dict(garch=(0.05, 0.9)), "dof": dict(dof=5), "rebalance": dict(rebalance=2),
    "overlay": dict(overlay={0: [("Long Put", 90.0, 1.0, 1.0)]}, spot=[100.0] * 3), "attribution": dict(attribution=True),
    "antithetic": dict(antithetic=True), "lifetime": dict(lifetime=True, cashflow=-0.01), "fold": dict(fold=True), "native_math": dict(native_math=True),
}


def test_entry_tables_and_the_front_end_over_the_recorder(mcp_lib):
    assert simulate._UNCERTAIN_CHOICE[0] == "mcp_simulate_uncertain" and simulate._KEYWORD_GROUP["drift_uncertainty"] == "du"
    groups = _ffi.UNCERTAIN_ENTRIES["mcp_simulate_uncertain"]
    for kw in ("rows", "period", "overlay", "attribution", "antithetic", "filtered", "regimes", "glide", "protect", "spending", "lifetime",
               "tolerance", "vol_target", "underwater", "dof", "garch", "jumps"):
        assert simulate._KEYWORD_GROUP[kw] not in groups, kw
    for kw in ("drawdown", "horizons", "flows", "drift_uncertainty"):
        assert simulate._KEYWORD_GROUP[kw] in groups, kw
    assert simulate._ENTRY_CHOICE[0][1] == "mcp_simulate_spending"           # the parent's table is untouched
    f32 = np.float32
    mu32, chol, W = np.full(N, 1e-3, f32), (0.01 * np.eye(N)).astype(f32), np.full((1, N), 1 / N, f32)
    M = np.tril(np.full((N, N), 0.002, f32))
    stats = f"ptr {_ffi.STATS_DTYPE.name}[1]"
    with front_end_cases.recording(mcp_lib) as (rec, ctx):
        prm = _ffi.make_params(N, 5, 1)
        (entry, kinds), = front_end_cases.record(rec, lambda: ctx.simulate_uncertain(prm, M, mu32, chol, W, 7, 0, PATHS, True))["calls"]
        assert entry == "mcp_simulate_uncertain" and len(kinds) == 23 and kinds[2:4] == ["McpDriftUncertainty", "NULL"]
        assert kinds[10:] == [0, "NULL", 0, "NULL", "ptr float32[1, 8]", stats, "NULL", "NULL", "NULL", "NULL", "NULL", "NULL", "NULL"]
        (entry, kinds), = front_end_cases.record(rec, lambda: ctx.simulate_uncertain(prm, M, mu32, chol, W, 7, 0, PATHS, False, drawdown=True))["calls"]
        assert kinds[14:18] == ["NULL", stats, "NULL", stats] and kinds[18] == "NULL"
        (entry, kinds), = front_end_cases.record(rec, lambda: ctx.simulate_uncertain(prm, M, mu32, chol, W, 7, 0, PATHS, True, horizons=np.array([2, 5], np.int32),
                                                                                     levels=(5.0,), flows=np.zeros(5, f32), target=0.5))["calls"]
        assert kinds[3] == "McpCashflow" and kinds[10:14] == [2, "ptr int32[2]", 1, "ptr float64[1]"]
        assert kinds[18:] == ["ptr uint64[1, 2]", "ptr float32[2, 1, 8]", f"ptr {_ffi.STATS_DTYPE.name}[2, 1]", "ptr float64[2, 1, 1]", "ptr uint64[2, 1, 2]"]
        for name, kw in (("rows", dict(rows=np.full((6, N), 1e-3, f32))), ("period", dict(period=2)), ("dof", dict(dof=5)), ("garch", dict(garch=(0.1, 0.8, 1.0))),
                         ("regimes", dict(regimes=(0.05, 0.2, 0.1, mu32.copy(), chol.copy()))), ("attribution", dict(attribution=True)),
                         ("antithetic", dict(antithetic=True)), ("protect", dict(protect=(np.zeros(6, f32), 3.0, 0.0, 1.0, 0.0))),
                         ("vol_target", dict(vol_target=(0.05, 0.7, 1.2, 0.0, 0.0, None))), ("underwater", dict(underwater=np.array([50.0]), drawdown=True))):
            got = front_end_cases.record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, True, mu=mu32, chol=chol, drift_uncertainty=M, **kw))
            assert got.get("raises") == ["ValueError", simulate._UNCERTAIN_CHOICE[1]], (name, got)
        mu, cov, w = np.full(N, 1e-3), 1e-4 * np.eye(N), np.full(N, 1 / N)
        paths = lambda **kw: simulate_paths(mu, cov, w, n_steps=6, n_paths=PATHS, **kw)   # noqa: E731
        for spec in (84, cov / 84, ("factor", M), ("factor", 0)):
            got = front_end_cases.record(rec, lambda: paths(drift_uncertainty=spec, store=True))
            (entry, kinds), = got["calls"]
            assert entry == "mcp_simulate_uncertain" and "drift_uncertainty" in got["keys"] and "terminal" in got["keys"]
        res = paths(drift_uncertainty=84, horizons=[1, 3, 6], bands=(5, 95), cashflow=-0.01, target=0.5)
        assert sorted(res["drift_uncertainty"]) == ["drift_std", "horizon_log_variance_share", "log_variance_share"] and "cashflow" in res
        law = drift_law(mu, np.linalg.cholesky(cov), drift_factor(84, cov), w, 6)
        assert res["drift_uncertainty"]["drift_std"] == law["drift_std"] and abs(res["drift_uncertainty"]["log_variance_share"] - 6 / 90) < 1e-6
        assert res["drift_uncertainty"]["horizon_log_variance_share"].shape == (3,)
        assert sorted(paths(drift_uncertainty=84, drawdown=True, compounding="log")["drift_uncertainty"]) == ["drift_std", "log_variance_share"]
        two = simulate_paths(mu, cov, np.array([w, w]), n_steps=6, n_paths=PATHS, drift_uncertainty=84)
        assert len(two) == 2 and all("drift_uncertainty" in d for d in two)
        assert len(paths(drift_uncertainty=84, as_array=True, store=True)) == 2 and len(paths(drift_uncertainty=84, drawdown=True, as_array=True)) == 2
        assert len(paths(drift_uncertainty=84, cashflow=-0.01, horizons=[2, 6], as_array=True)) == 5
        got = front_end_cases.record(rec, lambda: paths(drift_uncertainty=84, chol=np.linalg.cholesky(cov)))
        assert got["calls"][0][0] == "mcp_simulate_uncertain"
        for name, kw in PUBLIC_REFUSED.items():
            got = front_end_cases.record(rec, lambda: paths(drift_uncertainty=84, **kw))
            assert got.get("raises", [None])[0] == "ValueError", (name, got)
            assert got["raises"][1].startswith(simulate._PATHS_COMBINE["drift_uncertainty"][0] + ": not with ") and name in got["raises"][1], (name, got)
        for bad in (dict(drift_uncertainty=0), dict(drift_uncertainty=-cov), dict(drift_uncertainty="84"), dict(drift_uncertainty=("factor", np.eye(2))),
                    dict(drift_uncertainty=84, spot=[1.0] * 3), dict(drift_uncertainty=84, bands=(5.0,)), dict(drift_uncertainty=84, drawdown=True, horizons=[2]),
                    dict(drift_uncertainty=84, drawdown=True, cashflow=-0.01), dict(drift_uncertainty=84, cashflow=-0.01, compounding="log"),
                    dict(drift_uncertainty=84, target=0.5)):
            assert front_end_cases.record(rec, lambda: paths(**bad)).get("raises", [None])[0] == "ValueError", bad
        with pytest.raises(ValueError, match="simulate_sweep does not take drift_uncertainty"):
            simulate_sweep(mu, cov, weights=np.array([[0.5, 0.25, 0.25], [0.2, 0.3, 0.5]]), n_steps=6, n_paths=PATHS, drift_uncertainty=84)
    from monte_carlo_portfolio_amd import engine
    import inspect
    assert "uncertain" not in inspect.getsource(engine)


# ---- 6. the rows -------------------------------------------------------------------------------------------------------------------

SEVEN = [("FAM_PLAIN", "PK_PU", "mc_paths_pu_kernel<NB, KT, 1, false>"), ("FAM_PLAIN", "PK_PU | PK_LOGC", "mc_paths_pu_kernel<NB, KT, 1, true>"),
         ("FAM_DD", "PK_PU", "mc_paths_pu_dd_kernel<NB, KT, 1, false>"), ("FAM_DD", "PK_PU | PK_LOGC", "mc_paths_pu_dd_kernel<NB, KT, 1, true>"),
         ("FAM_HZ", "PK_PU", "mc_paths_pu_hz_kernel<NB, KT, 1, false>"), ("FAM_HZ", "PK_PU | PK_LOGC", "mc_paths_pu_hz_kernel<NB, KT, 1, true>"),
         ("FAM_CF", "PK_PU", "mc_paths_pu_cf_kernel<NB, KT, 1>")]


def test_the_ladder_has_the_seven_rows_and_the_selftest_names_them():
    """The selector of every accepted request with uncertainty names one of the seven rows, and none of them is the lean kernel's: the
    host selftest (tests/test_host_unit_cpu.py runs it) enumerates the requests, proves one row each and that every row is reached, and
    names the seven routes literally; here, that the ladder and the selftest say what this test file says."""
    ladder = open(os.path.join(CSRC, "mcp_paths_ladder.inc")).read()
    rows = re.findall(r"^MCP_ROW(?:_IF)?\((.*)\)$", ladder, flags=re.M)
    pu = [r for r in rows if "PK_PU" in r]
    assert pu == [f"{fam}, {mask}, {kernel}" for fam, mask, kernel in SEVEN]             # every NB, KT = 1 and 8: no condition
    assert not [r for r in rows if "PK_PU" in r and "PK_UHI" in r]
    route = open(os.path.join(CSRC, "mcp_route.h")).read()
    assert "PK_PU = 1u << 21" in route and "N_PATH_FLAGS_PU = N_PATH_FLAGS + 1;" in route and "N_PATH_FLAGS = 21;" in route
    selftest = open(os.path.join(CSRC, "host_selftest.cpp")).read()
    for _, _, kernel in SEVEN:
        assert f'"{kernel}"' in selftest, kernel
    assert "B_PU = 1 << N_BITS, N_BITS_PU = N_BITS + 1" in selftest and "b < N_PATH_FLAGS_PU" in selftest and "1 << N_BITS_PU" in selftest and "93u : 91u" in selftest and "85u" in selftest
    assert "(k.flags & mcp::PK_PU) && !(k.flags & mcp::PK_UHI)" in selftest
    host = open(os.path.join(CSRC, "mcp_host.cpp")).read()
    assert "if (rq.uncertain) k.flags |= PK_PU;" in host
    body = open(os.path.join(CSRC, "mcp_paths_body.inc")).read()
    m = re.search(r"static_assert\(!PU \|\| !\(([^)]*)\)", body)
    assert m and sorted(m.group(1).split(" || ")) == sorted("NATIVE FOLD UHI BOOT REB STT GV OV AT ANTI FH JP RS GP PI SP LT TB VT UW".split())

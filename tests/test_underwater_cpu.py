"""CPU checks of the time under water (SPEC.md 4.20 / 5.20): the extension header against _ffi.UNDERWATER_SIGNATURES and the exported
symbol; every argument rule and refusal of mcp_simulate_underwater through the C ABI with no device, and of
simulate_paths(underwater=True) with no context; the restatement (underwater_ref.py) against a plain per-path loop; the exact
properties (b), (c) and (e) and the coverage of the GPU test's inputs on the restatement; the two distribution-free laws on the
restatement at 10^6 paths; the rows the host selftest proves."""
import ctypes
import os
import re

import numpy as np
import pytest

import front_end_cases
import underwater_ref as ref_
from monte_carlo_portfolio_amd import _ffi, simulate, simulate_paths, simulate_sweep, spell_law
from monte_carlo_portfolio_amd.underwater import check_underwater

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcport_underwater.h")
CSRC = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
SEED, DRAWS, ROWS, CASES, market, pick = ref_.SEED, ref_.DRAWS, ref_.ROWS, ref_.CASES, ref_.market, ref_.pick


def _raw(name):
    fn = getattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    fn.restype = ctypes.c_int
    return fn


# ---- 1. header / binding / library ----------------------------------------------------------------------------------------------

def test_extension_header_binding_and_library_agree(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    assert sorted(protos) == sorted(_ffi.UNDERWATER_SIGNATURES) == ["mcp_simulate_underwater"]
    params = [p.strip() for p in protos["mcp_simulate_underwater"].split(",")]
    assert len(params) == len(_ffi.UNDERWATER_SIGNATURES["mcp_simulate_underwater"][1]) == 23
    assert [p.split()[-1].lstrip("*") for p in params[-8:]] == ["longest_out", "current_out", "longest_hist_out", "current_hist_out", "sums_out",
                                                                 "n_uw_levels", "uw_levels", "q_out"]
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "mcp_simulate_underwater") and hasattr(mcp_lib, "mcp_simulate_underwater")
    for table in (_ffi.SIGNATURES, _ffi.SIMULATE_ENTRIES, _ffi.EXTENSION_SIGNATURES, _ffi.SPEND_SIGNATURES, _ffi.LIFE_SIGNATURES,
                  _ffi.BAND_SIGNATURES, _ffi.VOLTARGET_SIGNATURES):
        assert "mcp_simulate_underwater" not in table
    assert mcp_lib.mcp_simulate_underwater.argtypes == _ffi.UNDERWATER_SIGNATURES["mcp_simulate_underwater"][1]
    assert _ffi.UNDERWATER_ENTRIES == {"mcp_simulate_underwater": ("ctx", "prm", "gv", "st", "jp", "mu", "chol", "W", "walk", "out", "dd", "uw")}
    assert '#include "mcport.h"' in text and 'extern "C"' in text and "MCP_ABI_VERSION" not in text and "typedef" not in text
    assert mcp_lib.mcp_abi_version() == _ffi.MCP_ABI_VERSION == 4
    assert "underwater" not in open(os.path.join(ROOT, "include", "mcport.h")).read()   # the main header is the parent's
    assert not [n for n in protos if n.startswith("mcp_launch")]                         # no enqueue-only entry point takes the counters


# ---- 2. the argument rules through the C ABI, without a device --------------------------------------------------------------------

def _call(prm, gv=None, st=None, jp=None, mu=True, W=True, stats=True, dd=True, mdd=False, lh=True, ch=True, sums=True, levels=(50.0, 95.0),
          q=None, store=False):
    """mcp_simulate_underwater with a NULL context on valid arrays of prm's shape; the keywords break one thing each."""
    N, K, T = prm.n_assets, prm.n_portfolios, min(prm.n_steps, 64)
    mu_a, L, Wm = np.full(N, 1e-3, np.float32), (0.03 * np.eye(N)).astype(np.float32), np.full((K, N), 1.0 / N, np.float32)
    lv = np.asarray(levels, np.float64)
    s, d = np.zeros(K, _ffi.STATS_DTYPE), np.zeros(K, _ffi.STATS_DTYPE)
    qd, m, c = np.zeros((K, 100), np.float32), np.zeros((K, 100), np.uint32), np.zeros((K, 100), np.uint32)
    hm, hc, sm = np.zeros((K, T + 1), np.uint64), np.zeros((K, T + 1), np.uint64), np.zeros((K, 2), np.uint64)
    qo = np.zeros((K, 2, max(lv.size, 1)), np.uint32)
    if q is None:
        q = lv.size > 0
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    return _raw("mcp_simulate_underwater")(
        None, ctypes.byref(prm), ref(gv), ref(st), ref(jp), vp(mu_a) if mu else None, vp(L), vp(Wm) if W else None,
        ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100), None, vp(s) if stats else None, vp(qd) if mdd else None,
        vp(d) if dd else None, vp(m) if store else None, vp(c) if store else None, vp(hm) if lh else None, vp(hc) if ch else None,
        vp(sm) if sums else None, lv.size, vp(lv) if lv.size else None, vp(qo) if q else None)


GV, ST, JP = _ffi.McpGarch(0.1, 0.8, 1.0, 0), _ffi.McpStudentT(5, 0), _ffi.McpJumps(0.2, -0.05, 0.04, None, 0)
BAD = [  # (keywords of _call, what the error names)
    ({"dd": False}, "dd_stats_out"), ({"dd": False, "mdd": True}, "dd_stats_out"), ({"lh": False}, "longest_hist_out"),
    ({"ch": False}, "current_hist_out"), ({"sums": False}, "sums_out"),
    ({"levels": (50.0, 101.0)}, "level"), ({"levels": (-1.0,)}, "level"), ({"levels": (float("nan"),)}, "level"),
    ({"levels": tuple(range(17))}, "level"), ({"q": False}, "q_out"), ({"levels": (), "q": True}, "q_out"),
    ({"mu": False}, "NULL pointer"), ({"W": False}, "NULL pointer"), ({"stats": False}, "NULL pointer"),
    ({"gv": _ffi.McpGarch(0.5, 0.6, 1.0, 0)}, "alpha + beta"), ({"st": _ffi.McpStudentT(2, 0)}, "dof"),
    ({"jp": _ffi.McpJumps(2.0, -0.1, 0.1, None, 0)}, "intensity"),
]
UNSUPPORTED = [  # (keywords of make_params, keywords of _call, what the error names)
    ({"n_steps": _ffi.MCP_MAX_LIFE_STEPS + 1}, {}, "MCP_MAX_LIFE_STEPS"), ({"fold": True, "n_portfolios": 1}, {}, "MCP_FLAG_FOLD"),
    ({"native_math": True}, {}, "MCP_FLAG_NATIVE_MATH"), ({"compounding": "log"}, {"gv": GV}, "log compounding"),
    ({"compounding": "log"}, {"st": ST}, "log compounding"), ({"compounding": "log"}, {"jp": JP}, "log compounding"),
    ({}, {"jp": JP, "gv": GV}, "jumps are not combined"), ({}, {"jp": JP, "st": ST}, "jumps are not combined"),
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
    for pkw, kw in (({}, {}), ({"compounding": "log"}, {}), ({}, {"gv": GV}), ({}, {"st": ST}), ({}, {"gv": GV, "st": ST}), ({}, {"jp": JP}),
                    ({}, {"levels": ()}), ({}, {"store": True, "mdd": True}), ({"n_portfolios": 20}, {}),
                    ({"n_steps": _ffi.MCP_MAX_LIFE_STEPS}, {})):
        assert _call(_prm(**pkw), **kw) == _ffi.MCP_E_ARG, (pkw, kw)
        assert b"ctx is NULL" in mcp_lib.mcp_last_error(), (pkw, kw, mcp_lib.mcp_last_error())


# ---- 3. the Python rules ----------------------------------------------------------------------------------------------------------

N, PATHS = front_end_cases.N, front_end_cases.PATHS
PUBLIC_REFUSED = {
    "vol_target": dict(vol_target=(0.01, 0.7)), "tolerance": dict(tolerance=0.05), "spending": dict(spending=(0.02, 2, 0.1, 0.1)),
    "protect": dict(protect=0.8), "glide": dict(glide=([2], [[0.5, 0.25, 0.25]])),
    "regimes": dict(regimes=(0.05, 0.2, np.full(N, -1e-3), 4e-4 * np.eye(N))), "rebalance": dict(rebalance=2), "cashflow": dict(cashflow=0.01),
    "overlay": dict(overlay={0: [("Long Put", 90.0, 1.0, 1.0)]}, spot=[100.0] * 3), "attribution": dict(attribution=True),
    "antithetic": dict(antithetic=True), "lifetime": dict(lifetime=True), "horizons": dict(horizons=[2, 6]), "fold": dict(fold=True),
    "native_math": dict(native_math=True),
}


def test_check_underwater_and_spell_law():
    assert np.array_equal(check_underwater((50, 95), 10), [50.0, 95.0]) and check_underwater((), 10).size == 0
    for bad in ((101,), (-1,), (float("nan"),), "ab", tuple(range(17))):
        with pytest.raises(ValueError, match="underwater_levels"):
            check_underwater(bad, 10)
    with pytest.raises(ValueError, match="n_steps"):
        check_underwater((50,), _ffi.MCP_MAX_LIFE_STEPS + 1)
    assert spell_law(1) == (1.0, 1.0) and spell_law(2) == (0.5, 0.5) and spell_law(5) == (0.0625, 70 / 256)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            spell_law(bad)


def test_entry_tables_and_the_front_end_over_the_recorder(mcp_lib):
    assert simulate._UNDERWATER_CHOICE[0] == "mcp_simulate_underwater" and simulate._KEYWORD_GROUP["underwater"] == "uw"
    groups = _ffi.UNDERWATER_ENTRIES["mcp_simulate_underwater"]
    for kw in ("rows", "period", "flows", "overlay", "attribution", "antithetic", "filtered", "regimes", "glide", "protect", "spending", "lifetime",
               "tolerance", "vol_target", "horizons"):
        assert simulate._KEYWORD_GROUP[kw] not in groups, kw
    for kw in ("dof", "garch", "jumps", "drawdown", "underwater"):
        assert simulate._KEYWORD_GROUP[kw] in groups, kw
    assert simulate._ENTRY_CHOICE[0][1] == "mcp_simulate_spending"           # the parent's table is untouched
    f32 = np.float32
    mu32, chol, W = np.full(N, 1e-3, f32), (0.01 * np.eye(N)).astype(f32), np.full((1, N), 1 / N, f32)
    uw = dict(underwater=np.array([50.0, 95.0]))
    stats = f"ptr {_ffi.STATS_DTYPE.name}[1]"
    with front_end_cases.recording(mcp_lib) as (rec, ctx):
        prm = _ffi.make_params(N, 5, 1)
        for store in (True, False):
            (entry, kinds), = front_end_cases.record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, store, mu=mu32, chol=chol, drawdown=True, **uw))["calls"]
            per_path = "ptr uint32[1, 8]" if store else "NULL"
            assert entry == "mcp_simulate_underwater" and len(kinds) == 23 and kinds[2:5] == ["NULL"] * 3
            assert kinds[11:15] == ["ptr float32[1, 8]" if store else "NULL", stats] * 2
            assert kinds[15:] == [per_path, per_path, "ptr uint64[1, 6]", "ptr uint64[1, 6]", "ptr uint64[1, 2]", 2, "ptr float64[2]",
                                  "ptr uint32[1, 2, 2]"]
        (entry, kinds), = front_end_cases.record(rec, lambda: ctx.simulate_underwater(prm, mu32, chol, W, 7, 0, PATHS, False, levels=(), dof=5,
                                                                                      garch=(0.1, 0.8, 1.0)))["calls"]
        assert kinds[2:5] == ["McpGarch", "McpStudentT", "NULL"] and kinds[20:] == [0, "NULL", "NULL"]
        got = front_end_cases.record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, True, mu=mu32, chol=chol, **uw))
        assert got.get("raises") == ["ValueError", "underwater needs drawdown"]
        for name, kw in (("rows", dict(rows=np.full((6, N), 1e-3, f32))), ("period", dict(period=2)), ("flows", dict(flows=np.zeros(5, f32))),
                         ("regimes", dict(regimes=(0.05, 0.2, 0.1, mu32.copy(), chol.copy()))), ("attribution", dict(attribution=True)),
                         ("antithetic", dict(antithetic=True)), ("protect", dict(protect=(np.zeros(6, f32), 3.0, 0.0, 1.0, 0.0))),
                         ("horizons", dict(horizons=np.array([2, 5], np.int32))), ("vol_target", dict(vol_target=(0.05, 0.7, 1.2, 0.0, 0.0, None)))):
            got = front_end_cases.record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, True, mu=mu32, chol=chol, drawdown=True, **uw, **kw))
            assert got.get("raises") == ["ValueError", simulate._UNDERWATER_CHOICE[1]], (name, got)
        mu, cov, w = np.full(N, 1e-3), 1e-4 * np.eye(N), np.full(N, 1 / N)
        paths = lambda **kw: simulate_paths(mu, cov, w, n_steps=6, n_paths=PATHS, **kw)   # noqa: E731
        got = front_end_cases.record(rec, lambda: paths(drawdown=True, underwater=True, store=True))
        (entry, kinds), = got["calls"]
        assert entry == "mcp_simulate_underwater" and "underwater" in got["keys"] and "drawdown" in got["keys"] and kinds[20] == 2
        res = paths(drawdown=True, underwater=True, underwater_levels=(5, 50, 95), store=True, jumps=(0.1, -0.01, 0.01))
        blk = res["underwater"]
        assert sorted(blk) == ["current", "longest", "p_under_water_at_end"] and "jumps" in res and "max_drawdown" in res
        for name in ("longest", "current"):
            assert sorted(blk[name]) == ["hist", "levels", "mean", "steps"] and blk[name]["hist"].shape == (7,) and blk[name]["hist"].dtype == np.uint64
            assert sorted(blk[name]["levels"]) == [5.0, 50.0, 95.0] and blk[name]["steps"].shape == (PATHS,) and blk[name]["steps"].dtype == np.uint32
        assert "steps" not in paths(drawdown=True, underwater=True)["underwater"]["longest"]
        two = simulate_paths(mu, cov, np.array([w, w]), n_steps=6, n_paths=PATHS, drawdown=True, underwater=True, compounding="log")
        assert len(two) == 2 and all("underwater" in d for d in two)
        assert len(paths(drawdown=True, underwater=True, as_array=True)) == 6 and len(paths(drawdown=True, underwater=True, as_array=True, store=True)) == 10
        got = front_end_cases.record(rec, lambda: paths(underwater=True))
        assert got.get("raises", [None])[0] == "ValueError" and "needs drawdown=True" in got["raises"][1]
        for name, kw in PUBLIC_REFUSED.items():
            got = front_end_cases.record(rec, lambda: paths(drawdown=True, underwater=True, **kw))
            assert got.get("raises", [None])[0] == "ValueError" and got["raises"][1] == simulate._PATHS_COMBINE["underwater"][0] + ": not with " + name, (name, got)
        for bad in (dict(jumps=(0.1, -0.01, 0.01), dof=5), dict(jumps=(0.1, -0.01, 0.01), garch=(0.05, 0.9)), dict(dof=5, compounding="log"),
                    dict(garch=(0.05, 0.9), compounding="log"), dict(jumps=(0.1, -0.01, 0.01), compounding="log"), dict(spot=[1.0] * 3),
                    dict(target=0.9), dict(bands=(5.0,)), dict(underwater_levels=(101,)), dict(underwater="yes")):
            kw = dict(dict(underwater=True), **bad)
            assert front_end_cases.record(rec, lambda: paths(drawdown=True, **kw)).get("raises", [None])[0] == "ValueError", bad
        with pytest.raises(ValueError, match="simulate_sweep does not take underwater"):
            simulate_sweep(mu, cov, weights=np.array([[0.5, 0.25, 0.25], [0.2, 0.3, 0.5]]), n_steps=6, n_paths=PATHS, drawdown=True, underwater=True)
    from monte_carlo_portfolio_amd import engine
    import inspect
    assert "underwater" not in inspect.getsource(engine)


# ---- 4. the restatement -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("draw,compounding", ROWS)
def test_restatement_equals_a_plain_loop_on_200_paths(draw, compounding):
    mu, L, W = market(3, 3)
    T = 12
    rho = ref_.rho_of(mu, L, W, T, SEED, np.arange(9, 209, dtype=np.uint64), **DRAWS[draw])
    got = ref_.walk(rho, compounding)
    for k in range(3):
        for p in range(200):
            x, q, m, c = ref_.loop_one_path(rho[k, :, p], compounding)
            assert np.float32(x).view(np.uint32) == got["V_T"][k, p].view(np.uint32) and np.float32(q).view(np.uint32) == got["q"][k, p].view(np.uint32)
            assert (m, c) == (int(got["m"][k, p]), int(got["c"][k, p])), (k, p)
    ref_.covers(got, T)


@pytest.mark.parametrize("draw,compounding", ROWS)
@pytest.mark.parametrize("N,K,T,begin,n", CASES)
def test_properties_b_c_and_the_coverage_of_the_gpu_tests_inputs(N, K, T, begin, n, draw, compounding):
    """The inputs of tests/test_gpu_underwater.py on the restatement alone: spells of every length 0 .. T - 1, paths that end at their
    peak and paths that end under water (covers), and the exact properties (b) and (c)."""
    mu, L, W = market(N, K)
    ids = np.arange(n) if n <= 1037 else pick(n, begin)
    ref = ref_.simulate(mu, L, W, T, SEED, (begin + ids).astype(np.uint64), compounding, **DRAWS[draw])
    print(ref_.covers(ref, T))
    ref_.properties(ref, T, compounding)
    if T == 1:
        assert not ref["m"].any() and not ref["c"].any()
    if compounding == "simple":
        assert np.all(ref["V_T"] > 0)


@pytest.mark.parametrize("draw,compounding", ROWS[:4])
def test_property_e_the_deterministic_anchors_on_the_restatement(draw, compounding):
    """chol = 0: every step moves every portfolio by its drift.  All mu_i > 0: every step is a new peak, m = c_T = 0; all mu_i < 0 (and 1 +
    mu_i > 0): the peak is X_1 and every later step is below it, m = c_T = T - 1."""
    T, N, K = 12, 5, 3
    _, _, W = market(N, K)
    L = np.zeros((N, N), np.float32)
    for sign, want in ((1.0, 0), (-1.0, T - 1)):
        mu = (sign * np.linspace(0.01, 0.05, N)).astype(np.float32)
        ref = ref_.simulate(mu, L, W, T, SEED, np.arange(64, dtype=np.uint64), compounding, **DRAWS[draw])
        assert np.all(ref["m"] == want) and np.all(ref["c"] == want), (sign, draw)


def test_a_return_to_the_peak_ends_a_spell_and_a_nan_is_never_under_water():
    f = np.float32
    rho = np.array([0.5, -0.5, 1.0, -0.25, -0.25, 0.0, 1.0, -0.5], f).reshape(1, 8, 1)   # V: 1.5 .75 1.5 1.125 .84 .84 1.69 .84
    out = ref_.walk(rho)
    assert out["under"][0, :, 0].tolist() == [False, True, False, True, True, True, False, True]      # step 3 returns to the peak exactly
    assert int(out["m"][0, 0]) == 3 and int(out["c"][0, 0]) == 1
    nan = np.array([0.1, -0.2, np.nan, 0.1], f).reshape(1, 4, 1)
    out = ref_.walk(nan)
    assert out["under"][0, :, 0].tolist() == [False, True, False, False] and int(out["m"][0, 0]) == 1 and int(out["c"][0, 0]) == 0


# ---- 5. the two laws on the restatement -------------------------------------------------------------------------------------------

def test_the_two_laws_hold_for_the_restatement_at_a_million_paths():
    """One asset, mu = 0, log compounding, T = 5: S_t is a symmetric random walk with continuous steps, so P(m = 0) = 2^-4 and P(c_T = 0)
    = 70 / 256 whatever the step's law (underwater.spell_law); each count within 5 binomial standard deviations."""
    T, n = 5, 1_000_000
    mu, L, W = np.zeros(1, np.float32), np.full((1, 1), 0.05, np.float32), np.ones((1, 1), np.float32)
    ref = ref_.simulate(mu, L, W, T, SEED, np.arange(n, dtype=np.uint64), "log")
    hm, hc = np.bincount(ref["m"][0], minlength=T + 1), np.bincount(ref["c"][0], minlength=T + 1)
    assert hm[T] == 0 and hc[T] == 0
    print(ref_.law_checks(hm, hc, T))


# ---- 6. the rows the host selftest proves -----------------------------------------------------------------------------------------

def test_the_ladder_has_the_four_rows_and_the_selftest_names_them():
    """tests/test_host_unit_cpu.py runs the selftest, which proves that every accepted request has exactly one row and that every row is
    reached; here: the rows it reads are the four of SPEC.md 4.20, and it asks for each of them by name."""
    route = open(os.path.join(CSRC, "mcp_route.h")).read()
    assert re.search(r"PK_UW = 1u << 20\b", route) and "constexpr int N_PATH_FLAGS = 21;" in route
    rows = re.findall(r"^MCP_ROW\((FAM_\w+), ([^,]*PK_UW[^,]*), (mc_paths_\w+)<([^>]*)>\)", open(os.path.join(CSRC, "mcp_paths_ladder.inc")).read(), re.M)
    assert rows == [("FAM_DD", "PK_UW", "mc_paths_uw_kernel", "NB, KT, 1, false"), ("FAM_DD", "PK_UW | PK_LOGC", "mc_paths_uw_kernel", "NB, KT, 1, true"),
                    ("FAM_DD", "PK_UW | PK_GV", "mc_paths_g_uw_kernel", "NB, KT, 1"), ("FAM_DD", "PK_UW | PK_JP", "mc_paths_j_uw_kernel", "NB, KT, 1")]
    selftest = open(os.path.join(CSRC, "host_selftest.cpp")).read()
    for _, _, kernel, args in rows:
        assert f'"{kernel}<{args}>"' in selftest, kernel
    assert "B_UW = 65536, N_BITS = 17" in selftest and '{"underwater", SRC_GAUSS, B_DD | B_UW}' in selftest

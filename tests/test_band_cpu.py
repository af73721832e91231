"""CPU checks of tolerance-band rebalancing (SPEC.md 4.18 / 5.18): the extension header against _ffi.BAND_SIGNATURES and the exported
symbols, and its C99 compile; every argument rule of mcp_simulate_banded through the C ABI with no device; mcp_band_reviews against the
formula; the exact properties (a), (b), (c) and (e) on the restatement itself (band_ref.py) against rebalance_ref.rebalanced; the
restatement against a binary64 dollar-holdings twin; tolerance_bands and band_law; the front end's routing and refusals."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import band_ref
import front_end_cases
from monte_carlo_portfolio_amd import _ffi, band_law, simulate, simulate_bootstrap, simulate_paths, synthetic, tolerance_bands
from monte_carlo_portfolio_amd.simulate import prepare_inputs
from monte_carlo_portfolio_amd.tolerance import check_tolerance, n_reviews
from rebalance_ref import gauss_returns, rebalanced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcport_band.h")
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None   # noqa: E731
SEED = 0xBA2D
_bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)   # noqa: E731


def _raw(name):
    fn = getattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    fn.restype = ctypes.c_int
    return fn


# ---- 1. header / binding / library ----------------------------------------------------------------------------------------------

def test_extension_header_binding_and_library_agree(mcp_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    assert sorted(protos) == sorted(_ffi.BAND_SIGNATURES) == ["mcp_band_reviews", "mcp_simulate_banded"]
    for name, params in protos.items():
        assert len(params.split(",")) == len(_ffi.BAND_SIGNATURES[name][1]), name
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name) and hasattr(mcp_lib, name)
        for table in (_ffi.SIGNATURES, _ffi.SIMULATE_ENTRIES, _ffi.EXTENSION_SIGNATURES, _ffi.SPEND_SIGNATURES, _ffi.LIFE_SIGNATURES):
            assert name not in table
    assert getattr(mcp_lib, "mcp_simulate_banded").argtypes == _ffi.BAND_SIGNATURES["mcp_simulate_banded"][1]
    assert len(_ffi.BAND_SIGNATURES["mcp_simulate_banded"][1]) == 27
    # the argument list of mcp_simulate_rebalanced with the band in the rule's place, then the eight trade outputs
    rb = _ffi.SIMULATE_ENTRIES["mcp_simulate_rebalanced"]
    assert _ffi.BAND_ENTRIES == {"mcp_simulate_banded": tuple("tb" if g == "rb" else g for g in rb) + ("trades",)}
    assert ctypes.sizeof(_ffi.McpBand) == 24
    assert '#include "mcport.h"' in text and 'extern "C"' in text and "MCP_ABI_VERSION" not in text
    assert mcp_lib.mcp_abi_version() == _ffi.MCP_ABI_VERSION == 4
    for other in ("mcport.h", "mcport_protect.h", "mcport_spend.h", "mcport_life.h"):     # the other headers are the parent's
        assert "mcp_band" not in open(os.path.join(ROOT, "include", other)).read()
    assert len([n for n in _ffi.SIGNATURES if n.startswith("mcp_simulate")]) == len(_ffi.SIMULATE_ENTRIES) == 16


def test_c99_compile_and_link_of_the_new_prototypes(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "tb.c"
    src.write_text(r'''
        #include <stdio.h>
        #include "mcport_band.h"
        int main(void) {
            mcp_params p = {0};
            float mu[2] = {0.001f, 0.002f}, chol[4] = {0.01f, 0.0f, 0.0f, 0.01f}, w[2] = {0.5f, 0.5f}, tol[2] = {0.05f, 0.05f};
            mcp_band bd = {3, 0, 0.001, 0};
            mcp_stats st, ts;
            uint64_t hist[4], sum;
            p.n_assets = 2; p.n_steps = 10; p.n_portfolios = 1; p.compounding = MCP_COMPOUND_SIMPLE; p.v0 = 1.0; p.alpha = 0.95;
            bd.tol = tol;
            if (sizeof(mcp_band) != 24) return 1;
            if (mcp_band_reviews(&p, &bd) != 3) return 2;
            if (mcp_simulate_banded(NULL, &p, &bd, mu, chol, NULL, w, 1, 0, 100, 0, NULL, 0, NULL, NULL, &st, NULL, NULL, NULL, NULL, hist, &sum,
                                    0, NULL, NULL, NULL, &ts) != MCP_E_ARG) return 3;
            printf("%s\n", mcp_last_error());
            bd.tol = NULL;
            if (mcp_simulate_banded(NULL, &p, &bd, mu, chol, NULL, w, 1, 0, 100, 0, NULL, 0, NULL, NULL, &st, NULL, NULL, NULL, NULL, hist, &sum,
                                    0, NULL, NULL, NULL, &ts) != MCP_E_ARG) return 4;
            return 0;
        }''')
    exe = tmp_path / "tb"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "ctx is NULL" in out.stdout, (out.returncode, out.stdout, out.stderr)


# ---- 2. argument rules through the C ABI, with a NULL context ------------------------------------------------------------------------

def _call(prm, bd=True, every=2, reserved=0, cost=1e-3, tol="ok", hist=True, total=True, ts=True, levels=(), q=None, trades=False, turn=False,
          boot=None, hz=(), both=False):
    """mcp_simulate_banded with a NULL context through an untyped handle (NULL pointers anywhere)."""
    N, K, T = prm.n_assets, prm.n_portfolios, prm.n_steps
    mu, L = np.full(N, 1e-3, np.float32), np.eye(N, dtype=np.float32) * 0.01
    W = np.full((K, N), 1.0 / N, np.float32)
    s, tst = np.zeros(K, _ffi.STATS_DTYPE), np.zeros(K, _ffi.STATS_DTYPE)
    h = np.asarray(hz, np.int32)
    hs = np.zeros(max(1, h.size * K), _ffi.STATS_DTYPE)
    table = np.full((K, N), 0.05, np.float32) if isinstance(tol, str) else None if tol is None else np.ascontiguousarray(tol, np.float32)
    band = _ffi.McpBand(every, reserved, cost, vp(table)) if bd else None
    lv = np.asarray(levels, np.float64)
    hh, tot = np.zeros((K, max(T, 1) + 1), np.uint64), np.zeros(K, np.uint64)
    qq = np.zeros((K, max(1, lv.size)), np.uint32)
    c, y = np.zeros((K, 100), np.uint32), np.zeros((K, 100), np.float32)
    q = lv.size > 0 if q is None else q
    gauss = boot is None or both
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    return _raw("mcp_simulate_banded")(
        None, ctypes.byref(prm), ref(band), vp(mu) if gauss else None, vp(L) if gauss else None, ref(boot), vp(W), ctypes.c_uint64(1),
        ctypes.c_uint64(0), ctypes.c_uint64(100), h.size, vp(h) if h.size else None, 0, None, None, vp(s), None, vp(hs) if h.size else None, None,
        vp(c) if trades else None, vp(hh) if hist else None, vp(tot) if total else None, lv.size, vp(lv) if lv.size else None,
        vp(qq) if q else None, vp(y) if turn else None, vp(tst) if ts else None)


def _tol(K, N, k, i, v):
    t = np.full((K, N), 0.05, np.float32)
    t[k, i] = v
    return t


BAD = [  # (keywords of _call, what the error names)
    ({"bd": False}, "band is NULL"), ({"tol": None}, "tol is NULL"),
    ({"tol": _tol(2, 4, 1, 2, -0.01)}, "tol[6]"), ({"tol": _tol(2, 4, 0, 3, float("nan"))}, "tol[3]"),
    ({"tol": _tol(2, 4, 1, 3, -float("inf"))}, "portfolio 1, asset 3"),
    ({"reserved": 1}, "reserved"), ({"every": -1}, "every"), ({"cost": -0.1}, "cost"), ({"cost": 1.0}, "cost"), ({"cost": float("nan")}, "cost"),
    ({"hist": False}, "trade_hist_out"), ({"total": False}, "trade_sum_out"), ({"ts": False}, "turnover_stats_out"),
    ({"levels": [50.0], "q": False}, "trade_q_out"), ({"q": True}, "trade_q_out"),
    ({"levels": [-1.0]}, "level"), ({"levels": [100.5]}, "level"), ({"levels": [float("nan")]}, "level"), ({"levels": [50.0] * 17}, "n_levels"),
    ({"hz": [5, 2]}, "horizon"), ({"boot": "rows", "both": True}, "exactly one draw source"),
]


@pytest.mark.parametrize("kw,what", BAD)
def test_bad_requests_return_e_arg_with_a_null_context(kw, what, mcp_lib):
    rows = np.zeros((5, 4), np.float32)
    if kw.get("boot") == "rows":
        kw = dict(kw, boot=_ffi.make_bootstrap(rows, 2.0))
    assert _call(_ffi.make_params(4, 10, 2), **kw) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()


def test_valid_requests_reach_the_null_context_and_the_refusals_are_unsupported(mcp_lib):
    prm = _ffi.make_params(4, 10, 2)
    rows = np.zeros((5, 4), np.float32)
    inf = float("inf")
    valid = [{}, {"every": 0}, {"every": 11}, {"cost": 0.0}, {"tol": np.zeros((2, 4))}, {"tol": np.full((2, 4), inf)}, {"tol": _tol(2, 4, 1, 1, inf)},
             {"trades": True, "turn": True}, {"levels": [0.0, 5.0, 100.0]}, {"levels": [50.0] * 16}, {"hz": [3, 10]},
             {"boot": _ffi.make_bootstrap(rows, 2.0)}]
    for kw in valid:
        assert _call(prm, **kw) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error(), (kw, mcp_lib.mcp_last_error())
    assert _call(_ffi.make_params(4, 0, 2)) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()       # no steps: one bin
    for kw in ({"compounding": "log"}, {"fold": True}, {"native_math": True}):
        assert _call(_ffi.make_params(4, 10, 1, **kw)) == _ffi.MCP_E_UNSUPPORTED, kw
    top = _ffi.MCP_MAX_LIFE_STEPS                                                   # n_reviews = floor((T - 1) / 1) = T - 1
    assert _call(_ffi.make_params(4, top + 1, 1), every=1) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()
    assert _call(_ffi.make_params(4, top + 2, 1), every=1) == _ffi.MCP_E_UNSUPPORTED and b"MCP_MAX_LIFE_STEPS" in mcp_lib.mcp_last_error()
    assert _call(_ffi.make_params(4, 2 * top + 2, 1), every=2) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()
    # the rebalancing call takes portfolio shards, so the banded call does
    assert _call(_ffi.make_params(4, 10, 2, shard_portfolios=True)) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error()


@pytest.mark.parametrize("T", [0, 1, 2, 7])
@pytest.mark.parametrize("e", [0, 1, 3, 6, 7, 8])
def test_band_reviews_is_the_formula(T, e, mcp_lib):
    want = (T - 1) // e if 1 <= e < T else 0
    assert want == sum(1 for s in range(1, T) if e >= 1 and s % e == 0)
    assert _ffi.band_reviews(T, e) == want == n_reviews(T, e) == band_ref.n_reviews(T, e)
    fn = _raw("mcp_band_reviews")
    assert fn(None, ctypes.byref(_ffi.McpBand(e, 0, 0.0, None))) == -1 and fn(ctypes.byref(_ffi.make_params(1, T, 1)), None) == -1
    assert fn(ctypes.byref(_ffi.make_params(1, T, 1)), ctypes.byref(_ffi.McpBand(-1, 0, 0.0, None))) == -1


# ---- 3. the restatement's exact properties -------------------------------------------------------------------------------------------

def _walk(N=5, K=3, T=24, n=400, scale=4.0):
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(N + K).dirichlet(np.ones(N), size=K)
    W[-1] *= 0.9
    mu32, L, W32 = prepare_inputs(np.asarray(mu) * scale, np.asarray(cov) * scale, W)
    paths = np.arange(n, dtype=np.uint64) + np.uint64((1 << 32) - 100)
    return gauss_returns(mu32, L, T, SEED, paths), W32


@pytest.mark.parametrize("e,cost", [(1, 0.0), (1, 1e-3), (5, 1e-3), (23, 0.0), (7, 2e-3)])
def test_property_a_zero_tolerance_is_the_calendar(e, cost):
    r, W = _walk()
    hz = [1, 5, 12, 24]
    got = band_ref.banded(r, W, 0.0, e, cost, v0=2.0, horizons=hz)
    want = rebalanced(r, W, e, cost, v0=2.0, horizons=hz)
    assert np.array_equal(_bits(got["V_T"]), _bits(want["V_T"])) and np.array_equal(_bits(got["V_h"]), _bits(want["V_h"]))
    assert np.all(got["c"] == band_ref.n_reviews(24, e)) and got["hits"].all() and np.all(got["Y"] > 0)


@pytest.mark.parametrize("tol,e", [(np.inf, 1), (np.inf, 5), (0.0, 0), (0.01, 0), (0.0, 24), (0.01, 30)])
def test_property_b_nothing_watched_or_no_review_is_buy_and_hold(tol, e):
    r, W = _walk()
    hz = [1, 5, 12, 24]
    got = band_ref.banded(r, W, tol, e, 1e-3, v0=2.0, horizons=hz)
    want = rebalanced(r, W, 0, 1e-3, v0=2.0, horizons=hz)
    assert np.array_equal(_bits(got["V_T"]), _bits(want["V_T"])) and np.array_equal(_bits(got["V_h"]), _bits(want["V_h"]))
    assert not got["c"].any() and np.array_equal(_bits(got["Y"]), np.zeros_like(_bits(got["Y"])))


def _mixed_table(W, tol):
    t = np.full(W.shape, tol, np.float32)
    t[:, 1] = np.inf
    return t


def test_property_c_and_e_on_a_mixed_table():
    r, W = _walk()
    T, e, hz = 24, 3, [3, 4, 12, 23]
    tol = _mixed_table(W, 0.03)
    got = band_ref.banded(r, W, tol, e, 1e-3, horizons=hz)
    frac = got["hits"].mean()
    assert 0.15 < frac < 0.85 and got["hits"].any(axis=(1, 2)).all()       # the case decides something
    for i, h in enumerate(hz):
        cut = band_ref.banded(r[:h], W, tol, e, 1e-3)
        assert np.array_equal(_bits(got["V_h"][i]), _bits(cut["V_T"])), h
        assert np.array_equal(cut["c"], got["hits"][:band_ref.n_reviews(h, e)].sum(axis=0)), h    # the trades before step h
    assert np.all(got["c"] <= band_ref.n_reviews(T, e)) and np.array_equal(got["c"], got["hits"].sum(axis=0))
    zero = got["c"] == 0
    assert zero.any() and np.array_equal(_bits(got["Y"][zero]), np.zeros(int(zero.sum()), np.uint32)) and np.all(got["Y"][~zero] > 0)
    # an unwatched asset decides nothing: its entry may be anything
    other = tol.copy()
    other[:, 1] = np.float32(1.0e30)
    assert np.array_equal(band_ref.banded(r, W, other, e, 1e-3)["c"], got["c"])


def test_restatement_against_the_dollar_holdings_twin():
    """N = 4, T = 60, e = 5, 20 000 paths, weights (0.4, 0.3, 0.2, 0.1), per-step vols 2 to 8 %, tol = 0.02.  On the paths whose decision
    sequences coincide V_T agrees within the first-order bound of the binary32 walk's roundings, u = 2^-24 each, relative to V: per step
    and asset the add and the fma of the B update (2 u on 1 + B_i, so 2 T u over the walk), and per event (the n_reviews reviews and T)
    the N4 fmas of the mark, the fma of V^ and, with a cost, tau's N4 fmas and subtractions scaled by kappa = 1e-3 and the fma of rho'
    (N4 + 4 roundings at most): (2 T + (n_reviews + 1)(N4 + 4)) u = 216 u = 1.3e-5.  The binary64 twin's own error is 2^-29 of that."""
    N, T, e, n, kap = 4, 60, 5, 20_000, 1e-3
    W = np.array([[0.4, 0.3, 0.2, 0.1]])
    vol = np.array([0.02, 0.04, 0.06, 0.08])
    corr = 0.3 + 0.7 * np.eye(N)
    mu32, L, W32 = prepare_inputs(np.full(N, 2e-3), corr * np.outer(vol, vol), W)
    r = gauss_returns(mu32, L, T, SEED, np.arange(n, dtype=np.uint64))
    got, twin = band_ref.banded(r, W32, 0.02, e, kap), band_ref.dollar_bands(r, W32, 0.02, e, kap)
    same = (got["hits"] == twin["hits"]).all(axis=0)[0]
    assert same.mean() >= 0.999, same.mean()
    share = got["hits"].mean()
    counts = np.bincount(got["c"][0], minlength=12)
    assert 0.3 < share < 0.9 and np.all(counts[1:] > 0), (share, counts)
    bound = (2 * T + (band_ref.n_reviews(T, e) + 1) * (N + 4)) * 2.0 ** -24
    rel = np.abs(got["V_T"][0, same].astype(np.float64) / twin["V_T"][0, same] - 1.0)
    assert rel.max() <= bound, (rel.max(), bound)
    assert np.array_equal(got["c"][0, same], twin["c"][0, same])


# ---- 4. tolerance_bands, band_law, check_tolerance -----------------------------------------------------------------------------------

def test_tolerance_bands():
    w = np.array([0.5, 0.3, 0.1, 0.1, 0.0])
    assert np.array_equal(tolerance_bands(w, absolute=0.05), np.full(5, 0.05))
    assert np.array_equal(tolerance_bands(w, relative=0.25), [0.125, 0.075, 0.025, 0.025, np.inf])
    assert np.array_equal(tolerance_bands(w, absolute=0.05, relative=0.25), [0.05, 0.05, 0.025, 0.025, 0.0])      # the 5/25 rule
    assert np.array_equal(tolerance_bands(-w, relative=0.25)[:4], [0.125, 0.075, 0.025, 0.025])
    W2 = np.stack([w, w[::-1]])
    assert tolerance_bands(W2, 0.05, 0.25).shape == (2, 5) and np.array_equal(tolerance_bands(W2, 0.05, 0.25)[1], [0.0, 0.025, 0.025, 0.05, 0.05])
    for bad in (dict(), dict(absolute=-1.0), dict(relative=float("nan")), dict(absolute=True), dict(relative="x")):
        with pytest.raises(ValueError):
            tolerance_bands(w, **bad)
    with pytest.raises(ValueError):
        tolerance_bands(np.zeros((2, 2, 2)), absolute=0.1)


def test_check_tolerance():
    tol, lv = check_tolerance(0.05, (5, 50), (2, 3), 10, 2)
    assert tol.dtype == np.float32 and tol.shape == (2, 3) and tol.flags.c_contiguous and np.all(tol == np.float32(0.05)) and list(lv) == [5.0, 50.0]
    assert np.array_equal(check_tolerance([0.1, np.inf, 0.0], (), (2, 3), 10, 2)[0], np.array([[0.1, np.inf, 0.0]] * 2, np.float32))
    assert check_tolerance(np.full((2, 3), 0.2), (), (2, 3), 10, 2)[0].shape == (2, 3)
    for bad in (-0.1, float("nan"), [0.1, 0.2], np.zeros((3, 3)), np.zeros((2, 3, 1)), "x", True, None):
        with pytest.raises(ValueError):
            check_tolerance(bad, (), (2, 3), 10, 2)
    for bad in ([-1.0], [101.0], [50.0] * 17, "x"):
        with pytest.raises(ValueError):
            check_tolerance(0.1, bad, (2, 3), 10, 2)
    with pytest.raises(ValueError):
        check_tolerance(0.1, (), (1, 1), _ffi.MCP_MAX_LIFE_STEPS + 2, 1)


def test_band_law():
    Phi = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))   # noqa: E731
    w, mu, s, tol = 0.5, 0.001, 0.05, 0.01
    up, dn = tol / (w * (1 - w) - tol * w), -tol / (w * (1 - w) + tol * w)
    assert abs(band_law(w, mu, s, tol) - ((1 - Phi((up - mu) / s)) + Phi((dn - mu) / s))) < 1e-15
    assert band_law(w, mu, s, 0.0) == 1.0 and band_law(w, mu, s, float("inf")) == 0.0
    assert band_law(w, mu, s, 0.5) < 1e-12 and band_law(0.3, mu, s, 0.005) > band_law(0.3, mu, s, 0.01) > band_law(0.3, mu, s, 0.02)
    # against the rule itself on a fine grid of r
    r = np.linspace(-0.5, 0.5, 2_000_001)
    dens = np.exp(-0.5 * ((r - mu) / s) ** 2) / (s * math.sqrt(2 * math.pi))
    trade = w * (1 - w) * np.abs(r) >= tol * (1 + w * r)
    assert abs(np.sum(dens[trade]) * (r[1] - r[0]) - band_law(w, mu, s, tol)) < 1e-5
    with pytest.raises(ValueError):
        band_law(w, mu, 0.0, tol)


# ---- 5. the front end over the recorder ----------------------------------------------------------------------------------------------

N, PATHS = front_end_cases.N, front_end_cases.PATHS


def test_entry_tables():
    assert simulate._BAND_CHOICE[0] == "mcp_simulate_banded" and simulate._KEYWORD_GROUP["tolerance"] == "tb"
    groups = _ffi.BAND_ENTRIES["mcp_simulate_banded"]
    for kw in ("dof", "period", "drawdown", "flows", "overlay", "garch", "attribution", "antithetic", "filtered", "jumps", "regimes", "glide",
               "protect", "spending", "lifetime"):
        assert simulate._KEYWORD_GROUP[kw] not in groups, kw
    for kw in ("rows", "horizons", "tolerance"):
        assert simulate._KEYWORD_GROUP[kw] in groups, kw
    assert simulate._ENTRY_CHOICE[0][1] == "mcp_simulate_spending"           # the parent's table is untouched
    assert "tolerance" in simulate._PATHS_COMBINE and "tolerance" in simulate._BOOTSTRAP_COMBINE


def test_call_routes_tolerance_and_refuses_every_other_keyword():
    f32 = np.float32
    mu, chol, W = np.full(N, 1e-3, f32), (0.01 * np.eye(N)).astype(f32), np.full((1, N), 1 / N, f32)
    tb = dict(tolerance=(2, 1e-3, np.full((1, N), 0.05, f32), np.array([50.0])))
    table = np.array([(_ffi.MCP_OVERLAY_PUT, 0.9, 0.01, 1.0)], _ffi.OVERLAY_ROW_DTYPE)
    others = {
        "dof": dict(dof=5), "period": dict(period=2, cost=1e-3), "drawdown": dict(drawdown=True), "flows": dict(flows=np.full(5, 0.01, f32), target=1.0),
        "overlay": dict(overlay=(table, np.array([0, 1, 1, 1], np.int32), np.ones(N, f32))), "garch": dict(garch=(0.05, 0.9, 1.0)),
        "attribution": dict(attribution=True), "antithetic": dict(antithetic=True), "jumps": dict(jumps=(0.1, -0.01, 0.01, None)),
        "regimes": dict(regimes=(0.05, 0.2, 0.1, mu.copy(), chol.copy())), "glide": dict(glide=(np.array([2], np.int32), np.full((1, 1, N), 1 / N, f32))),
        "protect": dict(protect=(np.zeros(6, f32), 3.0, 0.0, 1.0, 0.0)), "spending": dict(spending=(0.02, 2, 0.1, 0.1, 0.0, None)),
        "lifetime": dict(lifetime=np.array([50.0])),
    }
    with front_end_cases.recording() as (rec, ctx):
        prm = _ffi.make_params(N, 5, 1)
        for store in (True, False):
            got = front_end_cases.record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, store, mu=mu, chol=chol, **tb))
            (entry, kinds), = got["calls"]
            assert entry == "mcp_simulate_banded" and len(kinds) == 27 and kinds[2] == "McpBand" and kinds[5] == "NULL"
            tail = ["ptr uint32[1, 8]" if store else "NULL", "ptr uint64[1, 3]", "ptr uint64[1]", 1, "ptr float64[1]", "ptr uint32[1, 1]",
                    "ptr float32[1, 8]" if store else "NULL", f"ptr {_ffi.STATS_DTYPE.name}[1]"]
            assert kinds[19:] == tail, kinds[19:]
        hz = dict(horizons=np.array([2, 5], np.int32), levels=np.array([5.0, 50.0]))
        (entry, kinds), = front_end_cases.record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, True, mu=mu, chol=chol, **tb, **hz))["calls"]
        assert entry == "mcp_simulate_banded" and kinds[10:14] == [2, "ptr int32[2]", 2, "ptr float64[2]"]
        rows = dict(rows=np.full((6, N), 1e-3, f32), block=2.0)
        (entry, kinds), = front_end_cases.record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, True, **tb, **rows))["calls"]
        assert entry == "mcp_simulate_banded" and kinds[3:6] == ["NULL", "NULL", "McpBootstrap"]
        for name, kw in others.items():
            got = front_end_cases.record(rec, lambda: ctx._call(prm, W, 7, 0, PATHS, True, mu=mu, chol=chol, **tb, **kw))
            assert got.get("raises") == ["ValueError", simulate._BAND_CHOICE[1]], (name, got)


PUBLIC_REFUSED = {
    "drawdown": dict(drawdown=True), "cashflow": dict(cashflow=0.01), "glide": dict(glide=([2], [[0.5, 0.25, 0.25]])),
    "protect": dict(protect=0.8), "spending": dict(spending=(0.02, 2, 0.1, 0.1)), "overlay": dict(overlay={0: [("Long Put", 90.0, 1.0, 1.0)]}, spot=[100.0] * 3),
    "dof": dict(dof=5), "garch": dict(garch=(0.05, 0.9)), "jumps": dict(jumps=(0.1, -0.01, 0.01)),
    "regimes": dict(regimes=(0.05, 0.2, np.full(N, -1e-3), 4e-4 * np.eye(N))), "attribution": dict(attribution=True), "antithetic": dict(antithetic=True),
    "fold": dict(fold=True), "native_math": dict(native_math=True), "compounding='log'": dict(compounding="log"),
}


def test_public_functions_route_and_refuse(mcp_lib):
    mu, cov, w = np.full(N, 1e-3), 1e-4 * np.eye(N), np.full(N, 1 / N)
    returns = np.linspace(-0.02, 0.02, 10 * N).reshape(10, N)
    W2 = np.array([[0.5, 0.25, 0.25], [0.2, 0.3, 0.5]])
    paths = lambda **kw: simulate_paths(mu, cov, w, n_steps=6, n_paths=PATHS, **kw)   # noqa: E731
    boot = lambda **kw: simulate_bootstrap(returns, w, n_steps=6, n_paths=PATHS, **kw)   # noqa: E731
    with front_end_cases.recording(mcp_lib) as (rec, _):
        for fn, draws in ((paths, ["ptr float32[3]", "ptr float32[3, 3]", "NULL"]), (boot, ["NULL", "NULL", "McpBootstrap"])):
            for kw, every, n_rev in ((dict(tolerance=0.05), 1, 5), (dict(tolerance=0.05, rebalance=2, rebalance_cost=1e-3), 2, 2),
                                     (dict(tolerance=[0.05, np.inf, 0.0], rebalance="never"), 0, 0),
                                     (dict(tolerance=tolerance_bands(w, 0.05, 0.25), rebalance=6), 6, 0)):
                got = front_end_cases.record(rec, lambda: fn(**kw))
                (entry, kinds), = got["calls"]
                assert entry == "mcp_simulate_banded" and kinds[3:6] == draws and kinds[20] == f"ptr uint64[1, {n_rev + 1}]", (kw, kinds)
                assert "tolerance" in got["keys"] and "terminal" not in got["keys"]
            res = fn(tolerance=0.05, rebalance=2, store=True, horizons=[2, 6], bands=(5.0,))
            blk = res["tolerance"]
            assert blk["every"] == 2 and blk["n_reviews"] == 2 and blk["table"].shape == (3,) and blk["trades"]["hist"].shape == (3,)
            assert sorted(blk["trades"]) == ["hist", "mean", "paths", "q"] and sorted(blk["trades"]["q"]) == [5.0, 50.0, 95.0]
            assert blk["trades"]["paths"].shape == (PATHS,) and blk["turnover"]["paths"].shape == (PATHS,) and "horizons" in res
            assert sorted(blk["turnover"]) == ["cvar", "max", "mean", "min", "n_tail", "paths", "std", "var", "x_hi", "x_lo"]
            arr = fn(tolerance=0.05, rebalance=2, as_array=True, tolerance_levels=(50,))
            assert len(arr) == 5 and arr[1].shape == (1, 3) and arr[3].shape == (1, 1) and arr[4].dtype == _ffi.STATS_DTYPE
            assert len(fn(tolerance=0.05, rebalance=2, as_array=True, store=True)) == 8
        two = simulate_paths(mu, cov, W2, n_steps=6, n_paths=PATHS, tolerance=tolerance_bands(W2, relative=0.25), rebalance=3)
        assert len(two) == 2 and two[1]["tolerance"]["n_reviews"] == 1 and np.allclose(two[1]["tolerance"]["table"], [0.05, 0.075, 0.125])
        # refusals: every keyword the bands are not combined with, before anything is called
        for name, kw in PUBLIC_REFUSED.items():
            got = front_end_cases.record(rec, lambda: paths(tolerance=0.05, **kw))
            assert got.get("raises", [None])[0] == "ValueError" and got["raises"][1] == simulate._PATHS_COMBINE["tolerance"][0] + ": not with " + name, (name, got)
        for name in ("cashflow", "glide", "spending", "compounding='log'"):
            got = front_end_cases.record(rec, lambda: boot(tolerance=0.05, **PUBLIC_REFUSED[name]))
            assert got.get("raises", [None])[0] == "ValueError" and got["raises"][1] == simulate._BOOTSTRAP_COMBINE["tolerance"][0] + ": not with " + name, (name, got)
        for bad in (dict(tolerance=-0.1), dict(tolerance=[0.1, 0.2]), dict(tolerance=0.1, tolerance_levels=[101]), dict(tolerance=0.1, rebalance=0),
                    dict(tolerance=0.1, rebalance_cost=1.0), dict(tolerance=0.1, lifetime=True)):
            for fn in (paths, boot):
                assert front_end_cases.record(rec, lambda: fn(**bad)).get("raises", [None])[0] == "ValueError", bad
        from monte_carlo_portfolio_amd import engine
        with pytest.raises(ValueError, match="simulate_sweep does not take tolerance"):
            simulate.simulate_sweep(mu, cov, weights=W2, n_steps=6, n_paths=PATHS, tolerance=0.05)
        assert "tolerance" not in engine.PathEngine.__init__.__code__.co_varnames

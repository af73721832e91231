"""CPU checks of floor protection (SPEC.md 4.15 / 5.15): every argument rule and refusal of mcp_simulate_protected, mcp_protect_pivots
and mcp_protect_floor through the C ABI with no device and of simulate_paths(protect=...) with no context; the extension header
against _ffi.EXTENSION_SIGNATURES and the exported symbols, and its C99 compile and link; the floor helper against Python bit for
bit; the pivots against a binary64 restatement; protect_law against a binary64 twin on NumPy normals through the assertions the GPU
law test uses; the exact anchors on the restatement (protect_ref.py)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import front_end_cases
import protect_ref
from monte_carlo_portfolio_amd import _ffi, floor_schedule, protect_law, simulate_paths, simulate_sweep, synthetic
from monte_carlo_portfolio_amd.simulate import check_protect, prepare_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcport_protect.h")
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


def _raw(name):
    fn = getattr(ctypes.CDLL(_ffi.LIB_PATH), name)
    fn.restype = ctypes.c_int
    return fn


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. header / binding / library ----------------------------------------------------------------------------------------------

def _protos():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return text, dict(re.findall(r"\b(mcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))


def test_extension_header_binding_and_library_agree(mcp_lib):
    text, protos = _protos()
    assert sorted(protos) == sorted(_ffi.EXTENSION_SIGNATURES) == ["mcp_protect_floor", "mcp_protect_pivots", "mcp_simulate_protected"]
    for name, params in protos.items():
        assert len(params.split(",")) == len(_ffi.EXTENSION_SIGNATURES[name][1]), name
        assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), name) and hasattr(mcp_lib, name)
        assert name not in _ffi.SIGNATURES and name not in _ffi.SIMULATE_ENTRIES
    assert getattr(mcp_lib, "mcp_simulate_protected").argtypes == _ffi.EXTENSION_SIGNATURES["mcp_simulate_protected"][1]
    assert sorted(_ffi.EXTENSION_ENTRIES) == ["mcp_simulate_protected"]
    assert _ffi.EXTENSION_ENTRIES["mcp_simulate_protected"] == tuple("ctx prm pt gv st jp mu chol W walk hz_in out dd counts hz_out hz_counts".split())
    assert '#include "mcport.h"' in text and 'extern "C"' in text and "MCP_ABI_VERSION" not in text
    assert re.search(r"typedef struct \{\s*const float\s*\*floor;\s*double\s+multiplier, cap, rate, ratchet;\s*const double \*target;\s*"
                     r"int32_t\s+reserved;\s*\} mcp_protect;", text)
    assert [f[0] for f in _ffi.McpProtect._fields_] == ["floor", "multiplier", "cap", "rate", "ratchet", "target", "reserved"]
    assert ctypes.sizeof(_ffi.McpProtect) == 56
    assert mcp_lib.mcp_abi_version() == _ffi.MCP_ABI_VERSION == 4
    main = open(os.path.join(ROOT, "include", "mcport.h")).read()
    assert "protect" not in main                               # the main header is the parent's


def test_c99_compile_and_link_of_the_extension_header(tmp_path, mcp_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "pt.c"
    src.write_text(r'''
        #include <stdio.h>
        #include "mcport_protect.h"
        int main(void) {
            mcp_params p = {3, 4, 2, MCP_COMPOUND_SIMPLE, 0, 0, 1.0, 0.95, 0.0};
            float mu[3] = {0.01f, 0.002f, -0.001f}, chol[9] = {0.05f, 0, 0, 0.01f, 0.04f, 0, 0, 0, 0.03f};
            float w[6] = {0.5f, 0.3f, 0.2f, 0.2f, 0.3f, 0.5f}, floor[5];
            double piv[2];
            uint64_t counts[4];
            mcp_stats s[2];
            mcp_protect pt = {floor, 4.0, 1.0, 0.001, 0.0, NULL, 0};
            if (sizeof(mcp_protect) != 56) return 1;
            if (mcp_protect_floor(0.8, 0.001, 4, floor) != MCP_OK || floor[0] != 0.8f || !(floor[4] > floor[3])) return 2;
            if (mcp_protect_pivots(&p, &pt, mu, w, 0, NULL, piv, NULL) != MCP_OK) return 3;
            if (mcp_simulate_protected(NULL, &p, &pt, NULL, NULL, NULL, mu, chol, w, 1, 0, 8, 0, NULL, 0, NULL, NULL, s, NULL, NULL, counts,
                                       NULL, NULL, NULL, NULL) != MCP_E_ARG) return 4;
            pt.cap = 0.0;
            if (mcp_simulate_protected(NULL, &p, &pt, NULL, NULL, NULL, mu, chol, w, 1, 0, 8, 0, NULL, 0, NULL, NULL, s, NULL, NULL, counts,
                                       NULL, NULL, NULL, NULL) != MCP_E_ARG) return 5;
            printf("%s\n", mcp_last_error());
            return 0;
        }''')
    exe = tmp_path / "pt"
    libdir = os.path.dirname(_ffi.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe), f"-L{libdir}", "-lmcport", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                        "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "cap" in out.stdout, (out.returncode, out.stdout, out.stderr)


# ---- 2. argument rules through the C ABI, with a NULL context ------------------------------------------------------------------------

def _call(prm, pt="ok", floor=None, m=4.0, cap=1.0, rate=0.001, ratchet=0.0, target=None, reserved=0, gv=None, st=None, jp=None, hz=(),
          levels=(), counts=True, hz_counts=None, dd=False, mdd=False, mu=True, chol=True, W=True, stats=True):
    """mcp_simulate_protected with a NULL context through an untyped handle (NULL pointers anywhere)."""
    N, K, T = prm.n_assets, prm.n_portfolios, prm.n_steps
    mu_a, L = np.full(N, 1e-3, np.float32), np.eye(N, dtype=np.float32) * 0.01
    Wm = np.full((K, N), 1.0 / N, np.float32)
    s, d = np.zeros(K, _ffi.STATS_DTYPE), np.zeros(K, _ffi.STATS_DTYPE)
    cn = np.zeros((K, 2), np.uint64)
    h, lv = np.asarray(hz, np.int32), np.asarray(levels, np.float64)
    hs = np.zeros(max(1, h.size * K), _ffi.STATS_DTYPE)
    bb = np.zeros(max(1, h.size * K * lv.size), np.float64)
    hc = np.zeros((max(1, h.size), K, 2), np.uint64)
    q = np.zeros((K, 100), np.float32)
    fl = np.full(T + 1, 0.8, np.float32) if floor is None else np.asarray(floor, np.float32)
    tg = np.array([target], np.float64) if target is not None else None
    hz_counts = h.size > 0 if hz_counts is None else hz_counts
    if pt == "ok":
        pt = _ffi.McpProtect(vp(fl), m, cap, rate, ratchet, vp(tg) if tg is not None else None, reserved)
    elif pt == "null_floor":
        pt = _ffi.McpProtect(None, m, cap, rate, ratchet, None, 0)
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    return _raw("mcp_simulate_protected")(
        None, ctypes.byref(prm), ref(pt), ref(gv), ref(st), ref(jp), vp(mu_a) if mu else None, vp(L) if chol else None, vp(Wm) if W else None,
        ctypes.c_uint64(1), ctypes.c_uint64(0), ctypes.c_uint64(100), h.size, vp(h) if h.size else None, lv.size, vp(lv) if lv.size else None,
        None, vp(s) if stats else None, vp(q) if mdd else None, vp(d) if dd else None, vp(cn) if counts else None, None,
        vp(hs) if h.size else None, vp(bb) if lv.size else None, vp(hc) if hz_counts else None)


def _floor_with(T, t, value):
    f = np.full(T + 1, 0.8, np.float32)
    f[t] = value
    return f


BAD = [  # (keywords of _call, what the error names)
    ({"pt": None}, "protect is NULL"), ({"pt": "null_floor"}, "floor is NULL"), ({"reserved": 3}, "reserved"),
    ({"m": float("nan")}, "finite"), ({"m": float("inf")}, "finite"), ({"m": 1e60}, "finite"), ({"m": -0.5}, "multiplier"),
    ({"cap": float("nan")}, "finite"), ({"cap": 1e39}, "finite"), ({"cap": 0.0}, "cap"), ({"cap": -1.0}, "cap"), ({"cap": 1e-60}, "cap"),
    ({"rate": float("inf")}, "finite"), ({"rate": -1.0}, "rate"), ({"rate": -2.0}, "rate"), ({"rate": -1.0 + 1e-12}, "rate"),
    ({"ratchet": float("nan")}, "finite"), ({"ratchet": -0.1}, "ratchet"), ({"ratchet": 1.0}, "ratchet"), ({"ratchet": 1.0 - 1e-12}, "ratchet"),
    ({"target": float("nan")}, "target"), ({"target": 1e60}, "target"),
    ({"floor": _floor_with(10, 0, -0.1)}, "floor, step 0"), ({"floor": _floor_with(10, 10, np.nan)}, "floor, step 10"),
    ({"floor": _floor_with(10, 4, np.inf)}, "floor, step 4"),
    ({"counts": False}, "counts_out"), ({"hz": [2, 5], "hz_counts": False}, "hz_counts_out"), ({"hz_counts": True}, "hz_counts_out"),
    ({"mdd": True}, "mdd_out needs dd_stats_out"), ({"hz": [5, 2]}, "horizon"), ({"hz": [2, 11]}, "horizon"),
    ({"gv": _ffi.McpGarch(0.5, 0.6, 1.0, 0)}, "alpha + beta"), ({"st": _ffi.McpStudentT(2, 0)}, "dof"),
    ({"jp": _ffi.McpJumps(2.0, -0.1, 0.1, None, 0)}, "intensity"), ({"mu": False}, "NULL pointer"), ({"chol": False}, "NULL pointer"),
    ({"W": False}, "NULL pointer"), ({"stats": False}, "NULL pointer"),
]


@pytest.mark.parametrize("kw,what", BAD)
def test_bad_requests_return_e_arg_with_a_null_context(kw, what, mcp_lib):
    assert _call(_ffi.make_params(4, 10, 2), **kw) == _ffi.MCP_E_ARG
    assert what.encode() in mcp_lib.mcp_last_error(), mcp_lib.mcp_last_error()


def test_valid_requests_reach_the_null_context(mcp_lib):
    prm = _ffi.make_params(4, 10, 2)
    assert _call(_ffi.make_params(4, 10, 1, v0=1e-60)) == _ffi.MCP_E_ARG and b"rounds to zero" in mcp_lib.mcp_last_error()
    assert _call(prm, cap=0.0) == _ffi.MCP_E_ARG and b"cap" in mcp_lib.mcp_last_error()
    valid = [{}, {"m": 0.0}, {"ratchet": 0.9}, {"cap": 2.0 ** 20}, {"rate": -0.5}, {"target": 1.1}, {"floor": np.zeros(11, np.float32)},
             {"floor": _floor_with(10, 3, 5.0)}, {"dd": True}, {"dd": True, "mdd": True}, {"hz": [3, 10], "levels": [5.0, 95.0]},
             {"st": _ffi.McpStudentT(5, 0)}, {"gv": _ffi.McpGarch(0.1, 0.85, 1.5, 0)},
             {"gv": _ffi.McpGarch(0.1, 0.85, 1.5, 0), "st": _ffi.McpStudentT(5, 0)}, {"jp": _ffi.McpJumps(0.3, -0.05, 0.04, None, 0)}]
    for kw in valid:
        assert _call(prm, **kw) == _ffi.MCP_E_ARG and b"ctx is NULL" in mcp_lib.mcp_last_error(), (kw, mcp_lib.mcp_last_error())


@pytest.mark.parametrize("kw", [{"compounding": "log"}, {"fold": True}, {"native_math": True}])
def test_log_fold_and_native_math_are_unsupported(kw, mcp_lib):
    prm = _ffi.make_params(4, 10, 1, **kw)
    for more in ({}, {"hz": [2, 5]}, {"dd": True}, {"st": _ffi.McpStudentT(5, 0)}, {"jp": _ffi.McpJumps(0.3, -0.05, 0.04, None, 0)}):
        assert _call(prm, **more) == _ffi.MCP_E_UNSUPPORTED and b"protected paths" in mcp_lib.mcp_last_error()


def test_unsupported_combinations(mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    assert _call(prm, dd=True, hz=[2, 5]) == _ffi.MCP_E_UNSUPPORTED and b"horizons and the drawdown" in mcp_lib.mcp_last_error()
    jp = _ffi.McpJumps(0.3, -0.05, 0.04, None, 0)
    for more in ({"st": _ffi.McpStudentT(5, 0)}, {"gv": _ffi.McpGarch(0.1, 0.85, 1.0, 0)}):
        assert _call(prm, jp=jp, **more) == _ffi.MCP_E_UNSUPPORTED and b"jumps are not combined" in mcp_lib.mcp_last_error()
    # no mcp_launch_* entry point takes the protection: the header declares none
    assert not [n for n in _protos()[1] if n.startswith("mcp_launch")]


def test_pivot_and_floor_helper_argument_errors(mcp_lib):
    prm = _ffi.make_params(4, 10, 1)
    W, mu = np.full((1, 4), 0.25, np.float32), np.zeros(4, np.float32)
    fl, hz = np.full(11, 0.8, np.float32), np.array([3, 10], np.int32)
    out, hout = np.zeros(1, np.float64), np.zeros((2, 1), np.float64)
    fn = _raw("mcp_protect_pivots")
    ok = _ffi.McpProtect(vp(fl), 4.0, 1.0, 0.0, 0.0, None, 0)
    P, G = ctypes.byref(prm), ctypes.byref(ok)
    assert fn(P, None, vp(mu), vp(W), 0, None, vp(out), None) == _ffi.MCP_E_ARG
    assert fn(P, G, None, vp(W), 0, None, vp(out), None) == _ffi.MCP_E_ARG
    assert fn(P, G, vp(mu), None, 0, None, vp(out), None) == _ffi.MCP_E_ARG
    assert fn(P, G, vp(mu), vp(W), 0, None, None, None) == _ffi.MCP_E_ARG
    assert fn(P, G, vp(mu), vp(W), 2, vp(hz), vp(out), None) == _ffi.MCP_E_ARG
    assert fn(P, G, vp(mu), vp(W), 2, vp(np.array([10, 3], np.int32)), vp(out), vp(hout)) == _ffi.MCP_E_ARG
    assert fn(P, ctypes.byref(_ffi.McpProtect(vp(fl), -1.0, 1.0, 0.0, 0.0, None, 0)), vp(mu), vp(W), 0, None, vp(out), None) == _ffi.MCP_E_ARG
    assert fn(ctypes.byref(_ffi.make_params(4, 10, 1, "log")), G, vp(mu), vp(W), 0, None, vp(out), None) == _ffi.MCP_E_UNSUPPORTED
    assert fn(P, G, vp(mu), vp(W), 0, None, vp(out), None) == 0 and fn(P, G, vp(mu), vp(W), 2, vp(hz), vp(out), vp(hout)) == 0
    ff = _raw("mcp_protect_floor")
    ff.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
    buf = np.zeros(11, np.float32)
    for f0, r, n, o in ((float("nan"), 0.0, 10, buf), (0.8, float("inf"), 10, buf), (1e60, 0.0, 10, buf), (-0.1, 0.0, 10, buf),
                        (0.8, -1.0, 10, buf), (0.8, 0.0, 0, buf), (0.8, 0.0, 10, None), (1e38, 1.0, 10, buf)):
        assert ff(f0, r, n, vp(o) if o is not None else None) == _ffi.MCP_E_ARG, (f0, r, n)
    assert ff(0.8, 0.001, 10, vp(buf)) == 0


# ---- 3. the floor helper and the pivots ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("floor,rate,T,v0", [(0.8, 0.001, 252, 1.0), (0.8, 0.0, 12, 1.0), (0.95, 0.0123456789, 60, 10_000.0),
                                            (0.0, 0.5, 7, 1.0), (1.0 / 3.0, -0.25, 40, 3.0), (0.7, 1e-9, 1000, 1.0)])
def test_floor_helper_equals_python_bit_for_bit(floor, rate, T, v0, mcp_lib):
    got = _ffi.protect_floor(floor * v0, rate, T)
    want = floor_schedule(floor, rate, T, v0)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (T + 1,)
    assert np.array_equal(_bits(got), _bits(want))
    assert got[0] == np.float32(floor * v0)
    r32 = np.float32(rate)
    ref = protect_ref._fma32(got[:-1], np.full(T, r32, np.float32), got[:-1])     # every step is one correctly rounded fma
    assert np.array_equal(_bits(ref), _bits(got[1:]))


def _pivot64(S, v0, rf, m, mk, h):
    g = 1.0 + rf + m * (mk - rf)
    c = ((float(S[h]) + (v0 - float(S[0])) * math.pow(g, float(h))) / v0) - 1.0 if g > 0.0 else float("nan")
    if not math.isfinite(c):
        c = math.expm1(h * math.log1p(mk)) if mk > -1.0 else 0.0
        c = c if math.isfinite(c) else 0.0
    return c


@pytest.mark.parametrize("m,rate,v0", [(3.0, 0.001, 1.0), (5.0, 0.0, 10_000.0), (0.0, 0.002, 1.0), (1.0, 0.001, 2.5), (400.0, 0.001, 1.0)])
def test_pivots_equal_the_binary64_restatement(m, rate, v0, mcp_lib):
    N, K, T, hz = 5, 4, 60, [1, 12, 30, 60]
    mu, cov = synthetic.synthetic_market(N)
    mu32, _, W32 = prepare_inputs(mu, cov, synthetic.dirichlet_weights(N, K))
    if m == 400.0:
        mu32 = (mu32 - np.float32(0.01)).astype(np.float32)   # g <= 0: the plain call's pivot
    S = floor_schedule(0.8, rate, T, v0)
    S[T // 2:] += np.float32(0.01 * v0)
    pt = _ffi.make_protect(S, m, rate)
    got, ghz = _ffi.protect_pivots(_ffi.make_params(N, T, K, v0=v0), pt, mu32, W32, hz)
    v0d, rf, mm = float(np.float32(v0)), float(np.float32(rate)), float(np.float32(m))
    fell_back = 0
    for k in range(K):
        mk = 0.0
        for i in range(N):
            mk += float(W32[k, i]) * float(mu32[i])
        fell_back += 1.0 + rf + mm * (mk - rf) <= 0.0
        assert got[k] == pytest.approx(_pivot64(S, v0d, rf, mm, mk, T), rel=1e-14, abs=1e-300)
        for i, h in enumerate(hz):
            assert ghz[i, k] == pytest.approx(_pivot64(S, v0d, rf, mm, mk, h), rel=1e-14, abs=1e-300)
    assert (fell_back == K) == (m == 400.0)
    if m == 400.0:
        plain = _ffi.pivots(_ffi.make_params(N, T, K), mu32, np.eye(N, dtype=np.float32), W32)
        assert np.array_equal(got, plain)


# ---- 4. protect_law against the binary64 twin, through the GPU law test's assertions ------------------------------------------------

LAW = dict(N=3, T=12, m=3.0, floor=0.8, rate=0.001, cap=2.0 ** 20, ratchet=0.0)


def test_protect_law_holds_for_the_twin_at_a_million_paths():
    mu, cov = synthetic.synthetic_market(LAW["N"])
    w = np.array([0.2, 0.3, 0.5])
    protect = (LAW["floor"], LAW["m"], LAW["rate"], LAW["cap"], LAW["ratchet"])
    mean, var = protect_law(mu, cov, w, LAW["T"], protect)
    pv = check_protect(protect, LAW["T"])
    V = protect_ref.twin_values(mu, cov, w, LAW["T"], 1_000_000, pv, 20261019)
    fig = protect_ref.law_checks(V, mean, var)
    print(fig)
    # the closed form against its own definition, step by step, in binary64
    g = 1.0 + float(np.float32(0.001)) + 3.0 * (float(np.asarray(w, np.float32).astype(np.float64) @ np.asarray(mu, np.float32).astype(np.float64))
                                                 - float(np.float32(0.001)))
    c = 1.0 - float(pv[0][0])
    assert mean == pytest.approx(float(pv[0][12]) + c * g ** 12, rel=1e-15)
    assert var > 0 and protect_law(mu, cov, np.stack([w, w]), 12, protect)[0].shape == (2,)
    assert V.min() > float(pv[0][12])                     # neither a gap nor the cap acted: the law's premise


# ---- 5. the exact anchors, on the restatement ----------------------------------------------------------------------------------------

def _rho(N, K, T, n, scale=1.0, seed=5):
    mu, cov = synthetic.synthetic_market(N)
    mu32, L, W = prepare_inputs(mu, cov * scale, np.random.default_rng(seed).dirichlet(np.ones(N), size=K))
    return protect_ref.rho_of(mu32, L, W, T, 99, np.arange(n, dtype=np.uint64))


def test_anchor_a_zero_floor_is_the_plain_recurrence_bit_for_bit():
    from drawdown_ref import drawdown_state
    rho = _rho(3, 2, 24, 500, scale=30.0)
    T = rho.shape[1]
    for m in (1.0, 4.0):
        out = protect_ref.walk(rho, (np.zeros(T + 1, np.float32), m, 0.003, 1.0, 0.0), horizons=(5, 24))
        for k in range(2):
            VT, q = drawdown_state(rho[k], "simple", 1.0)
            assert np.array_equal(_bits(out["V_T"][k]), _bits(VT)) and np.array_equal(_bits(out["q"][k]), _bits(q))
        assert np.array_equal(_bits(out["V_h"][1]), _bits(out["V_T"]))
        assert np.all(out["branch"] == (protect_ref.E_CUSHION if m == 1.0 else protect_ref.E_CAP)) and not out["ratchet"].any()


def test_anchor_b_zero_multiplier_compounds_v0_at_the_riskless_rate():
    rho = _rho(3, 2, 24, 200)
    for v0, rate in ((1.0, 0.001), (10_000.0, 0.0), (2.5, -0.01)):
        out = protect_ref.walk(rho, (floor_schedule(0.8, rate, 24, v0), 0.0, rate, 1.0, 0.5), v0=v0)
        assert np.all(_bits(out["V_T"]) == _bits(protect_ref.compounded_v0(v0, rate, 24)))
        assert np.all(out["branch"] == protect_ref.E_ZERO)


def test_anchor_c_zero_ratchet_is_the_rule_without_the_peak():
    rho = _rho(3, 1, 24, 500, scale=30.0)
    S = floor_schedule(0.8, 0.001, 24)
    out = protect_ref.walk(rho, (S, 4.0, 0.001, 1.0, 0.0))
    assert not out["ratchet"].any()
    V = np.ones(500, np.float32)                            # the rule written without M at all
    for t in range(24):
        E = np.fmax(np.fmin(np.float32(4.0) * (V - S[t]), V), np.float32(0)).astype(np.float32)
        u = protect_ref._fma32(V - E, np.full(500, 0.001, np.float32), V)
        V = protect_ref._fma32(E, rho[0, t], u)
    assert np.array_equal(_bits(V), _bits(out["V_T"][0]))
    tipp = protect_ref.walk(rho, (S, 4.0, 0.001, 1.0, 0.9))
    assert tipp["ratchet"].any() and not np.array_equal(_bits(tipp["V_T"]), _bits(out["V_T"]))
    # the drawdown bound of the GPU invariant: S = 0, theta = 0.9, m = 4, wherever m |rho| (1 + 2^-20) < 1 on every step
    calm = _rho(3, 1, 24, 500)
    assert np.all(4.0 * np.abs(calm.astype(np.float64)) * (1 + 2.0 ** -20) < 1.0)
    dd = protect_ref.walk(calm, (np.zeros(25, np.float32), 4.0, 0.0, 1.0, 0.9))
    assert dd["ratchet"].all() and dd["q"].min() >= float(np.float32(0.9)) * (1 - 2.0 ** -22)


def test_the_restatement_takes_all_three_branches_under_p1_and_both_ratchet_states_under_p2():
    """The parameter sets of the GPU parity test on the draws of garch_ref at N = 3, T = 12."""
    rho = _rho(3, 3, 12, 600)
    S = floor_schedule(0.8, 0.001, 12)
    P1 = S.copy()
    P1[6:] += np.float32(0.19)
    b = protect_ref.walk(rho, (P1, 5.0, 0.001, 1.0, 0.0))["branch"]
    assert all(np.count_nonzero(b == x) > 100 for x in (protect_ref.E_ZERO, protect_ref.E_CUSHION, protect_ref.E_CAP)), np.bincount(b.ravel())
    r = protect_ref.walk(rho, (S, 4.0, 0.001, 1.0, 0.8))["ratchet"]
    assert np.count_nonzero(r) > 100 and np.count_nonzero(~r) > 100


# ---- 6. the Python front end, with no context ------------------------------------------------------------------------------------------

MU, COV, WV = np.full(3, 1e-3), 1e-4 * np.eye(3), np.full(3, 1 / 3)


@pytest.mark.parametrize("protect,match", [
    (0.8, "protect must be"), ("ab", "protect must be"), ((0.8,), "protect must be"), ((0.8, 4, 0, 1, 0, 0), "protect must be"),
    ((0.8, True), "protect must be"), ((0.8, "4"), "protect must be"), ((0.8, 4.0, None), "protect must be"),
    ((0.8, float("nan")), "finite"), ((0.8, 1e60), "finite"), ((0.8, -1.0), "multiplier"), ((0.8, 4.0, -1.0), "rate"),
    ((0.8, 4.0, 0.0, 0.0), "cap"), ((0.8, 4.0, 0.0, -2.0), "cap"), ((0.8, 4.0, 0.0, 1.0, 1.0), "ratchet"),
    ((0.8, 4.0, 0.0, 1.0, -0.1), "ratchet"), ((-0.1, 4.0), "floor"), ((float("inf"), 4.0), "floor"), ((True, 4.0), "protect must be"),
    (([0.8] * 6, 4.0), r"n_steps \+ 1 = 7"), (([0.8] * 6 + [-0.1], 4.0), "floors must be finite"), (([0.8] * 6 + [float("nan")], 4.0), "floors must be finite"),
    (([0.8] * 6 + ["x"], 4.0), "protect must be"),
])
def test_check_protect_refuses(protect, match):
    with pytest.raises(ValueError, match=match):
        simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, protect=protect)


def test_check_protect_defaults_and_schedule():
    floor, m, rate, cap, ratchet = check_protect((0.8, 4), 6, v0=100.0)
    assert (m, rate, cap, ratchet) == (4.0, 0.0, 1.0, 0.0) and np.all(floor == np.float32(80.0)) and floor.shape == (7,)
    floor, m, rate, cap, ratchet = check_protect((0.8, 4, 0.01, 2, 0.5), 6)
    assert (m, rate, cap, ratchet) == (4.0, 0.01, 2.0, 0.5) and np.array_equal(floor, floor_schedule(0.8, 0.01, 6))
    assert np.array_equal(check_protect((np.linspace(0.5, 0.8, 7), 1.5), 6)[0], np.linspace(0.5, 0.8, 7).astype(np.float32))
    assert check_protect(None, 6) is None


@pytest.mark.parametrize("kw,bad", [
    (dict(rebalance=2), "rebalance"), (dict(cashflow=0.01), "cashflow"), (dict(regimes=(0.05, 0.2, np.full(3, -1e-3), 4e-4 * np.eye(3))), "regimes"),
    (dict(glide=([2], [[0.5, 0.25, 0.25]])), "glide"), (dict(attribution=True), "attribution"), (dict(antithetic=True), "antithetic"),
    (dict(fold=True), "fold"), (dict(native_math=True), "native_math"), (dict(compounding="log"), "compounding='log'"),
    (dict(overlay={0: [(2, 90.0, 1.0, 1.0)]}, spot=[100.0] * 3), "overlay"),
])
def test_protect_refuses_what_is_not_built_with_one_sentence(kw, bad):
    with pytest.raises(ValueError) as e:
        simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, protect=(0.8, 4.0), **kw)
    assert str(e.value) == ("protect needs constant weights, simple compounding, the spec's normals and the unfolded recurrence: not with " + bad)


def test_protect_with_drawdown_and_horizons_or_two_draw_models_is_refused():
    with pytest.raises(ValueError, match="horizons need"):
        simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, protect=(0.8, 4.0), drawdown=True, horizons=[2, 6])
    with pytest.raises(ValueError, match="jumps need"):
        simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, protect=(0.8, 4.0), jumps=(0.1, -0.01, 0.01), dof=5)
    with pytest.raises(ValueError, match="does not take protect"):
        simulate_sweep(MU, COV, weights=np.stack([WV, WV]), n_steps=6, n_paths=8, protect=(0.8, 4.0))
    with pytest.raises(ValueError, match="target needs cashflow"):
        simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, target=1.0)                      # stays refused without protect
    with pytest.raises(ValueError, match="target must be"):
        simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, target=float("nan"), protect=(0.8, 4.0))


def test_the_front_end_reaches_the_extension_entry_point(mcp_lib):
    """simulate_paths(protect=...) over the recording stand-in for the library: the entry point, the groups in the header's order, and
    the 'protect' block."""
    S = "McpProtect"
    with front_end_cases.recording(mcp_lib) as (rec, _):
        res = simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, protect=(0.8, 4.0), target=1.0, horizons=[2, 6], bands=(5.0,), store=True)
        name, kinds = rec.calls[-1]
        assert name == "mcp_simulate_protected" and len(kinds) == len(_ffi.EXTENSION_SIGNATURES[name][1]) == 25
        assert kinds[:6] == ["NULL", "McpParams", S, "NULL", "NULL", "NULL"] and kinds[9:12] == [0, 0, 8]
        assert kinds[12:16] == [2, "ptr int32[2]", 1, "ptr float64[1]"] and kinds[18:20] == ["NULL", "NULL"]
        assert kinds[20] == "ptr uint64[1, 2]" and kinds[24] == "ptr uint64[2, 1, 2]"
        blk = res["protect"]
        assert sorted(blk) == sorted(["floor", "multiplier", "cap", "rate", "ratchet", "target", "n_gap", "gap_probability", "n_short",
                                      "shortfall_probability", "horizons"])
        assert blk["floor"].shape == (7,) and blk["target"] == 1.0 and blk["horizons"]["n_gap"].shape == (2,) and "cashflow" not in res
        simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, protect=(0.8, 4.0), dof=5, garch=(0.05, 0.9), drawdown=True)
        name, kinds = rec.calls[-1]
        assert name == "mcp_simulate_protected" and kinds[2:6] == [S, "McpGarch", "McpStudentT", "NULL"]
        assert kinds[18] == "NULL" and kinds[19].startswith("ptr ")
        simulate_paths(MU, COV, WV, n_steps=6, n_paths=8, protect=(0.8, 4.0), jumps=(0.1, -0.01, 0.01))
        assert rec.calls[-1][0] == "mcp_simulate_protected" and rec.calls[-1][1][2:6] == [S, "NULL", "NULL", "McpJumps"]
        out = simulate_paths(MU, COV, np.stack([WV, WV]), n_steps=6, n_paths=8, protect=(0.8, 4.0), as_array=True)
        assert len(out) == 2 and out[1].shape == (2, 2) and out[1].dtype == np.uint64
        plain = simulate_paths(MU, COV, WV, n_steps=6, n_paths=8)
        assert rec.calls[-1][0] == "mcp_simulate" and "protect" not in plain

"""GPU checks of floor protection (SPEC.md 4.15 / 5.15): terminal values, the drawdown q and the horizon rows bit-equal to the NumPy
restatement (protect_ref.py) over widths, portfolio counts, step counts, a path range across 2^32 and a second grid-stride tile, on
Gaussian, Student-t, GARCH and jump draws, under a stepped floor that reaches all three exposure branches and under a ratchet; the
records, bands and counts against NumPy on the stored values; the exact anchors against the calls without protection; the
invariants (no gap under small Gaussian steps, the ratchet's drawdown bound, gaps under crash jumps); the law at 10^6 paths; tiles,
shards and recovery after a refused call."""
import contextlib
import ctypes
import io
import os
import runpy
import sys

import numpy as np
import pytest

import protect_ref
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, floor_schedule, metrics, protect_law, simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import Context, check_protect, prepare_inputs
from oracle import ref_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x9_CF01
RATE = 0.001
DRAWS = {"gauss": {}, "t": {"dof": 5}, "garch": {"garch": (0.1, 0.85, 1.5)}, "jumps": {"jumps": (0.3, -0.05, 0.04)}}


def _market(N, K, seed=0):
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(seed + 31 * N + K).dirichlet(np.ones(N), size=K)
    if K > 1:
        W[-1] *= 0.9                                     # 10 % cash in one portfolio
    return prepare_inputs(mu, cov, W)


def _pick(n_paths, begin, count=12):
    ids = {0, 1, n_paths - 1, n_paths // 2}
    ids.update(np.linspace(0, n_paths - 1, count).astype(int).tolist())
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 3)))
    if n_paths > 8192 * 256:                             # the second grid-stride tile of the path kernels
        ids.update(range(8192 * 256 - 2, min(n_paths, 8192 * 256 + 3)))
    return np.array(sorted(ids), np.int64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _p1(T):
    """m = 5, b = 1, rf = 0.001, theta = 0 on the floors 0.8 (1.001)^t, plus 0.19 from step T // 2 on."""
    S = floor_schedule(0.8, RATE, T)
    S[T // 2:] += np.float32(0.19)
    return S, 5.0, RATE, 1.0, 0.0


def _p2(T):
    """P1's rising schedule without the step, m = 4, theta = 0.8."""
    return floor_schedule(0.8, RATE, T), 4.0, RATE, 1.0, 0.8


def _kw(draw):
    kw = dict(DRAWS[draw])
    if "jumps" in kw:
        kw["jumps"] = tuple(float(v) for v in kw["jumps"]) + (None,)
    return kw


def _run(ctx, prm, protect, mu, L, W, begin, n, draw="gauss", store=True, **kw):
    return ctx.simulate_protected(prm, protect, mu, L, W, SEED, begin, n, store, **_kw(draw), **kw)


def _hz(T):
    return sorted({1, max(1, T // 2), T})


def _covers(ref, T, which):
    """So that parity cannot pass on one branch alone: under P1 the compared path-steps hold E = 0, E = fl32(m C) and E = fl32(b V);
    under P2 steps where the ratchet binds and steps where it does not."""
    if T < 7:
        return
    if which == "P1":
        got = np.bincount(ref["branch"].ravel(), minlength=3)
        assert np.all(got > 0), got
    else:
        assert ref["ratchet"].any() and not ref["ratchet"].all()


CASES = [  # N, K, T, path_begin, n_paths
    (1, 1, 7, 0, 3000),
    (3, 3, 12, (1 << 32) - 1500, 3000),
    (13, 8, 1, 17, 5000),
    (13, 8, 12, 17, 5000),
    (16, 1, 60, 0, 4096),
    (17, 20, 7, 5, 2000),
    (64, 3, 7, (1 << 32) - 7, 300),
    (3, 1, 12, 0, 1_000_003),
    (3, 1, 7, 0, 8192 * 256 + 77),                       # past the 8192 workgroups of a launch: the second grid-stride tile
]


def _stats_are_numpy(st, values, k, n):
    want = ref_stats.path_stats(values)
    assert st[k]["var"] == want["var"] and st[k]["n_tail"] == want["n_tail"]
    assert st[k]["min"] == want["min"] and st[k]["max"] == want["max"] and st[k]["n"] == n
    for f in ("mean", "std", "sharpe", "cvar"):
        assert abs(st[k][f] - want[f]) <= 1e-12 * max(1.0, abs(want[f])), f


@pytest.mark.parametrize("draw", list(DRAWS))
@pytest.mark.parametrize("N,K,T,begin,n", CASES)
def test_values_equal_the_restatement(N, K, T, begin, n, draw, gpu_ctx):
    mu, L, W = _market(N, K, 3)
    prm = _ffi.make_params(N, T, K)
    ids = _pick(n, begin, 8 if N >= 16 else 24)
    hz, lv, target = _hz(T), (2.5, 50.0), 0.97
    rho = protect_ref.rho_of(mu, L, W, T, SEED, (begin + ids).astype(np.uint64), **DRAWS[draw])       # once, shared by P1 and P2
    for which, protect in (("P1", _p1(T)), ("P2", _p2(T))):
        ref = protect_ref.walk(rho, protect, horizons=hz)
        _covers(ref, T, which)
        S = protect[0]
        dd = _run(gpu_ctx, prm, protect, mu, L, W, begin, n, draw, drawdown=True, target=target)
        assert np.array_equal(_bits(dd.terminal[:, ids]), _bits(ref["V_T"]))
        assert np.array_equal(_bits(dd.qd[:, ids]), _bits(ref["q"]))
        h = _run(gpu_ctx, prm, protect, mu, L, W, begin, n, draw, horizons=hz, levels=lv, target=target)
        assert np.array_equal(_bits(h.terminal), _bits(dd.terminal))
        assert np.array_equal(_bits(h.horizon_terminal[:, :, ids]), _bits(ref["V_h"]))
        assert np.array_equal(_bits(h.horizon_terminal[-1]), _bits(h.terminal))
        assert np.array_equal(h.counts, dd.counts)
        for k in (0, K - 1):
            _stats_are_numpy(dd.stats, dd.terminal[k], k, n)
            assert h.stats[k]["var"] == dd.stats[k]["var"] and h.stats[k]["n_tail"] == dd.stats[k]["n_tail"]
            mdd = dd.qd[k].astype(np.float64) - 1.0
            dar = metrics.var(mdd, 0.95)
            assert dd.dd_stats[k]["var"] == dar and int(dd.dd_stats[k]["n_tail"]) == int(np.count_nonzero(mdd <= dar))
            assert dd.dd_stats[k]["min"] == mdd.min() and dd.dd_stats[k]["max"] == mdd.max()
            assert dd.counts[k, 0] == np.count_nonzero(dd.terminal[k] < S[T]) and dd.counts[k, 1] == np.count_nonzero(dd.terminal[k] < np.float32(target))
            for i, step in enumerate(hz):
                x = x_of(h.horizon_terminal[i, k])
                assert h.hz_stats[i, k]["var"] == np.percentile(x, (1 - 0.95) * 100)
                assert h.hz_stats[i, k]["min"] == x.min() and h.hz_stats[i, k]["max"] == x.max()
                for jj, q in enumerate(lv):
                    assert h.bands[i, k, jj] == np.percentile(x, q)
                assert h.hz_counts[i, k, 0] == np.count_nonzero(h.horizon_terminal[i, k] < S[step])
                assert h.hz_counts[i, k, 1] == np.count_nonzero(h.horizon_terminal[i, k] < np.float32(target))


@pytest.mark.parametrize("N,K,T", [(3, 3, 12), (16, 1, 40), (16, 8, 12), (64, 3, 5)])
def test_anchor_a_zero_floor_is_the_call_without_protection(N, K, T, gpu_ctx):
    """S = 0, theta = 0, b = 1, m >= 1: E = V on every step, so every stored value is the twin call's bit for bit; n, n_tail, var,
    x_lo and x_hi are exact, mean and std agree to SPEC.md 6's 1e-12 (the pivot differs)."""
    n, prm = 20_000, _ffi.make_params(N, T, K)
    mu, L, W = _market(N, K, 1)
    hz = _hz(T)
    twins = {"gauss": lambda **kw: gpu_ctx._call(prm, W, SEED, 7, n, True, mu=mu, chol=L, **kw),
             "t": lambda **kw: gpu_ctx._call(prm, W, SEED, 7, n, True, mu=mu, chol=L, dof=5, **kw),
             "garch": lambda **kw: gpu_ctx._call(prm, W, SEED, 7, n, True, mu=mu, chol=L, garch=(0.1, 0.85, 1.5), **kw),
             "jumps": lambda **kw: gpu_ctx._call(prm, W, SEED, 7, n, True, mu=mu, chol=L, jumps=(0.3, -0.05, 0.04, None), **kw)}
    for draw, twin in twins.items():
        for m in (1.0, 3.0):
            protect = (np.zeros(T + 1, np.float32), m, RATE, 1.0, 0.0)
            want, got = twin(drawdown=True), _run(gpu_ctx, prm, protect, mu, L, W, 7, n, draw, drawdown=True)
            assert np.array_equal(_bits(got.terminal), _bits(want.terminal)) and np.array_equal(_bits(got.qd), _bits(want.qd))
            assert got.dd_stats.tobytes() == want.dd_stats.tobytes() and not got.counts.any()
            wh, gh = twin(horizons=hz, levels=(5.0, 95.0)), _run(gpu_ctx, prm, protect, mu, L, W, 7, n, draw, horizons=hz, levels=(5.0, 95.0))
            assert np.array_equal(_bits(gh.horizon_terminal), _bits(wh.horizon_terminal)) and np.array_equal(gh.bands, wh.bands)
            for a, b in ((got.stats, want.stats), (gh.stats, wh.stats), (gh.hz_stats, wh.hz_stats)):
                for f in ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max"):
                    assert np.array_equal(a[f], b[f]), (draw, f)
                for f in ("mean", "std"):
                    assert np.all(np.abs(a[f] - b[f]) <= 1e-12 * np.maximum(1.0, np.abs(b[f]))), (draw, f)
    far = _run(gpu_ctx, prm, _p1(T), mu, L, W, 7, n)
    assert not np.array_equal(_bits(far.terminal), _bits(twins["gauss"]().terminal))


@pytest.mark.parametrize("v0,rate", [(1.0, 0.001), (10_000.0, 0.0), (2.5, -0.01)])
def test_anchor_b_zero_multiplier_compounds_v0(v0, rate, gpu_ctx):
    N, K, T, n = 5, 3, 24, 5000
    mu, L, W = _market(N, K, 2)
    protect = (floor_schedule(0.8, rate, T, v0), 0.0, rate, 1.0, 0.5)
    for draw in DRAWS:
        out = _run(gpu_ctx, _ffi.make_params(N, T, K, v0=v0), protect, mu, L, W, 3, n, draw, horizons=[1, T], levels=())
        assert np.all(_bits(out.terminal) == _bits(protect_ref.compounded_v0(v0, rate, T)))
        assert np.all(_bits(out.horizon_terminal[0]) == _bits(protect_ref.compounded_v0(v0, rate, 1)))
        assert not out.counts.any() and np.all(out.stats["min"] == out.stats["max"])


def test_gaussian_steps_never_gap_the_floor(gpu_ctx):
    N, K, T, n = 5, 3, 60, 200_000
    mu, L, W = _market(N, K, 4)
    protect = check_protect((0.8, 4.0), T)
    out = _run(gpu_ctx, _ffi.make_params(N, T, K), protect, mu, L, W, 0, n, horizons=[20, 40, 60], levels=())
    assert not out.counts.any() and not out.hz_counts.any()
    assert out.terminal.min() >= protect[0][T] and out.horizon_terminal.min() >= protect[0][0]


def test_the_ratchet_bounds_the_drawdown(gpu_ctx):
    """theta = 0.9, m = 4, S = 0: V' >= theta M wherever m |rho| < 1, so the worst q is at least theta32 (1 - 2^-22) by monotone
    rounding; the restatement shows m |rho| (1 + 2^-20) < 1 on every sampled step, and every stored q obeys the bound."""
    N, K, T, n = 3, 2, 60, 100_000
    mu, L, W = _market(N, K, 6)
    protect = (np.zeros(T + 1, np.float32), 4.0, 0.0, 1.0, 0.9)
    out = _run(gpu_ctx, _ffi.make_params(N, T, K), protect, mu, L, W, 0, n, drawdown=True)
    ids = _pick(n, 0, 200)
    ref = protect_ref.simulate_protected(mu, L, W, T, SEED, ids.astype(np.uint64), protect)
    assert np.all(4.0 * np.abs(ref["rho"].astype(np.float64)) * (1 + 2.0 ** -20) < 1.0)
    assert np.array_equal(_bits(out.qd[:, ids]), _bits(ref["q"])) and ref["ratchet"].all()
    bound = float(np.float32(0.9)) * (1 - 2.0 ** -22)
    assert out.qd.min() >= bound and out.dd_stats["min"].min() >= bound - 1.0
    free = gpu_ctx.simulate_drawdown(_ffi.make_params(N, T, K), mu, L, W, SEED, 0, n, True)
    assert free[3].min() < bound                              # without protection the same draws fall further


def test_crash_jumps_gap_the_floor_and_the_count_is_the_restatements(gpu_ctx):
    N, K, T, n = 3, 2, 24, 20_000
    mu, L, W = _market(N, K, 8)
    protect = check_protect((0.8, 4.0), T)
    jumps = (0.03, -0.45, 0.0)
    out = gpu_ctx.simulate_protected(_ffi.make_params(N, T, K), protect, mu, L, W, SEED, 0, n, True, jumps=jumps + (None,))
    rho = protect_ref.rho_of(mu, L, W, T, SEED, np.arange(n, dtype=np.uint64), jumps=jumps)
    ref = protect_ref.walk(rho, protect)
    assert np.array_equal(_bits(out.terminal), _bits(ref["V_T"]))
    want = np.count_nonzero(ref["V_T"] < protect[0][T], axis=1)
    assert np.all(out.counts[:, 0] > 0) and np.array_equal(out.counts[:, 0], want.astype(np.uint64)) and not out.counts[:, 1].any()
    calm = _run(gpu_ctx, _ffi.make_params(N, T, K), protect, mu, L, W, 0, n)
    assert not calm.counts.any()


def test_the_law_of_the_terminal_value(gpu_ctx):
    """N = 3, T = 12, 10^6 paths, m = 3, floor 0.8, rf = 0.001, b = 2^20, theta = 0: the assertions of protect_ref.law_checks against
    protect_law, which the binary64 twin passes on the CPU at the same size (test_protect_cpu.py)."""
    n, T = 1_000_000, 12
    mu, cov = synthetic.synthetic_market(3)
    w = np.array([0.2, 0.3, 0.5])
    protect = (0.8, 3.0, RATE, 2.0 ** 20, 0.0)
    mean, var = protect_law(mu, cov, w, T, protect)
    one = simulate_paths(mu, cov, w, n_steps=T, n_paths=n, seed=SEED, protect=protect, store=True, context=gpu_ctx)
    print(protect_ref.law_checks(one["terminal"], mean, var))
    assert one["protect"]["n_gap"] == 0 and one["protect"]["gap_probability"] == 0.0 and one["n"] == n
    assert abs(one["mean"] - (mean - 1.0)) < 5 * one["std"] / np.sqrt(n)
    mu32, _, W32 = prepare_inputs(mu, cov, w)
    piv, _ = _ffi.protect_pivots(_ffi.make_params(3, T, 1), _ffi.make_protect(*check_protect(protect, T)), mu32, W32)
    assert piv[0] == pytest.approx(mean - 1.0, rel=1e-12)


def test_small_terminal_budget_tiles_the_portfolios(gpu_ctx):
    N, K, T = 4, 20, 12
    mu, L, W = _market(N, K, 2)
    prm = _ffi.make_params(N, T, K)
    kw = dict(horizons=[4, 12], levels=(5.0, 95.0), target=0.99)
    want = _run(gpu_ctx, prm, _p1(T), mu, L, W, 0, 10_000, "jumps", **kw)
    c = Context(0, terminal_budget=3 * 3 * 10_000 * 4)
    try:
        got = _run(c, prm, _p1(T), mu, L, W, 0, 10_000, "jumps", **kw)
    finally:
        c.close()
    assert np.array_equal(want.terminal, got.terminal) and np.array_equal(want.horizon_terminal, got.horizon_terminal)
    assert np.array_equal(want.bands, got.bands) and np.array_equal(want.counts, got.counts) and np.array_equal(want.hz_counts, got.hz_counts)
    assert want.counts.any() and want.hz_counts.any()
    for f in ("var", "n_tail", "min", "max"):
        assert np.array_equal(want.stats[f], got.stats[f]) and np.array_equal(want.hz_stats[f], got.hz_stats[f])


def test_two_logical_shards_equal_one(gpu_ctx):
    N, K, T, n = 16, 3, 30, 30_001
    mu, L, W = _market(N, K, 9)
    prm = _ffi.make_params(N, T, K)
    hz = dict(horizons=[10, 30], levels=(50.0,), target=0.99)
    one = _run(gpu_ctx, prm, _p1(T), mu, L, W, 11, n, "t", **hz)
    one_dd = _run(gpu_ctx, prm, _p2(T), mu, L, W, 11, n, "jumps", drawdown=True)
    c = Context((0, 0))
    try:
        sh = _run(c, prm, _p1(T), mu, L, W, 11, n, "t", **hz)
        sd = _run(c, prm, _p2(T), mu, L, W, 11, n, "jumps", drawdown=True)
    finally:
        c.close()
    assert np.array_equal(one.terminal, sh.terminal) and np.array_equal(one.horizon_terminal, sh.horizon_terminal)
    assert np.array_equal(one.bands, sh.bands) and np.array_equal(one.counts, sh.counts) and np.array_equal(one.hz_counts, sh.hz_counts)
    assert one.counts.any()
    for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi", "cvar"):
        assert np.array_equal(one.stats[f], sh.stats[f]) and np.array_equal(one.hz_stats[f], sh.hz_stats[f]), f
    assert np.allclose(one.stats["mean"], sh.stats["mean"], rtol=1e-12) and np.allclose(one.stats["std"], sh.stats["std"], rtol=1e-12)
    assert np.array_equal(one_dd.terminal, sd.terminal) and np.array_equal(one_dd.qd, sd.qd) and np.array_equal(one_dd.counts, sd.counts)
    for f in ("var", "n_tail", "min", "max"):
        assert np.array_equal(one_dd.dd_stats[f], sd.dd_stats[f]), f


def test_refused_call_then_a_correct_one_then_a_gaussian_call(gpu_ctx):
    mu, L, W = _market(16, 3, 1)
    prm = _ffi.make_params(16, 40, 3)
    g0, gt0 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    fresh = Context(0)
    try:
        want = _run(fresh, prm, _p1(40), mu, L, W, 0, 50_000)
    finally:
        fresh.close()
    fn = _ffi.lib().mcp_simulate_protected
    st, cn = np.zeros(3, _ffi.STATS_DTYPE), np.zeros((3, 2), np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    S = _p1(40)[0]
    for bad in (_ffi.make_protect(S, -1.0), _ffi.make_protect(S, 4.0, cap=0.0), _ffi.make_protect(S, 4.0, ratchet=1.0)):
        assert fn(gpu_ctx._h, ctypes.byref(prm), ctypes.byref(bad), None, None, None, vp(mu), vp(L), vp(W), SEED, 0, 50_000, 0, None, 0,
                  None, None, vp(st), None, None, vp(cn), None, None, None, None) == _ffi.MCP_E_ARG
    with pytest.raises(_ffi.McpError):
        _run(gpu_ctx, _ffi.make_params(16, 40, 3, compounding="log"), _p1(40), mu, L, W, 0, 1000, store=False)
    got = _run(gpu_ctx, prm, _p1(40), mu, L, W, 0, 50_000)
    assert np.array_equal(want.terminal, got.terminal) and want.stats.tobytes() == got.stats.tobytes()
    assert np.array_equal(want.counts, got.counts)
    g1, gt1 = gpu_ctx.simulate(prm, mu, L, W, 77, 0, 50_000, True)
    assert np.array_equal(gt0, gt1) and g0.tobytes() == g1.tobytes()


def test_simulate_paths_returns_its_shapes(gpu_ctx):
    mu, cov = synthetic.synthetic_market(3)
    one = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, protect=(0.8, 4.0, RATE), target=1.0, store=True,
                         horizons=[1, 6, 12], bands=(5.0, 95.0), context=gpu_ctx)
    assert one["n"] == 5000 and one["terminal"].shape == (5000,) and one["horizon_terminal"].shape == (3, 5000)
    blk = one["protect"]
    assert blk["floor"].shape == (13,) and blk["n_gap"] == 0 and 0 < blk["n_short"] < 5000 and blk["horizons"]["n_short"].shape == (3,)
    assert blk["n_short"] == np.count_nonzero(one["terminal"] < np.float32(1.0)) and "cashflow" not in one
    dd = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, protect=(0.8, 4.0, RATE, 1.0, 0.9), dof=5, garch=(0.1, 0.85),
                        drawdown=True, store=True, context=gpu_ctx)
    assert isinstance(dd, list) and len(dd) == 3 and dd[0]["max_drawdown"].shape == (5000,) and "protect" in dd[2]
    s, d, c = simulate_paths(mu, cov, np.eye(3), n_steps=12, n_paths=5000, protect=(0.8, 4.0), jumps=(0.03, -0.45, 0.0), drawdown=True,
                             chol=np.linalg.cholesky(cov), as_array=True, context=gpu_ctx)     # chol: the diffusive factor, the jumps on top
    assert s.shape == d.shape == (3,) and c.shape == (3, 2) and c[:, 0].any()
    g = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, store=True, context=gpu_ctx)
    same = simulate_paths(mu, cov, [0.2, 0.3, 0.5], n_steps=12, n_paths=5000, protect=(0.0, 1.0), store=True, context=gpu_ctx)
    assert np.array_equal(g["terminal"], same["terminal"]) and g["var"] == same["var"] and "protect" not in g
    assert one["min"] > g["min"] and one["min"] >= float(blk["floor"][12]) - 1.0


def test_pipeline_prints_the_protection_lines(gpu_ctx):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        mod = runpy.run_path(os.path.join(ROOT, "examples", "pipeline.py"), run_name="pipeline_test")
    finally:
        sys.path.pop(0)
    data = os.path.join(ROOT, "tests", "golden", "data")
    files = [os.path.join(data, f) for f in ("Avalanche Historical Data.csv", "Cardano Historical Data.csv",
                                             "NEAR_USD Binance Historical Data.csv")]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mod["main"](files, n_paths=20_000)
    lines = [l for l in out.getvalue().splitlines() if l.startswith("protection on ")]
    print("\n".join(lines))
    assert len(lines) == 6 and sum("gap probability" in l for l in lines) == 5 and sum("not built" in l for l in lines) == 1
    floors = [l for l in lines if "80 % floor at m = 4" in l]
    assert len(floors) == 2          # the rows' steps are large (m |rho| > 1 happens): here even Gaussian steps gap the floor

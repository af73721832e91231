"""GPU checks of volatility targeting (SPEC.md 4.19 / 5.19): terminal values, the summed exposure Y, the drawdown q and the horizon
rows bit-equal to the NumPy restatement (voltarget_ref.py) over widths, portfolio counts, step counts, a path range across 2^32 and
a second grid-stride tile, on Gaussian, Student-t, GARCH and jump draws, under two input sets that between them reach every branch of
the rule (asserted on the restatement); the exposure record and the counts against NumPy on the stored values; the exact anchors
(a) to (d); the law of a constant exposure at 10^6 paths; tiles and shards."""
import contextlib
import io
import os
import re
import runpy
import sys

import numpy as np
import pytest

import voltarget_ref as ref_
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi, simulate_paths, synthetic, vol_target_law
from monte_carlo_portfolio_amd.simulate import Context, prepare_inputs
from oracle import ref_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x19_CF01
DRAWS = {"gauss": {}, "t": {"dof": 5}, "garch": {"garch": (0.15, 0.8, 1.5)}, "jumps": {"jumps": (0.3, -0.05, 0.04)}}
SETS = {"A": (ref_.SET_A, 0.05), "B": (ref_.SET_B, 0.08)}      # the rule's numbers and the portfolio step volatility of its market


def _set(which, draw):
    """The input set for a draw.  B on Student-t draws aims at 0.65 instead of 0.5: at nu = 5 a step now and then is so large that the
    estimate passes 0.5 on a path that survives it, which lends for one step (6e-5 of the live steps at 0.5, on the restatement), and
    set B is to borrow on every live step; at 0.65 none does, 27-46 % of the paths are ruined and the cap binds on three steps in four."""
    vt, vol = SETS[which]
    return ((0.65,) + vt[1:] if which == "B" and draw == "t" else vt), vol
BIG = 2.0 ** 60


def _market(N, K, vol, seed=0):
    """The synthetic market with its factor scaled so that the portfolios' mean step volatility is `vol`."""
    mu, cov = synthetic.synthetic_market(N)
    W = np.random.default_rng(seed + 31 * N + K).dirichlet(np.ones(N), size=K)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    return mu32, (ref_.scaled_chol(L, W32, vol) if vol else L), W32


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


def _kw(draw):
    kw = dict(DRAWS[draw])
    if "jumps" in kw:
        kw["jumps"] = tuple(float(v) for v in kw["jumps"]) + (None,)
    return kw


def _run(ctx, prm, vt, mu, L, W, begin, n, draw="gauss", store=True, **kw):
    return ctx.simulate_vol_target(prm, vt, mu, L, W, SEED, begin, n, store, **_kw(draw), **kw)


def _hz(T):
    return sorted({1, max(1, T // 2), T})


def _s0(prm, vt, L, W):
    """s0_k as the library uses it, which is the restatement's own sum bit for bit."""
    s0 = _ffi.vol_target_consts(prm, _ffi.make_vol_target(*vt), L, W)[1]
    assert np.array_equal(_bits(s0), _bits(ref_.default_s0(L, W)))
    return s0


def _record_is_numpy(st, values, k, n):
    """A record over x = values - 1 at v0 = 1: var is np.percentile, n, n_tail, min, max exact, the sums to 1e-12."""
    want = ref_stats.path_stats(values)
    assert st[k]["var"] == want["var"] and st[k]["n_tail"] == want["n_tail"]
    assert st[k]["min"] == want["min"] and st[k]["max"] == want["max"] and st[k]["n"] == n
    for f in ("mean", "std", "cvar"):
        assert abs(st[k][f] - want[f]) <= 1e-12 * max(1.0, abs(want[f])), f


CASES = [  # N, K, T, path_begin, n_paths
    (1, 1, 7, 17, 513),
    (16, 1, 60, 17, 257),
    (3, 1, 12, 17, 513),
    (3, 3, 12, (1 << 32) - 200, 513),                    # across a multiple of 2^32
    (13, 8, 12, 17, 513),
    (17, 20, 7, 5, 257),
    (64, 3, 7, 17, 257),
    (1, 1, 2, 3, 8192 * 256 + 257),                      # past the 8192 workgroups of a launch: the second grid-stride tile
]


@pytest.mark.parametrize("draw", list(DRAWS))
@pytest.mark.parametrize("N,K,T,begin,n", CASES)
def test_values_equal_the_restatement(N, K, T, begin, n, draw, gpu_ctx):
    prm = _ffi.make_params(N, T, K)
    ids = np.arange(n) if n <= 513 else _pick(n, begin, 24)
    hz, lv, target = _hz(T), (2.5, 50.0), 0.97
    for which in SETS:
        if which == "B" and T > 12:
            continue
        vt, vol = _set(which, draw)
        mu, L, W = _market(N, K, vol, 3)
        rho = ref_.rho_of(mu, L, W, T, SEED, (begin + ids).astype(np.uint64), **DRAWS[draw])
        ref = ref_.walk(rho, vt, _s0(prm, vt, L, W), horizons=hz)
        ref_.covers(ref, which, T)
        dd = _run(gpu_ctx, prm, vt, mu, L, W, begin, n, draw, drawdown=True, target=target)
        assert np.array_equal(_bits(dd.terminal[:, ids]), _bits(ref["V_T"]))
        assert np.array_equal(_bits(dd.qd[:, ids]), _bits(ref["q"]))
        assert dd.exposure_stats is None and dd.exposure is None
        h = _run(gpu_ctx, prm, vt, mu, L, W, begin, n, draw, horizons=hz, levels=lv, target=target)
        assert np.array_equal(_bits(h.terminal), _bits(dd.terminal))
        assert np.array_equal(_bits(h.exposure[:, ids]), _bits(ref["Y"]))
        assert np.array_equal(_bits(h.horizon_terminal[:, :, ids]), _bits(ref["V_h"]))
        assert np.array_equal(_bits(h.horizon_terminal[-1]), _bits(h.terminal))
        assert np.array_equal(h.counts, dd.counts)
        for k in (0, K - 1):
            _record_is_numpy(dd.stats, dd.terminal[k], k, n)
            _record_is_numpy(h.exposure_stats, h.exposure[k], k, n)
            assert h.exposure_stats[k]["sharpe"] == 0.0
            _record_is_numpy(dd.dd_stats, dd.qd[k], k, n)
            assert dd.counts[k, 0] == np.count_nonzero(dd.terminal[k] == 0) and dd.counts[k, 1] == np.count_nonzero(dd.terminal[k] < np.float32(target))
            for i in range(len(hz)):
                x = x_of(h.horizon_terminal[i, k])
                assert h.hz_stats[i, k]["var"] == np.percentile(x, (1 - 0.95) * 100)
                assert h.hz_stats[i, k]["min"] == x.min() and h.hz_stats[i, k]["max"] == x.max()
                for jj, q in enumerate(lv):
                    assert h.bands[i, k, jj] == np.percentile(x, q)
                assert h.hz_counts[i, k, 0] == np.count_nonzero(h.horizon_terminal[i, k] == 0)
                assert h.hz_counts[i, k, 1] == np.count_nonzero(h.horizon_terminal[i, k] < np.float32(target))
        if which == "B" and T >= 7:
            assert dd.counts[:, 0].any()                  # ruin is counted where the restatement shows it


@pytest.mark.parametrize("N,K,T", [(3, 3, 12), (16, 1, 40), (16, 8, 12), (64, 3, 5)])
def test_anchor_a_cap_one_and_a_far_target_is_the_call_without_targeting(N, K, T, gpu_ctx):
    """b = 1, tgt = 2^60: e = 1, E = V, u = V, D = +0 on every step, so while the values stay positive every stored value is the twin
    call's bit for bit -- values, drawdown, horizon rows, bands, order statistics; mean and std agree to SPEC.md 6's 1e-12 (the pivot
    differs in rounding); Y = T exactly."""
    n, prm = 20_000, _ffi.make_params(N, T, K)
    mu, L, W = _market(N, K, 0, 1)
    hz = _hz(T)
    vt = (BIG, 0.7, 1.0, 0.002, 0.001, None)
    for draw in DRAWS:
        twin = lambda **kw: gpu_ctx._call(prm, W, SEED, 7, n, True, mu=mu, chol=L, **_kw(draw), **kw)   # noqa: E731
        want, got = twin(drawdown=True), _run(gpu_ctx, prm, vt, mu, L, W, 7, n, draw, drawdown=True)
        assert want.terminal.min() > 0
        assert np.array_equal(_bits(got.terminal), _bits(want.terminal)) and np.array_equal(_bits(got.qd), _bits(want.qd))
        assert got.dd_stats.tobytes() == want.dd_stats.tobytes() and not got.counts.any()
        wh, gh = twin(horizons=hz, levels=(5.0, 95.0)), _run(gpu_ctx, prm, vt, mu, L, W, 7, n, draw, horizons=hz, levels=(5.0, 95.0))
        assert np.array_equal(_bits(gh.horizon_terminal), _bits(wh.horizon_terminal)) and np.array_equal(gh.bands, wh.bands)
        assert np.all(gh.exposure == np.float32(T)) and np.all(gh.exposure_stats["min"] == T - 1.0) and np.all(gh.exposure_stats["max"] == T - 1.0)
        for a, b in ((got.stats, want.stats), (gh.stats, wh.stats), (gh.hz_stats, wh.hz_stats)):
            for f in ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max"):
                assert np.array_equal(a[f], b[f]), (draw, f)
            for f in ("mean", "std"):
                assert np.all(np.abs(a[f] - b[f]) <= 1e-12 * np.maximum(1.0, np.abs(b[f]))), (draw, f)
    far = _run(gpu_ctx, prm, ref_.SET_A, mu, L, W, 7, n)
    assert not np.array_equal(_bits(far.terminal), _bits(gpu_ctx._call(prm, W, SEED, 7, n, True, mu=mu, chol=L).terminal))


def test_anchors_c_and_d_the_exposure_is_exact(gpu_ctx):
    """(c) lambda = 1: s stays s0_k, so e = fmin(tgt / sqrt(s0_k), b) on every step and Y is the binary32 sum of T equal terms.
    (d) T = 1: Y = e_0 on every path.  Both with the default s0 and with a given one, on every draw."""
    N, K, n = 5, 9, 3000
    mu, L, W = _market(N, K, 0.05, 2)
    given = np.linspace(1e-3, 4e-3, K)
    for draw in DRAWS:
        for T, lam in ((12, 1.0), (1, 0.7)):
            prm = _ffi.make_params(N, T, K)
            for s0 in (None, given):
                vt = (0.05, lam, 1.2, 0.002, 0.001, s0)
                used = _ffi.vol_target_consts(prm, _ffi.make_vol_target(*vt), L, W)[1]
                assert np.array_equal(used, ref_.default_s0(L, W) if s0 is None else given.astype(np.float32))
                e = np.fmin(np.float32(0.05) / np.sqrt(used), np.float32(1.2)).astype(np.float32)
                want = np.zeros(K, np.float32)
                for _ in range(T):
                    want = (want + e).astype(np.float32)
                out = _run(gpu_ctx, prm, vt, mu, L, W, 11, n, draw)
                assert np.array_equal(_bits(out.exposure), _bits(np.repeat(want[:, None], n, axis=1))), (draw, T, s0 is None)
                if s0 is not None:                        # both sides of the cap among the portfolios
                    assert np.any(e == np.float32(1.2)) and np.any(e < np.float32(1.2))


@pytest.mark.parametrize("cap", [0.5, 2.0])
def test_anchor_b_a_far_target_is_a_constant_mix_and_follows_its_law(cap, gpu_ctx):
    """tgt = 2^60: e = b on every step -- half in cash at b = 0.5, constant leverage at b = 2.  N = 3, T = 12, 10^6 paths: Y = T b
    exactly, and the mean of V_T within 5 standard errors of vol_target_law's (voltarget_ref.law_checks; the variance too)."""
    n, T = 1_000_000, 12
    mu, cov = synthetic.synthetic_market(3)
    w = np.array([0.2, 0.3, 0.5])
    vt = (BIG, 0.7, cap, 0.002, 0.001)
    mean, var = vol_target_law(mu, cov, w, T, vt)
    one = simulate_paths(mu, cov, w, n_steps=T, n_paths=n, seed=SEED, vol_target=vt, store=True, context=gpu_ctx)
    blk = one["vol_target"]
    assert blk["n_ruined"] == 0 and blk["exposure0"] == cap and one["n"] == n
    assert np.all(blk["exposure"]["paths"] == np.float32(T * cap)) and blk["exposure"]["mean"] == cap and blk["exposure"]["min"] == cap
    print(ref_.law_checks(one["terminal"], mean, var))
    mu32, L, W32 = prepare_inputs(mu, cov, w)
    piv, _ = _ffi.vol_target_pivots(_ffi.make_params(3, T, 1), _ffi.make_vol_target(*vt), mu32, L, W32)
    assert piv[0] == pytest.approx(mean - 1.0, rel=1e-12)


def test_two_logical_shards_and_two_tiles_equal_one_call(gpu_ctx):
    """Any partition of the path range and of the portfolios gives the same values, counts and order statistics: two logical shards
    of one device, and a terminal budget that forces two tiles of portfolios."""
    N, K, T, n = 5, 3, 12, 30_001
    vt, vol = SETS["B"]
    mu, L, W = _market(N, K, vol, 9)
    prm = _ffi.make_params(N, T, K)
    hz = dict(horizons=[4, 12], levels=(50.0,), target=0.9)
    one = _run(gpu_ctx, prm, vt, mu, L, W, 11, n, "t", **hz)
    one_dd = _run(gpu_ctx, prm, vt, mu, L, W, 11, n, "jumps", drawdown=True)
    assert one.counts.all() and one.hz_counts.any()
    for make in (lambda: Context((0, 0)), lambda: Context(0, terminal_budget=2 * n * 4 * (1 + 2 + 1))):
        c = make()
        try:
            sh = _run(c, prm, vt, mu, L, W, 11, n, "t", **hz)
            sd = _run(c, prm, vt, mu, L, W, 11, n, "jumps", drawdown=True)
        finally:
            c.close()
        assert np.array_equal(one.terminal, sh.terminal) and np.array_equal(one.horizon_terminal, sh.horizon_terminal)
        assert np.array_equal(one.exposure, sh.exposure)
        assert np.array_equal(one.bands, sh.bands) and np.array_equal(one.counts, sh.counts) and np.array_equal(one.hz_counts, sh.hz_counts)
        for f in ("var", "n_tail", "min", "max", "x_lo", "x_hi", "cvar"):
            assert np.array_equal(one.stats[f], sh.stats[f]) and np.array_equal(one.hz_stats[f], sh.hz_stats[f]), f
            assert np.array_equal(one.exposure_stats[f], sh.exposure_stats[f]), f
        assert np.allclose(one.stats["mean"], sh.stats["mean"], rtol=1e-12) and np.allclose(one.stats["std"], sh.stats["std"], rtol=1e-12)
        assert np.array_equal(one_dd.terminal, sd.terminal) and np.array_equal(one_dd.qd, sd.qd) and np.array_equal(one_dd.counts, sd.counts)
        for f in ("var", "n_tail", "min", "max"):
            assert np.array_equal(one_dd.dd_stats[f], sd.dd_stats[f]), f


def test_public_call_blocks_and_portfolio_shards(gpu_ctx):
    """simulate_paths(vol_target=...): the 'vol_target' block against the stored arrays, with the drawdown and without, and two
    portfolio shards against one call."""
    N, K, T, n = 4, 3, 12, 20_000
    mu, cov = synthetic.synthetic_market(N)
    cov = cov * 16.0                                     # about 0.08 per step
    W = np.random.default_rng(5).dirichlet(np.ones(N), size=K)
    vt = (0.5, 0.7, 8.0, 0.002, 0.001)
    res = simulate_paths(mu, cov, W, n_steps=T, n_paths=n, seed=SEED, vol_target=vt, store=True, target=0.9, horizons=[6, 12], context=gpu_ctx)
    for k, d in enumerate(res):
        blk = d["vol_target"]
        Y = blk["exposure"]["paths"].astype(np.float64)
        assert blk["n_ruined"] == np.count_nonzero(d["terminal"] == 0) > 0 and blk["ruin_probability"] == blk["n_ruined"] / n
        assert blk["n_short"] == np.count_nonzero(d["terminal"] < np.float32(0.9)) and blk["target_value"] == 0.9
        assert blk["exposure"]["min"] == pytest.approx(Y.min() / T, rel=1e-15) and blk["exposure"]["max"] == pytest.approx(Y.max() / T, rel=1e-15)
        assert blk["exposure"]["mean"] == pytest.approx(Y.mean() / T, rel=1e-12)
        assert blk["exposure"]["quantile"] == pytest.approx(np.percentile(Y, 5.0) / T, rel=1e-12)
        assert blk["horizons"]["n_ruined"][1] == blk["n_ruined"] and blk["cap"] == 8.0 and blk["exposure0"] <= 8.0
    dd = simulate_paths(mu, cov, W, n_steps=T, n_paths=n, seed=SEED, vol_target=vt, store=True, drawdown=True, context=gpu_ctx)
    assert "exposure" not in dd[0]["vol_target"] and np.array_equal(dd[1]["terminal"], res[1]["terminal"]) and "max_drawdown" in dd[0]
    c = Context((0, 0))
    try:
        two = simulate_paths(mu, cov, W, n_steps=T, n_paths=n, seed=SEED, vol_target=vt, store=True, target=0.9, horizons=[6, 12], context=c,
                             devices=[0, 0], shard="portfolios")
    finally:
        c.close()
    for a, b in zip(res, two):
        assert np.array_equal(a["terminal"], b["terminal"]) and np.array_equal(a["vol_target"]["exposure"]["paths"], b["vol_target"]["exposure"]["paths"])
        assert a["var"] == b["var"] and a["vol_target"]["n_ruined"] == b["vol_target"]["n_ruined"]


def test_pipeline_prints_the_volatility_target_lines(gpu_ctx):
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
    found = re.findall(r"optimum under the fitted GARCH, (held|volatility target): VaR = ([-+0-9.]+)  CVaR = ([-+0-9.]+)  mean max drawdown = "
                       r"([-+0-9.]+)", out.getvalue())
    assert [f[0] for f in found] == ["held", "volatility target"], out.getvalue()
    cap = re.search(r"\(target ([0-9.]+) per period, cap 1.5, first exposure ([0-9.]+), ruined (\d+) of 20000 paths\)", out.getvalue())
    assert cap and 0.0 < float(cap.group(2)) <= 1.5
    assert all(np.isfinite(float(v)) for f in found for v in f[1:])

"""Downside and shape statistics on the GPU (SPEC.md 5.22).

1. mcp_launch_downside on crafted rows in a torch tensor, against NumPy on mcp_terminal_to_x of the same values (tests/downside_ref.py):
   the counts exactly, every sum within the association bound (n - 1) 2^-53 sum |summand| of math.fsum of NumPy's summands, two launches
   byte for byte.  Rows lie stride = n + 3 apart behind a one-element offset, so that they start at every offset modulo 16 bytes and
   none 16-byte aligned at row 0; everything outside the rows is NaN.  Row kinds cycle: plain; 30 % of the values exactly at tau
   (in neither set); entirely below tau.  Log compounding: the device's expm1 may differ from the host's in the last bit, so no value
   sits at tau there (asserted: none within 1e-12), the bound is widened by 4 * 2^-53 per summand, and the first four values of every
   row are small against their distances to the pivot and to tau, so that at n <= 4, where the association term gives nothing, a last
   bit of x moves d^4 by less than that.
2. The same through simulate_paths / simulate_bootstrap (store=True, N = 3, T = 12, n = 1000): the raw sums against NumPy on the stored
   values, downside.finish of them against the returned record bit for bit, everything else in the result against the call without
   the keyword byte for byte; tiles, logical shards and portfolio shards against the one-shard call; a horizon's record against the
   terminal record of the call that ends there.
3. The normal law at 10^6 paths (tests/test_downside_cpu.py holds a binary64 twin to the same assertions).
"""
import ctypes
import math

import numpy as np
import pytest

import downside_ref as ref_
from monte_carlo_portfolio_amd import _ffi, downside, simulate_bootstrap, simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import Context

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025)
X_TAU = 0.013


def _tau_value(v0, compounding):
    """(the binary32 value whose x is tau, tau): tau is an x the device can meet exactly."""
    v = np.float32(v0 * (1.0 + X_TAU)) if compounding == "simple" else np.float32(math.log1p(X_TAU))
    return v, float(ref_.to_x(np.array([v]), v0, compounding)[0])


def _rows(rows, n, v0, compounding, seed):
    """([rows, n] binary32 values, [rows] pivots, tau)."""
    rng = np.random.default_rng(seed)
    v_tau, tau = _tau_value(v0, compounding)
    pivots = 0.02 + 0.001 * np.arange(rows)
    x = pivots[:, None] + 0.05 * rng.standard_normal((rows, n))
    if compounding == "log":
        x[:, :4] = (0.0005 * (np.arange(4) - 1.5))[None, :n]
    vals = (np.float32(v0) * (1.0 + x)).astype(np.float32) if compounding == "simple" else np.log1p(x).astype(np.float32)
    below = np.nextafter(v_tau, np.float32(-np.inf))
    for r in range(rows):
        kind = (r + rows) % 3
        if kind == 1 and compounding == "simple":
            vals[r, rng.random(n) < 0.3] = v_tau
            if n >= 4:
                vals[r, :3] = v_tau
        elif kind == 2:
            vals[r] = np.minimum(vals[r], below)
    return vals, pivots, tau


def _launch(lib, prm, vals, pivots, tau, offset=1, pad=3, twice=True):
    """mcp_launch_downside over `vals` laid out [rows][n + pad] behind `offset` NaN elements -> [rows] records."""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = vals.shape
    stride = n + pad
    host = np.full(offset + rows * stride + 8, -np.nan, np.float32)
    host[offset:offset + rows * stride].reshape(rows, stride)[:, :n] = vals
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    d_pivot = torch.from_numpy(np.ascontiguousarray(pivots, np.float64)).to(dev) if pivots is not None else None
    partials = torch.full(((lib.mcp_downside_ws_bytes(rows, n) + 7) // 8,), -1, dtype=torch.int64, device=dev)
    sums = torch.full((rows * 12,), -1, dtype=torch.int64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = []
    for _ in range(2 if twice else 1):
        _ffi.check(lib.mcp_launch_downside(ctypes.byref(prm), ctypes.c_void_p(buf.data_ptr() + 4 * offset), stride, n, rows,
                                           ctypes.c_void_p(d_pivot.data_ptr()) if d_pivot is not None else None, tau,
                                           ctypes.c_void_p(partials.data_ptr()), ctypes.c_void_p(sums.data_ptr()), st))
        out.append(sums.cpu().numpy().copy())
        sums.fill_(-1)
    if twice:
        assert np.array_equal(out[0], out[1]), "two launches differ"
    return out[0].view(_ffi.DOWNSIDE_SUMS_DTYPE)


@pytest.mark.parametrize("compounding", ["simple", "log"])
@pytest.mark.parametrize("v0", [1.0, 0.25, 1e4])
@pytest.mark.parametrize("rows", [1, 3, 9, 17])
def test_launch_on_crafted_rows(gpu_ctx, rows, v0, compounding):
    lib = _ffi.lib()
    prm = _ffi.make_params(1, 1, 1, compounding, v0)
    for n in NS:
        vals, pivots, tau = _rows(rows, n, v0, compounding, 1000 * rows + n)
        if rows == 9:
            pivots = None                                   # a NULL d_pivot: c = 0
        got = _launch(lib, prm, vals, pivots, tau)
        x = ref_.to_x(vals, v0, compounding)
        if compounding == "log":
            assert np.min(np.abs(x - tau)) > 1e-12
        for r in range(rows):
            ref_.check_record(got[r], x[r], 0.0 if pivots is None else pivots[r], tau, 4 * ref_.U if compounding == "log" else 0.0,
                              f"rows={rows} v0={v0} {compounding} n={n} r={r}")
            kind = (r + rows) % 3
            if kind == 2:
                assert int(got[r]["n_below"]) == n and int(got[r]["n_above"]) == 0
            if kind == 1 and compounding == "simple" and n >= 4:
                assert int(got[r]["n_below"]) + int(got[r]["n_above"]) <= n - 3


def test_launch_across_the_second_grid_stride_trip(gpu_ctx):
    """The sizes around the one the library names: the last n of one trip, the first of two (a 16-byte aligned row), and three more
    values behind a one-element offset, where head and tail scalars frame the vector body; two rows, so that blockIdx.y moves."""
    lib = _ffi.lib()
    trip = lib.mcp_downside_trip_n()
    assert lib.mcp_downside_grid(trip) == lib.mcp_downside_grid(10 * trip)
    prm = _ffi.make_params(1, 1, 1, "simple", 1.0)
    for n, offset, rows in ((trip - 4, 0, 1), (trip, 0, 1), (trip + 3, 1, 2)):
        vals, pivots, tau = _rows(rows, n, 1.0, "simple", n)
        got = _launch(lib, prm, vals, pivots, tau, offset=offset, pad=5 if offset else 0)
        x = ref_.to_x(vals, 1.0, "simple")
        for r in range(rows):
            ref_.check_record(got[r], x[r], pivots[r], tau, 0.0, f"trip n={n} r={r}")


# ---- 2. through the call ---------------------------------------------------------------------------------------------------------------

N_ASSETS, T, PATHS, SEED = 3, 12, 1000, 20260
TAU = 0.004


def _market(K):
    mu, cov = synthetic.synthetic_market(N_ASSETS)
    W = synthetic.dirichlet_weights(N_ASSETS, K) if K > 1 else np.full(N_ASSETS, 1.0 / N_ASSETS)
    return mu, cov, W


def _same(a, b, where=""):
    """Two results equal byte for byte: dicts key by key, arrays by their bytes, floats by their bits (NaN included)."""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for k in a:
            _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (p, q) in enumerate(zip(a, b)):
            _same(p, q, f"{where}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), where
    else:
        assert a == b, where


def _scale(f, want):
    """What 1e-10 is relative to when two records of the same values differ by association alone ((n - 1) 2^-53 = 1.1e-13 of every
    sum's mass at n = 1000): the figure itself -- except the two shape figures, which pass through zero while the masses behind them,
    E|z|^3 = 1.6 and E z^4 = 3 in units of sigma, do not."""
    return max(abs(want), 1.0) if f in ("skewness", "excess_kurtosis") else abs(want)


def _check_call(res, plain, tau, horizons=None, compounding="simple"):
    """One result with the keyword against the same call without it and against NumPy on the stored values -> the list of dicts."""
    res, plain = (r if isinstance(r, list) else [r] for r in (res, plain))
    for k, (d, p) in enumerate(zip(res, plain)):
        blk = d["downside"]
        _same({key: v for key, v in d.items() if key != "downside"}, p, f"portfolio {k}")
        assert blk["threshold"] == tau
        x = ref_.to_x(d["terminal"], 1.0, compounding)
        sums = np.zeros((), _ffi.DOWNSIDE_SUMS_DTYPE)
        for f in downside.SUM_FIELDS:
            sums[f] = blk["sums"][f]
        ref_.check_record(sums, x, blk["pivot"], tau, 4 * ref_.U if compounding == "log" else 0.0, f"call k={k}")
        again = downside.finish(blk["sums"], tau, blk["pivot"])
        for f in downside.STAT_FIELDS:
            assert np.float64(again[f]).tobytes() == np.float64(blk[f]).tobytes(), (k, f, again[f], blk[f])
        assert abs(blk["mean"] - d["mean"]) <= 1e-12 * max(1.0, abs(d["mean"]))
        if horizons is not None:
            assert len(blk["horizons"]) == len(horizons)
            for h, hb in enumerate(blk["horizons"]):
                xh = ref_.to_x(d["horizon_terminal"][h], 1.0, compounding)
                assert hb["p_below"] == np.mean(xh < tau) and hb["threshold"] == tau
                want = _ffi.downside_finish(ref_.raw_record(xh, hb["pivot"], tau), tau, hb["pivot"])
                for f in ("sortino", "downside_deviation", "skewness", "excess_kurtosis", "omega", "mean"):
                    assert abs(hb[f] - want[f]) <= 1e-10 * _scale(f, want[f]), (k, h, f, hb[f], want[f])
        else:
            assert "horizons" not in blk
    return res


CALLS = {
    "K = 1, the lean kernel": (1, {}),
    "K = 8": (8, {}),
    "K = 20 in passes, horizons": (20, dict(horizons=(1, 5, 12))),
    "dof = 5": (2, dict(dof=5)),
    "drawdown": (3, dict(drawdown=True)),
    "antithetic": (3, dict(antithetic=True)),
    "K = 17, the sweep kernel": (17, {}),
    "log compounding": (2, dict(compounding="log")),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_keyword_through_simulate_paths(gpu_ctx, name):
    K, kw = CALLS[name]
    mu, cov, W = _market(K)
    base = dict(n_steps=T, n_paths=PATHS, seed=SEED, store=True, context=gpu_ctx, **kw)
    with_kw = simulate_paths(mu, cov, W, downside=TAU, **base)
    plain = simulate_paths(mu, cov, W, **base)
    res = _check_call(with_kw, plain, TAU, kw.get("horizons"), kw.get("compounding", "simple"))
    assert len(res) == K
    plain_again = simulate_paths(mu, cov, W, **base)        # the request is spent: the next call is the plain one
    assert "downside" not in (plain_again if isinstance(plain_again, dict) else plain_again[0])


def test_the_keyword_through_simulate_bootstrap_and_true_means_rf(gpu_ctx):
    rng = np.random.default_rng(4)
    rows = 0.004 + 0.03 * rng.standard_normal((120, N_ASSETS))
    W = synthetic.dirichlet_weights(N_ASSETS, 2)
    base = dict(n_steps=T, n_paths=PATHS, seed=SEED, store=True, context=gpu_ctx, rf=0.0025)
    res = _check_call(simulate_bootstrap(rows, W, downside=True, **base), simulate_bootstrap(rows, W, **base), 0.0025)
    assert res[0]["downside"]["threshold"] == 0.0025
    mu, cov, W1 = _market(1)
    d = simulate_paths(mu, cov, W1, n_steps=T, n_paths=PATHS, seed=SEED, store=True, context=gpu_ctx, rf=0.0025, downside=True)
    assert d["downside"]["threshold"] == 0.0025 and abs(d["downside"]["sortino"] - (d["mean"] - 0.0025) / d["downside"]["downside_std"]) < 1e-12


def test_a_failing_call_spends_the_request(gpu_ctx):
    """Armed, a call that fails once it has taken the request, then a plain call: the plain call writes nothing into the request's
    arrays.  A call refused by its own argument rules never reaches the context and leaves the request for the next call."""
    lib = _ffi.lib()
    mu, cov, W = _market(2)
    stats, sums = np.zeros(2, _ffi.DOWNSIDE_STATS_DTYPE), np.zeros(2, _ffi.DOWNSIDE_SUMS_DTYPE)
    hz = np.zeros((1, 2), _ffi.DOWNSIDE_STATS_DTYPE)
    req = _ffi.McpDownside(0.0, 0, 0)
    _ffi.check(lib.mcp_ctx_request_downside(gpu_ctx._h, ctypes.byref(req), _ffi.ptr(sums), _ffi.ptr(stats), _ffi.ptr(hz)))
    with pytest.raises(_ffi.McpError, match="no horizons"):  # hz_stats_out with a call that has none: refused before it walks
        simulate_paths(mu, cov, W, n_steps=T, n_paths=PATHS, seed=SEED, context=gpu_ctx)
    simulate_paths(mu, cov, W, n_steps=T, n_paths=PATHS, seed=SEED, context=gpu_ctx)
    assert not stats.view(np.uint8).any() and not sums.view(np.uint8).any() and not hz.view(np.uint8).any()
    _ffi.check(lib.mcp_ctx_request_downside(gpu_ctx._h, ctypes.byref(req), _ffi.ptr(sums), _ffi.ptr(stats), None))
    from monte_carlo_portfolio_amd.simulate import prepare_inputs
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    with pytest.raises(_ffi.McpError):                       # refused by the call's own rules (n_steps < 0), before the context is looked at:
        gpu_ctx.simulate(_ffi.make_params(N_ASSETS, -1, 2), mu32, L, W32, SEED, 0, PATHS, False)
    assert not stats.view(np.uint8).any()                    # the request stays, and the next call that walks paths takes it
    simulate_paths(mu, cov, W, n_steps=T, n_paths=PATHS, seed=SEED, context=gpu_ctx)
    assert list(sums["n"]) == [PATHS, PATHS] and np.all(stats["p_below"] > 0) and stats["pivot"].all()
    stats[:], sums[:] = 0, 0
    simulate_paths(mu, cov, W, n_steps=T, n_paths=PATHS, seed=SEED, context=gpu_ctx)
    assert not stats.view(np.uint8).any() and not sums.view(np.uint8).any()
    _ffi.check(lib.mcp_ctx_request_downside(gpu_ctx._h, ctypes.byref(req), _ffi.ptr(sums), _ffi.ptr(stats), None))
    _ffi.check(lib.mcp_ctx_request_downside(gpu_ctx._h, None, None, None, None))     # withdrawn
    simulate_paths(mu, cov, W, n_steps=T, n_paths=PATHS, seed=SEED, context=gpu_ctx)
    assert not stats.view(np.uint8).any() and not sums.view(np.uint8).any()


def _records(res):
    out = []
    for d in res if isinstance(res, list) else [res]:
        rec = np.zeros((), _ffi.DOWNSIDE_SUMS_DTYPE)
        for f in downside.SUM_FIELDS:
            rec[f] = d["downside"]["sums"][f]
        out.append(rec)
    return out


@pytest.mark.parametrize("partition", ["tiles", "two logical shards", "three logical shards, antithetic", "portfolio shards"])
def test_partitions_count_exactly_and_sum_to_association(gpu_ctx, partition):
    K = 8
    mu, cov, W = _market(K)
    kw = dict(n_steps=T, n_paths=PATHS, seed=SEED, store=True, horizons=(3, 12), downside=TAU)
    extra = {}
    if partition == "tiles":
        ctx = Context(0, terminal_budget=2 * PATHS * 4 * 3)     # 4 bytes per value, terminal and two horizon rows: two portfolios per tile
    elif partition == "two logical shards":
        ctx = Context((0, 0))
    elif partition == "three logical shards, antithetic":
        ctx = Context((0, 0, 0))
        kw["antithetic"] = True
    else:
        ctx = Context((0, 0))
        extra = dict(devices=[0, 0], shard="portfolios")
    try:
        one = simulate_paths(mu, cov, W, context=gpu_ctx, **kw)
        got = simulate_paths(mu, cov, W, context=ctx, **kw, **extra)
    finally:
        ctx.close()
    for k, (a, b, da, db) in enumerate(zip(_records(one), _records(got), one, got)):
        assert da["terminal"].tobytes() == db["terminal"].tobytes()
        x = ref_.to_x(da["terminal"])
        assert da["downside"]["pivot"] == db["downside"]["pivot"]
        ref_.check_record(b, x, db["downside"]["pivot"], TAU, 0.0, f"{partition} k={k}")
        ref_.same_to_association(a, b, x, da["downside"]["pivot"], TAU, f"{partition} k={k}")
        for h in range(2):
            assert da["downside"]["horizons"][h]["p_below"] == db["downside"]["horizons"][h]["p_below"]
            assert abs(da["downside"]["horizons"][h]["sortino"] - db["downside"]["horizons"][h]["sortino"]) <= 1e-10 * abs(da["downside"]["horizons"][h]["sortino"])


def test_a_horizons_record_is_the_terminal_record_of_the_call_that_ends_there(gpu_ctx):
    K = 3
    mu, cov, W = _market(K)
    full = simulate_paths(mu, cov, W, n_steps=T, n_paths=PATHS, seed=SEED, store=True, horizons=(1, 5, 12), downside=TAU, context=gpu_ctx)
    for h, steps in enumerate((1, 5, 12)):
        short = simulate_paths(mu, cov, W, n_steps=steps, n_paths=PATHS, seed=SEED, store=True, downside=TAU, context=gpu_ctx)
        for k in range(K):
            assert full[k]["horizon_terminal"][h].tobytes() == short[k]["terminal"].tobytes()
            hb, tb = full[k]["downside"]["horizons"][h], short[k]["downside"]
            assert hb["p_below"] == tb["p_below"] and hb["pivot"] == tb["pivot"]          # the counts to the bit
            for f in ("mean", "sortino", "downside_std", "downside_deviation", "sortino_target", "mean_shortfall", "omega", "skewness",
                      "excess_kurtosis"):
                assert abs(hb[f] - tb[f]) <= 1e-10 * _scale(f, tb[f]), (steps, k, f, hb[f], tb[f])


# ---- 3. the law -------------------------------------------------------------------------------------------------------------------------

def test_the_normal_law_at_a_million_paths(gpu_ctx):
    """N = 1, T = 1, Gaussian draws, tau = the pivot: x = mu + sigma z is normal up to binary32 rounding."""
    n, sigma = 1_000_000, 0.04
    mu, cov, w = np.array([0.01]), np.array([[sigma * sigma]]), np.array([1.0])
    prm = _ffi.make_params(1, 1, 1)
    pivot = float(_ffi.pivots(prm, np.array([0.01], np.float32), np.array([[sigma]], np.float32), np.array([[1.0]], np.float32))[0])
    d = simulate_paths(mu, cov, w, n_steps=1, n_paths=n, seed=SEED, downside=pivot, context=gpu_ctx)
    blk = d["downside"]
    assert blk["pivot"] == pivot and blk["sums"]["n"] == n
    ref_.law_assertions(blk, float(np.float32(sigma)), n, "gpu")
    t = simulate_paths(mu, cov, w, n_steps=1, n_paths=n, seed=SEED, downside=pivot, dof=10, context=gpu_ctx)
    print("dof = 10 excess kurtosis", t["downside"]["excess_kurtosis"])
    assert t["downside"]["excess_kurtosis"] > 5 * math.sqrt(24.0 / n)

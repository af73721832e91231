"""Benchmark-relative statistics on the GPU (SPEC.md 5.23).

1. mcp_launch_relative on crafted rows in a torch tensor, against NumPy on mcp_terminal_to_x of the same values (tests/relative_ref.py):
   the counts exactly, every sum within the association bound (n - 1) 2^-53 sum |summand| of math.fsum of NumPy's summands, Y against
   fl32(1 + a), two launches byte for byte.  Rows lie stride = n + pad apart behind a leading offset; every pad in 0..3 is crossed with
   both offsets, so that (k - bench) stride mod 4 takes every residue and neither, one or both rows of a pair are 16-byte aligned; the
   Y array has a leading offset of its own.  Everything outside the live values is NaN, and NaN stays out of every word.  Row kinds
   cycle: plain; 30 % of the paths carrying the benchmark's own stored value (ties, in neither set); every path behind the benchmark;
   the benchmark itself has values of both signs and some exactly at x_b = 0.  Log compounding: the device's expm1 may differ from the
   host's in the last bit, so the bound is widened by 4 * 2^-53 per summand, no |a| lies within 1e-12 of 0 unless the stored values
   are equal, and the first four paths of every row carry one stored value, so that at n <= 4, where the association term gives
   nothing, a = 0 exactly.
2. The same across the second grid-stride trip.
3. Through simulate_paths / simulate_bootstrap / simulate_filtered (store=True, N = 3, T = 12, n = 1000, K = 5).
4. The refusals that reach the library, and the request's lifetime.
5. The one-step law at 10^6 paths (tests/test_relative_cpu.py holds a binary64 twin to the same assertions).
"""
import ctypes

import numpy as np
import pytest

import relative_ref as ref_
from monte_carlo_portfolio_amd import _ffi, filter_rows, relative, simulate_bootstrap, simulate_filtered, simulate_paths, spending_rule, synthetic
from monte_carlo_portfolio_amd.simulate import Context

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)
POISON = np.float32(-7.5)


def _bench_of(r, group, bench):
    return r // group * group + bench


def _rows(rows, n, group, bench, v0, compounding, seed):
    """([rows, n] binary32 values, [rows] pivots): the benchmark rows first, then every row's kind against its benchmark."""
    rng = np.random.default_rng(seed)
    pivots = 0.02 + 0.001 * np.arange(rows)
    x = 0.01 + 0.05 * rng.standard_normal((rows, n))
    if compounding == "log":
        x[:, :4] = (0.0005 * (np.arange(4) - 1.5))[None, :n]
    vals = (np.float32(v0) * (1.0 + x)).astype(np.float32) if compounding == "simple" else np.log1p(x).astype(np.float32)
    zero = np.float32(v0) if compounding == "simple" else np.float32(0.0)     # the stored value whose x is exactly 0
    first = 4 if compounding == "log" else 0
    for g0 in range(0, rows, group):
        rb = g0 + bench
        at_zero = rng.random(n) < 0.1
        at_zero[:first] = False
        vals[rb, at_zero] = zero
        if n > 6:
            vals[rb, 5] = zero
        for r in range(g0, g0 + group):
            kind = (r + rows) % 3
            if r == rb:
                continue
            if kind == 1:
                ties = rng.random(n) < 0.3
                ties[:3] = n >= 4
                vals[r, ties] = vals[rb, ties]
            elif kind == 2:
                below = np.nextafter(vals[rb], np.float32(-np.inf))
                if compounding == "log":                    # next to a stored value near 0 lies an |a| below 1e-12: step clear of it
                    below = vals[rb] - np.float32(1e-4)
                behind = np.minimum(vals[r], below)
                vals[r, first:] = behind[first:]
    return vals, pivots


def _device_buffers(lib, vals, offset, pad, y_offset):
    import torch
    dev = torch.device("cuda", 0)
    rows, n = vals.shape
    stride = n + pad
    host = np.full(offset + rows * stride + 8, -np.nan, np.float32)
    host[offset:offset + rows * stride].reshape(rows, stride)[:, :n] = vals
    buf = torch.from_numpy(host).to(dev)
    ybuf = torch.full((y_offset + rows * stride + 8,), float("nan"), dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0 and ybuf.data_ptr() % 16 == 0
    partials = torch.full(((lib.mcp_relative_ws_bytes(rows, n) + 7) // 8,), -1, dtype=torch.int64, device=dev)
    sums = torch.full((rows * 18,), -1, dtype=torch.int64, device=dev)
    return dev, buf, ybuf, partials, sums, stride


def _launch(lib, prm, vals, pivots, group, bench, offset=1, pad=3, y_offset=0, twice=True, active=True):
    """mcp_launch_relative over `vals` laid out [rows][n + pad] behind `offset` NaN elements -> ([rows] records, [rows, n] Y or None).
    Asserts that nothing outside the live Y values was written."""
    import torch
    rows, n = vals.shape
    dev, buf, ybuf, partials, sums, stride = _device_buffers(lib, vals, offset, pad, y_offset)
    if not active:
        ybuf.fill_(float(POISON))
    d_pivot = torch.from_numpy(np.ascontiguousarray(pivots, np.float64)).to(dev) if pivots is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out, ys = [], []
    for _ in range(2 if twice else 1):
        _ffi.check(lib.mcp_launch_relative(ctypes.byref(prm), ctypes.c_void_p(buf.data_ptr() + 4 * offset), stride, n, rows, group, bench,
                                           ctypes.c_void_p(d_pivot.data_ptr()) if d_pivot is not None else None,
                                           ctypes.c_void_p(partials.data_ptr()), ctypes.c_void_p(sums.data_ptr()),
                                           ctypes.c_void_p(ybuf.data_ptr() + 4 * y_offset) if active else None, st))
        out.append(sums.cpu().numpy().copy())
        ys.append(ybuf.cpu().numpy().copy())
        sums.fill_(-1)
    if twice:
        assert np.array_equal(out[0], out[1]) and ys[0].tobytes() == ys[1].tobytes(), "two launches differ"
    y = ys[0]
    if not active:
        assert np.all(y == POISON), "a NULL d_active wrote something"
        return out[0].view(_ffi.RELATIVE_SUMS_DTYPE), None
    live = np.zeros(y.size, bool)
    live[y_offset:y_offset + rows * stride].reshape(rows, stride)[:, :n] = True
    assert np.all(np.isnan(y[~live])) and not np.any(np.isnan(y[live])), "Y outside the live values, or NaN inside"
    return out[0].view(_ffi.RELATIVE_SUMS_DTYPE), y[y_offset:y_offset + rows * stride].reshape(rows, stride)[:, :n]


def _check_launch(lib, prm, rows, n, group, bench, v0, compounding, layouts, note):
    vals, pivots = _rows(rows, n, group, bench, v0, compounding, 1000 * rows + 10 * n + bench)
    if rows == 3:
        pivots = None                                       # a NULL d_pivot: c = 0
    c = np.zeros(rows) if pivots is None else pivots
    x = ref_.to_x(vals, v0, compounding)
    rbs = [_bench_of(r, group, bench) for r in range(rows)]
    want = [ref_.exact(x[r], x[rbs[r]], c[r], c[rbs[r]]) for r in range(rows)]          # once per pair of rows, for every layout
    a = np.stack([x[r] - x[rbs[r]] for r in range(rows)])
    y_want = (1.0 + a).astype(np.float32)
    if compounding == "log":
        equal = np.stack([vals[r] == vals[rbs[r]] for r in range(rows)])
        assert np.all((np.abs(a) > 1e-12) | equal)
    widen = 4 * ref_.U if compounding == "log" else 0.0
    for i, (offset, pad) in enumerate(layouts):
        y_offset = (offset + i // 2) % 2                    # Y's own alignment: with the values' and against it
        got, y = _launch(lib, prm, vals, pivots, group, bench, offset=offset, pad=pad, y_offset=y_offset)
        for r in range(rows):
            where = f"{note} n={n} bench={bench} offset={offset} pad={pad} r={r}"
            ref_.check_against(got[r], want[r], widen, where, quiet=i > 0)
            kind = (r + rows) % 3
            first = min(n, 4) if compounding == "log" else 0
            if r == rbs[r]:
                assert int(got[r]["n_under"]) == 0 == int(got[r]["n_over"]) and float(got[r]["e2"]) == 0.0
                assert int(got[r]["n_up"]) + int(got[r]["n_down"]) < n or n <= 6
            elif kind == 2:
                assert int(got[r]["n_under"]) == n - first and int(got[r]["n_over"]) == 0, where
            elif kind == 1 and n >= 4:
                assert int(got[r]["n_under"]) + int(got[r]["n_over"]) <= n - 3, where
        if compounding == "simple":
            assert y.tobytes() == y_want.tobytes(), f"{note} n={n} offset={offset} pad={pad}: Y differs from fl32(1 + a)"
        else:
            assert np.all(np.abs(y.astype(np.float64) - y_want) <= np.spacing(np.abs(y_want))), f"{note} n={n} offset={offset} pad={pad}"
    return vals, pivots, want


LAYOUTS = [(offset, pad) for pad in (0, 1, 2, 3) for offset in (0, 1)]


@pytest.mark.parametrize("compounding", ["simple", "log"])
@pytest.mark.parametrize("v0", [1.0, 0.25, 1e4])
@pytest.mark.parametrize("rows", [1, 3, 9])
def test_launch_on_crafted_rows(gpu_ctx, rows, v0, compounding):
    lib = _ffi.lib()
    prm = _ffi.make_params(1, 1, 1, compounding, v0)
    for n in NS:
        for bench in sorted({0, rows // 2, rows - 1}):
            _check_launch(lib, prm, rows, n, rows, bench, v0, compounding, LAYOUTS, f"rows={rows} v0={v0} {compounding}")


def test_launch_in_three_groups_of_three_and_without_the_active_array(gpu_ctx):
    lib = _ffi.lib()
    prm = _ffi.make_params(1, 1, 1, "simple", 1.0)
    for n in (5, 257, 1025):
        vals, pivots, want = _check_launch(lib, prm, 9, n, 3, 1, 1.0, "simple", LAYOUTS[2:6], "groups of 3")
        got, y = _launch(lib, prm, vals, pivots, 3, 1, offset=1, pad=1, active=False)      # NULL d_active: the poison stays
        assert y is None
        for r in range(9):
            ref_.check_against(got[r], want[r], 0.0, f"NULL d_active n={n} r={r}", quiet=True)


def test_launch_across_the_second_grid_stride_trip(gpu_ctx):
    """The sizes around the one the library names: the last n of one trip, the first of two (16-byte aligned rows), and three more
    values behind a one-element offset at pad 1, where head and tail scalars frame the vector body and the two rows differ in alignment;
    two rows against the second, so that blockIdx.y moves and the benchmark lies behind its row."""
    lib = _ffi.lib()
    trip = lib.mcp_relative_trip_n()
    assert lib.mcp_relative_grid(trip) == lib.mcp_relative_grid(10 * trip) and trip == lib.mcp_downside_trip_n()
    prm = _ffi.make_params(1, 1, 1, "simple", 1.0)
    for n, offset, pad in ((trip - 4, 0, 0), (trip, 0, 0), (trip + 3, 1, 1)):
        vals, pivots = _rows(2, n, 2, 1, 1.0, "simple", n)
        x = ref_.to_x(vals, 1.0, "simple")
        got, y = _launch(lib, prm, vals, pivots, 2, 1, offset=offset, pad=pad, y_offset=offset, twice=False)
        for r in range(2):
            ref_.check_record(got[r], x[r], x[1], pivots[r], pivots[1], 0.0, f"trip n={n} r={r}")
        assert y.tobytes() == (1.0 + (x - x[1])).astype(np.float32).tobytes()


# ---- 3. through the call ---------------------------------------------------------------------------------------------------------------

N_ASSETS, T, PATHS, SEED, K5 = 3, 12, 1000, 20261, 5
Q_ALPHA = (1 - 0.95) * 100          # the library's percentile level of VaR at alpha = 0.95, as tests/test_gpu_band.py has it


def _market(K):
    mu, cov = synthetic.synthetic_market(N_ASSETS)
    return mu, cov, synthetic.dirichlet_weights(N_ASSETS, K)


def _same(a, b, where=""):
    """Two results equal byte for byte: dicts key by key, arrays by their bytes, floats by their bits (NaN included)."""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), (where, sorted(a), sorted(b))
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


def _check_active(act, note):
    """The 'active' record against NumPy on the stored Y, at the tolerances of the turnover record's test (tests/test_gpu_band.py)."""
    y = act["y"].astype(np.float64) - 1.0
    print(f"{note}: active mean {act['mean']!r} numpy {y.mean()!r}  std {act['std']!r} numpy {y.std(ddof=1)!r}  var {act['var']!r}")
    assert act["var"] == np.percentile(y, Q_ALPHA) and act["worst"] == y.min() and act["best"] == y.max(), note
    assert act["n_tail"] == int(np.sum(y <= act["var"])), note
    tail = y[y <= act["var"]]
    assert abs(act["cvar"] - tail.mean()) <= 1e-12 * abs(tail.mean()), note
    assert abs(act["mean"] - y.mean()) <= 1e-12 * abs(y.mean()) and abs(act["std"] - y.std(ddof=1)) <= 1e-12 * max(1e-3, y.std(ddof=1)), note


def _check_call(res, plain, bench, horizons=None, compounding="simple", v0=1.0):
    """One result with the keyword against the same call without it and against NumPy on the stored values -> the list of dicts."""
    assert isinstance(res, list) and len(res) == len(plain)
    xs = [ref_.to_x(d["terminal"], v0, compounding) for d in res]
    for k, (d, p) in enumerate(zip(res, plain)):
        blk = d["relative"]
        _same({key: v for key, v in d.items() if key != "relative"}, p, f"portfolio {k}")
        assert blk["benchmark"] == bench and blk["bench_pivot"] == res[bench]["relative"]["pivot"]
        ref_.check_record(ref_.record_of(blk), xs[k], xs[bench], blk["pivot"], blk["bench_pivot"], 4 * ref_.U if compounding == "log" else 0.0,
                          f"call k={k} bench={bench}", quiet=k > 1)
        again = relative.finish(blk["sums"], blk["pivot"], blk["bench_pivot"])
        for f in relative.STAT_FIELDS:
            assert np.float64(again[f]).tobytes() == np.float64(blk[f]).tobytes(), (k, f, again[f], blk[f])
        a = xs[k] - xs[bench]
        if compounding == "simple":
            assert blk["active"]["y"].tobytes() == (1.0 + a).astype(np.float32).tobytes(), k
        _check_active(blk["active"], f"k={k} bench={bench}")
        assert abs(blk["active_mean"] - a.mean()) <= 1e-12 and abs(blk["tracking_error"] - a.std(ddof=1)) <= 1e-12
        if k == bench:
            assert blk["tracking_error"] == 0.0 == blk["information_ratio"] and blk["beta"] == 1.0 == blk["correlation"]
            assert blk["up_capture"] == (1.0 if blk["sums"]["n_up"] else 0.0) and blk["down_capture"] == (1.0 if blk["sums"]["n_down"] else 0.0)
            assert blk["active"]["worst"] == 0.0 == blk["active"]["best"]
        else:
            assert abs(blk["beta"] - np.cov(xs[k], xs[bench])[0, 1] / xs[bench].var(ddof=1)) <= 1e-9
            assert abs(blk["correlation"] - np.corrcoef(xs[k], xs[bench])[0, 1]) <= 1e-9
        if horizons is not None:
            assert len(blk["horizons"]) == len(horizons)
            for h, hb in enumerate(blk["horizons"]):
                xk, xb = (ref_.to_x(res[i]["horizon_terminal"][h], v0, compounding) for i in (k, bench))
                assert hb["p_under"] == np.mean(xk - xb < 0) and hb["benchmark"] == bench
                assert hb["bench_pivot"] == res[bench]["relative"]["horizons"][h]["pivot"]
                want = _ffi.relative_finish(ref_.raw_record(xk, xb, hb["pivot"], hb["bench_pivot"]), hb["pivot"], hb["bench_pivot"])
                for f in ("active_mean", "tracking_error", "information_ratio", "beta", "alpha", "correlation", "up_capture", "down_capture",
                          "mean_underperformance", "relative_downside_deviation"):
                    assert abs(hb[f] - want[f]) <= 1e-10 * max(abs(want[f]), 1e-3), (k, h, f, hb[f], want[f])
        else:
            assert "horizons" not in blk
    return res


def _boot_rows():
    return 0.004 + 0.03 * np.random.default_rng(4).standard_normal((120, N_ASSETS))


CALLS = {
    "plain": (simulate_paths, {}),
    "log compounding": (simulate_paths, dict(compounding="log")),
    "drawdown": (simulate_paths, dict(drawdown=True)),
    "horizons": (simulate_paths, dict(horizons=(1, 5, 12))),
    "student-t": (simulate_paths, dict(dof=5)),
    "garch": (simulate_paths, dict(garch=(0.1, 0.85))),
    "cashflow": (simulate_paths, dict(cashflow=-0.01, target=0.9)),
    "glide": (simulate_paths, dict(glide=([6], np.tile([[[0.6, 0.2, 0.2]]], (5, 1, 1))))),
    "spending": (simulate_paths, dict(spending=spending_rule("constant", 0.01, every=4, inflation=0.02))),
    "banded": (simulate_paths, dict(tolerance=0.02, rebalance=3)),
    "vol-target": (simulate_paths, dict(vol_target=(0.1, 0.9))),
    "antithetic": (simulate_paths, dict(antithetic=True)),
    "bootstrap": (simulate_bootstrap, dict(block=3.0)),
    "filtered": (simulate_filtered, {}),
}
SECOND = {"drawdown": "drawdown", "banded": "tolerance", "spending": "spending"}


def _call(name, W, **more):
    fn, kw = CALLS[name]
    base = dict(n_steps=T, n_paths=PATHS, seed=SEED, store=True, **kw, **more)
    if fn is simulate_paths:
        mu, cov, _ = _market(2)
        return fn(mu, cov, W, **base)
    if fn is simulate_bootstrap:
        return fn(_boot_rows(), W, **base)
    return fn(filter_rows(_boot_rows(), (0.10, 0.85)), W, **base)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_keyword_through_every_kind_of_call(gpu_ctx, name):
    W = _market(K5)[2]
    plain = _call(name, W, context=gpu_ctx)
    for bench in (0, 2, 4):
        res = _call(name, W, context=gpu_ctx, benchmark=bench)
        _check_call(res, plain, bench, CALLS[name][1].get("horizons"), CALLS[name][1].get("compounding", "simple"))
        if name in SECOND:                                  # the call's own second array and its record ride beside Y
            assert SECOND[name] in res[0] and SECOND[name] in plain[0]
    again = _call(name, W, context=gpu_ctx)                 # the request is spent: the next call is the plain one
    assert "relative" not in again[0]
    _same(again, plain, "the plain call after")


@pytest.mark.parametrize("K,horizons", [(20, (5, 12)), (40, None)])
def test_passes_of_eight_and_the_sweep_kernels(gpu_ctx, K, horizons):
    """K = 20 on the horizon walk: passes of 8; K = 40 on the plain walk: the MFMA sweep kernels, which take K >= 17 there."""
    mu, cov, W = _market(K)
    base = dict(n_steps=T, n_paths=PATHS, seed=SEED, store=True, context=gpu_ctx, horizons=horizons)
    plain = simulate_paths(mu, cov, W, **base)
    _check_call(simulate_paths(mu, cov, W, benchmark=K - 3, **base), plain, K - 3, horizons)


@pytest.mark.parametrize("partition", ["two logical shards", "three logical shards, antithetic"])
def test_logical_shards_count_exactly_and_sum_to_association(gpu_ctx, partition):
    mu, cov, W = _market(K5)
    kw = dict(n_steps=T, n_paths=PATHS, seed=SEED, store=True, horizons=(3, 12), benchmark=2)
    ctx = Context((0, 0)) if partition == "two logical shards" else Context((0, 0, 0))
    if partition != "two logical shards":
        kw["antithetic"] = True
    try:
        one = simulate_paths(mu, cov, W, context=gpu_ctx, **kw)
        got = simulate_paths(mu, cov, W, context=ctx, **kw)
    finally:
        ctx.close()
    xb = ref_.to_x(one[2]["terminal"])
    for k, (da, db) in enumerate(zip(one, got)):
        assert da["terminal"].tobytes() == db["terminal"].tobytes()
        ra, rb = da["relative"], db["relative"]
        assert ra["pivot"] == rb["pivot"] and ra["bench_pivot"] == rb["bench_pivot"]
        ref_.same_to_association(ref_.record_of(ra), ref_.record_of(rb), ref_.to_x(da["terminal"]), xb, ra["pivot"], ra["bench_pivot"],
                                 f"{partition} k={k}")
        _same(ra["active"], rb["active"], f"{partition} k={k} active")
        for h in range(2):
            assert ra["horizons"][h]["p_under"] == rb["horizons"][h]["p_under"]
            assert abs(ra["horizons"][h]["tracking_error"] - rb["horizons"][h]["tracking_error"]) <= 1e-10 * ra["horizons"][h]["tracking_error"]


def test_a_horizons_record_is_the_terminal_record_of_the_call_that_ends_there(gpu_ctx):
    mu, cov, W = _market(K5)
    full = simulate_paths(mu, cov, W, n_steps=T, n_paths=PATHS, seed=SEED, store=True, horizons=(1, 5, 12), benchmark=4, context=gpu_ctx)
    for h, steps in enumerate((1, 5, 12)):
        short = simulate_paths(mu, cov, W, n_steps=steps, n_paths=PATHS, seed=SEED, store=True, benchmark=4, context=gpu_ctx)
        for k in range(K5):
            assert full[k]["horizon_terminal"][h].tobytes() == short[k]["terminal"].tobytes()
            hb, tb = full[k]["relative"]["horizons"][h], short[k]["relative"]
            assert hb["p_under"] == tb["p_under"] and hb["p_over"] == tb["p_over"] and hb["pivot"] == tb["pivot"]   # the counts to the bit
            for f in relative.STAT_FIELDS:
                assert abs(hb[f] - tb[f]) <= 1e-10 * max(abs(tb[f]), 1e-3), (steps, k, f, hb[f], tb[f])


def test_downside_and_benchmark_together_are_each_alone(gpu_ctx):
    mu, cov, W = _market(K5)
    base = dict(n_steps=T, n_paths=PATHS, seed=SEED, store=True, horizons=(4, 12), drawdown=False, context=gpu_ctx)
    both = simulate_paths(mu, cov, W, downside=0.004, benchmark=2, **base)
    ds = simulate_paths(mu, cov, W, downside=0.004, **base)
    rl = simulate_paths(mu, cov, W, benchmark=2, **base)
    for k in range(K5):
        _same({key: v for key, v in both[k].items() if key != "relative"}, ds[k], f"downside k={k}")
        _same({key: v for key, v in both[k].items() if key != "downside"}, rl[k], f"relative k={k}")


# ---- 4. refusals and the request's lifetime -----------------------------------------------------------------------------------------------

def test_the_refusals_reach_the_library_and_leave_the_context_usable(gpu_ctx):
    mu, cov, W = _market(K5)
    kw = dict(n_steps=T, n_paths=PATHS, seed=SEED)
    small = Context(0, terminal_budget=3 * PATHS * 8)      # 8 bytes per path and portfolio with the request: 3 of the 5 portfolios
    try:
        with pytest.raises(_ffi.McpError, match="raise the budget or shard by paths"):
            simulate_paths(mu, cov, W, benchmark=0, context=small, **kw)
        plain = simulate_paths(mu, cov, W, context=small, **kw)           # usable, in two tiles, and the request is gone
        assert "relative" not in plain[0]
        _same(plain, simulate_paths(mu, cov, W, context=gpu_ctx, **kw), "after the refusal")
    finally:
        small.close()
    two = Context((0, 0))
    try:
        lib, prm = _ffi.lib(), _ffi.make_params(N_ASSETS, T, K5, shard_portfolios=True)   # shard="portfolios", past the front end's refusal
        from monte_carlo_portfolio_amd.simulate import prepare_inputs
        mu32, L, W32 = prepare_inputs(mu, cov, W)
        stats = np.zeros(K5, _ffi.RELATIVE_STATS_DTYPE)
        _ffi.check(lib.mcp_ctx_request_relative(two._h, ctypes.byref(_ffi.McpRelative(1, 0)), None, _ffi.ptr(stats), None, None, None))
        with pytest.raises(_ffi.McpError, match="shard by paths"):
            two.simulate(prm, mu32, L, W32, SEED, 0, PATHS, False)
        assert not stats.view(np.uint8).any()
        ok = simulate_paths(mu, cov, W, benchmark=1, context=two, **kw)   # the same context, by paths
        assert ok[1]["relative"]["beta"] == 1.0 and not stats.view(np.uint8).any()
    finally:
        two.close()


def test_a_failing_call_spends_the_request(gpu_ctx):
    """Armed, a call that fails once it has taken the request, then a plain call: the plain call writes nothing into the request's
    arrays.  A call refused by its own argument rules never reaches the context and leaves the request for the next call."""
    lib = _ffi.lib()
    mu, cov, W = _market(2)
    kw = dict(n_steps=T, n_paths=PATHS, seed=SEED, context=gpu_ctx)
    stats, sums = np.zeros(2, _ffi.RELATIVE_STATS_DTYPE), np.zeros(2, _ffi.RELATIVE_SUMS_DTYPE)
    act, hz = np.zeros(2, _ffi.STATS_DTYPE), np.zeros((1, 2), _ffi.RELATIVE_STATS_DTYPE)
    arm = lambda bench, hz_out=None: _ffi.check(lib.mcp_ctx_request_relative(gpu_ctx._h, ctypes.byref(_ffi.McpRelative(bench, 0)),   # noqa: E731
                                                                           _ffi.ptr(sums), _ffi.ptr(stats), _ffi.ptr(act), None, _ffi.ptr(hz_out)))
    untouched = lambda: not any(a.view(np.uint8).any() for a in (stats, sums, act, hz))      # noqa: E731
    arm(0, hz)
    with pytest.raises(_ffi.McpError, match="no horizons"):  # hz_stats_out with a call that has none: refused before it walks
        simulate_paths(mu, cov, W, **kw)
    simulate_paths(mu, cov, W, **kw)
    assert untouched()
    arm(2)
    with pytest.raises(_ffi.McpError, match="bench=2"):      # not a row of this call's two portfolios
        simulate_paths(mu, cov, W, **kw)
    simulate_paths(mu, cov, W, **kw)
    assert untouched()
    arm(1)
    from monte_carlo_portfolio_amd.simulate import prepare_inputs
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    with pytest.raises(_ffi.McpError):                       # refused by the call's own rules (n_steps < 0), before the context is looked at:
        gpu_ctx.simulate(_ffi.make_params(N_ASSETS, -1, 2), mu32, L, W32, SEED, 0, PATHS, False)
    assert untouched()                                       # the request stays, and the next call that walks paths takes it
    simulate_paths(mu, cov, W, **kw)
    assert list(sums["n"]) == [PATHS, PATHS] and stats["beta"][1] == 1.0 and stats["tracking_error"][0] > 0 and act["n"][0] == PATHS
    stats[:], sums[:], act[:] = 0, 0, 0
    simulate_paths(mu, cov, W, **kw)
    assert untouched()
    arm(1)
    _ffi.check(lib.mcp_ctx_request_relative(gpu_ctx._h, None, None, None, None, None, None))     # withdrawn
    simulate_paths(mu, cov, W, **kw)
    assert untouched()


# ---- 5. the law -------------------------------------------------------------------------------------------------------------------------

def test_the_one_step_law_at_a_million_paths(gpu_ctx):
    """N = 4, T = 1, Gaussian draws: x = w . r is normal up to binary32 rounding, and so is the active return against row 0."""
    n = 1_000_000
    mu, cov = synthetic.synthetic_market(4)
    W = np.array([[0.25, 0.25, 0.25, 0.25], [0.7, 0.1, 0.1, 0.1], [0.0, 0.2, 0.3, 0.5]])
    res = simulate_paths(mu, cov, W, n_steps=1, n_paths=n, seed=SEED, benchmark=0, context=gpu_ctx)
    for k in (1, 2):
        assert res[k]["relative"]["sums"]["n"] == n
        ref_.law_assertions(res[k]["relative"], relative.relative_law(mu, cov, W[k], W[0]), n, f"gpu k={k}")

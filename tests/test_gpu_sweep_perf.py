"""The sweep's series statistics on the device (SPEC.md 5.24, `sweep_perf_kernel` through `sweep.score_performance`, i.e. the C ABI).

The order of the sums is the definition, so the raw records equal the NumPy restatement (tests/sweep_perf_ref.py) byte for byte: at
the row minimum, one portfolio past a full wave, a ragged last wave of 2,500, both sides of the older kernels' 256-row switch, the
widest N and the longest R, at two risk-free rates; on hand-made rows through every branch (no negative, one negative, a repeated
trough, wealth 0 in the middle and at the first row) with the stated field values; the reference's recorded numbers within the bars
of the CPU test, optimum indices exact; mcp_sweep_historical undisturbed on the same context; the example end to end."""
import contextlib
import io
import math
import os
import re
import runpy
import sys

import numpy as np
import pytest

import sweep_perf_ref as ref_
from monte_carlo_portfolio_amd import _ffi, sweep
from sweep_perf_cases import CASES, assert_goldens, case_inputs, case_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = ("n", "n_neg", "peak_row", "trough_row", "S", "S_neg", "M2", "M2_neg", "prod", "mdd")
SHAPES = ((2, 1, 1), (13, 3, 65), (53, 3, 2500), (257, 7, 130), (1000, 64, 3), (4096, 16, 65))


def device_records(out):
    """The raw fields of score_performance(raw=True) back in one record array."""
    rec = np.zeros(len(out["n"]), _ffi.SWEEP_PERF_SUMS_DTYPE)
    for k in RAW:
        rec[k] = out[k]
    return rec


def assert_bytes(got, want, what):
    bad = [k for k in RAW if not np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8))]
    assert not bad, (what, bad, [(int(p), got[bad[0]][p], want[bad[0]][p]) for p in np.flatnonzero(got[bad[0]] != want[bad[0]])[:3]])


@pytest.mark.parametrize("R,N,P", SHAPES)
def test_raw_records_equal_the_restatement_byte_for_byte(gpu_ctx, R, N, P):
    rs = np.random.RandomState([R, N, P])
    returns = 0.02 * rs.standard_normal((R, N)) + 3e-4
    W = rs.dirichlet(np.ones(N), size=P)
    if P > 2:
        W[1] = 3.0 * W[1] - 2.0 / N                          # a long/short row
        W[2, : (N + 1) // 2] = 0.0                           # exact zeros
    for rf, ann in ((0.0, 12), (0.03, 52)):
        out = sweep.score_performance(returns, W, rf, ann, raw=True)
        want = ref_.raw_records(returns, W, rf, ann)
        assert_bytes(device_records(out), want, (R, N, P, rf))
        fin = sweep.performance_finish(want, ann)            # the library's finish of its own records: pow aside, the same bits
        for k in ("sharpe_ratio", "sortino_ratio", "annual_volatility", "max_drawdown"):
            assert np.array_equal(out[k], fin[k], equal_nan=True), k
        assert np.array_equal(out["peak_row"], want["peak_row"]) and np.array_equal(out["trough_row"], want["trough_row"])
        assert (want["peak_row"] <= want["trough_row"]).all() and (R == 2 or ((want["n_neg"] > 1).all() and (want["mdd"] < 0).all()))


ALL_UP = (0.25, 0.5, 0.125, 0.0, 0.25, 0.5, 0.0625, 0.125)           # e >= 0 at rf 0: n_neg = 0; wealth never falls
ONE_DOWN = (0.25, 0.5, -0.25, 0.125, 0.25, 0.0, 0.5, 0.125)          # exactly one negative
TWICE = (0.5, -0.5, 1.0, -0.5, 0.25, 0.0, 0.125, 0.0)                # wealth 1.5, 0.75, 1.5, 0.75, ...: the trough -1/2 twice
LOST_MID = (0.25, 0.5, -0.25, -1.0, 0.5, 0.25, 0.0, 0.125)           # -100 % at row 3: wealth 0 from there on
LOST_FIRST = (-1.0, 0.5, 0.25, -0.25, 0.5, 0.25, 0.0, 0.125)         # -100 % at row 0: the first peak is 0, 0 / 0
W_CRAFTED = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [0.25, 0.75]])


@pytest.mark.parametrize("pair", ((ALL_UP, ONE_DOWN), (TWICE, LOST_MID), (LOST_FIRST, ALL_UP)), ids=("up_onedown", "twice_lostmid", "lostfirst_up"))
def test_crafted_rows_take_every_branch(gpu_ctx, pair):
    """(R, N, P) = (8, 2, 4): the weights (1, 0) and (0, 1) make the two crafted series themselves (x = 0.0 + r * 1.0 + s * 0.0), every
    figure a dyadic rational; two mixtures ride along.  All four byte-equal to the restatement, the two pure ones at stated values."""
    returns = np.ascontiguousarray(np.array(pair, np.float64).T)
    out = sweep.score_performance(returns, W_CRAFTED, 0.0, 4, raw=True)
    assert_bytes(device_records(out), ref_.raw_records(returns, W_CRAFTED, 0.0, 4), pair)
    for p, series in enumerate(pair):
        x = np.array(series)
        assert out["n"][p] == 8 and out["S"][p] == x.sum() and out["prod"][p] == np.prod(1.0 + x)       # dyadic: any order is exact
        if series is ALL_UP:
            assert out["n_neg"][p] == 0 and out["S_neg"][p] == 0.0 and out["M2_neg"][p] == 0.0
            assert out["sortino_ratio"][p] == x.sum() / 8 / 1e-4 * 2.0                                    # the 1e-4 branch
            assert out["mdd"][p] == 0.0 and out["max_drawdown"][p] == 0.0 and out["calmar"][p] == 0.0
            assert out["peak_row"][p] == 0 and out["trough_row"][p] == 0 and out["sharpe_ratio"][p] > 0
        elif series is ONE_DOWN:
            assert out["n_neg"][p] == 1 and out["S_neg"][p] == -0.25 and out["M2_neg"][p] == 0.0
            assert math.isnan(out["sortino_ratio"][p]) and math.isfinite(out["sharpe_ratio"][p])
            assert out["mdd"][p] == -0.25 and out["peak_row"][p] == 1 and out["trough_row"][p] == 2
            assert math.isfinite(out["calmar"][p]) and out["calmar"][p] > 0
        elif series is TWICE:
            assert out["mdd"][p] == -0.5 and out["trough_row"][p] == 1 and out["peak_row"][p] == 0       # the first of the two
            assert out["n_neg"][p] == 2 and out["S_neg"][p] == -1.0 and out["M2_neg"][p] == 0.0
            assert out["sortino_ratio"][p] == math.inf                                                    # a zero downside_std, IEEE
        elif series is LOST_MID:
            assert out["prod"][p] == 0.0 and out["mdd"][p] == -1.0 and out["trough_row"][p] == 3 and out["peak_row"][p] == 1
            assert out["annual_return"][p] == -1.0 and out["calmar"][p] == -1.0 and out["n_neg"][p] == 2
        else:
            assert series is LOST_FIRST and out["prod"][p] == 0.0
            assert np.isnan(out["mdd"][p]) and out["trough_row"][p] == -1 and out["peak_row"][p] == -1
            assert np.isnan(out["max_drawdown"][p]) and np.isnan(out["calmar"][p]) and out["annual_return"][p] == -1.0
            assert np.array_equal(out["mdd"][p:p + 1].view(np.uint64), [0x7FF8000000000000])
    mixed = out["mdd"][2:]
    assert (np.isnan(mixed) | (mixed <= 0.0)).all()


@pytest.mark.parametrize("name,rf,ann", CASES)
def test_goldens_through_the_device(gpu_ctx, name, rf, ann):
    returns, W = case_inputs(name)
    out = sweep.score_performance(returns, W, rf, ann, raw=True)
    rec = device_records(out)
    assert_goldens(name, rf, ann, rec, out)
    assert_bytes(rec, case_records(name, rf, ann), (name, rf, ann))


def test_sweep_historical_is_undisturbed_on_the_same_context(gpu_ctx):
    """The two calls share the context's sweep buffer: the older call's five outputs before and after a score_performance call, on
    both of its kernels, byte for byte -- and the new call repeats its own bytes after the older one."""
    rs = np.random.RandomState(5)
    for R in (53, 600):
        returns = 0.02 * rs.standard_normal((R, 5))
        W = rs.dirichlet(np.ones(5), size=130)
        mean, cov = returns.mean(0) * 12, np.cov(returns.T) * 12
        before = sweep.score_portfolios(returns, mean, cov, W, 0.03)
        perf = sweep.score_performance(returns, W, 0.03, 12, raw=True)
        after = sweep.score_portfolios(returns, mean, cov, W, 0.03)
        again = sweep.score_performance(returns[:40], W[:70], 0.03, 12, raw=True)       # a smaller call in the same buffer
        perf2 = sweep.score_performance(returns, W, 0.03, 12, raw=True)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), (R, k)
        for k in perf:
            assert perf[k].tobytes() == perf2[k].tobytes(), (R, k)
        assert_bytes(device_records(again), ref_.raw_records(returns[:40], W[:70], 0.03, 12), R)


def test_run_sweep_picks_the_restatements_optimum(gpu_ctx):
    returns, _ = case_inputs("weekly_seed12345")
    _, _, W0, _, _ = sweep.run_sweep(returns, "Monte Carlo", 300, annual_factor=52, seed=1)
    for method, key in sweep._EXTRA_METRIC.items():
        risks, rets, W, metric, opt = sweep.run_sweep(returns, method, 300, annual_factor=52, seed=1, risk_free=0.03)
        assert np.array_equal(W, W0) and len(risks) == len(rets) == len(metric) == 300
        want = sweep.performance_finish(ref_.raw_records(returns, W, 0.03, 52), 52)[key]
        assert opt == ref_.select(list(want)) and metric[opt] == np.nanmax(metric)


def test_pipeline_prints_the_three_extra_optima(gpu_ctx):
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
        res, _ = mod["main"](files, n_paths=20_000)
    assert tuple(res) == sweep.METHODS
    for m in sweep.EXTRA_METHODS:
        line = re.search(r"^%s\s+opt_idx\s+(\d+)\s+risk .* score ([-+0-9.]+)$" % re.escape(m), out.getvalue(), re.M)
        assert line and 0 <= int(line.group(1)) < len(res["Monte Carlo"]["all_weights"]), out.getvalue()[:3000]
        if m == "Max Drawdown":
            assert -1.0 <= float(line.group(2)) <= 0.0

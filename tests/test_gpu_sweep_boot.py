"""The resampled historical sweep on the device (SPEC.md 5.25, mcp_sweep_boot.hip through `sweep.score_resampled`, i.e. the C ABI).

The order of every sum is the definition, so scores, optima and counts equal the NumPy restatement (tests/sweep_boot_ref.py) bit for
bit.  The shapes are the smallest at which the kernels can go wrong.  The score kernel has one strategy for every R; what changes
with the sizes, and where the cover sits on both sides of it:
  * the bitonic network runs on R rounded up to a power of two (R = 2, 64 | 65, 256 | 257, 300: padding rows 0, 0 | 63, 0 | 255, 212);
  * the sorted walks take 8 rows per trip (R = 2, 13, 65, 257, 300 end inside a trip; 64 and 256 on its edge);
  * a workgroup scores 256 replicates per pass and a wave 64 (B = 1, 63 | 64 | 65, 257, 300: absent lanes, a second pass);
  * few portfolios cut their replicates over up to ceil(1024 / P) workgroups (P = 1 and B > 256: two slices; P = 130: one pass each);
  * the counts kernel runs one lane per replicate in blocks of 256 (the same B);
  * the arg-max kernel takes 64 replicates per workgroup and cuts the portfolios into 16 slices of ceil(P / 16) (P = 1: fifteen empty
    slices; 64: full slices of 4; 65: thirteen of 5 and three empty; 130: fourteen of 9, one of 4, one empty)."""
import contextlib
import ctypes
import io
import math
import os
import re
import runpy
import sys

import numpy as np
import pytest

import sweep_boot_ref as ref_
from bootstrap_ref import boot_indices
from monte_carlo_portfolio_amd import _ffi, simulate_paths, sweep, synthetic
from sweep_boot_ref import LAW, law_input, law_ratio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1F2E3D4C5B6A7988                       # a 64-bit seed: both key words matter
BEGIN = 2 ** 32 - 3                             # the replicate ids cross into the high counter word
INF = math.inf
#         R    N    P    B  block alpha
COVER = ((2, 1, 1, 1, 1.0, 0.95),
         (2, 3, 65, 300, 4.0, 0.5),
         (13, 3, 64, 63, 4.0, 0.95),
         (13, 16, 130, 64, 1.0, 0.99),
         (64, 16, 65, 64, INF, 0.99),
         (64, 3, 1, 257, 1.0, 0.5),
         (65, 64, 1, 65, 1.0, 0.95),
         (256, 1, 130, 257, 4.0, 0.5),
         (257, 3, 64, 300, 1.0, 0.99),
         (300, 16, 130, 65, 4.0, 0.95),
         (300, 64, 65, 1, INF, 0.5))


def assert_bits(got, want, what):
    for k in ref_.FIGURES:
        g, w = np.ascontiguousarray(got[k]).view(np.uint64), np.ascontiguousarray(want[k]).view(np.uint64)
        bad = np.argwhere(g != w)
        assert g.shape == w.shape and not len(bad), (what, k, len(bad), [(tuple(i), got[k][tuple(i)], want[k][tuple(i)]) for i in bad[:3]])
    for m in ref_.CRITERIA:
        assert got["opt"][m].dtype == np.int32 and np.array_equal(got["opt"][m], want["opt"][m]), (what, m)
    if "counts" in got:
        assert got["counts"].dtype == np.uint16 and np.array_equal(got["counts"], want["counts"]), what


def market(R, N, P, seed):
    rs = np.random.RandomState(seed)
    returns = 0.02 * rs.standard_normal((R, N)) + 3e-4
    W = rs.dirichlet(np.ones(N), size=P)
    if P > 2:
        W[1] = 3.0 * W[1] - 2.0 / N                          # a long/short row
        W[2, : (N + 1) // 2] = 0.0                           # exact zeros
    return returns, W


@pytest.mark.parametrize("R,N,P,B,block,alpha", COVER)
def test_scores_optima_and_counts_equal_the_restatement_bit_for_bit(gpu_ctx, R, N, P, B, block, alpha):
    returns, W = market(R, N, P, [R, N, P, B])
    got = sweep.score_resampled(returns, W, 0.03, 12, alpha, B, block, SEED, BEGIN, counts=True)
    want = ref_.resampled(returns, W, 0.03, 12, alpha, SEED, BEGIN, B, block)
    assert_bits(got, want, (R, N, P, B, block, alpha))
    assert (got["counts"].sum(axis=1) == R).all() and all(np.isfinite(got[k]).all() for k in ref_.FIGURES)
    assert (got["cvar_95"] <= got["var_95"]).all()
    again = sweep.score_resampled(returns, W, 0.03, 12, alpha, B, block, SEED, BEGIN)           # without the counts: the same scores
    assert "counts" not in again and all(again[k].tobytes() == got[k].tobytes() for k in ref_.FIGURES)


def test_ties_signed_zeros_and_a_constant_series(gpu_ctx):
    """Rows 2, 5 and 9 are one row three times, row 7 is +0.0 and row 8 is -0.0 in every asset, asset 3 returns 1/4 in every row:
    portfolio 0 holds asset 3 alone (a constant series: port_std = 0, sharpe = 0 on every resample), portfolio 1 is all zeros, and
    portfolios 33 .. 65 repeat 0 .. 32, so every maximum is attained twice."""
    rs = np.random.RandomState(21)
    R, N, B = 16, 4, 130
    returns = 0.02 * rs.standard_normal((R, N))
    returns[5] = returns[9] = returns[2]
    returns[7], returns[8] = 0.0, -0.0
    returns[:, 3] = 0.25
    W = rs.dirichlet(np.ones(N), size=66)
    W[0] = (0.0, 0.0, 0.0, 1.0)
    W[1] = 0.0
    W[:, 3] = np.where(np.arange(66) < 2, W[:, 3], 0.0)       # the others do not hold the constant asset: their rows 7 and 8 tie at 0
    W[33:] = W[:33]                                           # every portfolio twice, in different slices of the arg-max: the first one wins
    assert np.signbit(returns[8, :3]).all() and not np.signbit(returns[7]).any()
    for block, alpha in ((1.0, 0.95), (4.0, 0.5), (INF, 0.99)):
        got = sweep.score_resampled(returns, W, 0.03, 4, alpha, B, block, SEED, BEGIN, counts=True)
        assert_bits(got, ref_.resampled(returns, W, 0.03, 4, alpha, SEED, BEGIN, B, block), (block, alpha))
        assert (got["port_std"][:2] == 0.0).all() and (got["sharpe"][:2] == 0.0).all()
        assert (got["port_return"][0] == 1.0).all() and (got["var_95"][0] == 0.25).all() and (got["cvar_95"][0] == 0.25).all()
        assert (got["port_std"][2:33] > 0.0).all() and all(got[k][33:].tobytes() == got[k][:33].tobytes() for k in ref_.FIGURES)
        assert all((got["opt"][m] < 33).all() for m in ref_.CRITERIA)


def test_two_rows_take_counts_0_1_2_between_two_ranks(gpu_ctx):
    returns, W = market(2, 3, 5, 8)
    assert ref_.percentile_rank(2, 0.95)[:2] == (0, 1)
    got = sweep.score_resampled(returns, W, 0.0, 12, 0.95, 64, 1.0, SEED, BEGIN, counts=True)
    assert sorted(set(got["counts"].ravel().tolist())) == [0, 1, 2]
    assert_bits(got, ref_.resampled(returns, W, 0.0, 12, 0.95, SEED, BEGIN, 64, 1.0), "R=2")
    both = got["counts"][:, 0] == 1                            # one of each row: the interpolated percentile of the two values
    y = ref_.series(returns, W)
    assert (got["var_95"][:, both] == np.percentile(y, (1 - 0.95) * 100, axis=1)[:, None]).all()
    twice = got["counts"][:, 0] == 2                           # row 0 twice: every figure collapses onto y[0]
    assert (got["var_95"][:, twice] == y[:, :1]).all() and (got["cvar_95"][:, twice] == y[:, :1]).all() and (got["port_std"][:, twice] == 0).all()


@pytest.mark.parametrize("R", (53, 300))
def test_one_circular_block_is_the_sweep_itself(gpu_ctx, R):
    """block = inf: every replicate holds every row once, so its var_95 is `score_portfolios`' bit for bit (both take the same two
    order statistics through the same lerp) and its cvar_95 is the same tail in another association: the tail sum of n_tail <= R terms
    is within gamma_n sum|terms| of any other order of it, n = R + 2 covering the division and the other kernel's compensated sum."""
    returns, W = market(R, 5, 130, R)
    mean, cov = returns.mean(0) * 12, np.cov(returns.T) * 12
    base = sweep.score_portfolios(returns, mean, cov, W, 0.03)
    got = sweep.score_resampled(returns, W, 0.03, 12, 0.95, 3, INF, SEED, BEGIN, counts=True)
    assert (got["counts"] == 1).all()
    y = ref_.series(returns, W)
    n = R + 2
    gam = n * 2.0 ** -53 / (1.0 - n * 2.0 ** -53)
    for q in range(3):
        assert got["var_95"][:, q].tobytes() == base["var_95"].tobytes()
        tail = y <= base["var_95"][:, None]
        bound = gam * np.where(tail, np.abs(y), 0.0).sum(axis=1) / tail.sum(axis=1)
        err = np.abs(got["cvar_95"][:, q] - base["cvar_95"])
        assert (err <= bound).all(), (R, q, float((err / bound).max()))
    assert all(got[k][:, 0].tobytes() == got[k][:, 2].tobytes() for k in ref_.FIGURES)


def test_any_partition_of_the_replicates_gives_the_same_bytes(gpu_ctx):
    returns, W = market(65, 3, 70, 4)
    whole = sweep.score_resampled(returns, W, 0.03, 12, 0.95, 130, 4.0, SEED, BEGIN, counts=True)
    head = sweep.score_resampled(returns, W, 0.03, 12, 0.95, 64, 4.0, SEED, BEGIN, counts=True)
    tail = sweep.score_resampled(returns, W, 0.03, 12, 0.95, 66, 4.0, SEED, BEGIN + 64, counts=True)
    for k in ref_.FIGURES:
        assert np.concatenate([head[k], tail[k]], axis=1).tobytes() == whole[k].tobytes(), k
    for m in ref_.CRITERIA:
        assert np.concatenate([head["opt"][m], tail["opt"][m]]).tobytes() == whole["opt"][m].tobytes(), m
    assert np.concatenate([head["counts"], tail["counts"]]).tobytes() == whole["counts"].tobytes()


def test_a_replicate_resamples_the_rows_its_bootstrap_path_walks(gpu_ctx):
    R, B = 37, 70
    returns, W = market(R, 2, 1, 6)
    for block in (1.0, 3.0):
        got = sweep.score_resampled(returns, W, 0.0, 12, 0.95, B, block, SEED, BEGIN, counts=True)["counts"]
        paths = np.uint64(BEGIN) + np.arange(B, dtype=np.uint64)
        rows = boot_indices(SEED, paths, R, R, block)        # [T = R, B]: what path g of a bootstrap call over R steps walks
        for q in range(B):
            assert np.array_equal(got[q], np.bincount(rows[:, q], minlength=R)), (block, q)
        assert np.array_equal(got, sweep.resample_counts(R, B, block, SEED, BEGIN))             # and the host function


def test_the_context_is_left_as_it_was(gpu_ctx):
    """The older sweep calls share the context's buffer with the new one: their bytes before and after it; and a downside request armed
    before the call is still armed after it -- the next call that walks paths takes it."""
    rs = np.random.RandomState(5)
    returns = 0.02 * rs.standard_normal((53, 5))
    W = rs.dirichlet(np.ones(5), size=130)
    mean, cov = returns.mean(0) * 12, np.cov(returns.T) * 12
    before = sweep.score_portfolios(returns, mean, cov, W, 0.03)
    perf = sweep.score_performance(returns, W, 0.03, 12, raw=True)
    lib = _ffi.lib()
    stats, sums = np.zeros(2, _ffi.DOWNSIDE_STATS_DTYPE), np.zeros(2, _ffi.DOWNSIDE_SUMS_DTYPE)
    req = _ffi.McpDownside(0.0, 0, 0)
    _ffi.check(lib.mcp_ctx_request_downside(gpu_ctx._h, ctypes.byref(req), _ffi.ptr(sums), _ffi.ptr(stats), None))
    boot = sweep.score_resampled(returns, W, 0.03, 12, 0.95, 65, 1.0, SEED, BEGIN)
    assert not stats.view(np.uint8).any() and not sums.view(np.uint8).any()
    after = sweep.score_portfolios(returns, mean, cov, W, 0.03)
    perf2 = sweep.score_performance(returns, W, 0.03, 12, raw=True)
    boot2 = sweep.score_resampled(returns, W, 0.03, 12, 0.95, 65, 1.0, SEED, BEGIN)
    assert not stats.view(np.uint8).any() and not sums.view(np.uint8).any()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    for k in perf:
        assert perf[k].tobytes() == perf2[k].tobytes(), k
    for k in ref_.FIGURES:
        assert boot[k].tobytes() == boot2[k].tobytes(), k
    mu, cv = synthetic.synthetic_market(3)
    simulate_paths(mu, cv, synthetic.dirichlet_weights(3, 2), n_steps=12, n_paths=4096, seed=1, context=gpu_ctx)
    assert list(sums["n"]) == [4096, 4096]                   # the request was still armed


def test_the_bootstrap_law_on_the_device(gpu_ctx):
    returns, W = law_input()
    got = sweep.score_resampled(returns, W, 0.0, 1, 0.95, LAW["B"], 1.0, LAW["seed"], 0)
    ratio = law_ratio(returns, got["port_return"][0])
    print("std over replicates / sqrt((R-1)/R) s / sqrt(R) =", ratio)
    assert abs(ratio - 1.0) <= LAW["margin"], ratio


def test_pipeline_prints_the_resampled_lines(gpu_ctx):
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
    text = out.getvalue()
    win = re.search(r"^resampled sweep \(1,000 replicates\): the Monte Carlo optimum wins ([0-9.]+) % of them, is in the top 5 % in "
                    r"([0-9.]+) %; (\d+) portfolios win at least once$", text, re.M)
    assert win and 0.0 <= float(win.group(1)) <= float(win.group(2)) <= 100.0 and 1 <= int(win.group(3)) <= 1000, text[:3000]
    ci = re.search(r"^  95 % interval of its Sharpe: ([-+0-9.]+) \.\. ([-+0-9.]+) \(standard error ([0-9.]+)\)$", text, re.M)
    assert ci and float(ci.group(1)) < float(ci.group(2)) and float(ci.group(3)) > 0
    assert re.search(r"^  resampled weights \[.*\] beside its own \[.*\]$", text, re.M)
    assert tuple(res) == sweep.METHODS

"""The fused statistics epilogues of the path kernels end to end, at v0 != 1, on nearly riskless books and on ragged path tiles.

Every call of the table in tests/stats_cases.py goes through simulate_paths; every portfolio of every call is compared with NumPy
on the oracle's terminal values: the values bit for bit, counts and order statistics exactly (in log compounding var, min and max
to 1e-12: x = expm1(S), and the device's expm1 is not NumPy's to the last bit), and mean, std, Sharpe, CVaR and the
tail sum within the bounds test_gpu_parity.py (scale 1) and test_low_volatility_end_to_end (scale < 1) already use.  One test
function per shape, i.e. per launch kind: the lean kernel, mc_paths_kernel, the 8-portfolio register-select epilogue of
mcp_paths_body.inc, and sweep_moments behind both MFMA sweep kernels at every tiling of sweep_plan.

What this catches:
  * a wrong pivot index, or a pivot that disagrees with the record's: the pivots of a call spread over about 1e-2, so the mean is
    off by that much where the bound is 1e-13;
  * a wrong v0d or inv_v0d (v0 = 0.25 takes the fma branch of sweep_moments with inv_v0d = 4, the other three the division);
  * a reduction that lands in another portfolio's slot or drops a half-tile: n, min, max and mean of every portfolio, at path
    counts of one lane, one path short of a tile and one path into the second half-tile;
  * a raw-moment formula: at scale 1e-4 sigma/|mean| is about 5e-4 and sum x^2 - sum x * mean loses (mean/sigma)^2 2e-16, about
    1e-9 of the variance on top of what the partial sums lose, against a bound of 1e-9 on std that the shifted sums meet with
    room to spare;
  * the below / v0d of finish_stats and the tie rule of the tail: cvar, sum_tail and n_tail with ties at the quantile.

What it cannot catch: a single-rounding difference between the fma form and the division form of x (one ulp of x, 1e-16
relative), which is below every bound here.
"""
import numpy as np
import pytest

import stats_cases as sc
from monte_carlo_portfolio_amd import simulate_paths
from monte_carlo_portfolio_amd.simulate import Context

pytestmark = pytest.mark.gpu


def run(case, **kw):
    mu, cov, W = sc.market(case.shape, case.scale)
    return simulate_paths(mu, cov, W, n_steps=sc.T, n_paths=case.n_paths, seed=sc.SEED, v0=case.v0, compounding=case.compounding,
                          store=True, as_array=True, rf=sc.RF, alpha=case.alpha, path_begin=case.shape.path_begin, **kw)


def close(got, want, rel, abs_=0.0, what=""):
    np.testing.assert_allclose(got, want, rtol=rel, atol=abs_, err_msg=what)


def assert_case(case, st, term):
    want = sc.expected(case)
    ref = sc.terminal(case.shape, case.v0, case.scale, case.n_paths, case.compounding)
    tag = case.tag
    assert st.shape == (case.shape.K,) and term.shape == ref.shape
    assert np.array_equal(np.ascontiguousarray(term).view(np.uint32), ref.view(np.uint32)), tag
    for key in ("n", "n_tail"):
        assert np.array_equal(st[key], want[key]), (key, tag)
    for key in ("var", "min", "max"):
        if case.compounding == "simple":
            assert np.array_equal(st[key], want[key]), (key, tag)
        else:                                                   # x = expm1(S): the device's expm1 and NumPy's differ in the last bit on
            close(st[key], want[key], 1e-12, what=f"{key} {tag}")   # some values (assert_stats: 1e-12); a neighbouring value is 1e-4 off
    if case.scale == 1.0:
        for key in ("mean", "std", "sharpe", "cvar", "sum_tail"):
            close(st[key], want[key], 1e-12, 1e-15, what=f"{key} {tag}")
    else:
        close(st["mean"], want["mean_ld"], 1e-13, what=f"mean {tag}")
        close(st["std"], want["std_ld"], 1e-9, what=f"std {tag}")
        close(st["sharpe"], want["sharpe_ld"], 1e-9, what=f"sharpe {tag}")
        close(st["cvar"], want["cvar"], 1e-12, what=f"cvar {tag}")
        close(st["sum_tail"], want["sum_tail"], 1e-12, what=f"sum_tail {tag}")


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: s.id)
def test_every_portfolio_of_every_call(gpu_ctx, shape):
    for case in sc.cases_of(shape):
        st, term = run(case)
        assert_case(case, st, np.atleast_2d(term))


def test_same_device_shards_at_v0_3_low_volatility(gpu_ctx):
    """Three logical shards of one device on (16, 300), v0 = 3, scale 1e-4: the merge of the records in stats_kernel and the
    below / v0d of finish_stats across ranks.  Counts and order statistics equal the one-device call exactly, sums to 1e-13 (as
    test_same_device_shards_equal_one_device asserts); and the sharded records meet the bounds of the matrix themselves."""
    case = sc.Case(sc.SHAPE_BY_ID["n16_k300"], 3.0, 1e-4, sc.N_PATHS, "simple", sc.ALPHA)
    one = run(case)
    ctx = Context([0, 0, 0])
    try:
        many = run(case, context=ctx, devices=[0, 0, 0], shard="paths")
        assert ctx.exchange() == ("kernel", "")
    finally:
        ctx.close()
    assert np.array_equal(one[1].view(np.uint32), many[1].view(np.uint32))
    for key in ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max"):
        assert np.array_equal(one[0][key], many[0][key]), key
    for key in ("mean", "std", "sharpe", "cvar", "sum_tail"):
        np.testing.assert_allclose(many[0][key], one[0][key], rtol=1e-13, atol=1e-16, err_msg=key)
    assert_case(case, many[0], many[1])


def test_tiled_portfolios_at_v0_one_tenth(gpu_ctx):
    """(16, 513) at v0 = 0.1 under a terminal budget with room for 200 portfolios: the sweep runs in tiles of portfolios and must
    give the records of the untiled run (as test_terminal_budget_tiles_the_portfolios asserts), which meet the matrix's bounds."""
    case = sc.Case(sc.SHAPE_BY_ID["n16_k513"], 0.1, 1.0, sc.N_PATHS, "simple", sc.ALPHA)
    whole = run(case)
    ctx = Context(0, terminal_budget=200 * sc.N_PATHS * 4)
    try:
        tiled = run(case, context=ctx)
    finally:
        ctx.close()
    for key in ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max"):
        assert np.array_equal(whole[0][key], tiled[0][key]), key
    for key in ("mean", "std", "sharpe", "cvar", "sum_tail"):
        np.testing.assert_allclose(tiled[0][key], whole[0][key], rtol=1e-13, atol=1e-16, err_msg=key)
    assert np.array_equal(whole[1].view(np.uint32), tiled[1].view(np.uint32))
    assert_case(case, tiled[0], tiled[1])

"""The two kernels of the sweep over historical rows (`sweep_hist_kernel`: rank counting, R <= 256; `sweep_hist_sorted_kernel`:
bitonic sort in LDS, R > 256) at the places tests/test_gpu_sweep.py never puts them: order statistics at rank 0 and rank R - 1,
`rank_lo == rank_hi`, both `_lerp` branches next to those ranks, exact ties across the quantile, the row counts around the
wave-strided loops, the kernel switch and the +inf padding, N = 1, 2 and 64, degenerate moments, and the argument rules of
`mcp_sweep_historical`.  Everything goes through `sweep.score_portfolios`, i.e. the C ABI.

Yardstick: tests/sweep_ref.py (pinned to the reference's recorded run by tests/test_sweep_ref_cpu.py).  Bars, none of them measured
(u = 2^-53, the unit roundoff of binary64):
  var_95       equal by value: order statistics are exact and NumPy's _lerp is restated literally.
  cvar_95      within 2 (u sum|x_tail| / n_tail + u |cvar|) of the longdouble tail mean: the sum of n_tail doubles in any order
               and one rounding of the divide, doubled; equal to var_95 where the tail is one value repeated.
  port_return  within 2 N u sum_i |w_i mean_i| of longdouble (N - 1 additions and one rounding per product, doubled).
  variance     w' cov w within 2 (N^2 + N) u sum_ij |w_i cov_ij w_j| of longdouble; port_std within that bound carried through
               the square root (error / (2 std)) plus 2 u std for the root itself.
  sharpe       4 ulp from (port_return - rf) / port_std formed from the GPU's own two outputs.
"""
import ctypes

import numpy as np
import pytest

import sweep_ref
from monte_carlo_portfolio_amd import _ffi, sweep

pytestmark = pytest.mark.gpu

P = 37
RF = 0.03
U = sweep_ref.U
R_GRID = (1, 2, 3, 21, 63, 64, 65, 128, 255, 256, 257, 511, 512, 513, 1024, 1025, 2049, 4095, 4096)
ALPHAS = (0.95, 0.99, 0.75, 0.5, 0.05, 1 - 2.0 ** -40, 2.0 ** -40, 1e-300)
N_MAIN = 7
N_EXTRA = {2: (1, 2, 64), 64: (1, 2, 64), 256: (1, 2, 64), 257: (1, 2, 64), 4096: (1, 2, 64)}
DISTINCT = 0                    # tie level "no ties": the R rows as drawn


def _tie_levels(R):
    """m distinct rows sampled R times with replacement, m in {1, 2, 5, R}, and the R rows as drawn (no ties at all)."""
    return tuple(dict.fromkeys((1, 2, 5, R))) + (DISTINCT,)


def _rows(R, N, m):
    """[R, N] returns drawn normal(4e-4, 0.02).  m > 0: R rows sampled with replacement from m distinct ones, so equal rows give
    bit-equal series values under every weight vector; where R >= 2 m every distinct row is taken at least twice (no tie run of
    length one), the rest at random, in shuffled order."""
    rng = np.random.default_rng([R, N, m])
    base = rng.normal(4e-4, 0.02, (m or R, N))
    if m == DISTINCT:
        return base
    idx = rng.choice(m, R, p=np.arange(1.0, m + 1) / (m * (m + 1) / 2))   # unequal shares: no run boundary at R / 2
    if R >= 2 * m:
        idx[:2 * m] = np.repeat(np.arange(m), 2)
        rng.shuffle(idx)
    return np.ascontiguousarray(base[idx])


def _moments(N):
    """A mean and a positive definite covariance that do not depend on R (pandas' covariance of one row is NaN)."""
    rng = np.random.default_rng(1000 + N)
    A = rng.normal(0.0, 0.02, (N + 3, N))
    return rng.normal(0.1, 0.2, N), A.T @ A * (252.0 / (N + 2))


def _weights(N):
    """P - 2 Dirichlet rows, one row with exact zeros (the first half of the assets; all of them at N = 1), one long/short row
    (three times a Dirichlet row, less 2 on its smallest entry: sum 1; at N = 1 the single weight -1)."""
    rs = np.random.RandomState(N)
    W = rs.dirichlet(np.ones(N), P)
    z = W[P - 2].copy()
    z[:(N + 1) // 2] = 0.0
    W[P - 2] = z / z.sum() if z.sum() > 0 else z
    W[P - 1] *= 3.0
    W[P - 1, np.argmin(W[P - 1])] -= 2.0 if N > 1 else 4.0
    assert (W[P - 2] == 0.0).any() and (W[P - 1] < 0).any()
    return W


def _rank_class(R, alpha):
    """The classes of (rank_lo, rank_hi, gamma) the grid has to reach, as a set of names."""
    lo, hi, g = _ffi.percentile_rank(R, alpha)
    out = {"gamma == 0"} if g == 0.0 else {"0 < gamma < 0.5"} if g < 0.5 else {"gamma >= 0.5"}
    if lo == 0 and hi == 1:
        out.add("rank 0 and 1")
    if hi == R - 1 and lo == R - 2:
        out.add("rank R-2 and R-1")
    if lo == hi == R - 1 and R > 1:
        out.add("rank_lo == rank_hi == R-1")
    if R == 1:
        out.add("R == 1")
    if R == 2 and hi == 1:
        out.add("R == 2, gamma < 0.5" if g < 0.5 else "R == 2, gamma >= 0.5")
    return out


def test_the_grid_reaches_every_rank_class(mcp_lib):
    """A later edit of R_GRID or ALPHAS cannot quietly drop a class: each is met on the rank-counting kernel (R <= 256) and on
    the sorted one (R > 256), from the library's own mcp_percentile_rank."""
    both = ("gamma == 0", "0 < gamma < 0.5", "gamma >= 0.5", "rank 0 and 1", "rank R-2 and R-1", "rank_lo == rank_hi == R-1")
    small_only = ("R == 1", "R == 2, gamma < 0.5", "R == 2, gamma >= 0.5")
    seen = {False: set(), True: set()}
    for R in R_GRID:
        for alpha in ALPHAS:
            seen[R > 256] |= _rank_class(R, alpha)
    assert set(both) <= seen[True], set(both) - seen[True]
    assert set(both + small_only) <= seen[False], set(both + small_only) - seen[False]
    assert _ffi.percentile_rank(4096, 1e-300) == (4095, 4095, 0.0) and 1 - 1e-300 == 1.0
    assert {256, 257} <= set(R_GRID) and max(R_GRID) == 4096 and set(N_EXTRA) <= set(R_GRID)


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _check(rows, mean, cov, W, s, alpha, tag, worst):
    """One call of the library against the restatement; `worst` collects the largest error over its bound per output."""
    got = sweep.score_portfolios(rows, mean, cov, W, RF, alpha)
    ref = sweep_ref.score(rows, mean, cov, W, RF, alpha, s)
    N = W.shape[1]
    assert np.array_equal(got["var_95"], ref["var_95"]), (tag, np.flatnonzero(got["var_95"] != ref["var_95"])[:5])

    assert (ref["n_tail"] > 0).all(), tag                                   # var is never below the smallest element
    bound = 2 * (U * ref["tail_abs"] / ref["n_tail"] + U * np.abs(got["cvar_95"]))
    err = np.abs((got["cvar_95"].astype(np.longdouble) - ref["tail_ld"]).astype(np.float64))
    worst["cvar_95"] = max(worst["cvar_95"], float(np.max(err / np.where(bound > 0, bound, 1.0))))
    assert (err <= bound).all(), (tag, "cvar_95", float(np.max(err / np.where(bound > 0, bound, 1.0))))
    flat = np.where(s <= ref["var_95"][None, :], s, ref["var_95"][None, :])
    flat = flat.min(axis=0) == ref["var_95"]                                # the tail is one value repeated
    assert np.array_equal(got["cvar_95"][flat], got["var_95"][flat]), (tag, "cvar_95 != var_95 on a flat tail")
    assert (got["cvar_95"] <= got["var_95"]).all(), tag

    bound = 2 * N * U * ref["ret_abs"]
    err = np.abs((got["port_return"].astype(np.longdouble) - ref["ret_ld"]).astype(np.float64))
    worst["port_return"] = max(worst["port_return"], float(np.max(err / np.where(bound > 0, bound, 1.0))))
    assert (err <= bound).all(), (tag, "port_return", float(np.max(err / np.where(bound > 0, bound, 1.0))))

    vbound = 2 * (N * N + N) * U * ref["pvar_abs"]
    std = np.sqrt(ref["pvar_ld"])                                           # longdouble
    pos = ref["pvar_ld"] > 0
    assert pos.sum() >= P - 1, tag                                          # only an all-zero weight row has no variance
    verr = np.abs((got["port_std"].astype(np.longdouble) ** 2 - ref["pvar_ld"]).astype(np.float64))
    # the square of the returned root carries the root's own rounding back: 2 std (2 u std) on top of the variance's bound
    assert (verr[pos] <= (vbound + 4 * U * ref["pvar_ld"].astype(np.float64))[pos]).all(), (tag, "variance")
    bound = (vbound[pos] / (2 * std[pos])).astype(np.float64) + 2 * U * std[pos].astype(np.float64)
    err = np.abs((got["port_std"][pos].astype(np.longdouble) - std[pos]).astype(np.float64))
    worst["port_std"] = max(worst["port_std"], float(np.max(err / bound)))
    assert (err <= bound).all(), (tag, "port_std", float(np.max(err / bound)))
    assert (got["port_std"][~pos] == 0.0).all() and (got["sharpe"][~pos] == 0.0).all(), tag

    want = (got["port_return"][pos] - RF) / got["port_std"][pos]
    ulps = _ulps(got["sharpe"][pos], want)
    worst["sharpe"] = max(worst["sharpe"], float(ulps.max()) / 4)
    assert (ulps <= 4).all(), (tag, "sharpe", float(ulps.max()))
    return ref


@pytest.mark.parametrize("R", R_GRID)
def test_edges_of_rank_ties_and_row_count(gpu_ctx, R):
    """Every alpha x tie level (x N where the row count sits at a boundary) at this R.  Where ties are built in (m in {2, 5},
    R >= 21) the reference's tail must be longer than rank_lo + 1 in some portfolio, i.e. a tie run really crosses the quantile
    (the kernel's count is then checked through cvar_95); at rank_lo == R - 1 the tail is the whole series and cannot be longer."""
    worst = dict.fromkeys(("cvar_95", "port_return", "port_std", "sharpe"), 0.0)
    for N in (N_MAIN,) + N_EXTRA.get(R, ()):
        mean, cov = _moments(N)
        W = _weights(N)
        for m in _tie_levels(R):
            rows = _rows(R, N, m)
            s = sweep_ref.series(rows, W)
            for alpha in ALPHAS:
                tag = f"R={R} N={N} m={m} alpha={alpha!r}"
                ref = _check(rows, mean, cov, W, s, alpha, tag, worst)
                lo, _, _ = _ffi.percentile_rank(R, alpha)
                if m in (2, 5) and R >= 21:
                    if lo == R - 1:
                        assert (ref["n_tail"] == R).all(), tag
                    else:
                        assert (ref["n_tail"] > lo + 1).any(), tag
                if m == 1:
                    assert (ref["n_tail"] == R).all(), tag
    print(f"R={R}: largest error over its bound", {k: round(v, 3) for k, v in worst.items()})


def test_degenerate_moments(gpu_ctx):
    rng = np.random.default_rng(3)
    N = N_MAIN
    rows, (mean, _), W = _rows(21, N, DISTINCT), _moments(N), _weights(N)
    s = sweep.score_portfolios(rows, mean, np.zeros((N, N)), W, RF, 0.95)
    assert (s["port_std"] == 0.0).all() and (s["sharpe"] == 0.0).all() and not np.signbit(s["sharpe"]).any()
    s = sweep.score_portfolios(rows, mean, -np.eye(N), W, RF, 0.95)
    ref = sweep_ref.score(rows, mean, -np.eye(N), W, RF, 0.95)
    assert np.isnan(s["port_std"]).all() and np.isnan(ref["port_std"]).all()
    assert (s["sharpe"] == 0.0).all() and (ref["sharpe"] == 0.0).all()       # `std > 0` is false for a NaN
    assert np.array_equal(s["var_95"], ref["var_95"])
    mean4, cov4 = _moments(4)                                                # the call efficient_frontier makes
    s = sweep.score_portfolios(np.zeros((1, 4)), mean4, cov4, rng.dirichlet(np.ones(4), 5), 0.0, 0.95)
    assert (s["var_95"] == 0.0).all() and (s["cvar_95"] == 0.0).all() and (s["port_std"] > 0).all()


# ---- the argument rules, at the C level ---------------------------------------------------------------------------------
_VP, _D = ctypes.c_void_p, ctypes.c_double
_RAW = ctypes.CFUNCTYPE(ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, _VP, _D, _D, _VP, _VP, _VP, _VP, _VP)
_PTRS = ("returns", "mean", "cov", "W", "port_return", "port_std", "sharpe", "var", "cvar")


class _Call:
    """mcp_sweep_historical with plain pointers (the binding's ndpointer arguments cannot carry NULL)."""

    def __init__(self, ctx, rows, mean, cov, W):
        self.fn = ctypes.cast(_ffi.lib().mcp_sweep_historical, _RAW)
        self.ctx, (self.R, self.N), self.P = ctx._h, rows.shape, W.shape[0]
        self.arrays = dict(zip(_PTRS, [rows, mean, cov, W] + [np.full(self.P, -7.0) for _ in range(5)]))

    def __call__(self, alpha=0.95, null=None, **over):
        a = {k: (None if k == null else v.ctypes.data_as(_VP)) for k, v in {**self.arrays, **over.pop("arrays", {})}.items()}
        rc = self.fn(over.get("ctx", self.ctx), over.get("N", self.N), over.get("R", self.R), over.get("P", self.P), a["returns"],
                     a["mean"], a["cov"], a["W"], RF, alpha, *[a[k] for k in _PTRS[4:]])
        return rc, _ffi.lib().mcp_last_error().decode()

    def outputs(self):
        return [self.arrays[k] for k in _PTRS[4:]]


def _small_case():
    rows, (mean, cov), W = _rows(21, N_MAIN, DISTINCT), _moments(N_MAIN), _weights(N_MAIN)
    return np.ascontiguousarray(rows), np.ascontiguousarray(mean), np.ascontiguousarray(cov), np.ascontiguousarray(W)


def test_argument_rules_then_a_correct_call(gpu_ctx):
    """Each bad argument is MCP_E_ARG with the field named in mcp_last_error(), no output is written, and a correct call on the
    same context afterwards gives what it gave before."""
    rows, mean, cov, W = _small_case()
    before = sweep.score_portfolios(rows, mean, cov, W, RF)
    call = _Call(gpu_ctx, rows, mean, cov, W)
    cases = [(dict(R=0), "n_rows=0"), (dict(R=4097), "n_rows=4097"), (dict(N=0), "n_assets=0"), (dict(N=65), "n_assets=65"),
             (dict(P=0), "n_portfolios=0"), (dict(P=-1), "n_portfolios=-1"), (dict(alpha=0.0), "alpha=0"), (dict(alpha=1.0), "alpha=1"),
             (dict(alpha=float("nan")), "alpha=nan"), (dict(alpha=-0.5), "alpha=-0.5"), (dict(ctx=None), "ctx is NULL")]
    cases += [(dict(null=k), f"{k} is NULL") for k in _PTRS]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == _ffi.MCP_E_ARG and text in msg, (kw, rc, msg)
    assert all((o == -7.0).all() for o in call.outputs())
    rc, msg = call()
    assert rc == 0, msg
    after = sweep.score_portfolios(rows, mean, cov, W, RF)
    for k, o in zip(("port_return", "port_std", "sharpe", "var_95", "cvar_95"), call.outputs()):
        assert before[k].tobytes() == after[k].tobytes() == o.tobytes(), k
    assert np.array_equal(after["var_95"], sweep_ref.score(rows, mean, cov, W, RF, 0.95)["var_95"])
    empty = sweep.score_portfolios(rows, mean, cov, np.empty((0, N_MAIN)), RF)
    assert len(empty) == 5 and all(v.shape == (0,) and v.dtype == np.float64 for v in empty.values())


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_is_rejected(gpu_ctx, bad):
    """A NaN or an infinity in one cell of returns, W, mean or cov: MCP_E_ARG naming the array and the first offending index
    from C (no output written), ValueError from Python -- not a finite number that looks like a VaR.  Both kernels' sizes."""
    for R in (21, 300):
        rows, (mean, cov), W = _rows(R, N_MAIN, DISTINCT), _moments(N_MAIN), _weights(N_MAIN)
        good = dict(zip(("returns", "mean", "cov", "W"), (rows, mean, cov, W)))
        before = sweep.score_portfolios(rows, mean, cov, W, RF)
        for name, cell, text in (("returns", (R - 2, 3), f"returns[{(R - 2) * N_MAIN + 3}] (row {R - 2}, asset 3)"),
                                 ("W", (P - 1, 6), f"W[{(P - 1) * N_MAIN + 6}] (portfolio {P - 1}, asset 6)"),
                                 ("mean", (0,), "mean[0]"), ("cov", (6, 6), "cov[48] (row 6, column 6)")):
            arr = good[name].copy()
            arr[cell] = bad
            call = _Call(gpu_ctx, rows, mean, cov, W)
            rc, msg = call(arrays={name: arr})
            assert rc == _ffi.MCP_E_ARG and text in msg and "not finite" in msg, (name, rc, msg)
            assert all((o == -7.0).all() for o in call.outputs())
            with pytest.raises(ValueError, match=f"NaN or infinite values in {name} "):
                sweep.score_portfolios(*[arr if k == name else good[k] for k in ("returns", "mean", "cov", "W")], RF)
        after = sweep.score_portfolios(rows, mean, cov, W, RF)
        assert all(before[k].tobytes() == after[k].tobytes() for k in before)

"""The reference's random-weight portfolio sweep (what app.py calls "Monte Carlo"), on the GPU.

Reference lines restated here (script code of tab 2, app.py:655-764; function twin app.py:265-284):
  * weights: up to 100 tries of `np.random.dirichlet(np.ones(N), size=1)[0]` per portfolio from NumPy's
    global legacy generator, accepted iff inside [min_weights, max_weights]; a portfolio with no
    accepted draw is skipped (app.py:699-707).  Drawn HERE ON THE HOST WITH THE SAME NUMPY CALLS, so the
    weights are bit-identical to the reference's for the same seed and the optimum index is decidable.
  * scoring: app.py:708-713 for all accepted weight vectors at once -> libmcport.so
    (`mcp_sweep_historical`, HIP kernel `sweep_hist_kernel`, binary64).
  * metric / optimum: sharpe | -var | -cvar, argmax / argmin / 0 (app.py:672-676, 717, 747).
  * allocation: weights * investment_amount (app.py:763-764).
Quirks kept on purpose: Q2 `user_rf` is subtracted as given (default 3.0,
"percent"); Q7 the four random methods share one RNG stream in the order Monte Carlo, VaR, CVaR, MPT;
Q8 skipped portfolios shorten the arrays; Q9 `efficient_frontier` keeps the last rejected draw.

Beyond the reference's loop (SPEC.md 5.24): its own series statistics -- sharpe_ratio, sortino_ratio, annual_volatility,
annual_return, max_drawdown (app.py:231-256), which it applies per asset only -- for every weight row of a sweep
(`score_performance`, HIP kernel `sweep_perf_kernel`), and the three criteria they give: EXTRA_METHODS.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _ffi
from .simulate import default_context

METHODS = ("Monte Carlo", "VaR", "CVaR", "MPT", "Equal Weight")          # app.py:671-677, dict order
_METRIC = {"Monte Carlo": "sharpe", "VaR": "var_95", "CVaR": "cvar_95", "MPT": "sharpe", "Equal Weight": "sharpe"}
EXTRA_METHODS = ("Sortino", "Max Drawdown", "Calmar")                    # SPEC.md 5.24: not in the reference's loop, not in METHODS
_EXTRA_METRIC = {"Sortino": "sortino_ratio", "Max Drawdown": "max_drawdown", "Calmar": "calmar"}
PERFORMANCE_KEYS = ("sharpe_ratio", "sortino_ratio", "annual_volatility", "annual_return", "max_drawdown", "calmar", "peak_row",
                    "trough_row")


def draw_weights(n_assets, n_portfolios=2500, min_weights=None, max_weights=None):
    """app.py:699-707.  Uses (and advances) NumPy's global legacy RNG exactly like the reference: per portfolio up to 100
    tries of `np.random.dirichlet(np.ones(N), size=1)[0]`, the first one inside [min, max] is kept, a portfolio without one
    is skipped.  The legacy generator fills a `size=B` request row by row with the same arithmetic as B requests of size 1,
    so the candidates are drawn in blocks and the accept / retry / skip walk replayed over them; the generator is then put
    where the reference's loop would have left it (the four random methods share one stream, quirk Q7).  Same weights,
    same stream position, two orders of magnitude less host time (`_draw_weights_loop` is the literal form; the tests compare)."""
    lo = np.zeros(n_assets) if min_weights is None else np.asarray(min_weights, float)
    hi = np.ones(n_assets) if max_weights is None else np.asarray(max_weights, float)
    ones = np.ones(n_assets)
    out = []
    remaining, tries_used = int(n_portfolios), 0          # tries already spent on the portfolio being drawn
    while remaining > 0:
        state = np.random.get_state()
        B = max(256, 2 * remaining)
        C = np.random.dirichlet(ones, size=B)              # the next B candidates of the stream
        ok = np.all(C >= lo, axis=1) & np.all(C <= hi, axis=1)
        hits = np.flatnonzero(ok)
        pos = 0                                            # candidates of this block consumed so far
        if hits.size and hits[0] < 100 - tries_used and (np.diff(hits) <= 100).all():
            take = min(remaining, hits.size)               # no portfolio runs out of tries before the last hit taken:
            out.append(C[hits[:take]])                     # portfolios simply take consecutive accepted candidates
            remaining -= take
            pos = int(hits[take - 1]) + 1
            tries_used = 0
        pos, tries_used, remaining = _walk_block(C, ok, out, remaining, tries_used, pos)
        if pos < B:                                        # stopped inside the block: rewind and consume exactly `pos` rows
            np.random.set_state(state)
            if pos:
                np.random.dirichlet(ones, size=pos)
    return np.concatenate(out).reshape(-1, n_assets) if out else np.empty((0, n_assets))


def _walk_block(C, ok, out, remaining, tries_used, pos=0):
    """The literal accept / retry / skip walk of app.py:699-707 over one block of candidates, from row `pos`.  Returns
    (rows consumed, tries spent on the unfinished portfolio, portfolios still to draw)."""
    B = len(ok)
    while remaining > 0 and pos < B:
        window = 100 - tries_used
        seg = ok[pos:pos + window]
        hit = np.flatnonzero(seg)
        if hit.size:                                       # accepted on try tries_used + hit[0] + 1
            out.append(C[pos + hit[0]][None, :])
            pos += int(hit[0]) + 1
            remaining -= 1
            tries_used = 0
        elif len(seg) == window:                           # 100 tries failed: the portfolio is skipped (Q8)
            pos += window
            remaining -= 1
            tries_used = 0
        else:                                              # block ends inside this portfolio's tries
            tries_used += len(seg)
            pos = B
    return pos, tries_used, remaining


def _draw_weights_loop(n_assets, n_portfolios=2500, min_weights=None, max_weights=None):
    """The reference's loop as written (app.py:699-707); kept as the yardstick for draw_weights."""
    lo = np.zeros(n_assets) if min_weights is None else np.asarray(min_weights, float)
    hi = np.ones(n_assets) if max_weights is None else np.asarray(max_weights, float)
    out = []
    ones = np.ones(n_assets)
    for _ in range(n_portfolios):
        for _ in range(100):
            ws = np.random.dirichlet(ones, size=1)[0]
            if np.all(ws >= lo) and np.all(ws <= hi):
                out.append(ws)
                break
    return np.array(out).reshape(len(out), n_assets)


def sweep_inputs(returns_df, annual_factor):
    """mean_returns, cov_matrix of app.py:679-680 (pandas cov: ddof = 1) and the [R, N] float64 matrix."""
    if hasattr(returns_df, "cov"):                       # pandas DataFrame: literally the reference's calls
        mean = (returns_df.mean() * annual_factor).to_numpy(dtype=np.float64)
        cov = (returns_df.cov() * annual_factor).to_numpy(dtype=np.float64)
        R = returns_df.to_numpy(dtype=np.float64)
    else:                                                # plain [R, N] array (the pandas-free ingest): the same numbers,
        from .ingest_np import pandas_cov, pandas_mean   # bit for bit, as the DataFrame route (tests/test_ingest_np.py)
        R = np.asarray(returns_df, np.float64)
        mean = pandas_mean(R) * annual_factor
        cov = pandas_cov(R) * annual_factor
    return np.ascontiguousarray(R), np.ascontiguousarray(mean), np.ascontiguousarray(cov)


def score_portfolios(R, mean, cov, W, rf, alpha=0.95, device=0):
    """app.py:708-713 for all rows of W on the GPU -> dict of float64 [P] arrays.

    Every value of R, mean, cov and W must be finite, the rule `simulate_bootstrap` has for historical rows: the kernels order
    the series with plain compares, under which a NaN has no place, so such input is a ValueError here (and MCP_E_ARG in
    `mcp_sweep_historical`), not a finite number that looks like a VaR.  The reference's ingest drops such rows."""
    W = np.ascontiguousarray(W, np.float64)
    if W.ndim != 2:
        raise ValueError(f"W must be a [P, N] matrix, got shape {W.shape}")
    P, N = W.shape
    R = np.ascontiguousarray(R, np.float64)
    mean = np.ascontiguousarray(mean, np.float64)
    cov = np.ascontiguousarray(cov, np.float64)
    if R.ndim != 2 or R.shape[1] != N:
        raise ValueError(f"returns must be an [R, {N}] matrix like the {N} columns of W, got shape {R.shape}")
    if mean.shape != (N,):
        raise ValueError(f"mean must have shape ({N},), got {mean.shape}")
    if cov.shape != (N, N):
        raise ValueError(f"cov must have shape ({N}, {N}), got {cov.shape}")
    _check_sweep_arrays((("returns", R, ("row", "asset")), ("W", W, ("portfolio", "asset")), ("mean", mean, ("asset",)),
                         ("cov", cov, ("row", "column"))))
    outs = [np.empty(P, np.float64) for _ in range(5)]
    if P:
        ctx = default_context(device)
        _ffi.check(_ffi.lib().mcp_sweep_historical(ctx._h, N, R.shape[0], P, R, mean, cov, W, float(rf), float(alpha), *outs))
    return dict(zip(("port_return", "port_std", "sharpe", "var_95", "cvar_95"), outs))


def _check_sweep_arrays(arrays):
    """The finiteness rule of the sweep's arrays, worded once: (name, array, axis names) each."""
    for name, a, axes in arrays:
        bad = ~np.isfinite(a)
        if bad.any():
            first = np.unravel_index(int(np.argmax(bad)), a.shape)
            where = ", ".join(f"{ax} {int(i)}" for ax, i in zip(axes, first))
            raise ValueError(f"NaN or infinite values in {name} (first: {where}); {int(bad.sum())} in all, drop them first")


def performance_finish(sums, ann_factor):
    """mcp_sweep_perf_finish (SPEC.md 5.24) restated in NumPy binary64, in the reference's order of operations, for an array of raw
    records (`_ffi.SWEEP_PERF_SUMS_DTYPE`) -> dict of [P] arrays keyed PERFORMANCE_KEYS.  Every figure but the two that pass through
    pow equals the library's bit for bit."""
    sums = np.atleast_1d(np.asarray(sums, _ffi.SWEEP_PERF_SUMS_DTYPE))
    ann = np.float64(ann_factor)
    if not (np.isfinite(ann) and ann > 0):
        raise ValueError(f"ann_factor={ann_factor!r} is not finite and > 0")
    n, nn, root = sums["n"].astype(np.float64), sums["n_neg"].astype(np.float64), np.sqrt(ann)
    with np.errstate(all="ignore"):
        mean_excess = sums["S"] / n
        std = np.sqrt(sums["M2"] / (n - 1.0))
        sharpe = np.where(std == 0.0, 0.0, mean_excess / std * root)                               # app.py:235-236
        downside_std = np.where(sums["n_neg"] == 0, 1e-4, np.sqrt(sums["M2_neg"] / (nn - 1.0)))    # app.py:242
        sortino = mean_excess / downside_std * root
        annual_return = np.power(sums["prod"], ann / n) - 1.0                                      # app.py:249
        mdd = sums["mdd"].copy()
        calmar = np.where(mdd == 0.0, 0.0, annual_return / np.abs(mdd))
    return {"sharpe_ratio": sharpe, "sortino_ratio": sortino, "annual_volatility": std * root, "annual_return": annual_return,
            "max_drawdown": mdd, "calmar": calmar, "peak_row": sums["peak_row"].copy(), "trough_row": sums["trough_row"].copy()}


def score_performance(R, W, risk_free=0.0, ann_factor=12, device=0, raw=False):
    """The reference's series statistics (app.py:231-256) of `R @ w` for all rows w of W on the GPU (SPEC.md 5.24) -> dict of
    float64 [P] arrays sharpe_ratio, sortino_ratio, annual_volatility, annual_return, max_drawdown, calmar and int arrays peak_row,
    trough_row (the rows of the deepest drawdown's peak and trough; -1 where the drawdown is NaN).  `risk_free` and `ann_factor`
    mean what they mean in `metrics.sortino_ratio`.  raw=True adds the fields of the raw record (n, n_neg, S, S_neg, M2, M2_neg,
    prod, mdd).  R and W must be finite, as for `score_portfolios`."""
    W = np.ascontiguousarray(W, np.float64)
    if W.ndim != 2:
        raise ValueError(f"W must be a [P, N] matrix, got shape {W.shape}")
    P, N = W.shape
    R = np.ascontiguousarray(R, np.float64)
    if R.ndim != 2 or R.shape[1] != N:
        raise ValueError(f"returns must be an [R, {N}] matrix like the {N} columns of W, got shape {R.shape}")
    if R.shape[0] < 2:
        raise ValueError(f"returns must have at least 2 rows for a sample deviation, got {R.shape[0]}")
    if not (np.isfinite(ann_factor) and ann_factor > 0):
        raise ValueError(f"ann_factor={ann_factor!r} is not finite and > 0")
    if not np.isfinite(risk_free):
        raise ValueError(f"risk_free={risk_free!r} is not finite")
    _check_sweep_arrays((("returns", R, ("row", "asset")), ("W", W, ("portfolio", "asset"))))
    sums = np.zeros(P, _ffi.SWEEP_PERF_SUMS_DTYPE)
    stats = np.zeros(P, _ffi.SWEEP_PERF_STATS_DTYPE)
    if P:
        ctx = default_context(device)
        _ffi.check(_ffi.lib().mcp_sweep_historical_perf(ctx._h, N, R.shape[0], P, _ffi.ptr(R), _ffi.ptr(W), float(risk_free),
                                                        float(ann_factor), _ffi.ptr(sums), _ffi.ptr(stats)))
    out = {k: np.ascontiguousarray(stats[k]) for k in PERFORMANCE_KEYS}
    if raw:
        out.update((k, np.ascontiguousarray(sums[k])) for k in ("n", "n_neg", "S", "S_neg", "M2", "M2_neg", "prod", "mdd"))
    return out


RESAMPLED_KEYS = ("port_return", "port_std", "sharpe", "var_95", "cvar_95")      # the order of scores_out (SPEC.md 5.25)
RESAMPLED_CRITERIA = {"Monte Carlo": "sharpe", "VaR": "var_95", "CVaR": "cvar_95"}  # the order of opt_out; the largest score wins


def _check_resample(n_rows, n_replicates, block, replicate_begin):
    if n_rows < 2:
        raise ValueError(f"returns must have at least 2 rows for a sample deviation, got {n_rows}")
    if n_rows > _ffi.MCP_SWEEP_MAX_ROWS:
        raise ValueError(f"returns has {n_rows} rows, the resampled sweep takes at most {_ffi.MCP_SWEEP_MAX_ROWS}")
    if not 0 <= n_replicates <= _ffi.MCP_SWEEP_MAX_REPLICATES:
        raise ValueError(f"n_replicates={n_replicates!r} outside [0, {_ffi.MCP_SWEEP_MAX_REPLICATES}]")
    if not block >= 1:
        raise ValueError(f"block={block!r} must be >= 1 (or inf)")
    if not 0 <= replicate_begin <= 2 ** 64 - 1 - n_replicates:
        raise ValueError(f"replicate_begin={replicate_begin!r} + n_replicates={n_replicates} leaves [0, 2^64)")


def resample_counts(n_rows, n_replicates=1000, block=1.0, seed=0, replicate_begin=0):
    """The row counts [B, R] (uint16) of the replicates of `score_resampled`, on the host (`mcp_sweep_boot_counts`, no device):
    `np.repeat(np.arange(R), counts[b])` is replicate b's resample, up to the order of its rows."""
    n_rows, n_replicates, replicate_begin = int(n_rows), int(n_replicates), int(replicate_begin)
    _check_resample(n_rows, n_replicates, block, replicate_begin)
    out = np.zeros((n_replicates, n_rows), np.uint16)
    _ffi.check(_ffi.lib().mcp_sweep_boot_counts(int(seed) & (2 ** 64 - 1), replicate_begin, n_replicates, n_rows, float(block),
                                                _ffi.ptr(out)))
    return out


def score_resampled(R, W, rf, annual_factor=12, alpha=0.95, n_replicates=1000, block=1.0, seed=0, replicate_begin=0, device=0,
                    counts=False):
    """All rows of W scored on `n_replicates` stationary-block-bootstrap resamples of the rows of R, on the GPU (SPEC.md 5.25) -> dict
    of float64 [P, B] arrays port_return, port_std, sharpe, var_95, cvar_95 (all five from the resampled series `R[j] @ w`: mean and
    sample deviation times `annual_factor`, NumPy's percentile, the tail mean) and `opt`: {"Monte Carlo", "VaR", "CVaR"} -> int32 [B],
    the first portfolio with the largest sharpe / var_95 / cvar_95 of each replicate.  Replicate `replicate_begin + b` resamples the
    rows that path `replicate_begin + b` of `simulate_bootstrap(seed=, block=)` walks over R steps; `block` is the mean block length
    (1: the i.i.d. bootstrap, inf: one circular block).  counts=True adds `counts` [B, R], how often each row was drawn.  R and W must
    be finite, as for `score_portfolios`."""
    W = np.ascontiguousarray(W, np.float64)
    if W.ndim != 2:
        raise ValueError(f"W must be a [P, N] matrix, got shape {W.shape}")
    P, N = W.shape
    R = np.ascontiguousarray(R, np.float64)
    if R.ndim != 2 or R.shape[1] != N:
        raise ValueError(f"returns must be an [R, {N}] matrix like the {N} columns of W, got shape {R.shape}")
    B, begin = int(n_replicates), int(replicate_begin)
    _check_resample(R.shape[0], B, block, begin)
    if not (np.isfinite(annual_factor) and annual_factor > 0):
        raise ValueError(f"annual_factor={annual_factor!r} is not finite and > 0")
    if not np.isfinite(rf):
        raise ValueError(f"rf={rf!r} is not finite")
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha={alpha!r} outside (0, 1)")
    if P * B > 2 ** 27:
        raise ValueError(f"{P} portfolios x {B} replicates exceed 2^27 scores per figure: score the replicates in ranges")
    _check_sweep_arrays((("returns", R, ("row", "asset")), ("W", W, ("portfolio", "asset"))))
    scores = np.zeros((5, P, B), np.float64)
    opt = np.zeros((3, B), np.int32)
    cnt = np.zeros((B, R.shape[0]), np.uint16) if counts else None
    if P and B:
        ctx = default_context(device)
        _ffi.check(_ffi.lib().mcp_sweep_resampled(ctx._h, N, R.shape[0], P, _ffi.ptr(R), _ffi.ptr(W), float(rf), float(annual_factor),
                                                  float(alpha), int(seed) & (2 ** 64 - 1), begin, B, float(block), _ffi.ptr(scores),
                                                  _ffi.ptr(opt), _ffi.ptr(cnt)))
    elif counts and B:
        cnt = resample_counts(R.shape[0], B, block, seed, begin)
    out = {k: scores[i] for i, k in enumerate(RESAMPLED_KEYS)}
    out["opt"] = {m: opt[i] for i, m in enumerate(RESAMPLED_CRITERIA)}
    if counts:
        out["counts"] = cnt
    return out


def resample_summary(scores, W, point=None, levels=(2.5, 97.5)):
    """What the replicates of `score_resampled` say, in host NumPy.  Per figure of RESAMPLED_KEYS a dict of `mean` [P] (over the
    replicates), `se` [P] (the bootstrap standard error, ddof = 1; NaN for fewer than 2 replicates) and `interval` [len(levels), P]
    (the percentile interval at `levels`); per criterion of `scores["opt"]` a dict of `wins` [P] (replicates won, summing to B),
    `win_share` [P] and `resampled_weights` [N] = the mean over the replicates of W[opt] (Michaud's resampled portfolio).  `point`:
    the index of a full-sample optimum, or a dict criterion -> index; adds `point`, `point_win_share` and `point_top5_share` -- the
    share of replicates in which fewer than ceil(P / 20) portfolios score above it -- to the criteria it names."""
    W = np.asarray(W, np.float64)
    P = W.shape[0]
    out = {}
    for k in RESAMPLED_KEYS:
        x = np.asarray(scores[k], np.float64)
        if x.ndim != 2 or x.shape[0] != P:
            raise ValueError(f"scores[{k!r}] must be a [{P}, B] matrix like the {P} rows of W, got shape {x.shape}")
        B = x.shape[1]
        if B < 1:
            raise ValueError("a summary needs at least one replicate")
        se = x.std(axis=1, ddof=1) if B > 1 else np.full(P, np.nan)
        out[k] = {"mean": x.mean(axis=1), "se": se, "interval": np.percentile(x, list(levels), axis=1)}
    points = point if isinstance(point, dict) else {m: point for m in scores["opt"]}
    for m, opt in scores["opt"].items():
        opt = np.asarray(opt)
        wins = np.bincount(opt, minlength=P).astype(np.int64)
        o = {"wins": wins, "win_share": wins / len(opt), "resampled_weights": W[opt].mean(axis=0)}
        at = points.get(m)
        if at is not None:
            x = np.asarray(scores[RESAMPLED_CRITERIA[m]], np.float64)
            above = (x > x[int(at)][None, :]).sum(axis=0)
            o.update(point=int(at), point_win_share=float(o["win_share"][int(at)]),
                     point_top5_share=float((above < max(1, -(-P // 20))).mean()))
        out[m] = o
    return out


def run_resampled_sweep(returns_df, method="Monte Carlo", n_portfolios=2500, min_weights=None, max_weights=None, user_rf=3.0,
                        annual_factor=12, seed=None, alpha=0.95, device=0, n_replicates=1000, block=1.0, resample_seed=0):
    """`run_sweep` for one of "Monte Carlo" | "VaR" | "CVaR" | "MPT", and how far its optimum can be trusted: the tuple of `run_sweep`
    plus `resample_summary` of `score_resampled` on the same weights, with the sweep's optimum as the summary's `point` under the
    method's own criterion (MPT: the Sharpe ratio).  The weights are drawn by `run_sweep` itself and the resampling draws nothing from
    NumPy, so the global stream is left where `run_sweep` leaves it; the replicates are keyed by `resample_seed` alone."""
    if method not in ("Monte Carlo", "VaR", "CVaR", "MPT"):
        raise ValueError(f"unknown method {method!r} for a resampled sweep")
    risks, rets, W, metric, opt = run_sweep(returns_df, method, n_portfolios, min_weights, max_weights, user_rf, annual_factor, seed,
                                            alpha, device)
    R = sweep_inputs(returns_df, annual_factor)[0]
    scores = score_resampled(R, W, user_rf, annual_factor, alpha, n_replicates, block, resample_seed, 0, device)
    criterion = "Monte Carlo" if method == "MPT" else method
    return risks, rets, W, metric, opt, resample_summary(scores, W, point={criterion: opt})


def select_optimum(method, metrics):
    """`opt_crit` of app.py:672-676 applied as at app.py:747 (the VaR/CVaR arrays hold -var, -cvar).  The EXTRA_METHODS take the
    largest finite score (for a drawdown the one closest to 0), the first index on a tie; a NaN or infinite score -- one negative
    return, a lost first row -- is no candidate."""
    if method == "Equal Weight":
        return 0
    if len(metrics) == 0:
        raise ValueError("no portfolio satisfied the weight constraints (the reference raises here too, Q8)")
    if method in EXTRA_METHODS:
        m = np.asarray(metrics, np.float64)
        ok = np.isfinite(m)
        if not ok.any():
            raise ValueError(f"no portfolio has a finite {_EXTRA_METRIC[method]}")
        return int(np.argmax(np.where(ok, m, -np.inf)))
    return int(np.argmax(metrics)) if _METRIC[method] == "sharpe" else int(np.argmin(metrics))


def run_sweep(returns_df, method="Monte Carlo", n_portfolios=2500, min_weights=None, max_weights=None,
              user_rf=3.0, annual_factor=12, seed=None, alpha=0.95, device=0, risk_free=0.0):
    """One method of the loop at app.py:682-722 -> (all_risks, all_returns, all_weights, all_metrics, opt_idx).

    `seed` (if given) seeds NumPy's global legacy RNG first; pass None to continue the current stream,
    which is how the reference's four random methods follow each other (Q7).

    The EXTRA_METHODS draw their weights exactly as "Monte Carlo" does and return the same tuple: risks and returns from
    `score_portfolios`, all_metrics the criterion of `score_performance` at `risk_free` (in `sortino_ratio`'s units, annual; only
    these methods read it -- `user_rf` keeps its meaning for the analytic Sharpe)."""
    if method not in METHODS and method not in EXTRA_METHODS:
        raise ValueError(f"unknown method {method!r}")
    R, mean, cov = sweep_inputs(returns_df, annual_factor)
    N = R.shape[1]
    if seed is not None:
        np.random.seed(seed)
    if method == "Equal Weight":
        w = np.ones(N) / N                                                      # app.py:686
        lo = np.zeros(N) if min_weights is None else np.asarray(min_weights, float)
        hi = np.ones(N) if max_weights is None else np.asarray(max_weights, float)
        W = w[None, :] if (np.all(w >= lo) and np.all(w <= hi)) else np.empty((0, N))
    else:
        W = draw_weights(N, n_portfolios, min_weights, max_weights)
    s = score_portfolios(R, mean, cov, W, user_rf, alpha, device)
    if method in EXTRA_METHODS:
        metric = score_performance(R, W, risk_free, annual_factor, device)[_EXTRA_METRIC[method]]
        return s["port_std"], s["port_return"], W, metric, select_optimum(method, metric)
    metric = {"sharpe": s["sharpe"], "var_95": -s["var_95"], "cvar_95": -s["cvar_95"]}[_METRIC[method]]   # app.py:717
    if method == "Equal Weight" and len(metric) == 0:
        raise IndexError("equal weights violate the constraints (the reference fails at app.py:749, Q8)")
    return s["port_std"], s["port_return"], W, metric, select_optimum(method, metric)


def run_all_methods(returns_df, n_portfolios=2500, min_weights=None, max_weights=None, user_rf=3.0,
                    annual_factor=12, seed=None, investment_amount=10000.0, device=0):
    """The whole loop of app.py:682-783 (without the plots): dict method -> results, RNG stream shared (Q7)."""
    if seed is not None:
        np.random.seed(seed)
    out = {}
    for m in METHODS:
        risks, rets, W, metrics, opt = run_sweep(returns_df, m, n_portfolios, min_weights, max_weights, user_rf,
                                                 annual_factor, None, 0.95, device)
        out[m] = {"all_risks": risks, "all_returns": rets, "all_weights": W, "all_metrics": metrics, "opt_idx": opt,
                  "weights": W[opt], "dollar_vals": allocation(W[opt], investment_amount)}
    return out


def allocation(weights, investment_amount=10000.0):
    """app.py:763-764."""
    return np.asarray(weights, float) * investment_amount


def capital_allocation_line(all_risks, all_metrics, user_rf, opt_idx, n=100):
    """The CAL overlay of the 'MPT' method, app.py:737-746 (x, y in percent)."""
    sharpe_star = all_metrics[opt_idx]
    cal_x = np.linspace(0, all_risks.max() * 1.3 * 100, n)
    return cal_x, user_rf * 100 + sharpe_star * cal_x


def efficient_frontier(mean_returns, cov_matrix, points=200, min_weights=None, max_weights=None, device=0):
    """app.py:265-284 (never called by the reference's UI): (results[3, points], weights[points, N]);
    rows of results: std, return, return/std (no risk-free rate here, unlike the live loop).  Keeps Q9:
    if all 100 draws of a point violate the constraints, the last rejected draw is used."""
    mean = np.ascontiguousarray(np.asarray(mean_returns, np.float64))
    cov = np.ascontiguousarray(np.asarray(cov_matrix, np.float64))
    N = len(mean)
    ones = np.ones(N)
    W = np.empty((points, N))
    for i in range(points):
        for _ in range(100):
            w = np.random.dirichlet(ones, size=1)[0]
            if min_weights is not None and not np.all(w >= min_weights):
                continue
            if max_weights is not None and not np.all(w <= max_weights):
                continue
            break
        W[i] = w
    results = np.zeros((3, points))
    if points:
        s = score_portfolios(np.zeros((1, N)), mean, cov, W, 0.0, 0.95, device)
        results[0], results[1], results[2] = s["port_std"], s["port_return"], s["sharpe"]
    return results, W

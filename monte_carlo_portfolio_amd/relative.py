"""Benchmark-relative statistics of a call's portfolios (SPEC.md 5.23).

simulate_paths(benchmark=b) compares every row of `weights` with row b on the same paths: the device reduces the pair to one raw record
of sums per row (include/mcport_relative.h, mcp_relative_sums) and stores the active returns, whose order statistics the select
chain takes; the library finishes the sums on the host.  `finish` restates those formulas in Python floats, operation for operation,
so that the tests compare bits.  `relative_law` gives the exact figures of a one-step Gaussian pair, which the law tests are held to.
"""
from __future__ import annotations

import math
import operator

import numpy as np

from . import _ffi

SUM_FIELDS = tuple(n for n, _ in _ffi.RELATIVE_SUMS_DTYPE.descr)
STAT_FIELDS = tuple(n for n, _ in _ffi.RELATIVE_STATS_DTYPE.descr)
COUNT_FIELDS = SUM_FIELDS[:5]
# the mcp_stats fields of the record of the active returns, by the names of the 'active' block
ACTIVE_FIELDS = (("mean", "mean"), ("std", "std"), ("var", "var"), ("cvar", "cvar"), ("n_tail", "n_tail"), ("worst", "min"), ("best", "max"))


def check_benchmark(benchmark, n_portfolios):
    """simulate_paths' `benchmark` -> None (not asked for) or the benchmark's row of `weights` as an int in [0, n_portfolios).
    ValueError for a bool, a float, a string, an array and a row outside the range."""
    if benchmark is None:
        return None
    if isinstance(benchmark, (bool, np.bool_)) or not isinstance(benchmark, (int, np.integer)):
        raise ValueError(f"benchmark must be None or an integer row of weights, got {benchmark!r}")
    b = operator.index(benchmark)
    if not 0 <= b < int(n_portfolios):
        raise ValueError(f"benchmark={b} is not a row of the {int(n_portfolios)} portfolios")
    return b


def finish(sums, pivot, bench_pivot):
    """mcp_relative_finish in Python floats: the finished record (a dict of STAT_FIELDS) of one raw record `sums` (a mapping or a
    record of SUM_FIELDS) about the row's pivot and the benchmark's.  One binary64 operation per operation, in SPEC.md 5.23's order."""
    n_i, nu_i, no_i, nup_i, ndn_i = (int(sums[f]) for f in COUNT_FIELDS)
    e1, e2, k1, b1, k2, b2, kb, u1, u2, up_k, up_b, down_k, down_b = (float(sums[f]) for f in SUM_FIELDS[5:])
    ck, cb = float(pivot), float(bench_pivot)
    n, nu, no = float(n_i), float(nu_i), float(no_i)
    el = e1 / n if n_i else 0.0
    active_mean = (ck - cb) + el
    q = e2 - e1 * el
    tracking_error = math.sqrt((q if q > 0.0 else 0.0) / (n - 1.0)) if n_i >= 2 else 0.0
    kl = k1 / n if n_i else 0.0
    bl = b1 / n if n_i else 0.0
    vk, vb, ckb = k2 - k1 * kl, b2 - b1 * bl, kb - k1 * bl
    beta = ckb / vb if vb > 0.0 else 0.0
    mk, mb = ck + kl, cb + bl
    vv = vk * vb if vk > 0.0 and vb > 0.0 else 0.0
    rho = ckb / math.sqrt(vv) if vv > 0.0 else 0.0
    return {"active_mean": active_mean, "tracking_error": tracking_error,
            "information_ratio": active_mean / tracking_error if tracking_error > 0.0 else 0.0,
            "p_under": nu / n if n_i else 0.0, "p_over": no / n if n_i else 0.0,
            "mean_underperformance": u1 / nu if nu_i else 0.0,
            "relative_downside_deviation": math.sqrt(u2 / n) if n_i else 0.0,
            "beta": beta, "alpha": mk - beta * mb, "correlation": 1.0 if rho > 1.0 else (-1.0 if rho < -1.0 else rho),
            "up_capture": up_k / up_b if nup_i and up_b != 0.0 else 0.0,
            "down_capture": down_k / down_b if ndn_i and down_b != 0.0 else 0.0,
            "pivot": ck, "bench_pivot": cb}


def relative_law(mu, cov, w, w_b):
    """The exact figures of a one-step Gaussian pair: r ~ N(mu, cov), x = w.r against x_b = w_b.r, so a = (w - w_b).r is normal.
    -> {active_mean, tracking_error, information_ratio, p_under = Phi(-IR), beta = cov(x, x_b) / var(x_b), correlation, alpha =
    E x - beta E x_b, var_k, var_b}.  ValueError when the benchmark's variance or the tracking error is not positive."""
    mu, cov = np.asarray(mu, np.float64), np.asarray(cov, np.float64)
    w, wb = np.asarray(w, np.float64), np.asarray(w_b, np.float64)
    d = w - wb
    var_a, var_k, var_b, c = float(d @ cov @ d), float(w @ cov @ w), float(wb @ cov @ wb), float(w @ cov @ wb)
    if not (var_b > 0.0 and var_a > 0.0 and var_k > 0.0):
        raise ValueError("relative_law needs a portfolio, a benchmark and an active return of positive variance")
    am, te = float(d @ mu), math.sqrt(var_a)
    ir = am / te
    beta = c / var_b
    return {"active_mean": am, "tracking_error": te, "information_ratio": ir, "p_under": 0.5 * math.erfc(ir / math.sqrt(2.0)),
            "beta": beta, "correlation": c / math.sqrt(var_k * var_b), "alpha": float(w @ mu) - beta * float(wb @ mu),
            "var_k": var_k, "var_b": var_b}


def active_to_dict(rec) -> dict:
    """The 'active' record of one portfolio: the mcp_stats fields of the stored Y = fl32(1 + a) over x = Y - 1 (SPEC.md 5.23) -- var
    is the relative VaR (the active return at the 100 (1 - alpha) percent point of the paths), cvar the mean of the active returns up
    to it, worst and best the extremes."""
    return {name: (int if field == "n_tail" else float)(rec[field]) for name, field in ACTIVE_FIELDS}


def relative_blocks(stats, sums, bench, active_stats, hz_stats=None, active=None):
    """The 'relative' block of every portfolio from the arrays of Context._call: the finished record's fields as floats, 'benchmark',
    the raw record under 'sums', 'active' (active_to_dict; with `active`, the stored binary32 row Y = 1 + a under 'y') and, with
    horizons, 'horizons': one dict of the finished fields per horizon."""
    blocks = []
    for k in range(stats.shape[0]):
        blk = {f: float(stats[k][f]) for f in STAT_FIELDS}
        blk["benchmark"] = int(bench)
        blk["sums"] = {f: (int if f in COUNT_FIELDS else float)(sums[k][f]) for f in SUM_FIELDS}
        blk["active"] = active_to_dict(active_stats[k])
        if active is not None:
            blk["active"]["y"] = active[k]
        if hz_stats is not None:
            blk["horizons"] = [dict({f: float(hz_stats[h, k][f]) for f in STAT_FIELDS}, benchmark=int(bench)) for h in range(hz_stats.shape[0])]
        blocks.append(blk)
    return blocks

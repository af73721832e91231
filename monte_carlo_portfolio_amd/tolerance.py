"""Tolerance-band rebalancing (SPEC.md 4.18 / 5.18): look at the portfolio on a schedule, trade only when an asset is out of its band.

simulate_paths(tolerance=...) and simulate_bootstrap(tolerance=...) review every path every `rebalance` steps and trade it back to the
weights when a watched asset's weight is off target by its tolerance or more; per path they count the trades and add up the turnover.
tolerance_bands builds the usual tables (absolute points, a share of the target, the "5/25" rule), and band_law is the exact
probability that the one review of a two-step walk trades, what the simulated trade count is checked against.
"""
from __future__ import annotations

import math

import numpy as np

from . import _ffi


def tolerance_bands(weights, absolute=None, relative=None):
    """The tolerance table of `weights` ([N] -> [N], [K, N] -> [K, N], float64): min(absolute, relative |w_i|) with both given, one of
    them alone otherwise.  With `relative` alone an asset of weight 0 has no band to leave and is not watched (+inf).  The "5/25" rule
    is absolute=0.05, relative=0.25.  ValueError without either, or for a negative or non-finite number."""
    w = np.abs(np.asarray(weights, np.float64))
    if w.ndim not in (1, 2):
        raise ValueError(f"weights must be [N] or [K, N], got shape {w.shape}")
    if absolute is None and relative is None:
        raise ValueError("tolerance_bands needs absolute, relative or both")
    for name, v in (("absolute", absolute), ("relative", relative)):
        if v is not None and (isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating))
                              or not math.isfinite(v) or v < 0):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    if relative is None:
        return np.full(w.shape, float(absolute))
    rel = float(relative) * w
    if absolute is None:
        return np.where(w == 0.0, np.inf, rel)
    return np.minimum(float(absolute), rel)


def check_tolerance(tolerance, levels, shape, n_steps, every):
    """SPEC.md 4.18 / 5.18 argument rules -> (tol float32 [K, N], levels float64 [L]).  tolerance: a number, [N] or [K, N], every entry
    >= 0 or +inf (not watched), rounded to binary32; levels: at most MCP_MAX_LEVELS percentages in [0, 100]; shape: (K, N) of the
    weights.  ValueError otherwise."""
    K, N = shape
    try:
        t = np.asarray(tolerance, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"tolerance must be a number, [N] or [K, N], got {tolerance!r}") from None
    if isinstance(tolerance, (bool, np.bool_)) or t.dtype == object or t.ndim > 2 or (t.ndim >= 1 and t.shape[-1] != N) or (t.ndim == 2 and t.shape[0] != K):
        raise ValueError(f"tolerance must be a number, [N] or [K, N] for weights [{K}, {N}], got shape {t.shape}")
    if not np.all(t >= 0.0):
        raise ValueError("tolerance entries must be >= 0, or inf for an asset that is not watched")
    with np.errstate(over="ignore"):
        tol = np.ascontiguousarray(np.broadcast_to(t, (K, N)), np.float32)
    try:
        lv = np.atleast_1d(np.asarray(levels, np.float64)).ravel()
    except (TypeError, ValueError):
        raise ValueError(f"tolerance_levels must be percentages in [0, 100], got {levels!r}") from None
    if lv.size > _ffi.MCP_MAX_LEVELS or not np.all((lv >= 0.0) & (lv <= 100.0)):
        raise ValueError(f"tolerance_levels must be at most {_ffi.MCP_MAX_LEVELS} percentages in [0, 100], got {levels!r}")
    if n_reviews(n_steps, every) > _ffi.MCP_MAX_LIFE_STEPS:
        raise ValueError(f"tolerance needs at most {_ffi.MCP_MAX_LIFE_STEPS} reviews, got {n_reviews(n_steps, every)}")
    return tol, lv


def n_reviews(n_steps, every):
    """The reviews of a walk of n_steps steps reviewed every `every` steps (SPEC.md 4.18): the steps s with s mod every == 0 and
    s < n_steps."""
    T, e = int(n_steps), int(every)
    return (T - 1) // e if 1 <= e < T else 0


def turnover_to_dict(rec) -> dict:
    """The turnover fields of one mcp_stats record over x = Y - 1 (SPEC.md 5.18), shifted back by +1: var is the turnover at the
    100 (1 - alpha) percent point of the paths, cvar the mean of the turnovers up to it."""
    return {"mean": float(rec["mean"]) + 1.0, "std": float(rec["std"]), "var": float(rec["var"]) + 1.0, "cvar": float(rec["cvar"]) + 1.0,
            "n_tail": int(rec["n_tail"]), "min": float(rec["min"]) + 1.0, "max": float(rec["max"]) + 1.0,
            "x_lo": float(rec["x_lo"]) + 1.0, "x_hi": float(rec["x_hi"]) + 1.0}


def tolerance_blocks(out, tol, every, levels, store, n):
    """The 'tolerance' block of every portfolio from the outputs of Context.simulate_banded: the rule (every, n_reviews, table), the
    trade counts (exact histogram, mean, order statistics {level: trades}), the turnover record and, with `store`, the per-path
    trades and turnover.  n: the paths of the call."""
    blocks = []
    for k in range(out.trade_hist.shape[0]):
        blk = {"every": int(every), "n_reviews": int(out.trade_hist.shape[1]) - 1, "table": tol[k].astype(np.float64),
               "trades": {"hist": out.trade_hist[k], "mean": int(out.trade_sum[k]) / n,
                          "q": {float(q): int(v) for q, v in zip(levels, out.trade_q[k])}},
               "turnover": turnover_to_dict(out.turnover_stats[k])}
        if store:
            blk["trades"]["paths"] = out.trades[k]
            blk["turnover"]["paths"] = out.turnover[k]
        blocks.append(blk)
    return blocks


def band_law(w, mu, sigma, tol):
    """The probability that the one review of a walk of 2 steps reviewed every step trades, exact, for one risky asset of weight w
    beside cash, a step return r ~ N(mu, sigma^2) and the tolerance tol.  After one step the asset's weight is w (1 + r) / (1 + w r),
    off target by w (1 - w) |r| / (1 + w r); the review trades iff w (1 - w) |r| >= tol (1 + w r), that is
    r >= tol / (w (1 - w) - tol w) or r <= -tol / (w (1 - w) + tol w): two normal tails.  (1 + w r > 0 is taken for granted: the
    other side has a probability far below any sampling error at the volatilities of returns.)  The rounding of the step itself moves
    the thresholds by a few ulps."""
    w, mu, sigma, tol = (float(v) for v in (w, mu, sigma, tol))
    a = abs(w * (1.0 - w))
    if not sigma > 0.0:
        raise ValueError(f"sigma must be > 0, got {sigma!r}")
    if tol == 0.0:
        return 1.0
    if math.isinf(tol):
        return 0.0

    def upper(x):                       # P(r >= x)
        return 0.5 * math.erfc((x - mu) / (sigma * math.sqrt(2.0)))
    p = 0.0
    up, dn = a - tol * w, a + tol * w
    if up > 0.0:
        p += upper(tol / up)
    if dn > 0.0:
        p += 1.0 - upper(-tol / dn)
    return p

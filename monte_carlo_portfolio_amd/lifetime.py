"""The time of ruin (SPEC.md 4.17 / 5.17): how long the money lasts.

simulate_paths(lifetime=True) and simulate_bootstrap(lifetime=True) count, per path, the steps that ended with money left; this module
turns the exact histogram of that count into the survival curve, and lifetime_law is the exact one-step ruin probability on Gaussian
draws, what the simulated histogram is checked against.
"""
from __future__ import annotations

import math

import numpy as np

from . import _ffi


def check_lifetime(lifetime, levels, n_steps):
    """SPEC.md 4.17 / 5.17 argument rules -> None (no lifetime) or the float64 [L] levels.  lifetime: True or False; levels: at most
    MCP_MAX_LEVELS percentages in [0, 100]; n_steps at most MCP_MAX_LIFE_STEPS.  ValueError for anything else."""
    if not isinstance(lifetime, (bool, np.bool_)):
        raise ValueError(f"lifetime must be True or False, got {lifetime!r}")
    if not lifetime:
        return None
    try:
        lv = np.atleast_1d(np.asarray(levels, np.float64)).ravel()
    except (TypeError, ValueError):
        raise ValueError(f"lifetime_levels must be percentages in [0, 100], got {levels!r}") from None
    if lv.size > _ffi.MCP_MAX_LEVELS or not np.all((lv >= 0.0) & (lv <= 100.0)):
        raise ValueError(f"lifetime_levels must be at most {_ffi.MCP_MAX_LEVELS} percentages in [0, 100], got {levels!r}")
    if int(n_steps) > _ffi.MCP_MAX_LIFE_STEPS:
        raise ValueError(f"lifetime needs n_steps <= {_ffi.MCP_MAX_LIFE_STEPS}, got {n_steps!r}")
    return lv


def survival_curve(hist, n=None):
    """S(s) = #{l >= s} / n for s = 0 .. T from the histogram hist[s] = #{l == s} (float64 [T + 1]; [K, T + 1] -> [K, T + 1]): S(0) = 1
    and 1 - S(h) is the ruin probability at horizon h.  The counts are summed from the top as integers; one division per entry.  n:
    the number of paths, by default the histogram's total."""
    h = np.asarray(hist, np.uint64)
    if h.ndim not in (1, 2) or h.shape[-1] < 1:
        raise ValueError(f"hist must be [T + 1] or [K, T + 1], got shape {h.shape}")
    n = h.sum(axis=-1, keepdims=True) if n is None else np.asarray(n, np.uint64)
    if np.any(n == 0):
        raise ValueError("an empty histogram has no survival curve")
    at_least = np.flip(np.cumsum(np.flip(h, -1), axis=-1, dtype=np.uint64), -1)
    return at_least.astype(np.float64) / n.astype(np.float64)


def lifetime_blocks(out, levels, store, n):
    """The 'lifetime' block of every portfolio from the outputs of Context.simulate_lifetime: the exact histogram, the survival curve,
    the restricted mean lifetime life_sum / n, the order statistics {level: steps}, the paths ruined inside the horizon and, with
    `store`, the lifetime of every path.  n: the paths of the call."""
    blocks = []
    for k in range(out.life_hist.shape[0]):
        hist = out.life_hist[k]
        blk = {"histogram": hist, "survival": survival_curve(hist, n), "mean": int(out.life_sum[k]) / n,
               "quantiles": {float(q): int(v) for q, v in zip(levels, out.life_q[k])}, "n_ruined": n - int(hist[-1])}
        if store:
            blk["steps"] = out.life[k]
        blocks.append(blk)
    return blocks


def lifetime_law(mu, cov, weights, withdrawal, v0=1.0):
    """P(l = 0) at n_steps = 1 under a constant withdrawal on Gaussian draws, exact: the step stores U = v0 (1 + rho) - c with rho ~
    N(w.mu, w' cov w), and the path is ruined when U <= 0, so P = Phi((c / v0 - 1 - w.mu) / sqrt(w' cov w)).  weights [N] -> a float;
    [K, N] -> float64 [K].  mu, the weights, c and v0 enter as the kernels see them, rounded to binary32; the rounding of the step
    itself moves the threshold by a few ulps of v0, far below any sampling error."""
    W = np.atleast_2d(np.asarray(weights, np.float32)).astype(np.float64)
    m = W @ np.asarray(mu, np.float32).astype(np.float64).ravel()
    s = np.sqrt(np.einsum("ki,ij,kj->k", W, np.asarray(cov, np.float64), W))
    z = (float(np.float32(withdrawal)) / float(np.float32(v0)) - 1.0 - m) / s
    p = np.array([0.5 * math.erfc(-float(x) / math.sqrt(2.0)) for x in z])
    return float(p[0]) if np.asarray(weights).ndim == 1 else p

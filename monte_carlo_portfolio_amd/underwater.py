"""The time under water (SPEC.md 4.20 / 5.20): how long a path stays below its running peak.

simulate_paths(drawdown=True, underwater=True) counts, per path, the longest run of consecutive steps strictly below the high-water
mark and the steps since the last peak at the horizon; this module turns the two exact histograms into the 'underwater' block, and
spell_law gives the two distribution-free probabilities that the simulated histograms are checked against.
"""
from __future__ import annotations

import math

import numpy as np

from . import _ffi


def check_underwater(levels, n_steps):
    """SPEC.md 4.20 / 5.20 argument rules -> the float64 [L] levels: at most MCP_MAX_LEVELS percentages in [0, 100]; n_steps at most
    MCP_MAX_LIFE_STEPS.  ValueError for anything else."""
    try:
        lv = np.atleast_1d(np.asarray(levels, np.float64)).ravel()
    except (TypeError, ValueError):
        raise ValueError(f"underwater_levels must be percentages in [0, 100], got {levels!r}") from None
    if lv.size > _ffi.MCP_MAX_LEVELS or not np.all((lv >= 0.0) & (lv <= 100.0)):
        raise ValueError(f"underwater_levels must be at most {_ffi.MCP_MAX_LEVELS} percentages in [0, 100], got {levels!r}")
    if int(n_steps) > _ffi.MCP_MAX_LIFE_STEPS:
        raise ValueError(f"underwater needs n_steps <= {_ffi.MCP_MAX_LIFE_STEPS}, got {n_steps!r}")
    return lv


def underwater_blocks(out, levels, store, n):
    """The 'underwater' block of every portfolio from the outputs of Context.simulate_underwater: for the longest spell m ('longest')
    and the spell at the horizon c_T ('current') the exact histogram 'hist' (uint64 [n_steps + 1], #{. == s}), the 'mean' in steps
    (sum / n) and the order statistics 'levels' {level: steps}; 'p_under_water_at_end' = 1 - hist_c[0] / n; with `store`, 'longest'
    and 'current' also carry the counter of every path as 'steps' (uint32 [n_paths]).  n: the paths of the call."""
    blocks = []
    for k in range(out.uw_longest_hist.shape[0]):
        blk = {}
        for r, (name, hist, per_path) in enumerate((("longest", out.uw_longest_hist[k], out.uw_longest),
                                                    ("current", out.uw_current_hist[k], out.uw_current))):
            blk[name] = {"hist": hist, "mean": int(out.uw_sums[k, r]) / n,
                         "levels": {float(q): int(v) for q, v in zip(levels, out.uw_q[k, r])}}
            if store:
                blk[name]["steps"] = per_path[k]
        blk["p_under_water_at_end"] = 1.0 - int(out.uw_current_hist[k, 0]) / n
        blocks.append(blk)
    return blocks


def spell_law(T):
    """(P(m = 0), P(c_T = 0)) of a walk of T >= 1 steps whose increments are independent, symmetric about zero and continuous, under
    log compounding with zero drift (S_t a symmetric random walk), whatever the increments' law:
      P(m = 0)   = 2^-(T - 1): the path never falls below its peak exactly when every step after the first goes up;
      P(c_T = 0) = C(2 (T - 1), T - 1) / 4^(T - 1): S_T is the maximum of S_1 .. S_T exactly when the T - 1 partial sums of the
                   reversed increments are all non-negative -- Sparre Andersen's theorem gives that probability for any symmetric
                   continuous step.
    Both are exact rationals with a power of two below, so the floats returned are exact for T <= 27."""
    T = int(T)
    if T < 1:
        raise ValueError(f"spell_law needs T >= 1, got {T!r}")
    n = T - 1
    return 0.5 ** n, math.comb(2 * n, n) / 4.0 ** n

"""Downside and shape statistics of a simulated distribution (SPEC.md 5.22).

simulate_paths(downside=True | tau) reduces x on the device to one raw record of sums per row (include/mcport_downside.h,
mcp_downside_sums) and the library finishes it on the host; `finish` restates those formulas in Python floats, operation for
operation, so that the tests compare bits.  `normal_law` gives the exact figures of a normal x, which the law tests are held to.
"""
from __future__ import annotations

import math

import numpy as np

from . import _ffi

SUM_FIELDS = tuple(n for n, _ in _ffi.DOWNSIDE_SUMS_DTYPE.descr)
STAT_FIELDS = tuple(n for n, _ in _ffi.DOWNSIDE_STATS_DTYPE.descr)


def check_downside(downside):
    """simulate_paths' `downside` -> None (not asked for), True (the threshold is rf) or the threshold as a float.  ValueError for
    False, a string, an array or a number that is not finite."""
    if downside is None:
        return None
    if isinstance(downside, (bool, np.bool_)):
        if downside:
            return True
        raise ValueError("downside must be None, True (the threshold is rf) or a finite threshold, got False")
    if isinstance(downside, (str, bytes)) or not np.isscalar(downside):
        raise ValueError(f"downside must be None, True (the threshold is rf) or a finite threshold, got {downside!r}")
    try:
        tau = float(downside)
    except (TypeError, ValueError):
        raise ValueError(f"downside must be None, True (the threshold is rf) or a finite threshold, got {downside!r}") from None
    if not math.isfinite(tau):
        raise ValueError(f"downside must be None, True (the threshold is rf) or a finite threshold, got {downside!r}")
    return tau


def finish(sums, tau, pivot):
    """mcp_downside_finish in Python floats: the finished record (a dict of STAT_FIELDS) of one raw record `sums` (a mapping or a
    record of SUM_FIELDS) about `pivot`, at the threshold `tau`.  One binary64 operation per operation, in SPEC.md 5.22's order."""
    n_i, nb_i = int(sums["n"]), int(sums["n_below"])
    s1, s2, s3, s4 = (float(sums[f]) for f in ("s1", "s2", "s3", "s4"))
    b1, b2, l1, l2, u1 = (float(sums[f]) for f in ("b1", "b2", "l1", "l2", "u1"))
    tau, pivot = float(tau), float(pivot)
    n, nb = float(n_i), float(nb_i)
    dl = s1 / n if n_i else 0.0
    mean = pivot + dl
    dl2 = dl * dl
    m2 = s2 - s1 * dl
    m3 = (s3 - (3.0 * dl) * s2) + ((2.0 * n) * dl) * dl2
    m4 = ((s4 - (4.0 * dl) * s3) + (6.0 * dl2) * s2) - ((3.0 * n) * dl2) * dl2
    if m2 > 0.0:
        v = m2 / n
        skewness = (m3 / n) / (v * math.sqrt(v))
        excess_kurtosis = (n * m4) / (m2 * m2) - 3.0
    else:
        skewness = excess_kurtosis = 0.0
    if nb_i >= 2:
        q = b2 - (b1 * b1) / nb
        downside_std = math.sqrt((q if q > 0.0 else 0.0) / (nb - 1.0))
    else:
        downside_std = math.nan if nb_i == 1 else 1e-4
    ex = mean - tau
    sortino = _div(ex, downside_std)
    downside_deviation = math.sqrt(l2 / n) if n_i else 0.0
    return {"mean": mean, "skewness": skewness, "excess_kurtosis": excess_kurtosis, "downside_std": downside_std, "sortino": sortino,
            "downside_deviation": downside_deviation, "sortino_target": ex / downside_deviation if downside_deviation > 0.0 else 0.0,
            "p_below": nb / n if n_i else 0.0, "mean_shortfall": l1 / nb if nb_i else 0.0,
            "omega": math.inf if l1 == 0.0 else u1 / (-l1), "pivot": pivot}


def _div(a, b):
    """a / b as IEEE binary64 has it where Python raises: a zero divisor."""
    if b == 0.0:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def normal_law(mu, sigma, tau):
    """The exact figures of x ~ N(mu, sigma^2) at the threshold tau: p_below = Phi(z), the lower partial moments
    l1 = E[(x - tau) 1{x < tau}] and l2 = E[(x - tau)^2 1{x < tau}] (the semivariance about tau), u1 = E[(x - tau) 1{x > tau}],
    omega = u1 / -l1, downside_deviation = sqrt(l2), and omega_se1: the delta-method standard error of the sample Omega times
    sqrt(n).  With z = (tau - mu) / sigma, phi and Phi the standard normal density and distribution:
        l1 = -sigma (z Phi(z) + phi(z)),       l2 = sigma^2 ((1 + z^2) Phi(z) + z phi(z)),   u1 = (mu - tau) - l1."""
    mu, sigma, tau = float(mu), float(sigma), float(tau)
    if not sigma > 0.0:
        raise ValueError(f"normal_law needs sigma > 0, got {sigma!r}")
    z = (tau - mu) / sigma
    phi = math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    Phi = 0.5 * math.erfc(-z / math.sqrt(2.0))
    l1 = -sigma * (z * Phi + phi)
    l2 = sigma * sigma * ((1.0 + z * z) * Phi + z * phi)
    u1 = (mu - tau) - l1
    u2 = sigma * sigma * (1.0 + z * z) - l2                # E[(x - tau)^2 1{x > tau}]
    omega = math.inf if l1 == 0.0 else u1 / -l1
    # Omega = U / D with U = mean (x - tau)+ and D = mean (tau - x)+: var U = u2 - u1^2, var D = l2 - l1^2, cov(U, D) = -u1 (-l1)
    du, dd = u1, -l1
    var = (u2 - du * du) / (dd * dd) + du * du * (l2 - dd * dd) / dd ** 4 + 2.0 * du * (du * dd) / dd ** 3
    return {"p_below": Phi, "l1": l1, "l2": l2, "u1": u1, "omega": omega, "downside_deviation": math.sqrt(l2),
            "mean_shortfall": l1 / Phi if Phi > 0.0 else 0.0, "omega_se1": math.sqrt(var)}


def downside_blocks(stats, sums, tau, hz_stats=None):
    """The 'downside' block of every portfolio from the arrays of Context._call: the finished record's fields as floats, 'threshold',
    the raw record under 'sums' and, with horizons, 'horizons': one such dict (without sums) per horizon."""
    blocks = []
    for k in range(stats.shape[0]):
        blk = {f: float(stats[k][f]) for f in STAT_FIELDS}
        blk["threshold"] = float(tau)
        blk["sums"] = {f: (int if f.startswith("n") else float)(sums[k][f]) for f in SUM_FIELDS}
        if hz_stats is not None:
            blk["horizons"] = [dict({f: float(hz_stats[h, k][f]) for f in STAT_FIELDS}, threshold=float(tau)) for h in range(hz_stats.shape[0])]
        blocks.append(blk)
    return blocks

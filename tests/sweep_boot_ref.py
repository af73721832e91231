"""NumPy restatement of the resampled historical sweep (SPEC.md 5.25, include/mcport_sweep_boot.h; test helper, not a test module):
the six steps as written, binary64, looping over the rows r and the sorted positions k and vectorised over the portfolios and the
replicates.  The rows of a replicate come from bootstrap_ref.boot_indices (replicate g walks what path g walks), the order of a
portfolio's series from np.argsort(kind="stable")."""
from __future__ import annotations

import math

import numpy as np

from bootstrap_ref import boot_indices

FIGURES = ("port_return", "port_std", "sharpe", "var_95", "cvar_95")
CRITERIA = ("Monte Carlo", "VaR", "CVaR")


def percentile_rank(n, alpha):
    """mcp_percentile_rank: the ranks and the weight of np.percentile(x, (1 - alpha) * 100) among n values, method 'linear'."""
    q = (1.0 - alpha) * 100.0 / 100.0
    vi = float(n - 1) * q
    if vi >= float(n - 1):
        return n - 1, n - 1, 0.0
    if vi < 0.0:
        return 0, 0, 0.0
    fl = math.floor(vi)
    return int(fl), int(fl) + 1, vi - fl


def replicate_rows(seed, replicate_begin, n_replicates, n_rows, block):
    """[R, B] the rows j_t of the replicates replicate_begin .. +B: path g of SPEC.md 2.1 with T = R steps on R rows."""
    g = np.uint64(replicate_begin) + np.arange(int(n_replicates), dtype=np.uint64)       # the range does not wrap (an argument rule)
    return boot_indices(int(seed), g, n_rows, n_rows, block)


def replicate_counts(seed, replicate_begin, n_replicates, n_rows, block):
    """[B, R] uint16 c_g[r] = #{t : j_t = r}."""
    idx = replicate_rows(seed, replicate_begin, n_replicates, n_rows, block)
    out = np.zeros((int(n_replicates), n_rows), np.uint16)
    for q in range(int(n_replicates)):
        out[q] = np.bincount(idx[:, q], minlength=n_rows)
    return out


def series(returns, W):
    """[P, R] y_p[r] = sum_i returns[r, i] W[p, i], i ascending from 0.0, multiply then add."""
    returns = np.asarray(returns, np.float64)
    W = np.atleast_2d(np.asarray(W, np.float64))
    y = np.zeros((W.shape[0], returns.shape[0]))
    for i in range(returns.shape[1]):
        y = y + returns[:, i][None, :] * W[:, i][:, None]
    return y


def score(returns, W, rf, ann, alpha, counts, parts=False):
    """Steps 1 and 3 to 6 on the counts [B, R] -> dict of the five figures as [P, B] float64 arrays and "opt": criterion -> int32 [B].
    parts=True adds S, M2, lo and the tail's ts, tc."""
    y = series(returns, W)                                      # [P, R]
    P, R = y.shape
    c = np.asarray(counts).astype(np.float64)                   # [B, R]; (double)c is exact
    B = c.shape[0]
    ci = np.asarray(counts).astype(np.int64)
    ann, rf = np.float64(ann), np.float64(rf)
    S = np.zeros((P, B))
    for r in range(R):
        S = S + c[:, r][None, :] * y[:, r][:, None]
    m = S / np.float64(R)
    M2 = np.zeros((P, B))
    for r in range(R):
        d = y[:, r][:, None] - m
        M2 = M2 + c[:, r][None, :] * (d * d)
    port_return = m * ann
    port_std = np.sqrt(M2 / np.float64(R - 1) * ann)
    with np.errstate(invalid="ignore", divide="ignore"):
        sharpe = np.where(port_std > 0.0, (port_return - rf) / port_std, 0.0)

    perm = np.argsort(y, axis=1, kind="stable")                 # ties by row; -0.0 == +0.0
    ys = np.take_along_axis(y, perm, axis=1)                    # [P, R]
    rank_lo, rank_hi, gamma = percentile_rank(R, alpha)
    cum = np.zeros((P, B), np.int64)
    lo, a, b = np.zeros((P, B)), np.zeros((P, B)), np.zeros((P, B))
    for k in range(R):
        before = cum
        cum = cum + ci.T[perm[:, k]]                            # [P, B]
        v = np.broadcast_to(ys[:, k][:, None], (P, B))
        lo = np.where((before == 0) & (cum > 0), v, lo)
        a = np.where((before <= rank_lo) & (cum > rank_lo), v, a)
        b = np.where((before <= rank_hi) & (cum > rank_hi), v, b)
    diff = b - a
    var = a + diff * np.float64(gamma)                          # numpy _lerp
    if gamma >= 0.5:
        var = b - diff * (np.float64(1.0) - np.float64(gamma))
    ts, tc = np.zeros((P, B)), np.zeros((P, B), np.int64)
    for k in range(R):
        v = np.broadcast_to(ys[:, k][:, None], (P, B))
        inside = v <= var
        ck = ci.T[perm[:, k]]
        ts = np.where(inside, ts + ck.astype(np.float64) * v, ts)
        tc = np.where(inside, tc + ck, tc)
    cvar = ts / tc.astype(np.float64)
    cvar = np.where(cvar < lo, lo, cvar)                        # min(max(., lo), var), by compares
    cvar = np.where(cvar > var, var, cvar)
    out = dict(zip(FIGURES, (port_return, port_std, sharpe, var, cvar)))
    out["opt"] = {name: np.argmax(out[key], axis=0).astype(np.int32)          # np.argmax: the first maximum
                  for name, key in zip(CRITERIA, ("sharpe", "var_95", "cvar_95"))}
    if parts:
        out.update(S=S, M2=M2, lo=lo, ts=ts, tc=tc, y=y, perm=perm)
    return out


def resampled(returns, W, rf, ann, alpha, seed, replicate_begin, n_replicates, block, parts=False):
    counts = replicate_counts(seed, replicate_begin, n_replicates, np.asarray(returns).shape[0], block)
    out = score(returns, W, rf, ann, alpha, counts, parts)
    out["counts"] = counts
    return out


# The bootstrap law at block = 1 (one asset at weight 1, ann = 1): the rows of a replicate are R independent draws from the R observed
# values, so the replicate's mean has variance ((R - 1) / R) s^2 / R with s the sample deviation (ddof = 1) of the observed values.
# The standard deviation of B near-normal values has relative standard error 1 / sqrt(2 B); the margin is five of them.
LAW = {"R": 64, "B": 4096, "seed": 20240607, "data_seed": 11, "margin": 5.0 / math.sqrt(2 * 4096)}


def law_input():
    rs = np.random.RandomState(LAW["data_seed"])
    return 0.03 * rs.standard_normal((LAW["R"], 1)) + 0.004, np.ones((1, 1))


def law_ratio(returns, port_return):
    """std over the replicates of port_return (ann = 1) over sqrt((R - 1) / R) s / sqrt(R)."""
    R = returns.shape[0]
    s = returns[:, 0].std(ddof=1)
    return float(np.asarray(port_return).std(ddof=1) / (math.sqrt((R - 1) / R) * s / math.sqrt(R)))

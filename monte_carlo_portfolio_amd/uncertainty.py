"""Drift uncertainty, the estimation risk of the mean (SPEC.md 2.7 / 4.21 / 5.21): the covariance of a sample mean, the three forms
of simulate_paths(drift_uncertainty=...) as one binary32 factor, the result block and the exact laws the simulated moments are
checked against.

The drift mu that a walk compounds is a sample mean over R observed rows; its covariance is cov / R.  With drift_uncertainty every
path draws its own drift once, m = mu + M g with g ~ N(0, I) and M M' that covariance, and walks on it: the sampling variance of the
terminal log value grows like T, the variance from not knowing the drift like T^2.
"""
from __future__ import annotations

import math

import numpy as np


def drift_cov(returns) -> np.ndarray:
    """The covariance of the sample mean of `returns` (a DataFrame or an [R, N] array): the sample covariance (ddof = 1) over R,
    binary64 [N, N].  ValueError for R < 2 or values that are not finite."""
    vals = returns.to_numpy() if hasattr(returns, "to_numpy") else returns
    rows = np.asarray(vals, np.float64)
    if rows.ndim == 1:
        rows = rows[:, None]
    if rows.ndim != 2 or rows.shape[0] < 2:
        raise ValueError(f"drift_cov needs at least 2 rows of returns [R, N], got shape {rows.shape}")
    if not np.all(np.isfinite(rows)):
        raise ValueError("drift_cov needs finite returns")
    return np.atleast_2d(np.cov(rows, rowvar=False, ddof=1)) / rows.shape[0]


def _finite32(a) -> bool:
    with np.errstate(over="ignore"):
        return bool(np.all(np.isfinite(a))) and bool(np.all(np.isfinite(np.asarray(a, np.float64).astype(np.float32))))


def drift_factor(spec, cov, chol=None) -> np.ndarray:
    """The binary32 lower-triangular factor M [N, N] of SPEC.md 4.21 from one of the three forms of `drift_uncertainty`:
      a positive scalar n_obs        M = fl32(chol64(cov) / sqrt(n_obs)): `cov` is the covariance of one step's returns, the drift its
                                     mean over n_obs observed steps
      an [N, N] matrix               the covariance of the drift itself, factored in binary64 (it must be positive definite)
      ("factor", M)                  a lower-triangular factor, used as given after np.tril and the cast; zeros are allowed
    ValueError for anything else, for a matrix of another shape or one that is not positive definite, and for values that are not
    finite before or after rounding to binary32.  `chol`: the factor of one step's covariance where the caller has it instead of `cov`
    (simulate_paths(chol=...)); n_obs then scales it."""
    cov = np.atleast_2d(np.asarray(cov if chol is None else chol, np.float64))
    n = cov.shape[0]
    msg = f"drift_uncertainty must be a positive number of observations, an ({n}, {n}) covariance of the drift or ('factor', M), got {spec!r}"
    if isinstance(spec, (bool, np.bool_)) or isinstance(spec, (str, bytes)) or spec is None:
        raise ValueError(msg)
    if isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], str):
        if spec[0] != "factor":
            raise ValueError(msg)
        m = np.asarray(spec[1], np.float64)
        if m.ndim == 0:
            m = np.full((n, n), float(m))
        if m.shape != (n, n) or not _finite32(m):
            raise ValueError(f"drift_uncertainty ('factor', M): M must be a finite ({n}, {n}) matrix, in binary32 too")
        return np.ascontiguousarray(np.tril(m).astype(np.float32))
    if isinstance(spec, (int, float, np.integer, np.floating)):
        n_obs = float(spec)
        if not (math.isfinite(n_obs) and n_obs > 0.0):
            raise ValueError(msg)
        try:
            low = np.linalg.cholesky(cov) if chol is None else np.tril(cov)
        except np.linalg.LinAlgError:
            raise ValueError("drift_uncertainty=n_obs needs a positive definite cov") from None
        m = low / math.sqrt(n_obs)
    else:
        c = np.asarray(spec, np.float64)
        if c.shape != (n, n) or not np.all(np.isfinite(c)):
            raise ValueError(msg)
        try:
            m = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError("drift_uncertainty: the covariance of the drift is not positive definite (a singular one goes as "
                             "('factor', M))") from None
    if not _finite32(m):
        raise ValueError("drift_uncertainty: the factor is not finite in binary32")
    return np.ascontiguousarray(np.tril(m).astype(np.float32))


def check_drift_uncertainty(spec, cov, chol=None):
    """None (no uncertainty) or drift_factor(spec, cov, chol)."""
    return None if spec is None else drift_factor(spec, cov, chol)


def _abc(mu, chol, M, w):
    """a = |L'w|^2, b = |M'w|^2, c = w.mu in binary64 from the binary32 values as rounded."""
    mu64 = np.asarray(mu, np.float32).astype(np.float64)
    L64 = np.tril(np.asarray(chol, np.float32)).astype(np.float64)
    M64 = np.tril(np.asarray(M, np.float32)).astype(np.float64)
    w64 = np.asarray(w, np.float32).astype(np.float64)
    return float(np.sum((L64.T @ w64) ** 2)), float(np.sum((M64.T @ w64) ** 2)), float(w64 @ mu64)


def drift_law(mu, chol, M, w, T, v0=1.0) -> dict:
    """The informative laws of SPEC.md 4.21 for one portfolio w after T steps, from the binary32 inputs as rounded: a = |L'w|^2,
    b = |M'w|^2, c = w.mu; the path's portfolio drift w.m is N(c, b) (drift_std = sqrt(b)); under log compounding S_T is N(T c, T a +
    T^2 b) (log_mean, log_var, and log_variance_share = T b / (a + T b), the part of log_var that is estimation risk); under simple
    compounding E[V_T] = v0 sum_j C(T, j) (1 + c)^(T - j) b^(j/2) E[g^j], E[g^j] = (j - 1)!! for even j and 0 for odd j
    (simple_mean)."""
    T = int(T)
    if T < 1:
        raise ValueError(f"T must be >= 1, got {T}")
    a, b, c = _abc(mu, chol, M, w)
    mean = 0.0
    for j in range(0, T + 1, 2):
        dfact = 1.0
        for i in range(j - 1, 0, -2):
            dfact *= i
        mean += math.comb(T, j) * (1.0 + c) ** (T - j) * b ** (j // 2) * dfact
    return {"a": a, "b": b, "c": c, "drift_std": math.sqrt(b), "log_mean": T * c, "log_var": T * a + T * T * b,
            "log_variance_share": T * b / (a + T * b) if a + T * b > 0 else 0.0, "simple_mean": float(np.float32(v0)) * mean}


def uncertainty_blocks(chol, M, W, n_steps, steps=None):
    """The 'drift_uncertainty' block of every portfolio: drift_std = sqrt(b_k) from the binary32 M, in binary64, log_variance_share =
    T b_k / (a_k + T b_k) and, with horizons, the same share per horizon."""
    out = []
    for w in np.atleast_2d(W):
        a, b, _ = _abc(np.zeros(np.asarray(chol).shape[0]), chol, M, w)
        share = lambda h: h * b / (a + h * b) if a + h * b > 0 else 0.0   # noqa: E731
        blk = {"drift_std": math.sqrt(b), "log_variance_share": share(int(n_steps))}
        if steps is not None:
            blk["horizon_log_variance_share"] = np.array([share(int(h)) for h in steps], np.float64)
        out.append(blk)
    return out

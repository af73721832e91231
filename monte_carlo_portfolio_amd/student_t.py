"""fit_student_t_dof: the degrees of freedom of the multivariate Student-t draws (SPEC.md 2.2) that best explain observed return
rows.  Host-side binary64 NumPy (plus math.lgamma); nothing here is on the GPU path.

The scale of the t law is tied to the sample covariance, S = Sigma_hat (nu - 2) / nu, so that simulate_paths(..., dof=nu) with
the same mean and covariance simulates the covariance the Gaussian call does: only the shape of the tails is fitted.
"""
from __future__ import annotations

import math

import numpy as np

from . import _ffi


def _rows(returns) -> np.ndarray:
    vals = returns.to_numpy() if hasattr(returns, "to_numpy") else returns
    X = np.asarray(vals, np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if X.ndim != 2:
        raise ValueError(f"returns must be an [R, N] matrix, got shape {X.shape}")
    R, N = X.shape
    if N < 1:
        raise ValueError("returns have no columns")
    bad = ~np.isfinite(X).all(axis=1)
    if bad.any():
        raise ValueError(f"returns hold NaN or infinite values in {int(bad.sum())} rows (first: row {int(np.argmax(bad))}); drop them first")
    if R < N + 2:
        raise ValueError(f"need at least N + 2 = {N + 2} return rows for {N} assets, got {R}")
    return X


def _dofs(dofs) -> list[int]:
    out = []
    for d in dofs:
        if isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, float, np.integer, np.floating)) or not float(d).is_integer():
            raise ValueError(f"dofs must be integers in [3, {_ffi.MCP_MAX_T_DOF}], got {d!r}")
        if not 3 <= d <= _ffi.MCP_MAX_T_DOF:
            raise ValueError(f"dofs must be integers in [3, {_ffi.MCP_MAX_T_DOF}], got {d!r}")
        out.append(int(d))
    if not out:
        raise ValueError("dofs is empty")
    return sorted(set(out))


class _Fit:
    """The sample moments of the rows: m, Sigma_hat (ddof = 1, as returns_df.cov()), log det Sigma_hat and the squared
    Mahalanobis distances d2_hat = (x - m)' Sigma_hat^-1 (x - m) of every row."""

    def __init__(self, X: np.ndarray):
        self.R, self.N = X.shape
        m = X.mean(axis=0)
        cov = np.atleast_2d(np.cov(X, rowvar=False, ddof=1))
        try:
            L = np.linalg.cholesky(cov)
        except np.linalg.LinAlgError as e:
            raise ValueError(f"the sample covariance of the returns is not positive definite: {e}") from None
        self.logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
        y = np.linalg.solve(L, (X - m).T)
        self.d2 = np.sum(y * y, axis=0)

    def loglik(self, nu: int) -> float:
        """l(nu) = sum_rows [lgamma((nu+N)/2) - lgamma(nu/2) - (N/2) log(nu pi) - 1/2 log det S - ((nu+N)/2) log1p(d^2/nu)] with
        S = Sigma_hat (nu-2)/nu, so d^2/nu = d2_hat/(nu-2) and log det S = log det Sigma_hat + N log((nu-2)/nu)."""
        N, R = self.N, self.R
        c = (math.lgamma((nu + N) / 2.0) - math.lgamma(nu / 2.0) - 0.5 * N * math.log(nu * math.pi)
             - 0.5 * (self.logdet + N * math.log((nu - 2.0) / nu)))
        return R * c - 0.5 * (nu + N) * float(np.sum(np.log1p(self.d2 / (nu - 2.0))))


def student_t_loglik(returns, dof: int) -> float:
    """The log-likelihood l(nu) of the rows under the multivariate t with nu = dof degrees of freedom, location the sample mean
    and covariance the sample covariance (scale Sigma_hat (nu - 2) / nu), binary64."""
    (nu,) = _dofs([dof])
    return _Fit(_rows(returns)).loglik(nu)


def fit_student_t_dof(returns, dofs=range(3, _ffi.MCP_MAX_T_DOF + 1)) -> int:
    """The nu in `dofs` (integers in [3, 32]) that maximises the log-likelihood of the return rows under the multivariate
    Student-t whose mean is the sample mean and whose covariance is the sample covariance (ddof = 1); the smallest such nu on
    ties.  returns: DataFrame (returns_matrix(...)) or [R, N] array, finite, R >= N + 2.  The result is what
    simulate_paths(..., dof=nu) takes; 32 means no evidence of fat tails.  ValueError for non-finite rows, too few rows, a
    covariance that is not positive definite, or dofs outside [3, 32]."""
    cand = _dofs(dofs)
    fit = _Fit(_rows(returns))
    best, best_ll = cand[0], fit.loglik(cand[0])
    for nu in cand[1:]:
        ll = fit.loglik(nu)
        if ll > best_ll:
            best, best_ll = nu, ll
    return best

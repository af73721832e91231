"""fit_garch: the (alpha, beta, h0) of the scalar GARCH(1,1) on the covariance (SPEC.md 4.9) that best explain observed return rows.
Host-side binary64 NumPy; nothing here is on the GPU path.

The level of the model is tied to the sample moments: with the sample mean m and covariance Sigma_hat (ddof = 1), every row gives
d_t = (x_t - m)' Sigma_hat^-1 (x_t - m) / N, whose mean is (R - 1) / R; the variance ratio runs h_1 = 1, h_{t+1} = (1 - alpha - beta)
+ alpha d_t + beta h_t, and the Gaussian log-likelihood of the rows given the ratios is, up to a constant that does not depend on
(alpha, beta), l(alpha, beta) = -1/2 sum_t [N log h_t + N d_t / h_t].  So simulate_paths(..., garch=fit[:3]) with the same mean and
covariance simulates the covariance the Gaussian call does in the long run: only the dynamics of the variance are fitted.

The maximiser is a deterministic two-stage grid on multiples of 0.002 (alpha = i / 500, beta = j / 500, i, j >= 0, i + j <= 499):
the coarse stage visits the multiples of 0.02 (i, j multiples of 10), the fine stage every grid point within 0.02 of the coarse best
in both coordinates.  Ties go to the smaller alpha, then the smaller beta.

filter_rows: the rows de-volatilised with that variance path, for filtered historical simulation (SPEC.md 2.4; simulate_filtered).
With h_1 = 1 and h_{t+1} = (1 - alpha - beta) + alpha d_t + beta h_t, row t becomes the residual e_t = (x_t - m) / sqrt(h_t) and carries
the shock s_t = d_t / h_t, its own d in units of its fitted variance; h0 = h_{R+1}.  The recurrence takes d_t back as fl64(s_t h_t),
within an ulp of d_t, so that the shocks it returns reproduce h0 exactly.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .student_t import _Fit, _rows

GRID = 500            # the grid: alpha = i / GRID, beta = j / GRID
COARSE = 10           # the coarse stage: i, j multiples of COARSE (step 0.02)
MAX_SUM = GRID - 1    # i + j <= 499: alpha + beta <= 0.998


class GarchFit(NamedTuple):
    """fit_garch's result; fit[:3] is what simulate_paths(garch=...) takes."""
    alpha: float
    beta: float
    h0: float             # h_{R+1} at the optimum: the variance ratio of the step after the last row ("today's regime")
    loglik: float         # l(alpha, beta)
    loglik_iid: float     # l(0, 0)


class _Garch:
    """The per-row d_t of the rows (sample mean, sample covariance with ddof = 1) and the likelihood of the recurrence on them."""

    def __init__(self, X: np.ndarray):
        f = _Fit(X)
        self.R, self.N = f.R, f.N
        self.d = f.d2 / f.N

    def walk(self, alphas, betas):
        """-> (l [n], h_{R+1} [n]) for n pairs (alpha, beta), the recurrence run over the rows for all pairs at once."""
        a = np.atleast_1d(np.asarray(alphas, np.float64))
        b = np.atleast_1d(np.asarray(betas, np.float64))
        w = 1.0 - a - b
        h = np.ones_like(a)
        acc = np.zeros_like(a)
        for dt in self.d:
            acc += np.log(h) + dt / h
            h = w + a * dt + b * h
        return -0.5 * self.N * acc, h

    def logliks(self, alphas, betas):
        return self.walk(alphas, betas)[0]


class FilteredRows(NamedTuple):
    """filter_rows' result: what simulate_filtered takes.  mu [N], resid [R, N] and shock [R] are float32."""
    mu: np.ndarray
    resid: np.ndarray
    shock: np.ndarray
    alpha: float
    beta: float
    h0: float             # h_{R+1}: the variance ratio of the step after the last row


def _filter64(X: np.ndarray, alpha: float, beta: float):
    """-> (m [N], resid [R, N], shock [R], h [R], h0) in binary64: the recurrence of the module docstring over the rows."""
    g = _Garch(X)
    m = X.mean(axis=0)
    w = 1.0 - alpha - beta
    h = np.empty(g.R, np.float64)
    shock = np.empty(g.R, np.float64)
    ht = 1.0
    for t in range(g.R):
        h[t] = ht
        shock[t] = g.d[t] / ht
        ht = w + alpha * (shock[t] * ht) + beta * ht
    return m, (X - m) / np.sqrt(h)[:, None], shock, h, float(ht)


def filter_rows(returns, garch=None) -> FilteredRows:
    """The return rows filtered by the scalar GARCH(1,1) on the covariance (SPEC.md 2.4): the sample mean m, the residual rows
    (x_t - m) / sqrt(h_t) and the shocks d_t / h_t along the fitted variance path h_t, and h0 = h_{R+1}, today's level.  garch: None
    fits (alpha, beta) with fit_garch; otherwise (alpha, beta[, h0]) -- an h0 given is ignored, the path decides it.  alpha = beta = 0
    gives the centred rows and h0 = 1.  returns: as fit_garch.  -> FilteredRows(mu, resid, shock, alpha, beta, h0), the arrays
    rounded to float32.  ValueError for rows fit_garch refuses, alpha or beta negative or not finite, or alpha + beta >= 1."""
    X = _rows(returns)
    if garch is None:
        alpha, beta = fit_garch(X)[:2]
    else:
        if len(garch) < 2:
            raise ValueError("garch must be (alpha, beta) or (alpha, beta, h0)")
        alpha, beta = float(garch[0]), float(garch[1])
    if not (np.isfinite(alpha) and np.isfinite(beta) and alpha >= 0.0 and beta >= 0.0 and alpha + beta < 1.0):
        raise ValueError(f"garch alpha={alpha} and beta={beta} must be >= 0 with alpha + beta < 1")
    m, resid, shock, _, h0 = _filter64(X, alpha, beta)
    return FilteredRows(m.astype(np.float32), resid.astype(np.float32), shock.astype(np.float32), float(alpha), float(beta), h0)


def garch_loglik(returns, alpha: float, beta: float) -> float:
    """l(alpha, beta) of the module docstring for the rows, binary64."""
    return float(_Garch(_rows(returns)).logliks([alpha], [beta])[0])


def _best(g: _Garch, pairs):
    """The pair of `pairs` (sorted by i, then j) with the largest likelihood, the first one on ties."""
    ij = np.asarray(sorted(pairs), np.int64)
    ll = np.asarray(g.logliks(ij[:, 0] / GRID, ij[:, 1] / GRID), np.float64)
    if not np.all(np.isfinite(ll)):
        raise ValueError("the GARCH likelihood of the returns is not finite")
    k = int(np.argmax(ll))                  # the first maximum: the smaller alpha, then the smaller beta
    return int(ij[k, 0]), int(ij[k, 1])


def fit_garch(returns) -> GarchFit:
    """The (alpha, beta) on the grid of the module docstring that maximise the likelihood of the return rows under the scalar
    GARCH(1,1) on the covariance of SPEC.md 4.9, with the mean and covariance held at the sample's (ddof = 1), and h0 = h_{R+1}, the
    variance ratio the recurrence gives for the step after the last row.  returns: DataFrame (returns_matrix(...)) or [R, N] array,
    finite, R >= N + 2.  -> GarchFit(alpha, beta, h0, loglik, loglik_iid); alpha = beta = 0 (h0 = 1) means no evidence of
    volatility clustering.  ValueError for non-finite rows, too few rows or a covariance that is not positive definite."""
    g = _Garch(_rows(returns))
    ci, cj = _best(g, [(i, j) for i in range(0, MAX_SUM + 1, COARSE) for j in range(0, MAX_SUM + 1 - i, COARSE)])
    fi, fj = _best(g, [(i, j) for i in range(max(ci - COARSE, 0), ci + COARSE + 1) for j in range(max(cj - COARSE, 0), cj + COARSE + 1)
                       if i + j <= MAX_SUM])
    ll, h = g.walk([fi / GRID, 0.0], [fj / GRID, 0.0])
    return GarchFit(fi / GRID, fj / GRID, float(h[0]), float(ll[0]), float(ll[1]))

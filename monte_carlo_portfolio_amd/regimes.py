"""Two-regime Markov switching on the host (Hamilton 1989; SPEC.md 2.6 / 4.13 / 5.13): the law of the regime chain the path kernels
draw and of the step's portfolio return, and a Baum-Welch estimator of the model from return rows.  Binary64 NumPy; nothing here is
on the GPU path.

The kernels move the regime by comparing one uniform 32-bit word with a threshold, so the chain's law is a function of the
thresholds alone: regime_law works on p^ = thr / 2^32 (mcp_regime_consts), which makes every closed form below exact for what is
simulated.

fit_regimes is a two-state Gaussian hidden Markov model, x_t | s_t = s ~ N(mu_s, cov_s), fitted by Baum-Welch (EM) with the scaled
forward-backward recursions:
  start     deterministic: the rows whose squared Mahalanobis distance from the sample mean under the sample covariance (ddof = 1,
            as fit_garch's d_t) is above the median form regime 1, the others regime 0; means and covariances of the two groups,
            p01 and p10 from the transitions between consecutive rows' groups (floored at 1 / R), the initial row's regime from its
            group.
  E step    alpha_t ~ (alpha_{t-1} P) b_t scaled to sum 1, the scales' logs sum to the log-likelihood; beta_t backwards on the same
            scales; gamma_t and the expected transitions xi from them.
  M step    p01 = sum xi_01 / sum_{t<R} gamma_t(0), p10 likewise; mu_s and cov_s the gamma-weighted mean and (biased) covariance;
            the first row's regime probability gamma_1(1).  Full covariances; an eigenvalue of cov_s below RIDGE times the mean
            sample variance is raised to it (a ridge that is idle on rows that fill the space, so the steps stay exact EM steps and
            the log-likelihood cannot decrease).
  stop      after MAX_ITER iterations, or when the log-likelihood gains less than TOL.
  order     regime 1 is the one with the larger equal-weight variance 1' cov_s 1 / N^2; the fit is relabelled to that.
loglik_iid is the log-likelihood of one Gaussian with the sample mean and the biased sample covariance -- the same model with one
regime.  The two-regime model has q = N + N (N + 1) / 2 + 3 more parameters (a mean, a covariance, p01, p10 and the first row's
regime); no_evidence states the rule that calls a fit no better than one regime: loglik - loglik_iid <= (q / 2) log R, Schwarz's
criterion -- nothing is fitted to it but the count q and the number of rows.
"""
from __future__ import annotations

import collections
import math

import numpy as np

from . import _ffi
from .student_t import _Fit, _rows

RegimeFit = collections.namedtuple("RegimeFit", "p01 p10 mu0 cov0 mu1 cov1 start loglik loglik_iid")
RegimeLaw = collections.namedtuple("RegimeLaw", "p01 p10 start pi mean var pivots")

MAX_ITER = 200        # Baum-Welch iterations at most
TOL = 1e-6            # stop when an iteration gains less log-likelihood than this
RIDGE = 1e-10         # eigenvalue floor of a regime's covariance, in units of the mean sample variance


def used_probabilities(p01, p10, start):
    """(p^01, p^10, p^start): the probabilities the kernels really use, thr / 2^32 (SPEC.md 2.6)."""
    return tuple(float(v) for v in _ffi.regime_consts(p01, p10, start)[1])


def stationary(p01, p10):
    """P(regime 1) in the long run, p01 / (p01 + p10); 0 if both are 0."""
    return p01 / (p01 + p10) if p01 + p10 > 0 else 0.0


def occupancy_path(p01, p10, start, T):
    """pi_t(1) = (pi P^t)_1 for t = 0 .. T-1: the probability that step t walks in regime 1."""
    out = np.empty(int(T), np.float64)
    q = float(start)
    for t in range(int(T)):
        out[t] = q
        q = (1.0 - q) * p01 + q * (1.0 - p10)
    return out


def regime_law(regimes, mu, L, mu1, L1, W, T) -> RegimeLaw:
    """The law of the T steps of a regime call: `regimes` = (p01, p10, start) as asked for, mu / L and mu1 / L1 the binary32 drifts and
    lower Cholesky factors of regimes 0 and 1, W [K, N] (or [N]) the binary32 weights.  -> RegimeLaw(p01, p10, start: the p^ used;
    pi [T]: P(s_t = 1); mean [T, K] = E rho_t = sum_s pi_t(s) m_ks; var [T, K] = Var rho_t = sum_s pi_t(s) (sigma2_ks + m_ks^2) -
    (E rho_t)^2 with m_ks = w_k . mu^(s) and sigma2_ks = |L^(s)' w_k|^2; pivots [T, K]: c_k(h) of SPEC.md 5.13 for h = 1 .. T, the
    exact mean of x_h, by the recursion of mcp_regime_pivots -- expm1(h log1p(m)) where the portfolio walks on one drift m only),
    all binary64 from the binary32 inputs."""
    p01, p10, start = used_probabilities(*tuple(regimes)[:3])
    W64 = np.atleast_2d(np.asarray(W, np.float32)).astype(np.float64)
    m = []                                                               # m_ks [K] per regime, i ascending as the library sums it
    for v in (mu, mu1):
        v64 = np.asarray(v, np.float32).astype(np.float64).ravel() + 0.0
        acc = np.zeros(W64.shape[0])
        for i in range(v64.size):
            acc = acc + W64[:, i] * v64[i]
        m.append(acc)
    s2 = [np.sum((W64 @ np.tril(np.asarray(f, np.float32).astype(np.float64))) ** 2, axis=1) for f in (L, L1)]
    T = int(T)
    pi = occupancy_path(p01, p10, start, T)
    mean = (1.0 - pi)[:, None] * m[0][None, :] + pi[:, None] * m[1][None, :]
    second = (1.0 - pi)[:, None] * (s2[0] + m[0] ** 2)[None, :] + pi[:, None] * (s2[1] + m[1] ** 2)[None, :]
    d0, d1 = 1.0 + m[0], 1.0 + m[1]
    piv = np.zeros((T, W64.shape[0]), np.float64)
    v0, v1 = (1.0 - start) * d0, start * d1
    for h in range(1, T + 1):
        if h > 1:
            u0, u1 = v0 * (1.0 - p01) + v1 * p10, v0 * p01 + v1 * (1.0 - p10)
            v0, v1 = u0 * d0, u1 * d1
        c = (v0 + v1) - 1.0
        piv[h - 1] = np.where(np.isfinite(c), c, 0.0)
    only0, only1 = start == 0.0 and p01 == 0.0, start == 1.0 and p10 == 0.0
    for k in range(W64.shape[0]):                                        # one drift only: mcp_pivots' own formula (libm, as the library)
        if m[0][k] == m[1][k] or only0 or only1:
            mk = float(m[1][k] if only1 else m[0][k])
            for h in range(1, T + 1):
                c = math.expm1(h * math.log1p(mk)) if mk > -1.0 else 0.0
                piv[h - 1, k] = c if math.isfinite(c) else 0.0
    return RegimeLaw(p01, p10, start, pi, mean, second - mean ** 2, piv)


def _log_density(X, mu, cov):
    """log N(x_t; mu, cov) for every row, binary64."""
    N = X.shape[1]
    Lc = np.linalg.cholesky(cov)
    y = np.linalg.solve(Lc, (X - mu).T)
    return -0.5 * (N * np.log(2.0 * np.pi) + 2.0 * np.sum(np.log(np.diag(Lc))) + np.sum(y * y, axis=0))


def _forward(logb, p01, p10, init):
    """The scaled forward recursion -> (alpha [R, 2], scale [R], loglik): alpha_t = P(s_t | x_1..t), the row's density taken relative
    to its larger one so that nothing underflows."""
    R = logb.shape[0]
    top = logb.max(axis=1)
    b = np.exp(logb - top[:, None])
    P = np.array([[1.0 - p01, p01], [p10, 1.0 - p10]])
    alpha = np.empty((R, 2))
    scale = np.empty(R)
    q00, q01, q10, q11 = 1.0 - p01, p01, p10, 1.0 - p10
    a0, a1 = 1.0 - init, init
    rows = b.tolist()                                     # plain floats: the recursion is sequential, two numbers wide
    al, sc = [], []
    for t in range(R):
        if t:
            a0, a1 = a0 * q00 + a1 * q10, a0 * q01 + a1 * q11
        a0, a1 = a0 * rows[t][0], a1 * rows[t][1]
        c = a0 + a1
        a0, a1 = a0 / c, a1 / c
        al.append((a0, a1))
        sc.append(c)
    alpha[:], scale[:] = al, sc
    return alpha, scale, b, P, float(np.sum(np.log(scale)) + np.sum(top))


def regime_loglik(returns, p01, p10, mu0, cov0, mu1, cov1, init=None) -> float:
    """The log-likelihood of the rows under the two-state Gaussian HMM, by the forward filter fit_regimes uses.  init: P(regime 1 in
    the first row), default the stationary probability."""
    X = _rows(returns)
    logb = np.stack([_log_density(X, np.asarray(mu0, np.float64), np.atleast_2d(np.asarray(cov0, np.float64))),
                     _log_density(X, np.asarray(mu1, np.float64), np.atleast_2d(np.asarray(cov1, np.float64)))], axis=1)
    return _forward(logb, float(p01), float(p10), stationary(p01, p10) if init is None else float(init))[4]


def _moments(X, g, floor):
    """The g-weighted mean and biased covariance of the rows, eigenvalues below `floor` raised to it."""
    n = g.sum()
    mu = g @ X / n
    D = X - mu
    cov = (D * g[:, None]).T @ D / n
    lam, Q = np.linalg.eigh(cov)
    if lam[0] < floor:
        cov = (Q * np.maximum(lam, floor)) @ Q.T
    return mu, cov


def baum_welch(returns, max_iter=MAX_ITER, tol=TOL):
    """fit_regimes with its trace -> (RegimeFit, logliks): logliks[i] is the log-likelihood of the parameters iteration i started
    from, the last entry that of the parameters returned."""
    X = _rows(returns)
    R, N = X.shape
    f = _Fit(X)
    floor = RIDGE * float(np.mean(np.var(X, axis=0)))
    lab = (f.d2 > np.median(f.d2)).astype(np.float64)
    if lab.sum() < N + 1 or (1.0 - lab).sum() < N + 1:
        raise ValueError(f"need at least 2 (N + 1) = {2 * (N + 1)} return rows with distinct distances to start two regimes, got {R}")
    g = np.stack([1.0 - lab, lab], axis=1)
    par = [_moments(X, g[:, s], floor) for s in (0, 1)]
    n01 = float(np.sum((lab[:-1] == 0) & (lab[1:] == 1)))
    n10 = float(np.sum((lab[:-1] == 1) & (lab[1:] == 0)))
    p01 = max(n01, 1.0) / max(float(np.sum(lab[:-1] == 0)), 1.0)
    p10 = max(n10, 1.0) / max(float(np.sum(lab[:-1] == 1)), 1.0)
    p01, p10 = min(p01, 1.0), min(p10, 1.0)
    init = float(lab[0])
    init = min(max(init, 1.0 / R), 1.0 - 1.0 / R)
    trace = []
    for it in range(int(max_iter) + 1):
        logb = np.stack([_log_density(X, *par[0]), _log_density(X, *par[1])], axis=1)
        alpha, scale, b, P, ll = _forward(logb, p01, p10, init)
        trace.append(ll)
        if it == int(max_iter) or (it > 0 and trace[-1] - trace[-2] < tol):
            break
        beta = np.empty((R, 2))
        rows, sc = b.tolist(), scale.tolist()
        b0 = b1 = 1.0
        bl = [(b0, b1)]
        for t in range(R - 2, -1, -1):
            x0, x1 = rows[t + 1][0] * b0 / sc[t + 1], rows[t + 1][1] * b1 / sc[t + 1]
            b0, b1 = P[0, 0] * x0 + P[0, 1] * x1, P[1, 0] * x0 + P[1, 1] * x1
            bl.append((b0, b1))
        beta[:] = bl[::-1]
        gamma = alpha * beta
        gamma /= gamma.sum(axis=1, keepdims=True)
        xi = alpha[:-1, :, None] * P[None, :, :] * (b[1:] * beta[1:])[:, None, :] / scale[1:, None, None]     # [R-1, 2, 2]
        from0, from1 = gamma[:-1, 0].sum(), gamma[:-1, 1].sum()
        keep = (par, p01, p10, init)
        p01 = float(xi[:, 0, 1].sum() / from0) if from0 > 0 else p01
        p10 = float(xi[:, 1, 0].sum() / from1) if from1 > 0 else p10
        p01, p10 = min(max(p01, 0.0), 1.0), min(max(p10, 0.0), 1.0)
        init = float(gamma[0, 1])
        if gamma[:, 0].sum() < N + 1 or gamma[:, 1].sum() < N + 1:       # a regime ran empty: keep the last full model
            par, p01, p10, init = keep
            break
        par = [_moments(X, gamma[:, s], floor) for s in (0, 1)]
    ll = trace[-1]
    if np.sum(par[0][1]) > np.sum(par[1][1]):                            # order: regime 1 has the larger 1' cov 1
        par, p01, p10, alpha = [par[1], par[0]], p10, p01, alpha[:, ::-1]
    start = float(alpha[-1, 0] * p01 + alpha[-1, 1] * (1.0 - p10))
    covb = np.atleast_2d(np.cov(X, rowvar=False, ddof=0))
    ll_iid = float(np.sum(_log_density(X, X.mean(axis=0), covb)))
    fit = RegimeFit(float(p01), float(p10), par[0][0], par[0][1], par[1][0], par[1][1], min(max(start, 0.0), 1.0), float(ll), ll_iid)
    return fit, np.asarray(trace, np.float64)


def fit_regimes(returns) -> RegimeFit:
    """The two-state Gaussian hidden Markov model of the module docstring fitted to return rows [R, N] (a DataFrame or an array,
    finite, R >= N + 2).  -> RegimeFit(p01, p10, mu0, cov0, mu1, cov1, start, loglik, loglik_iid): regime 1 is the one with the larger
    equal-weight variance; start is the filtered probability of regime 1 after the last row moved one step on -- the analogue of
    fit_garch's h0, a fan that starts from today's regime; simulate_paths(fit.mu0, fit.cov0, w, regimes=(fit.p01, fit.p10, fit.mu1,
    fit.cov1, fit.start)) simulates the fit.  no_evidence(fit, R) says whether the rows support two regimes at all."""
    return baum_welch(returns)[0]


def extra_parameters(n_assets: int) -> int:
    """q: what the two-regime model fits on top of one Gaussian -- a mean, a covariance, p01, p10 and the first row's regime."""
    n = int(n_assets)
    return n + n * (n + 1) // 2 + 3


def no_evidence(fit: RegimeFit, n_rows: int) -> bool:
    """Schwarz's criterion on the likelihood-ratio count of extra parameters: True when loglik - loglik_iid <= (q / 2) log R, i.e.
    the rows are explained as well by one regime (use the Gaussian call then)."""
    q = extra_parameters(np.asarray(fit.mu0).size)
    return bool(fit.loglik - fit.loglik_iid <= 0.5 * q * np.log(float(n_rows)))

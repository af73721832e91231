"""NumPy restatement of SPEC.md 4.15 (test helper, not a test module): the floor rule -- CPPI with an exposure cap and a drawdown
ratchet -- on the per-step portfolio returns that garch_ref.py (Gaussian, Student-t and GARCH draws: the GARCH walk serves all
three) and jump_ref.py already form, in binary32 in the spec's order; np.fmin / np.fmax are IEEE minNum / maxNum, as fminf / fmaxf.
Per path-step it also reports the branch the exposure took and whether the ratchet bound.  Below it, a binary64 twin on NumPy's
own normals and the assertions of the law test, which the CPU suite runs on the twin and the GPU suite on the device's values."""
from __future__ import annotations

import numpy as np

from garch_ref import garch_rho
from jump_ref import simulate_jumps
from oracle.np_oracle import _fma32

E_ZERO, E_CUSHION, E_CAP = 0, 1, 2      # the branch of E: +0, fl32(m C), fl32(b V)


def consts(protect):
    """(floor binary32 [T + 1], m, b, rf, theta binary32) of protect = (floor [T + 1], multiplier, rate, cap, ratchet)."""
    floor, m, rate, cap, ratchet = protect
    return np.asarray(floor, np.float32), np.float32(m), np.float32(cap), np.float32(rate), np.float32(ratchet)


def rho_of(mu, chol, W, T, seed, paths, dof=None, garch=None, jumps=None):
    """rho [K, T, n] binary32, the step's portfolio return exactly as the twin kernel forms it."""
    if jumps is not None:
        return simulate_jumps(mu, chol, W, T, seed, paths, jumps)["rho"]
    return garch_rho(mu, chol, W, T, seed, paths, garch if garch is not None else (0.0, 0.0, 1.0), dof)[0]


def walk(rho, protect, v0=1.0, horizons=()):
    """SPEC.md 4.15 on rho [K, T, n] -> dict(V_T [K, n], q [K, n], V_h [H, K, n] or None, branch [K, T, n] int8, ratchet [K, T, n] bool,
    exposure [K, T, n] the share E / V held in the risky portfolio, binary64):
        F = fmax(S_t, fl32(theta M)); C = V - F; E = fmax(fmin(fl32(m C), fl32(b V)), +0); u = fma(V - E, rf, V); V = fma(E, rho, u);
        M = fmax(M, V); then the drawdown of SPEC.md 4.2 on V: P = fmax(P, V), q = fmin(q, V / P)."""
    S, m, b, rf, th = consts(protect)
    rho = np.asarray(rho, np.float32)
    K, T, n = rho.shape
    hz = [int(h) for h in horizons]
    V = np.full((K, n), v0, np.float32)
    M = V.copy()
    P = np.full((K, n), -np.inf, np.float32)
    q = np.ones((K, n), np.float32)
    branch = np.zeros((K, T, n), np.int8)
    ratchet = np.zeros((K, T, n), bool)
    exposure = np.zeros((K, T, n))
    Vh = np.empty((len(hz), K, n), np.float32) if hz else None
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(T):
            tm = (th * M).astype(np.float32)
            F = np.fmax(S[t], tm)
            ratchet[:, t] = tm > S[t]
            C = (V - F).astype(np.float32)
            mc, bv = (m * C).astype(np.float32), (b * V).astype(np.float32)
            E = np.fmax(np.fmin(mc, bv), np.float32(0)).astype(np.float32)
            branch[:, t] = np.where(E == 0, E_ZERO, np.where(mc <= bv, E_CUSHION, E_CAP))
            exposure[:, t] = E.astype(np.float64) / V.astype(np.float64)
            rest = (V - E).astype(np.float32)
            for k in range(K):
                u = _fma32(rest[k], np.full(n, rf, np.float32), V[k])
                V[k] = _fma32(E[k], rho[k, t], u)
            M = np.fmax(M, V)
            P = np.fmax(P, V)
            q = np.fmin(q, (V / P).astype(np.float32))
            if t + 1 in hz:
                Vh[hz.index(t + 1)] = V
    return {"V_T": V, "q": q.astype(np.float32), "V_h": Vh, "branch": branch, "ratchet": ratchet, "exposure": exposure}


def simulate_protected(mu, chol, W, T, seed, paths, protect, dof=None, garch=None, jumps=None, v0=1.0, horizons=()):
    """Chosen path ids (path_begin included) -> walk() on the draws' rho, with rho itself under "rho"."""
    rho = rho_of(mu, chol, W, T, seed, paths, dof, garch, jumps)
    out = walk(rho, protect, v0, horizons)
    out["rho"] = rho
    return out


def compounded_v0(v0, rate, T):
    """Anchor (b), m = 0: V = fma(V, rf, V), T times from fl32(v0)."""
    v, rf = np.array([v0], np.float32), np.array([rate], np.float32)
    for _ in range(T):
        v = _fma32(v, rf, v)
    return v[0]


def twin_values(mu, cov, w, T, n_paths, protect, seed, v0=1.0):
    """The binary64 twin of the rule on NumPy's own normals -> V_T [n_paths] of one portfolio `w`; protect as consts() takes it, its
    numbers entering as their binary32 roundings."""
    S, m, b, rf, th = (np.asarray(x, np.float64) for x in consts(protect))
    mu, w = np.asarray(mu, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    L = np.linalg.cholesky(np.asarray(cov, np.float64))
    rng = np.random.default_rng(seed)
    V = np.full(n_paths, float(np.float32(v0)))
    M = V.copy()
    for t in range(T):
        rho = (mu + rng.standard_normal((n_paths, mu.shape[0])) @ L.T) @ w
        F = np.maximum(S[t], th * M)
        E = np.maximum(np.minimum(m * (V - F), b * V), 0.0)
        V = E * rho + ((V - E) * rf + V)
        M = np.maximum(M, V)
    return V


def law_checks(VT, mean, var):
    """The assertions of the law test on V_T [n] (binary32 from the device or binary64 from twin_values) against protect_law's exact
    (mean, var): the sample mean within 5 standard errors of `mean`, the standard error sqrt(m2 / n); the sample variance (about
    `mean`) within 5 standard errors of `var`, the standard error from the sample's own fourth moment, sqrt((m4 - m2^2) / n).  5
    standard errors is the bound for two two-sided normal tests at a false-alarm rate below 1e-5; it is not fitted to any run.
    -> the two figures in standard errors, for printing."""
    d = np.asarray(VT, np.float64) - mean
    n = d.size
    d2 = d * d
    m2 = d2.mean()
    z_mean = d.mean() / np.sqrt(m2 / n)
    z_var = (m2 - var) / np.sqrt((np.mean(d2 * d2) - m2 * m2) / n)
    print("law: z_mean", z_mean, "z_var", z_var, "mean", d.mean() + mean, "want", mean, "var", m2, "want", var)
    assert abs(z_mean) < 5.0, (z_mean, d.mean() + mean, mean)
    assert abs(z_var) < 5.0, (z_var, m2, var)
    return {"z_mean": float(z_mean), "z_var": float(z_var)}

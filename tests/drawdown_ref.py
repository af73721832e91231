"""NumPy restatement of SPEC.md section 4 + 4.2 (test helper, not a test module): the per-step portfolio returns, the
terminal values and the per-path drawdown state q (simple) / d (log) of chosen path ids, in binary32 in the spec's order
(oracle.np_oracle.step_normals and _fma32), plus a binary64 twin of the per-step returns for metrics.max_drawdown."""
from __future__ import annotations

import numpy as np

from oracle.np_oracle import _fma32, step_normals


def drawdown_state(rho, compounding="simple", v0=1.0):
    """SPEC.md 4.2 on given per-step returns rho [T, n] (binary32): -> (V_T [n], q or d [n]), both binary32.
    simple: V = fma(V, rho, V), P = fmax(P, V), q = fmin(q, V / P)  (P from -inf, q from 1);
    log:    S = S + rho,        P = fmax(P, S), d = fmin(d, S - P)  (P from -inf, d from 0)."""
    rho = np.asarray(rho, np.float32)
    n = rho.shape[1] if rho.ndim == 2 else 1
    rho = rho.reshape(rho.shape[0], n)
    log = compounding == "log"
    V = np.full(n, 0.0 if log else v0, np.float32)
    P = np.full(n, -np.inf, np.float32)
    q = np.full(n, 0.0 if log else 1.0, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(rho.shape[0]):
            V = (V + rho[t]).astype(np.float32) if log else _fma32(V, rho[t], V)
            P = np.fmax(P, V)
            q = np.fmin(q, (V - P) if log else (V / P))
    return V, q.astype(np.float32)


def mdd_of(q, compounding="simple"):
    """binary64 max drawdown from q / d: (double)q - 1 or expm1((double)d)."""
    q = np.asarray(q, np.float32).astype(np.float64)
    return np.expm1(q) if compounding == "log" else q - 1.0


def simulate_paths_dd(mu, chol, W, n_steps, seed, paths, compounding="simple", v0=1.0):
    """Chosen path ids (global, path_begin included) of SPEC.md 4: -> dict(rho [K, T, n] binary32, rho64 [K, T, n] binary64
    simple per-step returns whose cumprod(1 + .) is the path's value relative to v0, V_T [K, n], q [K, n]) in the spec's
    order (r_i = mu_i + sum_j L_ij z_j, j ascending, fma; rho = sum_i w_i r_i, i ascending, fma)."""
    mu = np.asarray(mu, np.float32) + np.float32(0)
    L = np.tril(np.asarray(chol, np.float32))
    W = np.atleast_2d(np.asarray(W, np.float32))
    N, K = mu.shape[0], W.shape[0]
    paths = np.asarray(paths, np.uint64)
    n = paths.shape[0]
    rho = np.zeros((K, n_steps, n), np.float32)
    for t in range(n_steps):
        z = step_normals(seed, paths, t, N)[:, :N]
        r = np.empty((n, N), np.float32)
        for i in range(N):
            acc = np.full(n, mu[i], np.float32)
            for j in range(i + 1):
                acc = _fma32(np.full(n, L[i, j], np.float32), z[:, j], acc)
            r[:, i] = acc
        for k in range(K):
            acc = np.zeros(n, np.float32)
            for i in range(N):
                acc = _fma32(np.full(n, W[k, i], np.float32), r[:, i], acc)
            rho[k, t] = acc
    VT = np.empty((K, n), np.float32)
    q = np.empty((K, n), np.float32)
    for k in range(K):
        VT[k], q[k] = drawdown_state(rho[k], compounding, v0)
    rho64 = rho.astype(np.float64)
    if compounding == "log":
        rho64 = np.expm1(rho64)          # cumprod(1 + expm1(rho)) = exp(S_t)
    return {"rho": rho, "rho64": rho64, "V_T": VT, "q": q}

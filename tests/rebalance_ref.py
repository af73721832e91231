"""NumPy restatement of SPEC.md 4.5 / 5.4 (test helper, not a test module): the asset returns of chosen paths (Gaussian draws of
SPEC.md 2-4 or bootstrap rows of SPEC.md 2.1 / 4.4), the rebalanced recurrence in binary32 in the spec's order (values at the end
and at horizons), a binary64 twin that tracks dollar holdings instead, and the pivot of the moments."""
from __future__ import annotations

import math

import numpy as np

from bootstrap_ref import boot_indices
from oracle.np_oracle import _fma32, step_normals


def n4_of(n):
    return 4 * ((n + 3) // 4)


def gauss_returns(mu, chol, n_steps, seed, paths):
    """[T, n, N4] binary32 r_i = mu_i + sum_j L_ij z_j (j ascending, fma; SPEC.md 4's first sum), zero-padded to N4."""
    mu = np.asarray(mu, np.float32) + np.float32(0)
    L = np.tril(np.asarray(chol, np.float32))
    N = mu.shape[0]
    paths = np.asarray(paths, np.uint64)
    out = np.zeros((n_steps, paths.size, n4_of(N)), np.float32)
    for t in range(n_steps):
        z = step_normals(seed, paths, t, N)[:, :N]
        for i in range(N):
            acc = np.full(paths.size, mu[i], np.float32)
            for j in range(i + 1):
                acc = _fma32(np.full(paths.size, L[i, j], np.float32), z[:, j], acc)
            out[t, :, i] = acc
    return out


def boot_returns(rows, n_steps, seed, paths, block):
    """[T, n, N4] binary32 rows Rt[j_t] of SPEC.md 2.1 / 4.4, zero-padded to N4."""
    rows = np.asarray(rows, np.float32)
    R, N = rows.shape
    padded = np.zeros((R, n4_of(N)), np.float32)
    padded[:, :N] = rows
    idx = boot_indices(seed, paths, n_steps, R, block)
    return padded[idx]


def _pad_w(W, n4):
    W = np.atleast_2d(np.asarray(W, np.float32))
    out = np.zeros((W.shape[0], n4), np.float32)
    out[:, :W.shape[1]] = W
    return out


def rebalanced(r, W, period, cost=0.0, v0=1.0, horizons=()):
    """SPEC.md 4.5 on the asset returns r [T, n, N4] (binary32) -> dict(V_T [K, n], V_h [H, K, n] or None), binary32.
    B_i = fma(B_i, r_i, B_i + r_i) every step; at the events (dates s mod m == 0 < T, horizons, T) rho^ = W.B (i ascending),
    V^ = fma(V, rho^, V); at a date rho' = fma(-kappa32, tau, rho^) (kappa32 > 0), V = fma(V, rho', V), B = +0."""
    r = np.asarray(r, np.float32)
    T, n, n4 = r.shape
    Wp = _pad_w(W, n4)
    K = Wp.shape[0]
    kap = np.float32(cost)
    V = np.full((K, n), np.float32(v0), np.float32)
    B = np.zeros((n, n4), np.float32)
    want = {int(h): i for i, h in enumerate(horizons)}
    Vh = np.empty((len(horizons), K, n), np.float32) if len(horizons) else None
    nd = period if 1 <= period < T else T
    for s in range(1, T + 1):
        rt = r[s - 1]
        a = (B + rt).astype(np.float32)
        B = _fma32(B, rt, a)
        if s != nd and s != T and s not in want:
            continue
        rh = np.zeros((K, n), np.float32)
        for i in range(n4):
            rh = _fma32(np.broadcast_to(Wp[:, i:i + 1], (K, n)), np.broadcast_to(B[None, :, i], (K, n)), rh)
        vh = _fma32(V, rh, V)
        if s in want:
            Vh[want[s]] = vh
        if s == T:
            V = vh
        elif s == nd:
            if kap > 0:
                tau = np.zeros((K, n), np.float32)
                for i in range(n4):
                    d = np.abs((B[None, :, i] - rh).astype(np.float32))
                    tau = _fma32(np.broadcast_to(np.abs(Wp[:, i:i + 1]), (K, n)), d, tau)
                rh = _fma32(np.full((K, n), -kap, np.float32), tau, rh)
            V = _fma32(V, rh, V)
            B = np.zeros_like(B)
            nd = s + period if period < T - s else T
    return {"V_T": V, "V_h": Vh}


def dollar_holdings(r, W, period, cost=0.0, v0=1.0):
    """binary64 twin of SPEC.md 4.5 that tracks the dollar holdings h_i of every asset (and the cash 1 - sum W at zero return):
    h_i *= 1 + r_i every step; at a date the portfolio's worth is traded back to W, the cost kappa sum_i |W_i tot - h_i| paid out
    of it.  -> V_T [K, n]."""
    r = np.asarray(r, np.float32).astype(np.float64)
    T, n, n4 = r.shape
    Wp = _pad_w(W, n4).astype(np.float64)
    K = Wp.shape[0]
    out = np.empty((K, n))
    for k in range(K):
        w = Wp[k]
        h = np.broadcast_to(v0 * w, (n, n4)).copy()
        cash = np.full(n, v0 * (1.0 - w.sum()))
        for s in range(1, T + 1):
            h *= 1.0 + r[s - 1]
            if period >= 1 and s % period == 0 and s < T:
                tot = h.sum(axis=1) + cash
                traded = np.abs(w[None, :] * tot[:, None] - h).sum(axis=1)
                tot = tot - cost * traded
                h = w[None, :] * tot[:, None]
                cash = (1.0 - w.sum()) * tot
        out[k] = h.sum(axis=1) + cash
    return out


def asset_means(mu=None, rows=None):
    """mu_i of SPEC.md 5.4 in binary64: the drift, or the mean of column i of the rows (j ascending)."""
    if rows is None:
        return np.asarray(mu, np.float32).astype(np.float64)
    rows = np.asarray(rows, np.float32).astype(np.float64)
    s = np.zeros(rows.shape[1])
    for row in rows:
        s = s + row
    return s / rows.shape[0]


def reb_pivots(W, n_steps, period, mu=None, rows=None):
    """SPEC.md 5.4 in binary64: F = floor((T-1)/m) segments of length m (m >= 1, m < T; else F = 0) and one of length T - F m;
    a_i(l) = expm1(l log1p(mu_i)), g(l) = sum_i W[k,i] a_i(l) (i ascending); c = expm1(F log1p(g(m)) + log1p(g(l_last))), 0 where it
    is not finite (and for T = 0)."""
    m_i = asset_means(mu, rows)
    W = np.atleast_2d(np.asarray(W, np.float32)).astype(np.float64)
    T, m = int(n_steps), int(period)
    if T <= 0:
        return np.zeros(W.shape[0])
    F = (T - 1) // m if 1 <= m < T else 0
    last = T - F * m
    out = []
    for w in W:
        gf = gl = 0.0
        for i in range(w.size):
            lp = math.log1p(m_i[i])
            gl += w[i] * math.expm1(last * lp)
            if F:
                gf += w[i] * math.expm1(m * lp)
        try:
            e = math.log1p(gl)
            if F:
                e = F * math.log1p(gf) + e
            c = math.expm1(e)
        except (ValueError, OverflowError):
            c = float("nan")
        out.append(c if math.isfinite(c) else 0.0)
    return np.asarray(out)

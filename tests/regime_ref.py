"""NumPy restatement of SPEC.md 2.6 / 4.13 (test helper, not a test module): the host constants of a regime request in pure
Python, the regime path s_t of chosen path ids from the Philox blocks on counter stream 4, the per-step portfolio returns with
every row walked on the drift and factor of the path's regime, in binary32 in the spec's order, and from them the terminal values,
the drawdown state (drawdown_ref.drawdown_state) and the values at horizons (horizons_ref.values_at_horizons).  Below it, the
closed forms of the chain and of the pivot as direct binary64 matrix products, a binary64 twin of the model on NumPy's own
generator, and the law assertions that the twin (CPU) and the device values (GPU) both have to pass."""
from __future__ import annotations

import math

import numpy as np

from drawdown_ref import drawdown_state
from horizons_ref import values_at_horizons
from oracle.np_oracle import _fma32, philox4x32_10, step_normals

_MASK = np.uint64(0xFFFFFFFF)
TWO32 = 4294967296.0


def regime_consts(p01, p10, start):
    """SPEC.md 2.6 host constants in pure Python -> (thr [3] ints in [0, 2^32], p^ [3] floats), for (01, 10, start)."""
    thr = [int(min(1 << 32, math.floor(float(p) * TWO32))) for p in (p01, p10, start)]
    return thr, [t / TWO32 for t in thr]


def regime_path(seed, paths, T, thr):
    """s uint8 [T, ids]: s_0 = x1 < thr_start of the block of t = 0; s_{t+1} = s_t == 0 ? x0 < thr01 : !(x0 < thr10), x0 of the
    block of step t; one block per path and step on counter (t, 4, p_lo, p_hi)."""
    paths = np.asarray(paths, np.uint64)
    s = np.zeros((max(T, 0), paths.size), np.uint8)
    cur = None
    for t in range(T):
        x = philox4x32_10(np.uint64(t), np.uint64(4), paths & _MASK, paths >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
        x0, x1 = x[0].astype(np.uint64), x[1].astype(np.uint64)
        if t == 0:
            cur = (x1 < np.uint64(thr[2])).astype(np.uint8)
        s[t] = cur
        cur = np.where(cur == 0, x0 < np.uint64(thr[0]), ~(x0 < np.uint64(thr[1]))).astype(np.uint8)
    return s


def _rows_of(mu, L, z):
    """r [ids, N]: row i is acc = mu_i, then acc = fma(L_ij, z_j, acc), j ascending, binary32."""
    n, N = z.shape[0], mu.shape[0]
    r = np.empty((n, N), np.float32)
    for i in range(N):
        acc = np.full(n, mu[i], np.float32)
        for j in range(i + 1):
            acc = _fma32(np.full(n, L[i, j], np.float32), z[:, j], acc)
        r[:, i] = acc
    return r


def simulate_regimes(mu, chol, mu1, chol1, W, T, seed, paths, probs, v0=1.0, horizons=()):
    """Chosen path ids (path_begin included) -> dict(rho [K, T, ids], s [T, ids], V_T [K, ids], q [K, ids], V_h [H, K, ids] or
    None), binary32 in the spec's order: the step's rows on (mu, L) of regime s_t, each regime a whole chain of its own, rho_k =
    sum_i w_ki r_i (i ascending, fma from +0), V = fma(V, rho, V).  probs = (p01, p10, start)."""
    mus = [np.asarray(m, np.float32) + np.float32(0) for m in (mu, mu1)]
    Ls = [np.tril(np.asarray(c, np.float32)) for c in (chol, chol1)]
    W = np.atleast_2d(np.asarray(W, np.float32))
    N, K = mus[0].shape[0], W.shape[0]
    paths = np.asarray(paths, np.uint64)
    n = paths.size
    thr, _ = regime_consts(*probs)
    s = regime_path(seed, paths, T, thr)
    rho = np.zeros((K, T, n), np.float32)
    for t in range(T):
        z = step_normals(seed, paths, t, N)[:, :N]
        r = np.where((s[t] != 0)[:, None], _rows_of(mus[1], Ls[1], z), _rows_of(mus[0], Ls[0], z))
        for k in range(K):
            acc = np.zeros(n, np.float32)
            for i in range(N):
                acc = _fma32(np.full(n, W[k, i], np.float32), r[:, i], acc)
            rho[k, t] = acc
    VT = np.empty((K, n), np.float32)
    q = np.empty((K, n), np.float32)
    for k in range(K):
        VT[k], q[k] = drawdown_state(rho[k], "simple", v0)
    Vh = values_at_horizons(rho, horizons, "simple", v0) if len(horizons) else None
    return {"rho": rho, "s": s, "V_T": VT, "q": q, "V_h": Vh}


def transitions_seen(s):
    """The set of (s_t, s_{t+1}) pairs in a regime path [T, ids]."""
    return {(int(a), int(b)) for a, b in zip(s[:-1].ravel(), s[1:].ravel())}


def chain_matrix(p01, p10):
    return np.array([[1.0 - p01, p01], [p10, 1.0 - p10]])


def occupancy_direct(p01, p10, start, T):
    """(pi P^t)_1 for t = 0 .. T-1 by matrix powers."""
    pi, P = np.array([1.0 - start, start]), chain_matrix(p01, p10)
    return np.array([(pi @ np.linalg.matrix_power(P, t))[1] for t in range(T)])


def pivots_direct(p01, p10, start, mu, mu1, W, hs):
    """c_k(h) = pi' D_k (P D_k)^(h-1) 1 - 1 as a direct binary64 matrix product, [len(hs), K]; 0 for h = 0."""
    W = np.atleast_2d(np.asarray(W, np.float32)).astype(np.float64)
    m0, m1 = (np.asarray(m, np.float32).astype(np.float64) for m in (mu, mu1))
    pi, P = np.array([1.0 - start, start]), chain_matrix(p01, p10)
    out = np.zeros((len(hs), W.shape[0]))
    for k, w in enumerate(W):
        D = np.diag([1.0 + float(w @ m0), 1.0 + float(w @ m1)])
        for i, h in enumerate(hs):
            out[i, k] = 0.0 if h == 0 else float(pi @ D @ np.linalg.matrix_power(P @ D, h - 1) @ np.ones(2)) - 1.0
    return out


def step_law(p01, p10, start, m, s2, T):
    """(pi [T], mean [T], var [T]) of rho_t for one portfolio with per-regime means m = (m0, m1) and variances s2 = (s2_0, s2_1):
    the informative formulas of SPEC.md 2.6, written directly."""
    pi = occupancy_direct(p01, p10, start, T)
    mean = (1.0 - pi) * m[0] + pi * m[1]
    second = (1.0 - pi) * (s2[0] + m[0] ** 2) + pi * (s2[1] + m[1] ** 2)
    return pi, mean, second - mean ** 2


def twin_values(p01, p10, start, m, sd, T, n_paths, seed, v0=1.0):
    """The binary64 twin of the model for one asset held alone, on NumPy's own generator -> V [T, n_paths] after every step: the
    regime from uniform 32-bit words through the same thresholds, rho = m_s + sd_s g."""
    thr, _ = regime_consts(p01, p10, start)
    rng = np.random.default_rng(seed)
    V = np.empty((T, n_paths))
    v = np.full(n_paths, float(v0))
    cur = rng.integers(0, 1 << 32, size=n_paths, dtype=np.uint64) < np.uint64(thr[2])
    for t in range(T):
        g = rng.standard_normal(n_paths)
        rho = np.where(cur, m[1] + sd[1] * g, m[0] + sd[0] * g)
        v = v * (1.0 + rho)
        V[t] = v
        x0 = rng.integers(0, 1 << 32, size=n_paths, dtype=np.uint64)
        cur = np.where(cur, ~(x0 < np.uint64(thr[1])), x0 < np.uint64(thr[0]))
    return V


def step_returns(V, v0):
    """rho_t = V_t / V_{t-1} - 1 in binary64 from values after every step [T, n] (V_0 = v0)."""
    V = np.asarray(V, np.float64)
    prev = np.vstack([np.full((1, V.shape[1]), float(v0)), V[:-1]])
    return V / prev - 1.0


def lag1_square_corr(rho):
    """(r, se): the correlation of rho_t^2 and rho_{t+1}^2 pooled over t (every pair centred and scaled by its own columns' sample
    moments, so a variance that drifts with t adds nothing) and its standard error, the sample's own: std(products) / sqrt(pairs)."""
    a = rho * rho
    u = (a - a.mean(axis=1, keepdims=True)) / a.std(axis=1, keepdims=True)
    prod = u[:-1] * u[1:]
    return float(prod.mean()), float(prod.std()) / math.sqrt(prod.size)


def law_checks(V, v0, pivots, mean_want, var_want, persistent):
    """The law assertions on V [T, n] (row t - 1: the values after step t; binary32 from the device or binary64 from twin_values) of
    one portfolio, every bound 5 standard errors of the sample's own:
      * the mean of x_h = V_h / v0 - 1 within 5 standard errors (sqrt(sample variance / n)) of pivots[h - 1], for every h;
      * mean((rho_t - mean_want[t])^2) within 5 standard errors (sqrt((m4 - m2^2) / n)) of var_want[t], for every t;
      * the lag-1 correlation of the squares (lag1_square_corr) more than 5 standard errors above 0 when `persistent`, within 5 of 0
        when not.
    5 standard errors is the bound for 2 T + 1 two-sided normal tests at a false-alarm rate below 1e-4 in all; it is not fitted to
    any run.  -> dict of the figures (in standard errors), for printing."""
    V = np.asarray(V, np.float64)
    T, n = V.shape
    x = V / float(v0) - 1.0
    z_mean = (x.mean(axis=1) - pivots) / (x.std(axis=1) / math.sqrt(n))
    rho = step_returns(V, v0)
    d2 = (rho - np.asarray(mean_want)[:, None]) ** 2
    m2 = d2.mean(axis=1)
    z_var = (m2 - var_want) / np.sqrt((np.mean(d2 * d2, axis=1) - m2 * m2) / n)
    r, se = lag1_square_corr(rho)
    fig = {"max |z_mean|": float(np.abs(z_mean).max()), "max |z_var|": float(np.abs(z_var).max()), "lag1": r, "lag1 / se": r / se}
    assert np.all(np.abs(z_mean) < 5.0), (z_mean, fig)
    assert np.all(np.abs(z_var) < 5.0), (z_var, fig)
    if persistent:
        assert r > 5.0 * se, fig
    else:
        assert abs(r) < 5.0 * se, fig
    return fig

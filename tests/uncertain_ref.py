"""NumPy restatement of SPEC.md 2.7 / 4.21 (test helper, not a test module): every path draws its drift once, m = mu + M g on counter
stream 5, and walks the Gaussian step of SPEC.md 4 from m instead of mu -- in binary32 in the spec's order, on oracle.np_oracle's
Philox, normals and emulated fma.  A vectorised walk gives V_T / S_T, the drawdown q / d (SPEC.md 4.2), the horizon rows V_h (4.3) and,
with flows, the cash-flow rule of cashflow_ref.py (4.7).  Below it the same rule as a plain per-path loop over binary32 scalars, and the
inputs of the GPU test."""
from __future__ import annotations

import numpy as np

from oracle.np_oracle import _fma32, normals, philox4x32_10, step_normals

_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
f32 = np.float32


def drift_normals(seed: int, paths, n_assets: int) -> np.ndarray:
    """g [n, N4] of SPEC.md 2.7: g[:, m nb + q] = normal m of the Philox block on counter (q, 5, p_lo, p_hi)."""
    nb = (n_assets + 3) // 4
    paths = np.asarray(paths, np.uint64)
    plo, phi = paths & _MASK, paths >> _S32
    g = np.empty((paths.shape[0], 4 * nb), np.float32)
    for q in range(nb):
        xs = philox4x32_10(np.uint64(q), np.uint64(5), plo, phi, seed & 0xFFFFFFFF, seed >> 32)
        for m in range(4):
            g[:, m * nb + q] = normals(xs[m])
    return g


def path_drift(mu, M, g) -> np.ndarray:
    """m [n, N] of SPEC.md 4.21: m_i = mu_i, then m_i = fma(M[i, j], g_j, m_i) for j = 0 .. i, binary32."""
    mu = np.asarray(mu, np.float32) + f32(0)
    M = np.tril(np.asarray(M, np.float32)) + f32(0)
    n, N = g.shape[0], mu.shape[0]
    out = np.empty((n, N), np.float32)
    for i in range(N):
        acc = np.full(n, mu[i], np.float32)
        for j in range(i + 1):
            acc = _fma32(np.full(n, M[i, j], np.float32), g[:, j], acc)
        out[:, i] = acc
    return out


def step_rho(m, L, W, z) -> np.ndarray:
    """rho [K, n] of one step: r_i = m_i, then fma(L[i, j], z_j, r_i), j ascending; rho_k = fma(W[k, i], r_i, rho_k) from +0, i ascending."""
    n, N = m.shape
    r = np.empty((n, N), np.float32)
    for i in range(N):
        acc = m[:, i].copy()
        for j in range(i + 1):
            acc = _fma32(np.full(n, L[i, j], np.float32), z[:, j], acc)
        r[:, i] = acc
    rho = np.zeros((W.shape[0], n), np.float32)
    for k in range(W.shape[0]):
        for i in range(N):
            rho[k] = _fma32(np.full(n, W[k, i], np.float32), r[:, i], rho[k])
    return rho


def simulate(mu, chol, M, W, T, seed, paths, compounding="simple", v0=1.0, drawdown=False, horizons=(), flows=None):
    """Chosen path ids (path_begin included) -> dict(V_T [K, n] (V, or S under log compounding), q [K, n] or None (q simple, d log), V_h
    [H, K, n] or None, m [n, N]), binary32.  M None: the walk of the call without uncertainty (every row starts at mu)."""
    paths = np.asarray(paths, np.uint64)
    mu = np.asarray(mu, np.float32) + f32(0)
    L = np.tril(np.asarray(chol, np.float32))
    W = np.atleast_2d(np.asarray(W, np.float32))
    N, K, n = mu.shape[0], W.shape[0], paths.shape[0]
    logc = compounding == "log"
    m = np.tile(mu, (n, 1)) if M is None else path_drift(mu, M, drift_normals(seed, paths, N))
    X = np.full((K, n), 0.0 if logc else v0, np.float32)
    P = np.full((K, n), -np.inf, np.float32)
    q = np.full((K, n), 0.0 if logc else 1.0, np.float32)
    want = {int(h): i for i, h in enumerate(horizons)}
    Vh = np.empty((len(want), K, n), np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for t in range(T):
            rho = step_rho(m, L, W, step_normals(seed, paths, t, N)[:, :N])
            if logc:
                X = (X + rho).astype(np.float32)
            elif flows is not None:                       # SPEC.md 4.7
                U = (_fma32(X, rho, X) + f32(flows[t])).astype(np.float32)
                X = np.where((X > 0) & (U > 0), U, f32(0.0)).astype(np.float32)
            else:
                X = _fma32(X, rho, X)
            if drawdown:                                  # SPEC.md 4.2
                P = np.fmax(P, X)
                q = np.fmin(q, ((X - P) if logc else (X / P)).astype(np.float32)).astype(np.float32)
            if t + 1 in want:
                Vh[want[t + 1]] = X
    return {"V_T": X, "q": q if drawdown else None, "V_h": Vh if want else None, "m": m}


def _fma(a, b, c):
    return _fma32(np.array([a], np.float32), np.array([b], np.float32), np.array([c], np.float32))[0]


def loop_one_path(mu, chol, M, W, T, seed, p, compounding="simple", v0=1.0, drawdown=False, horizons=(), flows=None):
    """The same rule for one path id p as plain loops over binary32 scalars -> (V_T [K], q [K] or None, V_h [H, K] or None)."""
    mu = np.asarray(mu, np.float32) + f32(0)
    L, Mm = np.tril(np.asarray(chol, np.float32)), np.tril(np.asarray(M, np.float32)) + f32(0)
    W = np.atleast_2d(np.asarray(W, np.float32))
    N, K = mu.shape[0], W.shape[0]
    logc = compounding == "log"
    g = drift_normals(seed, [p], N)[0]
    m = []
    for i in range(N):
        acc = mu[i]
        for j in range(i + 1):
            acc = _fma(Mm[i, j], g[j], acc)
        m.append(acc)
    X = [f32(0.0 if logc else v0)] * K
    P, q = [f32(-np.inf)] * K, [f32(0.0 if logc else 1.0)] * K
    Vh = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for t in range(T):
            z = step_normals(seed, np.array([p], np.uint64), t, N)[0]
            r = []
            for i in range(N):
                acc = m[i]
                for j in range(i + 1):
                    acc = _fma(L[i, j], z[j], acc)
                r.append(acc)
            for k in range(K):
                rho = f32(0.0)
                for i in range(N):
                    rho = _fma(W[k, i], r[i], rho)
                if logc:
                    X[k] = f32(X[k] + rho)
                elif flows is not None:
                    u = f32(_fma(X[k], rho, X[k]) + f32(flows[t]))
                    X[k] = u if (X[k] > 0 and u > 0) else f32(0.0)
                else:
                    X[k] = _fma(X[k], rho, X[k])
                if drawdown:
                    P[k] = np.fmax(P[k], X[k])
                    q[k] = np.fmin(q[k], f32(X[k] - P[k]) if logc else f32(X[k] / P[k]))
            if t + 1 in [int(h) for h in horizons]:
                Vh[t + 1] = list(X)
    return (np.array(X, np.float32), np.array(q, np.float32) if drawdown else None,
            np.array([Vh[int(h)] for h in horizons], np.float32) if len(horizons) else None)


# ---- the inputs of the GPU test ---------------------------------------------------------------------------------------------------------
SEED = 0x21_0C05
TILE = 8192 * 256                                        # paths of the first grid-stride tile of a launch
CASES = [  # N, K, T, path_begin, n_paths
    (3, 1, 1, 0, 300),
    (5, 3, 2, 0, 1037),
    (16, 9, 13, (1 << 32) - 200, 513),
    (17, 20, 7, 5, 257),
    (64, 3, 7, 17, 257),
    (1, 1, 2, 3, TILE + 257),
]
# the seven kernel rows: (family, compounding)
ROWS = [("plain", "simple"), ("plain", "log"), ("dd", "simple"), ("dd", "log"), ("hz", "simple"), ("hz", "log"), ("cf", "simple")]


def market(N, K, vol=0.05):
    """A market at about one step volatility `vol` per step: asset i drifts by 0.2 vol (+1, -1, 0)[i mod 3], the factor is vol (I + 0.1
    strictly lower ones) / sqrt(1 + 0.01 N), portfolio k holds 0.8 of asset k mod min(N, 3) and spreads the rest evenly."""
    mu = (0.2 * vol * np.array([(1.0, -1.0, 0.0)[i % 3] for i in range(N)])).astype(np.float32)
    L = (vol * (np.eye(N) + 0.1 * np.tril(np.ones((N, N)), -1)) / np.sqrt(1.0 + 0.01 * N)).astype(np.float32)
    W = np.full((K, N), 0.2 / N)
    for k in range(K):
        W[k, k % min(N, 3)] += 0.8
    return mu, L, W.astype(np.float32)


def dense_factor(N, scale=0.02, seed=7):
    """A dense random lower-triangular M that is no multiple of the market's L: every entry of the triangle drawn on its own."""
    rng = np.random.default_rng(seed + N)
    return np.tril(scale * rng.standard_normal((N, N))).astype(np.float32)


def holed_factor(N, scale=0.02, seed=11):
    """dense_factor with a zero row (the last asset's drift is known) and a zero column (g_0 moves nobody), where N allows it."""
    M = dense_factor(N, scale, seed)
    M[N - 1, :] = 0.0
    M[:, 0] = 0.0
    return M


def horizons_of(T):
    """A horizon on step 1, on T, and two in a row, as far as T allows."""
    return sorted({1, T} | ({T - 1} if T >= 3 else set()) | ({2} if T >= 4 else set()))


def flows_of(T, v0=1.0):
    """A schedule that ruins some paths and not others at the GPU test's volatilities: a withdrawal of 0.97 v0 on the first step leaves
    about 0.03 v0 give or take one step's return, then 0.004 v0 leaves on every later step, so that ruin goes on from horizon to
    horizon."""
    flows = np.full(T, -0.004 * v0, np.float32)
    flows[0] = -0.97 * v0
    return flows


def pick(n_paths, begin):
    """The local path ids a long range is compared on: every path where n_paths <= 1100; else the first and last 64 ids, the ids
    within 3 of the 2^32 crossing and the ids within 3 of the tile boundary."""
    if n_paths <= 1100:
        return np.arange(n_paths, dtype=np.int64)
    ids = set(range(64)) | set(range(n_paths - 64, n_paths))
    cross = (1 << 32) - begin
    if 0 < cross < n_paths:
        ids.update(range(max(0, cross - 3), min(n_paths, cross + 4)))
    if n_paths > TILE:
        ids.update(range(TILE - 3, min(n_paths, TILE + 4)))
    return np.array(sorted(ids), np.int64)

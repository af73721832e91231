"""NumPy restatement of SPEC.md 4.14 / 5.14 (test helper, not a test module): the cash-flow walk of cashflow_ref on the scheduled
target weights of a glide path.  The draws do not depend on the weights, so every segment's per-step portfolio returns come from
cashflow_ref.gauss_rho / boot_rho on that segment's weights (one call on the blocks stacked as rows); step t takes its column from
the segment that owns it and cashflow_ref.walk runs on the result.  The pivot is the per-segment Horner walk in binary64."""
from __future__ import annotations

import numpy as np

from cashflow_ref import boot_rho, gauss_rho, step_means, walk


def segment_of_steps(breaks, n_steps):
    """int [T]: g(s) = #{j : b_j < s} of the steps s = 1 .. T (index t = s - 1)."""
    br = np.asarray(breaks, np.int64).ravel()
    return np.array([int(np.count_nonzero(br < s)) for s in range(1, int(n_steps) + 1)], np.int64)


def blocks_of(W, targets):
    """[G + 1, K, N] binary32: block 0 the call's W [K, N], then the targets [G, K, N]."""
    W = np.atleast_2d(np.asarray(W, np.float32))
    targets = np.asarray(targets, np.float32).reshape(-1, W.shape[0], W.shape[1])
    return np.concatenate([W[None], targets], axis=0)


def glide_rho(breaks, targets, W, n_steps, seed, paths, mu=None, chol=None, dof=None, rows=None, block=1.0):
    """[K, T, n] binary32: column t from the returns of the segment that owns step t + 1."""
    blocks = blocks_of(W, targets)
    seg = segment_of_steps(breaks, n_steps)
    paths = np.asarray(paths, np.uint64)
    G1, K, N = blocks.shape
    # every row of a weight matrix is walked on its own, so the G + 1 blocks go through the restatement as one matrix of (G + 1) K rows
    stacked = np.ascontiguousarray(blocks.reshape(G1 * K, N))
    rho = boot_rho(rows, stacked, n_steps, seed, paths, block) if rows is not None else gauss_rho(mu, chol, stacked, n_steps, seed, paths, dof)
    rho = rho.reshape(G1, K, int(n_steps), paths.size)
    out = np.empty((K, int(n_steps), paths.size), np.float32)
    for t in range(int(n_steps)):
        out[:, t, :] = rho[seg[t], :, t, :]
    return out


def simulate_glide(breaks, targets, flows, W, n_steps, seed, paths, mu=None, chol=None, dof=None, rows=None, block=1.0, v0=1.0,
                   horizons=()):
    """Chosen path ids (path_begin included) -> dict(V_T [K, n], V_h [H, K, n] or None, rho [K, T, n]), binary32."""
    rho = glide_rho(breaks, targets, W, n_steps, seed, paths, mu=mu, chol=chol, dof=dof, rows=rows, block=block)
    flows = np.zeros(int(n_steps), np.float32) if flows is None else flows
    VT, Vh = walk(rho, flows, v0, horizons)
    return {"V_T": VT, "V_h": Vh, "rho": rho}


def walk64(rho, flows, v0=1.0):
    """cashflow_ref.walk in binary64 on the binary32 returns rho [K, T, n] -> V_T [K, n] float64 (the law test's rounding gap)."""
    rho = np.asarray(rho, np.float32).astype(np.float64)
    K, T, n = rho.shape
    flows = np.zeros(T) if flows is None else np.asarray(flows, np.float32).astype(np.float64)
    V = np.full((K, n), float(np.float32(v0)), np.float64)
    for t in range(T):
        U = V * rho[:, t] + V + flows[t]
        V = np.where((V > 0) & (U > 0), U, 0.0)
    return V


def horner_pivots(breaks, targets, W, flows, n_steps, mu=None, rows=None, v0=1.0, horizons=()):
    """SPEC.md 5.14: A_0 = fl32(v0), A_s = A_{s-1} (1 + m_{k,g(s)}) + c_s (a sum, a product, a sum; binary64) -> (pivot at T [K],
    pivots at the horizons [H, K]); pivot = max(A, 0) / fl32(v0) - 1, 0 where not finite."""
    blocks = blocks_of(W, targets)
    m = np.array([step_means(blocks[g], mu=mu, rows=rows) for g in range(blocks.shape[0])], np.float64)   # [G + 1, K]
    seg = segment_of_steps(breaks, n_steps)
    T = int(n_steps)
    c = np.zeros(T) if flows is None else np.asarray(flows, np.float32).astype(np.float64)
    v0d = float(np.float32(v0))

    def pivot(A):
        r = max(A, 0.0) / v0d - 1.0
        return r if np.isfinite(A) and np.isfinite(r) else 0.0
    K = blocks.shape[1]
    at_T, at_h = np.zeros(K), np.zeros((len(horizons), K))
    want = {int(h): i for i, h in enumerate(horizons)}
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(K):
            A = np.float64(v0d)
            for s in range(1, T + 1):
                g = np.float64(1.0) + m[seg[s - 1], k]
                A = A * g
                A = A + c[s - 1]
                if s in want:
                    at_h[want[s], k] = pivot(float(A))
            at_T[k] = pivot(float(A))
    return at_T, at_h

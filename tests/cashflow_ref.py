"""NumPy restatement of SPEC.md 4.7 / 5.6 (test helper, not a test module): the walk of chosen paths with a cash-flow schedule
and absorbing ruin, in binary32 in the spec's order, on the per-step portfolio returns of the other restatements (Gaussian and
Student-t: student_t_ref.t_rho; bootstrap: bootstrap_ref), the pivot's Horner walk in binary64 and the counts."""
from __future__ import annotations

import numpy as np

from bootstrap_ref import boot_indices, row_returns
from oracle.np_oracle import _fma32
from student_t_ref import t_rho


def walk(rho, flows, v0=1.0, horizons=()):
    """rho [K, T, n] binary32 per-step portfolio returns, flows [T] -> (V_T [K, n], V_h [H, K, n] or None), binary32: per step
    U = fma(V, rho, V); U = U + c_s; V = (V > 0 and U > 0) ? U : +0, from fl32(v0)."""
    rho = np.asarray(rho, np.float32)
    flows = np.asarray(flows, np.float32)
    K, T, n = rho.shape
    assert flows.shape == (T,)
    V = np.full((K, n), v0, np.float32)
    out = np.empty((len(horizons), K, n), np.float32)
    want = {int(h): i for i, h in enumerate(horizons)}
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            U = _fma32(V, rho[:, t], V)
            U = (U + flows[t]).astype(np.float32)
            V = np.where((V > 0) & (U > 0), U, np.float32(0.0)).astype(np.float32)
            if t + 1 in want:
                out[want[t + 1]] = V
    return V, (out if len(horizons) else None)


def gauss_rho(mu, chol, W, n_steps, seed, paths, dof=None):
    """[K, T, n] per-step returns of SPEC.md 4 (dof None) or 4.6 (Student-t)."""
    return t_rho(mu, chol, W, n_steps, seed, paths, dof if dof is not None else 5, unit_scale=dof is None)


def boot_rho(rows, W, n_steps, seed, paths, block):
    """[K, T, n] per-step returns of SPEC.md 4.4."""
    rows = np.asarray(rows, np.float32)
    idx = boot_indices(seed, paths, n_steps, rows.shape[0], block)
    return row_returns(rows, W)[:, idx]


def simulate_cf(flows, W, n_steps, seed, paths, mu=None, chol=None, dof=None, rows=None, block=1.0, v0=1.0, horizons=()):
    """Chosen path ids (path_begin included) -> dict(V_T [K, n], V_h [H, K, n] or None), binary32."""
    paths = np.asarray(paths, np.uint64)
    if rows is not None:
        rho = boot_rho(rows, W, n_steps, seed, paths, block)
    else:
        rho = gauss_rho(mu, chol, W, n_steps, seed, paths, dof)
    VT, Vh = walk(rho, flows, v0, horizons)
    return {"V_T": VT, "V_h": Vh, "rho": rho}


def step_means(W, mu=None, rows=None):
    """SPEC.md 5.6: m_k in binary64 -- sum_i W[k,i] mu_i (i ascending) or the mean over the rows of sum_i W[k,i] rows[j,i]."""
    W = np.atleast_2d(np.asarray(W, np.float32)).astype(np.float64)
    out = []
    for w in W:
        if rows is None:
            m = 0.0
            for i, v in enumerate((np.asarray(mu, np.float32) + np.float32(0)).astype(np.float64)):
                m += w[i] * v
        else:
            s = 0.0
            r64 = np.asarray(rows, np.float32).astype(np.float64)
            for r in r64:
                v = 0.0
                for i in range(r.size):
                    v += w[i] * r[i]
                s += v
            m = s / r64.shape[0]
        out.append(float(m))
    return out


def horner_pivots(m, flows, v0=1.0, horizons=()):
    """SPEC.md 5.6: A_0 = fl32(v0), A_s = A_{s-1} (1 + m) + c_s (a product, then a sum, binary64) -> (pivot at T [K], pivots at the
    horizons [H, K]); pivot = max(A, 0) / fl32(v0) - 1, 0 where not finite."""
    flows = np.asarray(flows, np.float32).astype(np.float64)
    v0d = float(np.float32(v0))

    def pivot(A):
        c = max(A, 0.0) / v0d - 1.0
        return c if np.isfinite(A) and np.isfinite(c) else 0.0
    at_T, at_h = [], np.zeros((len(horizons), len(m)))
    want = {int(h): i for i, h in enumerate(horizons)}
    with np.errstate(over="ignore", invalid="ignore"):
        for k, mk in enumerate(m):
            g = np.float64(1.0) + np.float64(mk)
            A = np.float64(v0d)
            for s in range(1, flows.size + 1):
                A = A * g
                A = A + flows[s - 1]
                if s in want:
                    at_h[want[s], k] = pivot(float(A))
            at_T.append(pivot(float(A)))
    return np.asarray(at_T), at_h


def counts_of(rows, target=None):
    """SPEC.md 5.6 on stored rows [..., n] -> uint64 [..., 2] {#(V == 0), #(V < fl32(target)) or 0}."""
    rows = np.asarray(rows, np.float32)
    ruined = np.count_nonzero(rows == 0, axis=-1)
    short = np.count_nonzero(rows < np.float32(target), axis=-1) if target is not None else np.zeros_like(ruined)
    return np.stack([ruined, short], axis=-1).astype(np.uint64)

"""NumPy restatement of SPEC.md 2.2 / 4.6 (test helper, not a test module): the chi and scale s of a step on counter stream 2, the
per-step portfolio returns of chosen paths with every normal scaled by s, in binary32 in the spec's order, and from them the
terminal values, the drawdown state (drawdown_ref.drawdown_state) and the values at horizons (horizons_ref.values_at_horizons).
NumPy's binary32 "/" and np.sqrt are correctly rounded, as the kernel's division and sqrtf are."""
from __future__ import annotations

import numpy as np

from drawdown_ref import drawdown_state
from horizons_ref import values_at_horizons
from oracle.np_oracle import _fma32, normals, philox4x32_10, step_normals

_MASK = np.uint64(0xFFFFFFFF)


def chi_and_scale(seed, paths, t, dof):
    """SPEC.md 2.2 for step t (0-based) of the global path ids `paths` -> (chi, s), binary32 [n] each: nt = ceil(nu/4) Philox
    blocks on counter (t nt + q, 2, p_lo, p_hi), g_k = Z(x_m(q)) for k = 4q + m < nu, chi = fma(g_k, g_k, chi) (k ascending,
    from +0), chi = max(chi, 2^-126), s = sqrt(fl32(nu - 2) / chi)."""
    paths = np.asarray(paths, np.uint64)
    plo, phi = paths & _MASK, paths >> np.uint64(32)
    nt = (dof + 3) // 4
    chi = np.zeros(paths.size, np.float32)
    for q in range(nt):
        xs = philox4x32_10(np.uint64(t * nt + q), np.uint64(2), plo, phi, seed & 0xFFFFFFFF, seed >> 32)
        for m in range(4):
            if 4 * q + m >= dof:
                break
            g = normals(xs[m])
            chi = _fma32(g, g, chi)
    chi = np.maximum(chi, np.float32(2.0 ** -126))
    s = np.sqrt(np.float32(dof - 2) / chi).astype(np.float32)
    return chi, s


def t_rho(mu, chol, W, n_steps, seed, paths, dof, unit_scale=False):
    """[K, T, n] binary32 per-step portfolio returns of SPEC.md 4.6: z' = fl32(s z), r_i = mu_i + sum_j L_ij z'_j (j ascending,
    fma), rho_k = sum_i w_ki r_i (i ascending, fma).  unit_scale: s = 1 (the Gaussian model of SPEC.md 4)."""
    mu = np.asarray(mu, np.float32) + np.float32(0)
    L = np.tril(np.asarray(chol, np.float32))
    W = np.atleast_2d(np.asarray(W, np.float32))
    N, K = mu.shape[0], W.shape[0]
    paths = np.asarray(paths, np.uint64)
    n = paths.size
    rho = np.zeros((K, n_steps, n), np.float32)
    for t in range(n_steps):
        z = step_normals(seed, paths, t, N)[:, :N]
        if not unit_scale:
            z = (chi_and_scale(seed, paths, t, dof)[1][:, None] * z).astype(np.float32)
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
    return rho


def simulate_t(mu, chol, W, n_steps, seed, paths, dof, v0=1.0, horizons=(), unit_scale=False):
    """Chosen path ids (path_begin included) -> dict(rho [K, T, n], V_T [K, n], q [K, n], V_h [H, K, n] or None), binary32."""
    rho = t_rho(mu, chol, W, n_steps, seed, paths, dof, unit_scale)
    K, _, n = rho.shape
    VT = np.empty((K, n), np.float32)
    q = np.empty((K, n), np.float32)
    for k in range(K):
        VT[k], q[k] = drawdown_state(rho[k], "simple", v0)
    Vh = values_at_horizons(rho, horizons, "simple", v0) if len(horizons) else None
    return {"rho": rho, "V_T": VT, "q": q, "V_h": Vh}

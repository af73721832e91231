"""Restatement of SPEC.md 2.3 / 5.10 (test helper, not a test module).  Antithetic pairs need no walk of their own: member 2j of
pair j is path j of the call without pairs, member 2j + 1 is path j of that call with the Cholesky factor negated (fma(L, -z, r) =
fma(-L, z, r) exactly, fl32(s (-z)) = -fl32(s z), the GARCH shock sees squares only).  So the restatement interleaves the existing
ones walked with L and with -L: oracle.mc_oracle.simulate for Gaussian terminal values, drawdown_ref / horizons_ref for the Gaussian
drawdown and horizons, student_t_ref and garch_ref for the other draws.  literal_pair_terminal is the definition itself -- the walk
on negated normals -- which pins that shortcut once.  pair_stats is SPEC.md 5.10 in NumPy from stored values."""
from __future__ import annotations

import numpy as np

from drawdown_ref import simulate_paths_dd
from garch_ref import simulate_garch
from horizons_ref import simulate_horizons
from oracle import mc_oracle
from oracle.np_oracle import _fma32
from student_t_ref import simulate_t


def interleave(plus, minus):
    """[..., m] values of the members 2j and of the members 2j + 1 -> [..., 2m], member 2j + s at column 2j + s."""
    plus, minus = np.asarray(plus), np.asarray(minus)
    out = np.empty(plus.shape[:-1] + (2 * plus.shape[-1],), plus.dtype)
    out[..., 0::2] = plus
    out[..., 1::2] = minus
    return out


def pair_ids(paths):
    """Global path ids -> the pair ids j = g >> 1 of the even ones (the ids must come as whole pairs, even id first)."""
    paths = np.asarray(paths, np.uint64)
    assert paths.size % 2 == 0 and np.all(paths[0::2] % np.uint64(2) == 0) and np.all(paths[1::2] == paths[0::2] + np.uint64(1))
    return paths[0::2] >> np.uint64(1)


def simulate_terminal(mu, chol, W, n_steps, n_paths, seed, path_begin=0, v0=1.0, compounding="simple"):
    """Gaussian draws, every path of [path_begin, path_begin + n_paths), both even -> terminal [K, n_paths] binary32."""
    assert path_begin % 2 == 0 and n_paths % 2 == 0
    L = np.asarray(chol, np.float32)
    a = mc_oracle.simulate(mu, L, W, n_steps, n_paths // 2, seed, path_begin // 2, v0, compounding)
    b = mc_oracle.simulate(mu, -L, W, n_steps, n_paths // 2, seed, path_begin // 2, v0, compounding)
    return interleave(a, b)


def simulate_sampled(mu, chol, W, n_steps, seed, paths, dof=None, garch=None, v0=1.0, compounding="simple", horizons=()):
    """Chosen global path ids (whole pairs) -> dict(V_T [K, n], q [K, n], V_h [H, K, n] or None), binary32, on the restatement of
    the request's draws: garch_ref (garch), student_t_ref (dof) or drawdown_ref / horizons_ref (Gaussian; simple or log)."""
    j = pair_ids(paths)
    L = np.asarray(chol, np.float32)
    out = []
    for Ls in (L, -L):
        if garch is not None:
            r = simulate_garch(mu, Ls, W, n_steps, seed, j, garch, dof=dof, v0=v0, horizons=horizons)
        elif dof is not None:
            r = simulate_t(mu, Ls, W, n_steps, seed, j, dof, v0=v0, horizons=horizons)
        else:
            r = simulate_paths_dd(mu, Ls, W, n_steps, seed, j, compounding, v0)
            r["V_h"] = simulate_horizons(mu, Ls, W, n_steps, seed, j, horizons, compounding, v0)["V_h"] if len(horizons) else None
        out.append(r)
    return {"V_T": interleave(out[0]["V_T"], out[1]["V_T"]), "q": interleave(out[0]["q"], out[1]["q"]),
            "V_h": interleave(out[0]["V_h"], out[1]["V_h"]) if len(horizons) else None}


def literal_pair_terminal(mu, chol, W, n_steps, seed, pairs, v0=1.0, compounding="simple"):
    """SPEC.md 2.3 as it is written, Gaussian draws: the normals of pair j from mc_oracle.step_normals at path id j, member s sees
    sigma z with sigma = +1, -1; r_i = mu_i + sum_j L_ij (sigma z_j) (j ascending, fma), rho = sum_i w_i r_i (i ascending, fma from
    +0), V = fma(V, rho, V) from fl32(v0) or S = S + rho from +0 -> [K, 2 len(pairs)] binary32, the pair's members adjacent."""
    mu = np.asarray(mu, np.float32) + np.float32(0)
    L = np.asarray(chol, np.float32)
    W = np.atleast_2d(np.asarray(W, np.float32))
    N, K = mu.shape[0], W.shape[0]
    out = np.empty((K, 2 * len(pairs)), np.float32)
    one = lambda v: np.full(1, v, np.float32)   # noqa: E731
    for c, j in enumerate(pairs):
        for s, sign in enumerate((np.float32(1), np.float32(-1))):
            V = np.full(K, 0.0 if compounding == "log" else v0, np.float32)
            for t in range(n_steps):
                z = sign * mc_oracle.step_normals(seed, int(j), t, N)[:N]
                r = np.empty(N, np.float32)
                for i in range(N):
                    acc = one(mu[i])
                    for jj in range(i + 1):
                        acc = _fma32(one(L[i, jj]), one(z[jj]), acc)
                    r[i] = acc[0]
                for k in range(K):
                    acc = one(0.0)
                    for i in range(N):
                        acc = _fma32(one(W[k, i]), one(r[i]), acc)
                    V[k] = V[k] + acc[0] if compounding == "log" else _fma32(one(V[k]), acc, one(V[k]))[0]
            out[:, 2 * c + s] = V
    return out


def pair_stats(x, c):
    """SPEC.md 5.10 in binary64 on the x [n] of one portfolio (n even, the pair's members adjacent) and its pivot c -> dict with the
    record's fields, and `abs_cross` = sum |summand| of cross, which bounds its rounding."""
    x = np.asarray(x, np.float64)
    n = x.size
    n_pairs = n // 2
    dp, dm = x[0::2] - c, x[1::2] - c
    cross = float(np.sum(dp * dm))
    mean = float(c + np.sum(x - c) / n)
    m2 = float(np.sum((x - mean) ** 2))
    s1 = (mean - c) * n
    C = cross - s1 * s1 / (2.0 * n)
    std = float(np.sqrt(m2 / (n - 1))) if n > 1 else 0.0
    return {"n_pairs": n_pairs, "cross": cross, "abs_cross": float(np.sum(np.abs(dp * dm))), "C": C, "m2": m2, "mean": mean,
            "pair_cov": C / (n_pairs - 1) if n_pairs >= 2 else 0.0,
            "pair_corr": 2.0 * C / m2 if m2 > 0 else 0.0,
            "mean_se": float(np.sqrt(max(m2 + 2.0 * C, 0.0) / (n * (n - 2.0)))) if n_pairs >= 2 else 0.0,
            "mean_se_iid": std / np.sqrt(n)}


def pair_mean_se(x):
    """np.std((x[0::2] + x[1::2]) / 2, ddof=1) / sqrt(n / 2): the standard error of the mean of the n / 2 independent pair means."""
    x = np.asarray(x, np.float64)
    y = 0.5 * (x[0::2] + x[1::2])
    return float(np.std(y, ddof=1) / np.sqrt(y.size))

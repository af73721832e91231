"""NumPy restatement of SPEC.md 4.19 (test helper, not a test module): volatility targeting -- the exposure e = fmin(tgt / sqrt(s), b)
on an EWMA of the path's own squared returns, cash at the riskless rate, borrowing at the spread on top, absorbing ruin -- on the
per-step portfolio returns that garch_ref.py (Gaussian, Student-t and GARCH draws: the GARCH walk serves all three) and jump_ref.py
already form, in binary32 in the spec's order; np.fmin / np.fmax are IEEE minNum / maxNum, as fminf / fmaxf, and NumPy's binary32
sqrt and division are correctly rounded.  Per path-step it also reports which branch the exposure took, whether the path borrowed
and whether it was still live.  Below it, a binary64 twin on given returns or on NumPy's own normals, the input sets of the GPU test
with their coverage assertions, and the assertions of the law test."""
from __future__ import annotations

import numpy as np

from garch_ref import garch_rho
from jump_ref import simulate_jumps
from oracle.np_oracle import _fma32

E_BELOW, E_BETWEEN, E_CAP = 0, 1, 2     # the branch of e: tgt / sqrt(s) < 1, in [1, b) -- or in [b, 1) under a cap below 1 --, and >= b
S_MAX = np.float32(2.0 ** 40)


def consts(vol_target):
    """(tgt, lam, oml, b, rf, sp) binary32 of vol_target = (target, decay, cap, rate, spread[, s0]); oml = fl32(1 - (double)lam)."""
    target, decay, cap, rate, spread = vol_target[:5]
    lam = np.float32(decay)
    return np.float32(target), lam, np.float32(1.0 - float(lam)), np.float32(cap), np.float32(rate), np.float32(spread)


def default_s0(chol, W):
    """s0_k = fl32(sum_j (sum_i W[k,i] L[i,j])^2), binary64 from the binary32 inputs, i and j ascending over the lower triangle."""
    L = np.tril(np.asarray(chol, np.float32)).astype(np.float64)
    W = np.atleast_2d(np.asarray(W, np.float32)).astype(np.float64)
    N = L.shape[0]
    out = np.zeros(W.shape[0])
    for k in range(W.shape[0]):
        q = 0.0
        for j in range(N):
            v = 0.0
            for i in range(j, N):
                v += W[k, i] * L[i, j]
            q += v * v
        out[k] = q
    return out.astype(np.float32)


def rho_of(mu, chol, W, T, seed, paths, dof=None, garch=None, jumps=None):
    """rho [K, T, n] binary32, the step's portfolio return exactly as the twin kernel forms it."""
    if jumps is not None:
        return simulate_jumps(mu, chol, W, T, seed, paths, jumps)["rho"]
    return garch_rho(mu, chol, W, T, seed, paths, garch if garch is not None else (0.0, 0.0, 1.0), dof)[0]


def walk(rho, vol_target, s0, v0=1.0, horizons=()):
    """SPEC.md 4.19 on rho [K, T, n] with s0 [K] binary32 -> dict(V_T [K, n], Y [K, n], q [K, n], V_h [H, K, n] or None, branch
    [K, T, n] int8, e [K, T, n] binary32, borrowed [K, T, n] bool (D > 0), live [K, T, n] bool (V > 0 before the step)):
        e = fmin(tgt / sqrt(s), b); E = fl32(e V); u = fma(V - E, rf, V); U = fma(E, rho, u); D = fmax(E - V, +0); U = fma(D, -sp, U);
        V = (V > 0 and U > 0) ? U : +0; Y = Y + e; s = fmin(fma(oml, fl32(rho rho), fl32(lam s)), 2^40);
    then the drawdown of SPEC.md 4.2 on V: P = fmax(P, V), q = fmin(q, V / P)."""
    tgt, lam, oml, b, rf, sp = consts(vol_target)
    rho = np.asarray(rho, np.float32)
    K, T, n = rho.shape
    hz = [int(h) for h in horizons]
    V = np.full((K, n), v0, np.float32)
    s = np.repeat(np.asarray(s0, np.float32).reshape(K, 1), n, axis=1)
    Y = np.zeros((K, n), np.float32)
    P = np.full((K, n), -np.inf, np.float32)
    q = np.ones((K, n), np.float32)
    branch = np.zeros((K, T, n), np.int8)
    es = np.zeros((K, T, n), np.float32)
    borrowed = np.zeros((K, T, n), bool)
    live = np.zeros((K, T, n), bool)
    Vh = np.empty((len(hz), K, n), np.float32) if hz else None
    zero = np.float32(0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for t in range(T):
            raw = (tgt / np.sqrt(s)).astype(np.float32)
            e = np.fmin(raw, b).astype(np.float32)
            branch[:, t] = np.where(raw >= b, E_CAP, np.where(raw < 1, E_BELOW, E_BETWEEN))
            es[:, t] = e
            live[:, t] = V > 0
            E = (e * V).astype(np.float32)
            rest = (V - E).astype(np.float32)
            D = np.fmax((E - V).astype(np.float32), zero).astype(np.float32)
            borrowed[:, t] = D > 0
            U = np.empty_like(V)
            for k in range(K):
                u = _fma32(rest[k], np.full(n, rf, np.float32), V[k])
                uk = _fma32(E[k], rho[k, t], u)
                U[k] = _fma32(D[k], np.full(n, -sp, np.float32), uk)
            V = np.where((V > 0) & (U > 0), U, zero).astype(np.float32)
            Y = (Y + e).astype(np.float32)
            g = (rho[:, t] * rho[:, t]).astype(np.float32)
            ls = (lam * s).astype(np.float32)
            for k in range(K):
                s[k] = np.fmin(_fma32(np.full(n, oml, np.float32), g[k], ls[k]), S_MAX)
            P = np.fmax(P, V)
            q = np.fmin(q, (V / P).astype(np.float32))
            if t + 1 in hz:
                Vh[hz.index(t + 1)] = V
    return {"V_T": V, "Y": Y, "q": q.astype(np.float32), "V_h": Vh, "branch": branch, "e": es, "borrowed": borrowed, "live": live}


def twin_on_rho(rho, vol_target, s0, v0=1.0):
    """The binary64 twin of walk() on the same returns rho [K, T, n] -> (V_T, Y) [K, n] binary64; the constants enter as their binary32
    roundings."""
    tgt, lam, oml, b, rf, sp = (float(x) for x in consts(vol_target))
    rho = np.asarray(rho, np.float32).astype(np.float64)
    K, T, n = rho.shape
    V = np.full((K, n), float(np.float32(v0)))
    s = np.repeat(np.asarray(s0, np.float32).astype(np.float64).reshape(K, 1), n, axis=1)
    Y = np.zeros((K, n))
    for t in range(T):
        e = np.minimum(tgt / np.sqrt(s), b)
        E = e * V
        U = E * rho[:, t] + ((V - E) * rf + V) - sp * np.maximum(E - V, 0.0)
        V = np.where((V > 0) & (U > 0), U, 0.0)
        Y = Y + e
        s = np.minimum(oml * rho[:, t] ** 2 + lam * s, 2.0 ** 40)
    return V, Y


def twin_values(mu, cov, w, T, n_paths, vol_target, seed, s0=None, v0=1.0, shares=False):
    """The binary64 twin of the rule on NumPy's own normals -> V_T [n_paths] of one portfolio `w`; vol_target as consts() takes it, its
    numbers entering as their binary32 roundings; s0 None: fl32(w' cov w).  shares=True -> (V_T, dict of the branch shares over the
    live path-steps and the share of ruined paths)."""
    tgt, lam, oml, b, rf, sp = (float(x) for x in consts(vol_target))
    mu, w = np.asarray(mu, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    cov = np.asarray(cov, np.float64)
    L = np.linalg.cholesky(cov)
    rng = np.random.default_rng(seed)
    V = np.full(n_paths, float(np.float32(v0)))
    s = np.full(n_paths, float(np.float32(w @ cov @ w)) if s0 is None else float(np.float32(s0)))
    cnt = np.zeros(4)
    for t in range(T):
        rho = (mu + rng.standard_normal((n_paths, mu.shape[0])) @ L.T) @ w
        raw = tgt / np.sqrt(s)
        e = np.minimum(raw, b)
        lv = V > 0
        cnt += [np.count_nonzero(lv), np.count_nonzero(lv & (raw >= b)), np.count_nonzero(lv & (raw < 1)), np.count_nonzero(lv & (raw >= 1) & (raw < b))]
        E = e * V
        U = E * rho + ((V - E) * rf + V) - sp * np.maximum(E - V, 0.0)
        V = np.where(lv & (U > 0), U, 0.0)
        s = np.minimum(oml * rho * rho + lam * s, 2.0 ** 40)
    if shares:
        return V, {"cap": cnt[1] / cnt[0], "below": cnt[2] / cnt[0], "between": cnt[3] / cnt[0], "ruined": float(np.mean(V == 0))}
    return V


# ---- the two input sets of the GPU test (the issue's A and B) ------------------------------------------------------------------------
SET_A = (0.05, 0.7, 1.2, 0.002, 0.001)   # on a market whose portfolio step volatility is about 0.05: all three branches of e
SET_B = (0.5, 0.7, 8.0, 0.002, 0.001)    # on about 0.08, T <= 12: always borrowing, the cap binding now and then, ruin


def scaled_chol(chol, W, vol):
    """`chol` scaled by one binary32 factor so that the mean portfolio step volatility sqrt(w' L L' w) of W is `vol`."""
    s0 = default_s0(chol, W).astype(np.float64)
    return (np.asarray(chol, np.float32) * np.float32(vol / np.sqrt(s0).mean())).astype(np.float32)


def shares(ref):
    """The shares the coverage assertions look at, over the live path-steps of a walk() result and over its paths."""
    lv = ref["live"]
    n_live = max(int(np.count_nonzero(lv)), 1)
    return {"cap": np.count_nonzero(lv & (ref["branch"] == E_CAP)) / n_live, "below": np.count_nonzero(lv & (ref["branch"] == E_BELOW)) / n_live,
            "between": np.count_nonzero(lv & (ref["branch"] == E_BETWEEN)) / n_live,
            "borrowed": np.count_nonzero(lv & ref["borrowed"]) / n_live, "ruined": float(np.mean(ref["V_T"] == 0))}


def covers(ref, which, T):
    """On the restatement, so that the check needs no GPU and parity cannot pass on one branch alone.  Set A, T >= 7: each of e = b,
    e < 1 and 1 < e < b takes >= 10 % of the live path-steps.  Set B, T >= 7: D > 0 on every live step, the cap binds on >= 10 % of
    them and 5 % to 50 % of the paths are ruined."""
    sh = shares(ref)
    print("coverage", which, "T", T, sh)
    if T < 7:
        return sh
    if which == "A":
        assert min(sh["cap"], sh["below"], sh["between"]) >= 0.10, sh
    else:
        assert sh["borrowed"] == 1.0 and sh["cap"] >= 0.10 and 0.05 <= sh["ruined"] <= 0.50, sh
    return sh


def law_checks(VT, mean, var=None):
    """The assertions of the law test on V_T [n] (binary32 from the device or binary64 from twin_values) against vol_target_law's exact
    (mean, var): the sample mean within 5 standard errors of `mean`, the standard error sqrt(m2 / n); with `var`, the sample variance
    (about `mean`) within 5 standard errors of it, the standard error from the sample's own fourth moment, sqrt((m4 - m2^2) / n).  5
    standard errors is the bound for two two-sided normal tests at a false-alarm rate below 1e-5; it is not fitted to any run.
    -> the figures in standard errors, for printing."""
    d = np.asarray(VT, np.float64) - mean
    n = d.size
    d2 = d * d
    m2 = d2.mean()
    z_mean = d.mean() / np.sqrt(m2 / n)
    out = {"z_mean": float(z_mean)}
    print("law: z_mean", z_mean, "mean", d.mean() + mean, "want", mean)
    assert abs(z_mean) < 5.0, (z_mean, d.mean() + mean, mean)
    if var is not None:
        z_var = (m2 - var) / np.sqrt((np.mean(d2 * d2) - m2 * m2) / n)
        print("law: z_var", z_var, "var", m2, "want", var)
        assert abs(z_var) < 5.0, (z_var, m2, var)
        out["z_var"] = float(z_var)
    return out

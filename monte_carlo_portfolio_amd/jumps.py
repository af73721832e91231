"""Merton jump-diffusion on the host (SPEC.md 2.5 / 4.12): the law of the market jump the path kernels draw, the split of a total
covariance into its diffusive part and the jump's, and a threshold estimator of the jump triple from return rows.

The kernels draw the count n of a path-step by comparing one uniform 32-bit word with eight thresholds, so the count's law is a
function of the thresholds alone; jump_law reads it off them, which makes every closed form below exact for what is simulated
(the Poisson tail beyond eight jumps is folded into n = 8: at intensity 1 that is a mass of 1e-5)."""
from __future__ import annotations

import collections

import numpy as np

from . import _ffi

JumpFit = collections.namedtuple("JumpFit", "intensity mean std loading n_jump_rows")
JumpLaw = collections.namedtuple("JumpLaw", "thresholds pmf mean_count var_count k3_count var_jump")

MAD_SCALE = 1.4826          # MAD -> standard deviation under normality
MAD_CUT = 3.0               # a row is a jump row when its centred market return is beyond 3 robust standard deviations


def _triple(jumps):
    lam, m, s = (float(v) for v in tuple(jumps)[:3])
    loading = jumps[3] if len(jumps) > 3 else None
    return lam, m, s, loading


def jump_law(jumps) -> JumpLaw:
    """The law of the count n and of the jump J of `jumps` = (intensity, mean, std[, loading]) as the kernels draw them:
    thresholds uint32 [8] (thr_k = floor(2^32 P(Poisson >= k))), pmf float64 [9] of n = 0 .. 8, the count's mean, variance and third
    central moment, and var_jump = s^2 E[n] + m^2 Var n with m, s rounded to binary32."""
    lam, m, s, _ = _triple(jumps)
    thr, mean_count, _ = _ffi.jump_consts(lam, m, s)
    upper = np.concatenate([[1.0], thr.astype(np.float64) / 2.0 ** 32, [0.0]])      # P(n >= k), k = 0 .. 9
    pmf = upper[:-1] - upper[1:]
    k = np.arange(9, dtype=np.float64)
    var_count = float(np.sum(pmf * (k - mean_count) ** 2))
    k3_count = float(np.sum(pmf * (k - mean_count) ** 3))
    m32, s32 = float(np.float32(m)), float(np.float32(s))
    return JumpLaw(thr, pmf, float(mean_count), var_count, k3_count, s32 * s32 * mean_count + m32 * m32 * var_count)


def _loading(jumps, n_assets):
    loading = _triple(jumps)[3]
    if loading is None:
        return np.ones(int(n_assets), np.float64)
    b = np.asarray(loading, np.float32).astype(np.float64).ravel()
    if b.size != int(n_assets):
        raise ValueError(f"jump loading has {b.size} entries, expected {n_assets}")
    return b


def diffusion_cov(cov, jumps, n_assets=None) -> np.ndarray:
    """cov - var_jump b b': the diffusive covariance of a jump-diffusion whose TOTAL per-step covariance is `cov` (SPEC.md 4.12:
    Cov(r) = L L' + Var(J) b b').  ValueError when what is left is not positive definite: the jumps alone would then carry more
    variance than the data show."""
    cov = np.asarray(cov, np.float64)
    n = cov.shape[0] if n_assets is None else int(n_assets)
    if cov.ndim != 2 or cov.shape != (n, n):
        raise ValueError(f"cov must be [{n}, {n}], got {cov.shape}")
    b = _loading(jumps, n)
    out = cov - jump_law(jumps).var_jump * np.outer(b, b)
    try:
        np.linalg.cholesky(out)
    except np.linalg.LinAlgError:
        raise ValueError("cov minus the jump covariance var_jump b b' is not positive definite: the jumps carry more variance than cov "
                         "holds (lower the intensity, the jump size or the loadings)") from None
    return out


def fit_jumps(returns) -> JumpFit:
    """A threshold estimate of the jump triple and the loadings from return rows [R, N] (a DataFrame or an array).  c_t is the
    equal-weight row mean; a row is a jump row when |c_t - median| > 3 * 1.4826 * MAD; intensity = jump rows / R (clipped to
    [0, 1]); mean and std are the mean and the ddof-1 standard deviation of c_t - median over the jump rows (std = 0 below two
    rows); b_i is the through-origin slope of asset i's centred return on c_t - median over the jump rows (1 without jump rows)."""
    vals = returns.to_numpy() if hasattr(returns, "to_numpy") else returns
    r = np.asarray(vals, np.float64)
    if r.ndim == 1:
        r = r[:, None]
    if r.ndim != 2 or r.shape[0] < 1 or not np.all(np.isfinite(r)):
        raise ValueError("fit_jumps wants a finite [R, N] array of return rows")
    R, N = r.shape
    c = r.mean(axis=1)
    med = float(np.median(c))
    d = c - med
    mad = float(np.median(np.abs(d)))
    rows = np.abs(d) > MAD_CUT * MAD_SCALE * mad
    k = int(np.count_nonzero(rows))
    if k == 0:
        return JumpFit(0.0, 0.0, 0.0, np.ones(N), 0)
    dj = d[rows]
    centred = r[rows] - np.median(r, axis=0)
    loading = centred.T @ dj / float(dj @ dj)
    return JumpFit(min(1.0, max(0.0, k / R)), float(dj.mean()), float(dj.std(ddof=1)) if k >= 2 else 0.0, loading, k)

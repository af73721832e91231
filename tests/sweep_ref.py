"""NumPy restatement of the sweep over historical rows, loop body app.py:708-713 for all rows of W at once (test helper, not a
test module): binary64 like the reference, plus the sums behind port_return, the variance and the tail mean evaluated in
np.longdouble with the sum of the absolute values of their terms, from which the GPU tests build their tolerances."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53          # unit roundoff of binary64


def series(R, W):
    """[rows, P] portfolio return series, accumulated in the kernels' order: assets ascending, multiply then add, no fused
    multiply-add (the library is built with -ffp-contract=off)."""
    R = np.asarray(R, np.float64)
    W = np.atleast_2d(np.asarray(W, np.float64))
    s = np.zeros((R.shape[0], W.shape[0]))
    for i in range(R.shape[1]):
        s = s + R[:, i:i + 1] * W[:, i][None, :]
    return s


def score(R, mean, cov, W, rf, alpha, s=None):
    """The five outputs of app.py:708-713 as float64 [P] arrays (port_return, port_std, sharpe, var_95, cvar_95), and
      n_tail                  the number of series elements <= var_95,
      ret_ld,  ret_abs        sum_i w_i mean_i in np.longdouble, and sum_i |w_i mean_i|,
      pvar_ld, pvar_abs       sum_ij w_i cov_ij w_j in np.longdouble, and sum_ij |w_i cov_ij w_j|,
      tail_ld, tail_abs       the mean of the tail elements in np.longdouble (var_95 where the tail is empty), and sum |x_tail|.
    `s`: series(R, W) where the caller has it already (it does not depend on alpha)."""
    R = np.asarray(R, np.float64)
    mean = np.asarray(mean, np.float64)
    cov = np.asarray(cov, np.float64)
    W = np.atleast_2d(np.asarray(W, np.float64))
    ld = np.longdouble
    s = series(R, W) if s is None else s
    var = np.percentile(s, (1 - alpha) * 100, axis=0)                       # app.py:259
    tail = s <= var[None, :]                                                # app.py:263
    n_tail = tail.sum(axis=0)
    xt = np.where(tail, s, 0.0)
    some = np.maximum(n_tail, 1)
    cvar = np.array([s[tail[:, p], p].mean() if n_tail[p] else var[p] for p in range(s.shape[1])])
    tail_ld = np.where(n_tail > 0, xt.astype(ld).sum(axis=0) / some.astype(ld), var.astype(ld))
    ret = W @ mean                                                          # app.py:708
    pvar = np.einsum("pi,ij,pj->p", W, cov, W)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(pvar)                                                 # app.py:709
        sharpe = np.where(std > 0, (ret - rf) / std, 0.0)                   # app.py:711
    rt = W.astype(ld) * mean.astype(ld)[None, :]
    vt = W.astype(ld)[:, :, None] * cov.astype(ld)[None, :, :] * W.astype(ld)[:, None, :]
    return {"port_return": ret, "port_std": std, "sharpe": sharpe, "var_95": var, "cvar_95": cvar, "n_tail": n_tail,
            "ret_ld": rt.sum(axis=1), "ret_abs": np.abs(rt).sum(axis=1).astype(np.float64),
            "pvar_ld": vt.sum(axis=(1, 2)), "pvar_abs": np.abs(vt).sum(axis=(1, 2)).astype(np.float64),
            "tail_ld": tail_ld, "tail_abs": np.abs(xt).sum(axis=0)}

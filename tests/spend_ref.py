"""NumPy restatement of SPEC.md 4.16 / 5.16 (test helper, not a test module): the walk of chosen paths under a spending rule, in
binary32 in the spec's order, on the per-step portfolio returns of cashflow_ref (Gaussian, Student-t, bootstrap), with the clamp
outcome of every live review; the five constants; the rule on the mean path in binary64 (the pivots); and the counts."""
from __future__ import annotations

import numpy as np

from cashflow_ref import boot_rho, counts_of, gauss_rho  # noqa: F401  (counts_of: the counts are SPEC.md 5.6's)
from oracle.np_oracle import _fma32

NEITHER, FLOOR, CEILING = 0, 1, 2


def consts(rate, down, up, inflation=0.0, first=None, v0=1.0):
    """(p32, g32, lo32, hi32, w0) of SPEC.md 4.16: the sums in binary64 rounded once; w0 = fl32(first) or fl32((double)p32 (double)fl32(v0))."""
    with np.errstate(over="ignore"):
        p32 = np.float32(rate)
        g32, lo32, hi32 = np.float32(1.0 + float(inflation)), np.float32(1.0 - float(down)), np.float32(1.0 + float(up))
        w0 = np.float32(first) if first is not None else np.float32(float(p32) * float(np.float32(v0)))
    return p32, g32, lo32, hi32, w0


def walk(rho, c, every, v0=1.0, horizons=()):
    """rho [K, T, n] binary32 per-step portfolio returns, c = consts(...) -> dict: V_T, Y_T [K, n]; V_h [H, K, n] or None; w [K, n]
    after the last review; outcome [R, K, n] int8 per review s = every, 2 every, .. <= T (-1: the path was not live at the review);
    bounds [R, 3, K, n] (lo bound, hi bound, new w) of every review; last_paid [K, n] the last positive payment; remainder [K, n]
    bool: the path was ruined on a step that paid a remainder U0 > 0."""
    rho = np.asarray(rho, np.float32)
    p32, g32, lo32, hi32, w0 = c
    K, T, n = rho.shape
    zero = np.float32(0.0)
    V = np.full((K, n), v0, np.float32)
    w = np.full((K, n), w0, np.float32)
    Y = np.zeros((K, n), np.float32)
    last = np.zeros((K, n), np.float32)
    rem = np.zeros((K, n), bool)
    out = np.empty((len(horizons), K, n), np.float32)
    want = {int(h): i for i, h in enumerate(horizons)}
    outcome, bounds = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(1, T + 1):
            U0 = _fma32(V, rho[:, s - 1], V)
            U = (U0 - w).astype(np.float32)
            live = (V > 0) & (U > 0)
            left = (V > 0) & (U0 > 0) & ~live
            paid = np.where(live, w, np.where(left, U0, zero)).astype(np.float32)
            rem |= left
            V = np.where(live, U, zero).astype(np.float32)
            Yn = (Y + paid).astype(np.float32)
            assert np.all(Yn >= Y)
            Y = Yn
            last = np.where(paid > 0, paid, last).astype(np.float32)
            if s in want:
                out[want[s]] = V
            if every >= 1 and s % every == 0:
                wp = (w * g32).astype(np.float32)
                aim, lo, hi = (p32 * V).astype(np.float32), (wp * lo32).astype(np.float32), (wp * hi32).astype(np.float32)
                w = np.fmin(np.fmax(aim, lo), hi).astype(np.float32)
                assert not np.any(np.isnan(w)) and not np.any(w < 0)
                inner = np.fmax(aim, lo)
                kind = np.where(inner > hi, CEILING, np.where(aim < lo, FLOOR, NEITHER))   # a NaN bound compares false: not taken
                outcome.append(np.where(V > 0, kind, -1).astype(np.int8))
                bounds.append(np.stack([lo, hi, w]))
    return {"V_T": V, "Y_T": Y, "V_h": out if len(horizons) else None, "w": w, "last_paid": last, "remainder": rem,
            "outcome": np.asarray(outcome, np.int8).reshape(len(outcome), K, n), "bounds": np.asarray(bounds, np.float32).reshape(len(bounds), 3, K, n)}


def simulate_sp(c, every, W, n_steps, seed, paths, mu=None, chol=None, dof=None, rows=None, block=1.0, v0=1.0, horizons=()):
    """Chosen path ids (path_begin included) -> the dict of walk() plus rho."""
    paths = np.asarray(paths, np.uint64)
    rho = boot_rho(rows, W, n_steps, seed, paths, block) if rows is not None else gauss_rho(mu, chol, W, n_steps, seed, paths, dof)
    res = walk(rho, c, every, v0, horizons)
    res["rho"] = rho
    return res


def mean_path(m, c, every, n_steps, v0=1.0, horizons=()):
    """SPEC.md 5.16: the rule on the mean path, binary64 on the doubles of the binary32 constants -> (c_V at T [K], c_V at the horizons
    [H, K], c_Y [K]); each 0 where not finite."""
    p, g, lo, hi, w0 = (np.float64(x) for x in c)
    v0d = float(np.float32(v0))

    def pivot(A):
        x = max(A, 0.0) / v0d - 1.0
        return x if np.isfinite(A) and np.isfinite(x) else 0.0
    at_T, at_h, at_Y = [], np.zeros((len(horizons), len(m))), []
    want = {int(h): i for i, h in enumerate(horizons)}
    with np.errstate(over="ignore", invalid="ignore"):
        for k, mk in enumerate(m):
            gk = np.float64(1.0) + np.float64(mk)
            A, w, Y = np.float64(v0d), np.float64(w0), np.float64(0.0)
            for s in range(1, n_steps + 1):
                A = A * gk
                A = A + (-w)
                Y = Y + w
                if s in want:
                    at_h[want[s], k] = pivot(float(A))
                if every >= 1 and s % every == 0:
                    wp = w * g
                    w = np.fmin(np.fmax(p * max(A, np.float64(0.0)), wp * lo), wp * hi)
            at_T.append(pivot(float(A)))
            x = float(Y) / v0d - 1.0
            at_Y.append(x if np.isfinite(x) else 0.0)
    return np.asarray(at_T), at_h, np.asarray(at_Y)


def outcome_shares(outcome):
    """Shares of (neither, floor, ceiling) among the live review path-steps of an outcome array (every portfolio pooled)."""
    live = outcome >= 0
    n = max(int(live.sum()), 1)
    return tuple(float(np.count_nonzero(outcome == k)) / n for k in (NEITHER, FLOOR, CEILING))

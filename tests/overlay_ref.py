"""NumPy restatement of SPEC.md 4.8 / 5.7 (test helper, not a test module): the option overlay of chosen paths in binary32 in the
spec's order -- the raw asset returns of the other restatements' draws (Gaussian and Student-t: the normals of
oracle.np_oracle.step_normals, the scale of student_t_ref.chi_and_scale), the price level of every asset that owns rows, the rows'
return, the weight dot -- and from the per-step portfolio returns the terminal values, the drawdown state and the values at
horizons exactly as student_t_ref does; the rule on a given price series in binary64 or binary32; and the pivot's deterministic
walk in binary64.  NumPy's binary32 "/" is correctly rounded, as the kernel's division is."""
from __future__ import annotations

import numpy as np

from drawdown_ref import drawdown_state
from horizons_ref import values_at_horizons
from oracle.np_oracle import _fma32, step_normals
from student_t_ref import chi_and_scale

LINEAR, CALL, PUT = 0, 1, 2


def _leg(kind, price, prev, strike, premium, dtype):
    """leg of one row: price - prev, or (d > 0 ? d : +0) - premium with d = price - strike (CALL) / strike - price (PUT)."""
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == LINEAR:
            return (price - prev).astype(dtype)
        d = (price - dtype(strike)).astype(dtype) if kind == CALL else (dtype(strike) - price).astype(dtype)
        pay = np.where(d > 0, d, dtype(0)).astype(dtype)
        return (pay - dtype(premium)).astype(dtype)


def rows_return32(rows, price, prev):
    """SPEC.md 4.8 for one asset, binary32 arrays price, prev [n]: num = fma(q_j, leg_j, num) over the rows in order from +0;
    r' = prev != 0 ? num / prev : +0."""
    price, prev = np.asarray(price, np.float32), np.asarray(prev, np.float32)
    num = np.zeros(price.shape, np.float32)
    for kind, strike, premium, qty in rows:
        num = _fma32(np.full(price.shape, qty, np.float32), _leg(int(kind), price, prev, np.float32(strike), np.float32(premium), np.float32), num)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(prev != 0, (num / np.where(prev != 0, prev, np.float32(1))).astype(np.float32), np.float32(0)).astype(np.float32)


def rows_return64(rows, price, prev):
    """The same rule in binary64 (a product then a sum per row, one division): what the pivot evaluates."""
    price, prev = np.asarray(price, np.float64), np.asarray(prev, np.float64)
    num = np.zeros(price.shape, np.float64)
    for kind, strike, premium, qty in rows:
        num = num + np.float64(qty) * _leg(int(kind), price, prev, np.float64(strike), np.float64(premium), np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(prev != 0, num / np.where(prev != 0, prev, 1.0), 0.0)


def series_returns(rows, prices, dtype=np.float64):
    """The rule along one price series [T + 1] (every step's price given, as options.calc_options_series sees it) -> [T]."""
    p = np.asarray(prices, dtype)
    fn = rows_return64 if dtype == np.float64 else rows_return32
    return fn(rows, p[1:], p[:-1])


def _asset_rows(overlay, i):
    table, begin, _ = overlay
    return [(int(r["kind"]), r["strike"], r["premium"], r["qty"]) for r in table[begin[i]:begin[i + 1]]]


def overlay_rho(mu, chol, W, n_steps, seed, paths, overlay=None, dof=None):
    """([K, T, n] binary32 per-step portfolio returns, {asset: its final prices [n]}) of SPEC.md 4.8: z' = fl32(s z) (Student-t) or z, r_i = mu_i + sum_j L_ij z'_j
    (j ascending, fma); an asset that owns rows: prev = P_i, price = fma(prev, r_i, prev), r'_i = rows_return32, P_i = price;
    rho_k = sum_i w_ki r'_i (i ascending, fma).  overlay: the (rows, row_begin, spot) triple of simulate.check_overlay or None."""
    mu = np.asarray(mu, np.float32) + np.float32(0)
    L = np.tril(np.asarray(chol, np.float32))
    W = np.atleast_2d(np.asarray(W, np.float32))
    N, K = mu.shape[0], W.shape[0]
    paths = np.asarray(paths, np.uint64)
    n = paths.size
    owned = {i: _asset_rows(overlay, i) for i in range(N)} if overlay is not None else {}
    owned = {i: r for i, r in owned.items() if r}
    P = {i: np.full(n, overlay[2][i], np.float32) for i in owned}
    rho = np.zeros((K, n_steps, n), np.float32)
    for t in range(n_steps):
        z = step_normals(seed, paths, t, N)[:, :N]
        if dof is not None:
            z = (chi_and_scale(seed, paths, t, dof)[1][:, None] * z).astype(np.float32)
        r = np.empty((n, N), np.float32)
        for i in range(N):
            acc = np.full(n, mu[i], np.float32)
            for j in range(i + 1):
                acc = _fma32(np.full(n, L[i, j], np.float32), z[:, j], acc)
            if i in owned:
                prev = P[i]
                with np.errstate(invalid="ignore", over="ignore"):
                    price = _fma32(prev, acc, prev)
                acc = rows_return32(owned[i], price, prev)
                P[i] = price
            r[:, i] = acc
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(K):
                acc = np.zeros(n, np.float32)
                for i in range(N):
                    acc = _fma32(np.full(n, W[k, i], np.float32), r[:, i], acc)
                rho[k, t] = acc
    return rho, P


def simulate_ov(mu, chol, W, n_steps, seed, paths, overlay=None, dof=None, v0=1.0, horizons=()):
    """Chosen path ids (path_begin included) -> dict(rho [K, T, n], V_T [K, n], q [K, n], V_h [H, K, n] or None, P {asset: final prices [n]}), binary32."""
    rho, P = overlay_rho(mu, chol, W, n_steps, seed, paths, overlay, dof)
    K, _, n = rho.shape
    VT = np.empty((K, n), np.float32)
    q = np.empty((K, n), np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(K):
            VT[k], q[k] = drawdown_state(rho[k], "simple", v0)
        Vh = values_at_horizons(rho, horizons, "simple", v0) if len(horizons) else None
    return {"rho": rho, "V_T": VT, "q": q, "V_h": Vh, "P": P}


def walk_pivots(overlay, mu, W, n_steps, horizons=()):
    """SPEC.md 5.7, binary64: P_i,0 = spot_i, per step price = prev (1 + mu_i), r'_i = rows_return64 (mu_i for an asset without
    rows), rho_k = sum_i W[k,i] r'_i (i ascending), A_k = A_k (1 + rho_k) from 1 -> (A_T - 1 [K], A_h - 1 [H, K]); 0 where not
    finite."""
    mu64 = (np.asarray(mu, np.float32) + np.float32(0)).astype(np.float64)
    W64 = np.atleast_2d(np.asarray(W, np.float32)).astype(np.float64)
    N, K = mu64.size, W64.shape[0]
    owned = {i: _asset_rows(overlay, i) for i in range(N)}
    P = np.asarray(overlay[2], np.float32).astype(np.float64)
    r = mu64.copy()
    A = np.ones(K)
    at_h = np.zeros((len(horizons), K))
    want = {int(h): i for i, h in enumerate(horizons)}
    fin = lambda c: c if np.isfinite(c) else 0.0   # noqa: E731
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(1, n_steps + 1):
            for i in range(N):
                if not owned[i]:
                    continue
                prev = P[i]
                price = prev * (1.0 + mu64[i])
                r[i] = float(rows_return64(owned[i], np.float64(price), np.float64(prev)))
                P[i] = price
            for k in range(K):
                rho = 0.0
                for i in range(N):
                    rho += W64[k, i] * r[i]
                A[k] = A[k] * (1.0 + rho)
            if t in want:
                at_h[want[t]] = [fin(a - 1.0) for a in A]
    return np.array([fin(a - 1.0) for a in A]), at_h

"""NumPy restatement of SPEC.md 4.18 (test helper, not a test module): tolerance-band rebalancing in binary32 in the spec's order on
the asset returns of rebalance_ref (gauss_returns / boot_returns), and a binary64 twin that tracks dollar holdings instead."""
from __future__ import annotations

import numpy as np

from oracle.np_oracle import _fma32
from rebalance_ref import _pad_w


def n_reviews(T, e):
    return (T - 1) // e if 1 <= e < T else 0


def pad_tol(tol, K, N, n4):
    """[K, n4] binary32: the table broadcast to [K, N], +inf (not watched) in the padding columns."""
    out = np.full((K, n4), np.inf, np.float32)
    out[:, :N] = np.broadcast_to(np.asarray(tol, np.float32), (K, N))
    return out


def banded(r, W, tol, every, cost=0.0, v0=1.0, horizons=()):
    """SPEC.md 4.18 on the asset returns r [T, n, N4] (binary32) -> dict(V_T [K, n], V_h [H, K, n] or None, c uint32 [K, n], Y binary32
    [K, n], hits bool [n_reviews, K, n]).  B is per portfolio: B_i = fma(B_i, r_i, B_i + r_i) every step; at the events (reviews s mod e
    == 0 < T, horizons, T) rho^ = W.B (i ascending over N4 from +0), V^ = fma(V, rho^, V); at a review, for watched i ascending,
    d = fl32(|B_i - rho^|), x = fl32(|W_i| d), g = fma(tol_i, rho^, tol_i), hit = OR (x >= g); where hit: tau = sum fma(|W_i|, |B_i -
    rho^|, tau) over all N4, rho' = fma(-kappa32, tau, rho^) (kappa32 > 0), V = fma(V, rho', V), B = +0, c += 1, Y = Y + tau."""
    r = np.asarray(r, np.float32)
    T, n, n4 = r.shape
    W = np.atleast_2d(np.asarray(W, np.float32))
    K, N = W.shape
    Wp = _pad_w(W, n4)
    tl = pad_tol(tol, K, N, n4)
    watched = np.isfinite(tl)
    kap = np.float32(cost)
    V = np.full((K, n), np.float32(v0), np.float32)
    B = np.zeros((K, n, n4), np.float32)
    c = np.zeros((K, n), np.uint32)
    Y = np.zeros((K, n), np.float32)
    hits = np.zeros((n_reviews(T, every), K, n), bool)
    want = {int(h): i for i, h in enumerate(horizons)}
    Vh = np.empty((len(horizons), K, n), np.float32) if len(horizons) else None
    nd = every if 1 <= every < T else T
    rev = 0
    for s in range(1, T + 1):
        rt = np.broadcast_to(r[s - 1][None], (K, n, n4))
        B = _fma32(B, rt, (B + rt).astype(np.float32))
        if s != nd and s != T and s not in want:
            continue
        rh = np.zeros((K, n), np.float32)
        for i in range(n4):
            rh = _fma32(np.broadcast_to(Wp[:, i:i + 1], (K, n)), B[:, :, i], rh)
        vh = _fma32(V, rh, V)
        if s in want:
            Vh[want[s]] = vh
        if s == T:
            V = vh
        elif s == nd:
            hit = np.zeros((K, n), bool)
            for i in range(n4):
                d = np.abs((B[:, :, i] - rh).astype(np.float32))
                x = (np.abs(Wp[:, i:i + 1]) * d).astype(np.float32)
                t_i = np.broadcast_to(np.where(watched[:, i:i + 1], tl[:, i:i + 1], np.float32(0)), (K, n)).astype(np.float32)
                g = _fma32(t_i, rh, t_i)
                with np.errstate(invalid="ignore"):
                    hit |= watched[:, i:i + 1] & (x >= g)
            tau = np.zeros((K, n), np.float32)
            for i in range(n4):
                d = np.abs((B[:, :, i] - rh).astype(np.float32))
                tau = _fma32(np.broadcast_to(np.abs(Wp[:, i:i + 1]), (K, n)), d, tau)
            rp = _fma32(np.full((K, n), -kap, np.float32), tau, rh) if kap > 0 else rh
            V = np.where(hit, _fma32(V, rp, V), V)
            B = np.where(hit[:, :, None], np.float32(0), B)
            c = c + hit.astype(np.uint32)
            Y = np.where(hit, (Y + tau).astype(np.float32), Y)
            hits[rev] = hit
            rev += 1
            nd = s + every if every < T - s else T
    return {"V_T": V, "V_h": Vh, "c": c, "Y": Y, "hits": hits}


def dollar_bands(r, W, tol, every, cost=0.0, v0=1.0):
    """binary64 twin of SPEC.md 4.18 that tracks the dollar holdings h_i of every asset (and the cash 1 - sum W at zero return), as
    rebalance_ref.dollar_holdings does: h_i *= 1 + r_i every step; at a review the portfolio is worth tot, asset i's weight is h_i /
    tot, and the path trades when a watched asset has |h_i - W_i tot| >= tol_i tot; the trade is dollar_holdings'.  -> dict(V_T [K, n],
    c [K, n], hits bool [n_reviews, K, n])."""
    r = np.asarray(r, np.float32).astype(np.float64)
    T, n, n4 = r.shape
    W = np.atleast_2d(np.asarray(W, np.float32))
    K, N = W.shape
    Wp = _pad_w(W, n4).astype(np.float64)
    tl = pad_tol(tol, K, N, n4).astype(np.float64)
    out = np.empty((K, n))
    cnt = np.zeros((K, n), np.uint32)
    hits = np.zeros((n_reviews(T, every), K, n), bool)
    for k in range(K):
        w = Wp[k]
        h = np.broadcast_to(v0 * w, (n, n4)).copy()
        cash = np.full(n, v0 * (1.0 - w.sum()))
        rev = 0
        for s in range(1, T + 1):
            h *= 1.0 + r[s - 1]
            if every >= 1 and s % every == 0 and s < T:
                tot = h.sum(axis=1) + cash
                off = np.abs(h - w[None, :] * tot[:, None])
                hit = np.any(np.isfinite(tl[k])[None, :] & (off >= np.where(np.isfinite(tl[k]), tl[k], 0.0)[None, :] * tot[:, None]), axis=1)
                after = tot - cost * off.sum(axis=1)
                h = np.where(hit[:, None], w[None, :] * after[:, None], h)
                cash = np.where(hit, (1.0 - w.sum()) * after, cash)
                cnt[k] += hit.astype(np.uint32)
                hits[rev, k] = hit
                rev += 1
        out[k] = h.sum(axis=1) + cash
    return {"V_T": out, "c": cnt, "hits": hits}

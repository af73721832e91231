"""NumPy restatement of SPEC.md 2.1 / 4.4 / 5.3 (test helper, not a test module): the row indices of the stationary block
bootstrap of chosen paths, their per-step portfolio returns in binary32 in the spec's order, the values at the end and at
horizons (horizons_ref.values_at_horizons), and the pivot of the moments."""
from __future__ import annotations

import math

import numpy as np

from horizons_ref import values_at_horizons
from oracle.np_oracle import _fma32, philox4x32_10

_MASK = np.uint64(0xFFFFFFFF)


def threshold(block) -> int:
    """thr = b == +inf ? 0 : min(2^32, floor(fl64(2^32 / b)))."""
    b = float(block)
    return 0 if math.isinf(b) else min(1 << 32, int(math.floor(2.0 ** 32 / b)))


def step_words(seed, paths, t):
    """x0, x1 of the Philox block of step t: counter (t, 1, p_lo, p_hi), key (seed_lo, seed_hi)."""
    paths = np.asarray(paths, np.uint64)
    x = philox4x32_10(np.uint64(t), np.uint64(1), paths & _MASK, paths >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
    return x[0], x[1]


def start_index(x0, n_rows):
    """mulhi(x0, R): the 32-bit word scaled to [0, R), exactly."""
    return ((np.asarray(x0, np.uint64) * np.uint64(n_rows)) >> np.uint64(32)).astype(np.int64)


def boot_indices(seed, paths, n_steps, n_rows, block):
    """[T, n] row indices j_t: a restart at t = 0 or when x1 < thr, else the next row circularly."""
    thr = threshold(block)
    paths = np.asarray(paths, np.uint64)
    out = np.empty((n_steps, paths.size), np.int64)
    j = np.zeros(paths.size, np.int64)
    for t in range(n_steps):
        x0, x1 = step_words(seed, paths, t)
        restart = np.full(paths.size, t == 0) | (x1.astype(np.int64) < thr)
        nxt = j + 1
        nxt[nxt == n_rows] = 0
        j = np.where(restart, start_index(x0, n_rows), nxt)
        out[t] = j
    return out


def row_returns(rows, W):
    """[K, R] binary32 rho_jk = fma chain over i = 0..N4-1 of W[k, i] * rows[j, i] from 0 (zero-padded to N4)."""
    rows = np.asarray(rows, np.float32)
    W = np.atleast_2d(np.asarray(W, np.float32))
    R, N = rows.shape
    acc = np.zeros((W.shape[0], R), np.float32)
    for i in range(4 * ((N + 3) // 4)):
        if i < N:
            acc = _fma32(np.broadcast_to(W[:, i:i + 1], acc.shape), np.broadcast_to(rows[None, :, i], acc.shape), acc)
        else:
            acc = _fma32(np.zeros_like(acc), np.zeros_like(acc), acc)
    return acc


def simulate_boot(rows, W, n_steps, seed, paths, block, compounding="simple", v0=1.0, horizons=()):
    """Chosen path ids (path_begin included) -> dict(idx [T, n], rho [K, T, n], V_T [K, n], V_h [H, K, n]), binary32 values."""
    rows = np.asarray(rows, np.float32)
    idx = boot_indices(seed, paths, n_steps, rows.shape[0], block)
    rr = row_returns(rows, W)
    rho = rr[:, idx]                                                   # [K, T, n]
    n = np.asarray(paths).size
    if n_steps == 0:
        VT = np.full((rr.shape[0], n), 0.0 if compounding == "log" else v0, np.float32)
    else:
        VT = values_at_horizons(rho, [n_steps], compounding, v0)[0]
    Vh = values_at_horizons(rho, list(horizons), compounding, v0) if len(horizons) else None
    return {"idx": idx, "rho": rho, "V_T": VT, "V_h": Vh, "row_rho": rr}


def boot_pivots(rows, W, n_steps, compounding="simple"):
    """SPEC.md 5.3 in binary64: rho_jk = sum_i W[k,i] rows[j,i] (i ascending), m = sum_j rho / R (j ascending),
    s2 = sum_j (rho - m)^2 / R; c = (1 + m)^T - 1 as expm1(T log1p(m)) (simple, 0 if m <= -1) or expm1(T (m + s2/2)) (log)."""
    rows = np.asarray(rows, np.float32).astype(np.float64)
    W = np.atleast_2d(np.asarray(W, np.float32)).astype(np.float64)
    out = []
    for w in W:
        rho = []
        for r in rows:
            v = 0.0
            for i in range(r.size):
                v += w[i] * r[i]
            rho.append(v)
        s = 0.0
        for v in rho:
            s += v
        m = s / len(rho)
        ss = 0.0
        for v in rho:
            ss += (v - m) * (v - m)
        s2 = ss / len(rho)
        if compounding == "log":
            c = math.expm1(n_steps * (m + 0.5 * s2))
        else:
            c = math.expm1(n_steps * math.log1p(m)) if m > -1.0 else 0.0
        out.append(c if math.isfinite(c) else 0.0)
    return np.asarray(out)

"""NumPy restatement of SPEC.md 4.3 / 5.2 (test helper, not a test module): the values of chosen paths after the steps of a
horizon list, in binary32 in the spec's order (the per-step returns of drawdown_ref.simulate_paths_dd), their x in binary64,
and NumPy's own percentile bookkeeping for the bands."""
from __future__ import annotations

import numpy as np

from drawdown_ref import simulate_paths_dd
from oracle.np_oracle import _fma32


def values_at_horizons(rho, horizons, compounding="simple", v0=1.0):
    """rho [K, T, n] binary32 per-step portfolio returns -> [H, K, n] binary32 V_h (simple: V = fma(V, rho, V) from v0) or
    S_h (log: S = S + rho from 0) after the steps h of `horizons`."""
    rho = np.asarray(rho, np.float32)
    K, T, n = rho.shape
    log = compounding == "log"
    V = np.full((K, n), 0.0 if log else v0, np.float32)
    out = np.empty((len(horizons), K, n), np.float32)
    want = {int(h): i for i, h in enumerate(horizons)}
    for t in range(T):
        V = (V + rho[:, t]).astype(np.float32) if log else _fma32(V, rho[:, t], V)
        if t + 1 in want:
            out[want[t + 1]] = V
    return out


def simulate_horizons(mu, chol, W, n_steps, seed, paths, horizons, compounding="simple", v0=1.0):
    """Chosen path ids (path_begin included) -> dict(V_T [K, n], V_h [H, K, n]), both binary32."""
    got = simulate_paths_dd(mu, chol, W, n_steps, seed, paths, compounding, v0)
    return {"V_T": got["V_T"], "V_h": values_at_horizons(got["rho"], horizons, compounding, v0)}


def x_of(v, compounding="simple", v0=1.0):
    """SPEC.md 5: x = (double)V / (double)(float)v0 - 1 (simple) or expm1((double)S) (log)."""
    v = np.asarray(v, np.float32).astype(np.float64)
    return np.expm1(v) if compounding == "log" else v / np.float64(np.float32(v0)) - 1.0


def lerp_rank(xs, lo, hi, gamma):
    """numpy's _lerp of the two order statistics of a sorted sample (the form mcp_percentile_rank's users evaluate)."""
    a, b = xs[lo], xs[hi]
    d = b - a
    return a + d * gamma if gamma < 0.5 else b - d * (1 - gamma)

"""Floor protection (SPEC.md 4.15 / 5.15): the floor schedule and the exact law of a CPPI walk.

floor_schedule builds the compounding floor that simulate_paths(protect=(floor, ...)) walks against, bit for bit what the
library's mcp_protect_floor builds; protect_law is the exact mean and variance of the terminal value on Gaussian draws while
neither the cap, a gap nor the ratchet acts, what the simulated moments are checked against.
"""
from __future__ import annotations

import math
import struct

import numpy as np


def _fma32(a, b, c) -> np.float32:
    """Correctly rounded binary32 fma(a, b, c) of three binary32 numbers: the product is exact in binary64, the sum is rounded to
    odd (TwoSum error term), so the rounding to binary32 is the only one."""
    p, c = float(a) * float(b), float(c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0.0 and math.isfinite(s):
        bits = struct.unpack("<q", struct.pack("<d", s))[0]
        if bits & 1 == 0:
            s = struct.unpack("<d", struct.pack("<q", bits + (1 if (err > 0) == (s > 0) else -1)))[0]
    return np.float32(s)


def floor_schedule(floor, rate, n_steps, v0=1.0) -> np.ndarray:
    """binary32 [n_steps + 1]: S_0 = fl32(floor v0) (the product in binary64), S_{t+1} = fma(S_t, fl32(rate), S_t) -- a floor that
    starts at the fraction `floor` of v0 and grows at the riskless rate per step.  Bit-equal to mcp_protect_floor(floor v0, rate,
    n_steps).  ValueError for a floor that is negative or not finite, rate <= -1, n_steps < 1 or a schedule that overflows."""
    f0, r = float(floor) * float(v0), float(rate)
    with np.errstate(over="ignore"):
        if not (math.isfinite(f0) and math.isfinite(r) and np.isfinite(np.float32(f0)) and np.isfinite(np.float32(r))):
            raise ValueError(f"floor={floor!r} (times v0) and rate={rate!r} must be finite, in binary32 too")
    if f0 < 0.0:
        raise ValueError(f"floor must be >= 0, got {floor!r}")
    if not (r > -1.0 and np.float32(r) > np.float32(-1.0)):
        raise ValueError(f"rate must be > -1, got {rate!r}")
    if int(n_steps) < 1:
        raise ValueError(f"n_steps must be >= 1, got {n_steps!r}")
    out = np.empty(int(n_steps) + 1, np.float32)
    out[0], r32 = np.float32(f0), np.float32(r)
    with np.errstate(over="ignore"):
        for t in range(int(n_steps)):
            out[t + 1] = _fma32(out[t], r32, out[t])
    if not np.all(np.isfinite(out)):
        raise ValueError("the floor schedule overflows binary32")
    return out


def protect_law(mu, cov, weights, n_steps, protect, v0=1.0):
    """(mean, var) of V_T on Gaussian draws while neither the cap, a gap nor the ratchet acts, exact, in binary64.  With the floor
    growing at the riskless rate the cushion C = V - S follows C' = C (1 + rf + m (rho - rf)), so with g = 1 + rf + m (w.mu - rf)
    and s2 = w' cov w: E[V_T] = S_T + (v0 - S_0) g^T and Var[V_T] = (v0 - S_0)^2 ((g^2 + m^2 s2)^T - g^(2T)).  weights [N] -> two
    floats; [K, N] -> two float64 [K] arrays.  `protect` as simulate_paths takes it; the weights, mu and the rule's numbers enter as
    the kernels see them, rounded to binary32."""
    from .simulate import check_protect
    pv = check_protect(protect, n_steps, v0)
    if pv is None:
        raise ValueError("protect_law needs a protect tuple")
    floor, m, rate, _, _ = pv
    m, rf = float(np.float32(m)), float(np.float32(rate))
    v, T = float(np.float32(v0)), int(n_steps)
    W = np.atleast_2d(np.asarray(weights, np.float32)).astype(np.float64)
    mu64 = np.asarray(mu, np.float32).astype(np.float64).ravel()
    cov64 = np.asarray(cov, np.float64)
    g = 1.0 + rf + m * (W @ mu64 - rf)
    s2 = np.einsum("ki,ij,kj->k", W, cov64, W)
    c0 = v - float(floor[0])
    mean = float(floor[T]) + c0 * g ** T
    var = c0 * c0 * ((g * g + m * m * s2) ** T - g ** (2 * T))
    if np.asarray(weights).ndim == 1:
        return float(mean[0]), float(var[0])
    return mean, var

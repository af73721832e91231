"""Spending rules (SPEC.md 4.16 / 5.16): the three named policies as parameter tuples, and the exact law of the percentage rule.

spending_rule builds the tuple that simulate_paths(spending=...) and simulate_bootstrap(spending=...) take; spending_law is the exact
mean and variance of the terminal value and the mean of the total paid out under the pure percentage rule on Gaussian draws, what the
simulated moments are checked against.
"""
from __future__ import annotations

import math

import numpy as np


def spending_rule(policy, rate, every=1, down=0.0, up=0.0, inflation=0.0, first=None):
    """The (rate, every, down, up, inflation, first) tuple of a named policy.
    "constant": the amount `first` (default rate times v0) every step, raised by `inflation` every `every` steps -- down = up = 0, so
    the value never moves it (the "4 % rule" with every = the steps of a year).
    "percentage": the fraction `rate` of the current value every step -- every = 1, down = 1, up = inf, no inflation.
    "floor_ceiling": between the two -- every `every` steps the withdrawal is inflated and then moved towards rate times the value,
    cut by at most `down` and raised by at most `up` per review ("dynamic spending")."""
    if policy == "constant":
        return (float(rate), int(every), 0.0, 0.0, float(inflation), first)
    if policy == "percentage":
        return (float(rate), 1, 1.0, math.inf, 0.0, None)
    if policy == "floor_ceiling":
        return (float(rate), int(every), float(down), float(up), float(inflation), first)
    raise ValueError(f"policy must be 'constant', 'percentage' or 'floor_ceiling', got {policy!r}")


def spending_law(mu, cov, weights, n_steps, rate, v0=1.0):
    """(mean of V_T, variance of V_T, mean of Y_T) under the pure percentage rule (every = 1, down = 1, up = inf, first absent) on
    Gaussian draws, exact, in binary64: V_s = V_{s-1} (1 + rho_s - p), so with a = 1 + w.mu - p and s2 = w' cov w, E[V_T] = v0 a^T,
    Var[V_T] = v0^2 ((a^2 + s2)^T - a^(2T)) and E[Y_T] = p v0 sum_{s<T} a^s.  weights [N] -> three floats; [K, N] -> three float64
    [K] arrays.  The weights, mu, the rate and v0 enter as the kernels see them, rounded to binary32.  The law leaves ruin out: it
    holds while p < 1 + rho on every step, which Gaussian draws break with a probability that is negligible at usual volatilities."""
    p, v, T = float(np.float32(rate)), float(np.float32(v0)), int(n_steps)
    W = np.atleast_2d(np.asarray(weights, np.float32)).astype(np.float64)
    mu64 = np.asarray(mu, np.float32).astype(np.float64).ravel()
    a = 1.0 + W @ mu64 - p
    s2 = np.einsum("ki,ij,kj->k", W, np.asarray(cov, np.float64), W)
    mean = v * a ** T
    var = v * v * ((a * a + s2) ** T - a ** (2 * T))
    paid = p * v * sum(a ** s for s in range(T))
    if np.asarray(weights).ndim == 1:
        return float(mean[0]), float(var[0]), float(paid[0])
    return mean, var, paid

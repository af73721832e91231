"""Volatility targeting (SPEC.md 4.19 / 5.19): the argument rules, the EWMA decay of a half-life and the exact law of a constant
exposure.

simulate_paths(vol_target=(target, decay[, cap[, rate[, spread[, s0]]]])) scales the exposure to the risky portfolio by target /
estimated volatility, the estimate an EWMA of the path's own squared returns; vol_target_law is the exact mean and variance of the
terminal value on Gaussian draws while the exposure is one number per portfolio -- a target so large that the cap always binds, or
decay = 1, which freezes the estimate at s0 -- and no path is ruined: what the simulated moments are checked against.
"""
from __future__ import annotations

import math

import numpy as np


def ewma_decay(halflife) -> float:
    """The decay whose weights halve every `halflife` steps: 0.5 ** (1 / halflife).  ValueError unless halflife is finite and > 0."""
    if isinstance(halflife, (bool, np.bool_)) or not isinstance(halflife, (int, float, np.integer, np.floating)):
        raise ValueError(f"halflife must be a number > 0, got {halflife!r}")
    h = float(halflife)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError(f"halflife must be finite and > 0, got {halflife!r}")
    return 0.5 ** (1.0 / h)


def check_vol_target(vol_target, n_portfolios=None):
    """SPEC.md 4.19 argument rules -> None (no targeting) or (target, decay, cap, rate, spread, s0 float64 [K] or None).
    `vol_target` is (target, decay[, cap[, rate[, spread[, s0]]]]), cap 1, rate 0, spread 0 and s0 None (the variance of the Gaussian
    part, per portfolio) by default.  target: the volatility aimed at, per step, > 0; decay: the EWMA's lambda in [0, 1]
    (ewma_decay(halflife)); cap: the largest exposure as a multiple of the value, > 0 (1: no leverage); rate: per step, > -1, earned on
    cash and paid on borrowing; spread: per step, >= 0, paid on top of rate on what is borrowed; s0: a number or one per portfolio, the
    initial variance estimate, finite and > 0.  ValueError for anything else: not a sequence of 2 to 6 entries, a bool or a string among
    the numbers, a value outside its range before or after rounding to binary32, an s0 of another length."""
    if vol_target is None:
        return None
    msg = f"vol_target must be (target, decay[, cap[, rate[, spread[, s0]]]]), got {vol_target!r}"
    if isinstance(vol_target, (str, bytes)) or not hasattr(vol_target, "__len__") or not 2 <= len(vol_target) <= 6:
        raise ValueError(msg)

    def number(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))

    def finite32(v):
        with np.errstate(over="ignore"):
            return bool(np.isfinite(v)) and bool(np.isfinite(np.float32(v)))
    vals = list(vol_target[:5]) + [1.0, 0.0, 0.0][len(vol_target[:5]) - 2:]
    if any(not number(v) for v in vals):
        raise ValueError(msg)
    target, decay, cap, rate, spread = (float(v) for v in vals)
    if not all(finite32(v) for v in (target, decay, cap, rate, spread)):
        raise ValueError(f"vol_target values must be finite, in binary32 too, got {vol_target!r}")
    if not (target > 0.0 and np.float32(target) > 0.0):
        raise ValueError(f"vol_target target must be > 0, got {target!r}")
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f"vol_target decay must be in [0, 1], got {decay!r}")
    if not (cap > 0.0 and np.float32(cap) > 0.0):
        raise ValueError(f"vol_target cap must be > 0, got {cap!r}")
    if not (rate > -1.0 and np.float32(rate) > np.float32(-1.0)):
        raise ValueError(f"vol_target rate must be > -1, got {rate!r}")
    if not spread >= 0.0:
        raise ValueError(f"vol_target spread must be >= 0, got {spread!r}")
    s0 = vol_target[5] if len(vol_target) == 6 else None
    if s0 is not None:
        if isinstance(s0, (str, bytes, bool, np.bool_)) or any(not number(v) for v in np.asarray(s0, object).ravel().tolist()):
            raise ValueError(msg)
        s0 = np.asarray(s0, np.float64).ravel()
        if n_portfolios is not None:
            if s0.size == 1:
                s0 = np.repeat(s0, int(n_portfolios))
            if s0.size != int(n_portfolios):
                raise ValueError(f"vol_target s0 must be one number or one per portfolio ({int(n_portfolios)}), got {s0.size}")
        with np.errstate(over="ignore", under="ignore"):
            s32 = s0.astype(np.float32)
        if not (np.all(np.isfinite(s0)) and np.all(s0 > 0.0) and np.all(np.isfinite(s32)) and np.all(s32 > 0)):
            raise ValueError(f"vol_target s0 must be finite and > 0, in binary32 too, got {vol_target[5]!r}")
        s0 = np.ascontiguousarray(s0)
    return target, decay, cap, rate, spread, s0


def vol_target_law(mu, cov, weights, n_steps, vol_target, v0=1.0):
    """(mean, var) of V_T on Gaussian draws while the exposure is the constant e_k = min(target / sqrt(s0_k), cap) and no path is
    ruined, exact, in binary64: with g = 1 + rf + e (w.mu - rf) - spread max(e - 1, 0) and s2 = w' cov w, E[V_T] = v0 g^T and
    Var[V_T] = v0^2 ((g^2 + e^2 s2)^T - g^(2T)).  That is the walk's law with decay = 1, or with a target so large that the cap
    always binds.  s0 None: s0_k = s2_k.  weights [N] -> two floats; [K, N] -> two float64 [K] arrays.  `vol_target` as simulate_paths
    takes it; the weights, mu and the rule's numbers enter as the kernels see them, rounded to binary32."""
    W = np.atleast_2d(np.asarray(weights, np.float32)).astype(np.float64)
    vt = check_vol_target(vol_target, W.shape[0])
    if vt is None:
        raise ValueError("vol_target_law needs a vol_target tuple")
    target, _, cap, rate, spread, s0 = vt
    tgt, b, rf, sp = (float(np.float32(v)) for v in (target, cap, rate, spread))
    v, T = float(np.float32(v0)), int(n_steps)
    mu64 = np.asarray(mu, np.float32).astype(np.float64).ravel()
    cov64 = np.asarray(cov, np.float64)
    s2 = np.einsum("ki,ij,kj->k", W, cov64, W)
    s0k = s2.astype(np.float32).astype(np.float64) if s0 is None else s0.astype(np.float32).astype(np.float64)
    e = np.minimum(tgt / np.sqrt(s0k), b)
    g = 1.0 + rf + e * (W @ mu64 - rf) - sp * np.maximum(e - 1.0, 0.0)
    mean = v * g ** T
    var = v * v * ((g * g + e * e * s2) ** T - g ** (2 * T))
    if np.asarray(weights).ndim == 1:
        return float(mean[0]), float(var[0])
    return mean, var


def vol_target_blocks(consts, s0, out, n_steps, alpha, target, store):
    """The 'vol_target' block of every portfolio: the binary32 constants and s0 as used, the first step's exposure, the ruined paths
    and those below `target`, with horizons the same per horizon and, without the drawdown, the record of the per-path average
    exposure Y / n_steps (the library reduces x = Y - 1: shifted back and divided here)."""
    tgt, lam, oml, b, rf, sp = (float(v) for v in consts)
    n = int(out.stats[0]["n"])
    T = float(n_steps)
    blocks = []
    for k in range(out.counts.shape[0]):
        e0 = float(np.minimum(np.float32(tgt) / np.sqrt(np.float32(s0[k])), np.float32(b)))
        blk = {"target": tgt, "decay": lam, "one_minus_decay": oml, "cap": b, "rate": rf, "spread": sp, "s0": float(s0[k]), "exposure0": e0,
               "target_value": target, "n_ruined": int(out.counts[k, 0]), "ruin_probability": float(out.counts[k, 0]) / n,
               "n_short": int(out.counts[k, 1]), "shortfall_probability": float(out.counts[k, 1]) / n}
        if out.hz_counts is not None:
            c = out.hz_counts[:, k, :]
            blk["horizons"] = {"n_ruined": c[:, 0].astype(np.int64), "ruin_probability": c[:, 0].astype(np.float64) / n,
                               "n_short": c[:, 1].astype(np.int64), "shortfall_probability": c[:, 1].astype(np.float64) / n}
        if out.exposure_stats is not None:
            r = out.exposure_stats[k]
            blk["exposure"] = {"mean": (float(r["mean"]) + 1.0) / T, "std": float(r["std"]) / T, "quantile": (float(r["var"]) + 1.0) / T,
                               "level": 1.0 - float(alpha), "min": (float(r["min"]) + 1.0) / T, "max": (float(r["max"]) + 1.0) / T}
            if store:
                blk["exposure"]["paths"] = out.exposure[k]
        blocks.append(blk)
    return blocks

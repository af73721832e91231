"""Glide paths (SPEC.md 4.14 / 5.14): builders and the exact law of scheduled target weights.

glide_path builds the (breaks, targets) pair that simulate_paths(glide=...) and simulate_bootstrap(glide=...) take, a linear move
from one weight vector to another in equal steps; glide_law is the exact mean and variance of the terminal return of such a walk
on Gaussian draws without cash flows, what the simulated moments are checked against.
"""
from __future__ import annotations

import numpy as np

from . import _ffi


def glide_path(start, end, n_steps, every):
    """(breaks, targets) of a linear glide from `start` to `end` over n_steps steps that moves every `every` steps.

    breaks = every, 2 every, ... < n_steps (G of them); the walk has G + 1 segments and segment j holds start + (end - start) j / G:
    segment 0 is `start` itself -- pass it as the call's weights -- and targets holds the segments 1 .. G, the last one `end`.
    start and end are [N] (targets [G, N]) or [K, N] (targets [K, G, N]).  ValueError when the shapes differ, when no break fits
    (every >= n_steps) or when more than 64 do."""
    a, b = np.asarray(start, np.float64), np.asarray(end, np.float64)
    if a.shape != b.shape or a.ndim not in (1, 2):
        raise ValueError(f"start and end must both be [N] or [K, N], got {a.shape} and {b.shape}")
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)) or int(every) < 1:
        raise ValueError(f"every must be a whole number of steps >= 1, got {every!r}")
    breaks = np.arange(int(every), int(n_steps), int(every), dtype=np.int32)
    G = int(breaks.size)
    if G == 0:
        raise ValueError(f"no break fits: every={every} must be below n_steps={n_steps}")
    if G > _ffi.MCP_MAX_GLIDE:
        raise ValueError(f"{G} breaks, at most {_ffi.MCP_MAX_GLIDE}: raise every={every}")
    frac = np.arange(1, G + 1, dtype=np.float64) / G
    if a.ndim == 1:
        targets = a[None, :] + (b - a)[None, :] * frac[:, None]
        targets[-1] = b                                    # the last segment is `end` itself, not start + (end - start) rounded
    else:
        targets = a[:, None, :] + (b - a)[:, None, :] * frac[None, :, None]
        targets[:, -1, :] = b
    return breaks, targets


def segment_of_steps(breaks, n_steps) -> np.ndarray:
    """int [n_steps]: the segment g(s) = #{j : breaks[j] < s} of every step s = 1 .. n_steps (SPEC.md 4.14)."""
    br = np.asarray(breaks, np.int64).ravel()
    return np.searchsorted(br, np.arange(1, int(n_steps) + 1), side="left")


def glide_law(mu, cov, weights, glide, n_steps):
    """(mean, var) of x_T = V_T / v0 - 1 on Gaussian draws without cash flows, exact, in binary64: with m_s = w_s.mu and
    v_s = w_s' cov w_s on the weights w_s of step s, E[x_T] = prod_s (1 + m_s) - 1 and Var[x_T] = prod_s ((1 + m_s)^2 + v_s) -
    prod_s (1 + m_s)^2 (the steps are independent).  weights [N] -> two floats; [K, N] -> two float64 [K] arrays.  glide is the
    (breaks, targets) pair of simulate_paths; the weights, targets and mu enter as the kernels see them, rounded to binary32."""
    from .simulate import check_glide
    gl = check_glide(glide, weights, n_steps)
    if gl is None:
        raise ValueError("glide_law needs a (breaks, targets) pair")
    W = np.atleast_2d(np.asarray(weights, np.float32)).astype(np.float64)
    mu64 = np.asarray(mu, np.float32).astype(np.float64).ravel()
    cov64 = np.asarray(cov, np.float64)
    seg = segment_of_steps(gl[0], n_steps)
    mean, var = np.zeros(W.shape[0]), np.zeros(W.shape[0])
    for k in range(W.shape[0]):
        ws = np.concatenate([W[k][None, :], gl[1][:, k, :].astype(np.float64)], axis=0)   # [G + 1, N]
        m = ws @ mu64
        v = np.einsum("gi,ij,gj->g", ws, cov64, ws)
        p1 = p2 = 1.0
        for g in seg:
            p1 *= 1.0 + m[g]
            p2 *= (1.0 + m[g]) ** 2 + v[g]
        mean[k], var[k] = p1 - 1.0, p2 - p1 * p1
    if np.asarray(weights).ndim == 1:
        return float(mean[0]), float(var[0])
    return mean, var

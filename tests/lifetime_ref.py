"""NumPy restatement of SPEC.md 4.17 / 5.17 (test helper, not a test module): the lifetime l of chosen paths on the cash-flow, glide
and spending walks of cashflow_ref, glide_ref and spend_ref -- every step's stored value from those restatements, l = #{s : V_s > 0}
-- and the survival statistics of a sample of lifetimes."""
from __future__ import annotations

import numpy as np

import cashflow_ref
import glide_ref
import spend_ref


def lifetime_of(v_steps, K, n):
    """V_s of every step s = 1 .. T ([T, K, n] binary32, or None at T = 0) -> l [K, n] uint32 = #{s : V_s > 0}."""
    if v_steps is None:
        return np.zeros((K, n), np.uint32)
    return np.count_nonzero(np.asarray(v_steps) > 0, axis=0).astype(np.uint32)


def simulate_life(W, n_steps, seed, paths, flows=None, glide=None, spending=None, v0=1.0, horizons=(), **draws):
    """Chosen path ids (path_begin included) -> dict(l [K, n] uint32, V_T [K, n], V_h [H, K, n] or None, V_s [T, K, n] or None, and
    Y_T with a spending rule).  flows [T]: the cash-flow walk, with glide = (breaks, targets) on the glide path; spending = (c, every)
    with c = spend_ref.consts(...): the spending walk.  `draws`: mu, chol[, dof] or rows, block."""
    paths = np.asarray(paths, np.uint64)
    W = np.atleast_2d(np.asarray(W, np.float32))
    every_step = tuple(range(1, int(n_steps) + 1))
    if spending is not None:
        res = spend_ref.simulate_sp(spending[0], spending[1], W, n_steps, seed, paths, v0=v0, horizons=every_step, **draws)
    elif glide is not None:
        res = glide_ref.simulate_glide(glide[0], glide[1], flows, W, n_steps, seed, paths, v0=v0, horizons=every_step, **draws)
    else:
        res = cashflow_ref.simulate_cf(flows, W, n_steps, seed, paths, v0=v0, horizons=every_step, **draws)
    v_steps = res["V_h"]
    out = {"l": lifetime_of(v_steps, W.shape[0], paths.size), "V_T": res["V_T"], "V_s": v_steps,
           "V_h": v_steps[[h - 1 for h in horizons]] if len(horizons) else None}
    if spending is not None:
        out["Y_T"] = res["Y_T"]
    return out


def survival_stats(life, n_steps, levels=()):
    """l [n] -> (hist uint64 [T + 1], life_sum, the order statistics at `levels` percent) with NumPy: np.bincount, np.sum and
    np.percentile(method="lower")."""
    life = np.asarray(life, np.int64).ravel()
    hist = np.bincount(life, minlength=int(n_steps) + 1).astype(np.uint64)
    q = np.array([np.percentile(life, lv, method="lower") for lv in levels], np.int64).astype(np.uint32)
    return hist, int(life.sum()), q

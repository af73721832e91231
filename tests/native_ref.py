"""Float64 reference of the native-math kernels (MCP_FLAG_NATIVE_MATH, `native_math=True`): NumPy, no device.  Test infrastructure.

The native kernels draw their normals by Box-Muller on the hardware's v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32
(box_muller_native, csrc/mcp_device.h).  Those values are outside SPEC.md's exact arithmetic, but the transform is a plain formula
on two binary32 inputs, and this module evaluates it in binary64 on the same Philox words (SPEC.md section 3, last paragraph):

    u     = fma(fl32(xa), 2^-32, 2^-32)        binary32, in [2^-32, 1]
    turns = fl32(xb) 2^-32                     binary32, in [0, 1]
    R     = sqrt(-2 ln u),   z_sin = R sin(2 pi turns),   z_cos = R cos(2 pi turns)        binary64 from those two binary32 values

Block q of step t is Philox(t NB + q, 0, p_lo, p_hi) as in np_oracle.step_normals; its words (x0, x1) give the assets q (sin) and
NB + q (cos), its words (x2, x3) the assets 2 NB + q (sin) and 3 NB + q (cos).

B bounds a kernel's draw against this reference: |z_gpu - z_ref| <= B max(1, R).  It is measured, not chosen
(tests/test_gpu_native.py::test_the_measurement_case): the largest scaled deviation over the 2^20 draws of that case, times four,
rounded up to a power of two; the factor of four covers the word pairs that were not drawn (the error of the four instructions is
piecewise smooth).  B_CAP is a condition on the kernels, not a measurement: every mistake the draw tests exist for moves a draw by
O(0.1 .. 1), and at 2^-13 they are still three orders of magnitude away from rounding.

TOLERANCE OF A FULL WALK (walk(), tolerance()).  A native kernel's terminal value against simulate_native_f64, per path and
portfolio k, summed over the steps t with R_max(t) = max(1, largest radius of the path's slots in step t):

    the draws' share      B R_max ||L' w_k||_1                                        every z_j is off by at most B R_max
    rounding allowance    (2N + 2) 2^-24 sum_i |w_ki| (|mu_i| + R_max sum_j |L_ij|)   the binary32 fma chains of SPEC.md section 4
    simple compounding    both times the largest |V_t| along the path (V_0 = v0 included), plus 2^-24 of it per step

The last term is the rounding of the update V = fma(V, rho, V) itself, at most half an ulp of the new value per step.  It does not scale
with rho, so no multiple of the two parts above covers it, and tests/test_native_ref_cpu.py shows that the exact binary32 walk of
the spec needs it (at N = 3 it exceeds the rounding allowance alone 2.7 times) and needs nothing more.  Log compounding's
S = S + rho rounds relative to |S| <= sum |rho| and stays inside the allowance.  Nothing here is measured except B.
"""
from __future__ import annotations

import collections

import numpy as np

from oracle import np_oracle

# measured on an MI355X (gfx950), 2^20 draws of seed 7 (test_the_measurement_case): largest |z_gpu - z_ref| / max(1, R)
MEASURED_MAX = 2.344e-7        # asset 3 of path 42412; the largest seen in any other case of tests/test_gpu_native.py is 2.330e-7
B = 2.0 ** -20                 # 9.54e-7: 4 x MEASURED_MAX = 9.38e-7, rounded up to a power of two
B_CAP = 2.0 ** -13             # 1.2e-4: B may not exceed it
U32 = 2.0 ** -24               # unit roundoff of binary32

_TWO_M32 = np.float32(2.0 ** -32)


def block_words(seed: int, paths, step: int, nb: int, q: int):
    """The four uint32 words of Philox block q of `step` for every path id."""
    paths = np.asarray(paths, np.uint64)
    return np_oracle.philox4x32_10(np.uint64(step * nb + q), np.uint64(0), paths & np.uint64(0xFFFFFFFF), paths >> np.uint64(32),
                                   seed & 0xFFFFFFFF, seed >> 32)


def pair_inputs(xa, xb):
    """(u, turns): the two binary32 inputs of the transform, from the radius word xa and the angle word xb."""
    u = np_oracle._fma32(np.asarray(xa, np.uint32).astype(np.float32), _TWO_M32, _TWO_M32)
    turns = np.asarray(xb, np.uint32).astype(np.float32) * _TWO_M32          # a power-of-two scaling: exact
    return u, turns


def box_muller_f64(xa, xb):
    """(z_sin, z_cos, R) in binary64 from one word pair."""
    u, turns = pair_inputs(xa, xb)
    R = np.sqrt(-2.0 * np.log(u.astype(np.float64))) + 0.0                   # + 0.0: R = 0, not -0, at u = 1
    a = 2.0 * np.pi * turns.astype(np.float64)
    return R * np.sin(a), R * np.cos(a), R


def native_step_normals(seed: int, paths, step: int, n_assets: int):
    """(z, R), both float64 [n_paths, N4]: the native normal of every asset slot of one step and the radius it was drawn with."""
    nb = (n_assets + 3) // 4
    paths = np.asarray(paths, np.uint64)
    z = np.empty((paths.shape[0], 4 * nb))
    R = np.empty_like(z)
    for q in range(nb):
        x = block_words(seed, paths, step, nb, q)
        for pair in range(2):
            zs, zc, r = box_muller_f64(x[2 * pair], x[2 * pair + 1])
            z[:, 2 * pair * nb + q], z[:, (2 * pair + 1) * nb + q] = zs, zc
            R[:, 2 * pair * nb + q] = R[:, (2 * pair + 1) * nb + q] = r
    return z, R


def market(N: int, K: int):
    """(mu, L, W) in binary32, read-only: a market in which no two numbers can change places unnoticed, after the one of
    tests/test_gpu_lean_gemv.py -- a drift with N distinct non-zero entries of both signs, a dense lower-triangular factor with
    N (N + 1) / 2 distinct non-zero entries of both signs (a positive diagonal), and K weight rows of both signs, distinct within a
    row and from row to row.  Its proportions are chosen so that tests/test_native_ref_cpu.py can show that a swapped weight, a
    shifted drift or a transposed factor moves nearly every path by far more than the tolerance: asset 0 carries 60 .. 80 % of
    every portfolio, column 0 of the factor is eight times the rest (so L w and L' w differ in size, not only in order), and the
    drift is of the size of a step's volatility, 0.04 at asset 0 against -0.03 .. at the last."""
    i = np.arange(N, dtype=np.float64)
    mu = np.where(i % 2 == 0, 0.04, -0.03) * (1.0 - 0.5 * i / N)
    if N % 2 == 1 and N > 1:
        mu[N - 1] = -0.031                                                  # the last asset against asset 0, whatever N's parity
    L = np.zeros((N, N))
    r, c = np.tril_indices(N)
    L[r, c] = 1e-3 * (0.5 + np.arange(r.size) / r.size) * np.where((r + c) % 4 == 3, -1.0, 1.0)
    L[np.arange(N), np.arange(N)] = 1.5e-3 + 1e-3 * i / N
    L[:, 0] = 8e-3 * (1.0 + 0.5 * i / N)
    L[0, 0] = 2.03e-3
    k = np.arange(K, dtype=np.float64)[:, None]
    raw = (1.0 + i[None, :] + 0.37 * ((i[None, :] * (k + 1.0)) % 5.0)) * np.where((i[None, :] + k) % 3 == 2, -0.5, 1.0)
    W = np.empty((K, N))
    W[:, 0] = 0.6 + 0.2 * ((k[:, 0] * 0.6180339887) % 1.0) if N > 1 else 1.0 + 0.1 * k[:, 0]
    if N > 1:
        W[:, 1:] = raw[:, 1:] / np.abs(raw[:, 1:]).sum(axis=1, keepdims=True) * (1.0 - W[:, :1])
    mu32, L32, W32 = mu.astype(np.float32), L.astype(np.float32), W.astype(np.float32)
    low = L32[np.tril_indices(N)]
    assert np.unique(low).size == low.size and np.all(low != 0.0) and np.all(np.triu(L32, 1) == 0.0)
    assert np.unique(mu32).size == N and np.all(mu32 != 0.0) and all(np.unique(w).size == N for w in W32)
    assert np.unique(W32, axis=0).shape[0] == K
    for a in (mu32, L32, W32):
        a.setflags(write=False)
    return mu32, L32, W32


Walk = collections.namedtuple("Walk", "terminal draws rounding update")


def walk(mu, chol, W, n_steps: int, n_paths: int, seed: int, path_begin: int = 0, v0: float = 1.0,
         compounding: str = "simple") -> Walk:
    """The float64 walk of SPEC.md section 4 on the native normals, inputs as the kernels get them (binary32 mu [N], chol [N, N]
    lower, W [K, N]), in the natural `z @ L.T`, `r @ W.T` form of np_oracle.simulate.  -> Walk, every field float64 [K, n_paths]:
    terminal (V_T, or S_T for 'log') and the three parts of the tolerance in the module's docstring -- `draws` per unit of B,
    `rounding` the allowance of the fma chains, `update` the rounding of V's own update (0 for 'log')."""
    mu = np.asarray(mu, np.float32).astype(np.float64)
    L = np.asarray(chol, np.float32).astype(np.float64)                     # as given: a test may pass a factor that is not lower
    W = np.atleast_2d(np.asarray(W, np.float32)).astype(np.float64)
    N, K = mu.shape[0], W.shape[0]
    paths = np.arange(path_begin, path_begin + n_paths, dtype=np.uint64)
    log = compounding == "log"
    V = np.full((n_paths, K), 0.0 if log else float(np.float32(v0)))
    vmax = np.abs(V)
    draws = np.zeros((n_paths, K))
    rounding = np.zeros((n_paths, K))
    update = np.zeros((n_paths, K))
    share = np.abs(L.T @ W.T).sum(axis=0)                                   # ||L' w_k||_1, [K]
    drift = np.abs(W) @ np.abs(mu)                                          # sum_i |w_ki| |mu_i|
    spread = np.abs(W) @ np.abs(L).sum(axis=1)                              # sum_i |w_ki| sum_j |L_ij|
    for t in range(n_steps):
        z, R = native_step_normals(seed, paths, t, N)
        rmax = np.maximum(1.0, R.max(axis=1))[:, None]                      # over all N4 slots: an upper bound for the N live ones
        z = z[:, :N]
        rho = (mu + z @ L.T) @ W.T
        V = V + rho if log else V * (1.0 + rho)
        draws += rmax * share
        rounding += (2 * N + 2) * U32 * (drift + rmax * spread)
        if not log:
            vmax = np.maximum(vmax, np.abs(V))
    if not log:
        draws, rounding, update = draws * vmax, rounding * vmax, n_steps * U32 * vmax
    return Walk(V.T.copy(), draws.T.copy(), rounding.T.copy(), update.T.copy())


def simulate_native_f64(mu, chol, W, n_steps: int, n_paths: int, seed: int, path_begin: int = 0, v0: float = 1.0,
                        compounding: str = "simple") -> np.ndarray:
    """Terminal values [K, n_paths] float64 of the walk on the native normals."""
    return walk(mu, chol, W, n_steps, n_paths, seed, path_begin, v0, compounding).terminal


def tolerance(w: Walk, b: float = B) -> np.ndarray:
    """[K, n_paths]: how far a native kernel's terminal value may lie from w.terminal (the module's docstring)."""
    return b * w.draws + w.rounding + w.update

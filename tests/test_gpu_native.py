"""The native-math kernels (MCP_FLAG_NATIVE_MATH) against the float64 evaluation of their own Box-Muller on the same Philox words
(tests/native_ref.py), draw by draw and walk by walk.

STAGE A reads every draw back.  One step in log compounding with mu = 0, chol = 2^-3 I and a unit weight vector e_i gives
S = 2^-3 z_i with no rounding (every fma has a zero or a one in it, and the MFMA sweep forms rho from one non-zero product per row),
so z_gpu = 8 S is bit for bit what block_normals<true> produced for asset i.  In simple compounding V = fl32(1 + z / 8) gives z to
within 8 2^-24, which is added to the bound for those cases only.  Asserted for every path and asset: the value is finite and
|z_gpu - z_ref| <= B max(1, R), B measured (native_ref.B; test_the_measurement_case) and capped at 2^-13.  An exchanged sin / cos,
a pair taken as (x0, x2), an angle taken from the radius word, a draw in another asset's slot or another constant all move a draw by
O(0.1 .. 1).

STAGE B walks T = 2 and 7 steps of a market with a dense factor, weights of both signs and a large drift (native_ref.market) on
every kernel family and compares the terminal values with native_ref.simulate_native_f64 within native_ref.tolerance: only these
kernels feed the drift and the weights of the full walk from SGPRs.
"""
import functools
import json
import os

import numpy as np
import pytest

import native_ref as nr
from monte_carlo_portfolio_amd import simulate_paths
from monte_carlo_portfolio_amd.engine import PathEngine

pytestmark = pytest.mark.gpu

SEED = 7
TWO32 = 1 << 32
SIMPLE_READBACK = 8 * 2.0 ** -24           # z from V = fl32(1 + z / 8), V in [1/4, 2): half an ulp of V is at most 2^-24
EXTREMES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_extremes.json")))


@functools.lru_cache(maxsize=None)
def reference(N, P, path_begin):
    """(z, R) float64 [P, N4] of step 0, computed once per configuration and shared (read-only)."""
    z, R = nr.native_step_normals(SEED, np.arange(path_begin, path_begin + P, dtype=np.uint64), 0, N)
    z.setflags(write=False)
    R.setflags(write=False)
    return z, R


def gpu_draws(N, W, P, comp, path_begin=0):
    """z_gpu float64 [K, P]: row k is the kernel's draw of the asset that the unit vector W[k] selects."""
    W = np.atleast_2d(np.asarray(W, np.float64))
    assert np.all((W == 0) | (W == 1)) and np.all(W.sum(axis=1) == 1)
    kw = dict(n_steps=1, n_paths=P, seed=SEED, compounding=comp, store=True, path_begin=path_begin, chol=np.eye(N) / 8, native_math=True)
    if W.shape[0] == 1:
        term = simulate_paths(np.zeros(N), None, W[0], **kw)["terminal"][None, :]
    else:
        term = simulate_paths(np.zeros(N), None, W, as_array=True, **kw)[1]
    assert term.dtype == np.float32 and term.shape == (W.shape[0], P)
    term = term.astype(np.float64)
    return 8.0 * (term if comp == "log" else term - 1.0)


def scaled_deviation(z_gpu, assets, N, P, comp, path_begin=0):
    """[K, P]: (|z_gpu - z_ref| less the read-back error of simple compounding) / max(1, R); z_gpu[k] is the draw of assets[k]."""
    z, R = reference(N, P, path_begin)
    assert np.all(np.isfinite(z_gpu))
    dev = np.abs(z_gpu - z[:, assets].T) - (SIMPLE_READBACK if comp == "simple" else 0.0)
    return dev / np.maximum(1.0, R[:, assets].T)


def assert_draws(z_gpu, assets, N, P, comp, path_begin=0):
    s = scaled_deviation(z_gpu, assets, N, P, comp, path_begin)
    k, p = np.unravel_index(np.argmax(s), s.shape)
    print(f"N={N} K={len(assets)} {comp}: largest scaled deviation {s[k, p]:.3e} (asset {assets[k]}, path {path_begin + p})")
    assert s[k, p] <= nr.B, (f"asset {assets[k]}, path {path_begin + p}: z_gpu {z_gpu[k, p]!r}, z_ref {reference(N, P, path_begin)[0][p, assets[k]]!r}, "
                             f"scaled deviation {s[k, p]:.3e} > B = {nr.B:.3e}")
    return s[k, p]


# ---- Stage A -------------------------------------------------------------------------------------------------------------------

ONE_CASES = [(N, "log") for N in (1, 2, 3, 4, 5, 8, 13, 16, 17, 33, 61, 64)] + [(N, "simple") for N in (4, 16, 64)]


@pytest.mark.parametrize("N,comp", ONE_CASES)
def test_one_portfolio_kernel_every_draw(gpu_ctx, N, comp):
    """mc_paths_kernel<NB, 1, 1, true, false, LOGC>, NB = 1, 2, 4, 5, 9, 16 and ragged N: every asset, one call each; 257 paths are two
    workgroups, the second with one live lane."""
    P = 257
    z_gpu = np.concatenate([gpu_draws(N, np.eye(N)[i], P, comp) for i in range(N)])
    assert_draws(z_gpu, list(range(N)), N, P, comp)


def boundary_rows(N, K=16):
    """K assets of N > 16: the slot boundaries m NB + q with q in {0, NB - 1}, asset N - 1, then the assets next to them to fill up."""
    nb = (N + 3) // 4
    cand = [m * nb + q for m in range(4) for q in (0, nb - 1)] + [N - 1] + [m * nb + q for q in range(1, nb - 1) for m in range(4)]
    rows = list(dict.fromkeys(a for a in cand if a < N))[:K]
    assert len(rows) == K
    return rows


@pytest.mark.parametrize("comp", ["log", "simple"])
@pytest.mark.parametrize("N", [2, 3, 4, 5, 8, 13, 16, 17, 33, 64])
def test_eight_portfolio_kernel_every_draw(gpu_ctx, N, comp):
    """mc_paths_kernel<NB, 8, 1, true, false, LOGC>: W = I_N for N <= 16 (K = N; N > 8 runs two passes), 16 boundary rows beyond."""
    P = 300
    assets = list(range(N)) if N <= 16 else boundary_rows(N)
    assert_draws(gpu_draws(N, np.eye(N)[assets], P, comp), assets, N, P, comp)


SWEEP_DRAW_CASES = ([(4 * nb, 129, "log") for nb in range(1, 17)]                              # shared MT 2, every NB
                    + [(16, K, c) for K in (17, 33, 65, 128, 300, 385, 520) for c in ("log", "simple")]    # the other branches of sweep_plan
                    + [(20, K, c) for K in (17, 128, 129, 300) for c in ("log", "simple")])


@pytest.mark.parametrize("N,K,comp", SWEEP_DRAW_CASES)
def test_sweep_kernels_every_draw(gpu_ctx, N, K, comp):
    """The NATIVE instantiations of mc_sweep_kernel and mc_sweep_shared_kernel: rows e_(k mod N); 130 paths are three 64-path wave
    tiles, the last with two live paths."""
    P = 130
    assets = [k % N for k in range(K)]
    assert_draws(gpu_draws(N, np.eye(N)[assets], P, comp), assets, N, P, comp)


@pytest.mark.parametrize("N,K,P", [(16, 1, 257), (13, 13, 300), (20, 129, 130)])
def test_path_ids_across_two_to_the_32(gpu_ctx, N, K, P):
    """path_begin = 2^32 - 100: both counter words change inside the launch, once on each family."""
    assets = [N - 1] if K == 1 else [k % N for k in range(K)]
    assert_draws(gpu_draws(N, np.eye(N)[assets], P, "log", TWO32 - 100), assets, N, P, "log", TWO32 - 100)


def test_the_measurement_case(gpu_ctx, record_property):
    """2^20 draws (N = 4, W = I_4, 2^18 paths, one step): the largest scaled deviation seen is what native_ref.B is set from."""
    N, P = 4, 1 << 18
    worst = assert_draws(gpu_draws(N, np.eye(N), P, "log"), list(range(N)), N, P, "log")
    record_property("largest_scaled_deviation", float(worst))
    record_property("B", nr.B)


@pytest.mark.parametrize("entry", EXTREMES["entries"], ids=lambda e: f"{e['what']}-{e['path']}")
def test_extreme_words(gpu_ctx, entry):
    """The ends of the transform (tests/golden/native_extremes.json): 64 paths around each entry on the one-portfolio and the
    8-portfolio kernel.  Everything is finite and inside Stage A's bound; where u rounds to 1 the radius is 0 and both draws of the
    pair are within B of 0.  Observed on the MI355X: at all three entries both draws come back as exact zeros, on both kernels, as the
    code says they should (log2(1) = 0, sqrt(-0) = -0)."""
    N, P, pb, j = 4, 64, entry["path"] - 17, 17
    assert entry["seed"] == SEED and EXTREMES["n_assets"] == N and EXTREMES["step"] == 0 and entry["block"] == 0
    one = np.concatenate([gpu_draws(N, np.eye(N)[i], P, "log", pb) for i in range(N)])
    eight = gpu_draws(N, np.eye(N), P, "log", pb)
    for z_gpu in (one, eight):
        assert_draws(z_gpu, list(range(N)), N, P, "log", pb)
        if entry["what"] == "u_one":
            pair = z_gpu[[entry["word"], entry["word"] + 1], j]
            print("u = 1:", pair)
            assert reference(N, P, pb)[1][j, entry["word"]] == 0.0 and np.all(np.abs(pair) <= nr.B)


# ---- Stage B -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def walk_reference(N, K, T, P, path_begin, v0, comp):
    mu, L, W = nr.market(N, K)
    return nr.walk(mu, L, W, T, P, SEED, path_begin, v0, comp)


def assert_walk(N, K, T, P, path_begin, v0, comp):
    mu, L, W = nr.market(N, K)
    kw = dict(n_steps=T, n_paths=P, seed=SEED, v0=v0, compounding=comp, store=True, path_begin=path_begin, chol=L, native_math=True)
    got = simulate_paths(mu, None, W[0], **kw)["terminal"][None, :] if K == 1 else simulate_paths(mu, None, W, as_array=True, **kw)[1]
    ref = walk_reference(N, K, T, P, path_begin, v0, comp)
    assert got.dtype == np.float32 and got.shape == ref.terminal.shape and np.all(np.isfinite(got))
    ratio = np.abs(got.astype(np.float64) - ref.terminal) / nr.tolerance(ref)
    k, p = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"N={N} K={K} T={T} v0={v0} {comp}: largest deviation / tolerance {ratio[k, p]:.3f}")
    assert ratio[k, p] <= 1.0, (f"T={T} v0={v0} {comp}: portfolio {k}, path {path_begin + p}: {got[k, p]!r} against {ref.terminal[k, p]!r}, "
                                f"{ratio[k, p]:.3g} tolerances")


@pytest.mark.parametrize("K", [1, 9, 40, 300])
@pytest.mark.parametrize("N", [3, 5, 16, 17, 64])
def test_full_walk_against_the_float64_evaluation(gpu_ctx, N, K):
    """K = 1: the one-portfolio kernel; 9: two passes of the 8-portfolio kernel; 40: the per-wave sweep kernel (N <= 16) or the shared
    one with MT 1; 300: the shared sweep kernel with MT 2 and the smaller one behind it.  Observed on the MI355X: at most 0.71 of the
    tolerance (N = 3, K = 300, T = 2, simple, v0 = 1)."""
    for T in (2, 7):
        for comp in ("simple", "log"):
            for v0 in (1.0, 3.0):
                assert_walk(N, K, T, 257, 0, v0, comp)


@pytest.mark.parametrize("comp", ["simple", "log"])
def test_full_walk_across_two_to_the_32(gpu_ctx, comp):
    assert_walk(17, 9, 7, 257, TWO32 - 100, 3.0, comp)


def test_path_engine_runs_the_same_native_kernel(gpu_ctx):
    """PathEngine(native_math=True).launch_paths_only -- what bench.py times for roofline.native_math_kernel -- leaves bit for bit the
    terminal values of simulate_paths(native_math=True)."""
    N, T, P = 16, 3, 513
    mu, L, W = nr.market(N, 1)
    eng = PathEngine(mu, L, W, T, P, native_math=True)
    eng.launch_paths_only(SEED)
    got = eng.terminal()
    eng.close()
    want = simulate_paths(mu, None, W[0], n_steps=T, n_paths=P, seed=SEED, store=True, chol=L, native_math=True)["terminal"]
    assert got.dtype == np.float32 and got.shape == (1, P)
    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32))

"""What tests/native_ref.py and the tolerances of tests/test_gpu_native.py rest on, without a device: the law of the reference
draws, their layout, the fixture of extreme words, the rounding allowance of the full walk, and how far the mistakes the full walk
is there for stand out of its tolerance."""
import itertools
import json
import os

import numpy as np
import pytest
from scipy.special import ndtr

import native_ref as nr
from oracle import np_oracle

SEED = 7
WALK_SHAPES = list(itertools.product((3, 5, 16, 17, 64), (1, 9, 40, 300), (2, 7), ("simple", "log"), (1.0, 3.0)))    # Stage B: N, K, T, compounding, v0
P = 257


def test_b_is_four_times_the_measured_maximum_and_within_its_cap():
    assert nr.B_CAP == 2.0 ** -13 and nr.B <= nr.B_CAP
    assert np.log2(nr.B) == np.round(np.log2(nr.B)) and nr.B / 2 < 4 * nr.MEASURED_MAX <= nr.B


def test_the_law_of_the_reference_draws():
    """2^20 blocks of one seed (N = 4: one block per path).  The Kolmogorov statistic of the 2^21 draws of the first word pair against
    N(0, 1) is below the critical value at 10^-6, sqrt(ln(2e6) / 2) / sqrt(2^21) = 1.9e-3 (measured 7.6e-4); mean and variance of
    all draws within 5 standard errors; z_sin with z_cos of a pair, and the draws of two asset slots fed by different pairs, are
    uncorrelated within 5 standard errors.  With Stage A of tests/test_gpu_native.py -- the kernels' draws are these to within B --
    this is what "statistically equivalent" rests on."""
    n = 1 << 20
    z, R = nr.native_step_normals(SEED, np.arange(n, dtype=np.uint64), 0, 4)
    assert z.shape == (n, 4) and np.all(np.isfinite(z)) and np.all(R[:, 0] == R[:, 1]) and np.all(R[:, 2] == R[:, 3])
    x = np.sort(z[:, :2].ravel())
    cdf = ndtr(x)
    i = np.arange(1, x.size + 1)
    ks = max(np.max(i / x.size - cdf), np.max(cdf - (i - 1) / x.size))
    print(f"Kolmogorov statistic {ks:.2e}")
    assert ks < np.sqrt(np.log(2e6) / 2) / np.sqrt(x.size) < 1.9e-3
    m = z.size
    assert abs(z.mean()) < 5 / np.sqrt(m)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / m)
    for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (0, 3)):
        assert abs(np.mean(z[:, a] * z[:, b])) < 5 / np.sqrt(n), (a, b)
    assert abs(np.mean(z[:-1, 0] * z[1:, 0])) < 5 / np.sqrt(n)                 # neighbouring paths


@pytest.mark.parametrize("nb", [1, 3, 16])
def test_the_layout_of_the_reference_draws(nb):
    """Slot m NB + q is built from word pair m / 2 of block q = Philox(t NB + q, 0, p_lo, p_hi), sin for even m and cos for odd m: the
    block np_oracle.step_normals takes that slot's word from.  Recomputed here from the Philox words with NumPy's own arithmetic."""
    step = 2
    paths = np.array([0, 1, 77, (1 << 32) - 1, 1 << 32, (5 << 32) + 123], np.uint64)
    z, R = nr.native_step_normals(SEED, paths, step, 4 * nb)
    spec = np_oracle.step_normals(SEED, paths, step, 4 * nb)
    for q in range(nb):
        x = np_oracle.philox4x32_10(np.uint64(step * nb + q), np.uint64(0), paths & np.uint64(0xFFFFFFFF), paths >> np.uint64(32),
                                    SEED & 0xFFFFFFFF, SEED >> 32)
        for m in range(4):
            assert np.array_equal(spec[:, m * nb + q], np_oracle.normals(x[m]))                        # the same block, word m
            xa, xb = x[2 * (m // 2)], x[2 * (m // 2) + 1]
            u = (xa.astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -32).astype(np.float32)   # exact sum, one rounding
            turns = (xb.astype(np.float32).astype(np.float64) * 2.0 ** -32).astype(np.float32)
            radius = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
            angle = 2.0 * np.pi * turns.astype(np.float64)
            want = radius * (np.sin(angle) if m % 2 == 0 else np.cos(angle))
            assert np.array_equal(z[:, m * nb + q], want) and np.array_equal(R[:, m * nb + q], radius), (q, m)


def test_the_fixture_of_extreme_words():
    """Every entry of tests/golden/native_extremes.json has the property it claims, recomputed from Philox."""
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_extremes.json")))
    assert fx["n_assets"] == 4 and fx["step"] == 0
    whats = [e["what"] for e in fx["entries"]]
    assert {"u_one", "xa_min", "turns_one", "xb_min", "quarter", "half", "three_quarters"} == set(whats)
    for e in fx["entries"]:
        x = nr.block_words(e["seed"], np.array([e["path"]], np.uint64), 0, 1, e["block"])[e["word"]]
        assert int(x[0]) == e["x"] and e["path"] < 1 << fx["log2_paths_scanned"], e
        radius_word = e["word"] in (0, 2)
        assert radius_word == (e["what"] in ("u_one", "xa_min")), e
        u, turns = nr.pair_inputs(x, x)
        z, R = nr.native_step_normals(e["seed"], np.array([e["path"]], np.uint64), 0, 4)
        if e["what"] == "u_one":
            assert u[0] == np.float32(1.0) and R[0, e["word"]] == 0.0 and np.all(z[0, e["word"]:e["word"] + 2] == 0.0)
        elif e["what"] == "xa_min":
            assert e["x"] < 64 and R[0, e["word"]] > 6.0                      # 2^27 words scanned: the smallest is below 2^6 (p = 1 - 2e-4)
        elif e["what"] == "turns_one":
            assert turns[0] == np.float32(1.0)
        elif e["what"] == "xb_min":
            assert e["x"] < 64 and turns[0] < 2.0 ** -26
        else:
            target = {"quarter": 0.25, "half": 0.5, "three_quarters": 0.75}[e["what"]]
            assert abs(e["x"] - target * 2.0 ** 32) < 128 and abs(float(turns[0]) - target) < 2.0 ** -25


def exact_binary32_walk(mu, L, W, T, n, path_begin, v0, comp):
    """np_oracle.simulate(..., exact=True)'s order of operations -- SPEC.md section 4 in binary32 with single-rounding fma -- fed with the
    reference normals rounded to binary32 -> [K, n] float32."""
    N, K = mu.shape[0], W.shape[0]
    paths = np.arange(path_begin, path_begin + n, dtype=np.uint64)
    V = np.full((n, K), 0.0 if comp == "log" else np.float32(v0), np.float32)
    for t in range(T):
        z = nr.native_step_normals(SEED, paths, t, N)[0][:, :N].astype(np.float32)
        r = np.empty((n, N), np.float32)
        for i in range(N):
            acc = np.full(n, mu[i], np.float32)
            for j in range(i + 1):
                acc = np_oracle._fma32(np.full(n, L[i, j], np.float32), z[:, j], acc)
            r[:, i] = acc
        for k in range(K):
            rho = np.zeros(n, np.float32)
            for i in range(N):
                rho = np_oracle._fma32(np.full(n, W[k, i], np.float32), r[:, i], rho)
            V[:, k] = V[:, k] + rho if comp == "log" else np_oracle._fma32(V[:, k], rho, V[:, k])
    return V.T


@pytest.mark.parametrize("N", [3, 5, 16, 17, 64])
def test_the_exact_binary32_walk_stays_inside_the_rounding_allowance(N):
    """At every Stage B shape with K <= 9: the spec's binary32 walk on the (rounded) reference normals lies within the rounding part of
    the tolerance -- no share of B -- of the float64 walk.  In simple compounding that needs the rounding of V's own update: the fma
    chains' allowance alone is exceeded at small N (asserted at N = 3, where it is missed 2.7 times over), which is why
    native_ref.tolerance carries the term."""
    worst = chains_only = 0.0
    for _, K, T, comp, v0 in (s for s in WALK_SHAPES if s[0] == N and s[1] <= 9):
        mu, L, W = nr.market(N, K)
        w = nr.walk(mu, L, W, T, P, SEED, 0, v0, comp)
        d = np.abs(exact_binary32_walk(mu, L, W, T, P, 0, v0, comp).astype(np.float64) - w.terminal)
        assert np.all(w.update == 0.0) or comp == "simple"
        worst = max(worst, float(np.max(d / (w.rounding + w.update))))
        if comp == "simple":
            chains_only = max(chains_only, float(np.max(d / w.rounding)))
    print(f"N={N}: largest deviation / allowance {worst:.3f}; in simple compounding without the update's term {chains_only:.3f}")
    assert worst <= 1.0
    assert N != 3 or chains_only > 1.0


@pytest.mark.parametrize("N", [3, 5, 16, 17, 64])
def test_mistakes_stand_out_of_the_tolerance(N):
    """At every Stage B shape, with B at its cap of 2^-13: two swapped weights (the first and the last asset's), the drift shifted by
    one asset and the transposed factor each move more than 90 % of the paths of every portfolio by more than 100 tolerances."""
    for _, K, T, comp, v0 in (s for s in WALK_SHAPES if s[0] == N):
        mu, L, W = nr.market(N, K)
        w = nr.walk(mu, L, W, T, P, SEED, 0, v0, comp)
        tol = nr.tolerance(w, nr.B_CAP)
        swapped = np.array(W)
        swapped[:, [0, N - 1]] = swapped[:, [N - 1, 0]]
        for name, args in (("weights", (mu, L, swapped)), ("drift", (np.roll(mu, 1), L, W)), ("factor", (mu, L.T, W))):
            moved = np.abs(nr.walk(*args, T, P, SEED, 0, v0, comp).terminal - w.terminal) > 100 * tol
            assert moved.mean(axis=1).min() > 0.9, (name, K, T, comp, v0, float(moved.mean(axis=1).min()))


def test_simulate_native_f64_is_the_walk_and_partitions_by_path():
    mu, L, W = nr.market(5, 3)
    whole = nr.simulate_native_f64(mu, L, W, 4, 100, SEED, (1 << 32) - 50, 3.0, "simple")
    parts = np.concatenate([nr.simulate_native_f64(mu, L, W, 4, 50, SEED, (1 << 32) - 50 + 50 * g, 3.0, "simple") for g in range(2)], axis=1)
    assert whole.shape == (3, 100) and np.allclose(whole, parts, rtol=1e-13, atol=0)
    assert np.array_equal(whole, nr.walk(mu, L, W, 4, 100, SEED, (1 << 32) - 50, 3.0, "simple").terminal)

"""The lean Gaussian kernel's factor step (mc_paths_lean_kernel: two row pairs in flight, their accumulators interleaved column
by column) against the CPU oracle, bit for bit on every path: float32 terminal values compared with == on their bit patterns,
no tolerance.

The inputs are chosen so that a swapped row, column, row pair or weight changes a bit: a dense lower-triangular factor whose
entries are all distinct, unequal weights and a non-zero, unequal drift.  N = 1, 4, 5, 8, 9, 12, 13, 16 runs NB = 1..4 Philox
blocks per step with a full and a padded last block; T = 1, 2, 7; n_paths = 1, 257 (a full tile plus one lane) and 513; both
compoundings.  One more case crosses 2^32 in its path range, so it stays on mc_paths_kernel (mcp::lean_range,
tests/test_lean_route_cpu.py) and must give the oracle's values too.
"""
import functools

import numpy as np
import pytest

from monte_carlo_portfolio_amd import simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import prepare_inputs
from oracle import mc_oracle

pytestmark = pytest.mark.gpu

SEED = synthetic.BENCH_SEED
TWO32 = 1 << 32
ASSETS = [1, 4, 5, 8, 9, 12, 13, 16]
STEPS = [1, 2, 7]
PATHS = [1, 257, 513]


@functools.lru_cache(maxsize=None)
def market(N):
    """(mu, L, w): a drift with N distinct non-zero entries, a dense lower-triangular factor with N (N + 1) / 2 distinct
    non-zero entries (a positive diagonal) and N distinct weights that sum to one; read-only."""
    i = np.arange(N, dtype=np.float64)
    mu = (3e-4 + 1.7e-4 * i) * np.where(i % 3 == 1, -1.0, 1.0)
    L = np.zeros((N, N))
    r, c = np.tril_indices(N)
    L[r, c] = 1e-3 * (1.0 + 0.37 * np.arange(r.size)) * np.where((r + c) % 4 == 3, -1.0, 1.0)
    L[np.arange(N), np.arange(N)] = 8e-3 + 1.1e-3 * i
    w = (1.0 + i) / (1.0 + i).sum()
    mu32, L32, W32 = prepare_inputs(mu, L @ L.T, w, chol=L)
    low = L32[np.tril_indices(N)]
    assert np.unique(low).size == low.size and np.all(low != 0.0) and np.all(np.triu(L32, 1) == 0.0)
    assert np.unique(mu32).size == N and np.all(mu32 != 0.0) and np.unique(W32).size == N
    for a in (mu, L, w, mu32, L32, W32):
        a.setflags(write=False)
    return mu, L, w, mu32, L32, W32


@functools.lru_cache(maxsize=None)
def oracle_terminal(N, T, P, path_begin, compounding):
    """The oracle's terminal values, computed once per configuration and shared (read-only)."""
    _, _, _, mu32, L32, W32 = market(N)
    ref = mc_oracle.simulate(mu32, L32, W32, T, P, SEED, path_begin=path_begin, compounding=compounding)[0]
    ref.setflags(write=False)
    return ref


def gpu(N, T, P, path_begin, compounding):
    mu, L, w, _, _, _ = market(N)
    return simulate_paths(mu, L @ L.T, w, n_steps=T, n_paths=P, seed=SEED, compounding=compounding, store=True,
                          path_begin=path_begin, chol=L)["terminal"]


def assert_bits(got, ref):
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("compounding", ["simple", "log"])
@pytest.mark.parametrize("N", ASSETS)
def test_every_path_equals_the_oracle(gpu_ctx, N, compounding):
    for T in STEPS:
        for P in PATHS:
            assert_bits(gpu(N, T, P, 5 * TWO32 + 7, compounding), oracle_terminal(N, T, P, 5 * TWO32 + 7, compounding))


@pytest.mark.parametrize("compounding", ["simple", "log"])
def test_a_range_across_two_to_the_32_falls_back(gpu_ctx, compounding):
    """[2^32 - 100, 2^32 + 157) has two high counter words: the launch runs mc_paths_kernel and equals the oracle."""
    assert_bits(gpu(16, 7, 257, TWO32 - 100, compounding), oracle_terminal(16, 7, 257, TWO32 - 100, compounding))

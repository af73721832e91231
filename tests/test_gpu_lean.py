"""The lean Gaussian kernel (mc_paths_lean_kernel: the plain walk of one portfolio for a launch whose paths share the high
Philox counter word) against the CPU oracle, bit for bit: float32 terminal values compared with == on their bit patterns,
no tolerance.  The launch is routed by mcp::lean_range (tests/test_lean_route_cpu.py): a path range inside one multiple of
2^32 runs the lean kernel, a range that crosses one stays on mc_paths_kernel, and both must give the oracle's values.

Rounds 1 and 2 of Philox differ per step, so T = 1 catches a hoisting error; n = 2*8192*256 + 1 runs the grid stride
(two full sweeps of the 8192-block grid and one more tile); the bases make p_hi 0, 1 and 5.
"""
import functools

import numpy as np
import pytest

from monte_carlo_portfolio_amd import simulate_paths, synthetic
from monte_carlo_portfolio_amd.simulate import prepare_inputs
from oracle import mc_oracle, ref_stats

pytestmark = pytest.mark.gpu

SEED = synthetic.BENCH_SEED
TWO32 = 1 << 32


@functools.lru_cache(maxsize=None)
def oracle_terminal(N, T, P, path_begin, compounding):
    """The oracle's terminal values, computed once per configuration and shared (read-only)."""
    mu, cov = synthetic.synthetic_market(N)
    mu32, L, W32 = prepare_inputs(mu, cov, synthetic.equal_weights(N))
    ref = mc_oracle.simulate(mu32, L, W32, T, P, SEED, path_begin=path_begin, compounding=compounding)[0]
    ref.setflags(write=False)
    return ref


def gpu(N, T, P, path_begin, compounding="simple"):
    mu, cov = synthetic.synthetic_market(N)
    return simulate_paths(mu, cov, synthetic.equal_weights(N), n_steps=T, n_paths=P, seed=SEED, compounding=compounding,
                          store=True, path_begin=path_begin)


def assert_bits(got, ref):
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("T", [1, 2, 3, 8])
def test_every_step_count(gpu_ctx, T):
    assert_bits(gpu(16, T, 257, 0)["terminal"], oracle_terminal(16, T, 257, 0, "simple"))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 2 * 8192 * 256 + 1])
def test_path_counts_and_the_grid_stride(gpu_ctx, P):
    got = gpu(16, 2, P, 0)
    ref = oracle_terminal(16, 2, P, 0, "simple")
    assert_bits(got["terminal"], ref)
    want = ref_stats.path_stats(ref)                      # the fused epilogue ran on the same registers
    assert got["n"] == want["n"] and got["n_tail"] == want["n_tail"] and got["var"] == want["var"]
    assert got["min"] == want["min"] and got["max"] == want["max"]


@pytest.mark.parametrize("base,P", [(0, 257), (TWO32 - 64, 64), (TWO32 - 64, 65), (TWO32, 257), (5 * TWO32 + 7, 257)])
@pytest.mark.parametrize("compounding", ["simple", "log"])
def test_path_bases_and_compounding(gpu_ctx, base, P, compounding):
    """p_hi = 0, 1 and 5; [2^32 - 64, 2^32) stays in the lean kernel, one path more crosses 2^32 and falls back."""
    assert_bits(gpu(16, 3, P, base, compounding)["terminal"], oracle_terminal(16, 3, P, base, compounding))


@pytest.mark.parametrize("compounding", ["simple", "log"])
def test_adjacent_ranges_concatenate(gpu_ctx, compounding):
    """Two lean launches on either side of 2^32 against one launch of the retained kernel across it, and the oracle."""
    left = gpu(16, 3, 64, TWO32 - 64, compounding)["terminal"]
    right = gpu(16, 3, 193, TWO32, compounding)["terminal"]
    whole = gpu(16, 3, 257, TWO32 - 64, compounding)["terminal"]
    assert_bits(np.concatenate([left, right]), whole)
    assert_bits(whole, oracle_terminal(16, 3, 257, TWO32 - 64, compounding))


def test_three_assets(gpu_ctx):
    """N = 3: one Philox block per step (NB = 1)."""
    assert_bits(gpu(3, 8, 257, 5 * TWO32 + 7)["terminal"], oracle_terminal(3, 8, 257, 5 * TWO32 + 7, "simple"))

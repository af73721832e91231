"""The raw records of the two row-sum launches, byte for byte (SPEC.md 5.22, 5.23).

Every addition in downside_kernel, relative_kernel and their merge has its operands and its order, and that order is the definition
of the result.  tests/golden/rowsum_parent.npz holds what the kernels wrote on an MI355X before they were folded onto one row walker,
one workgroup record and one merge (tests/golden/make_rowsum_parent_goldens.py); the inputs are tests/rowsum_cases.py's, from integer
arithmetic alone.  Simple compounding only: the log path goes through the device's expm1, whose last bit belongs to the ROCm version.

1. Byte equality with the fixture at the sizes where the walker, the record or the merge can go wrong:
     n = 1, 2, 5, 6                head and tail only, no body; the head clipped by n
     n = 1025                      two workgroups per row, the second on the body's last slot
     n = 66,000                    65 workgroups per row: one merge lane adds two records
     n = trip + 3, 3 trip          (trip = mcp_downside_trip_n()) the first double trip of the depth-2 body loop, taken by a few lanes
                                   only; a double trip and then the single-trip remainder
   Three rows for downside; six rows in groups of three with bench = 1 for relative, so that a row sits before and after its benchmark
   and is the benchmark.  Y against the fixture where it is kept and against fl32(1 + a) of NumPy at every size.
2. More rows than one gridDim.y holds (65,537; 65,538 in groups of two with bench = 1, so that row 65,534's benchmark lies in the
   second slice and row 65,535 is its own benchmark at the slice's first row), at n = 2, where every sum is a single rounding and
   tests/downside_ref.py / tests/relative_ref.py give the same bits: n of every record, and rows 0, 65,534, 65,535 and the last whole.
"""
import os

import numpy as np
import pytest

import downside_ref
import relative_ref
import rowsum_cases as cases
from monte_carlo_portfolio_amd import _ffi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowsum_parent.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _differing(got, want):
    return [(int(r), int(w)) for r, w in zip(*np.nonzero(got != want))][:8]


def test_the_fixture_holds_every_size(gpu_ctx, golden):
    lib = _ffi.lib()
    names = {f"{kind}_n{n}" for n in cases.sizes(lib) for kind in ("downside", "relative")}
    names |= {f"relative_y_n{n}" for n in cases.sizes(lib) if n <= cases.Y_KEPT_UP_TO}
    assert set(golden) == names
    assert lib.mcp_downside_grid(1025) == 2 and lib.mcp_downside_grid(66_000) == 65


def test_downside_records_are_the_parents_bytes(gpu_ctx, golden):
    lib = _ffi.lib()
    for n in cases.sizes(lib):
        vals, pivots = cases.rows(cases.DS_ROWS, n, 1000 + n)
        got, want = cases.run_downside(lib, vals, pivots), golden[f"downside_n{n}"]
        print(f"downside n={n}: (row, word) that differ {_differing(got, want)}")
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), f"n={n}"


def test_relative_records_and_y_are_the_parents_bytes(gpu_ctx, golden):
    lib = _ffi.lib()
    for n in cases.sizes(lib):
        vals, pivots = cases.rows(cases.RL_ROWS, n, 2000 + n)
        got, y = cases.run_relative(lib, vals, pivots, cases.RL_GROUP, cases.RL_BENCH)
        want = golden[f"relative_n{n}"]
        print(f"relative n={n}: (row, word) that differ {_differing(got, want)}")
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), f"n={n}"
        if n <= cases.Y_KEPT_UP_TO:
            assert y.tobytes() == golden[f"relative_y_n{n}"].tobytes(), f"Y n={n}"
        x = downside_ref.to_x(vals)
        rb = np.arange(cases.RL_ROWS) // cases.RL_GROUP * cases.RL_GROUP + cases.RL_BENCH
        assert y.tobytes() == (1.0 + (x - x[rb])).astype(np.float32).tobytes(), f"Y n={n} differs from fl32(1 + a)"


BIG_N = 2


def test_downside_rows_beyond_one_grid_slice(gpu_ctx):
    n_rows = 65_537
    vals, pivots = cases.rows(n_rows, BIG_N, 31, pivot_step=1e-7)
    got = cases.run_downside(_ffi.lib(), vals, pivots).reshape(-1).view(_ffi.DOWNSIDE_SUMS_DTYPE)
    assert np.array_equal(got["n"], np.full(n_rows, BIG_N, np.uint64))
    x = downside_ref.to_x(vals)
    for r in (0, 65_534, 65_535, n_rows - 1):
        want = downside_ref.raw_record(x[r], pivots[r], cases.TAU)
        assert got[r].tobytes() == want.tobytes(), (r, got[r], want)


def test_relative_rows_beyond_one_grid_slice(gpu_ctx):
    n_rows, group, bench = 65_538, 2, 1
    vals, pivots = cases.rows(n_rows, BIG_N, 37, pivot_step=1e-7)
    words, y = cases.run_relative(_ffi.lib(), vals, pivots, group, bench)
    got = words.reshape(-1).view(_ffi.RELATIVE_SUMS_DTYPE)
    assert np.array_equal(got["n"], np.full(n_rows, BIG_N, np.uint64))
    x = downside_ref.to_x(vals)
    rb = np.arange(n_rows) // group * group + bench
    assert y.tobytes() == (1.0 + (x - x[rb])).astype(np.float32).tobytes()
    for r in (0, 65_534, 65_535, n_rows - 1):
        want = relative_ref.raw_record(x[r], x[rb[r]], pivots[r], pivots[rb[r]])
        assert got[r].tobytes() == want.tobytes(), (r, got[r], want)

"""The inputs of test_gpu_stats_matrix.py and test_gpu_hist0.py, checked on the oracle and NumPy alone (tests/stats_cases.py): the
GPU tests compare kernels with these expected values, and they would pass vacuously on constant rows, on a reference that is itself
inexact at sigma << |mean|, without ties at the quantile, or with every value on one side of hist_kernel<0>'s window."""
import numpy as np
import pytest

import stats_cases as sc


def test_the_table_holds_one_shape_per_launch_kind():
    assert [(s.N, s.K) for s in sc.SHAPES] == [(16, 1), (16, 1), (16, 9), (5, 16), (16, 17), (16, 65), (16, 129), (16, 300), (16, 513),
                                               (20, 17), (20, 129)]
    lean, wrap = sc.SHAPES[:2]
    assert lean.path_begin == 0 and wrap.path_begin < sc.TWO32 < wrap.path_begin + sc.N_PATHS      # mcp::lean_range is false across 2^32
    assert 0.25 in sc.V0S and all(v0 != 1.0 for v0 in sc.V0S)
    assert [np.log2(v0) == np.round(np.log2(v0)) for v0 in sc.V0S] == [True, False, False, False]
    assert float(np.float32(0.1)) != 0.1 and sc.N_PATHS == 5 * 64 + 13
    for s in sc.SHAPES:
        cases = sc.cases_of(s)
        assert {(c.v0, c.scale) for c in cases if c.compounding == "simple" and c.n_paths == sc.N_PATHS and c.alpha == sc.ALPHA} == \
            {(v0, scale) for v0 in sc.V0S for scale in sc.SCALES}
        assert {c.scale for c in cases if c.alpha == sc.SECOND_ALPHA} == set(sc.SCALES)
        assert {c.scale for c in cases if c.compounding == "log"} == (set(sc.SCALES) if s.id in sc.LOG_SHAPES else set())
        assert {c.n_paths for c in cases} == ({sc.N_PATHS, 1, 63, 65} if s.id in sc.RAGGED_SHAPES else {sc.N_PATHS})
    assert len(sc.ALL_CASES) == len(set(sc.ALL_CASES)) == 192


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: s.id)
def test_rows_are_not_constant_and_the_reference_is_exact(shape):
    """Every portfolio of every call has at least 32 distinct terminal values (measured: at least 88 at n = 333 and 44 at n = 63,
    at scale 1e-4), so std is no rounding artefact; np.std(ddof=1) and the longdouble two-pass std agree to 1e-12 (measured:
    4.4e-16), so the tolerance of the GPU test absorbs no error of the reference; at scale 1e-4 sigma/|mean| lies between 4e-4 and
    1.5e-3 (measured: 4.2e-4 .. 1.4e-3)."""
    for c in sc.cases_of(shape):
        t = sc.terminal(c.shape, c.v0, c.scale, c.n_paths, c.compounding)
        e = sc.expected(c)
        assert t.shape == (shape.K, c.n_paths) and np.all(e["n"] == c.n_paths)
        if c.n_paths == 1:
            assert np.all(e["std"] == 0.0) and np.all(e["std_ld"] == 0.0) and np.all(e["sharpe_ld"] == 0.0)
            continue
        assert min(np.unique(t[k]).size for k in range(shape.K)) >= 32, c.tag
        np.testing.assert_allclose(e["std"], e["std_ld"], rtol=1e-12, err_msg=c.tag)
        np.testing.assert_allclose(e["mean"], e["mean_ld"], rtol=1e-12, err_msg=c.tag)
        if c.scale == 1e-4:
            ratio = e["std_ld"] / np.abs(e["mean_ld"])
            assert 4e-4 <= ratio.min() and ratio.max() <= 1.5e-3, (c.tag, ratio.min(), ratio.max())


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: s.id)
def test_low_volatility_cases_have_ties_at_the_quantile(shape):
    """n_tail > lo + 1 on at least one portfolio of a low-volatility call of every shape: the tail then holds values equal to the
    low order statistic beyond its rank, and the tie rule of the tail (every x <= var) is exercised."""
    tied = 0
    for c in sc.cases_of(shape):
        if c.scale < 1.0 and c.n_paths > 1:
            tied += int((sc.expected(c)["n_tail"] > sc.rank_lo(c.n_paths, c.alpha) + 1).sum())
    assert tied >= 1


def test_keys_and_digits():
    v = np.array([0.0, 1.0, -1.0, np.inf, -np.inf, 3.0, 1e-30, -1e-30, np.nan], np.float32)
    key = sc.float_to_key(v)
    assert np.array_equal(sc.key_to_float(key).view(np.uint32), v.view(np.uint32))
    finite = np.sort(v[:-1])
    assert np.all(np.diff(sc.float_to_key(finite).astype(np.int64)) > 0)                       # order preserving
    assert list(sc.digit0(np.array([0.0, 1.0, 3.0, np.inf, -np.inf, np.nan], np.float32))) == [1024, 1532, 1538, 2044, 3, 2046]
    assert sc.hist0_expected(v[None, :])[0, 0].sum() == v.size and sc.hist0_expected(v[None, :])[0, 1].sum() == 0


# (values, compounding, pivot) pairs that must put at least 10 % of the values inside the 16-bin window and at least 10 % outside: both
# branches of hist_kernel<0> run in one launch.  The others are all inside or (nearly) all outside, which is asserted too.
MIXED = ({("wide", "simple", p) for p in ("null", "zero", "first")} | {("normal", "log", "first")}
         | {("inf", "simple", p) for p in ("null", "zero", "first")} | {("edges", "simple", p) for p in sc.HIST_PIVOTS})
ALL_INSIDE = {("clustered", "simple", "null"), ("clustered", "simple", "zero"), ("clustered", "simple", "first"), ("clustered", "log", "first"),
              ("equal", "simple", "null"), ("equal", "simple", "zero"), ("equal", "simple", "first")}


@pytest.mark.parametrize("n", [1023, 4099])
def test_histogram_inputs_hit_and_miss_the_window(n):
    seen = set()
    for kind, comp, pk, values, pivot, dlo in sc.hist0_cases(n):
        assert values.shape == (sc.HIST_K, n) and values.dtype == np.float32 and dlo.shape == (sc.HIST_K,)
        assert np.all(dlo >= 0) and np.all(dlo <= sc.BINS - sc.WIN)
        f = sc.window_fraction(values, dlo)
        name = (kind, comp, pk)
        seen.add(name)
        if name in MIXED:
            assert 0.1 <= f <= 0.9, (name, f)
        elif name in ALL_INSIDE:
            assert f == 1.0, (name, f)
        else:
            assert f < 0.11, (name, f)
        assert not np.any(sc.digit0(values) == 0)                    # digit 0 is never asked for
    assert MIXED <= seen and ALL_INSIDE <= seen and len(seen) == 7 * len(sc.HIST_PIVOTS)


def test_both_clamps_of_the_window_are_reached():
    """Simple compounding: v0 (1 + 3e38) rounds to +inf, digit 2044, and 2044 - 8 > 2048 - 16 clamps to 2032; v0 (1 - 3e38) rounds
    to -inf, digit 3 < 8, and the subtraction clamps to 0.  A NaN pivot gives a NaN centre, digit 2046: the upper clamp again.  (In
    log compounding log1p keeps the centre finite and neither clamp is reached.)"""
    K = sc.HIST_K
    unclamped = sc.digit0(np.array([np.inf, -np.inf, np.nan], np.float32)) - sc.WIN // 2
    assert list(unclamped) == [2036, -5, 2038]
    assert np.all(sc.hist0_dlo(np.full(K, 3e38), K, sc.HIST_V0, "simple") == sc.BINS - sc.WIN)
    assert np.all(sc.hist0_dlo(np.full(K, -3e38), K, sc.HIST_V0, "simple") == 0)
    assert np.all(sc.hist0_dlo(np.full(K, np.nan), K, sc.HIST_V0, "simple") == sc.BINS - sc.WIN)
    assert np.all(sc.hist0_dlo(None, K, sc.HIST_V0, "simple") == sc.digit0(np.float32(3.0)) - 8)
    assert np.all(sc.hist0_dlo(np.full(K, -1.0), K, sc.HIST_V0, "simple") == 1024 - 8)          # vc = 0
    assert np.all(sc.hist0_dlo(np.full(K, -3e38), K, sc.HIST_V0, "log") == 1024 - 8)            # c <= -1: log1p(0)
    assert np.all(sc.hist0_dlo(np.full(K, np.nan), K, sc.HIST_V0, "log") == 1024 - 8)
    # the pivot of a row whose first value is infinite is infinite: per-row windows at both clamps in one launch
    v = sc.hist0_values("inf", 1023)
    dlo = sc.hist0_dlo(sc.hist0_pivot("first", v, sc.HIST_V0, "simple"), K, sc.HIST_V0, "simple")
    assert (dlo == 0).any() and (dlo == sc.BINS - sc.WIN).any() and ((dlo > 0) & (dlo < sc.BINS - sc.WIN)).any()


@pytest.mark.parametrize("n", [7, 1023])
def test_edge_values_sit_on_the_window_edges(n):
    """The "edges" rows hold exactly the digits dlo - 1, dlo, dlo + 15, dlo + 16 of their own window, plus 2047 when the window does
    not reach it; at a clamp the digits that do not exist (below 1, above 2047) are left out."""
    assert sc.edge_digits(1530) == [1529, 1530, 1545, 1546, 2047]
    assert sc.edge_digits(0) == [15, 16, 2047] and sc.edge_digits(2032) == [2031, 2032, 2047]
    for kind, comp, pk, values, pivot, dlo in sc.hist0_cases(n):
        if kind != "edges":
            continue
        d = sc.digit0(values)
        for k in range(sc.HIST_K):
            want = sc.edge_digits(int(dlo[k]))
            assert set(d[k]) == set(want), (pk, k)
            counts = np.bincount(d[k], minlength=sc.BINS)[want]
            assert counts.max() - counts.min() <= 1                  # the digits in turn


def test_padding_is_a_nan_that_sorts_below_every_value():
    """The padding behind a row is NaN with the sign bit set: digit 0, which no value of any case has, and the smallest keys there
    are -- so a kernel that reads it shows it in bin 0 (pass 0) or in the sum below the quantile's bucket (passes 1 and 2)."""
    v = sc.hist0_values("edges", 7, dlo=np.zeros(sc.HIST_K, np.int64))             # the rows with the smallest digits of all cases
    p = sc.padded(v, 3)
    assert p.shape == (sc.HIST_K, 10) and np.array_equal(p[:, :7].view(np.uint32), v.view(np.uint32))
    assert np.isnan(p[:, 7:]).all() and np.all(sc.digit0(p[:, 7:]) == 0)
    assert sc.float_to_key(p[:, 7:]).max() < sc.float_to_key(np.float32(-np.inf)) <= sc.float_to_key(v).min()
    assert sc.padded(v, 0).shape == v.shape

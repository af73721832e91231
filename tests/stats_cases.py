"""The case table of the K-portfolio statistics tests and its NumPy side (not a test module).

Two families of cases, each with the expected values computed here from NumPy alone:

  * MATRIX: calls of simulate_paths, one group per launch kind of the path kernels (lean, generic one-portfolio, passes of 8, the
    MFMA sweeps per wave and with shared draws), at v0 != 1, at three volatility scales, on ragged path tiles and in both
    compounding modes.  The expected record of a call is built on the oracle's terminal values, which are bit-identical to the
    kernels': counts, order statistics and tail from oracle.ref_stats.path_stats, mean and std from a two-pass evaluation in
    np.longdouble on x.
  * HIST0: rows of caller-supplied values, pivots and sizes for hist_kernel<0> and pass0_kernel through the device-level ABI, with
    the NumPy restatement of float_to_key, of the digit-0 histogram and of the kernel's window [dlo, dlo + 16).

tests/test_stats_cases_cpu.py asserts on this module alone that the cases cover what they claim to (so the GPU tests cannot pass
vacuously); tests/test_gpu_stats_matrix.py and tests/test_gpu_hist0.py run them on the kernels.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from monte_carlo_portfolio_amd import synthetic
from monte_carlo_portfolio_amd.simulate import prepare_inputs
from oracle import mc_oracle, ref_stats

SEED = synthetic.BENCH_SEED
T = 25
N_PATHS = 333                        # five 64-path wave tiles plus 13
RF = 0.01
ALPHA = 0.95
SECOND_ALPHA = 0.5                   # on SECOND_V0 only
SECOND_V0 = 3.0
TWO32 = 1 << 32

V0S = (0.25, 3.0, 10000.0, 0.1)      # 0.25: a power of two, inv_v0d exact; the others divide, and 0.1 is not representable
SCALES = (1.0, 1e-2, 1e-4)           # the covariance of synthetic_market(N) times scale^2


class Shape(NamedTuple):
    id: str
    N: int
    K: int
    path_begin: int
    launch: str                      # the launch kind this shape is in the table for (sweep_plan / the ladder)


SHAPES = (
    Shape("n16_k1_lean", 16, 1, 0, "lean kernel: every path id has the same high word"),
    Shape("n16_k1_across_2p32", 16, 1, TWO32 - 100, "mc_paths_kernel: the path range crosses 2^32"),
    Shape("n16_k9", 16, 9, 0, "passes of 8, the second with one live portfolio"),
    Shape("n5_k16", 5, 16, 0, "passes of 8, both full"),
    Shape("n16_k17", 16, 17, 0, "per-wave sweep, 1 tile"),
    Shape("n16_k65", 16, 65, 0, "per-wave sweep, 4 tiles"),
    Shape("n16_k129", 16, 129, 0, "shared draws MT 2"),
    Shape("n16_k300", 16, 300, 0, "shared draws MT 2 plus per-wave"),
    Shape("n16_k513", 16, 513, 0, "shared draws MT 4 plus a remainder of one portfolio"),
    Shape("n20_k17", 20, 17, 0, "N > 16: shared draws MT 1"),
    Shape("n20_k129", 20, 129, 0, "N > 16: shared draws MT 2"),
)
SHAPE_BY_ID = {s.id: s for s in SHAPES}
RAGGED_SHAPES = ("n16_k65", "n16_k300", "n20_k129")
RAGGED_PATHS = (1, 63, 65)           # one lane of a tile, one path short of a tile, one path into the second half-tile
RAGGED_SCALES = (1.0, 1e-4)
LOG_SHAPES = ("n16_k300", "n20_k129", "n16_k9")
LOG_V0 = 3.0


class Case(NamedTuple):
    shape: Shape
    v0: float
    scale: float
    n_paths: int
    compounding: str
    alpha: float

    @property
    def tag(self):
        return f"{self.shape.id} v0={self.v0} scale={self.scale} n={self.n_paths} {self.compounding} alpha={self.alpha}"


def cases_of(shape: Shape) -> list[Case]:
    """Every call of the matrix for one shape: simple compounding at every (v0, scale); the second alpha at SECOND_V0; the ragged
    path counts and log compounding on the shapes listed above."""
    out = [Case(shape, v0, sc, N_PATHS, "simple", ALPHA) for v0 in V0S for sc in SCALES]
    out += [Case(shape, SECOND_V0, sc, N_PATHS, "simple", SECOND_ALPHA) for sc in SCALES]
    if shape.id in RAGGED_SHAPES:
        out += [Case(shape, SECOND_V0, sc, n, "simple", ALPHA) for n in RAGGED_PATHS for sc in RAGGED_SCALES]
    if shape.id in LOG_SHAPES:
        out += [Case(shape, LOG_V0, sc, N_PATHS, "log", ALPHA) for sc in SCALES]
    return out


ALL_CASES = [c for s in SHAPES for c in cases_of(s)]


def market(shape: Shape, scale: float):
    """(mu, cov, W [K, N]) of a case, in float64 as simulate_paths takes them."""
    mu, cov = synthetic.synthetic_market(shape.N)
    return mu, cov * scale * scale, synthetic.dirichlet_weights(shape.N, shape.K)


@functools.lru_cache(maxsize=None)
def terminal(shape: Shape, v0: float, scale: float, n_paths: int, compounding: str) -> np.ndarray:
    """The oracle's terminal values [K, n_paths] float32 (read-only: shared among the tests)."""
    mu, cov, W = market(shape, scale)
    mu32, L, W32 = prepare_inputs(mu, cov, W)
    t = mc_oracle.simulate(mu32, L, W32, T, n_paths, SEED, path_begin=shape.path_begin, v0=v0, compounding=compounding)
    t.setflags(write=False)
    return t


def two_pass_longdouble(x: np.ndarray):
    """(mean, std ddof=1) of every row of x [K, n] by the two-pass formula in np.longdouble, rounded to float64 at the end."""
    xl = np.asarray(x, np.float64).astype(np.longdouble)
    n = xl.shape[1]
    mean = xl.sum(axis=1) / n
    if n < 2:
        return mean.astype(np.float64), np.zeros(xl.shape[0])
    m2 = ((xl - mean[:, None]) ** 2).sum(axis=1)
    return mean.astype(np.float64), np.sqrt(m2 / (n - 1)).astype(np.float64)


PATH_STATS_KEYS = ("n", "n_tail", "var", "min", "max", "cvar", "sum_tail", "mean", "std", "sharpe")


@functools.lru_cache(maxsize=None)
def expected(case: Case) -> dict:
    """Arrays [K] of the expected record of a call.  Keys of PATH_STATS_KEYS: oracle.ref_stats.path_stats row by row.  mean_ld,
    std_ld, sharpe_ld: the two-pass longdouble values and (mean_ld - rf) / std_ld (0 where std_ld is 0, as the kernels define it)."""
    t = terminal(case.shape, case.v0, case.scale, case.n_paths, case.compounding)
    rows = [ref_stats.path_stats(t[k], case.v0, case.compounding, case.alpha, RF) for k in range(t.shape[0])]
    out = {key: np.array([r[key] for r in rows]) for key in PATH_STATS_KEYS}
    x = ref_stats.terminal_to_x(t, case.v0, case.compounding)
    mean, std = two_pass_longdouble(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        sharpe = np.where(std > 0, (mean - RF) / std, 0.0)
    out.update(mean_ld=mean, std_ld=std, sharpe_ld=sharpe)
    return out


def rank_lo(n: int, alpha: float) -> int:
    """The rank of the low order statistic of np.percentile(x, (1 - alpha) * 100), method 'linear'."""
    return int(np.floor((n - 1) * ((1 - alpha) * 100 / 100.0)))


# ---------------------------------------------------------------- hist_kernel<0>: keys, digits, the window
BINS = 2048
WIN = 16
HIST_K = 19
HIST_V0 = 3.0
HIST_SIZES = (1, 5, 6, 7, 1023, 4099, 70_001)        # 1..7: head and tail only; 70,001: more than one block per row
HIST_PADS = (0, 1, 2, 3)                             # stride = n + s: rows start at all four offsets modulo 16 bytes
# value kind -> the compounding modes it runs in
HIST_VALUES = {"clustered": ("simple", "log"), "wide": ("simple",), "normal": ("log",), "equal": ("simple",), "inf": ("simple",),
               "edges": ("simple",)}
HIST_PIVOTS = ("null", "zero", "first", "minus_one", "plus_3e38", "minus_3e38", "nan")


def float_to_key(v) -> np.ndarray:
    """The order-preserving key of binary32 values: bits ^ (0xFFFFFFFF if sign else 0x80000000) (csrc/mcp_device.h)."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(key) -> np.ndarray:
    k = np.ascontiguousarray(key, np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)).view(np.float32)


def digit0(v) -> np.ndarray:
    return (float_to_key(v) >> 21).astype(np.int64)


def hist0_expected(values: np.ndarray) -> np.ndarray:
    """[K, 2, 2048] uint64: np.bincount of the digit-0 of every row in [k][0], zeros in [k][1]."""
    v = np.atleast_2d(values)
    out = np.zeros((v.shape[0], 2, BINS), np.uint64)
    for k in range(v.shape[0]):
        out[k, 0] = np.bincount(digit0(v[k]), minlength=BINS)
    return out


def hist0_dlo(pivot, K: int, v0: float, compounding: str) -> np.ndarray:
    """[K] the first bin of hist_kernel<0>'s window, computed as the kernel does: the digit of (float)(v0 (1 + c)) -- log:
    (float)log1p(c), c = 0 unless c > -1 -- minus 8, clamped to [0, 2048 - 16].  pivot None: the NULL pointer, c = 0."""
    c = np.zeros(K) if pivot is None else np.asarray(pivot, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if compounding == "log":
            vc = np.log1p(np.where(c > -1.0, c, 0.0)).astype(np.float32)
        else:
            vc = (np.float64(np.float32(v0)) * (1.0 + c)).astype(np.float32)
    dc = digit0(vc)
    dlo = np.where(dc >= WIN // 2, dc - WIN // 2, 0)
    return np.minimum(dlo, BINS - WIN)


def hist0_pivot(kind: str, values: np.ndarray, v0: float, compounding: str):
    """[K] float64 pivots of one kind, or None for the NULL pointer."""
    K = values.shape[0]
    if kind == "null":
        return None
    if kind == "first":
        with np.errstate(over="ignore", invalid="ignore"):
            return ref_stats.terminal_to_x(values[:, 0], v0, compounding).astype(np.float64)
    const = {"zero": 0.0, "minus_one": -1.0, "plus_3e38": 3e38, "minus_3e38": -3e38, "nan": np.nan}[kind]
    return np.full(K, const)


def edge_digits(dlo: int) -> list[int]:
    """The digits around a window [dlo, dlo + 16): one below, the first, the last, one above, and 2047 when the window does not
    reach it.  Digit 0 (a NaN pattern of the sign bit set) and digits past 2047 do not exist as values and are left out."""
    want = [dlo - 1, dlo, dlo + WIN - 1, dlo + WIN] + ([BINS - 1] if dlo + WIN - 1 < BINS - 1 else [])
    return [d for d in want if 1 <= d <= BINS - 1]


def hist0_values(kind: str, n: int, K: int = HIST_K, dlo=None) -> np.ndarray:
    """[K, n] float32 rows of one kind.  "edges" is built from keys around the windows `dlo` [K] of the pivot it runs with: the
    digits of edge_digits in turn, random low 21 bits."""
    rng = np.random.default_rng([n, sorted(HIST_VALUES).index(kind)])
    if kind == "clustered":
        return (1.0 + 0.05 * rng.standard_normal((K, n))).astype(np.float32)
    if kind == "wide":                                   # dozens of digits
        return np.exp(rng.normal(0.0, 4.0, (K, n))).astype(np.float32)
    if kind == "normal":                                 # both signs
        return rng.standard_normal((K, n)).astype(np.float32)
    if kind == "equal":
        return np.repeat((1.0 + 0.1 * np.arange(K, dtype=np.float32))[:, None], n, axis=1)
    if kind == "inf":
        v = (1.0 + 0.05 * rng.standard_normal((K, n))).astype(np.float32)
        where = rng.random((K, n))
        v[where < 0.1] = np.inf
        v[where > 0.9] = -np.inf
        return v
    if kind == "edges":
        out = np.empty((K, n), np.uint32)
        for k in range(K):
            d = np.array(edge_digits(int(dlo[k])), np.uint32)
            out[k] = (d[(np.arange(n) + k) % d.size] << np.uint32(21)) | rng.integers(0, 1 << 21, n, dtype=np.uint32)
        return key_to_float(out)
    raise KeyError(kind)


PAD_BITS = 0xFFFFFFFF            # a NaN with the sign bit set: key 0, digit 0, below every value in key order


def padded(values: np.ndarray, pad: int) -> np.ndarray:
    """[K, n + pad] float32: the rows with `pad` NaN elements behind each (what a kernel must leave unread).  The NaN carries the sign
    bit, so its key sorts BELOW every value: a kernel that reads it counts it in bin 0 of the digit-0 histogram, and in the later
    passes adds it to the sum below the quantile's bucket, which turns CVaR into NaN.  (A NaN without the sign bit has digit 2046,
    above every value: hist_kernel<1|2> would drop it unseen.)"""
    K, n = values.shape
    out = np.full((K, n + pad), PAD_BITS, np.uint32).view(np.float32)
    out[:, :n] = values
    return out


def hist0_cases(n: int):
    """Every (values kind, compounding, pivot kind, values [K, n], pivot [K] or None, dlo [K]) at size n.  The rows of a kind are the
    same for every pivot, except "edges", which follow the pivot's windows (built on the clustered rows' pivots)."""
    for kind, modes in HIST_VALUES.items():
        for comp in modes:
            base = hist0_values("clustered" if kind == "edges" else kind, n)
            for pk in HIST_PIVOTS:
                pivot = hist0_pivot(pk, base, HIST_V0, comp)
                dlo = hist0_dlo(pivot, HIST_K, HIST_V0, comp)
                values = hist0_values(kind, n, dlo=dlo) if kind == "edges" else base
                yield kind, comp, pk, values, pivot, dlo


def window_fraction(values: np.ndarray, dlo: np.ndarray) -> float:
    """The fraction of all values whose digit-0 lies inside its row's window."""
    d = digit0(values).reshape(values.shape)
    t = d - np.asarray(dlo)[:, None]
    return float(((t >= 0) & (t < WIN)).mean())

"""The case table of the enqueue-only path launches and its layout helpers (test helper, not a test module).

include/mcport.h hands a host that owns its buffers three launches -- mcp_launch_paths, mcp_launch_paths_drawdown and
mcp_launch_paths_horizons -- whose output arrays lie `stride` elements apart, a stride per array that the caller chooses.  The
mcp_simulate* calls, which every other GPU test goes through, pass one value for every stride: the path count.  A store site that
took n_paths for a stride, one array's stride for another's, kt for n_portfolios in the horizon row index, that dropped k_begin or
let a dead lane store would pass all of them.  The cases here are launches in which those quantities differ:

    n_paths = 321                   one workgroup, one wave and one lane: six 64-path tiles against two workgroups
    terminal_stride = n + 3, mdd_stride = n + 5, horizon_stride = n + 2      pairwise different, rows at every offset modulo 16 bytes
    T = 9, horizons (2, 5, 9)       the last horizon row is the terminal row
    SEED64 and, where they fit, the markets of tests/offdefault_cases.py (N = 5); tests/native_ref.py's market elsewhere

Every output array of a launch is allocated at rows x (the largest stride of the call) + TAIL elements and filled with FILL_BITS, a
quiet NaN that no walk produces, so that a kernel that takes a wrong stride still writes inside the allocation: the mistake shows
as damaged padding or a wrong live value (violations), never as a fault.  tests/test_launch_cases_cpu.py shows on NumPy alone that
violations rejects each of those mistakes in every case that can show it; tests/test_gpu_launch_cases.py runs the cases.

What the layout cannot show: a dead PORTFOLIO row that stores.  The sweep kernels' workgroups cover 128 or more portfolios and guard
the store with k < n_portfolios (csrc/mcp_sweep_paths.hip); a store of a row k >= K would land more than 64 elements behind the
last row, outside the allocation.  "A dead lane stores" below is about the dead path lanes of the last 64-path wave only.

kernel_of restates, for the three launch-level requests only, which kernel launch_paths_impl picks: route_kernel (csrc/mcp_host.cpp)
and sweep_plan (csrc/mcp_api.cpp).  It is how a case says which kernel it is in the table for, as stats_cases.Shape.launch does.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import drawdown_ref
import horizons_ref
import native_ref
import offdefault_cases as oc
import stats_cases as sc
from monte_carlo_portfolio_amd import _ffi
from oracle import mc_oracle

SEED = oc.SEED64
T = 9
HORIZONS = (2, 5, 9)
N_PATHS = 321                                # 256 + 64 + 1
V0, ALPHA, RF = oc.V0, oc.ALPHA, oc.RF
LEVELS = oc.LEVELS                           # the band levels of the host-level horizons call; BAND is the one the recipe reruns
BAND = 0
PAD_TERMINAL, PAD_MDD, PAD_HZ = 3, 5, 2
FAR = 1000                                   # the one case with terminal_stride = n + 1000
TAIL = 64                                    # elements behind the last row of every allocation
FILL_BITS = 0x7FD5A5A5                       # a quiet NaN with a payload: no kernel stores it
PATH_BLOCK, WAVE, KT8, SWEEP_MIN_K, LEAN_MAX_NB = 256, 64, 8, 17, 4
assert N_PATHS == PATH_BLOCK + WAVE + 1 and HORIZONS[-1] == T
assert len({N_PATHS + PAD_TERMINAL, N_PATHS + PAD_MDD, N_PATHS + PAD_HZ, N_PATHS}) == 4
assert {(N_PATHS + p) % 4 for p in (0, PAD_TERMINAL, PAD_MDD, PAD_HZ)} == {0, 1, 2, 3}      # rows start at every offset modulo 16 bytes

ENTRIES = {"paths": "mcp_launch_paths", "drawdown": "mcp_launch_paths_drawdown", "horizons": "mcp_launch_paths_horizons"}


class Case(NamedTuple):
    id: str
    entry: str               # a key of ENTRIES
    N: int
    K: int
    T: int
    comp: str
    native: bool             # MCP_FLAG_NATIVE_MATH
    fold: bool               # MCP_FLAG_FOLD
    path_begin: int
    n: int
    horizons: tuple          # () unless entry == "horizons"
    terminal_stride: int
    mdd_stride: int          # 0 unless entry == "drawdown"
    hz_stride: int           # 0 unless entry == "horizons"
    kernel: str              # the kernel(s) this launch runs: kernel_name(kernel_of(...))
    equal_strides: bool      # every stride equals n: what the mcp_simulate* calls do, exempt from the stride mistakes

    @property
    def flags(self):
        return (_ffi.MCP_FLAG_NATIVE_MATH if self.native else 0) | (_ffi.MCP_FLAG_FOLD if self.fold else 0)

    @property
    def exact(self):
        """Whether the launch has a bit-for-bit restatement (the native normals and the folded step have none)."""
        return not (self.native or self.fold)

    @property
    def strides(self):
        """{array: stride} of the arrays the launch stores."""
        out = {"terminal": self.terminal_stride}
        if self.entry == "drawdown":
            out["mdd"] = self.mdd_stride
        if self.entry == "horizons":
            out["horizon"] = self.hz_stride
        return out

    @property
    def rows(self):
        """{array: rows} of the same arrays."""
        out = {"terminal": self.K}
        if self.entry == "drawdown":
            out["mdd"] = self.K
        if self.entry == "horizons":
            out["horizon"] = len(self.horizons) * self.K
        return out


# ---- which kernel a launch runs -----------------------------------------------------------------------------------------------------

def lean_range(path_begin: int, n: int) -> bool:
    """mcp::lean_range (csrc/mcp_route.h): every path id of the launch has the same high word."""
    return n >= 1 and path_begin >> 32 == (path_begin + n - 1) >> 32


def sweep_plan(K: int, nb: int):
    """sweep_plan (csrc/mcp_api.cpp) with MCP_SWEEP_MT unset: [(shared, mt, k_begin, k_count)]."""
    out = []
    big = 4 if nb <= 4 else 2
    full = K // (128 * big) * (128 * big)
    if full:
        out.append((True, big, 0, full))
    r = K - full
    if r == 0:
        return out

    def per_wave(k):
        return 4 if k > 64 else 2 if k > 32 else 1
    if nb <= 4:
        if r <= 128:
            out.append((False, per_wave(r), full, r))
        elif r <= 256:
            out.append((True, 2, full, r))
        elif r <= 384:
            out += [(True, 2, full, 256), (False, per_wave(r - 256), full + 256, r - 256)]
        else:
            out.append((True, 4, full, r))
    else:
        out.append((True, 1 if r <= 128 else 2, full, r))
    return out


def kernel_of(entry, N, K, comp, native, fold, path_begin, n):
    """The kernels of one launch, as a tuple of selectors.  A one-lane-per-path launch is one selector (family, flags, KT) with
    flags a frozenset of LOGC, NATIVE, FOLD, UHI; a plain walk of K >= 17 portfolios is one ("SWEEP", shared, native, logc, MT) per
    segment of sweep_plan."""
    nb = (N + 3) // 4
    logc = comp == "log"
    if entry == "paths" and K >= SWEEP_MIN_K:
        return tuple(("SWEEP", shared, native, logc, mt) for shared, mt, _, _ in sweep_plan(K, nb))
    flags = set()
    if logc:
        flags.add("LOGC")
    if native:
        flags.add("NATIVE")
    if fold:
        flags.add("FOLD")
    family = {"paths": "FAM_PLAIN", "drawdown": "FAM_DD", "horizons": "FAM_HZ"}[entry]
    if family == "FAM_PLAIN" and K == 1 and not (native or fold) and nb <= LEAN_MAX_NB and lean_range(path_begin, n):
        flags.add("UHI")
    return ((family, frozenset(flags), 1 if K == 1 else KT8),)


def kernel_name(selectors) -> str:
    def one(s):
        if s[0] == "SWEEP":
            return f"{'mc_sweep_shared_kernel' if s[1] else 'mc_sweep_kernel'} MT={s[4]}{' native' if s[2] else ''}{' log' if s[3] else ''}"
        fam, flags, kt = s
        name = {"FAM_PLAIN": "mc_paths_lean_kernel" if "UHI" in flags else "mc_paths_kernel", "FAM_DD": "mc_paths_dd_kernel",
                "FAM_HZ": "mc_paths_hz_kernel"}[fam]
        return f"{name} {'|'.join(sorted(flags)) or '0'} KT={kt}"
    return " + ".join(one(s) for s in selectors)


def passes_of(c: Case):
    """[(k_begin, k_count)] of the kernel launches of a case: the passes of 8 portfolios of the one-lane-per-path kernels
    (csrc/mcp_paths_inst.hip), or the segments of sweep_plan."""
    if c.entry == "paths" and c.K >= SWEEP_MIN_K:
        return [(b, cnt) for _, _, b, cnt in sweep_plan(c.K, (c.N + 3) // 4)]
    if c.K == 1:
        return [(0, 1)]
    return [(b, min(KT8, c.K - b)) for b in range(0, c.K, KT8)]


# ---- the table ------------------------------------------------------------------------------------------------------------------------

def _case(id_, entry, N, K, comp="simple", begin=0, n=N_PATHS, native=False, fold=False, equal=False, far=False):
    pads = (0, 0, 0) if equal else (FAR if far else PAD_TERMINAL, PAD_MDD, PAD_HZ)
    return Case(id_, entry, N, K, T, comp, native, fold, begin, n, HORIZONS if entry == "horizons" else (), n + pads[0],
                n + pads[1] if entry == "drawdown" else 0, n + pads[2] if entry == "horizons" else 0,
                kernel_name(kernel_of(entry, N, K, comp, native, fold, begin, n)), equal)


# (N, K, path_begin) of the drawdown and horizon launches: KT = 1 (once across 2^32), KT = 8 in one, two and three passes
# (k_begin > 0), and K >= 17, where the partials take one slot per 64-path tile and launch_paths_impl pads them first
WALK_SHAPES = ((5, 1, 0), (16, 1, sc.TWO32 - 100), (5, 3, 0), (16, 9, 0), (20, 20, 0), (5, 17, 0))
PLAIN_LOG_SHAPES = ("n16_k1_lean", "n16_k1_across_2p32") + sc.LOG_SHAPES
NATIVE_SHAPES = (("n16_k1_lean", ("simple", "log")), ("n16_k9", ("simple", "log")), ("n16_k300", ("simple",)))


def _build():
    cases = []
    for s in sc.SHAPES:
        cases.append(_case(f"paths-{s.id}-simple", "paths", s.N, s.K, "simple", s.path_begin))
    for sid in PLAIN_LOG_SHAPES:
        s = sc.SHAPE_BY_ID[sid]
        cases.append(_case(f"paths-{s.id}-log", "paths", s.N, s.K, "log", s.path_begin))
    for sid, comps in NATIVE_SHAPES:
        s = sc.SHAPE_BY_ID[sid]
        cases += [_case(f"paths-{s.id}-native-{comp}", "paths", s.N, s.K, comp, s.path_begin, native=True) for comp in comps]
    cases += [_case(f"paths-n16_k1-fold-{comp}", "paths", 16, 1, comp, fold=True) for comp in ("simple", "log")]
    cases.append(_case("paths-n16_k1_lean-n1", "paths", 16, 1, n=1))
    cases.append(_case("paths-n16_k17-n65", "paths", 16, 17, n=65))
    cases.append(_case("paths-n16_k9-equal", "paths", 16, 9, equal=True))
    cases.append(_case("paths-n16_k9-far", "paths", 16, 9, far=True))
    for entry in ("drawdown", "horizons"):
        for N, K, begin in WALK_SHAPES:
            for comp in ("simple", "log"):
                cases.append(_case(f"{entry}-n{N}_k{K}-{comp}", entry, N, K, comp, begin))
        cases.append(_case(f"{entry}-n16_k9-equal", entry, 16, 9, equal=True))
    cases.append(_case("drawdown-n5_k3-n1", "drawdown", 5, 3, n=1))
    cases.append(_case("horizons-n5_k17-n65", "horizons", 5, 17, n=65))
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


CASES = _build()
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


# ---- inputs and restatements -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def market(N: int, K: int):
    """(mu, L, W) in binary32, read-only: the market and the long / short books of tests/offdefault_cases.py where they fit
    (N = 5), tests/native_ref.py's market of both signs at the other widths."""
    if N == oc.N:
        mu, L = oc.market(oc.LARGE)
        return mu, L, oc.weights(K)
    return native_ref.market(N, K)


def params(c: Case, **over):
    kw = dict(compounding=c.comp, v0=V0, alpha=ALPHA, rf=RF, native_math=c.native, fold=c.fold)
    kw.update(over)
    return _ffi.make_params(c.N, kw.pop("n_steps", c.T), kw.pop("n_portfolios", c.K), **kw)


def paths_of(c: Case):
    return np.arange(c.path_begin, c.path_begin + c.n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def expected(case_id: str):
    """{array: float32 [rows, n]} of a case from its restatement, read-only and shared: oracle.mc_oracle.simulate,
    drawdown_ref.simulate_paths_dd, horizons_ref.simulate_horizons (row h*K + k).  None for a case without one (Case.exact)."""
    c = BY_ID[case_id]
    if not c.exact:
        return None
    mu, L, W = market(c.N, c.K)
    if c.entry == "paths":
        out = {"terminal": mc_oracle.simulate(mu, L, W, c.T, c.n, SEED, c.path_begin, V0, c.comp)}
    elif c.entry == "drawdown":
        r = drawdown_ref.simulate_paths_dd(mu, L, W, c.T, SEED, paths_of(c), c.comp, V0)
        out = {"terminal": r["V_T"], "mdd": r["q"]}
    else:
        r = horizons_ref.simulate_horizons(mu, L, W, c.T, SEED, paths_of(c), c.horizons, c.comp, V0)
        out = {"terminal": r["V_T"], "horizon": r["V_h"].reshape(len(c.horizons) * c.K, c.n)}
    out = {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def ws_bytes(lib, c: Case) -> list:
    """Bytes of every work buffer of a case.  A horizon case runs the launch and the terminal select on K rows and the recipe of
    include/mcport.h on H*K rows in the same buffers: the larger of the two sizes, buffer by buffer (MCP_WS_BELOW does not grow
    with the rows)."""
    rows = c.rows.get("horizon", c.K)
    return [max(lib.mcp_ws_bytes(w, c.K, c.n), lib.mcp_ws_bytes(w, rows, c.n)) for w in range(_ffi.WS_COUNT)]


# ---- the caller-owned layout -------------------------------------------------------------------------------------------------------------

def alloc_elems(c: Case, array: str) -> int:
    """Elements of the allocation of one output array: its rows at the LARGEST stride of the call, plus TAIL."""
    return c.rows[array] * max(c.strides.values()) + TAIL


def filled(elems: int) -> np.ndarray:
    return np.full(elems, FILL_BITS, np.uint32)


def bits(values) -> np.ndarray:
    return np.ascontiguousarray(values, np.float32).view(np.uint32)


def violations(buf, want, stride: int, what: str = "") -> list:
    """What the GPU test asserts of one output array, as a list of complaints (empty: the array is right).  `buf`: the whole
    allocation as uint32; `want`: the float32 [rows, n] values it must hold.
      live      buf[r * stride + p] has the bits of want[r, p] for p < n
      padding   every element of [n, stride) of every row, and everything behind the last row, still holds FILL_BITS"""
    buf = np.asarray(buf, np.uint32).ravel()
    w = bits(want)
    rows, n = w.shape
    assert stride >= n and buf.size >= rows * stride
    body = buf[:rows * stride].reshape(rows, stride)
    out = []
    bad = np.argwhere(body[:, :n] != w)
    if bad.size:
        out.append(f"{what}: {len(bad)} of {w.size} live values differ, first at row {bad[0][0]} path {bad[0][1]}")
    pad = np.argwhere(body[:, n:] != FILL_BITS)
    if pad.size:
        out.append(f"{what}: {len(pad)} padding elements written, first at row {pad[0][0]} element {n + pad[0][1]}")
    tail = np.flatnonzero(buf[rows * stride:] != FILL_BITS)
    if tail.size:
        out.append(f"{what}: {tail.size} elements behind the last row written, first at {rows * stride + tail[0]}")
    return out


def live_of(buf, rows: int, n: int, stride: int) -> np.ndarray:
    """The float32 [rows, n] live values of an allocation."""
    return np.asarray(buf, np.uint32).ravel()[:rows * stride].reshape(rows, stride)[:, :n].copy().view(np.float32)


# ---- the store sites, restated with their possible mistakes --------------------------------------------------------------------------------

MISTAKES = ("n_paths for the stride", "another array's stride", "kt for n_portfolios", "no k_begin", "a dead lane stores")


def kernel_store(c: Case, array: str, want, mistake=None, other_stride=None) -> np.ndarray:
    """The allocation of `array` after the launch of case c, as uint32, if the kernels stored `want` [rows, n] the way the store
    sites of csrc/mcp_paths_body.inc and csrc/mcp_sweep_paths.hip do --

        terminal, mdd    row (k_begin + k) at (k_begin + k) * stride
        horizon          row (h * n_portfolios + k_begin + k) at that index times the stride

    pass by pass (passes_of), or with one of MISTAKES made at this array's store site.  "another array's stride" takes
    `other_stride`.  A dead lane is a lane of the last 64-path wave whose path id is not below n; the mistaken kernel lets it store
    (the value of path 0 of its row) before the live lanes do, so that a dead store that lands in the next row is overwritten, as it
    would be on the device whenever that row is written later.  A store beyond the allocation is dropped: this is NumPy, and
    alloc_elems is chosen so that none of the four stride and index mistakes leaves the allocation."""
    assert mistake is None or mistake in MISTAKES
    w = bits(want)
    rows, n = w.shape
    buf = filled(alloc_elems(c, array))
    stride = c.strides[array]
    if mistake == "n_paths for the stride":
        stride = n
    elif mistake == "another array's stride":
        stride = other_stride
    H = len(c.horizons) if array == "horizon" else 1
    assert rows == H * c.K
    lanes = -(-n // WAVE) * WAVE if mistake == "a dead lane stores" else n

    for dead in (True, False):                                  # the dead lanes of every pass first, then the live ones
        for k_begin, kt in passes_of(c):
            for h in range(H):
                for k in range(kt):
                    value_row = h * c.K + k_begin + k
                    base = 0 if mistake == "no k_begin" else k_begin
                    index = h * (kt if mistake == "kt for n_portfolios" else c.K) + base + k
                    lo, hi = (n, lanes) if dead else (0, n)
                    at = index * stride
                    hi = min(hi, buf.size - at)
                    if hi > lo:
                        buf[at + lo:at + hi] = w[value_row, 0] if dead else w[value_row, lo:hi]
    return buf

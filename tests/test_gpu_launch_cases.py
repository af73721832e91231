"""The enqueue-only path launches of include/mcport.h -- mcp_launch_paths, mcp_launch_paths_drawdown, mcp_launch_paths_horizons --
with caller-owned arrays at caller-chosen strides (tests/launch_cases.py), followed by the statistics steps and the two reduce
recipes the header gives an integrator.

Every case runs on a stream of its own (torch.cuda.Stream), once with d_partials = d_hist = NULL and twice with work buffers.  Each
output array is allocated at rows x (the largest stride of the call) + 64 elements and filled with one quiet-NaN pattern; after the
launch, launch_cases.violations holds it to

    live values   bit for bit the restatement's (oracle.mc_oracle, drawdown_ref, horizons_ref) and the host-level call's of the same
                  seed, range and parameters; the native-math and folded cases, which have no bit-for-bit restatement (DESIGN.md
                  section 3), to the host-level call alone; the last horizon row is the terminal row
    padding       [n_paths, stride) of every row and everything behind the last row still holds the pattern, compared as uint32

tests/test_launch_cases_cpu.py shows that these two assertions reject a store site that takes n_paths or another array's stride for
its stride, kt for n_portfolios, no k_begin, or lets a dead lane store.  With work buffers the terminal select, the drawdown recipe
(mcp_launch_pass0 over d_mdd at v0 = 1, rf = 0, no pivot) and the horizon recipe (n_portfolios = H*K, the pivots of mcp_pivots at
n_steps = h) then run with the case's strides, and every mcp_stats record is held to the host-level call's (the host sets the
Sharpe ratio of the drawdown and horizon records to 0, so that field is left out there):

    n, n_tail, var, x_lo, x_hi, min, max                bit for bit, in every case
    mean, m2, std (and the terminal sharpe)             bit for bit, in every case.  The path kernels' epilogue sums the terminal moments
                                                        lane by lane from registers; pass0_kernel, behind both recipes, reads element
                                                        i of a row with lane i of a fixed grid.  Neither order depends on the stride
    cvar, sum_tail                                      bit for bit where every row starts at the host-level call's offset modulo 16
                                                        bytes (r (stride - n) a multiple of 4 elements for every row r: the equal-
                                                        strides cases, n + 1000, every one-row array); elsewhere within 1e-12
                                                        relative, 1e-15 absolute of the host-level call's (the bounds of
                                                        tests/test_gpu_stats_matrix.py)

Why cvar and sum_tail are not bit for bit at every stride: hist_kernel<1> and <2> (csrc/mcp_stats_kernels.hip), which add up the
values below the quantile's bucket, read a row as a scalar head up to 16-byte alignment, a float4 body and a scalar tail.  Which lane
adds which element, and so the rounding of that fp64 sum, follows the row's alignment, which follows the stride.  In simple
compounding the terms are V - v0, binary32 differences that binary64 adds without rounding at these sizes; in log compounding they
are x = expm1(S), full binary64 numbers.  Every sum is also held to NumPy on the stored values within the same bounds."""
import ctypes

import numpy as np
import pytest

import launch_cases as lc
from drawdown_ref import mdd_of
from horizons_ref import x_of
from monte_carlo_portfolio_amd import _ffi

pytestmark = pytest.mark.gpu

FIELDS = _ffi.STATS_DTYPE.names
ORDER = ("n", "n_tail", "var", "x_lo", "x_hi", "min", "max")
MOMENTS = ("mean", "m2", "std", "sharpe")
TAIL_SUMS = ("cvar", "sum_tail")
RTOL, ATOL = 1e-12, 1e-15                  # tests/test_gpu_stats_matrix.py
assert set(ORDER + MOMENTS + TAIL_SUMS) == set(FIELDS)
_HOST = {}


def same_row_offsets(rows, stride, n):
    """Whether every row of an array at `stride` starts at the same offset modulo 16 bytes as at stride n (the host-level call's)."""
    return all(r * (stride - n) % 4 == 0 for r in range(rows))


def host_call(ctx, c):
    """The host-level call of a case's seed, range and parameters (the strides are its own: n_paths), once per process."""
    key = (c.entry, c.N, c.K, c.comp, c.native, c.fold, c.path_begin, c.n)
    if key not in _HOST:
        mu, L, W = lc.market(c.N, c.K)
        prm, walk = lc.params(c), (lc.SEED, c.path_begin, c.n)
        if c.entry == "paths":
            stats, term = ctx.simulate(prm, mu, L, W, *walk, True)
            out = dict(stats=stats, terminal=term)
        elif c.entry == "drawdown":
            stats, dd_stats, term, qd = ctx.simulate_drawdown(prm, mu, L, W, *walk, True)
            out = dict(stats=stats, dd_stats=dd_stats, terminal=term, mdd=qd)
        else:
            stats, hz_stats, bands, term, hz = ctx.simulate_horizons(prm, mu, L, W, *walk, c.horizons, lc.LEVELS, True)
            out = dict(stats=stats, hz_stats=hz_stats.reshape(-1), bands=bands.reshape(-1, len(lc.LEVELS)), terminal=term,
                       horizon=hz.reshape(len(c.horizons) * c.K, c.n))
        _HOST[key] = out
    return _HOST[key]


def assert_same_records(got, want, what, close=(), skip=()):
    """Two arrays of mcp_stats records, field by field: bit for bit, the fields of `close` within RTOL / ATOL."""
    assert got.shape == want.shape, what
    for f in FIELDS:
        if f in skip:
            continue
        if f in close:
            np.testing.assert_allclose(got[f], want[f], rtol=RTOL, atol=ATOL, err_msg=f"{what} {f}")
            continue
        a, b = np.ascontiguousarray(got[f]).view(np.uint64), np.ascontiguousarray(want[f]).view(np.uint64)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, f, f"{bad.size} of {a.size} records differ, first at {bad[0]}: {got[f][bad[0]]!r} != {want[f][bad[0]]!r}")


def assert_sums_of(rec, x, what, fields):
    """The sums of records against NumPy on x [rows, n], the binary64 x of the stored values: mean, std (ddof = 1), and the tail sum
    and mean over the n_tail smallest values of each row (the tail is x <= var, and x is monotone in the stored value)."""
    n = x.shape[1]
    xs = np.sort(x, axis=1)
    sum_tail = np.array([xs[r, :int(rec["n_tail"][r])].sum() for r in range(x.shape[0])])
    ref = {"mean": x.mean(axis=1), "std": x.std(axis=1, ddof=1) if n > 1 else np.zeros(x.shape[0]), "sum_tail": sum_tail,
           "cvar": sum_tail / rec["n_tail"]}
    assert np.all(rec["n_tail"] >= 1), what
    for f in fields:
        if f in ref:                                       # m2 goes with std, the Sharpe ratio with mean and std
            np.testing.assert_allclose(rec[f], ref[f], rtol=RTOL, atol=ATOL, err_msg=f"{what} {f} against NumPy on the stored values")


class Launch:
    """The device side of one case: inputs, the filled output arrays, zeroed work buffers and a stream of its own."""

    def __init__(self, c):
        import torch
        self.torch, self.lib, self.c = torch, _ffi.lib(), c
        dev = self.dev = torch.device("cuda", 0)
        self.mu, self.L, self.W = lc.market(c.N, c.K)
        self.prm = lc.params(c)
        self.packed = torch.from_numpy(_ffi.pack_params(self.mu, self.L, self.W)).to(dev)
        self.pivot = torch.from_numpy(_ffi.pivots(self.prm, self.mu, self.L, self.W)).to(dev)
        self.out = {a: torch.from_numpy(lc.filled(lc.alloc_elems(c, a)).view(np.int32)).to(dev) for a in c.strides}
        self.ws = [torch.zeros((b + 7) // 8, dtype=torch.int64, device=dev) for b in lc.ws_bytes(self.lib, c)]
        self.steps = np.asarray(c.horizons, np.int32)
        if c.entry == "horizons":                          # row h*K + k is pivoted at n_steps = h
            hp = np.concatenate([_ffi.pivots(lc.params(c, n_steps=h), self.mu, self.L, self.W) for h in c.horizons])
            self.hz_pivot = torch.from_numpy(hp).to(dev)
        self.stream = torch.cuda.Stream(dev)
        assert self.stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        self.st = ctypes.c_void_p(self.stream.cuda_stream)
        self.n_launches = 0
        torch.cuda.synchronize()                           # the uploads and fills above ran on the default stream

    @staticmethod
    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def sync(self):
        self.stream.synchronize()

    def refill(self):
        """Every output array back to the fill pattern."""
        for a, t in self.out.items():
            t.copy_(self.torch.from_numpy(lc.filled(t.numel()).view(np.int32)))
        self.torch.cuda.synchronize()
        assert all(np.all(self.array(a) == lc.FILL_BITS) for a in self.out)

    def array(self, a):
        """The whole allocation of an output array as uint32 (after sync)."""
        return self.out[a].cpu().numpy().view(np.uint32)

    def paths(self, with_ws):
        c, p, B = self.c, self.p, ctypes.byref(self.prm)
        P, H = (p(self.ws[_ffi.WS_PARTIALS]), p(self.ws[_ffi.WS_HIST])) if with_ws else (None, None)
        head = (B, p(self.packed), p(self.pivot), lc.SEED, c.path_begin, c.n, p(self.out["terminal"]), c.terminal_stride)
        if c.entry == "paths":
            rc = self.lib.mcp_launch_paths(*head, P, H, self.st)
        elif c.entry == "drawdown":
            rc = self.lib.mcp_launch_paths_drawdown(*head, p(self.out["mdd"]), c.mdd_stride, P, H, self.st)
        else:
            rc = self.lib.mcp_launch_paths_horizons(*head, len(self.steps), self.steps.ctypes.data_as(ctypes.c_void_p), p(self.out["horizon"]),
                                                    c.hz_stride, P, H, self.st)
        _ffi.check(rc)
        self.n_launches += 1

    def pass0(self, prm, values, stride, pivot):
        ws, p = self.ws, self.p
        _ffi.check(self.lib.mcp_launch_pass0(ctypes.byref(prm), p(values), stride, self.c.n, p(pivot), p(ws[_ffi.WS_PARTIALS]),
                                             p(ws[_ffi.WS_HIST]), self.st))

    def select(self, prm, values, stride, pivot, ranks):
        """scan(0) -> hist(1) -> scan(1) -> hist(2) -> final over `values` at `stride`, on the partials and the digit-0 histogram that
        the launch or a pass 0 left -> the [n_portfolios of prm] records; the histogram must be zero again afterwards."""
        lib, n, p, B = self.lib, self.c.n, self.p, ctypes.byref(prm)
        P, R, S, H, Q, O, BL = (p(self.ws[w]) for w in (_ffi.WS_PARTIALS, _ffi.WS_RECORD, _ffi.WS_STATE, _ffi.WS_HIST, _ffi.WS_QUANT, _ffi.WS_STATS,
                                                        _ffi.WS_BELOW))
        V, C, (lo, hi, g) = p(values), p(pivot), ranks
        _ffi.check(lib.mcp_launch_scan(B, 0, n, lo, hi, P, BL, C, H, S, R, self.st))
        _ffi.check(lib.mcp_launch_hist(B, 1, V, stride, n, S, C, BL, H, self.st))
        _ffi.check(lib.mcp_launch_scan(B, 1, n, lo, hi, P, BL, C, H, S, R, self.st))
        _ffi.check(lib.mcp_launch_hist(B, 2, V, stride, n, S, C, BL, H, self.st))
        _ffi.check(lib.mcp_launch_final(B, n, g, lo, hi, BL, H, S, R, Q, O, self.st))
        self.sync()
        rows = prm.n_portfolios
        rec = self.ws[_ffi.WS_STATS].cpu().numpy().view(np.uint8)[:rows * _ffi.STATS_DTYPE.itemsize].view(_ffi.STATS_DTYPE).copy()
        assert not self.ws[_ffi.WS_HIST].cpu().numpy().any(), (self.c.id, "the select leaves the histogram zero")
        return rec


def check_arrays(ln, host, tag):
    """Live values and padding of every output array of a finished launch."""
    c = ln.c
    want = lc.expected(c.id)
    got = {}
    for a, stride in c.strides.items():
        buf = got[a] = ln.array(a)
        assert buf.size == lc.alloc_elems(c, a)
        complaints = lc.violations(buf, host[a], stride, f"{c.id} [{tag}] {a} against the host-level call")
        if c.exact:
            complaints += lc.violations(buf, want[a], stride, f"{c.id} [{tag}] {a} against the restatement")
        assert not complaints, complaints
    if c.entry == "horizons":
        last = lc.live_of(got["horizon"], c.rows["horizon"], c.n, c.hz_stride)[-c.K:]
        assert np.array_equal(lc.bits(last), lc.bits(lc.live_of(got["terminal"], c.K, c.n, c.terminal_stride))), (c.id, tag, "the last horizon is T")
    return got


def check_drawdown_record(c, rec, q):
    """The recipe's order statistics against NumPy on the stored q / d: x = q - 1 or expm1(d).  Simple compounding: the quantile, the
    counts and the extremes exactly.  Log compounding: to 1e-12, the device's expm1 not being NumPy's to the last bit (the bound of
    tests/test_gpu_offdefault.py::assert_record)."""
    x = mdd_of(q, c.comp)
    var = np.percentile(x, (1 - lc.ALPHA) * 100, axis=1)
    assert np.array_equal(rec["n"], np.full(c.K, c.n)), c.id
    if c.comp == "simple":
        assert np.array_equal(rec["var"], var), (c.id, "drawdown-at-risk")
        assert np.array_equal(rec["n_tail"], (x <= var[:, None]).sum(axis=1)), c.id
        assert np.array_equal(rec["min"], x.min(axis=1)) and np.array_equal(rec["max"], x.max(axis=1)), c.id
    else:
        for f, ref in (("var", var), ("min", x.min(axis=1)), ("max", x.max(axis=1))):
            np.testing.assert_allclose(rec[f], ref, rtol=RTOL, atol=ATOL, err_msg=f"{c.id} {f}")
    return x


def run_with_work_buffers(ln, host, first):
    """The launch with the fused epilogue, the terminal select, then the recipe of the case's entry point -> every byte it left."""
    c = ln.c
    hist = ln.ws[_ffi.WS_HIST]
    assert not hist.cpu().numpy().any()                    # MCP_WS_HIST is zero when first used, and whenever a select has run
    ln.paths(True)
    ln.sync()
    left = {a: buf.tobytes() for a, buf in check_arrays(ln, host, "work buffers").items()}
    ranks = _ffi.percentile_rank(c.n, lc.ALPHA)
    rec = ln.select(ln.prm, ln.out["terminal"], c.terminal_stride, ln.pivot, ranks)
    if first:                                              # the moments always bit for bit; the tail sums where the rows lie alike
        close = () if same_row_offsets(c.K, c.terminal_stride, c.n) else TAIL_SUMS
        assert_same_records(rec, host["stats"], f"{c.id}: terminal records against the host-level call", close=close)
        x = x_of(lc.live_of(ln.array("terminal"), c.K, c.n, c.terminal_stride), c.comp, lc.V0)
        assert_sums_of(rec, x, f"{c.id}: terminal records", MOMENTS + TAIL_SUMS)
    left["stats"] = rec.tobytes()
    if c.entry == "drawdown":                              # include/mcport.h: a copy of the parameters with v0 = 1, rf = 0, no pivot
        prm1 = lc.params(c, v0=1.0, rf=0.0)
        ln.pass0(prm1, ln.out["mdd"], c.mdd_stride, None)
        rec = ln.select(prm1, ln.out["mdd"], c.mdd_stride, None, ranks)
        if first:
            assert np.all(host["dd_stats"]["sharpe"] == 0.0)
            close = () if same_row_offsets(c.K, c.mdd_stride, c.n) else TAIL_SUMS
            assert_same_records(rec, host["dd_stats"], f"{c.id}: drawdown records against the host-level call", close=close, skip=("sharpe",))
            x = check_drawdown_record(c, rec, lc.live_of(ln.array("mdd"), c.K, c.n, c.mdd_stride))
            assert_sums_of(rec, x, f"{c.id}: drawdown records", MOMENTS + TAIL_SUMS)
        left["dd_stats"] = rec.tobytes()
    if c.entry == "horizons":                              # include/mcport.h: n_portfolios = H*K, the pivots at n_steps = h
        rows = c.rows["horizon"]
        prmh = lc.params(c, n_portfolios=rows)
        ln.pass0(prmh, ln.out["horizon"], c.hz_stride, ln.hz_pivot)
        rec = ln.select(prmh, ln.out["horizon"], c.hz_stride, ln.hz_pivot, ranks)
        if first:
            assert np.all(host["hz_stats"]["sharpe"] == 0.0)
            close = () if same_row_offsets(rows, c.hz_stride, c.n) else TAIL_SUMS
            assert_same_records(rec, host["hz_stats"], f"{c.id}: horizon records against the host-level call", close=close, skip=("sharpe",))
            x = x_of(lc.live_of(ln.array("horizon"), rows, c.n, c.hz_stride), c.comp, lc.V0)
            assert_sums_of(rec, x, f"{c.id}: horizon records", MOMENTS + TAIL_SUMS)
        ln.pass0(prmh, ln.out["horizon"], c.hz_stride, ln.hz_pivot)
        band = ln.select(prmh, ln.out["horizon"], c.hz_stride, ln.hz_pivot, _ffi.percentile_rank_q(c.n, lc.LEVELS[lc.BAND]))
        band = np.ascontiguousarray(band["var"])
        if first:
            want = np.ascontiguousarray(host["bands"][:, lc.BAND])
            assert band.view(np.uint64).tolist() == want.view(np.uint64).tolist(), (c.id, "the band of one level", band, want)
        left["hz_stats"], left["band"] = rec.tobytes(), band.tobytes()
    return left


@pytest.mark.parametrize("cid", lc.CASE_IDS)
def test_launch_at_caller_chosen_strides(gpu_ctx, cid):
    c = lc.BY_ID[cid]
    host = host_call(gpu_ctx, c)
    if c.exact:                                            # the two references agree with each other before either is used
        for a, v in lc.expected(cid).items():
            assert np.array_equal(lc.bits(v), lc.bits(host[a])), (cid, a, "the host-level call against the restatement")
    ln = Launch(c)

    # d_partials = d_hist = NULL (include/mcport.h: both or neither): the stores alone; work buffers that were not passed stay zero
    ln.paths(False)
    ln.sync()
    check_arrays(ln, host, "NULL statistics buffers")
    for w in (_ffi.WS_HIST, _ffi.WS_PARTIALS):
        assert not ln.ws[w].cpu().numpy().any(), (cid, "a work buffer that was not passed was written", w)

    # with work buffers, twice on the same buffers; the output arrays are filled again before each run, so that every run's own
    # stores are checked
    ln.refill()
    one = run_with_work_buffers(ln, host, True)
    ln.refill()
    two = run_with_work_buffers(ln, host, False)
    assert one.keys() == two.keys()
    for name in one:
        assert one[name] == two[name], (cid, name, "a second run on the same buffers gives other bytes")
    assert ln.n_launches == 3

"""hist_kernel<0> (the digit-0 histogram behind the MFMA sweep kernels) against pass0_kernel and NumPy, and padded rows through the
whole select, all through the device-level ABI (include/mcport.h: mcp_launch_hist, mcp_launch_pass0, mcp_launch_scan,
mcp_launch_final).

The rows and pivots come from tests/stats_cases.py; tests/test_stats_cases_cpu.py asserts on NumPy alone that they reach the fast
path of the kernel (the 16-bin window with one column per lane) and its slow path in the same launch, both clamps of the window's
first bin, and the digits on either side of both window edges.  Here 19 rows of n values lie `stride = n + s` elements apart, s in
{0, 1, 2, 3}, so rows start at all four offsets modulo 16 bytes and the head / float4 body / tail split of hist_kernel meets each;
the s elements behind every row are NaN with the sign bit set (digit 0, below every value in key order), so a kernel that reads
one counts it in bin 0 of pass 0, or adds it to the sum below the quantile's bucket in passes 1 and 2 and CVaR comes out NaN.

Both kernels must give np.bincount(key >> 21) per row in hist[k][0] and leave hist[k][1] zero, whatever the pivot: a NULL pointer,
0, the x of the row's first value, -1 (window centre 0), +-3e38 (the clamps) and NaN.  Digit 2047 is asked for as a value too: it
is a NaN payload pattern, which these integer-only histograms count like any other key.
"""
import ctypes

import numpy as np
import pytest

import stats_cases as sc
from monte_carlo_portfolio_amd import _ffi

pytestmark = pytest.mark.gpu


def work_buffers(lib, K, n, dev):
    import torch
    return [torch.zeros((lib.mcp_ws_bytes(w, K, n) + 7) // 8, dtype=torch.int64, device=dev) for w in range(_ffi.WS_COUNT)]


@pytest.mark.parametrize("n", sc.HIST_SIZES)
def test_digit0_histogram_equals_pass0_and_numpy(gpu_ctx, n):
    import torch
    lib = _ffi.lib()
    K = sc.HIST_K
    dev = torch.device("cuda", 0)
    ws = work_buffers(lib, K, n, dev)
    hist, partials = ws[_ffi.WS_HIST], ws[_ffi.WS_PARTIALS]
    words = K * 2 * sc.BINS
    assert hist.numel() >= words
    zeros = torch.zeros(hist.numel(), dtype=torch.int64)             # host side: the histogram is cleared and read by plain copies
    H, P = ctypes.c_void_p(hist.data_ptr()), ctypes.c_void_p(partials.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    prm = {comp: _ffi.make_params(4, 1, K, comp, sc.HIST_V0) for comp in ("simple", "log")}
    n_cases = 0
    for kind, comp, pk, values, pivot, dlo in sc.hist0_cases(n):
        want = sc.hist0_expected(values).view(np.int64).reshape(-1)
        assert int(want.sum()) == K * n                              # every value counted once, the padding never
        d_pivot = torch.from_numpy(pivot).to(dev) if pivot is not None else None
        C = ctypes.c_void_p(d_pivot.data_ptr()) if d_pivot is not None else None
        B = ctypes.byref(prm[comp])
        for pad in sc.HIST_PADS:
            term = torch.from_numpy(sc.padded(values, pad)).to(dev)
            assert term.data_ptr() % 16 == 0
            T = ctypes.c_void_p(term.data_ptr())
            for rep in range(2):                                     # twice on the same buffers
                _ffi.check(lib.mcp_launch_hist(B, 0, T, n + pad, n, None, C, None, H, st))
                lean = hist.cpu().numpy()
                hist.copy_(zeros)
                _ffi.check(lib.mcp_launch_pass0(B, T, n + pad, n, C, P, H, st))
                full = hist.cpu().numpy()
                hist.copy_(zeros)
                tag = (kind, comp, pk, pad, rep)
                assert np.array_equal(lean[:words], want) and not lean[words:].any(), ("hist_kernel<0>", tag)
                assert np.array_equal(full[:words], want) and not full[words:].any(), ("pass0_kernel", tag)
            n_cases += 1
    assert n_cases == 7 * len(sc.HIST_PIVOTS) * len(sc.HIST_PADS)


@pytest.mark.parametrize("alpha", [0.95, 0.01])
def test_padded_rows_through_the_whole_select(gpu_ctx, alpha):
    """pass0 -> scan -> hist(1) -> scan -> hist(2) -> final on 19 rows of 4,099 values 4,102 elements apart, NaN behind every row,
    v0 = 3, per-row pivots.  Any read past n turns a sum into NaN or moves a count: this is the check that the padding is never
    touched by pass0_kernel, hist_kernel<1> and hist_kernel<2>."""
    import torch
    lib = _ffi.lib()
    K, n, pad, v0 = sc.HIST_K, 4099, 3, 3.0
    rng = np.random.default_rng(4099)
    v = (v0 * (1.02 + 0.05 * rng.standard_normal((K, n)))).astype(np.float32)     # mean of x about 0.02: rtol on the mean is meaningful
    x = v.astype(np.float64) / np.float64(np.float32(v0)) - 1.0
    dev = torch.device("cuda", 0)
    term = torch.from_numpy(sc.padded(v, pad)).to(dev)
    ws = work_buffers(lib, K, n, dev)
    ws[_ffi.WS_PIVOT] = torch.from_numpy(x[:, 0].copy()).to(dev)
    p = [ctypes.c_void_p(t.data_ptr()) for t in ws]
    prm = _ffi.make_params(4, 1, K, "simple", v0, alpha, 0.0)
    lo, hi, g = _ffi.percentile_rank(n, alpha)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    T, B, stride = ctypes.c_void_p(term.data_ptr()), ctypes.byref(prm), n + pad
    P, R, S, H, Q, O, BL, C = (p[_ffi.WS_PARTIALS], p[_ffi.WS_RECORD], p[_ffi.WS_STATE], p[_ffi.WS_HIST], p[_ffi.WS_QUANT], p[_ffi.WS_STATS],
                               p[_ffi.WS_BELOW], p[_ffi.WS_PIVOT])
    want_var = np.percentile(x, (1 - alpha) * 100, axis=1)
    tail = x <= want_var[:, None]
    first = None
    for rep in range(2):
        _ffi.check(lib.mcp_launch_pass0(B, T, stride, n, C, P, H, st))
        _ffi.check(lib.mcp_launch_scan(B, 0, n, lo, hi, P, BL, C, H, S, R, st))
        _ffi.check(lib.mcp_launch_hist(B, 1, T, stride, n, S, C, BL, H, st))
        _ffi.check(lib.mcp_launch_scan(B, 1, n, lo, hi, P, BL, C, H, S, R, st))
        _ffi.check(lib.mcp_launch_hist(B, 2, T, stride, n, S, C, BL, H, st))
        _ffi.check(lib.mcp_launch_final(B, n, g, lo, hi, BL, H, S, R, Q, O, st))
        torch.cuda.synchronize()
        rec = ws[_ffi.WS_STATS].cpu().numpy().view(np.uint8)[:K * _ffi.STATS_DTYPE.itemsize].view(_ffi.STATS_DTYPE).copy()
        assert np.array_equal(rec["n"], np.full(K, n))
        assert np.array_equal(rec["var"], want_var)
        assert np.array_equal(rec["n_tail"], tail.sum(axis=1))
        np.testing.assert_allclose(rec["cvar"], np.where(tail, x, 0.0).sum(axis=1) / tail.sum(axis=1), rtol=1e-12)
        np.testing.assert_allclose(rec["mean"], x.mean(axis=1), rtol=1e-12)
        np.testing.assert_allclose(rec["std"], x.std(axis=1, ddof=1), rtol=1e-12)
        assert np.array_equal(rec["min"], x.min(axis=1)) and np.array_equal(rec["max"], x.max(axis=1))
        assert not ws[_ffi.WS_HIST].cpu().numpy().any()            # read-and-clear protocol: the histogram is back to zero
        assert first is None or first.tobytes() == rec.tobytes()   # bit-identical on a second run
        first = rec

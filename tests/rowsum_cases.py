"""What tests/test_gpu_rowsum_bytes.py and tests/golden/make_rowsum_parent_goldens.py share: the sizes, the input rows and the two
launches whose raw records are held to recorded bytes.

The inputs come from integer arithmetic alone: LANES linear congruential generators (Knuth's 64-bit multiplier and increment) stepped
side by side, the top 24 bits of each state as a binary32 u in [0, 1), x = 0.01 + 0.001 r + 0.1 (u - 0.5) in binary64 and the stored
value fl32(1 + x).  No NumPy generator is involved, so the rows are the same under every NumPy version.  Simple compounding, v0 = 1.
"""
import ctypes

import numpy as np

from monte_carlo_portfolio_amd import _ffi

LCG_A, LCG_C, LANES = np.uint64(6364136223846793005), np.uint64(1442695040888963407), 4096
TAU = 0.013
DS_ROWS, RL_ROWS, RL_GROUP, RL_BENCH = 3, 6, 3, 1
Y_KEPT_UP_TO = 1025          # the fixture holds Y at the sizes up to this one


def sizes(lib):
    """The n at which a change to the row walker, the workgroup record or the merge can go wrong."""
    trip = int(lib.mcp_downside_trip_n())
    return (1, 2, 5, 6, 1025, 66_000, trip + 3, 3 * trip)


def lcg_uniform(count, seed):
    """[count] binary32 in [0, 1): lane l starts at seed + l and yields elements l, l + LANES, ..."""
    steps = -(-count // LANES)
    out = np.empty((steps, LANES), np.float32)
    with np.errstate(over="ignore"):
        s = (np.arange(LANES, dtype=np.uint64) + np.uint64(seed)) * LCG_A + LCG_C
        for i in range(steps):
            s = s * LCG_A + LCG_C
            out[i] = (s >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return out.reshape(-1)[:count]


def rows(n_rows, n, seed, pivot_step=0.001):
    """([n_rows, n] binary32 stored values, [n_rows] pivots)."""
    u = lcg_uniform(n_rows * n, seed).reshape(n_rows, n).astype(np.float64)
    pivots = 0.02 + pivot_step * np.arange(n_rows)
    x = (0.01 + pivot_step * np.arange(n_rows))[:, None] + 0.1 * (u - 0.5)
    return (1.0 + x).astype(np.float32), pivots


def _device(vals, pivots):
    """The rows laid stride = n + 3 apart behind a one-element offset, NaN everywhere else -> (device, buffer, pivots, stride)."""
    import torch
    dev = torch.device("cuda", 0)
    n_rows, n = vals.shape
    stride = n + 3
    host = np.full(1 + n_rows * stride + 8, -np.nan, np.float32)
    host[1:1 + n_rows * stride].reshape(n_rows, stride)[:, :n] = vals
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    return dev, buf, torch.from_numpy(np.ascontiguousarray(pivots, np.float64)).to(dev), stride


def run_downside(lib, vals, pivots):
    """mcp_launch_downside -> [rows, 12] uint64 words of the records."""
    import torch
    n_rows, n = vals.shape
    dev, buf, d_pivot, stride = _device(vals, pivots)
    partials = torch.full(((lib.mcp_downside_ws_bytes(n_rows, n) + 7) // 8,), -1, dtype=torch.int64, device=dev)
    sums = torch.full((n_rows * 12,), -1, dtype=torch.int64, device=dev)
    prm = _ffi.make_params(1, 1, 1, "simple", 1.0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _ffi.check(lib.mcp_launch_downside(ctypes.byref(prm), ctypes.c_void_p(buf.data_ptr() + 4), stride, n, n_rows,
                                       ctypes.c_void_p(d_pivot.data_ptr()), TAU, ctypes.c_void_p(partials.data_ptr()),
                                       ctypes.c_void_p(sums.data_ptr()), st))
    return sums.cpu().numpy().view(np.uint64).reshape(n_rows, 12)


def run_relative(lib, vals, pivots, group, bench):
    """mcp_launch_relative with `active` given -> ([rows, 18] uint64 words of the records, [rows, n] uint32 bits of Y).  Asserts that
    nothing outside the live Y values was written."""
    import torch
    n_rows, n = vals.shape
    dev, buf, d_pivot, stride = _device(vals, pivots)
    ybuf = torch.full((1 + n_rows * stride + 8,), float("nan"), dtype=torch.float32, device=dev)
    partials = torch.full(((lib.mcp_relative_ws_bytes(n_rows, n) + 7) // 8,), -1, dtype=torch.int64, device=dev)
    sums = torch.full((n_rows * 18,), -1, dtype=torch.int64, device=dev)
    prm = _ffi.make_params(1, 1, 1, "simple", 1.0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _ffi.check(lib.mcp_launch_relative(ctypes.byref(prm), ctypes.c_void_p(buf.data_ptr() + 4), stride, n, n_rows, group, bench,
                                       ctypes.c_void_p(d_pivot.data_ptr()), ctypes.c_void_p(partials.data_ptr()),
                                       ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(ybuf.data_ptr() + 4), st))
    y = ybuf.cpu().numpy()
    live = np.zeros(y.size, bool)
    live[1:1 + n_rows * stride].reshape(n_rows, stride)[:, :n] = True
    assert np.all(np.isnan(y[~live])) and not np.any(np.isnan(y[live])), "Y outside the live values, or NaN inside"
    y = np.ascontiguousarray(y[1:1 + n_rows * stride].reshape(n_rows, stride)[:, :n])
    return sums.cpu().numpy().view(np.uint64).reshape(n_rows, 18), y.view(np.uint32)


def record_all(lib):
    """{name: array} of everything the fixture holds, from the library in use."""
    out = {}
    for n in sizes(lib):
        vals, pivots = rows(DS_ROWS, n, 1000 + n)
        out[f"downside_n{n}"] = run_downside(lib, vals, pivots)
        vals, pivots = rows(RL_ROWS, n, 2000 + n)
        out[f"relative_n{n}"], y = run_relative(lib, vals, pivots, RL_GROUP, RL_BENCH)
        if n <= Y_KEPT_UP_TO:
            out[f"relative_y_n{n}"] = y
    return out

"""ctypes binding of libmcport.so (C ABI: include/mcport.h).

The library is the product's only compute path: if it is missing or cannot be loaded this module
raises -- there is no NumPy/CPU fallback (a silent fallback would void every parity claim).
"""
from __future__ import annotations

import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCP_LIB_PATH") or os.path.join(_PKG, "libmcport.so")     # MCP_LIB_PATH: a lab build (tools/kernel_lab.py)
CSRC = os.path.join(_PKG, "csrc")

MCP_ABI_VERSION = 4
MCP_MAX_ASSETS = 64
MCP_SELECT_BINS = 2048
MCP_MAX_HORIZONS = 64
MCP_MAX_LEVELS = 16
MCP_MAX_BOOT_ROWS = 1 << 20
MCP_MAX_T_DOF = 32
MCP_MAX_OVERLAY_ROWS = 8
MCP_MAX_ATTR_PORTFOLIOS = 16
MCP_MAX_JUMPS = 8
MCP_MAX_GLIDE = 64
MCP_OVERLAY_LINEAR, MCP_OVERLAY_CALL, MCP_OVERLAY_PUT = 0, 1, 2
MCP_COMPOUND = {"simple": 0, "log": 1}
MCP_FLAG_NATIVE_MATH = 1
MCP_FLAG_FOLD = 2
MCP_FLAG_SHARD_PORTFOLIOS = 4
MCP_E_ARG, MCP_E_NODEVICE, MCP_E_NOMEM, MCP_E_UNSUPPORTED, MCP_E_HIP, MCP_E_COMM = -1, -2, -3, -4, -5, -6
(WS_PARTIALS, WS_RECORD, WS_STATE, WS_HIST, WS_QUANT, WS_STATS, WS_BELOW, WS_PIVOT) = range(8)
WS_COUNT = 8
(EXCHANGE_UNSET, EXCHANGE_NONE, EXCHANGE_RCCL, EXCHANGE_KERNEL, EXCHANGE_P2P) = range(5)


class McpError(RuntimeError):
    """Raised for any negative return code of the C ABI; carries mcp_last_error()."""


class McpParams(ctypes.Structure):
    _fields_ = [
        ("n_assets", ctypes.c_int32), ("n_steps", ctypes.c_int32), ("n_portfolios", ctypes.c_int32),
        ("compounding", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("v0", ctypes.c_double), ("alpha", ctypes.c_double), ("rf", ctypes.c_double),
    ]


class McpStats(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64), ("n_tail", ctypes.c_uint64), ("mean", ctypes.c_double), ("m2", ctypes.c_double),
        ("std", ctypes.c_double), ("sharpe", ctypes.c_double), ("var", ctypes.c_double), ("cvar", ctypes.c_double),
        ("min", ctypes.c_double), ("max", ctypes.c_double), ("sum_tail", ctypes.c_double),
        ("x_lo", ctypes.c_double), ("x_hi", ctypes.c_double),
    ]


class McpBootstrap(ctypes.Structure):
    """mcp_bootstrap: the observed return rows of a bootstrap call (SPEC.md 2.1)."""
    _fields_ = [("rows", ctypes.c_void_p), ("n_rows", ctypes.c_int32), ("reserved", ctypes.c_int32), ("mean_block", ctypes.c_double)]


class McpRebalance(ctypes.Structure):
    """mcp_rebalance: the rebalancing rule of SPEC.md 4.5 (period 0: never, buy-and-hold; cost: proportional, in [0, 1))."""
    _fields_ = [("period", ctypes.c_int32), ("reserved", ctypes.c_int32), ("cost", ctypes.c_double)]


class McpBand(ctypes.Structure):
    """mcp_band: the tolerance bands of SPEC.md 4.18 (every: the review period, 0 never; cost: proportional, in [0, 1); tol: float32
    [K][N], every entry >= 0 or +inf for an asset that is not watched)."""
    _fields_ = [("every", ctypes.c_int32), ("reserved", ctypes.c_int32), ("cost", ctypes.c_double), ("tol", ctypes.c_void_p)]


class McpStudentT(ctypes.Structure):
    """mcp_student_t: the degrees of freedom nu in [3, MCP_MAX_T_DOF] of Student-t draws (SPEC.md 2.2)."""
    _fields_ = [("dof", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class McpFiltered(ctypes.Structure):
    """mcp_filtered: the filtered residual rows of a filtered-historical-simulation call (SPEC.md 2.4)."""
    _fields_ = [("mu", ctypes.c_void_p), ("resid", ctypes.c_void_p), ("shock", ctypes.c_void_p), ("n_rows", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("mean_block", ctypes.c_double)]


class McpGarch(ctypes.Structure):
    """mcp_garch: alpha, beta and the starting variance ratio h0 of the GARCH(1,1) recurrence of SPEC.md 4.9."""
    _fields_ = [("alpha", ctypes.c_double), ("beta", ctypes.c_double), ("h0", ctypes.c_double), ("reserved", ctypes.c_uint64)]


class McpJumps(ctypes.Structure):
    """mcp_jumps: intensity, mean and std of the market jump of SPEC.md 2.5 and the [N] binary32 loadings (NULL: all ones)."""
    _fields_ = [("intensity", ctypes.c_double), ("mean", ctypes.c_double), ("std", ctypes.c_double), ("loading", ctypes.c_void_p),
                ("reserved", ctypes.c_int32)]


class McpRegimes(ctypes.Structure):
    """mcp_regimes: the transition and start probabilities of SPEC.md 2.6 and regime 1's binary32 drift [N] and Cholesky factor [N, N]."""
    _fields_ = [("p01", ctypes.c_double), ("p10", ctypes.c_double), ("start", ctypes.c_double), ("mu1", ctypes.c_void_p),
                ("chol1", ctypes.c_void_p), ("reserved", ctypes.c_int32)]


class McpCashflow(ctypes.Structure):
    """mcp_cashflow: the schedule c_1 .. c_T (binary32, n_flows == n_steps) and the optional target of SPEC.md 4.7 / 5.6."""
    _fields_ = [("flows", ctypes.c_void_p), ("n_flows", ctypes.c_int32), ("has_target", ctypes.c_int32), ("target", ctypes.c_double)]


class McpGlide(ctypes.Structure):
    """mcp_glide: the breaks (int32 [G]) and target weight blocks (binary32 [G, K, N]) of the glide path of SPEC.md 4.14."""
    _fields_ = [("breaks", ctypes.c_void_p), ("targets", ctypes.c_void_p), ("n_breaks", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class McpProtect(ctypes.Structure):
    """mcp_protect (include/mcport_protect.h): the floor schedule (binary32 [n_steps + 1]), multiplier, cap, rate and ratchet of
    SPEC.md 4.15 and the optional target (NULL or one binary64 value)."""
    _fields_ = [("floor", ctypes.c_void_p), ("multiplier", ctypes.c_double), ("cap", ctypes.c_double), ("rate", ctypes.c_double),
                ("ratchet", ctypes.c_double), ("target", ctypes.c_void_p), ("reserved", ctypes.c_int32)]


class McpVolTarget(ctypes.Structure):
    """mcp_vol_target (include/mcport_voltarget.h): target, decay, cap, rate and spread of SPEC.md 4.19, the optional initial variance
    estimates (NULL or binary64 [K]) and the optional target value of the second count (NULL or one binary64 value)."""
    _fields_ = [("target", ctypes.c_double), ("decay", ctypes.c_double), ("cap", ctypes.c_double), ("rate", ctypes.c_double),
                ("spread", ctypes.c_double), ("s0", ctypes.c_void_p), ("target_value", ctypes.c_void_p), ("reserved", ctypes.c_int32)]


class McpDriftUncertainty(ctypes.Structure):
    """mcp_drift_uncertainty (include/mcport_uncertain.h): the lower-triangular factor M of the covariance of the drift (binary32
    [N, N]) of SPEC.md 2.7 / 4.21."""
    _fields_ = [("factor", ctypes.c_void_p), ("reserved", ctypes.c_int32)]


class McpSpending(ctypes.Structure):
    """mcp_spending (include/mcport_spend.h): the rate, the largest cut and raise per review, the inflation per review, the optional
    first withdrawal and target, and the review period of the spending rule of SPEC.md 4.16."""
    _fields_ = [("rate", ctypes.c_double), ("down", ctypes.c_double), ("up", ctypes.c_double), ("inflation", ctypes.c_double),
                ("first", ctypes.c_double), ("target", ctypes.c_double), ("every", ctypes.c_int32), ("has_first", ctypes.c_int32),
                ("has_target", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class McpOverlay(ctypes.Structure):
    """mcp_overlay: the option rows of SPEC.md 4.8 -- rows [n_rows] of OVERLAY_ROW_DTYPE, row_begin int32 [N + 1], spot binary32 [N]."""
    _fields_ = [("rows", ctypes.c_void_p), ("row_begin", ctypes.c_void_p), ("spot", ctypes.c_void_p), ("n_rows", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


# one mcp_overlay_row: kind 0 LINEAR, 1 CALL, 2 PUT; the sign of a short row is folded into qty
OVERLAY_ROW_DTYPE = np.dtype([("kind", np.int32), ("strike", np.float32), ("premium", np.float32), ("qty", np.float32)])
assert OVERLAY_ROW_DTYPE.itemsize == 16

STATS_DTYPE = np.dtype([
    ("n", np.uint64), ("n_tail", np.uint64), ("mean", np.float64), ("m2", np.float64), ("std", np.float64),
    ("sharpe", np.float64), ("var", np.float64), ("cvar", np.float64), ("min", np.float64), ("max", np.float64),
    ("sum_tail", np.float64), ("x_lo", np.float64), ("x_hi", np.float64),
])
assert STATS_DTYPE.itemsize == ctypes.sizeof(McpStats)

# one mcp_attr: an asset's parts of a portfolio's mean, CVaR and standard deviation, and the sums behind them (SPEC.md 5.9)
ATTR_DTYPE = np.dtype([("mean", np.float64), ("cvar", np.float64), ("vol", np.float64), ("sum", np.float64), ("sum_tail", np.float64),
                       ("sum_xc", np.float64)])
assert ATTR_DTYPE.itemsize == 48

# one mcp_pair: the pair statistics of a portfolio's antithetic sample (SPEC.md 5.10)
PAIR_DTYPE = np.dtype([("n_pairs", np.uint64), ("reserved", np.uint64), ("cross", np.float64), ("pair_cov", np.float64),
                       ("pair_corr", np.float64), ("mean_se", np.float64), ("mean_se_iid", np.float64)])
assert PAIR_DTYPE.itemsize == 56

RECORD_DTYPE = np.dtype([("n", np.float64), ("sum", np.float64), ("sumsq", np.float64), ("min", np.float64),
                         ("max", np.float64), ("below", np.float64), ("pivot", np.float64), ("pad", np.float64)])
# one moment partial of the path kernels' epilogue (csrc/mcp_stats_kernels.h: MomentPartial)
PARTIAL_DTYPE = np.dtype([("s1", np.float64), ("s2", np.float64), ("vmin", np.float32), ("vmax", np.float32), ("n", np.uint64)])
assert PARTIAL_DTYPE.itemsize == 32
QUANT_DTYPE = np.dtype([("x_lo", np.float64), ("x_hi", np.float64), ("var", np.float64), ("level2", np.float64),
                        ("n_tail", np.uint64), ("pad", np.uint64)])
RECORD_DOUBLES = RECORD_DTYPE.itemsize // 8

_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64
_int = ctypes.c_int
_PP = ctypes.POINTER(McpParams)

# every symbol include/mcport.h declares: (restype, argtypes)
SIGNATURES = {
    "mcp_abi_version": (_int, []),
    "mcp_device_count": (_int, []),
    "mcp_last_error": (ctypes.c_char_p, []),
    "mcp_ctx_create": (_int, [_int, ctypes.POINTER(_vp)]),
    "mcp_ctx_create_multi": (_int, [ctypes.POINTER(_int), _int, ctypes.POINTER(_vp)]),
    "mcp_ctx_device_count": (_int, [_vp]),
    "mcp_ctx_exchange_mode": (_int, [_vp]),
    "mcp_ctx_exchange_note": (ctypes.c_char_p, [_vp]),
    "mcp_ctx_set_terminal_budget": (_int, [_vp, ctypes.c_size_t]),
    "mcp_ctx_destroy": (None, [_vp]),
    "mcp_sweep_historical": (_int, [_vp, _int, _int, _int, _f64p, _f64p, _f64p, _f64p, ctypes.c_double, ctypes.c_double,
                                    _f64p, _f64p, _f64p, _f64p, _f64p]),
    "mcp_ws_bytes": (ctypes.c_size_t, [_int, _int, _u64]),
    "mcp_moment_slots": (_u64, [_int, _u64]),
    "mcp_pivots": (_int, [_PP, _f32p, _f32p, _f32p, _f64p]),
    "mcp_packed_len": (ctypes.c_size_t, [_int, _int]),
    "mcp_pack_params": (_int, [_int, _int, _f32p, _f32p, _f32p, _f32p, ctypes.c_size_t]),
    "mcp_launch_paths": (_int, [_PP, _vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _vp]),
    "mcp_launch_paths_drawdown": (_int, [_PP, _vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "mcp_launch_paths_horizons": (_int, [_PP, _vp, _vp, _u64, _u64, _u64, _vp, _u64, _int, _vp, _vp, _u64, _vp, _vp, _vp]),
    "mcp_bootstrap_pivots": (_int, [_PP, ctypes.POINTER(McpBootstrap), _f32p, _f64p]),
    "mcp_rebalance_pivots": (_int, [_PP, ctypes.POINTER(McpRebalance), _vp, ctypes.POINTER(McpBootstrap), _f32p, _f64p]),
    "mcp_filtered_pivots": (_int, [_PP, ctypes.POINTER(McpFiltered), _f32p, _f64p]),
    "mcp_jump_consts": (_int, [ctypes.POINTER(McpJumps), _int, _vp, _vp, ctypes.POINTER(ctypes.c_double), _vp]),
    "mcp_regime_consts": (_int, [ctypes.POINTER(McpRegimes), _vp, _vp]),
    "mcp_regime_pivots": (_int, [_PP, ctypes.POINTER(McpRegimes), _vp, _vp, _int, _vp, _vp, _vp]),
    "mcp_cashflow_pivots": (_int, [_PP, ctypes.POINTER(McpCashflow), _vp, ctypes.POINTER(McpBootstrap), _f32p, _f64p]),
    "mcp_glide_pivots": (_int, [_PP, ctypes.POINTER(McpGlide), ctypes.POINTER(McpCashflow), _vp, ctypes.POINTER(McpBootstrap), _vp, _int,
                                _vp, _vp, _vp]),
    "mcp_overlay_pivots": (_int, [_PP, ctypes.POINTER(McpOverlay), _f32p, _f32p, _f64p]),
    "mcp_percentile_rank_q": (_int, [_u64, ctypes.c_double, ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                                     ctypes.POINTER(ctypes.c_double)]),
    "mcp_percentile_rank": (_int, [_u64, ctypes.c_double, ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                                   ctypes.POINTER(ctypes.c_double)]),
    "mcp_launch_pass0": (_int, [_PP, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "mcp_launch_scan": (_int, [_PP, _int, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcp_launch_hist": (_int, [_PP, _int, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mcp_launch_final": (_int, [_PP, _u64, ctypes.c_double, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcp_launch_stats": (_int, [_PP, _int, _vp, _vp, _vp, _vp]),
    "mcp_launch_sum_u64": (_int, [ctypes.POINTER(_vp), _int, ctypes.c_size_t, _vp]),
    "mcp_stream_create": (_int, [_int, _int, ctypes.POINTER(_vp)]),
    "mcp_stream_destroy": (_int, [_vp]),
    "mcp_launch_normals": (_int, [_vp, _u64, _vp, _vp]),
    "mcp_icdf_table": (_int, [_f32p, ctypes.c_size_t]),
    "mcp_float_to_key": (ctypes.c_uint32, [ctypes.c_float]),
    "mcp_key_to_float": (ctypes.c_float, [ctypes.c_uint32]),
    "mcp_terminal_to_x": (ctypes.c_double, [_PP, ctypes.c_float]),
}

# The argument groups of the host entry points mcp_simulate*: the types each one stands for.  mu, chol and W have a second
# flavour, written `mu*`: an ndpointer, which takes the array itself.
ARG_GROUPS = {
    "ctx": [_vp], "prm": [_PP],
    "gl": [ctypes.POINTER(McpGlide)], "cf": [ctypes.POINTER(McpCashflow)], "rb": [ctypes.POINTER(McpRebalance)],
    "st": [ctypes.POINTER(McpStudentT)], "gv": [ctypes.POINTER(McpGarch)], "jp": [ctypes.POINTER(McpJumps)],
    "rs": [ctypes.POINTER(McpRegimes)], "ft": [ctypes.POINTER(McpFiltered)], "ov": [ctypes.POINTER(McpOverlay)],
    "bt": [ctypes.POINTER(McpBootstrap)], "pt": [ctypes.POINTER(McpProtect)],
    "sp": [ctypes.POINTER(McpSpending)], "wd": [_vp, _vp],     # withdrawn_out, wd_stats_out
    "life": [_vp, _vp, _vp, _int, _vp, _vp],              # life_out, life_hist_out, life_sum_out, n_life_levels, life_levels, life_q_out
    "tb": [ctypes.POINTER(McpBand)],
    "vt": [ctypes.POINTER(McpVolTarget)], "exposure": [_vp, _vp],     # exposure_out, exposure_stats_out
    "du": [ctypes.POINTER(McpDriftUncertainty)],
    # longest_out, current_out, longest_hist_out, current_hist_out, sums_out, n_uw_levels, uw_levels, q_out
    "uw": [_vp, _vp, _vp, _vp, _vp, _int, _vp, _vp],
    # trades_out, trade_hist_out, trade_sum_out, n_trade_levels, trade_levels, trade_q_out, turnover_out, turnover_stats_out
    "trades": [_vp, _vp, _vp, _int, _vp, _vp, _vp, _vp],
    "mu": [_vp], "chol": [_vp], "W": [_vp], "mu*": [_f32p], "chol*": [_f32p], "W*": [_f32p],
    "walk": [_u64, _u64, _u64],                           # seed, path_begin, n_paths
    "hz_in": [_int, _vp, _int, _vp],                      # n_horizons, horizons, n_levels, levels
    "out": [_vp, _vp],                                    # terminal_out, stats_out
    "dd": [_vp, _vp],                                     # mdd_out, dd_stats_out
    "hz_out": [_vp, _vp, _vp],                            # horizon_out, hz_stats_out, bands_out
    "counts": [_vp], "hz_counts": [_vp], "pairs": [_vp], "contrib": [_vp], "attr": [_vp], "attr_counts": [_vp],
}

# every mcp_simulate* entry point of include/mcport.h: its argument groups, in the header's order.  The one statement of that
# order on the Python side: SIGNATURES and Context._call (simulate.py) both follow it.
SIMULATE_ENTRIES = {
    "mcp_simulate": "ctx prm mu* chol* W* walk out",
    "mcp_simulate_drawdown": "ctx prm mu* chol* W* walk out dd",
    "mcp_simulate_horizons": "ctx prm mu* chol* W* walk hz_in out hz_out",
    "mcp_simulate_bootstrap": "ctx prm bt W* walk out",
    "mcp_simulate_bootstrap_horizons": "ctx prm bt W* walk hz_in out hz_out",
    "mcp_simulate_rebalanced": "ctx prm rb mu chol bt W* walk hz_in out hz_out",
    "mcp_simulate_student_t": "ctx prm st mu chol W walk hz_in out dd hz_out",
    "mcp_simulate_garch": "ctx prm gv st mu chol W walk hz_in out dd hz_out",
    "mcp_simulate_filtered": "ctx prm ft gv W walk hz_in out hz_out",
    "mcp_simulate_jumps": "ctx prm jp mu chol W walk hz_in out dd hz_out",
    "mcp_simulate_regimes": "ctx prm rs mu chol W walk hz_in out dd hz_out",
    "mcp_simulate_attribution": "ctx prm gv st mu chol W walk out contrib attr attr_counts",
    "mcp_simulate_antithetic": "ctx prm gv st mu chol W walk hz_in out dd hz_out pairs",
    "mcp_simulate_cashflow": "ctx prm cf mu chol bt st W walk hz_in out counts hz_out hz_counts",
    "mcp_simulate_glide": "ctx prm gl cf mu chol bt st W walk hz_in out counts hz_out hz_counts",
    "mcp_simulate_overlay": "ctx prm ov mu chol st W walk hz_in out dd hz_out",
}
SIMULATE_ENTRIES = {name: tuple(groups.split()) for name, groups in SIMULATE_ENTRIES.items()}
SIGNATURES.update((name, (_int, [t for g in groups for t in ARG_GROUPS[g]])) for name, groups in SIMULATE_ENTRIES.items())

# The entry points of the extension headers (include/mcport_protect.h), bound after SIGNATURES: SIGNATURES and SIMULATE_ENTRIES are
# include/mcport.h's alone.  EXTENSION_ENTRIES: the mcp_simulate* among them by argument groups, as SIMULATE_ENTRIES.
EXTENSION_ENTRIES = {
    "mcp_simulate_protected": "ctx prm pt gv st jp mu chol W walk hz_in out dd counts hz_out hz_counts",
}
EXTENSION_ENTRIES = {name: tuple(groups.split()) for name, groups in EXTENSION_ENTRIES.items()}
EXTENSION_SIGNATURES = {
    "mcp_protect_pivots": (_int, [_PP, ctypes.POINTER(McpProtect), _vp, _vp, _int, _vp, _vp, _vp]),
    "mcp_protect_floor": (_int, [ctypes.c_double, ctypes.c_double, _int, _vp]),
}
EXTENSION_SIGNATURES.update((name, (_int, [t for g in groups for t in ARG_GROUPS[g]])) for name, groups in EXTENSION_ENTRIES.items())

# The same pair of tables for include/mcport_spend.h: every extension header has its own, so that each header's test pins exactly
# the symbols that header declares.
SPEND_ENTRIES = {
    "mcp_simulate_spending": "ctx prm sp mu chol bt st W walk hz_in out counts hz_out hz_counts wd",
}
SPEND_ENTRIES = {name: tuple(groups.split()) for name, groups in SPEND_ENTRIES.items()}
SPEND_SIGNATURES = {
    "mcp_spending_pivots": (_int, [_PP, ctypes.POINTER(McpSpending), _vp, ctypes.POINTER(McpBootstrap), _vp, _int, _vp, _vp, _vp, _vp]),
    "mcp_spending_consts": (_int, [ctypes.POINTER(McpSpending), ctypes.c_double, _vp]),
}
SPEND_SIGNATURES.update((name, (_int, [t for g in groups for t in ARG_GROUPS[g]])) for name, groups in SPEND_ENTRIES.items())

# And for include/mcport_life.h (SPEC.md 4.17 / 5.17).
MCP_MAX_LIFE_STEPS = 1 << 20
LIFE_ENTRIES = {
    "mcp_simulate_lifetime": "ctx prm cf gl sp mu chol bt st W walk hz_in out counts hz_out hz_counts wd life",
}
LIFE_ENTRIES = {name: tuple(groups.split()) for name, groups in LIFE_ENTRIES.items()}
LIFE_SIGNATURES = {
    "mcp_lifetime_summary": (_int, [_vp, _int, _int, _vp, _vp, _vp]),
}
LIFE_SIGNATURES.update((name, (_int, [t for g in groups for t in ARG_GROUPS[g]])) for name, groups in LIFE_ENTRIES.items())

# And for include/mcport_band.h (SPEC.md 4.18 / 5.18).
BAND_ENTRIES = {
    "mcp_simulate_banded": "ctx prm tb mu chol bt W* walk hz_in out hz_out trades",
}
BAND_ENTRIES = {name: tuple(groups.split()) for name, groups in BAND_ENTRIES.items()}
BAND_SIGNATURES = {
    "mcp_band_reviews": (_int, [_PP, ctypes.POINTER(McpBand)]),
}
BAND_SIGNATURES.update((name, (_int, [t for g in groups for t in ARG_GROUPS[g]])) for name, groups in BAND_ENTRIES.items())

# And for include/mcport_voltarget.h (SPEC.md 4.19 / 5.19).
VOLTARGET_ENTRIES = {
    "mcp_simulate_vol_target": "ctx prm vt gv st jp mu chol W walk hz_in out dd exposure counts hz_out hz_counts",
}
VOLTARGET_ENTRIES = {name: tuple(groups.split()) for name, groups in VOLTARGET_ENTRIES.items()}
VOLTARGET_SIGNATURES = {
    "mcp_vol_target_pivots": (_int, [_PP, ctypes.POINTER(McpVolTarget), _vp, _vp, _vp, _int, _vp, _vp, _vp]),
    "mcp_vol_target_consts": (_int, [_PP, ctypes.POINTER(McpVolTarget), _vp, _vp, _vp]),
}
VOLTARGET_SIGNATURES.update((name, (_int, [t for g in groups for t in ARG_GROUPS[g]])) for name, groups in VOLTARGET_ENTRIES.items())

# And for include/mcport_underwater.h (SPEC.md 4.20 / 5.20).
UNDERWATER_ENTRIES = {
    "mcp_simulate_underwater": "ctx prm gv st jp mu chol W walk out dd uw",
}
UNDERWATER_ENTRIES = {name: tuple(groups.split()) for name, groups in UNDERWATER_ENTRIES.items()}
UNDERWATER_SIGNATURES = {}
UNDERWATER_SIGNATURES.update((name, (_int, [t for g in groups for t in ARG_GROUPS[g]])) for name, groups in UNDERWATER_ENTRIES.items())

# And for include/mcport_uncertain.h (SPEC.md 2.7 / 4.21 / 5.21).
UNCERTAIN_ENTRIES = {
    "mcp_simulate_uncertain": "ctx prm du cf mu chol W walk hz_in out dd counts hz_out hz_counts",
}
UNCERTAIN_ENTRIES = {name: tuple(groups.split()) for name, groups in UNCERTAIN_ENTRIES.items()}
UNCERTAIN_SIGNATURES = {}
UNCERTAIN_SIGNATURES.update((name, (_int, [t for g in groups for t in ARG_GROUPS[g]])) for name, groups in UNCERTAIN_ENTRIES.items())

# And for include/mcport_downside.h (SPEC.md 5.22): no mcp_simulate* among them -- the request arms a context and rides the next call.
class McpDownside(ctypes.Structure):
    """mcp_downside (include/mcport_downside.h): the threshold tau of SPEC.md 5.22, or use_rf != 0 for the call's rf."""
    _fields_ = [("tau", ctypes.c_double), ("use_rf", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# one mcp_downside_sums: the raw record of a row; one mcp_downside_stats: the finished record
DOWNSIDE_SUMS_DTYPE = np.dtype([("n", np.uint64), ("n_below", np.uint64), ("n_above", np.uint64), ("s1", np.float64), ("s2", np.float64),
                                ("s3", np.float64), ("s4", np.float64), ("b1", np.float64), ("b2", np.float64), ("l1", np.float64),
                                ("l2", np.float64), ("u1", np.float64)])
DOWNSIDE_STATS_DTYPE = np.dtype([(f, np.float64) for f in ("mean", "skewness", "excess_kurtosis", "downside_std", "sortino",
                                                           "downside_deviation", "sortino_target", "p_below", "mean_shortfall", "omega", "pivot")])
assert DOWNSIDE_SUMS_DTYPE.itemsize == 96 and DOWNSIDE_STATS_DTYPE.itemsize == 88
DOWNSIDE_SIGNATURES = {
    "mcp_downside_grid": (_u64, [_u64]),
    "mcp_downside_ws_bytes": (ctypes.c_size_t, [_int, _u64]),
    "mcp_downside_trip_n": (_u64, []),
    "mcp_launch_downside": (_int, [_PP, _vp, _u64, _u64, _int, _vp, ctypes.c_double, _vp, _vp, _vp]),
    "mcp_downside_finish": (_int, [_vp, ctypes.c_double, ctypes.c_double, _vp]),
    "mcp_ctx_request_downside": (_int, [_vp, ctypes.POINTER(McpDownside), _vp, _vp, _vp]),
}

# And for include/mcport_relative.h (SPEC.md 5.23): as the downside request, it arms a context and rides the next call.
class McpRelative(ctypes.Structure):
    """mcp_relative (include/mcport_relative.h): the benchmark's row of the call's W (SPEC.md 5.23)."""
    _fields_ = [("bench", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# one mcp_relative_sums: the raw record of a row against its benchmark; one mcp_relative_stats: the finished record
RELATIVE_SUMS_DTYPE = np.dtype([(f, np.uint64) for f in ("n", "n_under", "n_over", "n_up", "n_down")] +
                               [(f, np.float64) for f in ("e1", "e2", "k1", "b1", "k2", "b2", "kb", "u1", "u2", "up_k", "up_b", "down_k",
                                                          "down_b")])
RELATIVE_STATS_DTYPE = np.dtype([(f, np.float64) for f in ("active_mean", "tracking_error", "information_ratio", "p_under", "p_over",
                                                           "mean_underperformance", "relative_downside_deviation", "beta", "alpha",
                                                           "correlation", "up_capture", "down_capture", "pivot", "bench_pivot")])
assert RELATIVE_SUMS_DTYPE.itemsize == 144 and RELATIVE_STATS_DTYPE.itemsize == 112
RELATIVE_SIGNATURES = {
    "mcp_relative_grid": (_u64, [_u64]),
    "mcp_relative_ws_bytes": (ctypes.c_size_t, [_int, _u64]),
    "mcp_relative_trip_n": (_u64, []),
    "mcp_launch_relative": (_int, [_PP, _vp, _u64, _u64, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "mcp_relative_finish": (_int, [_vp, ctypes.c_double, ctypes.c_double, _vp]),
    "mcp_ctx_request_relative": (_int, [_vp, ctypes.POINTER(McpRelative), _vp, _vp, _vp, _vp, _vp]),
}

# And for include/mcport_sweep_perf.h (SPEC.md 5.24): the series statistics of the historical sweep's portfolios.
# one mcp_sweep_perf_sums: the raw record of a portfolio; one mcp_sweep_perf_stats: the finished record
SWEEP_PERF_SUMS_DTYPE = np.dtype([(f, np.int32) for f in ("n", "n_neg", "peak_row", "trough_row")] +
                                 [(f, np.float64) for f in ("S", "S_neg", "M2", "M2_neg", "prod", "mdd")])
SWEEP_PERF_STATS_DTYPE = np.dtype([(f, np.float64) for f in ("sharpe_ratio", "sortino_ratio", "annual_volatility", "annual_return",
                                                             "max_drawdown", "calmar")] +
                                  [(f, np.int32) for f in ("peak_row", "trough_row")])
assert SWEEP_PERF_SUMS_DTYPE.itemsize == 64 and SWEEP_PERF_STATS_DTYPE.itemsize == 56
SWEEP_PERF_SIGNATURES = {
    "mcp_sweep_historical_perf": (_int, [_vp, _int, _int, _int, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp, _vp]),
    "mcp_sweep_perf_finish": (_int, [_vp, ctypes.c_double, _vp]),
}

# And for include/mcport_sweep_boot.h (SPEC.md 5.25): the resampled historical sweep.
MCP_SWEEP_MAX_ROWS = 4096                 # mcport.h
MCP_SWEEP_MAX_REPLICATES = 4096
SWEEP_BOOT_SIGNATURES = {
    "mcp_sweep_resampled": (_int, [_vp, _int, _int, _int, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, _u64, _u64,
                                   _int, ctypes.c_double, _vp, _vp, _vp]),
    "mcp_sweep_boot_counts": (_int, [_u64, _u64, _int, _int, ctypes.c_double, _vp]),
}

_LIB = None


def build(force: bool = False, jobs: int = 8) -> str:
    """Compile libmcport.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, f"-j{jobs}"] + (["-B"] if force else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libmcport.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    return LIB_PATH


def _preload_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7, the same as /opt/rocm's).  If libmcport.so pulled in the system copy first, a later
    `import torch` would load a second runtime and find no GPU; so when torch is installed its copy is
    loaded first and libmcport.so's DT_NEEDED binds to it by SONAME."""
    if "torch" in sys.modules:
        return                                  # torch already brought its runtime
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def preload_rccl() -> None:
    """Multi-device contexts load librccl at run time (dlopen("librccl.so.1") inside libmcport.so).  When torch is
    installed its bundled librccl (built against the HIP runtime this process already uses) is loaded first, so the
    library's dlopen resolves to it by SONAME."""
    if os.environ.get("MCP_RCCL_LIB"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "librccl.so")
        if os.path.exists(cand):
            try:
                # default (RTLD_LOCAL) binding: the library's later dlopen("librccl.so.1") finds this copy by SONAME all the
                # same, and librccl's symbols stay out of the global scope -- promoted to RTLD_GLOBAL they interpose symbols of
                # a torch imported LATER in the same process, which then aborts at exit ("double free or corruption")
                ctypes.CDLL(cand)
            except OSError:
                pass


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        _preload_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C {CSRC} -j8` (or __graft_entry__.build()). "
                "There is no CPU fallback for the path engine.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in list(EXTENSION_SIGNATURES.items()) + list(SPEND_SIGNATURES.items()) + list(LIFE_SIGNATURES.items()) + \
                list(BAND_SIGNATURES.items()) + list(VOLTARGET_SIGNATURES.items()) + list(UNDERWATER_SIGNATURES.items()) + \
                list(UNCERTAIN_SIGNATURES.items()) + list(DOWNSIDE_SIGNATURES.items()) + list(RELATIVE_SIGNATURES.items()) + \
                list(SWEEP_PERF_SIGNATURES.items()) + list(SWEEP_BOOT_SIGNATURES.items()):
            fn = getattr(L, name)          # additive entry points, detected by symbol: a library without them is too old
            fn.restype = res
            fn.argtypes = args
        got = L.mcp_abi_version()
        if got != MCP_ABI_VERSION:
            raise ImportError(f"libmcport.so ABI {got} != binding ABI {MCP_ABI_VERSION}; rebuild")
        _LIB = L
    return _LIB


def check(rc: int) -> int:
    if rc < 0:
        raise McpError(f"libmcport error {rc}: {lib().mcp_last_error().decode('utf-8', 'replace')}")
    return rc


def ptr(a):
    """The void * of an array's data; None (NULL) for None."""
    return a.ctypes.data_as(_vp) if a is not None else None


def ref(x):
    """A ctypes struct by reference; None (NULL) for None."""
    return ctypes.byref(x) if x is not None else None


def make_params(n_assets, n_steps, n_portfolios, compounding="simple", v0=1.0, alpha=0.95, rf=0.0,
                native_math=False, fold=False, shard_portfolios=False) -> McpParams:
    if compounding not in MCP_COMPOUND:
        raise ValueError(f"compounding must be 'simple' or 'log', got {compounding!r}")
    return McpParams(int(n_assets), int(n_steps), int(n_portfolios), MCP_COMPOUND[compounding],
                     (MCP_FLAG_NATIVE_MATH if native_math else 0) | (MCP_FLAG_FOLD if fold else 0)
                     | (MCP_FLAG_SHARD_PORTFOLIOS if shard_portfolios else 0), 0,
                     float(v0), float(alpha), float(rf))


def pack_params(mu: np.ndarray, chol: np.ndarray, W: np.ndarray) -> np.ndarray:
    n = mu.shape[0]
    k = W.shape[0]
    out = np.zeros(lib().mcp_packed_len(n, k), np.float32)
    check(lib().mcp_pack_params(n, k, mu, chol, W, out, out.size))
    return out


def pivots(prm: McpParams, mu: np.ndarray, chol: np.ndarray, W: np.ndarray) -> np.ndarray:
    """[K] shifts of the moments (include/mcport.h: mcp_pivots): the analytic mean of x per portfolio, pure host arithmetic."""
    out = np.zeros(W.shape[0], np.float64)
    check(lib().mcp_pivots(ctypes.byref(prm), mu, chol, W, out))
    return out


def make_bootstrap(rows: np.ndarray, block: float) -> McpBootstrap:
    """mcp_bootstrap over a C-contiguous binary32 [R, N] array (the caller keeps `rows` alive for the call)."""
    if rows.dtype != np.float32 or rows.ndim != 2 or not rows.flags.c_contiguous:
        raise ValueError("bootstrap rows must be a C-contiguous float32 [R, N] array")
    return McpBootstrap(rows.ctypes.data_as(ctypes.c_void_p), int(rows.shape[0]), 0, float(block))


def make_filtered(mu: np.ndarray, resid: np.ndarray, shock: np.ndarray, block: float) -> McpFiltered:
    """mcp_filtered over C-contiguous binary32 arrays mu [N], resid [R, N], shock [R] (the caller keeps them alive for the call)."""
    for a, nd in ((mu, 1), (resid, 2), (shock, 1)):
        if a.dtype != np.float32 or a.ndim != nd or not a.flags.c_contiguous:
            raise ValueError("filtered mu [N], resid [R, N] and shock [R] must be C-contiguous float32 arrays")
    if resid.shape != (shock.shape[0], mu.shape[0]):
        raise ValueError(f"filtered resid has shape {resid.shape}, mu and shock want {(shock.shape[0], mu.shape[0])}")
    return McpFiltered(mu.ctypes.data_as(ctypes.c_void_p), resid.ctypes.data_as(ctypes.c_void_p), shock.ctypes.data_as(ctypes.c_void_p),
                       int(resid.shape[0]), 0, float(block))


def filtered_pivots(prm: McpParams, mu: np.ndarray, resid: np.ndarray, shock: np.ndarray, W: np.ndarray) -> np.ndarray:
    """[K] shifts of the moments of filtered paths (SPEC.md 5.11; include/mcport.h, mcp_filtered_pivots), pure host arithmetic."""
    out = np.zeros(W.shape[0], np.float64)
    mu, resid, shock = (np.ascontiguousarray(a, np.float32) for a in (mu, resid, shock))
    ft = make_filtered(mu, resid, shock, 1.0)
    check(lib().mcp_filtered_pivots(ctypes.byref(prm), ctypes.byref(ft), W, out))
    return out


def make_jumps(intensity: float, mean: float, std: float, loading: np.ndarray | None = None) -> McpJumps:
    """mcp_jumps; `loading` is None (all ones) or a C-contiguous binary32 [N] array (the caller keeps it alive for the call)."""
    if loading is not None and (loading.dtype != np.float32 or loading.ndim != 1 or not loading.flags.c_contiguous):
        raise ValueError("jump loadings must be a C-contiguous float32 [N] array")
    return McpJumps(float(intensity), float(mean), float(std), ptr(loading), 0)


def jump_consts(intensity: float, mean: float, std: float, loading=None, mu=None, n_assets: int | None = None):
    """(thr uint32 [8], mean_count, drift float32 [N] or None): the host constants of SPEC.md 2.5 (include/mcport.h,
    mcp_jump_consts), pure host arithmetic.  `mu` [N]: also the compensated drift."""
    ld = np.ascontiguousarray(loading, np.float32) if loading is not None else None
    mu32 = np.ascontiguousarray(mu, np.float32) if mu is not None else None
    n = mu32.size if mu32 is not None else ld.size if ld is not None else int(n_assets or 1)
    thr = np.zeros(MCP_MAX_JUMPS, np.uint32)
    mean_count = ctypes.c_double()
    drift = np.zeros(n, np.float32) if mu32 is not None else None
    jp = make_jumps(intensity, mean, std, ld)
    check(lib().mcp_jump_consts(ctypes.byref(jp), n, ptr(mu32), ptr(thr), ctypes.byref(mean_count), ptr(drift)))
    return thr, mean_count.value, drift


def make_regimes(p01: float, p10: float, start: float, mu1: np.ndarray | None, chol1: np.ndarray | None) -> McpRegimes:
    """mcp_regimes; `mu1` [N] and `chol1` [N, N] are C-contiguous binary32 arrays (the caller keeps them alive for the call)."""
    for a, nd in ((mu1, 1), (chol1, 2)):
        if a is not None and (a.dtype != np.float32 or a.ndim != nd or not a.flags.c_contiguous):
            raise ValueError("regime mu1 [N] and chol1 [N, N] must be C-contiguous float32 arrays")
    return McpRegimes(float(p01), float(p10), float(start), ptr(mu1), ptr(chol1), 0)


def regime_consts(p01: float, p10: float, start: float):
    """(thr uint64 [3], p float64 [3]) for (p01, p10, start): the thresholds of SPEC.md 2.6 and the probabilities the kernel really
    uses (include/mcport.h, mcp_regime_consts), pure host arithmetic."""
    thr, p = np.zeros(3, np.uint64), np.zeros(3, np.float64)
    rs = make_regimes(p01, p10, start, None, None)
    check(lib().mcp_regime_consts(ctypes.byref(rs), ptr(thr), ptr(p)))
    return thr, p


def regime_pivots(prm: McpParams, regimes, mu: np.ndarray, mu1: np.ndarray, W: np.ndarray, horizons=None):
    """([K] pivots at n_steps, [H, K] at the horizons or None): the exact means of SPEC.md 5.13 (include/mcport.h, mcp_regime_pivots),
    pure host arithmetic.  `regimes` is (p01, p10, start)."""
    mu, mu1 = (np.ascontiguousarray(a, np.float32) for a in (mu, mu1))
    W = np.ascontiguousarray(W, np.float32)
    n = mu.size
    chol1 = np.zeros((n, n), np.float32)                  # not read by the pivots; the rules want a pointer
    rs = make_regimes(*regimes, mu1, chol1)
    hz = np.ascontiguousarray(horizons, np.int32) if horizons is not None and len(horizons) else None
    out = np.zeros(W.shape[0], np.float64)
    hout = np.zeros((hz.size, W.shape[0]), np.float64) if hz is not None else None
    check(lib().mcp_regime_pivots(ctypes.byref(prm), ctypes.byref(rs), ptr(mu), ptr(W), 0 if hz is None else hz.size, ptr(hz), ptr(out),
                                  ptr(hout)))
    return out, hout


def bootstrap_pivots(prm: McpParams, rows: np.ndarray, W: np.ndarray, block: float = 1.0) -> np.ndarray:
    """[K] shifts of the moments of bootstrap paths (SPEC.md 5.3; include/mcport.h, mcp_bootstrap_pivots), pure host arithmetic."""
    out = np.zeros(W.shape[0], np.float64)
    rows = np.ascontiguousarray(rows, np.float32)
    bt = make_bootstrap(rows, block)
    check(lib().mcp_bootstrap_pivots(ctypes.byref(prm), ctypes.byref(bt), W, out))
    return out


def rebalance_pivots(prm: McpParams, period: int, W: np.ndarray, mu: np.ndarray | None = None, rows: np.ndarray | None = None,
                     cost: float = 0.0) -> np.ndarray:
    """[K] shifts of the moments of rebalanced paths (SPEC.md 5.4; include/mcport.h, mcp_rebalance_pivots), pure host arithmetic:
    pass the drift `mu` (Gaussian draws) or the binary32 [R, N] `rows` (bootstrap draws)."""
    out = np.zeros(W.shape[0], np.float64)
    rb = McpRebalance(int(period), 0, float(cost))
    mu_p = np.ascontiguousarray(mu, np.float32) if mu is not None else None
    bt = make_bootstrap(np.ascontiguousarray(rows, np.float32), 1.0) if rows is not None else None
    check(lib().mcp_rebalance_pivots(ctypes.byref(prm), ctypes.byref(rb), ptr(mu_p), ref(bt), W, out))
    return out


def make_cashflow(flows: np.ndarray, target=None) -> McpCashflow:
    """mcp_cashflow over a C-contiguous binary32 [T] array (the caller keeps `flows` alive for the call)."""
    if flows.dtype != np.float32 or flows.ndim != 1 or not flows.flags.c_contiguous:
        raise ValueError("cash flows must be a C-contiguous float32 [n_steps] array")
    return McpCashflow(flows.ctypes.data_as(ctypes.c_void_p) if flows.size else None, int(flows.size), 0 if target is None else 1,
                       0.0 if target is None else float(target))


def cashflow_pivots(prm: McpParams, flows: np.ndarray, W: np.ndarray, mu: np.ndarray | None = None,
                    rows: np.ndarray | None = None) -> np.ndarray:
    """[K] shifts of the moments of paths with cash flows (SPEC.md 5.6; include/mcport.h, mcp_cashflow_pivots), pure host
    arithmetic: pass the drift `mu` (Gaussian and Student-t draws) or the binary32 [R, N] `rows` (bootstrap draws)."""
    out = np.zeros(W.shape[0], np.float64)
    flows = np.ascontiguousarray(flows, np.float32)
    cf = make_cashflow(flows)
    mu_p = np.ascontiguousarray(mu, np.float32) if mu is not None else None
    bt = make_bootstrap(np.ascontiguousarray(rows, np.float32), 1.0) if rows is not None else None
    check(lib().mcp_cashflow_pivots(ctypes.byref(prm), ctypes.byref(cf), ptr(mu_p), ref(bt), W, out))
    return out


def make_glide(breaks: np.ndarray, targets: np.ndarray) -> McpGlide:
    """mcp_glide over C-contiguous arrays, breaks int32 [G] and targets binary32 [G, K, N] (the caller keeps them alive for the call)."""
    if breaks.dtype != np.int32 or breaks.ndim != 1 or not breaks.flags.c_contiguous:
        raise ValueError("glide breaks must be a C-contiguous int32 [G] array")
    if targets.dtype != np.float32 or targets.ndim != 3 or targets.shape[0] != breaks.size or not targets.flags.c_contiguous:
        raise ValueError("glide targets must be a C-contiguous float32 [G, K, N] array")
    G = int(breaks.size)
    return McpGlide(breaks.ctypes.data_as(ctypes.c_void_p) if G else None, targets.ctypes.data_as(ctypes.c_void_p) if G else None, G, 0)


def glide_pivots(prm: McpParams, breaks, targets, W: np.ndarray, flows=None, mu: np.ndarray | None = None,
                 rows: np.ndarray | None = None, horizons=None):
    """([K] pivots at n_steps, [H, K] at the horizons or None): the shifts of the moments of a glide path (SPEC.md 5.14;
    include/mcport.h, mcp_glide_pivots), pure host arithmetic.  breaks [G], targets [G, K, N]; flows None: no cash flows; pass the
    drift `mu` (Gaussian and Student-t draws) or the binary32 [R, N] `rows` (bootstrap draws)."""
    W = np.ascontiguousarray(W, np.float32)
    breaks = np.ascontiguousarray(breaks, np.int32).ravel()
    targets = np.ascontiguousarray(targets, np.float32).reshape(breaks.size, W.shape[0], W.shape[1])
    gl = make_glide(breaks, targets)
    fl = np.ascontiguousarray(flows, np.float32) if flows is not None else None
    cf = make_cashflow(fl) if fl is not None else None
    mu_p = np.ascontiguousarray(mu, np.float32) if mu is not None else None
    bt = make_bootstrap(np.ascontiguousarray(rows, np.float32), 1.0) if rows is not None else None
    hz = np.ascontiguousarray(horizons, np.int32) if horizons is not None and len(horizons) else None
    out = np.zeros(W.shape[0], np.float64)
    hout = np.zeros((hz.size, W.shape[0]), np.float64) if hz is not None else None
    check(lib().mcp_glide_pivots(ctypes.byref(prm), ctypes.byref(gl), ref(cf), ptr(mu_p), ref(bt), ptr(W),
                                 0 if hz is None else hz.size, ptr(hz), ptr(out), ptr(hout)))
    return out, hout


def make_protect(floor: np.ndarray, multiplier: float, rate: float = 0.0, cap: float = 1.0, ratchet: float = 0.0, target=None) -> McpProtect:
    """mcp_protect over a C-contiguous binary32 [n_steps + 1] floor schedule (the caller keeps it alive for the call); the target,
    when given, lives in a one-element array kept on the struct."""
    if floor.dtype != np.float32 or floor.ndim != 1 or not floor.flags.c_contiguous:
        raise ValueError("the protect floor must be a C-contiguous float32 [n_steps + 1] array")
    tg = np.array([float(target)], np.float64) if target is not None else None
    pt = McpProtect(ptr(floor), float(multiplier), float(cap), float(rate), float(ratchet), ptr(tg), 0)
    pt._keep = (floor, tg)
    return pt


def protect_floor(floor0: float, rate: float, n_steps: int) -> np.ndarray:
    """binary32 [n_steps + 1]: S_0 = fl32(floor0), S_{t+1} = fma(S_t, fl32(rate), S_t) (include/mcport_protect.h, mcp_protect_floor)."""
    out = np.zeros(int(n_steps) + 1 if int(n_steps) >= 0 else 0, np.float32)
    check(lib().mcp_protect_floor(float(floor0), float(rate), int(n_steps), ptr(out)))
    return out


def protect_pivots(prm: McpParams, protect: McpProtect, mu: np.ndarray, W: np.ndarray, horizons=None):
    """([K] pivots at n_steps, [H, K] at the horizons or None): the shifts of the moments of protected paths (SPEC.md 5.15;
    include/mcport_protect.h, mcp_protect_pivots), pure host arithmetic."""
    W = np.ascontiguousarray(W, np.float32)
    mu32 = np.ascontiguousarray(mu, np.float32)
    hz = np.ascontiguousarray(horizons, np.int32) if horizons is not None and len(horizons) else None
    out = np.zeros(W.shape[0], np.float64)
    hout = np.zeros((hz.size, W.shape[0]), np.float64) if hz is not None else None
    check(lib().mcp_protect_pivots(ctypes.byref(prm), ctypes.byref(protect), ptr(mu32), ptr(W), 0 if hz is None else hz.size, ptr(hz),
                                   ptr(out), ptr(hout)))
    return out, hout


def make_spending(rate: float, every: int, down: float, up: float, inflation: float = 0.0, first=None, target=None) -> McpSpending:
    """mcp_spending of the spending rule of SPEC.md 4.16 (include/mcport_spend.h); first None: w0 = fl32(p32 fl32(v0)); target None:
    no second count."""
    return McpSpending(float(rate), float(down), float(up), float(inflation), 0.0 if first is None else float(first),
                       0.0 if target is None else float(target), int(every), int(first is not None), int(target is not None), 0)


def spending_consts(spending: McpSpending, v0: float) -> np.ndarray:
    """binary32 [5] {p32, g32, lo32, hi32, w0}: the constants of the rule as the walk uses them (include/mcport_spend.h,
    mcp_spending_consts), pure host arithmetic."""
    out = np.zeros(5, np.float32)
    check(lib().mcp_spending_consts(ctypes.byref(spending), float(v0), ptr(out)))
    return out


def spending_pivots(prm: McpParams, spending: McpSpending, W: np.ndarray, mu: np.ndarray | None = None, rows: np.ndarray | None = None,
                    horizons=None):
    """([K] pivots of V at n_steps, [H, K] at the horizons or None, [K] pivots of the total paid out): the spending rule on the mean
    path (SPEC.md 5.16; include/mcport_spend.h, mcp_spending_pivots), pure host arithmetic.  Pass the drift `mu` (Gaussian and
    Student-t draws) or the binary32 [R, N] `rows` (bootstrap draws)."""
    W = np.ascontiguousarray(W, np.float32)
    mu_p = np.ascontiguousarray(mu, np.float32) if mu is not None else None
    bt = make_bootstrap(np.ascontiguousarray(rows, np.float32), 1.0) if rows is not None else None
    hz = np.ascontiguousarray(horizons, np.int32) if horizons is not None and len(horizons) else None
    out = np.zeros(W.shape[0], np.float64)
    wout = np.zeros(W.shape[0], np.float64)
    hout = np.zeros((hz.size, W.shape[0]), np.float64) if hz is not None else None
    check(lib().mcp_spending_pivots(ctypes.byref(prm), ctypes.byref(spending), ptr(mu_p), ref(bt), ptr(W), 0 if hz is None else hz.size,
                                    ptr(hz), ptr(out), ptr(hout), ptr(wout)))
    return out, hout, wout


def lifetime_summary(hist, levels=()):
    """(life_sum, uint32 [L] order statistics at the ranks `lo` of mcp_percentile_rank_q) of one lifetime histogram hist[0 .. T]
    (SPEC.md 5.17; include/mcport_life.h, mcp_lifetime_summary), pure host arithmetic."""
    h = np.ascontiguousarray(hist, np.uint64).ravel()
    lv = np.ascontiguousarray(levels, np.float64).ravel()
    total = np.zeros(1, np.uint64)
    q = np.zeros(lv.size, np.uint32)
    check(lib().mcp_lifetime_summary(ptr(h), h.size - 1, lv.size, ptr(lv) if lv.size else None, ptr(total), ptr(q) if lv.size else None))
    return int(total[0]), q


def make_band(every: int, cost: float, tol: np.ndarray) -> McpBand:
    """mcp_band over the C-contiguous float32 [K, N] table `tol` (the caller keeps it alive for the call)."""
    return McpBand(int(every), 0, float(cost), ptr(tol))


def band_reviews(n_steps: int, every: int) -> int:
    """n_reviews of SPEC.md 4.18 (include/mcport_band.h, mcp_band_reviews), pure host arithmetic."""
    n = lib().mcp_band_reviews(ctypes.byref(McpParams(n_steps=int(n_steps))), ctypes.byref(McpBand(int(every), 0, 0.0, None)))
    return check(n)


def make_drift_uncertainty(factor: np.ndarray) -> McpDriftUncertainty:
    """mcp_drift_uncertainty over the binary32 factor M [N, N] of SPEC.md 4.21 (include/mcport_uncertain.h); the array is kept on the
    struct."""
    m = np.ascontiguousarray(factor, np.float32)
    du = McpDriftUncertainty(m.ctypes.data, 0)
    du._keep = m
    return du


def downside_finish(sums, tau: float, pivot: float):
    """One finished record (a DOWNSIDE_STATS_DTYPE scalar) of one raw record `sums` (a DOWNSIDE_SUMS_DTYPE scalar or 0-d array):
    SPEC.md 5.22 (include/mcport_downside.h, mcp_downside_finish), pure host arithmetic."""
    s = np.array(sums, DOWNSIDE_SUMS_DTYPE).reshape(1)
    out = np.zeros(1, DOWNSIDE_STATS_DTYPE)
    check(lib().mcp_downside_finish(ptr(s), float(tau), float(pivot), ptr(out)))
    return out[0]


def relative_finish(sums, pivot: float, bench_pivot: float):
    """One finished record (a RELATIVE_STATS_DTYPE scalar) of one raw record `sums` (a RELATIVE_SUMS_DTYPE scalar or 0-d array) about
    the row's and the benchmark's pivots: SPEC.md 5.23 (include/mcport_relative.h, mcp_relative_finish), pure host arithmetic."""
    s = np.array(sums, RELATIVE_SUMS_DTYPE).reshape(1)
    out = np.zeros(1, RELATIVE_STATS_DTYPE)
    check(lib().mcp_relative_finish(ptr(s), float(pivot), float(bench_pivot), ptr(out)))
    return out[0]


def make_vol_target(target: float, decay: float, cap: float = 1.0, rate: float = 0.0, spread: float = 0.0, s0=None,
                    target_value=None) -> McpVolTarget:
    """mcp_vol_target of the rule of SPEC.md 4.19 (include/mcport_voltarget.h); s0 None: the default of the Gaussian part; the arrays
    behind the two pointers are kept on the struct."""
    s0a = np.ascontiguousarray(s0, np.float64).ravel() if s0 is not None else None
    tg = np.array([float(target_value)], np.float64) if target_value is not None else None
    vt = McpVolTarget(float(target), float(decay), float(cap), float(rate), float(spread), ptr(s0a), ptr(tg), 0)
    vt._keep = (s0a, tg)
    return vt


def vol_target_consts(prm: McpParams, vol_target: McpVolTarget, chol: np.ndarray | None, W: np.ndarray | None):
    """(binary32 [6] {tgt, lam, oml, b, rf, sp}, binary32 [K] s0): the constants of the rule as the walk uses them
    (include/mcport_voltarget.h, mcp_vol_target_consts), pure host arithmetic."""
    chol32 = np.ascontiguousarray(chol, np.float32) if chol is not None else None
    W32 = np.ascontiguousarray(W, np.float32) if W is not None else None
    out = np.zeros(6 + max(int(prm.n_portfolios), 0), np.float32)
    check(lib().mcp_vol_target_consts(ctypes.byref(prm), ref(vol_target), ptr(chol32), ptr(W32), ptr(out)))
    return out[:6].copy(), out[6:].copy()


def vol_target_pivots(prm: McpParams, vol_target: McpVolTarget, mu: np.ndarray, chol: np.ndarray, W: np.ndarray, horizons=None):
    """([K] pivots at n_steps, [H, K] at the horizons or None): the shifts of the moments of volatility-targeted paths (SPEC.md 5.19;
    include/mcport_voltarget.h, mcp_vol_target_pivots), pure host arithmetic."""
    W = np.ascontiguousarray(W, np.float32)
    mu32 = np.ascontiguousarray(mu, np.float32)
    chol32 = np.ascontiguousarray(chol, np.float32)
    hz = np.ascontiguousarray(horizons, np.int32) if horizons is not None and len(horizons) else None
    out = np.zeros(W.shape[0], np.float64)
    hout = np.zeros((hz.size, W.shape[0]), np.float64) if hz is not None else None
    check(lib().mcp_vol_target_pivots(ctypes.byref(prm), ref(vol_target), ptr(mu32), ptr(chol32), ptr(W), 0 if hz is None else hz.size,
                                      ptr(hz), ptr(out), ptr(hout)))
    return out, hout


def make_overlay(rows: np.ndarray, row_begin: np.ndarray, spot: np.ndarray) -> McpOverlay:
    """mcp_overlay over C-contiguous arrays (rows of OVERLAY_ROW_DTYPE, row_begin int32 [N + 1], spot float32 [N]; the caller keeps
    them alive for the call)."""
    if rows.dtype != OVERLAY_ROW_DTYPE or rows.ndim != 1 or not rows.flags.c_contiguous:
        raise ValueError("overlay rows must be a C-contiguous [n_rows] array of OVERLAY_ROW_DTYPE")
    if row_begin.dtype != np.int32 or spot.dtype != np.float32 or row_begin.ndim != 1 or spot.ndim != 1 or row_begin.size != spot.size + 1:
        raise ValueError("overlay row_begin must be int32 [N + 1] and spot float32 [N]")
    return McpOverlay(rows.ctypes.data_as(ctypes.c_void_p) if rows.size else None, row_begin.ctypes.data_as(ctypes.c_void_p),
                      spot.ctypes.data_as(ctypes.c_void_p), int(rows.size), 0)


def overlay_pivots(prm: McpParams, overlay, mu: np.ndarray, W: np.ndarray) -> np.ndarray:
    """[K] shifts of the moments of overlaid paths (SPEC.md 5.7; include/mcport.h, mcp_overlay_pivots), pure host arithmetic:
    `overlay` is the (rows, row_begin, spot) triple of simulate.check_overlay."""
    out = np.zeros(W.shape[0], np.float64)
    ov = make_overlay(*overlay)
    check(lib().mcp_overlay_pivots(ctypes.byref(prm), ctypes.byref(ov), np.ascontiguousarray(mu, np.float32), W, out))
    return out


def percentile_rank_q(n_total: int, q: float):
    """(rank_lo, rank_hi, gamma) of np.percentile(x, q) over n_total values, q in percent (include/mcport.h)."""
    lo, hi, g = _u64(), _u64(), ctypes.c_double()
    check(lib().mcp_percentile_rank_q(n_total, q, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(g)))
    return lo.value, hi.value, g.value


def percentile_rank(n_total: int, alpha: float):
    lo, hi, g = _u64(), _u64(), ctypes.c_double()
    check(lib().mcp_percentile_rank(n_total, alpha, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(g)))
    return lo.value, hi.value, g.value

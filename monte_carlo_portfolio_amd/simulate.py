"""simulate_paths: the Monte Carlo path simulator behind the Streamlit-shaped surface.

Replaces, for a *simulated* terminal-value distribution, what the reference computes per portfolio
on *historical* returns at app.py:708-713 (portfolio mean/vol, Sharpe, 5 % VaR, CVaR).  Inputs are
the same objects the reference builds at app.py:679-680 (mean vector, covariance matrix), here per
step.  All arithmetic on the path happens in libmcport.so's HIP kernels (SPEC.md); this module only
validates, factors Sigma (float64 Cholesky on the host, cast to fp32) and marshals arrays.
"""
from __future__ import annotations

import atexit
import collections
import ctypes
import threading

import numpy as np

from . import _ffi

_CTX_LOCK = threading.Lock()
_CTX: dict[tuple, "Context"] = {}


# Which mcp_simulate* entry point a call of Context._call takes: the first row whose keywords are all given.  Last in a row, the
# sentence that refuses a keyword the entry point has no argument group for (None: a plain one naming the entry point and the
# keyword).  A new feature adds its row here, its groups to _ffi.SIMULATE_ENTRIES and its keyword to _KEYWORD_GROUP.
_ENTRY_CHOICE = (
    (("spending",), "mcp_simulate_spending", "spending is not combined with cashflow, glide, protect, drawdown, rebalance, overlay, garch, "
                                             "jumps, regimes, filtered rows, attribution or antithetic"),
    (("protect",), "mcp_simulate_protected", "protect is not combined with overlay, cashflow, rebalance, bootstrap or filtered rows, regimes, "
                                             "glide, attribution or antithetic"),
    (("glide",), "mcp_simulate_glide", "glide is not combined with drawdown, rebalance, overlay, garch, attribution, antithetic, jumps, "
                                       "regimes or filtered rows"),
    (("filtered",), "mcp_simulate_filtered", "filtered rows take garch, block and horizons only"),
    (("regimes",), "mcp_simulate_regimes", "regimes are not combined with overlay, cashflow, rebalance, bootstrap rows, dof, garch, jumps, "
                                           "attribution or antithetic"),
    (("jumps",), "mcp_simulate_jumps", "jumps are not combined with overlay, cashflow, rebalance, bootstrap rows, dof, garch, attribution "
                                       "or antithetic"),
    (("antithetic",), "mcp_simulate_antithetic", "antithetic pairs are not combined with overlay, cashflow, rebalance, bootstrap rows or "
                                                 "attribution"),
    (("attribution",), "mcp_simulate_attribution", "attribution is not combined with overlay, cashflow, rebalance, bootstrap rows, "
                                                   "horizons or drawdown"),
    (("garch",), "mcp_simulate_garch", None),
    (("overlay",), "mcp_simulate_overlay", None),
    (("flows",), "mcp_simulate_cashflow", None),
    (("dof",), "mcp_simulate_student_t", None),
    (("period",), "mcp_simulate_rebalanced", None),
    (("rows", "horizons"), "mcp_simulate_bootstrap_horizons", None),
    (("rows",), "mcp_simulate_bootstrap", None),
    (("horizons",), "mcp_simulate_horizons", None),
    (("drawdown",), "mcp_simulate_drawdown", None),
    ((), "mcp_simulate", None),
)
# The lifetime (SPEC.md 4.17) is an opt-in on three of those calls, not a feature of its own: with it the call takes this entry point,
# whatever the table above would choose, and a keyword that entry point has no argument group for is refused with this sentence.
_LIFE_CHOICE = ("mcp_simulate_lifetime", "lifetime is not combined with protect, drawdown, rebalance, overlay, garch, jumps, regimes, "
                                         "filtered rows, attribution or antithetic")
# Tolerance bands (SPEC.md 4.18) take the rebalancing rule's place: with `tolerance` the call takes this entry point, whatever the table
# above would choose, and a keyword that entry point has no argument group for is refused with this sentence.  (It is not the first
# row of _ENTRY_CHOICE: tests/test_spend_cpu.py pins that row.)
_BAND_CHOICE = ("mcp_simulate_banded", "tolerance is not combined with drawdown, cashflow, glide, protect, spending, overlay, dof, garch, "
                                       "jumps, regimes, filtered rows, attribution or antithetic")
# Volatility targeting (SPEC.md 4.19) is a rule in the update of V on the Gaussian, Student-t, GARCH and jump walks: with `vol_target` the
# call takes this entry point, whatever the table above would choose, and a keyword that entry point has no argument group for is
# refused with this sentence.
_VOLTARGET_CHOICE = ("mcp_simulate_vol_target", "vol_target is not combined with overlay, cashflow, rebalance, bootstrap or filtered rows, "
                                                "regimes, glide, protect, spending, lifetime, tolerance, attribution or antithetic")
# The time under water (SPEC.md 4.20) is an opt-in on the drawdown walk of the Gaussian, Student-t, GARCH and jump calls, not a feature of
# its own: with `underwater` the call takes this entry point, whatever the table above would choose, and a keyword that entry point
# has no argument group for is refused with this sentence.
_UNDERWATER_CHOICE = ("mcp_simulate_underwater", "underwater is not combined with horizons, overlay, cashflow, rebalance, bootstrap or "
                                                 "filtered rows, regimes, glide, protect, spending, lifetime, tolerance, vol_target, "
                                                 "attribution or antithetic")
# Drift uncertainty (SPEC.md 2.7 / 4.21) is a per-path drift on the Gaussian walk, its drawdown, its horizons and its cash flows: with
# `drift_uncertainty` the call takes this entry point, whatever the table above would choose, and a keyword that entry point has no
# argument group for is refused with this sentence.
_UNCERTAIN_CHOICE = ("mcp_simulate_uncertain", "drift_uncertainty is not combined with dof, garch, jumps, regimes, overlay, rebalance, "
                                               "bootstrap or filtered rows, glide, protect, spending, lifetime, tolerance, vol_target, "
                                               "underwater, attribution or antithetic")
# the argument group of _ffi.SIMULATE_ENTRIES that carries each feature keyword of Context._call
_KEYWORD_GROUP = {"rows": "bt", "dof": "st", "period": "rb", "drawdown": "dd", "horizons": "hz_in", "flows": "cf", "overlay": "ov",
                  "garch": "gv", "attribution": "attr", "antithetic": "pairs", "filtered": "ft", "jumps": "jp", "regimes": "rs",
                  "glide": "gl", "protect": "pt", "spending": "sp", "lifetime": "life", "tolerance": "tb", "vol_target": "vt", "underwater": "uw",
                  "drift_uncertainty": "du",
                  # SPEC.md 5.22: no argument of an entry point -- the request arms the context, which every entry point takes
                  "downside": "ctx"}


class Context:
    """Owns one mcp_ctx: device buffers + one stream per device.  `device` is a device index or a sequence of them
    (one context over several GPUs, exchanging through RCCL inside the library; a device listed
    more than once holds several logical shards).  Calls are serialised by the library."""

    def __init__(self, device=0, terminal_budget: int | None = None):
        devs = [int(device)] if np.isscalar(device) else [int(d) for d in device]
        self._h = ctypes.c_void_p()
        if len(devs) > 1 and len(set(devs)) == len(devs):
            _ffi.preload_rccl()
        arr = (ctypes.c_int * len(devs))(*devs)
        _ffi.check(_ffi.lib().mcp_ctx_create_multi(arr, len(devs), ctypes.byref(self._h)))
        self.device = devs[0]
        self.devices = tuple(devs)
        if terminal_budget is not None:
            self.set_terminal_budget(terminal_budget)

    def set_terminal_budget(self, nbytes: int):
        """Upper bound on resident terminal values per device; larger sweeps are produced and reduced in tiles of
        portfolios (include/mcport.h, mcp_ctx_set_terminal_budget)."""
        _ffi.check(_ffi.lib().mcp_ctx_set_terminal_budget(self._h, int(nbytes)))

    def exchange(self):
        """(mode, note): how the shards of this context exchange histograms and records -- 'unset' before the first
        path-sharded call, then 'none' (one shard), 'rccl', 'kernel' (logical shards of one device) or 'p2p' (distinct devices
        without RCCL: the kernel over peer access; `note` then says why RCCL was not used)."""
        lib = _ffi.lib()
        names = {_ffi.EXCHANGE_UNSET: "unset", _ffi.EXCHANGE_NONE: "none", _ffi.EXCHANGE_RCCL: "rccl", _ffi.EXCHANGE_KERNEL: "kernel",
                 _ffi.EXCHANGE_P2P: "p2p"}
        return names[lib.mcp_ctx_exchange_mode(self._h)], lib.mcp_ctx_exchange_note(self._h).decode("utf-8", "replace")

    def close(self):
        if self._h:
            _ffi.lib().mcp_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, prm: _ffi.McpParams, W, seed: int, path_begin: int, n_paths: int, store: bool, mu=None, chol=None, rows=None,
              block: float = 1.0, dof=None, period=None, cost: float = 0.0, drawdown: bool = False, horizons=None, levels=(),
              flows=None, target=None, overlay=None, garch=None, attribution=False, antithetic=False, filtered=None, jumps=None, regimes=None,
              glide=None, protect=None, spending=None, lifetime=None, tolerance=None, vol_target=None, underwater=None,
              drift_uncertainty=None, downside=None, benchmark=None):
        """The one library call behind every simulate_* method: benchmark-relative statistics (benchmark: the row of W every portfolio is compared with, SPEC.md 5.23; a request on the context as downside is, with every keyword below), downside and shape statistics (downside: True for the threshold rf or the threshold tau, SPEC.md 5.22; the request arms the context and rides whatever call this is, so it combines with every keyword below), drift uncertainty (drift_uncertainty: the binary32 factor M [N, N] of uncertainty.drift_factor, SPEC.md 2.7 / 4.21; on Gaussian draws with the drawdown, horizons or flows), the time under water (underwater: the levels in percent of the two counters' order statistics, SPEC.md 4.20 / 5.20; needs `drawdown`), a volatility target (vol_target: the (target, decay, cap, rate, spread, s0 or None) of voltarget.check_vol_target, SPEC.md 4.19 / 5.19; `target` is then its second count, and without `drawdown` the call leaves the exposure record), tolerance bands (tolerance: (every, cost, tol float32 [K, N], levels in percent of the trade counts' order statistics), SPEC.md 4.18 / 5.18; the rule carries its own period and cost, so not with `period`), the lifetime (lifetime: the levels in percent of its order statistics, SPEC.md 4.17 / 5.17; needs flows or spending), a spending rule (spending: the (rate, every, down, up, inflation, first or None) of check_spending; `target` is then its second count), floor protection (protect: the (floor, multiplier, rate, cap, ratchet) of check_protect; `target` is then its second count), two regimes (regimes: the (p01, p10, start, mu1, chol1) of check_regimes), market jumps (jumps: the (intensity, mean, std, loading or None) of check_jumps), GARCH volatility (garch: the (alpha, beta, h0) of check_garch), an option overlay (overlay: the triple of check_overlay), cash flows (flows, target), Student-t draws (dof), rebalancing
        (period, cost), bootstrap rows (rows, block) or Gaussian draws (mu, chol), with the drawdown or horizons.  Allocates the
        outputs that were asked for and passes NULL for the rest -> _Outputs, None where not asked for (terminal, qd,
        horizon_terminal: with `store` only; counts, hz_counts: with `flows` only; attr [K, N] records of ATTR_DTYPE and attr_counts
        [K, 2] with `attribution` only, contributions [K, N, n_paths] with `store` on top; pairs [K] records of PAIR_DTYPE with
        `antithetic` only)."""
        K, N = prm.n_portfolios, prm.n_assets
        bt = _ffi.make_bootstrap(rows, block) if rows is not None else None
        given = [kw for kw, on in (("rows", rows is not None), ("dof", dof is not None), ("period", period is not None),
                                   ("drawdown", drawdown), ("horizons", horizons is not None), ("flows", flows is not None),
                                   ("overlay", overlay is not None), ("garch", garch is not None), ("attribution", attribution),
                                   ("antithetic", antithetic), ("filtered", filtered is not None), ("jumps", jumps is not None),
                                   ("regimes", regimes is not None), ("glide", glide is not None),
                                   ("protect", protect is not None), ("spending", spending is not None),
                                   ("lifetime", lifetime is not None), ("tolerance", tolerance is not None),
                                   ("vol_target", vol_target is not None), ("underwater", underwater is not None),
                                   ("drift_uncertainty", drift_uncertainty is not None), ("downside", downside is not None)) if on]
        has = set(given).issuperset
        entry, refusal = _UNCERTAIN_CHOICE if drift_uncertainty is not None else _UNDERWATER_CHOICE if underwater is not None else _BAND_CHOICE if tolerance is not None else _LIFE_CHOICE if lifetime is not None else _VOLTARGET_CHOICE if vol_target is not None else next((e, r) for needs, e, r in _ENTRY_CHOICE if has(needs))
        groups = next(t[entry] for t in (_ffi.SIMULATE_ENTRIES, _ffi.EXTENSION_ENTRIES, _ffi.SPEND_ENTRIES, _ffi.LIFE_ENTRIES,
                                            _ffi.BAND_ENTRIES, _ffi.VOLTARGET_ENTRIES, _ffi.UNDERWATER_ENTRIES, _ffi.UNCERTAIN_ENTRIES)
                      if entry in t)
        # the library states the rules (check_request); a keyword the entry point has no argument for is refused here, not dropped
        for kw in given:
            if _KEYWORD_GROUP[kw] not in groups:
                raise ValueError(refusal or f"{entry} has no argument for {kw}")
        if underwater is not None and not drawdown:            # SPEC.md 4.20: the counters ride the drawdown walk
            raise ValueError("underwater needs drawdown")
        if filtered is not None and garch is None:             # SPEC.md 4.11: the one keyword an entry point cannot do without
            raise ValueError(refusal)
        stats = np.zeros(K, _ffi.STATS_DTYPE)
        term = np.empty((K, n_paths), np.float32) if store else None
        dd_stats = raw = hz_stats = bands = hz_term = steps = lv = None
        H = L = 0
        if drawdown:
            dd_stats = np.zeros(K, _ffi.STATS_DTYPE)
            raw = np.empty((K, n_paths), np.float32) if store else None
        if horizons is not None:
            steps = np.ascontiguousarray(horizons, np.int32).ravel()
            lv = np.ascontiguousarray(levels, np.float64).ravel()
            H, L = steps.size, lv.size
            hz_stats = np.zeros((H, K), _ffi.STATS_DTYPE)
            bands = np.zeros((H, K, L), np.float64)
            hz_term = np.empty((H, K, n_paths), np.float32) if store else None
        has_counts = "counts" in groups and not (drift_uncertainty is not None and flows is None)   # SPEC.md 4.21: the counts are the flows'
        counts = np.zeros((K, 2), np.uint64) if has_counts else None
        hz_counts = np.zeros((H, K, 2), np.uint64) if has_counts and "hz_counts" in groups and horizons is not None else None
        pairs = np.zeros(K, _ffi.PAIR_DTYPE) if "pairs" in groups else None
        attr = np.zeros((K, N), _ffi.ATTR_DTYPE) if "attr" in groups else None
        attr_counts = np.zeros((K, 2), np.uint64) if "attr_counts" in groups else None
        contrib = np.empty((K, N, n_paths), np.float32) if "contrib" in groups and store else None
        has_wd = "wd" in groups and spending is not None       # the lifetime's entry point takes them with a spending rule only
        wd_stats = np.zeros(K, _ffi.STATS_DTYPE) if has_wd else None
        withdrawn = np.empty((K, n_paths), np.float32) if has_wd and store else None
        life = life_hist = life_sum = life_q = life_lv = None
        if lifetime is not None:
            life_lv = np.ascontiguousarray(lifetime, np.float64).ravel()
            life = np.empty((K, n_paths), np.uint32) if store else None
            life_hist = np.zeros((K, prm.n_steps + 1), np.uint64)
            life_sum = np.zeros(K, np.uint64)
            life_q = np.zeros((K, life_lv.size), np.uint32)
        uw_longest = uw_current = uw_longest_hist = uw_current_hist = uw_sums = uw_q = uw_lv = None
        if underwater is not None:
            uw_lv = np.ascontiguousarray(underwater, np.float64).ravel()
            uw_longest = np.empty((K, n_paths), np.uint32) if store else None
            uw_current = np.empty((K, n_paths), np.uint32) if store else None
            uw_longest_hist = np.zeros((K, prm.n_steps + 1), np.uint64)
            uw_current_hist = np.zeros((K, prm.n_steps + 1), np.uint64)
            uw_sums = np.zeros((K, 2), np.uint64)
            uw_q = np.zeros((K, 2, uw_lv.size), np.uint32)
        has_exposure = "exposure" in groups and not drawdown  # SPEC.md 5.19: one second array, the drawdown's when it is asked for
        exposure_stats = np.zeros(K, _ffi.STATS_DTYPE) if has_exposure else None
        exposure = np.empty((K, n_paths), np.float32) if has_exposure and store else None
        trades = trade_hist = trade_sum = trade_q = trade_lv = turnover = turnover_stats = tol = None
        if tolerance is not None:
            from .tolerance import n_reviews
            tol = np.ascontiguousarray(tolerance[2], np.float32)
            trade_lv = np.ascontiguousarray(tolerance[3], np.float64).ravel()
            trades = np.empty((K, n_paths), np.uint32) if store else None
            turnover = np.empty((K, n_paths), np.float32) if store else None
            trade_hist = np.zeros((K, n_reviews(prm.n_steps, tolerance[0]) + 1), np.uint64)
            trade_sum = np.zeros(K, np.uint64)
            trade_q = np.zeros((K, trade_lv.size), np.uint32)
            turnover_stats = np.zeros(K, _ffi.STATS_DTYPE)
        vals = {"ctx": (self._h,), "prm": (prm,), "mu": (mu,), "chol": (chol,), "W": (W,), "walk": (seed, path_begin, n_paths),
                "hz_in": (H, steps if H else None, L, lv if L else None), "out": (term, stats), "dd": (raw, dd_stats),
                "hz_out": (hz_term, hz_stats, bands if L else None), "counts": (counts,), "hz_counts": (hz_counts,), "pairs": (pairs,),
                "contrib": (contrib,), "attr": (attr,), "attr_counts": (attr_counts,), "bt": (bt,),
                "pt": (_ffi.make_protect(*protect, target=target) if protect is not None else None,),
                "sp": (_ffi.make_spending(*spending, target=target) if spending is not None else None,), "wd": (withdrawn, wd_stats),
                "life": (life, life_hist, life_sum, 0 if life_lv is None else life_lv.size, life_lv if life_lv is not None and life_lv.size else None,
                         life_q if life_lv is not None and life_lv.size else None),
                "tb": (_ffi.make_band(tolerance[0], tolerance[1], tol) if tolerance is not None else None,),
                "vt": (_ffi.make_vol_target(*vol_target, target_value=target) if vol_target is not None else None,),
                "exposure": (exposure, exposure_stats),
                "du": (_ffi.make_drift_uncertainty(drift_uncertainty) if drift_uncertainty is not None else None,),
                "uw": (uw_longest, uw_current, uw_longest_hist, uw_current_hist, uw_sums, 0 if uw_lv is None else uw_lv.size,
                       uw_lv if uw_lv is not None and uw_lv.size else None, uw_q if uw_lv is not None and uw_lv.size else None),
                "trades": (trades, trade_hist, trade_sum, 0 if trade_lv is None else trade_lv.size,
                           trade_lv if trade_lv is not None and trade_lv.size else None, trade_q if trade_lv is not None and trade_lv.size else None,
                           turnover, turnover_stats),
                "gl": (_ffi.make_glide(*glide) if glide is not None else None,),               # flows None: the all-zero schedule
                "cf": (_ffi.make_cashflow(flows, target) if flows is not None else None,),
                "rb": (_ffi.McpRebalance(int(period), 0, float(cost)) if period is not None else None,),
                "st": (_ffi.McpStudentT(int(dof), 0) if dof is not None else None,),
                "gv": (_ffi.McpGarch(float(garch[0]), float(garch[1]), float(garch[2]), 0) if garch is not None else None,),
                "jp": (_ffi.make_jumps(*jumps) if jumps is not None else None,),
                "rs": (_ffi.make_regimes(*regimes) if regimes is not None else None,),
                "ft": (_ffi.make_filtered(*filtered, block) if filtered is not None else None,),
                "ov": (_ffi.make_overlay(*overlay) if overlay is not None else None,)}

        def arg(group, v):               # a struct by reference and an array by its address; the ndpointer flavour takes the array
            if isinstance(v, np.ndarray):
                return v if group.endswith("*") else _ffi.ptr(v)
            return ctypes.byref(v) if isinstance(v, ctypes.Structure) else v
        ds_stats = ds_sums = ds_hz_stats = ds_tau = None
        if downside is not None:                               # SPEC.md 5.22: arm the context; the call below takes the request
            ds_tau = float(prm.rf) if downside is True else float(downside)
            ds_stats, ds_sums = np.zeros(K, _ffi.DOWNSIDE_STATS_DTYPE), np.zeros(K, _ffi.DOWNSIDE_SUMS_DTYPE)
            ds_hz_stats = np.zeros((H, K), _ffi.DOWNSIDE_STATS_DTYPE) if H else None
            _ffi.check(_ffi.lib().mcp_ctx_request_downside(self._h, ctypes.byref(_ffi.McpDownside(ds_tau, int(downside is True), 0)),
                                                           _ffi.ptr(ds_sums), _ffi.ptr(ds_stats), _ffi.ptr(ds_hz_stats)))
        rl_stats = rl_sums = rl_hz_stats = rl_active_stats = rl_active = None
        if benchmark is not None:                              # SPEC.md 5.23: likewise
            rl_stats, rl_sums = np.zeros(K, _ffi.RELATIVE_STATS_DTYPE), np.zeros(K, _ffi.RELATIVE_SUMS_DTYPE)
            rl_active_stats = np.zeros(K, _ffi.STATS_DTYPE)
            rl_active = np.empty((K, n_paths), np.float32) if store else None
            rl_hz_stats = np.zeros((H, K), _ffi.RELATIVE_STATS_DTYPE) if H else None
            rc = _ffi.lib().mcp_ctx_request_relative(self._h, ctypes.byref(_ffi.McpRelative(int(benchmark), 0)), _ffi.ptr(rl_sums),
                                                     _ffi.ptr(rl_stats), _ffi.ptr(rl_active_stats), _ffi.ptr(rl_active), _ffi.ptr(rl_hz_stats))
            if rc < 0 and downside is not None:                # the downside request is already in place: it goes with this one
                why = _ffi.lib().mcp_last_error()
                _ffi.lib().mcp_ctx_request_downside(self._h, None, None, None, None)
                raise _ffi.McpError(f"libmcport error {rc}: {why.decode('utf-8', 'replace')}")
            _ffi.check(rc)

        def withdraw():
            if downside is not None:
                _ffi.lib().mcp_ctx_request_downside(self._h, None, None, None, None)
            if benchmark is not None:
                _ffi.lib().mcp_ctx_request_relative(self._h, None, None, None, None, None, None)
        try:
            rc = getattr(_ffi.lib(), entry)(*(arg(g, v) for g in groups for v in vals[g.rstrip("*")]))
        except BaseException:
            withdraw()                                         # the call never reached the library: withdraw the requests
            raise
        if rc < 0 and (downside is not None or benchmark is not None):   # a call refused before its rules were looked at leaves the requests in place
            why = _ffi.lib().mcp_last_error()
            withdraw()
            raise _ffi.McpError(f"libmcport error {rc}: {why.decode('utf-8', 'replace')}")
        _ffi.check(rc)
        return _Outputs(stats, dd_stats, hz_stats, bands, term, raw, hz_term, counts, hz_counts, attr, attr_counts, contrib, pairs,
                        wd_stats, withdrawn, life_hist, life_sum, life_q, life, trade_hist, trade_sum, trade_q, trades, turnover_stats, turnover,
                        exposure_stats, exposure, uw_longest_hist, uw_current_hist, uw_sums, uw_q, uw_longest, uw_current,
                        ds_stats, ds_sums, ds_hz_stats, ds_tau, rl_stats, rl_sums, rl_hz_stats, rl_active_stats, rl_active,
                        None if benchmark is None else int(benchmark))

    def simulate_uncertain(self, prm: _ffi.McpParams, factor, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                           drawdown: bool = False, horizons=None, levels=(), flows=None, target=None):
        """simulate() / simulate_drawdown() / simulate_horizons() / simulate_cashflow() on Gaussian draws with the drift of every path
        drawn once, m = mu + M g (SPEC.md 2.7 / 4.21; include/mcport_uncertain.h, mcp_simulate_uncertain): `factor` is the binary32
        lower-triangular M [N, N] (uncertainty.drift_factor) -> _Outputs as those calls leave them; counts and hz_counts with `flows`
        only."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, drawdown=drawdown, horizons=horizons, levels=levels,
                          flows=flows, target=target, drift_uncertainty=np.ascontiguousarray(factor, np.float32))

    def simulate_underwater(self, prm: _ffi.McpParams, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                            levels=(50.0, 95.0), dof=None, garch=None, jumps=None):
        """simulate_drawdown() / simulate_student_t() / simulate_garch() / simulate_jumps() with the drawdown and the time under water of
        every path switched on (SPEC.md 4.20 / 5.20; include/mcport_underwater.h, mcp_simulate_underwater).  `levels`: the percentages
        of the two counters' order statistics.  -> _Outputs of that call with uw_longest_hist and uw_current_hist [K, n_steps + 1]
        uint64, uw_sums [K, 2] uint64 {sum of m, sum of c_T}, uw_q [K, 2, len(levels)] uint32 and, with `store`, uw_longest and
        uw_current [K, n_paths] uint32."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, dof=dof, garch=garch, jumps=jumps, drawdown=True,
                          underwater=np.asarray(levels, np.float64).ravel())

    def simulate_banded(self, prm: _ffi.McpParams, every: int, cost: float, tol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                        levels=(5.0, 50.0, 95.0), mu=None, chol=None, rows=None, block: float = 1.0, horizons=None, bands=()):
        """simulate_rebalanced() with the trade of every review decided per path by the tolerance table `tol` [K, N] (SPEC.md 4.18 / 5.18;
        include/mcport_band.h, mcp_simulate_banded): `every` is the review period (0: never), `cost` the proportional cost.  `levels`:
        the percentages of the trade counts' order statistics; `bands`: the levels of the horizons' bands.  -> _Outputs of
        simulate_rebalanced with trade_hist [K, n_reviews + 1] uint64, trade_sum [K] uint64, trade_q [K, len(levels)] uint32,
        turnover_stats [K] mcp_stats records over Y - 1 and, with `store`, trades [K, n_paths] uint32 and turnover [K, n_paths]
        binary32."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, rows=rows, block=block, horizons=horizons, levels=bands,
                          tolerance=(int(every), float(cost), np.ascontiguousarray(tol, np.float32), np.asarray(levels, np.float64).ravel()))

    def simulate_lifetime(self, prm: _ffi.McpParams, W, seed: int, path_begin: int, n_paths: int, store: bool, levels=(5.0, 25.0, 50.0),
                          flows=None, glide=None, spending=None, mu=None, chol=None, rows=None, block: float = 1.0, dof=None, target=None,
                          horizons=None, bands=()):
        """simulate_cashflow() (flows), simulate_glide() (flows and glide) or simulate_spending() (spending) with the lifetime of every
        path switched on (SPEC.md 4.17 / 5.17; include/mcport_life.h, mcp_simulate_lifetime): exactly one of flows and spending.
        `levels`: the percentages of the lifetime's order statistics; `bands`: the levels of the horizons' bands.  -> _Outputs of that
        call with life_hist [K, n_steps + 1] uint64, life_sum [K] uint64, life_q [K, len(levels)] uint32 and, with `store`, life
        [K, n_paths] uint32."""
        sp = None if spending is None else tuple(spending) + (0.0, None)[len(tuple(spending)) - 4:]
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, rows=rows, block=block, dof=dof, target=target,
                          horizons=horizons, levels=bands, flows=None if flows is None else np.ascontiguousarray(flows, np.float32),
                          glide=None if glide is None else (np.ascontiguousarray(glide[0], np.int32), np.ascontiguousarray(glide[1], np.float32)),
                          spending=sp,
                          lifetime=np.asarray(levels, np.float64).ravel())

    def simulate(self, prm: _ffi.McpParams, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool):
        o = self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol)
        return o.stats, o.terminal

    def simulate_drawdown(self, prm: _ffi.McpParams, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool):
        """simulate() plus the max drawdown of every path (SPEC.md 4.2 / 5.1; include/mcport.h, mcp_simulate_drawdown) ->
        (stats, dd_stats, terminal, qd): dd_stats is a [K] mcp_stats record array over the per-path drawdowns; with `store`,
        qd is the kernels' binary32 [K, n_paths] q (simple: mdd = q - 1) or d (log: mdd = expm1(d)), see mdd_from_raw."""
        o = self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, drawdown=True)
        return o.stats, o.dd_stats, o.terminal, o.qd

    def simulate_horizons(self, prm: _ffi.McpParams, mu, chol, W, seed: int, path_begin: int, n_paths: int, horizons, levels,
                          store: bool):
        """simulate() plus the values after the steps `horizons` (SPEC.md 4.3 / 5.2; include/mcport.h, mcp_simulate_horizons)
        -> (stats [K], hz_stats [H, K] mcp_stats records, bands [H, K, L] float64 np.percentile(x_h, levels), terminal,
        horizon_terminal): with `store`, terminal is [K, n_paths] and horizon_terminal the binary32 [H, K, n_paths] V_h / S_h."""
        o = self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, horizons=horizons, levels=levels)
        return o.stats, o.hz_stats, o.bands, o.terminal, o.horizon_terminal

    def simulate_bootstrap(self, prm: _ffi.McpParams, rows, W, block: float, seed: int, path_begin: int, n_paths: int,
                           store: bool):
        """simulate() on bootstrap paths (SPEC.md 2.1 / 4.4; include/mcport.h, mcp_simulate_bootstrap): rows is the binary32
        [R, N] table of observed returns, block the mean block length -> (stats [K], terminal [K, n_paths] or None)."""
        o = self._call(prm, W, seed, path_begin, n_paths, store, rows=rows, block=block)
        return o.stats, o.terminal

    def simulate_bootstrap_horizons(self, prm: _ffi.McpParams, rows, W, block: float, seed: int, path_begin: int, n_paths: int,
                                    horizons, levels, store: bool):
        """simulate_horizons() on bootstrap paths (include/mcport.h, mcp_simulate_bootstrap_horizons) -> (stats, hz_stats,
        bands, terminal, horizon_terminal) as simulate_horizons."""
        o = self._call(prm, W, seed, path_begin, n_paths, store, rows=rows, block=block, horizons=horizons, levels=levels)
        return o.stats, o.hz_stats, o.bands, o.terminal, o.horizon_terminal

    def simulate_rebalanced(self, prm: _ffi.McpParams, period: int, cost: float, W, seed: int, path_begin: int, n_paths: int,
                            store: bool, mu=None, chol=None, rows=None, block: float = 1.0, horizons=None, levels=()):
        """simulate() / simulate_horizons() / simulate_bootstrap[_horizons]() with the weights rebalanced every `period` steps
        (0: bought and held) at the proportional cost `cost` (SPEC.md 4.5 / 5.4; include/mcport.h, mcp_simulate_rebalanced).
        Draws: `mu` and `chol` (Gaussian) or `rows` and `block` (bootstrap).  -> (stats [K], hz_stats [H, K], bands [H, K, L],
        terminal, horizon_terminal) as simulate_horizons; the horizon entries are None without horizons."""
        o = self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, rows=rows, block=block, period=period, cost=cost,
                       horizons=horizons, levels=levels)
        return o.stats, o.hz_stats, o.bands, o.terminal, o.horizon_terminal

    def simulate_student_t(self, prm: _ffi.McpParams, dof: int, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                           drawdown: bool = False, horizons=None, levels=()):
        """simulate() / simulate_drawdown() / simulate_horizons() on Student-t draws with `dof` degrees of freedom (SPEC.md 2.2 /
        4.6; include/mcport.h, mcp_simulate_student_t; simple compounding only) -> (stats [K], dd_stats [K] or None, hz_stats
        [H, K], bands [H, K, L], terminal, qd, horizon_terminal): the entries of the blocks not asked for are None; with `store`,
        terminal is [K, n_paths], qd the binary32 drawdown q [K, n_paths], horizon_terminal [H, K, n_paths]."""
        return tuple(self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, dof=dof, drawdown=drawdown,
                                horizons=horizons, levels=levels))[:7]

    def simulate_garch(self, prm: _ffi.McpParams, garch, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                       dof=None, drawdown: bool = False, horizons=None, levels=()):
        """simulate() / simulate_drawdown() / simulate_horizons() / simulate_student_t() with the GARCH(1,1) variance ratio of
        SPEC.md 4.9 scaling every step's normals: `garch` is (alpha, beta, h0) (SPEC.md 4.9 / 5.8; include/mcport.h,
        mcp_simulate_garch; simple compounding only); dof=None: Gaussian draws -> _Outputs; the entries of the blocks not asked
        for are None."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, dof=dof, drawdown=drawdown, horizons=horizons,
                          levels=levels, garch=garch)

    def simulate_jumps(self, prm: _ffi.McpParams, jumps, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                       drawdown: bool = False, horizons=None, levels=()):
        """simulate() / simulate_drawdown() / simulate_horizons() with the market jump of SPEC.md 2.5 added to every step: `jumps`
        is the (intensity, mean, std, loading) of check_jumps, loading None (all ones) or binary32 [N]; `chol` is the diffusive
        factor (SPEC.md 4.12 / 5.12; include/mcport.h, mcp_simulate_jumps; simple compounding only) -> _Outputs; the entries of the
        blocks not asked for are None."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, drawdown=drawdown, horizons=horizons,
                          levels=levels, jumps=jumps)

    def simulate_regimes(self, prm: _ffi.McpParams, regimes, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                         drawdown: bool = False, horizons=None, levels=()):
        """simulate() / simulate_drawdown() / simulate_horizons() on the two regimes of SPEC.md 2.6: `regimes` is (p01, p10, start, mu1,
        chol1) with mu1 binary32 [N] and chol1 binary32 [N, N], the drift and lower Cholesky factor of regime 1; `mu` and `chol` are
        regime 0 (SPEC.md 4.13 / 5.13; include/mcport.h, mcp_simulate_regimes; simple compounding only) -> _Outputs; the entries of
        the blocks not asked for are None."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, drawdown=drawdown, horizons=horizons,
                          levels=levels, regimes=regimes)

    def simulate_filtered(self, prm: _ffi.McpParams, filtered, garch, W, block: float, seed: int, path_begin: int, n_paths: int,
                          store: bool, horizons=None, levels=(), downside=None, benchmark=None):
        """simulate_bootstrap[_horizons]() on filtered rows (SPEC.md 2.4 / 4.11; include/mcport.h, mcp_simulate_filtered; simple
        compounding only): `filtered` is the binary32 (mu [N], resid [R, N], shock [R]) triple, `garch` (alpha, beta, h0) -> _Outputs;
        the horizon entries are None without horizons."""
        return self._call(prm, W, seed, path_begin, n_paths, store, block=block, horizons=horizons, levels=levels, garch=garch,
                          filtered=filtered, downside=downside, benchmark=benchmark)

    def simulate_attribution(self, prm: _ffi.McpParams, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool, dof=None,
                             garch=None):
        """simulate() / simulate_student_t() / simulate_garch() (no drawdown, no horizons) followed by the second walk that
        attributes every portfolio's mean, CVaR and standard deviation to its assets (SPEC.md 4.10 / 5.9; include/mcport.h,
        mcp_simulate_attribution; simple compounding, K <= 16, path shards) -> _Outputs: stats and terminal bit for bit those of the
        call without it, attr [K, N] records of _ffi.ATTR_DTYPE, attr_counts [K, 2] uint64 {n, n_tail} and, with `store`,
        contributions [K, N, n_paths] binary32."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, dof=dof, garch=garch, attribution=True)

    def simulate_antithetic(self, prm: _ffi.McpParams, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool, dof=None,
                            garch=None, drawdown: bool = False, horizons=None, levels=()):
        """simulate() / simulate_drawdown() / simulate_horizons() / simulate_student_t() / simulate_garch() on antithetic pairs
        (SPEC.md 2.3 / 5.10; include/mcport.h, mcp_simulate_antithetic; path_begin and n_paths even; log compounding on Gaussian
        draws only; path shards) -> _Outputs: the paths 2j and 2j + 1 share the draws of path j of the call without pairs, path
        2j + 1 with the asset normals negated; the statistics are over all n_paths values, pairs [K] records of _ffi.PAIR_DTYPE."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, dof=dof, garch=garch, drawdown=drawdown,
                          horizons=horizons, levels=levels, antithetic=True)

    def simulate_cashflow(self, prm: _ffi.McpParams, flows, W, seed: int, path_begin: int, n_paths: int, store: bool, mu=None,
                          chol=None, rows=None, block: float = 1.0, dof=None, target=None, horizons=None, levels=()):
        """simulate() / simulate_horizons() / simulate_bootstrap[_horizons]() / simulate_student_t() with the schedule `flows`
        (binary32 [n_steps]; positive: paid in, negative: taken out) applied at the end of every step and ruin absorbing (SPEC.md
        4.7 / 5.6; include/mcport.h, mcp_simulate_cashflow; simple compounding only).  Draws: `mu` and `chol` (Gaussian, or
        Student-t with `dof`) or `rows` and `block` (bootstrap).  -> _Outputs (stats [K], hz_stats [H, K], bands [H, K, L], terminal,
        horizon_terminal, counts [K, 2] uint64 {n_ruined, n_short}, hz_counts [H, K, 2]); the horizon entries are None without
        horizons, n_short is 0 without `target`."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, rows=rows, block=block, dof=dof,
                          horizons=horizons, levels=levels, flows=np.ascontiguousarray(flows, np.float32), target=target)

    def simulate_glide(self, prm: _ffi.McpParams, glide, W, seed: int, path_begin: int, n_paths: int, store: bool, flows=None, mu=None,
                       chol=None, rows=None, block: float = 1.0, dof=None, target=None, horizons=None, levels=()):
        """simulate_cashflow() on the scheduled target weights of a glide path (SPEC.md 4.14 / 5.14; include/mcport.h,
        mcp_simulate_glide; simple compounding only): `glide` is (breaks int32 [G], targets binary32 [G, K, N]); step s walks on
        target block #{j : breaks[j] < s}, block 0 being `W`.  flows None: the all-zero schedule.  Draws and -> _Outputs as
        simulate_cashflow."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, rows=rows, block=block, dof=dof,
                          horizons=horizons, levels=levels, flows=None if flows is None else np.ascontiguousarray(flows, np.float32),
                          target=target, glide=(np.ascontiguousarray(glide[0], np.int32), np.ascontiguousarray(glide[1], np.float32)))

    def simulate_protected(self, prm: _ffi.McpParams, protect, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                           dof=None, garch=None, jumps=None, target=None, drawdown: bool = False, horizons=None, levels=()):
        """simulate() / simulate_student_t() / simulate_garch() / simulate_jumps(), with their drawdown or horizons, under the floor
        rule of SPEC.md 4.15 (CPPI with an exposure cap and a drawdown ratchet; include/mcport_protect.h, mcp_simulate_protected;
        simple compounding only): `protect` is (floor binary32 [n_steps + 1], multiplier, rate, cap, ratchet) -> _Outputs with counts
        [K, 2] uint64 {n_gap: V_T below the floor, n_short: V_T below `target`, 0 without one} and hz_counts [H, K, 2]; the entries of
        the blocks not asked for are None."""
        floor = np.ascontiguousarray(protect[0], np.float32)
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, dof=dof, garch=garch, jumps=jumps, target=target,
                          drawdown=drawdown, horizons=horizons, levels=levels, protect=(floor,) + tuple(float(v) for v in protect[1:5]))

    def simulate_vol_target(self, prm: _ffi.McpParams, vol_target, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                            dof=None, garch=None, jumps=None, target=None, drawdown: bool = False, horizons=None, levels=()):
        """simulate() / simulate_student_t() / simulate_garch() / simulate_jumps(), with their drawdown or horizons, under the
        volatility target of SPEC.md 4.19 (include/mcport_voltarget.h, mcp_simulate_vol_target; simple compounding only): `vol_target`
        is (target, decay, cap, rate, spread, s0 float64 [K] or None) -> _Outputs with counts [K, 2] uint64 {n_ruined, n_short: V_T
        below `target`, 0 without one}, hz_counts [H, K, 2] and, without `drawdown`, exposure_stats [K] (the record of the summed
        exposure Y_T - 1) and, with `store`, exposure [K, n_paths] binary32."""
        vt = tuple(vol_target) + (1.0, 0.0, 0.0, None)[len(tuple(vol_target)) - 2:]
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, dof=dof, garch=garch, jumps=jumps, target=target,
                          drawdown=drawdown, horizons=horizons, levels=levels, vol_target=vt)

    def simulate_spending(self, prm: _ffi.McpParams, spending, W, seed: int, path_begin: int, n_paths: int, store: bool, mu=None,
                          chol=None, rows=None, block: float = 1.0, dof=None, target=None, horizons=None, levels=()):
        """simulate_cashflow() with a withdrawal that depends on the path in place of the schedule (SPEC.md 4.16 / 5.16;
        include/mcport_spend.h, mcp_simulate_spending; simple compounding only): `spending` is (rate, every, down, up[, inflation[,
        first]]), first None: rate times v0.  Draws as simulate_cashflow -> _Outputs with counts [K, 2] uint64 {n_ruined, n_short},
        hz_counts [H, K, 2], wd_stats [K] (the record of the total paid out Y_T) and, with `store`, withdrawn [K, n_paths] binary32."""
        sp = tuple(spending) + (0.0, None)[len(tuple(spending)) - 4:]
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, rows=rows, block=block, dof=dof, target=target,
                          horizons=horizons, levels=levels, spending=sp)

    def simulate_overlay(self, prm: _ffi.McpParams, overlay, mu, chol, W, seed: int, path_begin: int, n_paths: int, store: bool,
                         dof=None, drawdown: bool = False, horizons=None, levels=()):
        """simulate() / simulate_drawdown() / simulate_horizons() / simulate_student_t() with the option rows `overlay` (the (rows,
        row_begin, spot) triple of check_overlay) applied to every asset's return inside the walk (SPEC.md 4.8 / 5.7;
        include/mcport.h, mcp_simulate_overlay; simple compounding only) -> _Outputs; the entries of the blocks not asked for are
        None."""
        return self._call(prm, W, seed, path_begin, n_paths, store, mu=mu, chol=chol, dof=dof, drawdown=drawdown, horizons=horizons,
                          levels=levels, overlay=overlay)


# What Context._call returns: mcp_stats record arrays (stats [K], dd_stats [K], hz_stats [H, K]), bands [H, K, L] and the stored
# binary32 arrays (terminal [K, n], qd [K, n], horizon_terminal [H, K, n]); with cash flows the counts {n_ruined, n_short} of
# SPEC.md 5.6 (counts [K, 2], hz_counts [H, K, 2], uint64).
# With attribution the records of SPEC.md 5.9 (attr [K, N] of ATTR_DTYPE, attr_counts [K, 2] uint64 {n, n_tail}) and, stored, the
# binary32 contributions [K, N, n].  With antithetic pairs the records of SPEC.md 5.10 (pairs [K] of PAIR_DTYPE).  With a spending rule
# the record of the total paid out (wd_stats [K]) and, stored, the binary32 withdrawn [K, n] (SPEC.md 5.16).  With a volatility target
# and no drawdown the record of the summed exposure (exposure_stats [K], over Y - 1) and, stored, the binary32 exposure [K, n] (5.19).
# With a downside request the records of SPEC.md 5.22 (downside_stats [K] of DOWNSIDE_STATS_DTYPE, downside_sums [K] of
# DOWNSIDE_SUMS_DTYPE, downside_hz_stats [H, K] with horizons) and the threshold they are about (downside_tau).  With a relative
# request the records of SPEC.md 5.23 (relative_stats [K] of RELATIVE_STATS_DTYPE, relative_sums [K] of RELATIVE_SUMS_DTYPE,
# relative_hz_stats [H, K] with horizons, relative_active_stats [K] of STATS_DTYPE over Y - 1 and, stored, the binary32 relative_active
# [K, n] Y) and the row they are against (relative_bench).
_Outputs = collections.namedtuple("_Outputs", "stats dd_stats hz_stats bands terminal qd horizon_terminal counts hz_counts attr "
                                  "attr_counts contributions pairs wd_stats withdrawn life_hist life_sum life_q life trade_hist trade_sum trade_q trades "
                                  "turnover_stats turnover exposure_stats exposure uw_longest_hist uw_current_hist uw_sums uw_q uw_longest uw_current "
                                  "downside_stats downside_sums downside_hz_stats downside_tau "
                                  "relative_stats relative_sums relative_hz_stats relative_active_stats relative_active relative_bench",
                                  defaults=(None,) * 36)


def check_cashflow(cashflow, target, n_steps):
    """SPEC.md 4.7 argument rules -> (flows, target): flows None (no cash flows) or the binary32 [n_steps] schedule -- a number is
    that amount after every step, a sequence must hold exactly n_steps numbers --, target None or a finite float.  ValueError for
    a bool, another length, an entry that is not finite (also after rounding to binary32), or a target without cashflow."""
    def number(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    if target is not None:
        if cashflow is None:
            raise ValueError("target needs cashflow (a goal without flows: cashflow=0)")
        if not number(target) or not np.isfinite(float(target)):
            raise ValueError(f"target must be a finite number, got {target!r}")
        target = float(target)
    if cashflow is None:
        return None, None
    if isinstance(cashflow, (bool, np.bool_)):
        raise ValueError(f"cashflow must be a number or a sequence of n_steps numbers, got {cashflow!r}")
    if number(cashflow):
        vals = np.full(int(n_steps), float(cashflow), np.float64)
    else:
        if isinstance(cashflow, (str, bytes)) or any(not number(v) for v in np.asarray(cashflow, object).ravel().tolist()):
            raise ValueError("cashflow must be a number or a sequence of n_steps numbers (no bools, no strings)")
        vals = np.asarray(cashflow, np.float64)
        if vals.ndim != 1 or vals.size != int(n_steps):
            raise ValueError(f"cashflow must hold exactly n_steps={n_steps} numbers, got shape {vals.shape}")
    with np.errstate(over="ignore"):
        flows = np.ascontiguousarray(vals.astype(np.float32))
    if not np.all(np.isfinite(flows)):
        raise ValueError("cashflow entries must be finite (in binary32)")
    return flows, target


def check_glide(glide, weights, n_steps):
    """SPEC.md 4.14 argument rules -> None (no glide path) or (breaks int32 [G], targets binary32 [G, K, N], C-contiguous).  `glide`
    is (breaks, targets): breaks, at most 64 strictly increasing whole steps in [1, n_steps - 1]; targets, the weights held AFTER
    each break, [G, N] for a weight vector and [K, G, N] for K portfolios.  ValueError for anything else: not a pair, bools, breaks
    out of range or order, a shape that does not match the weights, an entry that is not finite (also after rounding to
    binary32)."""
    if glide is None:
        return None
    if isinstance(glide, (str, bytes)) or not hasattr(glide, "__len__") or len(glide) != 2:
        raise ValueError("glide must be a (breaks, targets) pair (glide.glide_path(...) builds one)")
    raw = np.atleast_1d(np.asarray(glide[0], object)).ravel().tolist()
    if any(isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, np.integer)) for b in raw):
        raise ValueError("glide breaks must be whole step numbers (no bools, no floats)")
    G = len(raw)
    if G > _ffi.MCP_MAX_GLIDE:
        raise ValueError(f"glide takes at most {_ffi.MCP_MAX_GLIDE} breaks, got {G}")
    if any(not 1 <= int(b) <= int(n_steps) - 1 for b in raw):
        raise ValueError(f"glide breaks must lie in [1, n_steps - 1 = {int(n_steps) - 1}], got {[int(b) for b in raw]}")
    if any(int(b) <= int(a) for a, b in zip(raw, raw[1:])):
        raise ValueError(f"glide breaks must be strictly increasing, got {[int(b) for b in raw]}")
    w = np.asarray(weights)
    if w.ndim not in (1, 2):
        raise ValueError(f"glide needs weights [N] or [K, N], got shape {w.shape}")
    N = w.shape[-1]
    try:
        t64 = np.asarray(glide[1], np.float64)
    except (TypeError, ValueError):
        raise ValueError("glide targets must be numbers") from None
    want = (G, N) if w.ndim == 1 else (w.shape[0], G, N)
    if G == 0 and t64.size == 0:
        t64 = np.zeros(want, np.float64)
    if t64.shape != want:
        raise ValueError(f"glide targets must have shape {want} ([G, N] for a weight vector, [K, G, N] for K portfolios), got {t64.shape}")
    with np.errstate(over="ignore"):
        t32 = t64.astype(np.float32)
    if not np.all(np.isfinite(t32)):
        raise ValueError("glide targets must be finite (in binary32)")
    targets = np.ascontiguousarray(t32[:, None, :] if w.ndim == 1 else np.transpose(t32, (1, 0, 2)))
    return np.ascontiguousarray([int(b) for b in raw], np.int32).reshape(G), targets


def _glide_blocks(gl, W):
    """The 'glide' block of every portfolio: the breaks and the binary32 weights [G + 1, N] as used, segment 0 the call's weights."""
    return [{"breaks": gl[0].astype(np.int64), "weights": np.concatenate([W[k][None, :], gl[1][:, k, :]], axis=0)} for k in range(W.shape[0])]


def check_protect(protect, n_steps, v0=1.0):
    """SPEC.md 4.15 argument rules -> None (no protection) or (floor binary32 [n_steps + 1], multiplier, rate, cap, ratchet).
    `protect` is (floor, multiplier[, rate[, cap[, ratchet]]]), rate 0, cap 1 and ratchet 0 by default.  floor: a number, the floor
    as a fraction of v0 that grows at `rate` per step (protect.floor_schedule), or an explicit sequence of n_steps + 1 floors in the
    units of v0.  ValueError for anything else: not a sequence of 2 to 5 entries, a bool or a string among the numbers, a value that is
    not finite before or after rounding to binary32, a negative floor, multiplier < 0, cap <= 0, rate <= -1, ratchet outside
    [0, 1), a floor sequence of another length."""
    if protect is None:
        return None
    msg = f"protect must be (floor, multiplier[, rate[, cap[, ratchet]]]), got {protect!r}"
    if isinstance(protect, (str, bytes)) or not hasattr(protect, "__len__") or not 2 <= len(protect) <= 5:
        raise ValueError(msg)

    def number(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))

    def finite32(v):
        with np.errstate(over="ignore"):
            return bool(np.isfinite(v)) and bool(np.isfinite(np.float32(v)))
    vals = list(protect[1:]) + [0.0, 1.0, 0.0][len(protect) - 2:]
    if any(not number(v) for v in vals):
        raise ValueError(msg)
    m, rate, cap, ratchet = (float(v) for v in vals)
    if not all(finite32(v) for v in (m, rate, cap, ratchet)):
        raise ValueError(f"protect values must be finite, in binary32 too, got {protect!r}")
    if m < 0.0:
        raise ValueError(f"protect multiplier must be >= 0, got {m!r}")
    if not (cap > 0.0 and np.float32(cap) > 0.0):
        raise ValueError(f"protect cap must be > 0, got {cap!r}")
    if not (rate > -1.0 and np.float32(rate) > np.float32(-1.0)):
        raise ValueError(f"protect rate must be > -1, got {rate!r}")
    if not (0.0 <= ratchet < 1.0 and np.float32(ratchet) < np.float32(1.0)):
        raise ValueError(f"protect ratchet must be in [0, 1), got {ratchet!r}")
    fl = protect[0]
    if number(fl):
        if not finite32(float(fl) * float(v0)) or float(fl) < 0.0:
            raise ValueError(f"the protect floor must be a finite fraction of v0 >= 0, got {fl!r}")
        from .protect import floor_schedule
        floor = floor_schedule(float(fl), rate, n_steps, v0)
    else:
        if isinstance(fl, (str, bytes, bool, np.bool_)) or any(not number(v) for v in np.asarray(fl, object).ravel().tolist()):
            raise ValueError(msg)
        f64 = np.asarray(fl, np.float64).ravel()
        if f64.size != int(n_steps) + 1:
            raise ValueError(f"a protect floor sequence must hold n_steps + 1 = {int(n_steps) + 1} numbers, got {f64.size}")
        with np.errstate(over="ignore"):
            floor = np.ascontiguousarray(f64.astype(np.float32))
    if not np.all(np.isfinite(floor)) or np.any(floor < 0):
        raise ValueError("the protect floors must be finite (in binary32) and >= 0")
    return floor, m, rate, cap, ratchet


def _protect_blocks(pv, counts, hz_counts, n, target):
    """The 'protect' block of every portfolio: the schedule and the binary32 parameters as used, the paths that end below the floor
    (n_gap, gap_probability), below the target (n_short, shortfall_probability; 0 without one) and, with horizons, the same per
    horizon against S_h."""
    floor, m, rate, cap, ratchet = pv
    out = []
    for k in range(counts.shape[0]):
        blk = {"floor": floor.copy(), "multiplier": float(np.float32(m)), "cap": float(np.float32(cap)), "rate": float(np.float32(rate)),
               "ratchet": float(np.float32(ratchet)), "target": target, "n_gap": int(counts[k, 0]), "gap_probability": float(counts[k, 0]) / n,
               "n_short": int(counts[k, 1]), "shortfall_probability": float(counts[k, 1]) / n}
        if hz_counts is not None:
            c = hz_counts[:, k, :]
            blk["horizons"] = {"n_gap": c[:, 0].astype(np.int64), "gap_probability": c[:, 0].astype(np.float64) / n,
                               "n_short": c[:, 1].astype(np.int64), "shortfall_probability": c[:, 1].astype(np.float64) / n}
        out.append(blk)
    return out


def check_spending(spending, v0=1.0):
    """SPEC.md 4.16 argument rules -> None (no spending rule) or (rate, every, down, up, inflation, first or None).  `spending` is
    (rate, every, down, up[, inflation[, first]]), inflation 0 and first None (rate times v0) by default (spending.spending_rule
    builds the three named policies).  rate: the fraction of the current value aimed at per step, finite, >= 0; every: review every
    that many whole steps, >= 0, 0 never; down in [0, 1] and up in [0, inf], inf allowed: the largest cut and raise per review;
    inflation: finite, > -1, applied per review; first: the first withdrawal in currency, finite, >= 0.  ValueError for anything
    else: not such a tuple, bools, a value outside its range before or after rounding to binary32, v0 that is not positive in
    binary32."""
    if spending is None:
        return None
    msg = f"spending must be (rate, every, down, up[, inflation[, first]]), got {spending!r}"
    if isinstance(spending, (str, bytes)) or not hasattr(spending, "__len__") or not 4 <= len(spending) <= 6:
        raise ValueError(msg)
    vals = list(spending) + [0.0, None][len(spending) - 4:]
    rate, every, down, up, inflation, first = vals
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)):
        raise ValueError(f"spending every must be a whole number of steps (no bools, no floats), got {every!r}")
    if not 0 <= int(every) <= 2 ** 31 - 1:
        raise ValueError(f"spending every must be >= 0, got {every!r}")
    nums = [rate, down, up, inflation] + ([first] if first is not None else [])
    if any(isinstance(v, (bool, np.bool_)) for v in nums):
        raise ValueError(msg)
    try:
        rate, down, up, inflation = (float(v) for v in nums[:4])
        first = None if first is None else float(first)
    except (TypeError, ValueError):
        raise ValueError(msg) from None
    with np.errstate(over="ignore", invalid="ignore"):
        f32 = lambda v: float(np.float32(v))   # noqa: E731
        if not (np.isfinite(rate) and rate >= 0.0 and np.isfinite(f32(rate))):
            raise ValueError(f"spending rate must be finite and >= 0, in binary32 too, got {rate!r}")
        if not (0.0 <= down <= 1.0):
            raise ValueError(f"spending down must be in [0, 1], got {down!r}")
        if not up >= 0.0:
            raise ValueError(f"spending up must be >= 0 (inf allowed), got {up!r}")
        if not (np.isfinite(inflation) and inflation > -1.0 and f32(inflation) > -1.0 and f32(1.0 + inflation) > 0.0 and np.isfinite(f32(1.0 + inflation))):
            raise ValueError(f"spending inflation must be finite and > -1, in binary32 too, got {inflation!r}")
        if first is not None and not (np.isfinite(first) and first >= 0.0 and np.isfinite(f32(first))):
            raise ValueError(f"spending first must be finite and >= 0, in binary32 too, got {first!r}")
        v32 = f32(v0)
        if not (v32 > 0.0 and np.isfinite(v32)):
            raise ValueError(f"spending needs a v0 that is positive and finite in binary32, got {v0!r}")
        if first is None and not np.isfinite(f32(f32(rate) * v32)):
            raise ValueError(f"spending rate {rate!r} times v0 {v0!r} overflows binary32")
    return rate, int(every), down, up, inflation, first


def _spending_blocks(sv, v0, out, n, target):
    """The 'spending' block of every portfolio: the binary32 constants as used, the ruined and the short paths (with horizons, per
    horizon too) and 'withdrawn', the record of x_Y = Y_T / fl32(v0) - 1 with its mean / var / cvar also as multiples of v0."""
    p32, g32, lo32, hi32, w0 = (float(c) for c in _ffi.spending_consts(_ffi.make_spending(*sv), v0))
    blocks = []
    for k in range(out.counts.shape[0]):
        blk = {"rate": p32, "every": sv[1], "growth": g32, "lo": lo32, "hi": hi32, "first": w0, "target": target}
        blk.update(_cash_block(out.counts[k], n, target))
        if out.hz_counts is not None:
            blk["horizons"] = _cash_block(out.hz_counts[:, k, :], n, target)
        wd = stats_to_dict(out.wd_stats[k])
        wd.update({f + "_v0": wd[f] + 1.0 for f in ("mean", "var", "cvar")})
        blk["withdrawn"] = wd
        blocks.append(blk)
    return blocks


def _spending_result(out, sv, v0, single, store, as_array, steps, levels, compounding, target):
    """What simulate_paths / simulate_bootstrap return for a spending call: with as_array the tuple of the call without the rule, then
    counts[, hz_counts], wd_stats[, withdrawn]; else the dicts of _result with the 'spending' block and, with `store`, 'withdrawn'."""
    res = _result(out._replace(counts=None, hz_counts=None), single, store, as_array, steps, levels, compounding)
    if as_array:
        return ((res if isinstance(res, tuple) else (res,)) + ((out.counts,) if out.hz_counts is None else (out.counts, out.hz_counts))
                + ((out.wd_stats, out.withdrawn) if store else (out.wd_stats,)))
    for k, (d, blk) in enumerate(zip([res] if isinstance(res, dict) else res, _spending_blocks(sv, v0, out, int(out.stats[0]["n"]), target))):
        d["spending"] = blk
        if store:
            d["withdrawn"] = out.withdrawn[k]
    return res


def check_overlay(overlay, spot, n_assets):
    """SPEC.md 4.8 argument rules -> None (no overlay) or (rows [n_rows] of _ffi.OVERLAY_ROW_DTYPE, row_begin int32 [N + 1], spot
    binary32 [N]).  `overlay` is a dict {asset index: rows} or a length-N list of row lists, rows being the tuples (row_type,
    strike, premium, qty) of options.strategy_rows with the seven row types of options.ROW_TYPES; strike and premium in price
    units.  The sign of a selling row is folded into qty (negation is exact) and the numbers are rounded to binary32.  `spot`: the
    assets' current prices [N] (a number for one asset), needed as soon as one asset owns rows; assets without rows may carry any
    finite value.  ValueError for an unknown row type, a bool, a number that is not finite (also after rounding), a missing or
    non-positive spot, an index out of range or more than MCP_MAX_OVERLAY_ROWS rows on an asset."""
    from .options import BUY_ASSET, LONG_CALL, LONG_PUT, SELL_ASSET, SHORT_CALL, SHORT_FUTURES, SHORT_PUT
    kinds = {BUY_ASSET: (_ffi.MCP_OVERLAY_LINEAR, 1.0), SELL_ASSET: (_ffi.MCP_OVERLAY_LINEAR, -1.0),
             SHORT_FUTURES: (_ffi.MCP_OVERLAY_LINEAR, -1.0), LONG_CALL: (_ffi.MCP_OVERLAY_CALL, 1.0),
             SHORT_CALL: (_ffi.MCP_OVERLAY_CALL, -1.0), LONG_PUT: (_ffi.MCP_OVERLAY_PUT, 1.0), SHORT_PUT: (_ffi.MCP_OVERLAY_PUT, -1.0)}

    def number(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    if overlay is None:
        if spot is not None:
            raise ValueError("spot needs overlay (prices matter to option rows only)")
        return None
    N = int(n_assets)
    per_asset = [[] for _ in range(N)]
    if isinstance(overlay, dict):
        for key, rows in overlay.items():
            if not isinstance(key, (int, np.integer)) or isinstance(key, (bool, np.bool_)) or not 0 <= key < N:
                raise ValueError(f"overlay asset index {key!r} outside [0, {N})")
            per_asset[int(key)] = list(rows)
    else:
        if isinstance(overlay, (str, bytes)) or not hasattr(overlay, "__len__") or len(overlay) != N:
            raise ValueError(f"overlay must be a dict {{asset index: rows}} or a list of {N} row lists")
        per_asset = [list(rows) if rows is not None else [] for rows in overlay]
    out, begin = [], [0]
    for i, rows in enumerate(per_asset):
        if len(rows) > _ffi.MCP_MAX_OVERLAY_ROWS:
            raise ValueError(f"asset {i} owns {len(rows)} overlay rows, at most {_ffi.MCP_MAX_OVERLAY_ROWS}")
        for row in rows:
            if not isinstance(row, (tuple, list)) or len(row) != 4:
                raise ValueError(f"an overlay row is (row_type, strike, premium, qty), got {row!r}")
            row_type, strike, premium, qty = row
            if not isinstance(row_type, str) or row_type not in kinds:
                raise ValueError(f"unknown overlay row type {row_type!r} (options.ROW_TYPES)")
            if not all(number(v) for v in (strike, premium, qty)):
                raise ValueError(f"overlay strike, premium and qty must be numbers (no bools), got {row!r}")
            kind, sign = kinds[row_type]
            with np.errstate(over="ignore"):
                vals = np.array([strike, premium, sign * float(qty)], np.float64).astype(np.float32)
            if not np.all(np.isfinite(vals)):
                raise ValueError(f"overlay strike, premium and qty must be finite (in binary32), got {row!r}")
            out.append((kind, vals[0], vals[1], vals[2]))
        begin.append(len(out))
    table = np.array(out, _ffi.OVERLAY_ROW_DTYPE) if out else np.zeros(0, _ffi.OVERLAY_ROW_DTYPE)
    if spot is None:
        if out:
            raise ValueError("overlay rows need spot, the assets' current prices [N]")
        spot32 = np.ones(N, np.float32)
    else:
        vals = np.atleast_1d(np.asarray(spot, object)).ravel().tolist()
        if len(vals) != N or not all(number(v) for v in vals):
            raise ValueError(f"spot must hold {N} numbers (no bools)")
        with np.errstate(over="ignore"):
            spot32 = np.asarray(vals, np.float64).astype(np.float32)
        if not np.all(np.isfinite(spot32)):
            raise ValueError("spot must be finite (in binary32)")
        for i in range(N):
            if begin[i + 1] > begin[i] and not spot32[i] > 0:
                raise ValueError(f"spot of asset {i} must be positive (it owns overlay rows), got {vals[i]!r}")
    return np.ascontiguousarray(table), np.asarray(begin, np.int32), np.ascontiguousarray(spot32)


def check_dof(dof):
    """SPEC.md 2.2 argument rule -> None (Gaussian draws) or the int nu in [3, MCP_MAX_T_DOF]; ValueError otherwise (a bool,
    a non-integral value, a value out of range)."""
    if dof is None:
        return None
    if isinstance(dof, (bool, np.bool_)) or not isinstance(dof, (int, float, np.integer, np.floating)):
        raise ValueError(f"dof must be an integer in [3, {_ffi.MCP_MAX_T_DOF}], got {dof!r}")
    if not float(dof).is_integer() or not 3 <= dof <= _ffi.MCP_MAX_T_DOF:
        raise ValueError(f"dof must be an integer in [3, {_ffi.MCP_MAX_T_DOF}], got {dof!r}")
    return int(dof)


def check_garch(garch):
    """SPEC.md 4.9 argument rules -> None (no GARCH) or the floats (alpha, beta, h0), h0 = 1 for a pair; ValueError otherwise (not
    a sequence of 2 or 3 numbers, a bool or a string among them, a non-finite value, alpha < 0, beta < 0, fl32(alpha) + fl32(beta)
    >= 1, fl32(h0) <= 0)."""
    if garch is None:
        return None
    msg = f"garch must be (alpha, beta) or (alpha, beta, h0), got {garch!r}"
    if isinstance(garch, (str, bytes)) or not hasattr(garch, "__len__") or len(garch) not in (2, 3):
        raise ValueError(msg)
    vals = []
    for v in garch:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(msg)
        if not np.isfinite(v):
            raise ValueError(f"garch values must be finite, got {garch!r}")
        vals.append(float(v))
    if len(vals) == 2:
        vals.append(1.0)
    with np.errstate(over="ignore"):
        a, b, g = (np.float32(v) for v in vals)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(g)):
        raise ValueError(f"garch values must be finite in binary32, got {garch!r}")
    if not (a >= 0 and b >= 0):
        raise ValueError(f"garch alpha and beta must be >= 0, got {garch!r}")
    if not float(a) + float(b) < 1.0 or not np.float32(1.0 - float(a) - float(b)) > 0:
        raise ValueError(f"garch alpha + beta must be < 1 in binary32, got {garch!r}")
    if not g > 0:
        raise ValueError(f"garch h0 must be > 0 in binary32, got {garch!r}")
    return tuple(vals)


def check_jumps(jumps, n_assets):
    """SPEC.md 2.5 argument rules -> None (no jumps) or (intensity, mean, std, loading): three floats and None (all ones) or the
    binary32 [N] loadings; ValueError otherwise (not a sequence of 3 or 4 entries, a bool or a string among the numbers, a value
    that is not finite before or after rounding to binary32, intensity outside [0, 1], std < 0, loadings of another length)."""
    if jumps is None:
        return None
    msg = f"jumps must be (intensity, mean, std) or (intensity, mean, std, loading), got {jumps!r}"
    if isinstance(jumps, (str, bytes)) or not hasattr(jumps, "__len__") or len(jumps) not in (3, 4):
        raise ValueError(msg)
    vals = []
    for v in tuple(jumps)[:3]:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(msg)
        with np.errstate(over="ignore"):
            if not np.isfinite(v) or not np.isfinite(np.float32(v)):
                raise ValueError(f"jumps values must be finite, in binary32 too, got {jumps!r}")
        vals.append(float(v))
    if not 0.0 <= vals[0] <= 1.0:
        raise ValueError(f"jumps intensity must be in [0, 1] (expected jumps per step), got {vals[0]!r}")
    if not vals[2] >= 0.0:
        raise ValueError(f"jumps std must be >= 0, got {vals[2]!r}")
    loading = None
    if len(jumps) == 4 and jumps[3] is not None:
        try:
            with np.errstate(over="ignore"):
                loading = np.ascontiguousarray(np.asarray(jumps[3], np.float64).astype(np.float32)).ravel()
        except (TypeError, ValueError):
            raise ValueError(msg) from None
        if np.asarray(jumps[3]).dtype == np.bool_ or loading.size != int(n_assets):
            raise ValueError(f"jumps loading must hold one number per asset ({n_assets}), got {jumps[3]!r}")
        if not (np.all(np.isfinite(np.asarray(jumps[3], np.float64))) and np.all(np.isfinite(loading))):
            raise ValueError(f"jumps loading must be finite, in binary32 too, got {jumps[3]!r}")
    return vals[0], vals[1], vals[2], loading


def check_regimes(regimes, n_assets, factor=False):
    """SPEC.md 2.6 argument rules -> None (no regimes) or (p01, p10, start, mu1 float32 [N], L1 float32 [N, N]).  `regimes` is (p01,
    p10, mu1, cov1) or (p01, p10, mu1, cov1, start); factor=True (the call passed chol=): the fourth entry is regime 1's lower
    Cholesky factor chol1, taken untouched, instead of its covariance.  start=None or absent: the stationary p01 / (p01 + p10), 0 if
    both are 0.  ValueError otherwise (not a sequence of 4 or 5 entries, a bool or a string among the probabilities, a probability
    that is not finite or outside [0, 1], mu1 or cov1 of another shape or not finite, in binary32 too, cov1 not positive definite)."""
    if regimes is None:
        return None
    def msg():                                               # formatted on failure only: the tuple holds arrays
        return f"regimes must be (p01, p10, mu1, cov1) or (p01, p10, mu1, cov1, start), got {regimes!r}"
    if isinstance(regimes, (str, bytes)) or not hasattr(regimes, "__len__") or len(regimes) not in (4, 5):
        raise ValueError(msg())
    n = int(n_assets)
    probs = [regimes[0], regimes[1]] + ([regimes[4]] if len(regimes) == 5 and regimes[4] is not None else [])
    vals = []
    for v in probs:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(msg())
        if not np.isfinite(v) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"regimes p01, p10 and start must be probabilities in [0, 1], got {v!r}")
        vals.append(float(v))
    p01, p10 = vals[0], vals[1]
    start = vals[2] if len(vals) == 3 else (p01 / (p01 + p10) if p01 + p10 > 0 else 0.0)
    try:
        with np.errstate(over="ignore"):
            mu64, c64 = np.asarray(regimes[2], np.float64), np.asarray(regimes[3], np.float64)
            mu1 = np.ascontiguousarray(np.atleast_1d(mu64).astype(np.float32)).ravel()
            c32 = np.atleast_2d(c64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(msg()) from None
    if mu1.size != n or c32.shape != (n, n):
        raise ValueError(f"regimes mu1 must hold {n} numbers and {'chol1' if factor else 'cov1'} be [{n}, {n}], got shapes "
                         f"{np.shape(regimes[2])} and {np.shape(regimes[3])}")
    if not (np.all(np.isfinite(mu64)) and np.all(np.isfinite(c64)) and np.all(np.isfinite(mu1)) and np.all(np.isfinite(c32))):
        raise ValueError("regimes mu1 and cov1 must be finite, in binary32 too")
    L1 = np.ascontiguousarray(np.tril(c32), np.float32) if factor else cholesky_factor(np.atleast_2d(c64))
    return p01, p10, start, mu1, L1


def check_rebalance(rebalance, rebalance_cost):
    """SPEC.md 4.5 argument rules -> (period, cost): period None (constant weights, no rebalancing), 0 (rebalance="never": bought
    and held) or the int k >= 1 of rebalance=k (traded back to the weights every k steps); cost in [0, 1).  ValueError otherwise."""
    if isinstance(rebalance_cost, (bool, np.bool_)) or not isinstance(rebalance_cost, (int, float, np.integer, np.floating)):
        raise ValueError(f"rebalance_cost must be a number in [0, 1), got {rebalance_cost!r}")
    cost = float(rebalance_cost)
    if not 0.0 <= cost < 1.0:
        raise ValueError(f"rebalance_cost must be in [0, 1), got {rebalance_cost!r}")
    if rebalance is None:
        if cost != 0.0:
            raise ValueError("rebalance_cost needs rebalance (an int period >= 1 or 'never'): constant weights trade for free")
        return None, 0.0
    if isinstance(rebalance, str) and rebalance == "never":
        return 0, cost
    if isinstance(rebalance, (bool, np.bool_)) or not isinstance(rebalance, (int, np.integer)) or not 1 <= rebalance <= 2**31 - 1:
        raise ValueError(f"rebalance must be a whole number of steps >= 1 or 'never', got {rebalance!r}")
    return int(rebalance), cost


def check_horizons(horizons, bands, n_steps):
    """SPEC.md 4.3 / 5.2 argument rules -> (steps int32 [H], levels float64 [L]); ValueError otherwise."""
    h = np.asarray(horizons)
    if h.ndim != 1 or h.size < 1 or h.size > _ffi.MCP_MAX_HORIZONS:
        raise ValueError(f"horizons must be a list of 1..{_ffi.MCP_MAX_HORIZONS} steps, got shape {h.shape}")
    if not np.issubdtype(h.dtype, np.integer) and not (np.issubdtype(h.dtype, np.floating) and np.all(h == np.round(h))):
        raise ValueError(f"horizons must be whole steps, got {horizons!r}")
    steps = h.astype(np.int64)
    if steps[0] < 1 or steps[-1] > n_steps or np.any(np.diff(steps) <= 0):
        raise ValueError(f"horizons must be strictly increasing steps in [1, n_steps={n_steps}], got {steps.tolist()}")
    levels = np.asarray(bands, np.float64).ravel()
    if levels.size > _ffi.MCP_MAX_LEVELS:
        raise ValueError(f"at most {_ffi.MCP_MAX_LEVELS} band levels, got {levels.size}")
    if not np.all((levels >= 0.0) & (levels <= 100.0)):
        raise ValueError(f"band levels are percentages in [0, 100], got {levels.tolist()}")
    return steps.astype(np.int32), levels


def mdd_from_raw(qd, compounding="simple") -> np.ndarray:
    """SPEC.md 4.2: the per-path max drawdown in binary64 from the kernel's binary32 q (simple: q - 1) or d (log: expm1(d))."""
    qd = np.asarray(qd, np.float32).astype(np.float64)
    return np.expm1(qd) if compounding == "log" else qd - 1.0


def _close_default_contexts() -> None:
    """Interpreter exit: destroy the cached contexts (streams, device buffers, RCCL communicators) while the HIP runtime
    and the library are still loaded."""
    with _CTX_LOCK:
        for ctx in list(_CTX.values()):
            try:
                ctx.close()
            except Exception:
                pass
        _CTX.clear()


atexit.register(_close_default_contexts)


def default_context(device=0) -> Context:
    """Process-wide context per device (or per tuple of devices)."""
    key = (int(device),) if np.isscalar(device) else tuple(int(d) for d in device)
    with _CTX_LOCK:
        if key not in _CTX:
            _CTX[key] = Context(key)
        return _CTX[key]


def cholesky_factor(cov: np.ndarray) -> np.ndarray:
    """Lower Cholesky factor of Sigma, float64 -> float32.  Raises ValueError if Sigma is not PD
    (e.g. fewer return rows than assets)."""
    cov = np.asarray(cov, np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError(f"cov must be square, got {cov.shape}")
    try:
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"covariance matrix is not positive definite: {e}") from None
    return np.ascontiguousarray(L, np.float32)


def prepare_inputs(mu, cov, weights, chol=None):
    mu = np.ascontiguousarray(mu, np.float32).ravel()
    n = mu.shape[0]
    if not 1 <= n <= _ffi.MCP_MAX_ASSETS:
        raise ValueError(f"n_assets={n} outside [1, {_ffi.MCP_MAX_ASSETS}]")
    L = cholesky_factor(cov) if chol is None else np.ascontiguousarray(np.tril(chol), np.float32)
    if L.shape != (n, n):
        raise ValueError(f"cov/chol shape {L.shape} does not match mu ({n})")
    W = np.ascontiguousarray(np.atleast_2d(np.asarray(weights, np.float32)))
    if W.shape[1] != n:
        raise ValueError(f"weights have {W.shape[1]} columns, expected {n}")
    return mu, L, W


def stats_to_dict(rec) -> dict:
    return {name: (int(rec[name]) if name in ("n", "n_tail") else float(rec[name])) for name in rec.dtype.names}


def drawdown_to_dict(rec) -> dict:
    """The drawdown fields of one mcp_stats record of mcp_simulate_drawdown (SPEC.md 5.1): DaR / CDaR are its var / cvar,
    the worst / best drawdown its min / max."""
    return {"mean": float(rec["mean"]), "std": float(rec["std"]), "dar": float(rec["var"]), "cdar": float(rec["cvar"]),
            "n_tail": int(rec["n_tail"]), "worst": float(rec["min"]), "best": float(rec["max"]),
            "x_lo": float(rec["x_lo"]), "x_hi": float(rec["x_hi"])}


def attribution_to_dict(attr, counts, rec) -> dict:
    """The 'attribution' block of one portfolio (SPEC.md 5.9) from its [N] mcp_attr records, its {n, n_tail} and its mcp_stats
    record: the parts, their shares (0 where the parts sum to 0) and the residuals statistic - sum of parts."""
    mean, cvar, vol = (np.array(attr[f], np.float64) for f in ("mean", "cvar", "vol"))

    def share(parts):
        tot = float(parts.sum())
        return parts / tot if tot != 0.0 else np.zeros_like(parts)
    return {"mean": mean, "cvar": cvar, "vol": vol, "cvar_share": share(cvar), "vol_share": share(vol), "n_tail": int(counts[1]),
            "residual": {"mean": float(rec["mean"]) - float(mean.sum()), "cvar": float(rec["cvar"]) - float(cvar.sum()),
                         "vol": float(rec["std"]) - float(vol.sum())}}


def antithetic_to_dict(rec) -> dict:
    """The 'antithetic' block of one portfolio from its mcp_pair record (SPEC.md 5.10); variance_ratio is the variance of the mean
    over what independent paths would have given, (mean_se / mean_se_iid)^2, 0 when the denominator is 0."""
    se, iid = float(rec["mean_se"]), float(rec["mean_se_iid"])
    return {"n_pairs": int(rec["n_pairs"]), "pair_corr": float(rec["pair_corr"]), "pair_cov": float(rec["pair_cov"]), "mean_se": se,
            "mean_se_iid": iid, "variance_ratio": (se / iid) ** 2 if iid != 0.0 else 0.0}


# Which features of simulate_paths combine: per feature, what it needs (the head of the refusal), the names it is not combined
# with, and whether the refusal lists the offending names only (True) or all of them as one fixed sentence (False).  A name is a
# keyword -- given when it is not None, or true for a flag -- or keyword='value'.  The rows stand in the order the rules are
# checked, so the same rule wins when two apply.  The C side states the same rules for the library (check_request).
_FLAGS = ("drawdown", "attribution", "antithetic", "fold", "native_math", "lifetime", "underwater")
_PATHS_COMBINE = {
    # SPEC.md 5.22: a reduction of what the call stores anyway, so no name is excluded
    "downside": ("downside reads the values of whatever walk the call runs", (), True),
    # SPEC.md 5.23: likewise, but every row needs the benchmark's beside it -- nothing is excluded but what splits the portfolios
    "benchmark": ("benchmark needs every portfolio and the benchmark's on the same shard", ("shard='portfolios'",), True),
    "drift_uncertainty": ("drift_uncertainty needs Gaussian draws, constant weights, the spec's normals and the unfolded recurrence",
                          ("underwater", "vol_target", "tolerance", "spending", "protect", "glide", "regimes", "jumps", "garch", "dof",
                           "rebalance", "overlay", "attribution", "antithetic", "lifetime", "fold", "native_math"), True),
    "underwater": ("underwater=True needs the drawdown walk on Gaussian, Student-t, GARCH or jump draws, the spec's normals and the unfolded "
                   "recurrence",
                   ("vol_target", "tolerance", "spending", "protect", "glide", "regimes", "rebalance", "cashflow", "overlay", "attribution",
                    "antithetic", "lifetime", "horizons", "fold", "native_math"), True),
    "vol_target": ("vol_target needs constant weights, simple compounding, the spec's normals and the unfolded recurrence",
                   ("tolerance", "spending", "protect", "glide", "regimes", "rebalance", "cashflow", "overlay", "attribution", "antithetic",
                    "lifetime", "fold", "native_math", "compounding='log'"), True),
    "tolerance": ("tolerance needs the rebalancing walk -- Gaussian draws, simple compounding, the spec's normals and the unfolded recurrence",
                  ("drawdown", "cashflow", "glide", "protect", "spending", "overlay", "dof", "garch", "jumps", "regimes", "attribution",
                   "antithetic", "fold", "native_math", "compounding='log'"), True),
    "spending": ("spending needs the cashflow walk without a schedule -- constant weights, simple compounding, the spec's normals and the "
                 "unfolded recurrence",
                 ("cashflow", "glide", "protect", "drawdown", "rebalance", "overlay", "garch", "jumps", "regimes", "attribution", "antithetic",
                  "fold", "native_math", "compounding='log'"), True),
    "protect": ("protect needs constant weights, simple compounding, the spec's normals and the unfolded recurrence",
                ("rebalance", "cashflow", "overlay", "regimes", "glide", "attribution", "antithetic", "fold", "native_math",
                 "compounding='log'"), True),
    "glide": ("glide needs the cashflow walk -- simple compounding, the spec's normals and the unfolded recurrence",
              ("drawdown", "rebalance", "overlay", "garch", "attribution", "antithetic", "jumps", "regimes", "fold", "native_math",
               "compounding='log'"), True),
    "regimes": ("regimes need Gaussian draws, constant weights, simple compounding, the spec's normals and the unfolded recurrence",
                ("dof", "garch", "jumps", "rebalance", "cashflow", "overlay", "attribution", "antithetic", "fold", "native_math",
                 "compounding='log'"), True),
    "jumps": ("jumps need Gaussian draws, constant weights, simple compounding, the spec's normals and the unfolded recurrence",
              ("dof", "garch", "rebalance", "cashflow", "overlay", "attribution", "antithetic", "fold", "native_math",
               "compounding='log'"), True),
    "antithetic": ("antithetic needs constant weights, the spec's normals, the unfolded recurrence and path shards",
                   ("rebalance", "cashflow", "overlay", "attribution", "fold", "native_math", "shard='portfolios'"), True),
    "attribution": ("attribution needs constant weights, simple compounding, the spec's normals, the unfolded recurrence and path shards",
                    ("drawdown", "horizons", "rebalance", "cashflow", "overlay", "fold", "native_math", "compounding='log'",
                     "shard='portfolios'"), True),
    "garch": ("garch needs simple compounding, the spec's normals, the unfolded recurrence and constant weights",
              ("rebalance", "cashflow", "overlay", "fold", "native_math", "compounding='log'"), False),
    "overlay": ("overlay needs simple compounding, the spec's normals, the unfolded recurrence and constant weights",
                ("rebalance", "cashflow", "fold", "native_math", "compounding='log'"), False),
    "cashflow": ("cashflow needs simple compounding, the spec's normals, the unfolded recurrence and constant weights",
                 ("drawdown", "rebalance", "fold", "native_math", "compounding='log'"), False),
    "dof": ("dof needs simple compounding, the spec's normals, the unfolded recurrence and constant weights",
            ("fold", "native_math", "rebalance", "compounding='log'"), False),
    "rebalance": ("rebalance needs the spec's normals and the unfolded recurrence", ("drawdown", "fold", "native_math"), False),
    "drawdown": ("drawdown=True needs the spec's normals and the unfolded recurrence", ("fold", "native_math"), False),
    "horizons": ("horizons need the spec's normals and the unfolded recurrence", ("drawdown", "fold", "native_math"), False),
}
# simulate_bootstrap: the same two features on observed rows
_BOOTSTRAP_COMBINE = {
    "tolerance": ("tolerance needs the rebalancing walk and simple compounding",
                  ("cashflow", "glide", "spending", "compounding='log'"), True),
    "spending": ("spending needs the cashflow walk without a schedule, constant weights and simple compounding",
                 ("cashflow", "glide", "rebalance", "compounding='log'"), True),
    "glide": ("glide needs the cashflow walk and simple compounding", ("rebalance", "compounding='log'"), False),
    "cashflow": ("cashflow needs simple compounding and constant weights", ("rebalance", "compounding='log'"), False),
}


def _check_benchmark(benchmark, weights, as_array, shard):
    """The `benchmark` keyword of simulate_paths, simulate_bootstrap and simulate_filtered -> None or the row (relative.check_benchmark),
    with the two refusals that need no device (SPEC.md 5.23)."""
    from .relative import check_benchmark
    bm = check_benchmark(benchmark, 1 if np.ndim(weights) < 2 else np.shape(weights)[0])
    if bm is not None and as_array:
        raise ValueError("benchmark fills the 'relative' block of the result dicts: not with as_array")
    _check_combines(_PATHS_COMBINE, "benchmark", dict(benchmark=bm, shard=shard))
    return bm


def _given(name, kw):
    """Whether the call's keywords `kw` hold `name` (a row of _PATHS_COMBINE explains the names)."""
    if "=" in name:
        key, value = name.split("=")
        return kw[key] == value.strip("'")
    return bool(kw[name]) if name in _FLAGS else kw[name] is not None


def _check_combines(table, feature, kw):
    """ValueError if `feature` is given together with a name its row of `table` excludes."""
    head, names, listed = table[feature]
    bad = [name for name in names if _given(name, kw)] if _given(feature, kw) else []
    if bad:
        raise ValueError(f"{head}: not with " + (", ".join(bad) if listed else ", ".join(names[:-1]) + " or " + names[-1]))


def simulate_paths(mu, cov, weights, n_steps=252, n_paths=10_000, seed=0, v0=1.0, compounding="simple",
                   rf=0.0, alpha=0.95, devices=None, store=False, path_begin=0, chol=None,
                   native_math=False, as_array=False, fold=False, shard="auto", context=None, drawdown=False,
                   horizons=None, bands=(), rebalance=None, rebalance_cost=0.0, dof=None, cashflow=None, target=None,
                   overlay=None, spot=None, garch=None, attribution=False, antithetic=False, jumps=None, regimes=None, glide=None,
                   protect=None, spending=None, lifetime=False, lifetime_levels=(5, 25, 50), tolerance=None, tolerance_levels=(5, 50, 95),
                   vol_target=None, underwater=False, underwater_levels=(50, 95), drift_uncertainty=None, downside=None, benchmark=None):
    """Simulate `n_paths` correlated return paths and reduce them to risk statistics.

    mu [N], cov [N,N] are per-step mean and covariance (the reference's `mean_returns`, `cov_matrix`
    of app.py:679-680 divided by `annual_factor`); weights [N] or [K,N].  Returns a dict for a single
    weight vector or a list of dicts for K portfolios (as_array=True: the [K] record array of mcp_stats
    instead); with store=True the dict carries 'terminal' (float32 [n_paths] or [K, n_paths]).

    devices: None / [d] -> one GPU; [d0, d1, ...] -> the path range sharded over those GPUs inside the library (RCCL
    all-reduce of the radix-select histograms, one all-gather of the moment records).
    shard="portfolios" (or "auto" with K >= 512 per device) shards the weight matrix instead: every GPU walks all
    paths for its slice of the portfolios, no collective at all (BASELINE configs[4]).

    drawdown=True: also the max drawdown of every path (SPEC.md 4.2), tracked inside the path kernel, reduced per portfolio
    (SPEC.md 5.1): every dict gains 'drawdown' {mean, std, dar, cdar, n_tail, worst, best, x_lo, x_hi} and, with store=True,
    'max_drawdown' (float64 per-path drawdowns).  as_array=True returns (stats, dd_stats) [+ (terminal, max_drawdown) with
    store].  Not with fold or native_math (ValueError).

    horizons=[h_1 < ... < h_H] (steps in [1, n_steps], at most 64), bands=(q_1, ...) (percentages, at most 16): also the value of
    every path after step h (SPEC.md 4.3: bit for bit the terminal value of the same call with n_steps = h) and, per horizon,
    the statistics of x_h = V_h/v0 - 1 (log: expm1(S_h)) at alpha and np.percentile(x_h, q) for every level (SPEC.md 5.2).
    Every dict gains 'horizons' {steps, levels, bands [H, L], mean, std, var, cvar, min, max, n_tail [H]} and, with store=True,
    'horizon_terminal' (float32 [H, n_paths], raw V_h / S_h).  as_array=True returns (stats, hz_stats [H, K], bands [H, K, L])
    [+ (terminal, horizon_terminal [H, K, n_paths]) with store].  Not with drawdown, fold or native_math (ValueError).

    rebalance=None (default): constant weights, the portfolio traded back to `weights` after every step for free (SPEC.md 4).
    rebalance=k (int >= 1): the holdings drift with the prices and are traded back to `weights` every k steps; rebalance="never":
    bought and held; rebalance_cost: the proportional cost in [0, 1) of the fraction traded, paid out of the portfolio (SPEC.md
    4.5, simple compounding only).  The result has the shape of the same call without it, horizons and bands included (pivots of
    SPEC.md 5.4); rebalance=1 with no cost gives the constant-weight values bit for bit, on the rebalancing kernel.  Not with
    drawdown, fold, native_math or compounding="log" (ValueError).

    dof=None (default): Gaussian steps r = mu + L z.  dof=nu (an int in [3, 32]): multivariate Student-t steps with nu degrees
    of freedom, r = mu + L s z with one s = sqrt((nu - 2) / chi2_nu) per path and step shared by all assets (SPEC.md 2.2 / 4.6):
    the same mean and covariance as the Gaussian call, fat tails, assets that crash together, and the Gaussian call's own z
    (common random numbers with the same seed).  The result has the shape of the same call without it, drawdown and horizons
    blocks included (pivots of SPEC.md 5).  fit_student_t_dof(returns) estimates nu from return rows.  Not with fold,
    native_math, rebalance or compounding="log" (ValueError).

    cashflow=None (default): the paths are left alone.  cashflow=c (a number): c is paid in (c > 0) or taken out (c < 0), in the
    units of v0, at the end of every step; cashflow=[c_1, ..., c_T]: a schedule of exactly n_steps amounts (rounded to binary32).
    A path whose value is not positive after a flow is ruined: it is stored as 0 and stays there (SPEC.md 4.7).  target=g: also
    count the paths below g.  Every dict gains 'cashflow' {contributed (the binary64 sum of the flows), n_ruined,
    ruin_probability} plus n_short, shortfall_probability with a target, and the 'horizons' block n_ruined, ruin_probability [H]
    (the survival curve; plus the two shortfall arrays with a target).  The statistics are those of x = V_T/v0 - 1, terminal
    wealth over the INITIAL value: with flows this is not a return on the capital paid in -- form one from 'contributed'.
    as_array=True returns the tuple of the same call without cash flows with counts [K, 2] uint64 {n_ruined, n_short} (and
    hz_counts [H, K, 2] with horizons) appended.  Combines with dof and horizons / bands; not with drawdown, rebalance, fold,
    native_math or compounding="log", and target needs cashflow (ValueError).

    overlay=None (default): every asset contributes its own return.  overlay={i: rows} (or a list of N row lists), spot=[N current
    prices]: asset i is held through the option strategy `rows` -- the tuples (row_type, strike, premium, qty) of
    options.strategy_rows, strike and premium in price units -- exactly as the reference replaces an asset's return series by
    options.calc_options_series before anything else is computed: inside the path kernel every step's return of asset i becomes
    sum_rows qty * leg(price, prev) / prev at the price level of that path (SPEC.md 4.8), the options struck again every step as
    in the reference.  The result has the shape of the same call without it (drawdown, horizons / bands, dof, store and as_array
    all combine; pivots of SPEC.md 5.7); an overlay without rows gives the plain call's values bit for bit.  Not with rebalance,
    cashflow, fold, native_math or compounding="log" (ValueError).

    garch=None (default): every step's covariance is `cov`.  garch=(alpha, beta) or (alpha, beta, h0): volatility clustering, a
    scalar GARCH(1,1) on the covariance (SPEC.md 4.9): step t draws with the covariance h_t cov, one variance ratio h per path,
    h_{t+1} = (1 - alpha - beta) + alpha (eps_t' cov^-1 eps_t / N) + beta h_t from h0 (default 1: the long-run level; h0 != 1
    starts the paths "from today's volatility", E[h_t] = 1 + (alpha + beta)^t (h0 - 1)).  The conditional mean of every step is mu
    (pivots of SPEC.md 5.8) and the asset normals are the Gaussian call's own; alpha = 0, h0 = 1 is the call without it bit for
    bit.  fit_garch(returns)[:3] estimates the triple from return rows.  The result has the shape of the same call without it
    (drawdown, horizons / bands, dof, store and as_array all combine).  Not with rebalance, cashflow, overlay, fold, native_math or
    compounding="log" (ValueError).

    attribution=False (default): the statistics say how risky a portfolio is.  attribution=True: also which holding the risk comes
    from (SPEC.md 4.10 / 5.9).  After the call's statistics are known the same paths are walked a second time, one portfolio per pass,
    carrying next to the value the money A_i every asset made or lost along the path (sum_i A_i = V_T - v0); nothing per step is
    stored.  Every dict gains 'attribution' {mean, cvar, vol (float64 [N]: the asset's parts of the portfolio's mean, CVaR and
    standard deviation, which add up to them -- component CVaR and component volatility), cvar_share, vol_share (the parts over
    their sum: the risk pie), n_tail, residual {mean, cvar, vol} (the statistic minus the sum of its parts: binary32 rounding of the
    walk, bounded in SPEC.md 6)} and, with store=True, 'contributions' (float32 [N, n_paths], the A_i of every path).
    as_array=True appends (attr [K, N] records of _ffi.ATTR_DTYPE, counts [K, 2] uint64 {n, n_tail}) and, with store,
    contributions [K, N, n_paths].  Combines with dof, garch, store, as_array and devices (path shards), for at most 16 portfolios;
    the statistics and the stored terminal values are bit for bit those of the call without it.  Costs one more walk per portfolio.
    Not built: attribution with drawdown, horizons, rebalance, cashflow, overlay, fold, native_math, compounding="log",
    shard="portfolios" or more than 16 portfolios (ValueError), on bootstrap paths (simulate_bootstrap), in simulate_sweep (call
    simulate_paths for the optimum), in PathEngine and at the mcp_launch_* level.

    antithetic=False (default): independent paths.  antithetic=True: antithetic pairs (SPEC.md 2.3 / 5.10; n_paths and path_begin
    even).  The paths 2j and 2j + 1 share every draw of path j of the call without it and path 2j + 1 sees the asset normals negated
    (the Student-t scale and the GARCH variance are shared), so the pair's returns are strongly negatively correlated and the mean
    -- what Sharpe ranks on -- is far more accurate than n_paths independent paths give; tail statistics gain less.  Every
    statistic is the usual one over all n_paths values.  Every dict gains 'antithetic' {n_pairs, pair_corr, pair_cov, mean_se (the
    standard error of the mean, from the n_paths / 2 independent pair means: std / sqrt(n) is wrong for such a sample), mean_se_iid
    (std / sqrt(n), what independent paths would have given), variance_ratio (their ratio squared)}.  as_array=True appends the [K]
    record array of _ffi.PAIR_DTYPE last.  A kernel lane walks both members on one set of draws.  Combines with dof, garch,
    drawdown, horizons / bands, store, as_array, devices (path shards, cut at even path ids) and compounding="log" on Gaussian
    draws.  Not built: antithetic with rebalance, cashflow, overlay, attribution, fold, native_math or shard="portfolios"
    (ValueError), on bootstrap paths (observed rows have no sign to flip), in simulate_sweep (call simulate_paths for the
    optimum), in PathEngine and at the mcp_launch_* level.

    jumps=None (default): every step is Gaussian around mu.  jumps=(intensity, mean, std) or (intensity, mean, std, loading): Merton
    jump-diffusion (SPEC.md 2.5 / 4.12).  Every path-step also takes a market jump J, the sum of n normal(mean, std^2) jumps with n
    ~ Poisson(intensity) (0 <= intensity <= 1 expected jumps per step, at most 8 in one step), and asset i moves by loading_i J
    (default: all ones): with a negative mean the assets fall harder than they rise, fall together, and fall within one step --
    what VaR, CVaR, the drawdown and the lower fan band are most sensitive to.  mu stays the mean of every step (the drift is
    compensated, pivots of SPEC.md 5.12) and `cov` stays the TOTAL per-step covariance: the diffusion is factored from
    jumps.diffusion_cov(cov, jumps) = cov - Var(J) b b' (ValueError when that is not positive definite), so the call has the
    Gaussian call's mean and covariance and differs in skew and tails; an explicit chol= is taken as the diffusive factor
    untouched.  The asset normals are the Gaussian call's own (common random numbers with the same seed); intensity = 0 is the call
    without it bit for bit.  fit_jumps(returns) estimates the triple and the loadings from return rows.  The result has the shape of
    the same call without it (drawdown, horizons / bands, store, as_array, devices and shard all combine); every dict gains 'jumps'
    {intensity, mean_count (the mean of the count the kernels draw), variance_share (the jump's share of the portfolio's one-step
    variance)}.  Not built: jumps with dof, garch, rebalance, cashflow, overlay, attribution, antithetic, fold, native_math or
    compounding="log" (ValueError), on bootstrap or filtered paths (the rows carry their own jumps), in PathEngine and at the
    mcp_launch_* level; jumps with cashflow -- ruin under crash risk -- is the obvious next step.

    regimes=None (default): one mean and one covariance for the whole walk.  regimes=(p01, p10, mu1, cov1) or (p01, p10, mu1, cov1,
    start): two-regime Markov switching (Hamilton 1989; SPEC.md 2.6 / 4.13).  Every path carries a regime, 0 (calm) or 1 (crisis),
    that moves once per step with P(0 -> 1) = p01 and P(1 -> 0) = p10; a step in regime 0 draws r = mu + L z, a step in regime 1
    r = mu1 + L1 z: `mu` and `cov` are regime 0, mu1 [N] and cov1 [N, N] regime 1 (factored in float64 like cov; ValueError when it
    is not positive definite) -- a crisis that lasts 1 / p10 steps on average, in which means, volatilities and correlations all
    change.  start = P(regime 1 in the first step), default the stationary p01 / (p01 + p10) (0 if both are 0).  With an explicit
    chol= the fourth entry is read the same way: regimes=(p01, p10, mu1, chol1[, start]), chol1 the lower Cholesky factor of regime 1,
    taken untouched as chol is.  All portfolios and assets of a path share its regime.  The asset normals are the Gaussian call's own
    (common random numbers with the same seed); identical regimes, or start = 0 with p01 = 0, are the Gaussian call bit for bit.
    regimes.fit_regimes(returns) estimates everything from return rows, its `start` from the last row ("today's regime").  The
    result has the shape of the same call without it (drawdown, horizons / bands, store, as_array, devices and shard all combine); every
    dict gains 'regimes' {p01, p10, start: as the kernels use them (multiples of 2^-32), stationary: the long-run probability of
    regime 1, mean_duration: (1 / p01, 1 / p10) expected steps in regime 0 and 1 (inf where the probability is 0) and, with
    horizons, occupancy: per horizon h the expected share of the first h steps walked in regime 1}.  Not built: regimes with dof,
    garch, jumps, rebalance, cashflow, overlay, attribution, antithetic, fold, native_math or compounding="log" (ValueError), on
    bootstrap or filtered paths, in PathEngine and at the mcp_launch_* level.

    glide=None (default): the weights are held from the first step to the last.  glide=(breaks, targets): a glide path, target
    weights on a calendar (SPEC.md 4.14 / 5.14) -- target-date funds, "100 minus age", de-risking before the goal.  breaks: at most
    64 strictly increasing steps in [1, n_steps - 1]; targets: the weights held after each break, [G, N] for a weight vector and
    [K, G, N] for K portfolios (glide.glide_path(start, end, n_steps, every) builds a linear one).  `weights` is held through step
    breaks[0], targets[0] through step breaks[1], and so on; the portfolio stands at its current target at the start of every step,
    and the trade at a break is free (holdings that drift between breaks are rebalance's subject, not built together).  The walk is
    the cashflow walk -- the same draws, flows and absorbing ruin -- so glide with cashflow=None is the call with cashflow=0 and the
    result has that call's shape, 'cashflow' block and as_array tuple included; every dict gains 'glide' {breaks, weights (float32
    [G + 1, N] as used, segment 0 = weights)}.  Targets equal to the weights give the cashflow call bit for bit.
    glide.glide_law(mu, cov, weights, glide, n_steps) is the exact mean and variance for Gaussian draws without flows.  Combines
    with cashflow / target, dof, horizons / bands, store, as_array, devices and bootstrap rows (simulate_bootstrap).  Not built:
    glide with drawdown, rebalance, overlay, garch, attribution, antithetic, jumps, regimes, fold, native_math or
    compounding="log" (ValueError), on filtered rows, in simulate_sweep, in PathEngine and at the mcp_launch_* level.

    protect=None (default): the whole value rides the weights.  protect=(floor, multiplier[, rate[, cap[, ratchet]]]): floor
    protection inside the walk (SPEC.md 4.15 / 5.15) -- CPPI: before every step, multiplier times the cushion V - F above the floor
    F is held in the portfolio `weights`, at most cap times V (default 1: no leverage), never less than 0, and the rest earns the
    riskless `rate` per step (default 0).  floor: a fraction of v0 that grows at `rate` (0.8: never lose more than 20 %), or an
    explicit sequence of n_steps + 1 floors.  ratchet (default 0) in [0, 1): the floor is also at least ratchet times the running
    peak of V -- TIPP, drawdown control.  The allocation reacts to the path, the draws are the call's own; floor 0, ratchet 0, cap 1
    and multiplier >= 1 is the call without it bit for bit.  Under small Gaussian steps the floor holds; under jumps or dof it can be
    gapped through, and every dict gains 'protect' {floor (float32 [n_steps + 1] as used), multiplier, cap, rate, ratchet, target,
    n_gap, gap_probability (paths that end below the floor), n_short, shortfall_probability (below `target`; 0 without one) and,
    with horizons, 'horizons' {the same four, [H], against the floor of that step}}.  as_array=True appends counts [K, 2] uint64
    {n_gap, n_short} (and hz_counts [H, K, 2] with horizons).  protect.protect_law(mu, cov, weights, n_steps, protect) is the exact
    mean and variance on Gaussian draws while neither the cap, a gap nor the ratchet acts.  Combines with dof, garch, jumps,
    drawdown or horizons / bands, store, target, as_array and devices.  Not built: protect with rebalance, cashflow, overlay,
    regimes, glide, attribution, antithetic, fold, native_math or compounding="log" (ValueError), on bootstrap or filtered rows, in
    simulate_sweep, in PathEngine and at the mcp_launch_* level.

    spending=None (default): the only withdrawals are cashflow's, fixed before the first draw.  spending=(rate, every, down, up[,
    inflation[, first]]): a withdrawal that reacts to the path (SPEC.md 4.16 / 5.16).  Every step pays out the current amount w, from
    `first` (default rate times v0); every `every` steps w is inflated by `inflation` and then moved to rate times the current
    value, but cut by at most the share `down` and raised by at most the share `up` (inf: no ceiling).  every=0 or down=up=0 is the
    constant inflation-adjusted amount ("4 % rule"), every=1, down=1, up=inf the fixed percentage of the value, anything between a
    floor-and-ceiling rule (spending.spending_rule names the three).  Ruin is absorbing as in cashflow; the step of ruin pays out
    what is left.  `target` is then the rule's second count.  The result has the shape of the call without it plus 'spending'
    {rate, every, growth, lo, hi, first (binary32 as used), target, n_ruined, ruin_probability[, n_short, shortfall_probability],
    horizons {the same per horizon}, withdrawn {the mcp_stats fields of x_Y = Y_T / v0 - 1 at alpha, and mean_v0 / var_v0 / cvar_v0 =
    x + 1, the payout as a multiple of v0}} and, with store=True, 'withdrawn' float32 [n_paths], the total paid out per path;
    as_array appends counts[, hz_counts], wd_stats[, withdrawn].  With every=0 the values are those of cashflow=-first bit for bit.
    spending.spending_law is the exact law of the pure percentage rule.  Combines with dof, horizons / bands, target, store, as_array,
    devices and bootstrap rows (simulate_bootstrap).  Not built: spending with cashflow, glide, protect, drawdown, rebalance, overlay,
    garch, jumps, regimes, attribution, antithetic, fold, native_math or compounding="log" (ValueError), on filtered rows, in
    simulate_sweep, in PathEngine and at the mcp_launch_* level.

    lifetime=False (default): ruin is a count at the end and at the horizons.  lifetime=True, with cashflow (with or without glide) or
    spending: how long the money lasts (SPEC.md 4.17 / 5.17).  The walk counts per path the steps l that ended with money left: l ==
    n_steps is a path not ruined inside the horizon, l < n_steps one ruined in step l + 1.  Everything else the call returns is that
    of the call without it, bit for bit.  Every dict gains 'lifetime' {histogram uint64 [n_steps + 1] (#{l == s}), survival float64
    [n_steps + 1] (the share of paths with l >= s; 1 - survival[h] is the ruin probability at h), mean (the restricted mean lifetime
    in steps), quantiles {level: steps} for lifetime_levels in percent (np.percentile(l, q, method="lower"): 5 -> the lifetime that
    95 % of the paths exceed or meet), n_ruined and, with store=True, steps uint32 [n_paths]}; as_array appends life_hist, life_sum,
    life_q[, life].  All integers are exact and independent of devices and tiles.  Not built: lifetime without cashflow or spending
    (a walk without ruin; glide alone included), with protect, drawdown, rebalance, overlay, garch, jumps, regimes, attribution or
    antithetic (ValueError), on filtered rows, in simulate_sweep, in PathEngine and at the mcp_launch_* level.

    tolerance=None (default): `rebalance` trades on the calendar.  tolerance=a number, [N], [K, N] or tolerance_bands(...): tolerance-band
    rebalancing (SPEC.md 4.18 / 5.18).  `rebalance` becomes the review period (None: every step; "never": no review): at a review a
    path is traded back to `weights`, at rebalance_cost, only when an asset's weight is off its target by its tolerance or more (inf: the
    asset is not watched); a path inside its bands changes nothing.  tolerance=0 is rebalance=k bit for bit, tolerance=inf is
    rebalance="never".  Every dict gains 'tolerance' {every, n_reviews, table float64 [N], trades {hist uint64 [n_reviews + 1] (#{c ==
    s}), mean, q {level: trades} for tolerance_levels in percent (np.percentile(c, q, method="lower")) and, with store=True, paths uint32
    [n_paths]}, turnover {mean, std, var, cvar, min, max, n_tail, x_lo, x_hi of the total two-sided fraction of value traded per path
    and, with store=True, paths float32 [n_paths]}}; as_array appends trade_hist, trade_sum, trade_q, turnover_stats (over Y - 1)[,
    trades, turnover].  The counts are exact and independent of devices and tiles.  Every portfolio is a walk of its own: K portfolios
    cost K walks.  Combines with horizons / bands, store, as_array, devices, path_begin and bootstrap rows (simulate_bootstrap).  Not
    built: tolerance with drawdown, cashflow, glide, protect, spending, overlay, dof, garch, jumps, regimes, attribution, antithetic, fold,
    native_math or compounding="log" (ValueError), on filtered rows, in simulate_sweep, in PathEngine and at the mcp_launch_* level.

    vol_target=None (default): the whole value rides the weights.  vol_target=(target, decay[, cap[, rate[, spread[, s0]]]]): volatility
    targeting inside the walk (SPEC.md 4.19 / 5.19) -- before every step the exposure to the weights is e = min(target / sqrt(s), cap),
    s an exponentially weighted average of the path's own squared portfolio returns (decay = voltarget.ewma_decay(halflife); it starts
    at s0, by default the variance w' cov w of the Gaussian part); the rest of the value earns `rate` per step, what is borrowed above
    the value (cap > 1) pays rate + spread, and a path that loses everything is ruined for good.  The draws, the drawdown and the
    horizons are those of the same call without it, on the targeted value.  With cap=1 and a target that always binds the cap the
    stored values are the plain call's bit for bit.  Every dict gains 'vol_target' {target, decay, one_minus_decay, cap, rate, spread
    (binary32, as used), s0, exposure0 (the first step's exposure), target_value, n_ruined, ruin_probability, n_short,
    shortfall_probability (below `target`; 0 without one), with horizons the same per horizon and, without drawdown, exposure {mean,
    std, quantile (at level 1 - alpha), level, min, max of the per-path average exposure and, with store=True, paths float32
    [n_paths]: the per-path SUM of the exposures}}; as_array appends counts[, hz_counts] and, without drawdown, exposure_stats (over
    Y - 1)[, exposure].  voltarget.vol_target_law is the exact law of a constant exposure.  Combines with dof, garch, jumps (alone),
    drawdown or horizons / bands, target, store, as_array, devices and shard="portfolios".  Not built: vol_target with tolerance,
    spending, protect, glide, regimes, rebalance, cashflow, overlay, attribution, antithetic, lifetime, fold, native_math or
    compounding="log" (ValueError), on bootstrap or filtered rows, in simulate_sweep, in PathEngine and at the mcp_launch_* level.

    underwater=False (default): the drawdown says how deep a path falls, not for how long.  underwater=True, with drawdown=True: the time
    under water (SPEC.md 4.20 / 5.20) -- per path the longest run m of consecutive steps strictly below the running peak and the steps
    c_T since the last peak at the horizon (0: the path ends at its high-water mark), two uint32 counters on the drawdown walk; every
    other output is that of the call without it, bit for bit.  Every dict gains 'underwater' {longest and current, each {hist uint64
    [n_steps + 1] (#{. == s}), mean (steps), levels {level: steps} for underwater_levels in percent (np.percentile(., q,
    method="lower")), with store steps uint32 [n_paths]}, p_under_water_at_end (1 - hist_c[0] / n)}; as_array appends longest_hist,
    current_hist, sums [K, 2], q [K, 2, L][, longest, current].  All integers are exact and independent of devices and tiles.
    underwater.spell_law gives the two distribution-free probabilities of a symmetric walk.  Combines with dof, garch, jumps (alone),
    compounding="log" (Gaussian draws), store, as_array, devices and shard="portfolios".  Not built: underwater without drawdown, with
    vol_target, tolerance, spending, protect, glide, regimes, rebalance, cashflow, overlay, attribution, antithetic, lifetime, horizons,
    fold or native_math (ValueError), on bootstrap or filtered rows, in simulate_sweep, in PathEngine and at the mcp_launch_* level.

    drift_uncertainty=None (default): every path walks on `mu` as if it were known.  drift_uncertainty=n_obs | cov_of_drift |
    ("factor", M): estimation risk inside the walk (SPEC.md 2.7 / 4.21 / 5.21) -- `mu` is a sample mean, so every path draws its own
    drift once, m = mu + M g with g ~ N(0, I), and compounds on it at every step.  A positive number n_obs takes M = chol(cov) /
    sqrt(n_obs), the standard error of a mean over n_obs observed steps; an [N, N] matrix is the covariance of the drift itself
    (uncertainty.drift_cov(returns)), factored here; ("factor", M) is a lower-triangular factor used as given, zeros allowed.  The
    draws of the steps are those of the same call without it (common random numbers), and with M = 0 every stored value is that
    call's, bit for bit.  The fan of `horizons` and the ruin probability of `cashflow` widen: the variance of the log value gains
    h^2 b_k on top of h a_k.  Every dict gains 'drift_uncertainty' {drift_std (sqrt(b_k), the standard deviation of the portfolio's
    drift), log_variance_share (T b_k / (a_k + T b_k)) and, with horizons, horizon_log_variance_share}; as_array returns what the
    call without it returns.  uncertainty.drift_law gives the exact laws.  Combines with drawdown, horizons / bands,
    compounding="log", cashflow and target, store, as_array, devices and shard="portfolios".  Not built: drift_uncertainty with
    underwater, vol_target, tolerance, spending, protect, glide, regimes, jumps, garch, dof, rebalance, overlay, attribution,
    antithetic, lifetime, fold or native_math (ValueError), on bootstrap or filtered rows, in simulate_sweep, in PathEngine and at
    the mcp_launch_* level.

    downside=None (default): the statistics above say how wide the distribution is and how bad its tail, not how it is shaped.
    downside=True | tau: one more streaming reduction over the values the call keeps on the device anyway (SPEC.md 5.22), whatever
    walk produced them and with or without `store`.  tau is the threshold in units of x, True takes rf (the reference subtracts
    risk_free before it looks at the sign, app.py:238-243).  Every dict gains 'downside' {sortino (the reference's ratio: (mean -
    tau) / downside_std, not annualised), downside_std (np.std(ddof=1) of the excess returns below zero; 1e-4 when there are none,
    NaN for one), downside_deviation (the target semideviation sqrt(mean min(x - tau, 0)^2)), sortino_target (on that deviation),
    p_below (the probability of x < tau: of a loss at tau = 0), mean_shortfall (mean of x - tau over those paths), omega (gains over
    losses about tau), skewness, excess_kurtosis (population forms, scipy.stats' defaults), mean, threshold, sums (the raw record)}
    and, with horizons, 'horizons': a list of the same dicts per horizon, so that p_below runs along the fan.  Every other entry of
    the result is the call's without the keyword, bit for bit.  downside.normal_law gives the exact figures of a normal x.  Combines
    with every other keyword, devices and shard="portfolios".  Not with as_array (the records live in the dicts; ValueError), in
    simulate_sweep, in PathEngine; mcp_launch_downside is the enqueue-only form.

    benchmark=None (default): every statistic above describes one portfolio alone.  benchmark=b, an integer row of `weights`: every
    portfolio against that row on the same paths (SPEC.md 5.23) -- one more streaming reduction over the values the call keeps on
    the device, two rows at a time, whatever walk produced them.  With a = x_k - x_b the active return of a path, every dict gains
    'relative' {active_mean, tracking_error (np.std(a, ddof=1)), information_ratio (their quotient, not annualised), p_under and
    p_over (the probability of ending behind / ahead; ties in neither), mean_underperformance (mean of a over the paths behind),
    relative_downside_deviation (sqrt(mean min(a, 0)^2)), beta, alpha (mean_k - beta mean_b), correlation, up_capture and
    down_capture (sum of x_k over sum of x_b on the paths where the benchmark gains / loses), pivot, bench_pivot, benchmark, sums (the
    raw record), active {mean, std, var, cvar, n_tail, worst, best}: the statistics of the stored binary32 Y = 1 + a over Y - 1 at the
    call's alpha, so var / cvar are the relative VaR / CVaR; with store=True also 'y', the [n_paths] row of Y} and, with horizons,
    'horizons': the finished fields per horizon against the benchmark's row of that horizon.  A quotient whose denominator is 0 is 0;
    the benchmark's own row has tracking_error 0, beta 1, captures 1.  Every other entry of the result is the call's without the
    keyword, bit for bit.  relative.relative_law gives the exact figures of a one-step Gaussian pair.  Combines with every other
    keyword, `downside` included, and with devices; all portfolios must fit one tile: not with shard="portfolios" (ValueError), not
    under a terminal budget that cuts K (McpError).  ValueError for a bool, a float, a row outside `weights` and with as_array.  Not in
    simulate_sweep or PathEngine; mcp_launch_relative is the enqueue-only form.
    """
    from .downside import check_downside
    ds = check_downside(downside)
    if ds is not None and as_array:
        raise ValueError("downside fills the 'downside' block of the result dicts: not with as_array")
    bm = _check_benchmark(benchmark, weights, as_array, shard)
    if drift_uncertainty is not None:
        return _simulate_uncertain(mu, cov, weights, n_steps, n_paths, seed, v0, compounding, rf, alpha, devices, store, path_begin, chol,
                                   native_math, as_array, fold, shard, context, drawdown, horizons, bands, rebalance, rebalance_cost, dof,
                                   cashflow, target, overlay, spot, garch, attribution, antithetic, jumps, regimes, glide, protect, spending,
                                   lifetime, tolerance, vol_target, underwater, drift_uncertainty, ds, bm)
    if not isinstance(underwater, (bool, np.bool_)):
        raise ValueError(f"underwater must be True or False, got {underwater!r}")
    if underwater:
        return _simulate_underwater(mu, cov, weights, n_steps, n_paths, seed, v0, compounding, rf, alpha, devices, store, path_begin, chol,
                                    native_math, as_array, fold, shard, context, drawdown, horizons, bands, rebalance, rebalance_cost, dof,
                                    cashflow, target, overlay, spot, garch, attribution, antithetic, jumps, regimes, glide, protect, spending,
                                    lifetime, tolerance, vol_target, underwater_levels, ds, bm)
    if vol_target is not None:
        return _simulate_vol_target(mu, cov, weights, n_steps, n_paths, seed, v0, compounding, rf, alpha, devices, store, path_begin, chol,
                                    native_math, as_array, fold, shard, context, drawdown, horizons, bands, rebalance, rebalance_cost, dof,
                                    cashflow, target, overlay, spot, garch, attribution, antithetic, jumps, regimes, glide, protect, spending,
                                    lifetime, tolerance, vol_target, ds, bm)
    from .lifetime import check_lifetime
    lt = check_lifetime(lifetime, lifetime_levels, n_steps)
    if lt is not None and cashflow is None and spending is None:
        raise ValueError("lifetime needs a walk with ruin: cashflow (with or without glide) or spending")
    if tolerance is not None:
        kw = dict(tolerance=tolerance, spending=spending, protect=protect, glide=glide, regimes=regimes, jumps=jumps, antithetic=antithetic,
                  attribution=attribution, garch=garch, overlay=overlay, cashflow=cashflow, dof=dof, drawdown=drawdown, fold=fold,
                  native_math=native_math, compounding=compounding)
        _check_combines(_PATHS_COMBINE, "tolerance", kw)
        period, cost = check_rebalance(1 if rebalance is None else rebalance, rebalance_cost)
        steps, levels = _check_walk(n_steps, horizons, bands, period, compounding, shard)
        mu32, L, W = prepare_inputs(mu, cov, weights, chol)
        from .tolerance import check_tolerance
        tol, tlv = check_tolerance(tolerance, tolerance_levels, W.shape, n_steps, period)
        prm, ctx = _setup(mu32.shape[0], n_steps, W.shape[0], compounding, v0, alpha, rf, False, False, devices, shard, context)
        out = ctx._call(prm, W, int(seed), int(path_begin), int(n_paths), store, mu=mu32, chol=L, horizons=steps, levels=levels,
                        tolerance=(period, cost, tol, tlv), downside=ds, benchmark=bm)
        return _with_tolerance(_result(out, np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding), out, tol, period,
                               tlv, store, as_array)
    kw = dict(spending=spending, protect=protect, glide=glide, regimes=regimes, jumps=jumps, antithetic=antithetic, attribution=attribution, garch=garch, overlay=overlay,
              cashflow=cashflow, dof=dof, rebalance=rebalance, drawdown=drawdown, horizons=horizons, fold=fold, native_math=native_math,
              compounding=compounding, shard=shard)
    sv = check_spending(spending, v0)
    _check_combines(_PATHS_COMBINE, "spending", kw)
    pv = check_protect(protect, n_steps, v0)
    _check_combines(_PATHS_COMBINE, "protect", kw)
    goal = None
    if sv is not None and target is not None:              # the target of a spending call is the rule's second count
        goal = check_cashflow(0.0, target, n_steps)[1]
        target = None
    if pv is not None and target is not None:              # the target of a protected call is the second count's, not a cash-flow goal
        goal = check_cashflow(0.0, target, n_steps)[1]
        target = None
    gl = check_glide(glide, weights, n_steps)
    _check_combines(_PATHS_COMBINE, "glide", kw)
    if gl is not None and cashflow is None:
        kw["cashflow"] = cashflow = 0.0
    rv = check_regimes(regimes, len(np.atleast_1d(np.asarray(mu))), factor=chol is not None)
    _check_combines(_PATHS_COMBINE, "regimes", kw)
    if rv is not None:
        with np.errstate(over="ignore"):
            if not (np.all(np.isfinite(np.asarray(mu, np.float64))) and np.all(np.isfinite(np.asarray(mu, np.float64).astype(np.float32)))
                    and np.all(np.isfinite(np.asarray(cov if chol is None else chol, np.float64)))):
                raise ValueError("regimes need finite mu and cov")
    jv = check_jumps(jumps, len(np.atleast_1d(np.asarray(mu))))
    _check_combines(_PATHS_COMBINE, "jumps", kw)
    if not isinstance(antithetic, (bool, np.bool_)):
        raise ValueError(f"antithetic must be True or False, got {antithetic!r}")
    _check_combines(_PATHS_COMBINE, "antithetic", kw)
    if antithetic and (int(n_paths) % 2 or int(path_begin) % 2):
        raise ValueError(f"antithetic pairs need an even n_paths and an even path_begin, got n_paths={n_paths}, path_begin={path_begin}")
    if not isinstance(attribution, (bool, np.bool_)):
        raise ValueError(f"attribution must be True or False, got {attribution!r}")
    _check_combines(_PATHS_COMBINE, "attribution", kw)
    if attribution:
        k_attr = np.atleast_2d(np.asarray(weights)).shape[0]
        if k_attr > _ffi.MCP_MAX_ATTR_PORTFOLIOS:
            raise ValueError(f"attribution takes at most {_ffi.MCP_MAX_ATTR_PORTFOLIOS} portfolios, got {k_attr}: call simulate_paths "
                             "for the portfolios of interest")
    gv = check_garch(garch)
    _check_combines(_PATHS_COMBINE, "garch", kw)
    ov = check_overlay(overlay, spot, len(np.atleast_1d(np.asarray(mu))))
    _check_combines(_PATHS_COMBINE, "overlay", kw)
    flows, target = check_cashflow(cashflow, target, n_steps)
    _check_combines(_PATHS_COMBINE, "cashflow", kw)
    dof = check_dof(dof)
    _check_combines(_PATHS_COMBINE, "dof", kw)
    period, cost = check_rebalance(rebalance, rebalance_cost)
    for feature in ("rebalance", "drawdown", "horizons"):
        _check_combines(_PATHS_COMBINE, feature, kw)
    steps, levels = _check_walk(n_steps, horizons, bands, period, compounding, shard)
    if jv is not None and chol is None:                    # `cov` is the total covariance: the diffusion gets what the jumps leave
        from .jumps import diffusion_cov
        cov = diffusion_cov(cov, jv)
    mu32, L, W = prepare_inputs(mu, cov, weights, chol)
    prm, ctx = _setup(mu32.shape[0], n_steps, W.shape[0], compounding, v0, alpha, rf, native_math, fold, devices,
                      "paths" if attribution or antithetic else shard, context)
    out = ctx._call(prm, W, int(seed), int(path_begin), int(n_paths), store, mu=mu32, chol=L, dof=dof, period=period, cost=cost,
                    drawdown=drawdown, horizons=steps, levels=levels, flows=flows, target=target if pv is None and sv is None else goal,
                    overlay=ov, garch=gv, attribution=bool(attribution), antithetic=bool(antithetic), jumps=jv, regimes=rv, glide=gl, protect=pv,
                    spending=sv, downside=ds, benchmark=bm, **({} if lt is None else {"lifetime": lt}))
    if sv is not None:                                     # the counts are the 'spending' block's, not a 'cashflow' block's
        res = _spending_result(out, sv, v0, np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding, goal)
    elif pv is not None:                                     # the counts are the 'protect' block's, not a 'cashflow' block's
        res = _result(out._replace(counts=None, hz_counts=None), np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding)
        if as_array:
            res = (res if isinstance(res, tuple) else (res,)) + ((out.counts,) if out.hz_counts is None else (out.counts, out.hz_counts))
        else:
            for d, blk in zip([res] if isinstance(res, dict) else res,
                              _protect_blocks(pv, out.counts, out.hz_counts, int(out.stats[0]["n"]), goal)):
                d["protect"] = blk
    else:
        res = _result(out, np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding, flows, target)
    if gl is not None and not as_array:
        for d, blk in zip([res] if isinstance(res, dict) else res, _glide_blocks(gl, W)):
            d["glide"] = blk
    if jv is not None and not as_array:
        for d, blk in zip([res] if isinstance(res, dict) else res, _jump_blocks(jv, L, W)):
            d["jumps"] = blk
    if rv is not None and not as_array:
        blk = _regime_block(rv, steps)
        for d in [res] if isinstance(res, dict) else res:
            d["regimes"] = dict(blk)
    return res if lt is None else _with_lifetime(res, out, lt, store, as_array)


def _simulate_vol_target(mu, cov, weights, n_steps, n_paths, seed, v0, compounding, rf, alpha, devices, store, path_begin, chol, native_math,
                         as_array, fold, shard, context, drawdown, horizons, bands, rebalance, rebalance_cost, dof, cashflow, target, overlay,
                         spot, garch, attribution, antithetic, jumps, regimes, glide, protect, spending, lifetime, tolerance, vol_target, downside=None, benchmark=None):
    """simulate_paths with a volatility target (SPEC.md 4.19 / 5.19): the rules of what it combines with, then the draws' own rules
    in simulate_paths' order, the call and the 'vol_target' block."""
    from .voltarget import check_vol_target, vol_target_blocks
    if not isinstance(lifetime, (bool, np.bool_)):
        raise ValueError(f"lifetime must be True or False, got {lifetime!r}")
    kw = dict(vol_target=vol_target, tolerance=tolerance, spending=spending, protect=protect, glide=glide, regimes=regimes, jumps=jumps,
              antithetic=antithetic, attribution=attribution, garch=garch, overlay=overlay, cashflow=cashflow, dof=dof, rebalance=rebalance,
              drawdown=drawdown, horizons=horizons, lifetime=lifetime, fold=fold, native_math=native_math, compounding=compounding,
              shard=shard)
    vt = check_vol_target(vol_target, np.atleast_2d(np.asarray(weights)).shape[0])
    _check_combines(_PATHS_COMBINE, "vol_target", kw)
    if spot is not None:
        raise ValueError("spot belongs to overlay: vol_target takes none")
    goal = check_cashflow(0.0, target, n_steps)[1] if target is not None else None   # the target of a targeted call is the second count's
    jv = check_jumps(jumps, len(np.atleast_1d(np.asarray(mu))))
    _check_combines(_PATHS_COMBINE, "jumps", kw)
    gv = check_garch(garch)
    dof = check_dof(dof)
    for feature in ("drawdown", "horizons"):
        _check_combines(_PATHS_COMBINE, feature, kw)
    steps, levels = _check_walk(n_steps, horizons, bands, None, compounding, shard)
    if jv is not None and chol is None:                    # `cov` is the total covariance: the diffusion gets what the jumps leave
        from .jumps import diffusion_cov
        cov = diffusion_cov(cov, jv)
    mu32, L, W = prepare_inputs(mu, cov, weights, chol)
    prm, ctx = _setup(mu32.shape[0], n_steps, W.shape[0], compounding, v0, alpha, rf, False, False, devices, shard, context)
    vts = _ffi.make_vol_target(*vt)
    consts, s0 = _ffi.vol_target_consts(prm, vts, L, W)    # the library's rules, s0's among them, before anything is launched
    out = ctx._call(prm, W, int(seed), int(path_begin), int(n_paths), store, mu=mu32, chol=L, dof=dof, drawdown=bool(drawdown), horizons=steps,
                    levels=levels, target=goal, garch=gv, jumps=jv, vol_target=vt, downside=downside, benchmark=benchmark)
    res = _result(out._replace(counts=None, hz_counts=None), np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding)
    if as_array:
        return ((res if isinstance(res, tuple) else (res,)) + ((out.counts,) if out.hz_counts is None else (out.counts, out.hz_counts))
                + (() if out.exposure_stats is None else (out.exposure_stats, out.exposure) if store else (out.exposure_stats,)))
    for d, blk in zip([res] if isinstance(res, dict) else res, vol_target_blocks(consts, s0, out, n_steps, alpha, goal, store)):
        d["vol_target"] = blk
    if jv is not None:
        for d, blk in zip([res] if isinstance(res, dict) else res, _jump_blocks(jv, L, W)):
            d["jumps"] = blk
    return res


def _simulate_uncertain(mu, cov, weights, n_steps, n_paths, seed, v0, compounding, rf, alpha, devices, store, path_begin, chol, native_math,
                        as_array, fold, shard, context, drawdown, horizons, bands, rebalance, rebalance_cost, dof, cashflow, target, overlay,
                        spot, garch, attribution, antithetic, jumps, regimes, glide, protect, spending, lifetime, tolerance, vol_target,
                        underwater, drift_uncertainty, downside=None, benchmark=None):
    """simulate_paths with drift uncertainty (SPEC.md 2.7 / 4.21 / 5.21): the rules of what it combines with, then the underlying
    call's own rules in simulate_paths' order, the call and the 'drift_uncertainty' block."""
    from .uncertainty import check_drift_uncertainty, uncertainty_blocks
    for name, flag in (("lifetime", lifetime), ("underwater", underwater), ("attribution", attribution), ("antithetic", antithetic)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False, got {flag!r}")
    kw = dict(drift_uncertainty=drift_uncertainty, underwater=underwater, vol_target=vol_target, tolerance=tolerance, spending=spending,
              protect=protect, glide=glide, regimes=regimes, jumps=jumps, antithetic=antithetic, attribution=attribution, garch=garch,
              overlay=overlay, cashflow=cashflow, dof=dof, rebalance=rebalance, drawdown=drawdown, horizons=horizons, lifetime=lifetime,
              fold=fold, native_math=native_math, compounding=compounding, shard=shard)
    _check_combines(_PATHS_COMBINE, "drift_uncertainty", kw)
    if spot is not None:
        raise ValueError("spot belongs to overlay: drift_uncertainty takes none")
    M = check_drift_uncertainty(drift_uncertainty, cov, chol)
    flows, target = check_cashflow(cashflow, target, n_steps)
    for feature in ("cashflow", "drawdown", "horizons"):
        _check_combines(_PATHS_COMBINE, feature, kw)
    steps, levels = _check_walk(n_steps, horizons, bands, None, compounding, shard)
    mu32, L, W = prepare_inputs(mu, cov, weights, chol)
    if M.shape != L.shape:
        raise ValueError(f"drift_uncertainty: the factor is {M.shape}, the market has {L.shape[0]} assets")
    prm, ctx = _setup(mu32.shape[0], n_steps, W.shape[0], compounding, v0, alpha, rf, False, False, devices, shard, context)
    out = ctx._call(prm, W, int(seed), int(path_begin), int(n_paths), store, mu=mu32, chol=L, drawdown=bool(drawdown), horizons=steps,
                    levels=levels, flows=flows, target=target, drift_uncertainty=M, downside=downside, benchmark=benchmark)
    res = _result(out, np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding, flows, target)
    if as_array:
        return res
    for d, blk in zip([res] if isinstance(res, dict) else res, uncertainty_blocks(L, M, W, n_steps, steps)):
        d["drift_uncertainty"] = blk
    return res


def _simulate_underwater(mu, cov, weights, n_steps, n_paths, seed, v0, compounding, rf, alpha, devices, store, path_begin, chol, native_math,
                         as_array, fold, shard, context, drawdown, horizons, bands, rebalance, rebalance_cost, dof, cashflow, target, overlay,
                         spot, garch, attribution, antithetic, jumps, regimes, glide, protect, spending, lifetime, tolerance, vol_target,
                         underwater_levels, downside=None, benchmark=None):
    """simulate_paths with the time under water (SPEC.md 4.20 / 5.20): the rules of what it combines with, then the draws' own rules in
    simulate_paths' order, the call and the 'underwater' block."""
    from .underwater import check_underwater, underwater_blocks
    if not isinstance(lifetime, (bool, np.bool_)):
        raise ValueError(f"lifetime must be True or False, got {lifetime!r}")
    if not drawdown:
        raise ValueError("underwater=True needs drawdown=True: the spells are counted against the running peak of the drawdown walk")
    kw = dict(underwater=True, vol_target=vol_target, tolerance=tolerance, spending=spending, protect=protect, glide=glide, regimes=regimes,
              jumps=jumps, antithetic=antithetic, attribution=attribution, garch=garch, overlay=overlay, cashflow=cashflow, dof=dof,
              rebalance=rebalance, drawdown=drawdown, horizons=horizons, lifetime=lifetime, fold=fold, native_math=native_math,
              compounding=compounding, shard=shard)
    lv = check_underwater(underwater_levels, n_steps)
    _check_combines(_PATHS_COMBINE, "underwater", kw)
    if spot is not None:
        raise ValueError("spot belongs to overlay: underwater takes none")
    if target is not None:
        raise ValueError("target belongs to cashflow, protect, spending or vol_target: underwater takes none")
    jv = check_jumps(jumps, len(np.atleast_1d(np.asarray(mu))))
    _check_combines(_PATHS_COMBINE, "jumps", kw)
    gv = check_garch(garch)
    _check_combines(_PATHS_COMBINE, "garch", kw)
    dof = check_dof(dof)
    _check_combines(_PATHS_COMBINE, "dof", kw)
    _check_walk(n_steps, None, bands, None, compounding, shard)
    if jv is not None and chol is None:                    # `cov` is the total covariance: the diffusion gets what the jumps leave
        from .jumps import diffusion_cov
        cov = diffusion_cov(cov, jv)
    mu32, L, W = prepare_inputs(mu, cov, weights, chol)
    prm, ctx = _setup(mu32.shape[0], n_steps, W.shape[0], compounding, v0, alpha, rf, False, False, devices, shard, context)
    out = ctx._call(prm, W, int(seed), int(path_begin), int(n_paths), store, mu=mu32, chol=L, dof=dof, drawdown=True, garch=gv, jumps=jv,
                    underwater=lv, downside=downside, benchmark=benchmark)
    res = _result(out, np.asarray(weights).ndim == 1, store, as_array, None, (), compounding)
    if as_array:
        return ((res if isinstance(res, tuple) else (res,)) + (out.uw_longest_hist, out.uw_current_hist, out.uw_sums, out.uw_q)
                + ((out.uw_longest, out.uw_current) if store else ()))
    for d, blk in zip([res] if isinstance(res, dict) else res, underwater_blocks(out, lv, store, int(out.stats[0]["n"]))):
        d["underwater"] = blk
    if jv is not None:
        for d, blk in zip([res] if isinstance(res, dict) else res, _jump_blocks(jv, L, W)):
            d["jumps"] = blk
    return res


def _with_tolerance(res, out, tol, every, levels, store, as_array):
    """The result of a call with its band outputs (SPEC.md 5.18): as_array appends trade_hist, trade_sum, trade_q, turnover_stats[,
    trades, turnover]; else every dict gains the 'tolerance' block."""
    from .tolerance import tolerance_blocks
    if as_array:
        return ((res if isinstance(res, tuple) else (res,)) + (out.trade_hist, out.trade_sum, out.trade_q, out.turnover_stats)
                + ((out.trades, out.turnover) if store else ()))
    for d, blk in zip([res] if isinstance(res, dict) else res, tolerance_blocks(out, tol, every, levels, store, int(out.stats[0]["n"]))):
        d["tolerance"] = blk
    return res


def _with_lifetime(res, out, levels, store, as_array):
    """The result of a call with its lifetime outputs (SPEC.md 5.17): as_array appends life_hist, life_sum, life_q[, life]; else
    every dict gains the 'lifetime' block."""
    from .lifetime import lifetime_blocks
    if as_array:
        return (res if isinstance(res, tuple) else (res,)) + (out.life_hist, out.life_sum, out.life_q) + ((out.life,) if store else ())
    for d, blk in zip([res] if isinstance(res, dict) else res, lifetime_blocks(out, levels, store, int(out.stats[0]["n"]))):
        d["lifetime"] = blk
    return res


def _regime_block(rv, steps):
    """The 'regimes' block of a result dict: the probabilities the kernels use (SPEC.md 2.6), the long-run probability of regime 1,
    the expected steps in each regime and, with horizons, the expected share of the first h steps walked in regime 1."""
    from .regimes import occupancy_path, stationary, used_probabilities
    p01, p10, start = used_probabilities(rv[0], rv[1], rv[2])
    blk = {"p01": p01, "p10": p10, "start": start, "stationary": stationary(p01, p10),
           "mean_duration": (1.0 / p01 if p01 > 0 else float("inf"), 1.0 / p10 if p10 > 0 else float("inf"))}
    if steps is not None:
        cum = np.cumsum(occupancy_path(p01, p10, start, int(steps[-1])))
        blk["occupancy"] = np.array([cum[h - 1] / h for h in steps.astype(np.int64)], np.float64)
    return blk


def _jump_blocks(jv, L, W):
    """The 'jumps' block of every portfolio: the intensity asked for, the mean of the count the kernels draw and the jump's share
    Var(J) (w.b)^2 / (w' L L' w + Var(J) (w.b)^2) of the one-step variance (0 where that is 0)."""
    from .jumps import jump_law
    law = jump_law(jv)
    L64, W64 = np.tril(L).astype(np.float64), W.astype(np.float64)
    b = np.ones(L64.shape[0]) if jv[3] is None else jv[3].astype(np.float64)
    out = []
    for w in W64:
        diff, jump = float(w @ L64 @ L64.T @ w), law.var_jump * float(w @ b) ** 2
        out.append({"intensity": jv[0], "mean_count": law.mean_count, "variance_share": jump / (diff + jump) if diff + jump > 0 else 0.0})
    return out


def _check_walk(n_steps, horizons, bands, period, compounding, shard):
    """The argument rules of simulate_paths and simulate_bootstrap alike: rebalancing compounds simply, bands need horizons, and
    `shard` -> (steps, levels) of check_horizons, or (None, ()) without horizons."""
    if period is not None and compounding == "log":
        raise ValueError("rebalance needs simple compounding: not with compounding='log'")
    if horizons is not None:
        steps, levels = check_horizons(horizons, bands, n_steps)
    elif len(np.atleast_1d(np.asarray(bands, np.float64))):
        raise ValueError("bands need horizons")
    else:
        steps, levels = None, ()
    if shard not in ("auto", "paths", "portfolios"):
        raise ValueError("shard must be 'auto', 'paths' or 'portfolios'")
    return steps, levels


def _setup(n_assets, n_steps, K, compounding, v0, alpha, rf, native_math, fold, devices, shard, context):
    """-> (mcp_params, Context) of a call: shard="portfolios" (or "auto" with K >= 512 per device) shards the weight matrix."""
    devs = (0,) if not devices else tuple(int(d) for d in devices)
    by_portfolio = len(devs) > 1 and (shard == "portfolios" or (shard == "auto" and K >= 512 * len(devs)))
    prm = _ffi.make_params(n_assets, n_steps, K, compounding, v0, alpha, rf, native_math, fold, by_portfolio)
    return prm, context if context is not None else default_context(devs)


def _cash_block(counts, n, target, contributed=None):
    """The counts {n_ruined, n_short} [..., 2] of SPEC.md 5.6 over n paths as the fields of a result dict."""
    c = np.asarray(counts)
    scalar = c.ndim == 1
    cast = (lambda a: int(a)) if scalar else (lambda a: a.astype(np.int64))            # noqa: E731
    prob = (lambda a: float(a) / n) if scalar else (lambda a: a.astype(np.float64) / n)   # noqa: E731
    d = {} if contributed is None else {"contributed": contributed}
    d.update(n_ruined=cast(c[..., 0]), ruin_probability=prob(c[..., 0]))
    if target is not None:
        d.update(n_short=cast(c[..., 1]), shortfall_probability=prob(c[..., 1]))
    return d


def _result(out, single, store, as_array, steps, levels, compounding, flows=None, target=None):
    """What simulate_paths / simulate_bootstrap return for Context._call's outputs `out`: with as_array the record arrays (stats,
    then (hz_stats, bands) or dd_stats, then with `store` terminal and horizon_terminal or max_drawdown); else one dict per
    portfolio (one dict for a single weight vector) with its 'drawdown' / 'horizons' blocks and, with `store`, the stored arrays."""
    stats, dd_stats, hz_stats, hz_bands, term, qd, hz_term, counts, hz_counts = out[:9]
    attr, attr_counts, contrib, pairs = out[9:13]
    mdd = mdd_from_raw(qd, compounding) if dd_stats is not None and store else None
    if as_array and pairs is not None:    # SPEC.md 5.10: what the call without pairs returns, then the [K] pair records
        base = _result(out._replace(pairs=None), single, store, as_array, steps, levels, compounding, flows, target)
        return (base if isinstance(base, tuple) else (base,)) + (pairs,)
    if as_array:                          # [K] structured arrays (fields of mcp_stats), for large sweeps
        cash = () if counts is None else (counts,) if hz_counts is None else (counts, hz_counts)
        if hz_stats is not None:
            return ((stats, hz_stats, hz_bands, term, hz_term) if store else (stats, hz_stats, hz_bands)) + cash
        if dd_stats is not None:
            return (stats, dd_stats, term, mdd) if store else (stats, dd_stats)
        if cash:
            return ((stats, term) if store else (stats,)) + cash
        if attr is not None:              # SPEC.md 5.9
            return ((stats, term) if store else (stats,)) + (attr, attr_counts) + ((contrib,) if store else ())
        return (stats, term) if store else stats
    res = [stats_to_dict(stats[k]) for k in range(stats.shape[0])]
    if out.downside_stats is not None:   # SPEC.md 5.22
        from .downside import downside_blocks
        for d, blk in zip(res, downside_blocks(out.downside_stats, out.downside_sums, out.downside_tau, out.downside_hz_stats)):
            d["downside"] = blk
    if out.relative_stats is not None:   # SPEC.md 5.23
        from .relative import relative_blocks
        for d, blk in zip(res, relative_blocks(out.relative_stats, out.relative_sums, out.relative_bench, out.relative_active_stats,
                                               out.relative_hz_stats, out.relative_active if store else None)):
            d["relative"] = blk
    for k, d in enumerate(res):
        if dd_stats is not None:
            d["drawdown"] = drawdown_to_dict(dd_stats[k])
        if hz_stats is not None:
            d["horizons"] = dict({"steps": steps.astype(np.int64), "levels": levels.copy(), "bands": hz_bands[:, k, :]},
                                 **{f: hz_stats[f][:, k].astype(np.int64 if f == "n_tail" else np.float64)
                                    for f in ("mean", "std", "var", "cvar", "min", "max", "n_tail")})
            if hz_counts is not None:
                d["horizons"].update(_cash_block(hz_counts[:, k, :], int(stats[k]["n"]), target))
        if counts is not None:            # SPEC.md 5.6; contributed: the binary64 sum of the binary32 flows
            d["cashflow"] = _cash_block(counts[k], int(stats[k]["n"]), target, float(np.sum(flows.astype(np.float64))))
        if attr is not None:
            d["attribution"] = attribution_to_dict(attr[k], attr_counts[k], stats[k])
        if pairs is not None:
            d["antithetic"] = antithetic_to_dict(pairs[k])
        if store:
            d["terminal"] = term[k]
            if contrib is not None:
                d["contributions"] = contrib[k]
            if dd_stats is not None:
                d["max_drawdown"] = mdd[k]
            if hz_stats is not None:
                d["horizon_terminal"] = hz_term[:, k, :]
    return res[0] if single else res


def bootstrap_inputs(returns, weights):
    """SPEC.md 2.1 argument rules -> (rows binary32 [R, N] C-contiguous, W binary32 [K, N]); ValueError otherwise.  `returns`
    is a DataFrame (returns_matrix(...), app.py:667) or an [R, N] array; its values are rounded to binary32 to nearest."""
    vals = returns.to_numpy() if hasattr(returns, "to_numpy") else returns
    rows64 = np.asarray(vals, np.float64)
    if rows64.ndim == 1:
        rows64 = rows64[:, None]
    if rows64.ndim != 2 or rows64.shape[0] < 1:
        raise ValueError(f"returns must be an [R, N] matrix with R >= 1, got shape {rows64.shape}")
    R, N = rows64.shape
    if R > _ffi.MCP_MAX_BOOT_ROWS:
        raise ValueError(f"at most {_ffi.MCP_MAX_BOOT_ROWS} return rows, got {R}")
    if not 1 <= N <= _ffi.MCP_MAX_ASSETS:
        raise ValueError(f"n_assets={N} outside [1, {_ffi.MCP_MAX_ASSETS}]")
    rows = np.ascontiguousarray(rows64.astype(np.float32))
    bad = ~np.isfinite(rows).all(axis=1)
    if bad.any():
        raise ValueError(f"returns hold NaN or infinite values in {int(bad.sum())} rows (first: row {int(np.argmax(bad))}); drop them first")
    W = np.ascontiguousarray(np.atleast_2d(np.asarray(weights, np.float32)))
    if W.ndim != 2 or W.shape[1] != N:
        raise ValueError(f"weights have {W.shape[-1]} columns, the returns {N}")
    return rows, W


def simulate_bootstrap(returns, weights, n_steps=252, n_paths=10_000, block=1.0, seed=0, v0=1.0, compounding="simple",
                       rf=0.0, alpha=0.95, devices=None, store=False, path_begin=0, as_array=False, shard="auto", context=None,
                       horizons=None, bands=(), rebalance=None, rebalance_cost=0.0, cashflow=None, target=None, glide=None, spending=None,
                       lifetime=False, lifetime_levels=(5, 25, 50), tolerance=None, tolerance_levels=(5, 50, 95), downside=None,
                       benchmark=None, **unsupported):
    """simulate_paths on paths resampled from the observed return rows instead of a normal model: the stationary block
    bootstrap of Politis & Romano (SPEC.md 2.1 / 4.4).  Every step of a path uses one whole row of `returns` (all assets of one
    date together), so fat tails, skew, the co-movement within a row and -- with a mean block length `block` > 1 -- short-range
    serial dependence survive.  block = 1: every row drawn independently; block = inf: one random start, then consecutive
    rows (circularly).  All portfolios see the same rows.

    returns: DataFrame (returns_matrix(...), app.py:667) or [R, N] array of per-step returns, finite, R <= 2^20; weights [N]
    or [K, N].  Returns exactly what simulate_paths returns for the same arguments, 'horizons' block included (pivots of
    SPEC.md 5.3).  ValueError for NaN rows, a width that does not match the weights, block < 1, or the simulate_paths keywords
    that have no meaning here (fold, native_math, drawdown, chol).  rebalance / rebalance_cost as in simulate_paths (SPEC.md 4.5,
    pivots of SPEC.md 5.4; not with compounding="log").  cashflow / target as in simulate_paths (SPEC.md 4.7, pivots of SPEC.md
    5.6; not with rebalance or compounding="log").  glide as in simulate_paths (SPEC.md 4.14, pivots of SPEC.md 5.14 on the row
    means; not with rebalance or compounding="log").  spending as in simulate_paths (SPEC.md 4.16, pivots of SPEC.md 5.16 on the
    row means; not with cashflow, glide, rebalance or compounding="log").  lifetime / lifetime_levels as in simulate_paths (SPEC.md
    4.17 / 5.17; with cashflow, with or without glide, or spending).  tolerance / tolerance_levels as in simulate_paths (SPEC.md 4.18 /
    5.18, pivots of SPEC.md 5.4; not with cashflow, glide, spending or compounding="log").  downside as in simulate_paths (SPEC.md
    5.22; with every keyword here, not with as_array).
    """
    from .downside import check_downside
    ds = check_downside(downside)
    if ds is not None and as_array:
        raise ValueError("downside fills the 'downside' block of the result dicts: not with as_array")
    bm = _check_benchmark(benchmark, weights, as_array, shard)
    from .lifetime import check_lifetime
    lt = check_lifetime(lifetime, lifetime_levels, n_steps)
    if lt is not None and cashflow is None and spending is None:
        raise ValueError("lifetime needs a walk with ruin: cashflow (with or without glide) or spending")
    if unsupported.get("overlay") is not None or unsupported.get("spot") is not None:
        raise ValueError("simulate_bootstrap does not take overlay: the rows are observed returns with no price level to strike an "
                         "option at -- apply the strategy to the returns matrix first (options.calc_options_series per asset, as "
                         "the reference does), or call simulate_paths(overlay=...)")
    if unsupported.get("attribution"):
        raise ValueError("simulate_bootstrap does not take attribution: the second walk re-draws normals, the bootstrap's rows are not "
                         "built into it -- call simulate_paths(attribution=True)")
    unsupported.pop("attribution", None)
    if unsupported.get("antithetic"):
        raise ValueError("simulate_bootstrap does not take antithetic: observed rows have no sign to flip -- antithetic pairs negate "
                         "the normals of a parametric model, call simulate_paths(antithetic=True)")
    unsupported.pop("antithetic", None)
    if unsupported.get("garch") is not None:
        raise ValueError("simulate_bootstrap does not take garch: the rows carry their own dynamics -- a mean block length block > 1 "
                         "keeps the volatility regimes of the observed rows; GARCH is a parametric model, call "
                         "simulate_paths(garch=...)")
    if unsupported:
        raise ValueError(f"simulate_bootstrap does not take {sorted(unsupported)} (no normals: no fold / native_math / dof -- "
                         "Student-t draws are a parametric model, call simulate_paths(dof=...); drawdown on bootstrap paths is "
                         "not supported)")
    if tolerance is not None:
        kw = dict(tolerance=tolerance, spending=spending, glide=glide, cashflow=cashflow, compounding=compounding)
        _check_combines(_BOOTSTRAP_COMBINE, "tolerance", kw)
        period, cost = check_rebalance(1 if rebalance is None else rebalance, rebalance_cost)
        b = float(block)
        if not b >= 1.0:
            raise ValueError(f"block (mean block length) must be >= 1 or inf, got {block!r}")
        steps, levels = _check_walk(n_steps, horizons, bands, period, compounding, shard)
        rows, W = bootstrap_inputs(returns, weights)
        from .tolerance import check_tolerance
        tol, tlv = check_tolerance(tolerance, tolerance_levels, W.shape, n_steps, period)
        prm, ctx = _setup(rows.shape[1], n_steps, W.shape[0], compounding, v0, alpha, rf, False, False, devices, shard, context)
        out = ctx._call(prm, W, int(seed), int(path_begin), int(n_paths), store, rows=rows, block=b, horizons=steps, levels=levels,
                        tolerance=(period, cost, tol, tlv), downside=ds, benchmark=bm)
        return _with_tolerance(_result(out, np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding), out, tol, period,
                               tlv, store, as_array)
    kw = dict(spending=spending, glide=glide, cashflow=cashflow, rebalance=rebalance, compounding=compounding)
    sv = check_spending(spending, v0)
    _check_combines(_BOOTSTRAP_COMBINE, "spending", kw)
    goal = None
    if sv is not None and target is not None:
        goal = check_cashflow(0.0, target, n_steps)[1]
        target = None
    gl = check_glide(glide, weights, n_steps)
    _check_combines(_BOOTSTRAP_COMBINE, "glide", kw)
    if gl is not None and cashflow is None:
        kw["cashflow"] = cashflow = 0.0
    flows, target = check_cashflow(cashflow, target, n_steps)
    _check_combines(_BOOTSTRAP_COMBINE, "cashflow", kw)
    period, cost = check_rebalance(rebalance, rebalance_cost)
    b = float(block)
    if not b >= 1.0:
        raise ValueError(f"block (mean block length) must be >= 1 or inf, got {block!r}")
    steps, levels = _check_walk(n_steps, horizons, bands, period, compounding, shard)
    rows, W = bootstrap_inputs(returns, weights)
    prm, ctx = _setup(rows.shape[1], n_steps, W.shape[0], compounding, v0, alpha, rf, False, False, devices, shard, context)
    out = ctx._call(prm, W, int(seed), int(path_begin), int(n_paths), store, rows=rows, block=b, period=period, cost=cost,
                    horizons=steps, levels=levels, flows=flows, target=target if sv is None else goal, glide=gl, spending=sv, downside=ds, benchmark=bm,
                    **({} if lt is None else {"lifetime": lt}))
    if sv is not None:
        res = _spending_result(out, sv, v0, np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding, goal)
        return res if lt is None else _with_lifetime(res, out, lt, store, as_array)
    res = _result(out, np.asarray(weights).ndim == 1, store, as_array, steps, levels, compounding, flows, target)
    if gl is not None and not as_array:
        for d, blk in zip([res] if isinstance(res, dict) else res, _glide_blocks(gl, W)):
            d["glide"] = blk
    return res if lt is None else _with_lifetime(res, out, lt, store, as_array)


def filtered_inputs(filtered, weights):
    """SPEC.md 2.4 argument rules -> (mu [N], resid [R, N], shock [R], W [K, N]), binary32 and C-contiguous; ValueError otherwise.
    `filtered` is a garch.FilteredRows or a (mu, resid, shock) triple; its values are rounded to binary32 to nearest."""
    if hasattr(filtered, "resid"):
        filtered = (filtered.mu, filtered.resid, filtered.shock)
    if isinstance(filtered, (str, bytes)) or not hasattr(filtered, "__len__") or len(filtered) != 3:
        raise ValueError("filtered must be a FilteredRows (filter_rows(...)) or a (mu, resid, shock) triple")
    mu, resid, shock = (np.asarray(a, np.float64) for a in filtered)
    mu, shock = np.atleast_1d(mu), np.atleast_1d(shock)
    if resid.ndim == 1:
        resid = resid[:, None]
    if resid.ndim != 2 or resid.shape[0] < 1 or mu.ndim != 1 or shock.ndim != 1:
        raise ValueError(f"filtered wants mu [N], resid [R, N] with R >= 1 and shock [R], got shapes {mu.shape}, {resid.shape}, {shock.shape}")
    R, N = resid.shape
    if mu.shape[0] != N or shock.shape[0] != R:
        raise ValueError(f"filtered resid is [{R}, {N}], mu has {mu.shape[0]} entries and shock {shock.shape[0]}")
    if R > _ffi.MCP_MAX_BOOT_ROWS:
        raise ValueError(f"at most {_ffi.MCP_MAX_BOOT_ROWS} residual rows, got {R}")
    if not 1 <= N <= _ffi.MCP_MAX_ASSETS:
        raise ValueError(f"n_assets={N} outside [1, {_ffi.MCP_MAX_ASSETS}]")
    with np.errstate(over="ignore"):
        mu, resid, shock = (np.ascontiguousarray(a.astype(np.float32)) for a in (mu, resid, shock))
    for name, a in (("mu", mu), ("resid", resid), ("shock", shock)):
        if not np.isfinite(a).all():
            raise ValueError(f"filtered {name} holds NaN or infinite values (first: index {int(np.argmax(~np.isfinite(a).ravel()))})")
    if (shock < 0).any():
        raise ValueError(f"filtered shock must be >= 0 (first: row {int(np.argmax(shock < 0))})")
    W = np.ascontiguousarray(np.atleast_2d(np.asarray(weights, np.float32)))
    if W.ndim != 2 or W.shape[1] != N:
        raise ValueError(f"weights have {W.shape[-1]} columns, the residual rows {N}")
    return mu, resid, shock, W


def simulate_filtered(filtered, weights, n_steps=252, n_paths=10_000, garch=None, block=1.0, seed=0, v0=1.0, rf=0.0, alpha=0.95,
                      horizons=None, levels=(), devices=None, store=False, as_array=False, path_begin=0, shard="auto", context=None,
                      downside=None, benchmark=None, **unsupported):
    """Filtered historical simulation (Barone-Adesi, Giannopoulos & Vosper 1999; SPEC.md 2.4 / 4.11): simulate_bootstrap on rows
    that garch.filter_rows de-volatilised with the fitted GARCH(1,1) variance path, every draw re-scaled by the path's own simulated
    variance ratio h -- the empirical shocks of the bootstrap (tails, skew, assets that crash together) with the volatility
    clustering of simulate_paths(garch=...), and a fan that starts from today's variance level.  A step draws a row j as the
    bootstrap does, r = mu + sqrt(h) resid[j], and h moves on the row's shock.

    filtered: a FilteredRows (filter_rows(returns)) or a (mu [N], resid [R, N], shock [R]) triple, finite, shock >= 0, R <= 2^20;
    weights [N] or [K, N].  garch: (alpha, beta[, h0]) as simulate_paths takes it; None takes (alpha, beta, h0) from the FilteredRows
    (a plain triple then needs garch).  alpha = 0 with h0 = 1 is simulate_bootstrap on the rows resid + mu bit for bit.  block: the
    mean block length of simulate_bootstrap (1: classical FHS).  horizons / levels: simulate_paths' horizons / bands.  Returns what
    simulate_bootstrap returns for the same arguments (pivots of SPEC.md 5.11).  Simple compounding only: ValueError for
    compounding="log" and for the simulate_paths keywords that have no meaning here (dof, fold, native_math, drawdown, rebalance,
    cashflow, overlay, attribution, antithetic).  downside as in simulate_paths (SPEC.md 5.22; not with as_array)."""
    from .downside import check_downside
    ds = check_downside(downside)
    if ds is not None and as_array:
        raise ValueError("downside fills the 'downside' block of the result dicts: not with as_array")
    bm = _check_benchmark(benchmark, weights, as_array, shard)
    comp = unsupported.pop("compounding", "simple")
    if comp != "simple":
        raise ValueError(f"simulate_filtered compounds simply: not with compounding={comp!r}")
    if unsupported:
        raise ValueError(f"simulate_filtered does not take {sorted(unsupported)}: filtered rows combine with garch, block and horizons "
                         "only (SPEC.md 4.11)")
    if garch is None:
        if not hasattr(filtered, "h0"):
            raise ValueError("garch=None needs a FilteredRows (filter_rows(...)): a (mu, resid, shock) triple carries no (alpha, beta, h0)")
        garch = (filtered.alpha, filtered.beta, filtered.h0)
    gv = check_garch(garch)
    b = float(block)
    if not b >= 1.0:
        raise ValueError(f"block (mean block length) must be >= 1 or inf, got {block!r}")
    steps, lv = _check_walk(n_steps, horizons, levels, None, "simple", shard)
    mu, resid, shock, W = filtered_inputs(filtered, weights)
    prm, ctx = _setup(resid.shape[1], n_steps, W.shape[0], "simple", v0, alpha, rf, False, False, devices, shard, context)
    out = ctx.simulate_filtered(prm, (mu, resid, shock), gv, W, b, int(seed), int(path_begin), int(n_paths), store, horizons=steps,
                                levels=lv, downside=ds, benchmark=bm)
    return _result(out, np.asarray(weights).ndim == 1, store, as_array, steps, lv, "simple")


def simulate_sweep(mu, cov, weights=None, n_portfolios=2500, min_weights=None, max_weights=None, n_steps=252,
                   n_paths=100_000, seed=0, rf=0.0, alpha=0.95, method="Monte Carlo", np_seed=None, **kw):
    """The reference's sweep (app.py:682-722) scored on SIMULATED terminal values instead of historical rows:
    weights drawn exactly as app.py:699-707 (host, NumPy legacy RNG; pass `weights` to supply them), all
    portfolios on common random numbers in one launch (MFMA kernel for K >= 17), metric and optimum as at
    app.py:672-676 / 717 / 747.  -> dict(all_weights, stats [K] record array, all_metrics, opt_idx); drawdown=True adds
    'drawdown_stats', the [K] record array of the per-path max drawdowns (simulate_paths)."""
    from .sweep import _METRIC, draw_weights, select_optimum
    if weights is None:
        if np_seed is not None:
            np.random.seed(np_seed)
        weights = draw_weights(len(np.atleast_1d(mu)), n_portfolios, min_weights, max_weights)
    W = np.atleast_2d(np.asarray(weights, np.float64))
    if kw.get("horizons") is not None or len(np.atleast_1d(np.asarray(kw.get("bands", ()), np.float64))):
        raise ValueError("simulate_sweep does not take horizons or bands: call simulate_paths for the optimum")
    if kw.get("cashflow") is not None or kw.get("target") is not None:
        raise ValueError("simulate_sweep does not take cashflow or target: call simulate_paths for the optimum")
    if kw.get("glide") is not None:
        raise ValueError("simulate_sweep does not take glide: call simulate_paths for the optimum")
    if kw.get("protect") is not None:
        raise ValueError("simulate_sweep does not take protect: call simulate_paths for the optimum")
    if kw.get("spending") is not None:
        raise ValueError("simulate_sweep does not take spending: call simulate_paths for the optimum")
    if kw.get("tolerance") is not None:
        raise ValueError("simulate_sweep does not take tolerance: call simulate_paths for the optimum")
    if kw.get("vol_target") is not None:
        raise ValueError("simulate_sweep does not take vol_target: call simulate_paths for the optimum")
    if kw.get("underwater"):
        raise ValueError("simulate_sweep does not take underwater: call simulate_paths for the optimum")
    if kw.get("drift_uncertainty") is not None:
        raise ValueError("simulate_sweep does not take drift_uncertainty: call simulate_paths for the optimum")
    if kw.get("benchmark") is not None:
        raise ValueError("simulate_sweep does not take benchmark: the sweep returns record arrays -- call simulate_paths for the optimum")
    if kw.get("downside") is not None:
        raise ValueError("simulate_sweep does not take downside: the sweep returns record arrays -- call simulate_paths for the optimum")
    if kw.get("attribution"):
        raise ValueError("simulate_sweep does not take attribution: call simulate_paths for the optimum")
    kw.pop("attribution", None)
    if kw.get("antithetic"):
        raise ValueError("simulate_sweep does not take antithetic: the sweep ranks the portfolios on common random numbers -- call "
                         "simulate_paths(antithetic=True) for the optimum, whose mean then carries its standard error")
    kw.pop("antithetic", None)
    drawdown = bool(kw.get("drawdown", False))
    stats = simulate_paths(mu, cov, W, n_steps=n_steps, n_paths=n_paths, seed=seed, rf=rf, alpha=alpha, as_array=True, **kw)
    dd_stats = None
    if drawdown:
        stats, dd_stats = stats[0], stats[1]
    metric = {"sharpe": stats["sharpe"], "var_95": -stats["var"], "cvar_95": -stats["cvar"]}[_METRIC[method]]
    out = {"all_weights": W, "stats": stats, "all_metrics": metric, "opt_idx": select_optimum(method, metric),
           "all_risks": stats["std"], "all_returns": stats["mean"]}
    if drawdown:
        out["drawdown_stats"] = dd_stats
    return out

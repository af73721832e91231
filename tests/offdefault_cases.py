"""One small off-default case per public walk family (test helper, not a test module): a 64-bit seed whose two words are both
non-zero, path ids whose high word is 6 .. 7 or sits at 2^63, and a market of both signs with a short and a leveraged book.

Nearly every GPU test of the suite runs on a seed below 2^32 (Philox key word k1 = 0), on path ids whose high word is 0 or 1, and on
long-only weights.  A seed cut to 32 bits, a high counter word assumed uniform over a launch or a sign lost in |W| would pass all of
them.  The cases here are the inputs that would not; each is held to the restatement its family already has (tests/*_ref.py, and
oracle.mc_oracle for the plain walk).  tests/test_offdefault_cases_cpu.py proves on the restatements alone that every case moves
under those mistakes; tests/test_gpu_offdefault.py runs them on the device.

A case is (id, entry, comp, K, scale, begin, n, kw, ref, kind, prm):
    entry   the mcp_simulate* entry point Context._call takes for `kw` (checked on the CPU through the recorder)
    kw      the feature keywords of Context._call (mu and chol included where the draws are Gaussian)
    ref     ref(seed, paths, wmap) -> {field of simulate._Outputs: array}; `wmap` is applied to every weight array (identity, or
            np.abs for the sign test)
    kind    'clamped' (a walk with the ruin clamp to +0), 'floor' (floor protection: no ruin, three exposure branches) or 'free'
    prm     keywords of _ffi.make_params beyond the shared ones (native_math, fold)

WHAT THE ARGUMENT RULES REFUSED: nothing.  Negative weights, a leveraged row, ids at 2^63 and the seed are accepted by every entry
point.  Antithetic pairs need an even path_begin and an even path count, so those cases run 1026 paths from the even begins below
(513 pairs whose pair ids cross a multiple of 2^32, as tests/test_gpu_antithetic.py arranges); attribution takes simple compounding
only; the folded step and the lean kernel exist for one portfolio only and run on the long/short row alone.
"""
from __future__ import annotations

import collections
import functools
import os
import re

import numpy as np

import antithetic_ref
import attribution_ref
import band_ref
import bootstrap_ref
import drawdown_ref
import fhs_ref
import garch_ref
import horizons_ref
import jump_ref
import lifetime_ref
import native_ref
import overlay_ref
import protect_ref
import rebalance_ref
import regime_ref
import spend_ref
import student_t_ref
import uncertain_ref
import underwater_ref
import voltarget_ref
from monte_carlo_portfolio_amd import _ffi, options
from monte_carlo_portfolio_amd.simulate import check_overlay
from oracle import mc_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Both words non-zero and different, bit 31 of each set (a sign extension of either shows), bit 63 set (a signed conversion shows).
SEED64 = 0xC0FFEE8D_9E3779B1
assert (SEED64 >> 32) != (SEED64 & 0xFFFFFFFF) and (SEED64 >> 31) & 1 and SEED64 >> 63 and (SEED64 >> 32) and (SEED64 & 0xFFFFFFFF)

N, T, HZ, NP, V0, ALPHA, RF = 5, 9, (2, 9), 513, 2.5, 0.9, 0.003
LEVELS = (5.0, 50.0, 95.0)
INT_LEVELS = (5.0, 50.0, 95.0)
BEGIN_HI = (7 << 32) - 200                       # 200 paths with p_hi = 6, 313 with p_hi = 7
BEGIN_TOP = (1 << 63) + (1 << 32) - 200          # p_hi = 2^31 and 2^31 + 1
PAIR_NP = 2 * NP
PAIR_BEGIN_HI = 2 * BEGIN_HI                     # the pair ids are the range above
PAIR_BEGIN_TOP = (1 << 63) + (2 << 32) - 400     # pair ids from 2^62 + 2^32 - 200
LEAN_BEGIN = BEGIN_HI - 313                      # 513 paths that all have p_hi = 6: mcp::lean_range holds
assert (LEAN_BEGIN + NP - 1) >> 32 == LEAN_BEGIN >> 32 == 6 and (BEGIN_HI + NP - 1) >> 32 == 7
assert BEGIN_TOP + NP < 1 << 64 and PAIR_BEGIN_TOP + PAIR_NP < 1 << 64 and PAIR_BEGIN_HI % 2 == 0 and PAIR_BEGIN_TOP % 2 == 0

# The volatility scales (a factor on the Cholesky factor below), chosen on the restatements; the shares they give are stated in the
# docstring of tests/test_offdefault_cases_cpu.py.
MODERATE = 0.05          # the clamped families: some paths are ruined, most are not
LARGE = 0.45             # the families without a clamp: the leveraged row's V goes through zero on some paths
VT_SCALE = 0.12          # the volatility target: its own leverage does the rest
PROTECT_SCALE = 0.10     # floor protection: the cushion is lost on some paths, the cap binds on others

_f32 = np.float32


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- the market -----------------------------------------------------------------------------------------------------------------

W3 = _ro(np.array([[0.30, 0.25, 0.20, 0.15, 0.10],                  # long only
                   [0.90, -0.40, 0.50, -0.30, 0.30],                # long / short, sums to 1
                   [1.10, 0.70, -0.50, 0.30, 0.20]], np.float32))   # leveraged (sums to 1.8) with a short leg
W1 = _ro(W3[1:2].copy())
LONG_SHORT, LEVERAGED = 1, 2


@functools.lru_cache(maxsize=None)
def weights(K):
    """[K, N] binary32: W3's rows first; beyond them every row is one of W3's with a pattern of both signs added, all rows distinct."""
    if K == 1:
        return W1
    k = np.arange(K, dtype=np.float64)[:, None]
    i = np.arange(N, dtype=np.float64)[None, :]
    W = W3.astype(np.float64)[np.arange(K) % 3] + np.where(k >= 3, 0.07 * np.sin(1.0 + 0.9 * k + 2.3 * i), 0.0)
    W = W.astype(np.float32)
    assert np.unique(W, axis=0).shape[0] == K and np.array_equal(W[:3], W3)
    return _ro(W)


@functools.lru_cache(maxsize=None)
def market(scale):
    """(mu [N], L [N, N]) binary32, read-only, after native_ref.market: a drift of both signs with N distinct entries and a dense
    lower-triangular factor of both signs with a positive diagonal, N (N + 1) / 2 distinct entries, times `scale`."""
    mu = np.array([0.021, -0.013, 0.017, -0.008, 0.011])
    L = np.array([[1.00, 0.00, 0.00, 0.00, 0.00],
                  [0.35, 0.90, 0.00, 0.00, 0.00],
                  [-0.28, 0.22, 0.80, 0.00, 0.00],
                  [0.31, -0.26, 0.18, 0.70, 0.00],
                  [-0.15, 0.33, -0.24, 0.12, 0.60]]) * scale
    mu32, L32 = mu.astype(np.float32), L.astype(np.float32)
    low = L32[np.tril_indices(N)]
    assert np.unique(low).size == low.size and np.all(np.diag(L32) > 0) and (low < 0).any() and np.unique(mu32).size == N
    return _ro(mu32, L32)


@functools.lru_cache(maxsize=None)
def market16():
    """native_ref.market at N = 16, K = 1 for the lean kernel's second width."""
    return native_ref.market(16, 1)


@functools.lru_cache(maxsize=None)
def rows_table(R, scale):
    """[R, N] binary32 observed returns of both signs: fixed normals through the market's factor, plus its drift."""
    mu, L = market(scale)
    z = np.random.default_rng(0xB007).standard_normal((R, N))
    return _ro((mu.astype(np.float64) + z @ L.astype(np.float64).T).astype(np.float32))


@functools.lru_cache(maxsize=None)
def filtered_triple(R, scale):
    """(mu [N], resid [R, N], shock [R]) binary32 of a filtered request: the rows above less the drift, shocks around 1."""
    mu, _ = market(scale)
    resid = (rows_table(R, scale).astype(np.float64) - mu.astype(np.float64)).astype(np.float32)
    shock = (0.25 + np.random.default_rng(0xF115).chisquare(3, R) / 4.0).astype(np.float32)
    return _ro(mu.copy(), resid, shock)


R_LDS, R_GLOBAL = 100, 700                       # R ceil(N / 4) <= 1088: the table sits in LDS; above: in global memory
BLOCK = 3.0
GARCH = (0.1, 0.85, 1.5)
DOF = 5
JUMPS = (0.3, -0.05, 0.04, _ro(np.array([1.0, 0.5, -0.5, 1.5, 0.8], np.float32)))
FLOWS = _ro(np.array([-0.30, -0.25, 0.15, -0.35, -0.30, -0.25, 0.10, -0.35, -0.30], np.float32))
TARGET = 1.0
SPENDING = (0.16, 2, 0.35, 1.0, 0.01, None)       # rate, every, down, up, inflation, first
GLIDE_BREAKS = _ro(np.array([4], np.int32))
PROTECT_TARGET = 2.4
BAND_EVERY, BAND_COST, BAND_TOL = 2, 1e-3, (0.06, 0.15, 0.20)   # per row of W3; the one-portfolio case: the long/short row's
REB_PERIOD, REB_COST = 2, 1e-3


def glide_targets(W):
    """[1, K, N] binary32: after the break every portfolio holds its weights in reverse order (the signs move to other assets)."""
    return np.ascontiguousarray(W[None, :, ::-1]).astype(np.float32)


def band_table(W):
    """[K, N] binary32: only assets with a negative weight are watched where the row has one (the long-only row: assets 1 and 3)."""
    tol = np.full(W.shape, np.inf, np.float32)
    for k, w in enumerate(W):
        watch = np.flatnonzero(w < 0) if (w < 0).any() else np.array([1, 3])
        tol[k, watch] = BAND_TOL[LONG_SHORT if len(W) == 1 else k]
    return tol


def regimes_of(scale):
    """(p01, p10, start, mu1, chol1): the crisis regime has the drift's signs turned and twice the factor with column 1 negated."""
    mu, L = market(scale)
    L1 = (2.0 * L).astype(np.float32)
    L1[2:, 1] = -L1[2:, 1]
    return 0.2, 0.3, 0.4, (-1.5 * mu).astype(np.float32), L1


def overlay_triple():
    """A protective put on asset 1 (short in two rows), stock plus a short call on asset 3, a long call on asset 4."""
    B, S, LC, SC, LP, SP, SF = options.ROW_TYPES
    spot = 20.0 + 7.5 * np.arange(N)
    ov = {1: [(B, 0, 0, 1.0), (LP, 0.9 * spot[1], 0.01 * spot[1], 1.0)], 3: [(B, 0, 0, 1.0), (SC, 1.1 * spot[3], 0.02 * spot[3], 1.0)],
          4: [(LC, spot[4], 0.05 * spot[4], 1.0)]}
    return check_overlay(ov, spot, N)


def protect_of(which):
    """(floor [T + 1], multiplier, rate, cap, ratchet): a stepped floor that reaches all three exposure branches, or a ratchet."""
    floor = (0.8 * V0 * (1.0 + RF) ** np.arange(T + 1)).astype(np.float32)
    if which == "step":
        floor[T // 2:] += _f32(0.1 * V0)
        return floor, 5.0, RF, 1.5, 0.0
    return floor, 5.0, RF, 1.0, 0.8


VOL_TARGET = (0.35, 0.8, 12.0, RF, 0.002, None)   # target, decay, cap, rate, spread, s0 (None: the Gaussian part's variance)


def drift_factor(scale):
    """The binary32 lower-triangular M [N, N] of a drift-uncertainty request, of both signs."""
    M = np.tril(0.15 * scale * np.array([[1.0, 0, 0, 0, 0], [-0.5, 0.9, 0, 0, 0], [0.4, 0.3, 0.8, 0, 0], [0.2, -0.6, 0.1, 0.7, 0],
                                           [-0.3, 0.2, 0.5, -0.4, 0.6]]))
    return np.ascontiguousarray(M, np.float32)


# ---- the restatements -------------------------------------------------------------------------------------------------------------

def segments(paths):
    """A list of (begin, count) of the runs of consecutive ids in `paths` (the C oracle and native_ref walk ranges)."""
    p = [int(v) for v in np.asarray(paths, np.uint64)]
    cuts = [0] + [i for i in range(1, len(p)) if p[i] != p[i - 1] + 1] + [len(p)]
    return [(p[a], b - a) for a, b in zip(cuts, cuts[1:])]


def _std(r, dd=False, hz=False):
    out = {"terminal": r["V_T"]}
    if dd:
        out["qd"] = r["q"]
    if hz:
        out["horizon_terminal"] = r["V_h"]
    return out


Case = collections.namedtuple("Case", "id entry comp K scale begin n kw ref kind prm")


def _case(id_, entry, kw, ref, comp="simple", K=3, scale=LARGE, begin=BEGIN_HI, n=NP, kind="free", **prm):
    return Case(id_, entry, comp, K, scale, begin, n, kw, ref, kind, prm)


def params(c, **over):
    """The mcp_params of a case."""
    kw = dict(compounding=c.comp, v0=V0, alpha=ALPHA, rf=RF)
    kw.update(c.prm)
    kw.update(over)
    return _ffi.make_params(N, T, c.K, **kw)


def _build():
    cases = []
    flip = [0]

    def begin(pairs=False):
        """BEGIN_HI and BEGIN_TOP in turn, so that both ranges run on every part of the ladder."""
        flip[0] ^= 1
        return ((PAIR_BEGIN_HI, PAIR_BEGIN_TOP) if pairs else (BEGIN_HI, BEGIN_TOP))[flip[0]]

    def gauss(scale):
        mu, L = market(scale)
        return dict(mu=mu, chol=L)

    # -- the plain walk: K = 1 (mc_paths_kernel on a crossing range; the lean kernel has a test of its own), K = 3, K = 40 (MFMA sweep)
    for comp in ("simple", "log"):
        for K in (1, 3, 40):
            mu, L = market(LARGE)

            def ref(seed, paths, wmap, K=K, comp=comp, mu=mu, L=L, fold=False):
                return {"terminal": np.concatenate([mc_oracle.simulate(mu, L, wmap(weights(K)), T, cnt, seed, b, V0, comp, fold=fold)
                                                    for b, cnt in segments(paths)], axis=1)}
            cases.append(_case(f"plain-K{K}-{comp}", "mcp_simulate", gauss(LARGE), ref, comp, K, begin=begin()))
            if K == 1:
                cases.append(_case(f"fold-K1-{comp}", "mcp_simulate", gauss(LARGE), functools.partial(ref, fold=True), comp, 1, begin=begin(),
                                   fold=True))

        def ref(seed, paths, wmap, comp=comp):                  # float64: held to native_ref.tolerance, not to the bit
            mu, L = market(LARGE)
            return {"terminal": np.concatenate([native_ref.simulate_native_f64(mu, L, wmap(W3), T, cnt, seed, b, V0, comp)
                                                for b, cnt in segments(paths)], axis=1)}
        cases.append(_case(f"native-{comp}", "mcp_simulate", gauss(LARGE), ref, comp, begin=begin(), native_math=True))

        def ref(seed, paths, wmap, comp=comp):
            mu, L = market(LARGE)
            return _std(drawdown_ref.simulate_paths_dd(mu, L, wmap(W3), T, seed, paths, comp, V0), dd=True)
        cases.append(_case(f"drawdown-{comp}", "mcp_simulate_drawdown", dict(gauss(LARGE), drawdown=True), ref, comp, begin=begin()))

        def ref(seed, paths, wmap, comp=comp):
            mu, L = market(LARGE)
            return _std(horizons_ref.simulate_horizons(mu, L, wmap(W3), T, seed, paths, HZ, comp, V0), hz=True)
        cases.append(_case(f"horizons-{comp}", "mcp_simulate_horizons", dict(gauss(LARGE), horizons=HZ, levels=LEVELS), ref, comp, begin=begin()))

        for where, R in (("lds", R_LDS), ("global", R_GLOBAL)):
            def ref(seed, paths, wmap, comp=comp, R=R, hz=()):
                return _std(bootstrap_ref.simulate_boot(rows_table(R, LARGE), wmap(W3), T, seed, paths, BLOCK, comp, V0, hz), hz=bool(hz))
            cases.append(_case(f"bootstrap-{where}-{comp}", "mcp_simulate_bootstrap", dict(rows=rows_table(R, LARGE), block=BLOCK), ref, comp,
                               begin=begin()))
            cases.append(_case(f"bootstrap-hz-{where}-{comp}", "mcp_simulate_bootstrap_horizons",
                               dict(rows=rows_table(R, LARGE), block=BLOCK, horizons=HZ, levels=LEVELS), functools.partial(ref, hz=HZ), comp,
                               begin=begin()))

        def ref(seed, paths, wmap, comp=comp, dd=False, hz=()):
            mu, L = market(LARGE)
            return _std(uncertain_ref.simulate(mu, L, drift_factor(LARGE), wmap(W3), T, seed, paths, comp, V0, dd, hz), dd=dd, hz=bool(hz))
        du = dict(gauss(LARGE), drift_uncertainty=drift_factor(LARGE))
        cases.append(_case(f"uncertain-{comp}", "mcp_simulate_uncertain", du, ref, comp, begin=begin()))
        cases.append(_case(f"uncertain-dd-{comp}", "mcp_simulate_uncertain", dict(du, drawdown=True), functools.partial(ref, dd=True), comp,
                           begin=begin()))
        cases.append(_case(f"uncertain-hz-{comp}", "mcp_simulate_uncertain", dict(du, horizons=HZ, levels=LEVELS), functools.partial(ref, hz=HZ),
                           comp, begin=begin()))

        def ref(seed, paths, wmap, comp=comp):
            mu, L = market(LARGE)
            r = underwater_ref.simulate(mu, L, wmap(W3), T, seed, paths, comp, V0)
            return {"terminal": r["V_T"], "qd": r["q"], "uw_longest": r["m"], "uw_current": r["c"]}
        cases.append(_case(f"underwater-{comp}", "mcp_simulate_underwater", dict(gauss(LARGE), drawdown=True, underwater=np.array(INT_LEVELS)),
                           ref, comp, begin=begin()))

        def ref(seed, paths, wmap, comp=comp, dd=False, hz=()):
            mu, L = market(LARGE)
            return _std(antithetic_ref.simulate_sampled(mu, L, wmap(W3), T, seed, paths, v0=V0, compounding=comp, horizons=hz), dd=dd, hz=bool(hz))
        cases.append(_case(f"antithetic-dd-{comp}", "mcp_simulate_antithetic", dict(gauss(LARGE), antithetic=True, drawdown=True),
                           functools.partial(ref, dd=True), comp, begin=begin(True), n=PAIR_NP))
        cases.append(_case(f"antithetic-hz-{comp}", "mcp_simulate_antithetic", dict(gauss(LARGE), antithetic=True, horizons=HZ, levels=LEVELS),
                           functools.partial(ref, hz=HZ), comp, begin=begin(True), n=PAIR_NP))

    # -- simple compounding only from here on
    def ref(seed, paths, wmap, dd=False, hz=()):
        mu, L = market(LARGE)
        return _std(antithetic_ref.simulate_sampled(mu, L, wmap(W3), T, seed, paths, garch=GARCH, v0=V0, horizons=hz), dd=dd, hz=bool(hz))
    cases.append(_case("antithetic-garch-dd", "mcp_simulate_antithetic", dict(gauss(LARGE), antithetic=True, garch=GARCH, drawdown=True),
                       functools.partial(ref, dd=True), begin=begin(True), n=PAIR_NP))
    cases.append(_case("antithetic-garch-hz", "mcp_simulate_antithetic", dict(gauss(LARGE), antithetic=True, garch=GARCH, horizons=HZ, levels=LEVELS),
                       functools.partial(ref, hz=HZ), begin=begin(True), n=PAIR_NP))

    def draws_ref(which, scale=LARGE):
        """ref(seed, paths, wmap, dd, hz) of the Student-t, GARCH, GARCH-t, jump and regime walks."""
        def ref(seed, paths, wmap, dd=False, hz=()):
            mu, L = market(scale)
            if which == "t":
                r = student_t_ref.simulate_t(mu, L, wmap(W3), T, seed, paths, DOF, V0, hz)
            elif which in ("garch", "garch-t"):
                r = garch_ref.simulate_garch(mu, L, wmap(W3), T, seed, paths, GARCH, DOF if which == "garch-t" else None, V0, hz)
            elif which == "jumps":
                r = jump_ref.simulate_jumps(mu, L, wmap(W3), T, seed, paths, JUMPS, V0, hz)
            else:
                p01, p10, start, mu1, L1 = regimes_of(scale)
                r = regime_ref.simulate_regimes(mu, L, mu1, L1, wmap(W3), T, seed, paths, (p01, p10, start), V0, hz)
            return _std(r, dd=dd, hz=bool(hz))
        return ref
    draw_kw = {"t": ("mcp_simulate_student_t", dict(dof=DOF)), "garch": ("mcp_simulate_garch", dict(garch=GARCH)),
               "jumps": ("mcp_simulate_jumps", dict(jumps=JUMPS)),
               "regimes": ("mcp_simulate_regimes", dict(regimes=regimes_of(LARGE)))}
    for which, (entry, kw) in draw_kw.items():
        cases.append(_case(f"{which}-dd", entry, dict(gauss(LARGE), drawdown=True, **kw), functools.partial(draws_ref(which), dd=True), begin=begin()))
        cases.append(_case(f"{which}-hz", entry, dict(gauss(LARGE), horizons=HZ, levels=LEVELS, **kw), functools.partial(draws_ref(which), hz=HZ),
                           begin=begin()))

    for where, R in (("lds", R_LDS), ("global", R_GLOBAL)):
        def ref(seed, paths, wmap, R=R):
            f = filtered_triple(R, LARGE)
            return _std(fhs_ref.simulate_fhs(f[0], f[1], f[2], wmap(W3), T, seed, paths, BLOCK, GARCH, V0, HZ), hz=True)
        cases.append(_case(f"filtered-{where}", "mcp_simulate_filtered",
                           dict(filtered=filtered_triple(R, LARGE), garch=GARCH, block=BLOCK, horizons=HZ, levels=LEVELS), ref, begin=begin()))

    def ref(seed, paths, wmap, source="gauss"):
        mu, L = market(LARGE)
        r = (rebalance_ref.gauss_returns(mu, L, T, seed, paths) if source == "gauss"
             else rebalance_ref.boot_returns(rows_table(R_LDS, LARGE), T, seed, paths, BLOCK))
        return _std(rebalance_ref.rebalanced(r, wmap(W3), REB_PERIOD, REB_COST, V0, HZ), hz=True)
    cases.append(_case("rebalanced", "mcp_simulate_rebalanced", dict(gauss(LARGE), period=REB_PERIOD, cost=REB_COST, horizons=HZ, levels=LEVELS),
                       ref, begin=begin()))
    cases.append(_case("rebalanced-boot", "mcp_simulate_rebalanced",
                       dict(rows=rows_table(R_LDS, LARGE), block=BLOCK, period=REB_PERIOD, cost=REB_COST, horizons=HZ, levels=LEVELS),
                       functools.partial(ref, source="boot"), begin=begin()))

    for K, source in ((1, "gauss"), (3, "boot")):
        def ref(seed, paths, wmap, K=K, source=source):
            mu, L = market(LARGE)
            W = weights(K) if K == 1 else W3
            r = (rebalance_ref.gauss_returns(mu, L, T, seed, paths) if source == "gauss"
                 else rebalance_ref.boot_returns(rows_table(R_LDS, LARGE), T, seed, paths, BLOCK))
            b = band_ref.banded(r, wmap(W), band_table(W), BAND_EVERY, BAND_COST, V0, HZ)
            return {"terminal": b["V_T"], "horizon_terminal": b["V_h"], "trades": b["c"], "turnover": b["Y"], "_hits": b["hits"]}
        W = weights(K) if K == 1 else W3
        src = gauss(LARGE) if source == "gauss" else dict(rows=rows_table(R_LDS, LARGE), block=BLOCK)
        cases.append(_case(f"banded-K{K}-{source}", "mcp_simulate_banded",
                           dict(src, tolerance=(BAND_EVERY, BAND_COST, band_table(W), np.array(INT_LEVELS)), horizons=HZ, levels=LEVELS), ref, K=K,
                           begin=begin()))

    for garch in (None, GARCH):
        def ref(seed, paths, wmap, garch=garch):
            mu, L = market(LARGE)
            r = attribution_ref.contributions(mu, L, wmap(W3), T, seed, paths, None, garch, V0)
            return {"terminal": r["V_T"], "contributions": r["A"]}
        cases.append(_case("attribution" + ("-garch" if garch else ""), "mcp_simulate_attribution",
                           dict(gauss(LARGE), attribution=True, **({"garch": garch} if garch else {})), ref, begin=begin()))

    ov = overlay_triple()
    for dd in (False, True):
        def ref(seed, paths, wmap, dd=dd):
            mu, L = market(LARGE)
            return _std(overlay_ref.simulate_ov(mu, L, wmap(W3), T, seed, paths, ov, None, V0, () if dd else HZ), dd=dd, hz=not dd)
        kw = dict(gauss(LARGE), overlay=ov, drawdown=True) if dd else dict(gauss(LARGE), overlay=ov, horizons=HZ, levels=LEVELS)
        cases.append(_case("overlay-dd" if dd else "overlay", "mcp_simulate_overlay", kw, ref, begin=begin()))

    # -- the walks with the ruin clamp, on the moderate scale
    sp_c = spend_ref.consts(SPENDING[0], SPENDING[2], SPENDING[3], SPENDING[4], SPENDING[5], V0)
    for life in (False, True):
        def ref(seed, paths, wmap, which, life=life):
            mu, L = market(MODERATE)
            W = wmap(W3)
            kw = dict(spending=(sp_c, SPENDING[1])) if which == "spending" else dict(flows=FLOWS)
            if which == "glide":
                kw["glide"] = (GLIDE_BREAKS, wmap(glide_targets(W3)))
            r = lifetime_ref.simulate_life(W, T, seed, paths, v0=V0, horizons=HZ, mu=mu, chol=L, **kw)
            out = {"terminal": r["V_T"], "horizon_terminal": r["V_h"]}
            if life:
                out["life"] = r["l"]
            if which == "spending":
                out["withdrawn"] = r["Y_T"]
            return out
        extra = dict(lifetime=np.array(INT_LEVELS)) if life else {}

        def entry(name, life=life):
            return "mcp_simulate_lifetime" if life else name
        tag = "lifetime-" if life else ""
        base = dict(gauss(MODERATE), horizons=HZ, levels=LEVELS, target=TARGET, **extra)
        cases.append(_case(tag + "cashflow", entry("mcp_simulate_cashflow"), dict(base, flows=FLOWS), functools.partial(ref, which="cashflow"),
                           scale=MODERATE, begin=begin(), kind="clamped"))
        cases.append(_case(tag + "glide", entry("mcp_simulate_glide"), dict(base, flows=FLOWS, glide=(GLIDE_BREAKS, glide_targets(W3))),
                           functools.partial(ref, which="glide"), scale=MODERATE, begin=begin(), kind="clamped"))
        cases.append(_case(tag + "spending", entry("mcp_simulate_spending"), dict(base, spending=SPENDING), functools.partial(ref, which="spending"),
                           scale=MODERATE, begin=begin(), kind="clamped"))

    def ref(seed, paths, wmap):
        mu, L = market(MODERATE)
        return _std(uncertain_ref.simulate(mu, L, drift_factor(MODERATE), wmap(W3), T, seed, paths, "simple", V0, False, HZ, FLOWS), hz=True)
    cases.append(_case("uncertain-cf", "mcp_simulate_uncertain",
                       dict(gauss(MODERATE), drift_uncertainty=drift_factor(MODERATE), flows=FLOWS, target=TARGET, horizons=HZ, levels=LEVELS), ref,
                       scale=MODERATE, begin=begin(), kind="clamped"))

    for draw, dkw in (("garch", dict(garch=GARCH)), ("jumps", dict(jumps=JUMPS))):
        for dd in (True, False):
            def ref(seed, paths, wmap, dkw=dkw, dd=dd, which="step" if dd else "ratchet"):
                mu, L = market(PROTECT_SCALE)
                r = protect_ref.simulate_protected(mu, L, wmap(W3), T, seed, paths, protect_of(which), v0=V0, horizons=() if dd else HZ, **dkw)
                return dict(_std(r, dd=dd, hz=not dd), _branch=r["branch"])
            kw = dict(gauss(PROTECT_SCALE), protect=protect_of("step" if dd else "ratchet"), target=PROTECT_TARGET, **dkw)
            kw.update(dict(drawdown=True) if dd else dict(horizons=HZ, levels=LEVELS))
            cases.append(_case(f"protected-{draw}" + ("-dd" if dd else ""), "mcp_simulate_protected", kw, ref, scale=PROTECT_SCALE, begin=begin(),
                               kind="floor"))

            def ref(seed, paths, wmap, dkw=dkw, dd=dd):
                mu, L = market(VT_SCALE)
                W = wmap(W3)
                rho = voltarget_ref.rho_of(mu, L, W, T, seed, paths, **dkw)
                r = voltarget_ref.walk(rho, VOL_TARGET, voltarget_ref.default_s0(L, W), V0, () if dd else HZ)
                out = _std(r, dd=dd, hz=not dd)
                if not dd:
                    out["exposure"] = r["Y"]
                return out
            kw = dict(gauss(VT_SCALE), vol_target=VOL_TARGET, target=TARGET, **dkw)
            kw.update(dict(drawdown=True) if dd else dict(horizons=HZ, levels=LEVELS))
            cases.append(_case(f"voltarget-{draw}" + ("-dd" if dd else ""), "mcp_simulate_vol_target", kw, ref, scale=VT_SCALE, begin=begin(),
                               kind="clamped"))

    # -- the downside request rides another call: the horizons walk and the cash-flow walk
    by_id = {c.id: c for c in cases}
    for src, tau in (("horizons-simple", True), ("cashflow", 0.05)):
        c = by_id[src]
        cases.append(c._replace(id=f"downside-{src}", kw=dict(c.kw, downside=tau)))
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


CASES = _build()
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


def case_weights(c):
    return weights(c.K)


def paths_of(c):
    return np.arange(c.begin, c.begin + c.n, dtype=np.uint64)


def identity(W):
    return W


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """The restatement of a case on SEED64 and its own ids, computed once per process and shared read-only."""
    c = BY_ID[case_id]
    out = c.ref(SEED64, paths_of(c), identity)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def public_entry_points():
    """The mcp_simulate* names the headers under include/ declare."""
    names = set()
    inc = os.path.join(ROOT, "include")
    for f in sorted(os.listdir(inc)):
        if f.endswith(".h"):
            names.update(re.findall(r"^int (mcp_simulate\w*)\(", open(os.path.join(inc, f)).read(), re.M))
    return names

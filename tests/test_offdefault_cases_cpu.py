"""The off-default cases (tests/offdefault_cases.py) have teeth: on the restatements alone, without a device, every case moves under
the mistakes it is there for, its clamps and sign branches are entered on some paths and not on others, the table covers every
public entry point, and the Python front end hands the 64-bit seed and a path_begin above 2^63 through unchanged.

WHAT IS COUNTED.  A case's stored binary32 arrays (terminal values, drawdown q / d, horizon rows, contributions, payout, exposure,
turnover) are pooled and compared bit by bit with a second run of the restatement under one mistake:
    seed       high word zeroed, low word zeroed, the two words swapped       at least 99 % of the values change
    p_hi       zeroed, or taken from the first path for the whole range       at least 40 % change (200 of 513 ids lie before the crossing)
    |W| for W  on the long/short and the leveraged row                        at least 90 % of those rows' values change
The integer records (lifetime, trade count, spells under water) live on T + 1 = 10 values or fewer, so two unrelated runs agree on
most paths whatever the seed; they are not pooled.  They come out of the same walk as the binary32 arrays of their case, whose
sensitivity is counted, and each is asserted to differ under every mistake on at least one path.

OBSERVED (this table on SEED64; the smallest pooled share over the 71 cases, each time the overlay with a drawdown, whose puts floor
two assets): seed high word zeroed 0.9935, low word zeroed 0.9912, words swapped 0.9916; p_hi zeroed 0.9916, p_hi of the first path
0.6053 (313 / 513 = 0.6101 where no value repeats); |W| 0.9722.  The native-math cases, counted as values that move by more than twice
native_ref.tolerance: 0.9987 or more, 0.6101 for the first path's p_hi.
Ruined share of the long-only / long-short / leveraged row in the clamped families (MODERATE = 0.05; the volatility target on
VT_SCALE = 0.12): cash flows 0 / 0 / 0.033, glide 0 / 0 / 0.025, spending 0 / 0 / 0.041, the same with a lifetime 0.033, 0.029, 0.039,
drift uncertainty with flows 0 / 0 / 0.041, volatility target 0.064 / 0.025 / 0.074 on GARCH and 0.068 / 0.010 / 0.062 on jump draws.
The shares are small on purpose: a path ruined in both of two runs keeps its +0, and 99 % of the values have to move.
Share of negative terminal values of the leveraged row, simple compounding, families without a clamp (LARGE = 0.45): 0.255 (overlay
with a drawdown) to 0.485 (GARCH); the plain walk 0.417.
Band cases: the long/short row, which watches only the two assets it is short in, trades at 0.789 (K = 1, Gaussian) and 0.708 (K = 3,
bootstrap) of its reviews.  Floor protection (PROTECT_SCALE = 0.10; it has no ruin, so it is asked for its branches instead): every
case reaches E = 0, E = m C and E = b V, on at least 834 of 13 851 path-steps each; the ratchet binds on about two thirds of them.
"""
import contextlib
import functools
import inspect

import numpy as np
import pytest

import front_end_cases as fe
import native_ref
import offdefault_cases as oc
from monte_carlo_portfolio_amd import _ffi, simulate as sim


class Recorder(fe.Recorder):
    """front_end_cases.Recorder that also takes the downside request, which arms the (here NULL) context before the call."""

    def __getattr__(self, name):
        if name == "mcp_ctx_request_downside":
            return lambda *args: 0
        return super().__getattr__(name)


@contextlib.contextmanager
def recording(real=None):
    with fe.recording(real) as (_, ctx):
        rec = Recorder(real)
        saved, _ffi.lib = _ffi.lib, (lambda: rec)
        try:
            yield rec, ctx
        finally:
            _ffi.lib = saved


MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
HI, LO = oc.SEED64 >> 32, oc.SEED64 & 0xFFFFFFFF
SEEDS = {"seed_hi": LO, "seed_lo": HI << 32, "swapped": (LO << 32) | HI}


def _pairs(c):
    return "antithetic" in c.kw


def _with_hi(c, fn):
    """The case's ids with the high word of the Philox counter replaced by fn(p_hi): the counter holds the path id, or the pair id
    (path id >> 1) on antithetic pairs."""
    p = oc.paths_of(c)
    j = p >> np.uint64(1) if _pairs(c) else p
    j = (fn(j >> S32) << S32) | (j & MASK)
    return (j << np.uint64(1)) | (p & np.uint64(1)) if _pairs(c) else j


PHI = {"p_hi_zero": lambda hi: hi * np.uint64(0), "p_hi_first": lambda hi: hi * np.uint64(0) + hi[0]}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _rows(name, a, ks):
    return a[:, ks] if name == "horizon_terminal" else a[ks]


@functools.lru_cache(maxsize=None)
def _native_tolerance(cid):
    c = oc.BY_ID[cid]
    mu, L = oc.market(c.scale)
    return native_ref.tolerance(native_ref.walk(mu, L, oc.case_weights(c), oc.T, c.n, oc.SEED64, c.begin, oc.V0, c.comp))


def changed(c, other, ks=None):
    """(share of the pooled binary32 stored values whose bits differ, {integer record: differs anywhere}).  The native-math cases are
    held to native_ref.tolerance on the device, not to the bit, so there a value counts as changed when it moved by more than twice
    that tolerance: no device value can then lie within the tolerance of both."""
    base = oc.expected(c.id)
    diff, total, ints = 0, 0, {}
    if c.prm.get("native_math"):
        a, b, tol = base["terminal"], other["terminal"], _native_tolerance(c.id)
        if ks is not None:
            a, b, tol = a[ks], b[ks], tol[ks]
        return float(np.mean(np.abs(a - b) > 2.0 * tol)), ints
    for name, a in base.items():
        if name.startswith("_"):
            continue
        b = other[name]
        if ks is not None:
            a, b = _rows(name, a, ks), _rows(name, b, ks)
        if a.dtype.kind == "f":
            diff += int(np.count_nonzero(_bits(a) != _bits(b)))
            total += a.size
        else:
            ints[name] = bool(np.any(a != b))
    return diff / total, ints


@pytest.mark.parametrize("cid", oc.CASE_IDS)
def test_every_case_moves_under_the_mistakes_it_is_there_for(cid):
    c = oc.BY_ID[cid]
    p = oc.paths_of(c)
    for what, seed in SEEDS.items():
        share, ints = changed(c, c.ref(seed, p, oc.identity))
        print(f"{cid} {what}: {share:.4f} {ints}")
        assert share >= 0.99 and all(ints.values()), (what, share, ints)
    for what, fn in PHI.items():
        q = _with_hi(c, fn)
        assert np.array_equal(q & MASK if not _pairs(c) else (q >> np.uint64(1)) & MASK, (p if not _pairs(c) else p >> np.uint64(1)) & MASK)
        share, ints = changed(c, c.ref(oc.SEED64, q, oc.identity))
        print(f"{cid} {what}: {share:.4f} {ints}")
        assert share >= 0.40 and all(ints.values()), (what, share, ints)
    ks = [0] if c.K == 1 else [oc.LONG_SHORT, oc.LEVERAGED]
    share, ints = changed(c, c.ref(oc.SEED64, p, np.abs), ks)
    print(f"{cid} |W|: {share:.4f} {ints}")
    assert share >= 0.90 and all(ints.values()), (share, ints)


@pytest.mark.parametrize("cid", [c.id for c in oc.CASES if c.kind == "clamped"])
def test_clamped_families_ruin_some_paths_and_not_others(cid):
    V = oc.expected(cid)["terminal"]
    ruined = np.mean(V == 0, axis=1)
    print(f"{cid}: ruined share per row {np.round(ruined, 3).tolist()}")
    assert np.any((ruined > 0.02) & (ruined < 0.98)), ruined
    assert np.all(V >= 0) and not np.any(np.signbit(V)), "the clamp is to +0"


@pytest.mark.parametrize("cid", [c.id for c in oc.CASES if c.kind == "free" and c.comp == "simple" and c.K >= 3])
def test_the_leveraged_row_goes_through_zero_where_nothing_clamps(cid):
    V = oc.expected(cid)["terminal"][oc.LEVERAGED]
    share = float(np.mean(V < 0))
    print(f"{cid}: negative terminal values of the leveraged row {share:.3f}")
    assert 0.01 < share < 0.99, share


@pytest.mark.parametrize("cid", [c.id for c in oc.CASES if c.kind == "floor"])
def test_floor_protection_reaches_every_exposure_branch(cid):
    got = np.bincount(oc.expected(cid)["_branch"].ravel(), minlength=3)
    print(f"{cid}: path-steps per branch (E = 0, m C, b V) {got.tolist()}")
    assert np.all(got > 0), got


@pytest.mark.parametrize("cid", [c.id for c in oc.CASES if "tolerance" in c.kw])
def test_the_band_cases_trade_on_some_reviews_only_and_watch_a_short_asset(cid):
    c = oc.BY_ID[cid]
    W = oc.case_weights(c)
    k = 0 if c.K == 1 else oc.LONG_SHORT
    tol = c.kw["tolerance"][2]
    watched = np.isfinite(tol[k])
    assert watched.any() and np.all(W[k][watched] < 0), "the long/short row watches assets it is short in, and no others"
    hits = oc.expected(cid)["_hits"][:, k]
    print(f"{cid}: the long/short row trades at {hits.mean():.3f} of its reviews")
    assert hits.any() and not hits.all() and 0.05 < hits.mean() < 0.95
    assert np.any(hits.any(axis=0) & ~hits.all(axis=0)), "one path trades at one review and not at another"


def test_the_plain_cases_of_the_c_oracle_equal_the_numpy_restatement():
    """The plain cases take their values from oracle.mc_oracle; the other families' restatements are NumPy's.  Once, on the case's own
    ids: the two are the same walk."""
    import drawdown_ref
    for cid in ("plain-K3-simple", "plain-K3-log"):
        c = oc.BY_ID[cid]
        mu, L = oc.market(c.scale)
        want = drawdown_ref.simulate_paths_dd(mu, L, oc.W3, oc.T, oc.SEED64, oc.paths_of(c), c.comp, oc.V0)["V_T"]
        assert np.array_equal(_bits(oc.expected(cid)["terminal"]), _bits(want))


def test_the_table_names_every_public_entry_point():
    """A family added later without a case fails here: the entry points of the table are those the headers declare."""
    assert {c.entry for c in oc.CASES} == oc.public_entry_points()
    kws = set().union(*(c.kw for c in oc.CASES))
    assert set(sim._KEYWORD_GROUP) <= kws | {"rows"} and "rows" in kws        # every feature keyword of Context._call rides some case
    assert {True, False} == {bool(c.prm.get("native_math")) for c in oc.CASES} == {bool(c.prm.get("fold")) for c in oc.CASES}
    assert {40} <= {c.K for c in oc.CASES}, "the MFMA sweep kernels run at K >= 17"
    assert {oc.BEGIN_HI, oc.BEGIN_TOP, oc.PAIR_BEGIN_HI, oc.PAIR_BEGIN_TOP} == {c.begin for c in oc.CASES}


def _walk_args(args):
    i = args.index(oc.SEED64)
    return args[i:i + 3]


@pytest.mark.parametrize("cid", oc.CASE_IDS)
def test_the_front_end_hands_seed_and_begin_through(cid):
    """Context._call on the case's own keywords reaches the entry point the table names, with seed, path_begin and n_paths as given."""
    c = oc.BY_ID[cid]
    with recording() as (rec, ctx):
        ctx._call(oc.params(c), oc.case_weights(c), oc.SEED64, c.begin, c.n, True, **c.kw)
    calls = [call for call in rec.calls if call[0] == c.entry]
    assert len(calls) == 1 and len(rec.calls) == 1, rec.calls
    assert _walk_args(calls[0][1]) == [oc.SEED64, c.begin, c.n]


def _wrapper_calls():
    """Every Context.simulate_* method on the inputs of a case of the table, seed and path_begin by position."""
    S, B, n = oc.SEED64, oc.BEGIN_TOP, oc.NP
    mu, L = oc.market(oc.LARGE)
    W, rows, hz, lv = oc.W3, oc.rows_table(oc.R_LDS, oc.LARGE), oc.HZ, oc.LEVELS
    prm = _ffi.make_params(oc.N, oc.T, 3, v0=oc.V0)
    return {
        "simulate": lambda c: c.simulate(prm, mu, L, W, S, B, n, True),
        "simulate_drawdown": lambda c: c.simulate_drawdown(prm, mu, L, W, S, B, n, True),
        "simulate_horizons": lambda c: c.simulate_horizons(prm, mu, L, W, S, B, n, hz, lv, True),
        "simulate_bootstrap": lambda c: c.simulate_bootstrap(prm, rows, W, oc.BLOCK, S, B, n, True),
        "simulate_bootstrap_horizons": lambda c: c.simulate_bootstrap_horizons(prm, rows, W, oc.BLOCK, S, B, n, hz, lv, True),
        "simulate_rebalanced": lambda c: c.simulate_rebalanced(prm, 2, 1e-3, W, S, B, n, True, mu=mu, chol=L),
        "simulate_banded": lambda c: c.simulate_banded(prm, 2, 1e-3, oc.band_table(W), W, S, B, n, True, mu=mu, chol=L),
        "simulate_student_t": lambda c: c.simulate_student_t(prm, oc.DOF, mu, L, W, S, B, n, True),
        "simulate_garch": lambda c: c.simulate_garch(prm, oc.GARCH, mu, L, W, S, B, n, True),
        "simulate_jumps": lambda c: c.simulate_jumps(prm, oc.JUMPS, mu, L, W, S, B, n, True),
        "simulate_regimes": lambda c: c.simulate_regimes(prm, oc.regimes_of(oc.LARGE), mu, L, W, S, B, n, True),
        "simulate_filtered": lambda c: c.simulate_filtered(prm, oc.filtered_triple(oc.R_LDS, oc.LARGE), oc.GARCH, W, oc.BLOCK, S, B, n, True),
        "simulate_attribution": lambda c: c.simulate_attribution(prm, mu, L, W, S, B, n, True),
        "simulate_antithetic": lambda c: c.simulate_antithetic(prm, mu, L, W, S, B, n + 1, True),
        "simulate_cashflow": lambda c: c.simulate_cashflow(prm, oc.FLOWS, W, S, B, n, True, mu=mu, chol=L),
        "simulate_glide": lambda c: c.simulate_glide(prm, (oc.GLIDE_BREAKS, oc.glide_targets(W)), W, S, B, n, True, flows=oc.FLOWS, mu=mu, chol=L),
        "simulate_spending": lambda c: c.simulate_spending(prm, oc.SPENDING, W, S, B, n, True, mu=mu, chol=L),
        "simulate_lifetime": lambda c: c.simulate_lifetime(prm, W, S, B, n, True, flows=oc.FLOWS, mu=mu, chol=L),
        "simulate_overlay": lambda c: c.simulate_overlay(prm, oc.overlay_triple(), mu, L, W, S, B, n, True),
        "simulate_protected": lambda c: c.simulate_protected(prm, oc.protect_of("step"), mu, L, W, S, B, n, True),
        "simulate_vol_target": lambda c: c.simulate_vol_target(prm, oc.VOL_TARGET, mu, L, W, S, B, n, True),
        "simulate_underwater": lambda c: c.simulate_underwater(prm, mu, L, W, S, B, n, True),
        "simulate_uncertain": lambda c: c.simulate_uncertain(prm, oc.drift_factor(oc.LARGE), mu, L, W, S, B, n, True),
    }


def test_every_context_method_hands_seed_and_begin_through():
    table = _wrapper_calls()
    methods = {name for name, _ in inspect.getmembers(sim.Context, inspect.isfunction) if name.startswith("simulate")}
    assert set(table) == methods, methods ^ set(table)
    with recording() as (rec, ctx):
        for name, call in table.items():
            del rec.calls[:]
            call(ctx)
            assert len(rec.calls) == 1, (name, rec.calls)
            n = oc.NP + 1 if name == "simulate_antithetic" else oc.NP
            assert _walk_args(rec.calls[0][1]) == [oc.SEED64, oc.BEGIN_TOP, n], name


def test_the_public_functions_hand_seed_and_begin_through(mcp_lib):
    """simulate_paths on every feature keyword, simulate_bootstrap, simulate_filtered and simulate_sweep: every library call they make
    carries SEED64 and BEGIN_TOP, and together they reach every entry point but none the table does not name."""
    from monte_carlo_portfolio_amd import options
    mu, cov, w = np.full(3, 1e-3), 1e-4 * np.eye(3), np.array([0.9, -0.4, 0.5])
    base = dict(n_steps=6, n_paths=8, seed=oc.SEED64, path_begin=oc.BEGIN_TOP, store=True)
    paths = {
        "plain": {}, "drawdown": dict(drawdown=True), "horizons": dict(horizons=[2, 6], bands=(5.0, 50.0)), "rebalance": dict(rebalance=2),
        "dof": dict(dof=5), "cashflow": dict(cashflow=-0.01, target=1.0), "garch": dict(garch=(0.05, 0.9)),
        "overlay": dict(overlay={0: [(options.LONG_PUT, 90.0, 1.0, 1.0)]}, spot=[100.0, 100.0, 100.0]),
        "attribution": dict(attribution=True), "antithetic": dict(antithetic=True), "jumps": dict(jumps=(0.1, -0.01, 0.01)),
        "regimes": dict(regimes=(0.05, 0.2, np.full(3, -1e-3), 4e-4 * np.eye(3))), "glide": dict(glide=([2], [[0.5, 0.25, 0.25]])),
        "protect": dict(protect=(0.8, 4.0)), "spending": dict(spending=(0.04, 2, 0.1, 0.2)), "lifetime": dict(cashflow=-0.2, lifetime=True),
        "tolerance": dict(rebalance=2, tolerance=0.05), "vol_target": dict(vol_target=(0.01, 0.9)),
        "underwater": dict(drawdown=True, underwater=True), "drift_uncertainty": dict(drift_uncertainty=1e-5 * np.eye(3)),
        "downside": dict(downside=True), "fold": dict(fold=True), "native_math": dict(native_math=True), "log": dict(compounding="log"),
    }
    returns = np.linspace(-0.02, 0.02, 30).reshape(10, 3)
    reached = set()
    with recording(mcp_lib) as (rec, _):
        def run(what, fn):
            del rec.calls[:]
            fn()
            assert rec.calls, what
            for name, args in rec.calls:
                assert _walk_args(args)[:2] == [oc.SEED64, oc.BEGIN_TOP], (what, name)
                reached.add(name)
        for what, kw in paths.items():
            run(what, lambda: sim.simulate_paths(mu, cov, w, **base, **kw))
        run("bootstrap", lambda: sim.simulate_bootstrap(returns, w, **base))
        run("bootstrap horizons", lambda: sim.simulate_bootstrap(returns, w, horizons=[2, 6], **base))
        run("filtered", lambda: sim.simulate_filtered((np.zeros(3), returns, np.ones(10)), w, garch=(0.05, 0.9), **base))
        run("sweep", lambda: sim.simulate_sweep(mu, cov, weights=np.array([[0.9, -0.4, 0.5], [0.2, 0.3, 0.5]]), n_steps=6, n_paths=8,
                                                seed=oc.SEED64, path_begin=oc.BEGIN_TOP))
    assert reached == oc.public_entry_points(), reached ^ oc.public_entry_points()


def test_seed_and_path_begin_are_64_bit_unsigned_in_every_binding():
    """ctypes converts a Python int to the declared type without a range check on some of them: a c_int or c_int64 seed would take
    SEED64 and hand on something else.  Every mcp_simulate* and mcp_launch_paths* declares seed, path_begin and n_paths c_uint64."""
    import ctypes
    tables = [_ffi.SIMULATE_ENTRIES, _ffi.EXTENSION_ENTRIES, _ffi.SPEND_ENTRIES, _ffi.LIFE_ENTRIES, _ffi.BAND_ENTRIES, _ffi.VOLTARGET_ENTRIES,
              _ffi.UNDERWATER_ENTRIES, _ffi.UNCERTAIN_ENTRIES]
    sigs = [_ffi.SIGNATURES, _ffi.EXTENSION_SIGNATURES, _ffi.SPEND_SIGNATURES, _ffi.LIFE_SIGNATURES, _ffi.BAND_SIGNATURES,
            _ffi.VOLTARGET_SIGNATURES, _ffi.UNDERWATER_SIGNATURES, _ffi.UNCERTAIN_SIGNATURES]
    assert _ffi.ARG_GROUPS["walk"] == [ctypes.c_uint64] * 3
    seen = set()
    for entries, sig in zip(tables, sigs):
        for name, groups in entries.items():
            at = sum(len(_ffi.ARG_GROUPS[g]) for g in groups[:groups.index("walk")])
            assert sig[name][1][at:at + 3] == [ctypes.c_uint64] * 3, name
            seen.add(name)
    assert seen == oc.public_entry_points()
    # include/mcport.h: mcp_launch_paths*(prm, packed, pivots, seed, path_begin, n_paths, ...)
    launches = [n for n in _ffi.SIGNATURES if n.startswith("mcp_launch_paths")]
    assert sorted(launches) == ["mcp_launch_paths", "mcp_launch_paths_drawdown", "mcp_launch_paths_horizons"]
    for name in launches:
        assert _ffi.SIGNATURES[name][1][3:6] == [ctypes.c_uint64] * 3, name
    assert ctypes.c_uint64(oc.SEED64).value == oc.SEED64 and ctypes.c_uint64(oc.BEGIN_TOP).value == oc.BEGIN_TOP

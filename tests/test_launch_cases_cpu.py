"""tests/launch_cases.py checked without a GPU: that the table covers what it claims to, that the assertions of
tests/test_gpu_launch_cases.py (launch_cases.violations: live values plus untouched padding) reject every mistake a store site
could make, in every case that can show it, and what check_request says about a launch that the other CPU tests leave out.

THE CASES THAT CANNOT SHOW A MISTAKE, all by construction and none by a coincidence of the table (test_every_store_mistake_is_
rejected asserts that they are exactly these):

    n_paths for the stride, another array's stride
        the all-equal-strides cases (one per entry point: the layout of the mcp_simulate* calls), and the terminal and drawdown arrays
        of the K = 1 cases, whose one row starts at the array's first element whatever the stride is.  The horizon array of a K = 1
        case has H rows and shows both.
    kt for n_portfolios, no k_begin
        launches of one pass (K <= 8, and the sweeps of one segment), where kt IS n_portfolios and k_begin is 0.
    a dead lane stores
        none: in the equal-strides cases it still lands behind the last row.
"""
import ctypes

import numpy as np
import pytest

import launch_cases as lc
import stats_cases as sc
from monte_carlo_portfolio_amd import _ffi


def test_the_strides_are_what_the_table_says():
    for c in lc.CASES:
        strides = list(c.strides.values())
        assert all(s >= c.n for s in strides), c.id
        assert set(c.strides) == {"paths": {"terminal"}, "drawdown": {"terminal", "mdd"}, "horizons": {"terminal", "horizon"}}[c.entry]
        if c.equal_strides:
            assert set(strides) == {c.n}, c.id
        else:
            assert len(set(strides + [c.n])) == len(strides) + 1, c.id              # pairwise distinct, and none of them n
        for a in c.strides:
            assert lc.alloc_elems(c, a) == c.rows[a] * max(strides) + 64
        assert c.T == 9 and (c.horizons == (2, 5, 9)) == (c.entry == "horizons") and c.horizons in ((), (2, 5, 9))
    regular = [c for c in lc.CASES if not c.equal_strides and c.terminal_stride != c.n + lc.FAR]
    assert {(c.terminal_stride - c.n, c.mdd_stride and c.mdd_stride - c.n, c.hz_stride and c.hz_stride - c.n) for c in regular} == \
        {(3, 0, 0), (3, 5, 0), (3, 0, 2)}
    assert sorted(c.entry for c in lc.CASES if c.equal_strides) == ["drawdown", "horizons", "paths"]
    assert [c.id for c in lc.CASES if c.terminal_stride == c.n + 1000] == ["paths-n16_k9-far"]
    assert {c.n for c in lc.CASES} == {321, 1, 65} and sum(c.n != 321 for c in lc.CASES) >= 2
    assert lc.SEED >> 32 and lc.SEED & 0xFFFFFFFF and lc.FILL_BITS >> 22 == 0x1FF and np.isnan(np.uint32(lc.FILL_BITS).view(np.float32))


def test_the_cases_are_the_ones_asked_for():
    by = {}
    for c in lc.CASES:
        by.setdefault(c.entry, []).append(c)
    plain = [c for c in by["paths"] if c.n == 321 and not c.equal_strides and c.terminal_stride == c.n + 3]
    shape_of = {(s.N, s.K, s.path_begin): s.id for s in sc.SHAPES}
    simple = {shape_of[c.N, c.K, c.path_begin] for c in plain if c.comp == "simple" and c.exact}
    log = {shape_of[c.N, c.K, c.path_begin] for c in plain if c.comp == "log" and c.exact}
    assert simple == set(sc.SHAPE_BY_ID) and log >= set(sc.LOG_SHAPES)
    native = {(c.K, c.comp) for c in plain if c.native}
    assert {K for K, _ in native} == {1, 9, 300} and all(not c.fold for c in plain if c.native)
    assert {(c.K, c.comp) for c in plain if c.fold} == {(1, "simple"), (1, "log")}
    for entry in ("drawdown", "horizons"):
        walks = [c for c in by[entry] if c.n == 321 and not c.equal_strides]
        assert {(c.N, c.K, c.comp) for c in walks} == {(N, K, comp) for N, K in ((5, 1), (16, 1), (5, 3), (16, 9), (20, 20), (5, 17))
                                                        for comp in ("simple", "log")}
        assert all((c.path_begin < sc.TWO32 < c.path_begin + c.n) == ((c.N, c.K) == (16, 1)) for c in walks)
        assert {len(lc.passes_of(c)) for c in walks} == {1, 2, 3} and all(c.exact for c in by[entry])
        # K >= 17 on the one-lane-per-path kernels: six 64-path slots per portfolio against two workgroups, so that launch_paths_impl
        # pads the partials first
        assert any(c.K >= 17 and -(-c.n // 64) > -(-c.n // 256) for c in walks)


def test_the_cases_name_every_launch_level_kernel():
    """mc_paths_kernel at 0, LOGC, NATIVE, NATIVE|LOGC (KT = 1 and 8) and FOLD, FOLD|LOGC (KT = 1 only), the
    lean kernels UHI, UHI|LOGC (KT = 1 only), mc_paths_dd_kernel and mc_paths_hz_kernel at 0 and LOGC (KT = 1 and 8), and the four
    sweep launches of launch_paths_impl: launch_sweep_shared and launch_sweep_paths, each on the spec's and on the native normals."""
    seen = set()
    for c in lc.CASES:
        sel = lc.kernel_of(c.entry, c.N, c.K, c.comp, c.native, c.fold, c.path_begin, c.n)
        assert c.kernel == lc.kernel_name(sel) and c.kernel
        seen.update(sel)
    f = frozenset
    want = {("FAM_PLAIN", f(fl), kt) for fl in ((), ("LOGC",), ("NATIVE",), ("NATIVE", "LOGC")) for kt in (1, 8)}
    want |= {("FAM_PLAIN", f(fl), 1) for fl in (("FOLD",), ("FOLD", "LOGC"), ("UHI",), ("UHI", "LOGC"))}
    want |= {(fam, f(fl), kt) for fam in ("FAM_DD", "FAM_HZ") for fl in ((), ("LOGC",)) for kt in (1, 8)}
    assert want <= seen, want - seen
    assert {s for s in seen if s[0] != "SWEEP"} == want                          # and no selector that has no row in the ladder
    sweeps = {s for s in seen if s[0] == "SWEEP"}
    assert {(shared, native) for _, shared, native, _, _ in sweeps} == {(True, False), (True, True), (False, False), (False, True)}
    assert {(shared, mt) for _, shared, _, _, mt in sweeps} >= {(True, 4), (True, 2), (True, 1), (False, 1), (False, 4)}
    assert {(shared, logc) for _, shared, _, logc, _ in sweeps} == {(True, False), (True, True), (False, False), (False, True)}
    # the names: what a reader of the table sees
    assert lc.BY_ID["paths-n16_k1_lean-simple"].kernel == "mc_paths_lean_kernel UHI KT=1"
    assert lc.BY_ID["paths-n16_k1_across_2p32-log"].kernel == "mc_paths_kernel LOGC KT=1"
    assert lc.BY_ID["paths-n16_k300-native-simple"].kernel == "mc_sweep_shared_kernel MT=2 native + mc_sweep_kernel MT=2 native"
    assert lc.BY_ID["horizons-n5_k17-log"].kernel == "mc_paths_hz_kernel LOGC KT=8"


def test_sweep_plan_restates_the_launch_kinds_of_the_shapes():
    """The segments agree with what stats_cases.Shape.launch says of every sweep shape."""
    for s in sc.SHAPES:
        if s.K < 17:
            continue
        plan = lc.sweep_plan(s.K, (s.N + 3) // 4)
        assert sum(cnt for *_, cnt in plan) == s.K and plan[0][2] == 0
        assert all(a[2] + a[3] == b[2] for a, b in zip(plan, plan[1:]))
        said = s.launch
        if "per-wave sweep" in said:
            assert [(sh, mt) for sh, mt, _, _ in plan] == [(False, {"1 tile": 1, "4 tiles": 4}[said.split(", ")[1]])]
        if "shared draws MT" in said:
            mt = int(said.split("shared draws MT ")[1][0])
            assert (True, mt) in [(sh, m) for sh, m, _, _ in plan], s.id
        if "plus" in said:
            assert len(plan) == 2


def test_work_buffer_sizes_of_the_horizon_recipe(mcp_lib):
    """The launch and the terminal select use the work buffers for K rows, the horizon recipe for H*K rows.  For every buffer but one
    the larger of the two sizes is mcp_ws_bytes(w, H*K, n).  MCP_WS_BELOW is the exception: it holds K * stream_slots(K) doubles,
    stream_slots(K) = 16384 / K rounded down and clamped to 1 .. 2048, which does not grow with K -- 9 rows take 9 * 1820 = 16,380
    doubles, 27 rows 27 * 606 = 16,362.  A buffer sized for H*K rows alone is 18 doubles short for the terminal select of K = 9 (hist(1)
    and hist(2) write slot k * 1820 + block, one block per 8,192 values: the missing slots are reached from about 1.5 * 10^7 paths
    on).  So the rule is the larger of the two for every buffer: mcp_simulate_horizons (tile_buffers), include/mcport.h,
    INTEGRATION.md and launch_cases.ws_bytes state it alike."""
    n_cases, below_shrinks = 0, []
    for c in lc.CASES:
        if c.entry != "horizons":
            continue
        rows = len(c.horizons) * c.K
        sizes = lc.ws_bytes(mcp_lib, c)
        for w in range(_ffi.WS_COUNT):
            own, recipe = mcp_lib.mcp_ws_bytes(w, c.K, c.n), mcp_lib.mcp_ws_bytes(w, rows, c.n)
            assert 0 < own and sizes[w] == max(own, recipe), (c.id, w)
            if w == _ffi.WS_BELOW:
                assert own == 8 * c.K * min(2048, 16384 // c.K) and recipe == 8 * rows * min(2048, 16384 // rows)
                if own > recipe:
                    below_shrinks.append(c.K)
            else:
                assert own <= recipe, (c.id, w)
        n_cases += 1
    assert n_cases >= 13 and sorted(set(below_shrinks)) == [9]
    for c in lc.CASES:                                              # the other launches: the sizes of their own K rows
        if c.entry != "horizons":
            assert lc.ws_bytes(mcp_lib, c) == [mcp_lib.mcp_ws_bytes(w, c.K, c.n) for w in range(_ffi.WS_COUNT)]


def test_restatements_have_the_shapes_and_the_last_horizon_is_the_terminal_row():
    """On three small cases (the GPU test computes the rest): shapes, row order h*K + k, and no FILL_BITS among the values."""
    for cid in ("paths-n16_k9-simple", "drawdown-n5_k3-log", "horizons-n5_k3-simple", "horizons-n5_k17-n65"):
        c = lc.BY_ID[cid]
        want = lc.expected(cid)
        assert set(want) == set(c.strides)
        for a, v in want.items():
            assert v.shape == (c.rows[a], c.n) and v.dtype == np.float32 and not np.any(lc.bits(v) == lc.FILL_BITS)
            assert np.unique(lc.bits(v), axis=0).shape[0] == v.shape[0]                      # no two rows alike
        if c.entry == "horizons":
            assert np.array_equal(lc.bits(want["horizon"][-c.K:]), lc.bits(want["terminal"]))
    assert lc.expected("paths-n16_k9-native-simple") is None and lc.expected("paths-n16_k1-fold-log") is None


def _values(c, array):
    """Stand-ins for a restatement: distinct finite values per row and path (the sensitivity of the layout does not depend on what
    the values are, only on their being different from each other and from the fill)."""
    rows, n = c.rows[array], c.n
    v = (1.0 + np.arange(rows, dtype=np.float64)[:, None] + np.arange(n, dtype=np.float64)[None, :] / 1024.0
         + {"terminal": 0.0, "mdd": 0.25, "horizon": 0.5}[array] / 1024.0)
    return v.astype(np.float32)


def _cannot_show(c, array, mistake):
    one_pass = len(lc.passes_of(c)) == 1
    if mistake in ("n_paths for the stride", "another array's stride"):
        return c.equal_strides or c.rows[array] == 1
    if mistake in ("kt for n_portfolios", "no k_begin"):
        return one_pass
    return False


def _applicable(c, array):
    """(mistake, other stride) pairs of the store site of one array of one case."""
    out = [("n_paths for the stride", None), ("no k_begin", None), ("a dead lane stores", None)]
    out += [("another array's stride", s) for a, s in c.strides.items() if a != array]
    if array == "horizon":
        out.append(("kt for n_portfolios", None))
    return out


def test_every_store_mistake_is_rejected():
    """For every case, every array and every mistake: the correct layout passes violations, the mistaken layout does not -- except
    where the mistaken kernel IS the correct one (the module's docstring), and there the two layouts are equal byte for byte."""
    rejected = {m: 0 for m in lc.MISTAKES}
    exempt = []
    for c in lc.CASES:
        for array, stride in c.strides.items():
            want = _values(c, array)
            right = lc.kernel_store(c, array, want)
            assert lc.violations(right, want, stride, array) == [], c.id
            assert np.array_equal(lc.bits(lc.live_of(right, c.rows[array], c.n, stride)), lc.bits(want))
            for mistake, other in _applicable(c, array):
                wrong = lc.kernel_store(c, array, want, mistake, other)
                complaints = lc.violations(wrong, want, stride, array)
                if _cannot_show(c, array, mistake):
                    assert np.array_equal(wrong, right), (c.id, array, mistake)
                    exempt.append((c.id, array, mistake))
                else:
                    assert complaints, (c.id, array, mistake)
                    rejected[mistake] += 1
    assert all(rejected[m] > 0 for m in lc.MISTAKES), rejected
    # every entry point meets every mistake its arrays can make, in a case that shows it
    for entry, arrays in (("paths", ("terminal",)), ("drawdown", ("terminal", "mdd")), ("horizons", ("terminal", "horizon"))):
        for array in arrays:
            for mistake in lc.MISTAKES:
                if mistake == "another array's stride" and entry == "paths" or mistake == "kt for n_portfolios" and array != "horizon":
                    continue
                assert any(not _cannot_show(c, array, mistake) for c in lc.CASES if c.entry == entry), (entry, array, mistake)
    # the exempt ones, by name: the equal-strides cases, the one-row arrays and the one-pass launches, and nothing else
    stride_exempt = {(cid, a) for cid, a, m in exempt if m == "n_paths for the stride"}
    assert stride_exempt == {(c.id, a) for c in lc.CASES for a in c.strides if c.equal_strides or (c.K == 1 and a != "horizon")}
    pass_exempt = {cid for cid, _, m in exempt if m == "no k_begin"}
    assert pass_exempt == {c.id for c in lc.CASES if c.K <= 8 or (c.entry == "paths" and c.K >= 17 and len(lc.sweep_plan(c.K, (c.N + 3) // 4)) == 1)}
    assert not [e for e in exempt if e[2] == "a dead lane stores"]
    print(f"rejected: {rejected}; cannot show: {len(exempt)} (case, array, mistake) triples")


def test_a_damaged_padding_element_or_live_value_is_reported():
    c = lc.BY_ID["horizons-n16_k9-simple"]
    want = _values(c, "horizon")
    for at, word in ((c.n, "padding"), (c.hz_stride * 5 + c.n + 1, "padding"), (c.rows["horizon"] * c.hz_stride, "behind the last row"),
                     (lc.alloc_elems(c, "horizon") - 1, "behind the last row"), (c.hz_stride * 26 + c.n - 1, "live")):
        buf = lc.kernel_store(c, "horizon", want)
        buf[at] ^= 1
        got = lc.violations(buf, want, c.hz_stride, "horizon")
        assert len(got) == 1 and word in got[0], (at, got)


# ---- what check_request says about a launch ----------------------------------------------------------------------------------------------

def _launch(lib, entry, prm, n, strides, partials=None, hist=None, buf=ctypes.c_void_p(16)):
    """One launch whose device pointers are never dereferenced: check_request refuses it before a device is touched."""
    hz = np.array(lc.HORIZONS, np.int32)
    B = ctypes.byref(prm)
    if entry == "paths":
        return lib.mcp_launch_paths(B, buf, None, lc.SEED, 0, n, buf, strides["terminal"], partials, hist, None)
    if entry == "drawdown":
        return lib.mcp_launch_paths_drawdown(B, buf, None, lc.SEED, 0, n, buf, strides["terminal"], buf, strides["mdd"], partials, hist, None)
    return lib.mcp_launch_paths_horizons(B, buf, None, lc.SEED, 0, n, buf, strides["terminal"], len(hz), hz.ctypes.data_as(ctypes.c_void_p), buf,
                                         strides["horizon"], partials, hist, None)


ARRAYS = {"paths": ("terminal",), "drawdown": ("terminal", "mdd"), "horizons": ("terminal", "horizon")}
STRIDE_NAME = {"terminal": "terminal_stride", "mdd": "mdd_stride", "horizon": "horizon_stride"}


@pytest.mark.parametrize("entry", list(ARRAYS))
def test_argument_rules_of_a_launch(mcp_lib, entry):
    prm = _ffi.make_params(5, lc.T, 3)
    n = lc.N_PATHS
    buf = ctypes.c_void_p(16)
    for short in ARRAYS[entry]:                                      # each stride one below n_paths is refused by name
        strides = {a: n + 7 for a in ARRAYS[entry]}
        strides[short] = n - 1
        assert _launch(mcp_lib, entry, prm, n, strides) == _ffi.MCP_E_ARG
        assert f"{STRIDE_NAME[short]} {n - 1} < n_paths {n}".encode() in mcp_lib.mcp_last_error(), (short, mcp_lib.mcp_last_error())
    ok = {a: n for a in ARRAYS[entry]}
    for partials, hist in ((buf, None), (None, buf)):                # both or neither
        assert _launch(mcp_lib, entry, prm, n, ok, partials, hist) == _ffi.MCP_E_ARG
        assert b"d_partials and d_hist go together" in mcp_lib.mcp_last_error()
    assert _launch(mcp_lib, entry, prm, 0, {a: 0 for a in ARRAYS[entry]}) == _ffi.MCP_E_ARG
    assert b"n_paths must be >= 1" in mcp_lib.mcp_last_error()
    # n_paths = 0 is refused whatever the strides are, and before them
    assert _launch(mcp_lib, entry, prm, 0, {a: 8 for a in ARRAYS[entry]}, buf, buf) == _ffi.MCP_E_ARG
    assert b"n_paths must be >= 1" in mcp_lib.mcp_last_error()

"""The path kernels' normal transform at the ends of the table, draw by draw: the searched Philox words of
tests/golden/icdf_extremes.json (v = 0 next to the LDS pad, every octave's smallest and largest word, u rounding up to 1/2, bin
edges) read back from every kernel kind that turns Philox words into the spec's normals -- block_normals of mcp_device.h in its
interleaved body (mc_paths_kernel, both MFMA sweep kernels) and in its centred body on the binade-scaled table
(mc_paths_lean_kernel).  normals_kernel, which tests/test_gpu_parity.py feeds chosen words, calls normal_icdf and runs neither body.

THE READ-BACK (tests/icdf_extremes.py states why it is exact).  One step, mu = 0, chol = I / 8, unit weight rows.  In log
compounding 8 S is the kernel's z; it is compared with mc_oracle.normals of the same words on bit patterns, a zero draw as +0 (the
step's fma(1/8, -0, +0) is +0).  In simple compounding the terminal bits are those of np.float32(1 + z_ref / 8).  No tolerance.

THE LAUNCH.  Per entry 128 paths from path - 63 on: the extreme word sits in the last lane of wave 0, and the 127 ordinary paths
around it are compared as well, for every selected asset.  Word m of block q is asset m NB + q of a step with NB = ceil(N / 4)
blocks; a shape takes an entry where it draws block q and that slot is an asset, not padding.  Every function prints how many
entries, launches and draws it compared.

Not reached from here: the unfolded one-portfolio kernel at NB <= 4, which runs only when a launch crosses a multiple of 2^32 (the
same template and the same block_normals as its NB = 5 and 8-portfolio instantiations below), and the chi-square and jump normals of
the streams 2 and 3, whose words the fixture's search did not cover.
"""
import numpy as np
import pytest

import icdf_extremes as ix
from monte_carlo_portfolio_amd import simulate_paths

pytestmark = pytest.mark.gpu

MODES = ("log", "simple")


def terminal(N, W, comp, entry, fold=False):
    """float32 [K, 128]: the terminal values of the read-back launch around `entry` for the unit weight rows W."""
    W = np.atleast_2d(np.asarray(W, np.float64))
    assert np.all((W == 0) | (W == 1)) and np.all(W.sum(axis=1) == 1)
    kw = dict(n_steps=1, n_paths=ix.P, seed=entry["seed"], compounding=comp, store=True, path_begin=ix.path_begin(entry),
              chol=np.eye(N) / 8)
    if W.shape[0] == 1:
        term = simulate_paths(np.zeros(N), None, W[0], fold=fold, **kw)["terminal"][None, :]
    else:
        term = simulate_paths(np.zeros(N), None, W, as_array=True, **kw)[1]
    assert term.dtype == np.float32 and term.shape == (W.shape[0], ix.P)
    return term


def assert_draws(term, assets, N, comp, entry, what):
    """Every path and every row of the launch against the oracle's normals of the same words, on bit patterns -> draws compared."""
    z_ref = ix.launch_normals(entry["seed"], ix.path_begin(entry), (N + 3) // 4)[:, assets].T        # [K, 128]
    if comp == "log":
        got, want = term * np.float32(8), z_ref + np.float32(0)             # 8 S is z: a scaling by 2^3, exact
    else:
        got, want = term, (1.0 + z_ref.astype(np.float64) / 8.0).astype(np.float32)
        assert np.array_equal(want.view(np.uint32), ix.expected(z_ref, comp).view(np.uint32))
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        k, p = bad[0]
        x = ix.launch_words(entry["seed"], ix.path_begin(entry), (N + 3) // 4)[p, assets[k]]
        pytest.fail(f"{what} N={N} {comp}, entry {entry}: {len(bad)} of {got.size} draws differ; first at row {k} (asset {assets[k]}), path "
                    f"{ix.path_begin(entry) + p} (lane {p}), word {int(x):#010x}: got {got[k, p]!r} ({int(got.view(np.uint32)[k, p]):#010x}), "
                    f"want {want[k, p]!r} ({int(want.view(np.uint32)[k, p]):#010x})")
    return got.size


class Tally:
    def __init__(self, what, record_property):
        self.what, self.record, self.entries, self.launches, self.draws, self.classes = what, record_property, set(), 0, 0, set()

    def add(self, i, entry, draws):
        self.entries.add(i)
        self.classes.update(ix.classes(entry))
        self.launches += 1
        self.draws += draws

    def close(self):
        """Every entry of the fixture was compared on this kernel kind, so every class was."""
        print(f"{self.what}: {len(self.entries)} entries, {self.launches} launches, {self.draws} draws compared bit for bit")
        self.record("entries", len(self.entries))
        self.record("launches", self.launches)
        self.record("draws", self.draws)
        assert self.entries == set(range(len(ix.ENTRIES)))
        assert {"v_zero", "deep", "rounds_up", "bin_edge"} | {f"octave_{E}" for E in range(1, 33)} <= self.classes


def one_portfolio(what, shapes, record_property, fold=False):
    """The entry's own asset through a one-portfolio kernel, one launch per entry, shape and mode."""
    t = Tally(what, record_property)
    for i, e in enumerate(ix.ENTRIES):
        for N in shapes:
            a = ix.asset_of(e, N)
            if a is None:
                continue
            for comp in MODES:
                t.add(i, e, assert_draws(terminal(N, np.eye(N)[a], comp, e, fold), [a], N, comp, e, what))
    t.close()


def test_lean_kernel_draws_at_the_table_edges(gpu_ctx, record_property):
    """mc_paths_lean_kernel<NB, LOGC>, NB = 1..4 with and without padded assets: the centred transform on the scaled table."""
    one_portfolio("mc_paths_lean_kernel", (4, 8, 12, 16, 5, 13), record_property)


def test_one_portfolio_kernel_draws_at_the_table_edges(gpu_ctx, record_property):
    """mc_paths_kernel<NB, 1, ...>, NB = 5 and 16: N > 16 keeps a one-portfolio launch off the lean kernel."""
    one_portfolio("mc_paths_kernel<NB, 1>", (20, 64), record_property)


def test_folded_kernel_draws_at_the_table_edges(gpu_ctx, record_property):
    """mc_paths_kernel<NB, 1, ...> on the folded step (SPEC.md 4.1), NB = 1 and 4."""
    one_portfolio("mc_paths_kernel<NB, 1> folded", (4, 16), record_property, fold=True)


def test_eight_portfolio_kernel_draws_at_the_table_edges(gpu_ctx, record_property):
    """mc_paths_kernel<NB, 8, ...> with W = I_N: every asset of every path of the launch (N = 13 and 16 run two passes)."""
    t = Tally("mc_paths_kernel<NB, 8>", record_property)
    for i, e in enumerate(ix.ENTRIES):
        for N in (4, 13, 16):
            if ix.asset_of(e, N) is None:
                continue
            for comp in MODES:
                t.add(i, e, assert_draws(terminal(N, np.eye(N), comp, e), list(range(N)), N, comp, e, t.what))
    t.close()


def test_sweep_kernels_draws_at_the_table_edges(gpu_ctx, record_property):
    """mc_sweep_kernel and mc_sweep_shared_kernel, the branches of the sweep plan that test_gpu_native.py names: rows e_(k mod N), so
    every asset is read back by at least one row -- but for N = 20 with K = 17, whose rows stop at asset 16: that shape takes the
    entries whose word it reads."""
    t = Tally("sweep kernels", record_property)
    for i, e in enumerate(ix.ENTRIES):
        for N, K in ((16, 17), (16, 129), (16, 513), (20, 17), (20, 129)):
            assets = [k % N for k in range(K)]
            if ix.asset_of(e, N) not in assets:
                continue
            for comp in MODES:
                t.add(i, e, assert_draws(terminal(N, np.eye(N)[assets], comp, e), assets, N, comp, e, t.what))
    t.close()

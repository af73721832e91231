"""tests/golden/icdf_extremes.json cannot pass vacuously (CPU only): every word is what this project's Philox gives at its address,
every class of tests/golden/make_icdf_extremes.py is present and holds what its name says, the words read every octave of the table
from entry 0 to entry 1024, the two oracles agree on them bit for bit and lie within the bound of tests/test_oracle_rng.py against
float64 ndtri, and the C oracle's own walk leaves exactly the values that tests/test_gpu_icdf_draws.py expects of the kernels.
"""
import numpy as np
import pytest

import icdf_extremes as ix
import native_ref
from oracle import mc_oracle, np_oracle
from test_oracle_rng import NORMAL_REL_BOUND, _math_reference

ENTRIES = ix.ENTRIES
X = np.array([e["x"] for e in ENTRIES], np.uint32)
V = (X & np.uint32(0x7FFFFFFF)).astype(np.int64)
SIGN = (X >> np.uint32(31)).astype(np.int64)


def of_class(name):
    return [i for i, e in enumerate(ENTRIES) if name in ix.classes(e)]


def test_format_and_addresses():
    assert 0 < len(ENTRIES) <= 96 and ix.FIXTURE["n_assets"] == 16 and ix.FIXTURE["step"] == 0
    assert ix.FIXTURE["words_scanned"] == sum(s["words"] for s in ix.FIXTURE["scanned"]) > 0
    assert all(s["words"] == 16 * (s["path_end"] - s["path_first"]) for s in ix.FIXTURE["scanned"])
    seen = set()
    for e in ENTRIES:
        assert set(e) == {"seed", "path", "block", "word", "x", "what"}
        assert ix.LANE <= e["path"] < (1 << 32) - (ix.P - ix.LANE) and 0 <= e["block"] < 4 and 0 <= e["word"] < 4
        assert any(s["seed"] == e["seed"] and s["path_first"] <= e["path"] < s["path_end"] for s in ix.FIXTURE["scanned"])
        seen.add((e["seed"], e["path"], e["block"], e["word"]))
    assert len(seen) == len(ENTRIES)


def test_philox_reproduces_every_word():
    for e in ENTRIES:
        x = native_ref.block_words(e["seed"], np.array([e["path"]], np.uint64), 0, 4, e["block"])[e["word"]][0]
        assert int(x) == e["x"], e
        # and the launch of the GPU test has it in lane 63, in the slot of every shape that draws the block
        for nb in range(e["block"] + 1, 6):
            assert int(ix.launch_words(e["seed"], ix.path_begin(e), nb)[ix.LANE, e["word"] * nb + e["block"]]) == e["x"]


def test_every_class_is_present_and_true():
    known = {"v_zero", "deep", "rounds_up", "bin_edge"} | {f"octave_{E}" for E in range(1, 33)}
    assert all(set(ix.classes(e)) <= known and ix.classes(e) for e in ENTRIES)
    # v_zero: table entry 0, and the C oracle's largest draw
    zero = of_class("v_zero")
    assert zero and all(V[i] == 0 for i in zero) and set(zero) == set(np.flatnonzero(V == 0))
    assert np.all(np.abs(mc_oracle.normals(X[zero])) == np.float32(6.337958))
    # octave_E: one or two words of that octave per E, the ends of what the file holds of it; both signs across the class
    signs = set()
    for E in range(1, 33):
        idx = of_class(f"octave_{E}")
        assert 1 <= len(idx) <= 2 and all(ix.octave(V[i]) == E for i in idx), E
        held = [V[i] for i in range(len(ENTRIES)) if ix.octave(V[i]) == E]
        assert {V[i] for i in idx} == {min(held), max(held)}, E
        signs |= {SIGN[i] for i in idx}
    assert signs == {0, 1}
    assert all(len(of_class(f"octave_{E}")) == 2 for E in range(3, 33))         # octaves 1 and 2 hold one value of v each
    # deep: v < 64, every such word of the file, and the four smallest v all met
    deep = of_class("deep")
    assert set(deep) == set(np.flatnonzero(V < 64)) and {0, 1, 2, 3} <= {V[i] for i in deep}
    # rounds_up: fl32(v) is a power of two above v; the top class (u rounds to 1/2: octave 33, Z = +-0) with either sign
    up = of_class("rounds_up")
    ks = set()
    for i in up:
        f = np.float32(V[i])
        assert float(f) > V[i] and np.float32(f).view(np.uint32) & np.uint32(0x7FFFFF) == 0
        ks.add(int(np.log2(float(f))))
    assert ks <= set(range(25, 32)) and {29, 30, 31} <= ks
    top = [i for i in up if V[i] >= 0x7FFFFFC0]
    assert {SIGN[i] for i in top} == {0, 1}
    assert np.all(ix.table_index(X[top])[0] == 1024) and np.all(mc_oracle.normals(X[top]) == 0.0)
    # bin_edge: four table entries in four octaves, and of each a word at (or next to) its first and one at its last delta
    e_of, delta = ix.table_index(X)
    edge = of_class("bin_edge")
    bins = sorted({int(e_of[i]) for i in edge})
    assert bins == sorted(ix.FIXTURE["bin_entries"]) and len(bins) == 4 and len({b // 32 for b in bins}) == 4
    assert max(b // 32 for b in bins) - min(b // 32 for b in bins) >= 16           # spread over the octaves
    for b in bins:
        d = sorted(int(delta[i]) for i in edge if e_of[i] == b)
        assert len(d) == 2 and d[0] < (1 << 17) < d[1], (b, d)


def test_the_words_read_the_whole_table_range():
    e_of, _ = ix.table_index(X)
    assert {int(e) // 32 + 1 for e in e_of} == set(range(1, 34))                   # the 32 octaves of v and octave 33
    assert e_of.min() == 0 and e_of.max() == 1024
    assert {ix.octave(v) for v in V} == set(range(1, 33))
    # a word reads the octave of its v, or the next one where u = fl32((v + 1/2) 2^-32) rounds up to that octave's first value
    up = np.array(["rounds_up" in ix.classes(e) for e in ENTRIES])
    step = e_of // 32 + 1 - np.array([ix.octave(v) for v in V])
    assert set(step) == {0, 1} and np.all(step[up] == 1)
    assert np.all(ix.table_index(X[step == 1])[1] == 0) and np.all(e_of[step == 1] % 32 == 0)


def test_the_two_oracles_agree_and_meet_the_float64_bound():
    zc, zn = mc_oracle.normals(X), np_oracle.normals(X)
    assert zc.dtype == zn.dtype == np.float32 and np.array_equal(zc.view(np.uint32), zn.view(np.uint32))
    want, _ = _math_reference(X)
    err = np.abs(zc.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
    print(f"largest scaled deviation from float64 ndtri: {err.max():.3e} at x = {int(X[np.argmax(err)]):#x}")
    assert err.max() < NORMAL_REL_BOUND
    # the neighbours in the launches too (np_oracle is slow: the entry's own block only)
    for e in ENTRIES[::8]:
        x = ix.launch_words(e["seed"], ix.path_begin(e), 4)
        z = ix.launch_normals(e["seed"], ix.path_begin(e), 4)
        assert np.array_equal(z.view(np.uint32), np_oracle.normals(x).view(np.uint32))


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("comp", ["log", "simple"])
def test_the_oracle_walk_leaves_the_expected_read_back(comp, fold):
    """What the GPU test expects of a kernel is what mc_oracle.simulate leaves for the same launch: N = 16, every entry, its asset."""
    N = 16
    for e in ENTRIES:
        a = ix.asset_of(e, N)
        z = ix.launch_normals(e["seed"], ix.path_begin(e), 4)
        got = mc_oracle.simulate(np.zeros(N, np.float32), np.eye(N, dtype=np.float32) / 8, np.eye(N, dtype=np.float32)[a], 1, ix.P, e["seed"],
                                 path_begin=ix.path_begin(e), compounding=comp, n_threads=1, fold=fold)[0]
        assert np.array_equal(got.view(np.uint32), ix.expected(z[:, a], comp).view(np.uint32)), e
        if comp == "log":
            z_entry = mc_oracle.normals(np.array([e["x"]], np.uint32)) + np.float32(0)
            assert int((got * np.float32(8)).view(np.uint32)[ix.LANE]) == int(z_entry.view(np.uint32)[0])


def test_asset_of_skips_missing_blocks_and_padding():
    e = {"block": 1, "word": 3}
    assert ix.asset_of(e, 16) == 13 and ix.asset_of(e, 4) is None and ix.asset_of(e, 5) is None and ix.asset_of(e, 8) == 7
    assert ix.asset_of(e, 13) is None and ix.asset_of(e, 20) == 16 and ix.asset_of(e, 64) == 49
    assert ix.asset_of({"block": 0, "word": 1}, 5) == 2 and ix.asset_of({"block": 0, "word": 2}, 5) == 4

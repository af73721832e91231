"""The searched Philox words at the ends of the spec's normal transform (tests/golden/icdf_extremes.json, written by
tests/golden/make_icdf_extremes.py) and what the draw read-back of tests/test_gpu_icdf_draws.py expects of them.  Test
infrastructure, no device.

THE READ-BACK.  One step with mu = +0, chol = 2^-3 I and a unit weight row e_i leaves, in the recurrence of SPEC.md section 4,
r_i = fma(2^-3, z_i, +0) and rho = r_i with no rounding: every other fma has a zero factor, and a power-of-two scaling of
|z| in [2^-30, 8) is exact.  The folded step (SPEC.md 4.1: c = 0, v_j = 2^-3 for j = i and 0 elsewhere) and the MFMA sweep
(one non-zero product per row) give the same.  So

    log compounding       S = +0 + rho = z_i / 8,  and 8 S is the kernel's z_i bit for bit -- but for the sign of a zero:
                          z = -0 (u = 1/2 under a set bit 31) enters fma(2^-3, -0, +0) = +0, as IEEE 754 has it.  expected()
                          therefore adds +0 to z / 8, which changes that one bit pattern and no other.
    simple compounding    V = fma(1, rho, 1) = fl32(1 + z_i / 8): one rounding.

tests/test_icdf_extremes_cpu.py holds the C oracle's own walk (mc_oracle.simulate, folded and unfolded) to exactly these values.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from oracle import mc_oracle, np_oracle

FIXTURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icdf_extremes.json")))
ENTRIES = FIXTURE["entries"]
SCAN_NB = (FIXTURE["n_assets"] + 3) // 4     # the entries' blocks are q = 0 .. SCAN_NB - 1 of step 0
P = 128                                      # paths per launch: two waves, a workgroup's first half or more
LANE = 63                                    # the entry's path is path_begin + LANE, the last lane of wave 0


def classes(entry) -> list:
    return entry["what"].split("+")


def octave(v: int) -> int:
    """E of the issue's notation: 1 for v = 0, otherwise floor(log2(v + 1/2)) + 2."""
    return 1 if v == 0 else int(v).bit_length() + 1


def table_index(x):
    """(e, delta) of SPEC.md section 3 for words x: the table entry 0..1055 that the word reads and its 18-bit delta."""
    x = np.asarray(x, np.uint32)
    v = (x & np.uint32(0x7FFFFFFF)).astype(np.float32)
    u = np_oracle._fma32(v, np.float32(2.0 ** -32), np.float32(2.0 ** -33))
    b = u.view(np.uint32) - np.uint32(np_oracle.ICDF_E_LO << 23)
    return (b >> np.uint32(18)).astype(np.int64), (b & np.uint32(0x3FFFF)).astype(np.int64)


def path_begin(entry) -> int:
    return entry["path"] - LANE


def asset_of(entry, N: int):
    """Word m of block q is asset m NB + q of a step with NB = ceil(N / 4) blocks: that asset, or None where the step draws no block q
    or the slot is padding."""
    nb = (N + 3) // 4
    a = entry["word"] * nb + entry["block"]
    return a if entry["block"] < nb and a < N else None


@functools.lru_cache(maxsize=None)
def launch_words(seed: int, begin: int, nb: int) -> np.ndarray:
    """x uint32 [P, 4 nb] of step 0: column m nb + q is word m of Philox block q.  Computed once per launch, shared, read-only."""
    paths = np.arange(begin, begin + P, dtype=np.uint64)
    x = np.empty((P, 4 * nb), np.uint32)
    for q in range(nb):
        xs = np_oracle.philox4x32_10(np.uint64(q), np.uint64(0), paths & np.uint64(0xFFFFFFFF), paths >> np.uint64(32),
                                     seed & 0xFFFFFFFF, seed >> 32)
        for m in range(4):
            x[:, m * nb + q] = xs[m]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def launch_normals(seed: int, begin: int, nb: int) -> np.ndarray:
    """z float32 [P, 4 nb]: the C oracle's normals of launch_words.  Computed once per launch, shared, read-only."""
    z = mc_oracle.normals(launch_words(seed, begin, nb))
    z.setflags(write=False)
    return z


def expected(z, compounding: str) -> np.ndarray:
    """The binary32 terminal value of the read-back set-up for the normals z (the module's docstring)."""
    r = np.asarray(z, np.float32) * np.float32(0.125) + np.float32(0.0)
    return r if compounding == "log" else np.float32(1.0) + r

"""Generator of tests/golden/icdf_extremes.json: Philox words at the ends of the spec's normal transform (SPEC.md section 3).

Random seeds never reach them, so they are searched once.  Scanned is step 0 at N = 16: the blocks q = 0..3 on the counter
(q, 0, p_lo, p_hi), sixteen words per path id.  With v = x & 0x7fffffff the octave of a word is E = 1 for v = 0, otherwise
floor(log2(v + 1/2)) + 2 = bit_length(v) + 1 (E = 1..32; table entries 32 (E - 1) .. 32 E - 1), and octave 33 (entry 1024, Z = +-0)
is reached only by v >= 0x7fffffc0, where fl32(v) = 2^31 and u rounds to exactly 1/2.

TWO SCANS, both in the order seed, path, block, word; a tie goes to the word met first.

  full      seed SEEDS[0], paths [PATH_FIRST, 2^BASE_LOG2): every class below is collected from every word.
  targeted  the following paths in rounds of 2^ROUND_LOG2, then the next seeds from PATH_FIRST on, until v = 1, v = 2, v = 3, v = 0
            and every octave have been met (one v = 1 is expected per 2^31 words): of these words only those with v < TARGET_BELOW
            are looked at, and every one of them is taken (classes deep, v_zero and octave_E).  The ends are checked when a round
            is complete, so the result does not depend on how the work is divided.

An entry is {seed, path, block, word, x, what}; `what` joins the classes the word belongs to with '+':

    v_zero      v = 0: table entry 0, the largest |z| (every one met)
    octave_E    E = 1..32: the smallest and the largest v met in that octave
    deep        every word met with v < 64 (full scan) or v < TARGET_BELOW (targeted scan)
    rounds_up   fl32(v) is a power of two 2^k above v (k = 25..31): per k the largest v met, and for k = 31 (v >= 0x7fffffc0,
                octave 33) the largest v met of either sign of bit 31
    bin_edge    for the table entries BIN_ENTRIES the words whose 18-bit delta (b & 0x3ffff of SPEC.md section 3) is the smallest
                and the largest met in that bin

Paths below PATH_FIRST = 63 and from 2^32 - 64 on are left out: the GPU test launches the 128 paths [path - 63, path + 65), which
must exist and share their high counter word.  The file holds at most MAX_ENTRIES entries; the generator fails if the scans give
more.  Only this project's own Philox (oracle/np_oracle.py) is involved.  Run from the repository root (a few minutes on 8 cores):

    python tests/golden/make_icdf_extremes.py
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import native_ref  # noqa: E402

SEEDS = (7, 8, 9, 10, 11, 12)
BASE_LOG2 = 25                  # full scan: 2^25 paths, 2^29 words
ROUND_LOG2 = 25                 # targeted scan: checked for completeness every 2^25 paths
CHUNK = 1 << 20
PATH_FIRST = 63
PATH_END = (1 << 32) - 64
NB = 4                          # N = 16
DEEP_BELOW = 64
TARGET_BELOW = 4
MAX_ENTRIES = 96
BIN_ENTRIES = (32 * 13 + 9, 32 * 19 + 0, 32 * 25 + 31, 32 * 31 + 17)      # octaves 14, 20, 26 and 32: an inner, a first, a last, an inner bin


def octave(v: int) -> int:
    return 1 if v == 0 else int(v).bit_length() + 1


def words_of(seed, lo, hi):
    """x uint32 [4 blocks, 4 words, hi - lo] of step 0 at N = 16."""
    paths = np.arange(lo, hi, dtype=np.uint64)
    return np.stack([np.stack(native_ref.block_words(seed, paths, 0, NB, q)) for q in range(NB)])


def scan_chunk(job):
    """One chunk of paths -> (deep, best): deep the list of candidates with a small v; best {slot: (key, candidate)}, the smallest key
    per slot.  A candidate is (seed, path, block, word, x); a key ends in (seed index, path, block, word), the scan order."""
    si, lo, hi, full = job
    seed = SEEDS[si]
    x = words_of(seed, lo, hi)
    v = x & np.uint32(0x7FFFFFFF)
    flat_v = v.ravel()
    best = {}

    def cand(f):
        q, m, j = np.unravel_index(int(f), x.shape)
        return (seed, lo + int(j), int(q), int(m), int(x[q, m, j]))

    def offer(slot, primary, flats):
        """The first word in scan order among the flat indices `flats`, all of one primary key."""
        c = min((cand(f) for f in flats), key=lambda c: c[1:4])
        key = (primary, si) + c[1:4]
        if slot not in best or key < best[slot][0]:
            best[slot] = (key, c)

    deep = sorted((cand(f) for f in np.flatnonzero(flat_v < (DEEP_BELOW if full else TARGET_BELOW))), key=lambda c: c[1:4])
    for c in deep:                                              # the low octaves' ends come from these words in either scan
        vv = c[4] & 0x7FFFFFFF
        for slot, primary in ((("octave_min", octave(vv)), vv), (("octave_max", octave(vv)), -vv)):
            key = (primary, si) + c[1:4]
            if slot not in best or key < best[slot][0]:
                best[slot] = (key, c)
    if not full:
        return deep, best
    vs = np.sort(flat_v)
    for E in range(octave(DEEP_BELOW), 33):                     # v in [2^(E-2), 2^(E-1))
        i0, i1 = np.searchsorted(vs, [1 << (E - 2), 1 << (E - 1)])
        if i1 > i0:
            offer(("octave_min", E), int(vs[i0]), np.flatnonzero(flat_v == vs[i0]))
            offer(("octave_max", E), -int(vs[i1 - 1]), np.flatnonzero(flat_v == vs[i1 - 1]))
    f32 = flat_v.astype(np.float32)                             # RNE to 24 bits
    fb = f32.view(np.uint32)
    up = np.flatnonzero(((fb & np.uint32(0x7FFFFF)) == 0) & (f32.astype(np.float64) > flat_v) & (flat_v >= (1 << 24)))
    k_up = (fb[up] >> np.uint32(23)).astype(np.int64) - 127
    for k in np.unique(k_up):
        sel = up[k_up == k]
        top = int(flat_v[sel].max())
        offer(("rounds_up", int(k)), -top, sel[flat_v[sel] == top])
        if k == 31:
            sign = (x.ravel()[sel] >> np.uint32(31)).astype(np.int64)
            for s in (0, 1):
                if np.any(sign == s):
                    top = int(flat_v[sel[sign == s]].max())
                    offer(("rounds_up_sign", s), -top, sel[(sign == s) & (flat_v[sel] == top)])
    # b of SPEC.md section 3: u = (fl32(v) 2^-32 + 2^-33) is exact in binary64, so the cast is the fma's single rounding
    u = (f32.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)
    b = u.view(np.uint32) - np.uint32(94 << 23)
    for e in BIN_ENTRIES:
        sel = np.flatnonzero((b >> np.uint32(18)) == e)
        if sel.size:
            d = (b[sel] & np.uint32(0x3FFFF)).astype(np.int64)
            offer(("bin_first", e), int(d.min()), sel[d == d.min()])
            offer(("bin_last", e), -int(d.max()), sel[d == d.max()])
    return deep, best


def main():
    deep, best, scanned = [], {}, []

    def run(pool, si, lo, hi, full):
        jobs = [(si, a, min(a + CHUNK, hi), full) for a in range(lo, hi, CHUNK)]
        for d, b in pool.imap(scan_chunk, jobs):                # in order: a tie goes to the earlier chunk
            deep.extend(d)
            for slot, kc in b.items():
                if slot not in best or kc[0] < best[slot][0]:
                    best[slot] = kc
        scanned.append({"seed": SEEDS[si], "path_first": lo, "path_end": hi, "words": 4 * NB * (hi - lo),
                        "scan": "full" if full else f"v < {TARGET_BELOW}"})
        print(f"seed {SEEDS[si]}, paths [{lo}, {hi}), {'full' if full else 'targeted'}: {len(deep)} small words so far", flush=True)

    def complete():
        met = {c[4] & 0x7FFFFFFF for c in deep}
        return {0, 1, 2, 3} <= met and all(("octave_min", E) in best for E in range(1, 33))

    with multiprocessing.Pool(min(os.cpu_count() or 1, 16)) as pool:
        run(pool, 0, PATH_FIRST, 1 << BASE_LOG2, True)
        si, lo = 0, 1 << BASE_LOG2
        while not complete():
            if lo >= PATH_END:
                si, lo = si + 1, PATH_FIRST
            hi = min((lo | ((1 << ROUND_LOG2) - 1)) + 1, PATH_END)
            run(pool, si, lo, hi, False)
            lo = hi

    classes = {}                                                # candidate -> its classes, in the order they are named above

    def tag(c, what):
        classes.setdefault(c, [])
        if what not in classes[c]:
            classes[c].append(what)

    for c in deep:
        if c[4] & 0x7FFFFFFF == 0:
            tag(c, "v_zero")
    for (kind, arg), (_, c) in sorted(best.items()):
        if kind in ("octave_min", "octave_max"):
            tag(c, f"octave_{arg}")
    for c in deep:
        tag(c, "deep")
    for (kind, arg), (_, c) in sorted(best.items()):
        if kind in ("rounds_up", "rounds_up_sign"):
            tag(c, "rounds_up")
    for (kind, arg), (_, c) in sorted(best.items()):
        if kind in ("bin_first", "bin_last"):
            tag(c, "bin_edge")
    order = sorted(classes, key=lambda c: (SEEDS.index(c[0]),) + c[1:4])
    entries = [{"seed": c[0], "path": c[1], "block": c[2], "word": c[3], "x": c[4], "what": "+".join(classes[c])} for c in order]
    if len(entries) > MAX_ENTRIES:
        raise SystemExit(f"{len(entries)} entries, more than {MAX_ENTRIES}")
    with open(os.path.join(HERE, "icdf_extremes.json"), "w") as f:
        json.dump({"n_assets": 4 * NB, "step": 0, "bin_entries": list(BIN_ENTRIES), "scanned": scanned,
                   "words_scanned": sum(s["words"] for s in scanned), "entries": entries}, f, indent=1)
        f.write("\n")
    print(len(entries), "entries;", sum(s["words"] for s in scanned), "words scanned")


if __name__ == "__main__":
    main()

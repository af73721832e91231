"""Generator of tests/golden/native_extremes.json: Philox words at the ends of the native Box-Muller transform (tests/native_ref.py).

Random seeds never reach them, so they are searched once: the first 2^26 path ids of one seed at N = 4 (one block per step), step 0.
Words 0 and 2 of a block are radius words (xa), words 1 and 3 angle words (xb).  Found and written, each as
{seed, path, block, word, x, what}:

    u_one        xa so large that u = fma(fl32(xa), 2^-32, 2^-32) rounds to 1.0: the radius is 0 (every one found)
    xa_min       the smallest xa: the largest radius
    turns_one    xb so large that turns = fl32(xb) 2^-32 rounds to 1.0 (every one found)
    xb_min       the smallest xb
    quarter, half, three_quarters    the xb nearest to 1/4, 1/2 and 3/4 of a turn: the zeros of cos, sin and cos

Only this project's own Philox (oracle/np_oracle.py) is involved.  Run from the repository root:  python tests/golden/make_native_extremes.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import native_ref  # noqa: E402

SEED = 7
LOG2_PATHS = 26
CHUNK = 1 << 20
ROUNDS_UP = 0xFFFFFF80          # fl32(x) = 2^32 from here on (the tie at 0xFFFFFF80 goes to the even 2^32)


def main():
    ones = {"u_one": [], "turns_one": []}
    best = {}                    # what -> (distance, path, word, x)

    def nearest(what, words, x, target, base):
        d = np.abs(x.astype(np.int64) - target)
        w, j = np.unravel_index(np.argmin(d), d.shape)
        if what not in best or d[w, j] < best[what][0]:
            best[what] = (int(d[w, j]), base + int(j), words[w], int(x[w, j]))

    for base in range(0, 1 << LOG2_PATHS, CHUNK):
        x = np.stack(native_ref.block_words(SEED, np.arange(base, base + CHUNK, dtype=np.uint64), 0, 1, 0))
        for what, words in (("u_one", (0, 2)), ("turns_one", (1, 3))):
            for w in words:
                for j in np.flatnonzero(x[w] >= ROUNDS_UP):
                    ones[what].append((base + int(j), w, int(x[w, j])))
        nearest("xa_min", (0, 2), x[[0, 2]], 0, base)
        nearest("xb_min", (1, 3), x[[1, 3]], 0, base)
        for what, target in (("quarter", 1 << 30), ("half", 1 << 31), ("three_quarters", 3 << 30)):
            nearest(what, (1, 3), x[[1, 3]], target, base)
    entries = [{"seed": SEED, "path": p, "block": 0, "word": w, "x": x, "what": what} for what in ("u_one", "turns_one")
               for p, w, x in ones[what]]
    entries += [{"seed": SEED, "path": p, "block": 0, "word": w, "x": x, "what": what} for what, (_, p, w, x) in best.items()]
    with open(os.path.join(HERE, "native_extremes.json"), "w") as f:
        json.dump({"n_assets": 4, "step": 0, "log2_paths_scanned": LOG2_PATHS, "entries": entries}, f, indent=1)
        f.write("\n")
    print(len(entries), "entries")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/ref_overlay.json by RUNNING THE REFERENCE's calc_options_series on fixed price series.

The reference is loaded as make_goldens.py loads it (the function definitions compiled from the file's own AST; this script
holds none of its source).  Only numbers are written: the price series, the strategies' rows (the row type as its index in
options.ROW_TYPES) and the reference's return series.  Every input is a binary32 value, so the binary32 restatement of SPEC.md
4.8 sees exactly what the reference saw.  On a machine without the reference the script exits 0 without touching the fixture.

Usage: python tests/golden/make_overlay_goldens.py
"""
import json
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_goldens  # noqa: E402
from monte_carlo_portfolio_amd import options  # noqa: E402

OUT = os.path.join(HERE, "ref_overlay.json")
S0 = 100.0


def f32(v):
    return float(np.float32(v))


def price_series():
    """A seeded geometric walk of 40 steps from 100 with 3 % steps (it crosses the strikes at 90, 100 and 110 % of the start
    within a few steps of each other: the drift alternates), and the same walk with a price of exactly 0 in the middle."""
    rng = np.random.default_rng(20240817)
    steps = rng.normal(0.0, 0.03, 40) + np.where(np.arange(40) % 16 < 8, -0.012, 0.014)
    walk = np.r_[S0, S0 * np.cumprod(1.0 + steps)]
    zero = walk.copy()
    zero[17] = 0.0
    return {"walk": [f32(v) for v in walk], "zero": [f32(v) for v in zero]}


def strategies():
    out = {}
    for name in options.STRATEGIES:
        out[name] = options.strategy_rows(name, S0, qty_asset=1.0, qty_contract=1.0, premium_put=1.5, premium_call=1.25,
                                          premium_put_low=0.375)
    out["three-row collar"] = [(options.BUY_ASSET, 0, 0, 2.0), (options.LONG_PUT, 95.0, 1.75, 2.0), (options.SHORT_CALL, 108.0, 1.125, 1.5)]
    return {k: [(t, f32(s), f32(p), f32(q)) for t, s, p, q in rows] for k, rows in out.items()}


def main():
    if not os.path.exists(make_goldens.APP):
        print("reference not present: fixture left as it is")
        return 0
    ns, _ = make_goldens.load_functions()
    series = price_series()
    cases = []
    for sname, prices in series.items():
        for name, rows in strategies().items():
            ret = ns["calc_options_series"](rows, pd.Series(prices))
            cases.append({"series": sname, "strategy": name,
                          "rows": [[options.ROW_TYPES.index(t), s, p, q] for t, s, p, q in rows],
                          "returns": [float(v) for v in ret.to_numpy()]})
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump({"series": series, "cases": cases}, f, indent=1)
    print(f"wrote {OUT}: {len(cases)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())

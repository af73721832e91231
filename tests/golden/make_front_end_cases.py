#!/usr/bin/env python3
"""Write tests/golden/front_end_cases.json: what the Python front end of the PARENT commit does with its keywords.

The collector is tests/front_end_cases.py of this tree; the package it records is the one under PARENT, a checkout of the
commit to compare with that holds a built libmcport.so, for instance

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/monte_carlo_portfolio_amd/csrc -j8
    python tests/golden/make_front_end_cases.py /tmp/parent

No GPU is needed: the mcp_simulate* functions of the library are replaced by a recorder.  The fixture holds three blocks: "call"
(Context._call), "public" (simulate_paths, simulate_bootstrap, simulate_filtered, simulate_sweep) and "argtypes" (the argument
types of every row of _ffi.SIGNATURES, by name).

Usage: python tests/golden/make_front_end_cases.py PARENT
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(parent):
    sys.path[:0] = [os.path.abspath(parent), os.path.dirname(HERE)]
    import front_end_cases
    from monte_carlo_portfolio_amd import _ffi
    assert os.path.abspath(_ffi.__file__).startswith(os.path.abspath(parent) + os.sep), _ffi.__file__
    out = {"call": front_end_cases.call_cases(), "public": front_end_cases.public_cases(_ffi.lib()), "argtypes": front_end_cases.argtypes()}
    with open(os.path.join(HERE, "front_end_cases.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    for block in ("call", "public"):
        raised = sum("raises" in c for c in out[block].values())
        print(f"{block}: {len(out[block])} cases, {raised} raise")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

#!/usr/bin/env python3
"""Generate tests/golden/rowsum_parent.npz: the raw records of mcp_launch_downside and mcp_launch_relative, word for word, as the
library built from the commit BEFORE the row-sum kernels were folded onto one row walker, one workgroup record and one merge wrote
them on an MI355X.  tests/test_gpu_rowsum_bytes.py holds every later build to these bytes: the order of the sums is the definition
of the result.

Inputs, sizes and launches are tests/rowsum_cases.py's (rows from integer arithmetic, simple compounding, stride = n + 3 behind a
one-element offset); this script adds nothing of its own.  The file holds, per size n, `downside_n<n>` [3, 12] and `relative_n<n>`
[6, 18] as uint64 words, and `relative_y_n<n>` [6, n] as the uint32 bits of Y for n <= 1025.

It needs a GPU and must run against a build of that parent commit: point MCP_LIB_PATH at its libmcport.so.  Run against any later
build it would only record what that build computes, which proves nothing; regenerate only when SPEC.md 5.22 / 5.23 themselves change.

Usage: MCP_LIB_PATH=<parent build>/libmcport.so python tests/golden/make_rowsum_parent_goldens.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(argv):
    import rowsum_cases
    from monte_carlo_portfolio_amd import _ffi
    out = argv[0] if argv else os.path.join(HERE, "rowsum_parent.npz")
    arrays = rowsum_cases.record_all(_ffi.lib())
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {len(arrays)} arrays, {os.path.getsize(out)} bytes, library {_ffi.LIB_PATH}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

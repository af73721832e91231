"""csrc/mcp_host.cpp -- every argument rule, host constant, pivot, packer and the tile layout -- needs no device header, so
`make host-selftest` builds it with the plain C++ compiler that ships beside hipcc, under AddressSanitizer + UBSan, together with
csrc/host_selftest.cpp, and runs that program: every pure entry point and, per feature, check_request, tile_layout + pack_tile
and request_pivots on heap buffers of exactly the documented lengths, then the routing of every combination of features:
check_request, route_kernel and the rows of csrc/mcp_paths_ladder.inc, the text the device build includes.  The build itself proves the unit is free of the device
runtime; an overrun is a sanitizer report and a non-zero exit.  No GPU, nothing loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")


def test_host_unit_selftest_under_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "host-selftest", f"BUILD={tmp_path}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "host_selftest ok" in r.stdout

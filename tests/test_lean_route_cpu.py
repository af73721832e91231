"""mcp::lean_range (csrc/mcp_route.h), the host predicate that routes a plain Gaussian launch to mc_paths_lean_kernel: true
exactly when every path id of [path_begin, path_begin + n_paths) has the same high 32 bits.  The header needs nothing but
<stdint.h>, so the function is compiled alone into a small host program: no GPU, no HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO32 = 1 << 32

CASES = [
    (0, 1, True), (0, 257, True), (0, TWO32, True), (0, TWO32 + 1, False),
    (TWO32 - 64, 64, True), (TWO32 - 64, 65, False), (TWO32 - 1, 1, True), (TWO32 - 1, 2, False),
    (TWO32, 1, True), (TWO32, 257, True), (TWO32, TWO32, True), (TWO32, TWO32 + 1, False),
    (5 * TWO32 + 7, 257, True), (5 * TWO32 + 7, TWO32 - 7, True), (5 * TWO32 + 7, TWO32 - 6, False),
    (0, 0, False), (TWO32, 0, False),                                  # an empty launch has no p_hi
    ((1 << 64) - 1, 1, True), ((1 << 64) - 1, 2, False), ((1 << 64) - 64, 65, False),   # a range that wraps past 2^64
]


def test_lean_range_at_the_boundaries(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    rows = "\n".join(f"  {{{b}ull, {n}ull, {int(want)}}}," for b, n, want in CASES)
    src = tmp_path / "route.cpp"
    src.write_text('#include <stdio.h>\n#include "mcp_route.h"\n'
                   "static const struct { uint64_t begin, n; int want; } cases[] = {\n" + rows + "\n};\n"
                   "int main() {\n  int bad = 0;\n  for (const auto& c : cases)\n"
                   "    if ((int)mcp::lean_range(c.begin, c.n) != c.want) {\n"
                   '      printf("lean_range(%llu, %llu) != %d\\n", (unsigned long long)c.begin, (unsigned long long)c.n, c.want);\n'
                   "      bad = 1;\n    }\n  return bad;\n}\n")
    exe = tmp_path / "route"
    inc = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{inc}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout

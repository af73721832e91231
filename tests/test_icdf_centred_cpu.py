"""normal_icdf_centred (mcp_device.h: the lean kernel's ten-instruction normal transform on a binade-scaled table) against the
transform of SPEC.md section 3, on the host, in exact binary32 arithmetic (fmaf), exhaustively: every one of the 1,056 table
entries times every one of the 2^18 low-mantissa patterns of u -- a superset of the u a 31-bit word can produce -- 2.8e8
evaluations of both, a few seconds of C.  Per pattern: the same bits of a, the same table entry, byte offset 16 i + 8.  Per entry:
every scaled coefficient is zero or a normal number and equals ldexpf(c, -k E) (scaling back returns c).  Then whole words: the ends
v = 0 and v = 2^31 - 1 with both signs, and a strided sweep of words, where y = fma(fl32(v), 4, 2) must be u 2^34 exactly.

The C++ below restates both transforms from SPEC.md section 3 and DESIGN.md section 4.1; the device code is held to the oracle
bit for bit by tests/test_gpu_icdf_centred.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monte_carlo_portfolio_amd", "csrc")

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static const float T[1056][4] = {
#include "mcp_icdf_table.inc"
};
static float S[1056][4];    // entry i scaled by its binade E = 1 + i / 32: {c0, c1 2^-E, c2 2^-2E, c3 2^-3E}

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float asfloat(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

// SPEC.md section 3 from u: the table entry through *e, the result a
static float spec_a(float u, uint32_t* e) {
  const uint32_t b = bits(u) - (94u << 23);
  *e = b >> 18;
  const float dc = asfloat((b & 0x3ffffu) | 0x3f800000u) - 0x1.04p+0f;
  const float* c = T[*e];
  return fmaf(fmaf(fmaf(c[3], dc, c[2]), dc, c[1]), dc, c[0]);
}
// normal_icdf_centred from y = u 2^34: the table's byte offset through *off, the result a
static float centred_a(float y, uint32_t* off) {
  const uint32_t m18 = 0x0003ffffu, ctr = 0x00020000u;
  const uint32_t yc = (m18 & ctr) | (~m18 & bits(y));
  *off = (yc >> 14) & 0xffffu;
  const float d = y - asfloat(yc);
  const float* c = S[(*off - 8u) / 16u];
  return fmaf(fmaf(fmaf(c[3], d, c[2]), d, c[1]), d, c[0]);
}
static uint32_t z_spec(uint32_t x) {
  uint32_t e;
  const float a = spec_a(fmaf((float)(x & 0x7fffffffu), 0x1p-32f, 0x1p-33f), &e);
  return (bits(a) & 0x7fffffffu) | (x & 0x80000000u);
}
static uint32_t z_centred(uint32_t x) {
  uint32_t off;
  const float a = centred_a(fmaf((float)(x & 0x7fffffffu), 0x1p+2f, 0x1p+1f), &off);
  return (bits(a) & 0x7fffffffu) | (x & 0x80000000u);
}

int main() {
  // the scaled table: exact, no subnormal, no overflow
  for (int i = 0; i < 1056; i++) {
    const int E = 1 + i / 32;
    for (int k = 0; k < 4; k++) {
      const float c = T[i][k], s = ldexpf(c, -k * E);
      if (!((s == 0.0f && c == 0.0f) || std::isnormal(s))) { printf("entry %d c%d: scaled %a is neither zero nor normal\n", i, k, s); return 1; }
      if (bits(ldexpf(s, k * E)) != bits(c)) { printf("entry %d c%d: %a does not scale back to %a\n", i, k, s, c); return 1; }
      S[i][k] = s;
    }
  }
  // every entry x every low-mantissa pattern
  unsigned long long n = 0;
  for (uint32_t i = 0; i < 1056; i++) {
    for (uint32_t l = 0; l < (1u << 18); l++) {
      const float u = asfloat(((94u << 23) + (i << 18)) | l);
      uint32_t e, off;
      const float a0 = spec_a(u, &e), a1 = centred_a(ldexpf(u, 34), &off);
      if (e != i || off != 16u * i + 8u || (off - 8u) / 16u != e || bits(a0) != bits(a1)) {
        printf("entry %u low bits %#x: spec entry %u a %a, centred offset %u a %a\n", i, l, e, a0, off, a1);
        return 1;
      }
      n++;
    }
  }
  // whole words: the ends with both signs, then a strided sweep (stride odd, so every residue of the low bits turns up)
  const uint32_t ends[4] = {0u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  for (int j = 0; j < 4; j++)
    if (z_spec(ends[j]) != z_centred(ends[j])) { printf("word %#x: %#x / %#x\n", ends[j], z_spec(ends[j]), z_centred(ends[j])); return 1; }
  if (fabsf(asfloat(z_spec(0u)) - 6.337958f) > 1e-6f) { printf("Z(0) = %a\n", asfloat(z_spec(0u))); return 1; }
  if (z_spec(0x7fffffffu) != 0u || z_spec(0xffffffffu) != 0x80000000u) { printf("Z(2^31 - 1) is not +-0\n"); return 1; }
  unsigned long long w = 0;
  for (uint64_t x = 0; x < (1ull << 32); x += 4099u, w++) {
    const float f = (float)((uint32_t)x & 0x7fffffffu);
    if (bits(fmaf(f, 0x1p+2f, 0x1p+1f)) != bits(ldexpf(fmaf(f, 0x1p-32f, 0x1p-33f), 34))) { printf("word %#llx: y is not u 2^34\n", (unsigned long long)x); return 1; }
    if (z_spec((uint32_t)x) != z_centred((uint32_t)x)) { printf("word %#llx: %#x / %#x\n", (unsigned long long)x, z_spec((uint32_t)x), z_centred((uint32_t)x)); return 1; }
  }
  printf("ok %llu patterns %llu words\n", n, w);
  return 0;
}
"""


def test_centred_transform_is_the_spec_transform_for_every_entry_and_delta(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # the Makefile's compiler, host code only
    src, exe = tmp_path / "icdf_centred.cpp", tmp_path / "icdf_centred"
    src.write_text(PROGRAM)
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == f"ok {1056 * (1 << 18)} patterns {((1 << 32) + 4098) // 4099} words", out.stdout

// mcp_route.h -- what names a path kernel, and the host-side routing predicates that depend on nothing but integers (no HIP
// header: the tests compile this file alone, and mcp_host.cpp and host_selftest.cpp build with a plain C++ compiler).
#pragma once
#include <stdint.h>

namespace mcp {

// Do the paths [path_begin, path_begin + n_paths) share the high 32 bits of their ids?  Then the Philox counter word p_hi is one
// value for the whole launch and the plain Gaussian walk may run on mc_paths_lean_kernel (mcp_paths.h, UHI).  An empty range and
// a range that crosses a multiple of 2^32 (or wraps past 2^64) do not.
inline bool lean_range(uint64_t path_begin, uint64_t n_paths) {
  if (n_paths == 0) return false;
  const uint64_t last = path_begin + (n_paths - 1);
  return last >= path_begin && (path_begin >> 32) == (last >> 32);
}

constexpr int ICDF_ENTRIES = 1056;   // 33 octaves x 32 mantissa bins of float4 {c0,c1,c2,c3}: 16.5 KiB of LDS per workgroup
// The LDS copy of the table carries ICDF_PAD unused entries in front: u is formed with its exponent pre-scaled by 2^-93
// (binary32 exponent field 1..33 instead of 94..126; same significand, so the same table entry and the same delta), and
// then bits(u) >> 18 indexes the padded table directly -- the spec's subtraction of (94 << 23) costs no instruction.
constexpr int ICDF_PAD = 32;
constexpr int ICDF_LDS_ENTRIES = ICDF_ENTRIES + ICDF_PAD;

// The LDS copy of the row table takes the slot of the inverse-CDF table (ICDF_LDS_ENTRIES float4: the bootstrap needs neither
// that table nor the drift copy in its padding): R rows of NB float4 fit when R * NB <= ICDF_LDS_ENTRIES (N = 16: 272 rows).
constexpr bool boot_fits_lds(uint64_t n_rows, int nb) { return n_rows * (uint64_t)nb <= (uint64_t)ICDF_LDS_ENTRIES; }
// The filtered rows carry their shock table behind them in the same slot, ceil(R/4) float4 more (N = 16: 256 rows).
constexpr bool filt_fits_lds(uint64_t n_rows, int nb) {
  return n_rows * (uint64_t)nb + (n_rows + 3) / 4 <= (uint64_t)ICDF_LDS_ENTRIES;
}

// Which path kernel a launch runs: the family of the walk and one bit per property of the kernel.  A selector names a kernel, not
// a request: mcph::route_kernel (mcp_host.cpp) builds it from a checked request and sets no bit that the kernel does not consume,
// and mcp_paths_ladder.inc lists every selector that has a kernel, matched by equality (selects below).
constexpr int LEAN_MAX_NB = 4;     // mc_paths_lean_kernel exists for N <= 16 only: from NB = 5 on the listings show it at more registers
                                   // than mc_paths_kernel, at NB = 12, 14 and 15 at one wave per SIMD fewer, and nothing above 4 was timed
enum PathFamily { FAM_PLAIN, FAM_DD, FAM_HZ, FAM_REB, FAM_CF, FAM_OV, FAM_AT };
enum PathFlag : uint32_t {
  PK_LOGC = 1u << 0,     // log compounding (the plain, drawdown, horizon, bootstrap and antithetic Gaussian kernels only)
  PK_BOOT = 1u << 1,     // the draws are rows of the bootstrap's table
  PK_BLDS = 1u << 2,     // with PK_BOOT: the row table is copied into LDS (boot_fits_lds; with PK_FH: filt_fits_lds)
  PK_STT = 1u << 3,      // the Student-t kernels
  PK_DD = 1u << 4,       // FAM_OV only: the overlay kernel that also tracks the drawdown
  PK_GV = 1u << 5,       // the GARCH walk on Student-t draws.  It also serves Student-t and Gaussian requests of a family with one
                         // walk (nu = 0; alpha = beta = 0, h0 = 1): the attribution, the protection and the antithetic GARCH kernels
  PK_KT8 = 1u << 6,      // passes of 8 portfolios instead of 1 (the ladder's KT; no row names it)
  PK_NATIVE = 1u << 7,   // the plain Gaussian kernel on native math
  PK_FOLD = 1u << 8,     // the plain Gaussian kernel on the folded step
  PK_ANTI = 1u << 9,     // the antithetic kernels of the plain, drawdown and horizon families: Gaussian draws, or PK_GV
  PK_FH = 1u << 10,      // with PK_BOOT, FAM_HZ (H = 0: one segment): filtered residual rows, SPEC.md 4.11
  PK_UHI = 1u << 11,     // the plain Gaussian walk of one portfolio whose launch passes lean_range: mc_paths_lean_kernel
  PK_JP = 1u << 12,      // the jump-diffusion kernels of the plain, drawdown and horizon families (SPEC.md 2.5), or the jump walk of PK_PI
  PK_RS = 1u << 13,      // the regime-switching kernels of the same three families (SPEC.md 2.6)
  PK_GP = 1u << 14,      // FAM_CF only: the glide-path kernel, the cash-flow walk on scheduled target weights (SPEC.md 4.14)
  PK_PI = 1u << 15,      // the floor-protection kernel (SPEC.md 4.15): FAM_DD with the drawdown, else FAM_HZ (H = 0 included); PK_GV or PK_JP
  PK_SP = 1u << 16,      // FAM_CF only: the spending kernel, the cash-flow walk on the path's own withdrawal (SPEC.md 4.16)
  PK_LT = 1u << 17,      // with exactly one of PK_GP and PK_SP: that kernel's lifetime twin (SPEC.md 4.17)
  PK_TB = 1u << 18,      // FAM_REB only, never PK_KT8: the tolerance-band kernel (SPEC.md 4.18), K portfolios as K passes of one
  PK_VT = 1u << 19,      // the volatility-targeting kernel (SPEC.md 4.19): FAM_DD with the drawdown, else FAM_HZ (H = 0 included); PK_GV or PK_JP
  PK_UW = 1u << 20,      // FAM_DD only: the drawdown kernel's twin that also counts the time under water (SPEC.md 4.20); alone, or with one
                         // of PK_LOGC, PK_GV and PK_JP
  PK_PU = 1u << 21       // the Gaussian walk on a drift drawn once per path (SPEC.md 2.7 / 4.21): FAM_PLAIN, FAM_DD and FAM_HZ alone or with
                         // PK_LOGC, FAM_CF alone; never PK_UHI
};
constexpr int N_PATH_FLAGS = 21;                      // the bits PK_LOGC .. PK_UW
constexpr int N_PATH_FLAGS_PU = N_PATH_FLAGS + 1;     // ... and PK_PU behind them: the 22 bits a selector may carry
struct PathKernel {
  int family;            // PathFamily
  uint32_t flags;        // PathFlag bits
};
// Does `k` select the row (family, mask) of mcp_paths_ladder.inc?  Everything but the pass width must be equal.
constexpr bool selects(const PathKernel& k, int family, uint32_t mask) { return k.family == family && (k.flags & ~(uint32_t)PK_KT8) == mask; }

}  // namespace mcp

// mcp_route.h -- host-side routing predicates of the path kernels that depend on nothing but integers (no HIP header: the
// tests compile this file alone).
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

}  // namespace mcp

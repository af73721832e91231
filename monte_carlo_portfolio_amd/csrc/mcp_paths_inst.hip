// mcp_paths_inst.hip -- the path kernels of mcp_paths.h for ONE value of NB (= ceil(N/4), -DMCP_NB=n) and their one entry point,
// launch_paths_nb<n>: the table of mcp_paths_ladder.inc is the only place that maps a selector (PathKernel) to a kernel, and what it
// names is what this unit instantiates.  Built once per NB in 1..16 so the 16 translation units compile in parallel (see Makefile).
#include <cstdlib>

#include "mcp_paths.h"
#include "mcp_stats_kernels.h"

#ifndef MCP_NB
#error "compile with -DMCP_NB=<1..16>"
#endif

#define MCP_CAT_(a, b) a##b
#define MCP_CAT(a, b) MCP_CAT_(a, b)

namespace mcp {

// MCP_PATHS_LDS_PAD (bytes, env, experiment): extra dynamic LDS per workgroup.  4608 on top of the 16 KiB of tables
// makes 7 instead of 8 workgroups fit a CU, which leaves one wave slot per SIMD free for the small statistics
// kernels of the previous batch when batches are pipelined (engine.PathEngine).
static size_t lds_pad() {
  static const size_t pad = [] { const char* e = getenv("MCP_PATHS_LDS_PAD"); return e ? (size_t)atol(e) : (size_t)0; }();
  return pad;
}

// Every pass of KT portfolios (k_begin = 0, KT, ...) of one kernel.  A, the kernel's own argument struct, is deduced from the
// kernel and built by value from the blocks of `s` that it has, so the arguments cannot be another kernel's.
template <int KT, class A>
static hipError_t run(void (*kernel)(A), const PathLaunchArgs& s, hipStream_t stream) {
  A x = make_args<A>(s);
  const int grid = path_grid(x.n_paths);
  for (x.k_begin = 0; x.k_begin < x.n_portfolios; x.k_begin += KT) {
    kernel<<<grid, PATH_BLOCK, lds_pad(), stream>>>(x);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// Every row of mcp_paths_ladder.inc that exists at this NB and KT: the kernel of the row that `k` equals, in passes of KT portfolios.
template <int KT>
static hipError_t ladder(const PathKernel& k, const PathLaunchArgs& s, hipStream_t stream) {
  constexpr int NB = MCP_NB;
#define MCP_ROW_IF(cond, family, mask, ...) \
  if constexpr (cond) { if (selects(k, family, mask)) return run<KT>(__VA_ARGS__, s, stream); }
#include "mcp_paths_ladder.inc"
#undef MCP_ROW_IF
  return hipErrorInvalidValue;
}

hipError_t MCP_CAT(launch_paths_nb, MCP_NB)(const PathKernel& k, const PathLaunchArgs& s, hipStream_t stream) {
  return (k.flags & PK_KT8) ? ladder<8>(k, s, stream) : ladder<1>(k, s, stream);
}

}  // namespace mcp

// mcp_paths_inst.hip -- instantiates mc_paths_kernel for ONE value of NB (= ceil(N/4), -DMCP_NB=n).
// Built once per NB in 1..16 so the 16 translation units compile in parallel (see Makefile).
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

#define MCP_GO(kernel, A) kernel<<<grid, PATH_BLOCK, lds_pad(), stream>>>(static_cast<const A&>(a))

// The plain Gaussian kernel with the native-math or folded step (one portfolio, or KT = 8 passes without FOLD).
template <int KT, bool NATIVE, bool FOLD>
static void go_plain(bool lg, const PathArgs& a, int grid, hipStream_t stream) {
  if (lg) MCP_GO((mc_paths_kernel<MCP_NB, KT, 1, NATIVE, FOLD, true>), PathArgs);
  else MCP_GO((mc_paths_kernel<MCP_NB, KT, 1, NATIVE, FOLD, false>), PathArgs);
}

// Every family on the spec's normals and the unfolded recurrence (or no normals: the bootstrap), KT = 1 or 8, compounding LG
// (the rebalancing, Student-t, GARCH, cash-flow and overlay kernels compound simply and take no LG).
template <int KT, bool LG>
static void go(const PathKernel& k, const PathArgs& a, int grid, hipStream_t stream) {
  switch (k.family) {
    case FAM_PLAIN:
      if (k.gv) MCP_GO((mc_paths_g_kernel<MCP_NB, KT, 1>), PathArgsG);
      else if (k.stt) MCP_GO((mc_paths_t_kernel<MCP_NB, KT, 1>), PathArgsT);
      else if (k.boot && k.blds) MCP_GO((mc_paths_boot_kernel<MCP_NB, KT, 1, LG, true>), PathArgsBT);
      else if (k.boot) MCP_GO((mc_paths_boot_kernel<MCP_NB, KT, 1, LG, false>), PathArgsBT);
      else MCP_GO((mc_paths_kernel<MCP_NB, KT, 1, false, false, LG>), PathArgs);
      break;
    case FAM_DD:
      if (k.gv) MCP_GO((mc_paths_g_dd_kernel<MCP_NB, KT, 1>), PathArgsGDD);
      else if (k.stt) MCP_GO((mc_paths_t_dd_kernel<MCP_NB, KT, 1>), PathArgsTDD);
      else MCP_GO((mc_paths_dd_kernel<MCP_NB, KT, 1, LG>), PathArgsDD);
      break;
    case FAM_HZ:
      if (k.gv) MCP_GO((mc_paths_g_hz_kernel<MCP_NB, KT, 1>), PathArgsGHZ);
      else if (k.stt) MCP_GO((mc_paths_t_hz_kernel<MCP_NB, KT, 1>), PathArgsTHZ);
      else if (k.boot && k.blds) MCP_GO((mc_paths_boot_hz_kernel<MCP_NB, KT, 1, LG, true>), PathArgsBTHZ);
      else if (k.boot) MCP_GO((mc_paths_boot_hz_kernel<MCP_NB, KT, 1, LG, false>), PathArgsBTHZ);
      else MCP_GO((mc_paths_hz_kernel<MCP_NB, KT, 1, LG>), PathArgsHZ);
      break;
    case FAM_REB:
      if (k.boot && k.blds) MCP_GO((mc_paths_reb_kernel<MCP_NB, KT, 1, true, true>), PathArgsRB);
      else if (k.boot) MCP_GO((mc_paths_reb_kernel<MCP_NB, KT, 1, true, false>), PathArgsRB);
      else MCP_GO((mc_paths_reb_kernel<MCP_NB, KT, 1, false, false>), PathArgsRB);
      break;
    case FAM_CF:
      if (k.stt) MCP_GO((mc_paths_cf_kernel<MCP_NB, KT, 1, false, false, true>), PathArgsCF);
      else if (k.boot && k.blds) MCP_GO((mc_paths_cf_kernel<MCP_NB, KT, 1, true, true, false>), PathArgsCF);
      else if (k.boot) MCP_GO((mc_paths_cf_kernel<MCP_NB, KT, 1, true, false, false>), PathArgsCF);
      else MCP_GO((mc_paths_cf_kernel<MCP_NB, KT, 1, false, false, false>), PathArgsCF);
      break;
    case FAM_OV:
      if (k.stt && k.dd) MCP_GO((mc_paths_ov_kernel<MCP_NB, KT, 1, true, true>), PathArgsOV);
      else if (k.stt) MCP_GO((mc_paths_ov_kernel<MCP_NB, KT, 1, true, false>), PathArgsOV);
      else if (k.dd) MCP_GO((mc_paths_ov_kernel<MCP_NB, KT, 1, false, true>), PathArgsOV);
      else MCP_GO((mc_paths_ov_kernel<MCP_NB, KT, 1, false, false>), PathArgsOV);
      break;
  }
}

hipError_t MCP_CAT(launch_paths_nb, MCP_NB)(int variant, const PathKernel& k, const PathArgs& a, int grid, hipStream_t stream) {
  if (k.family == FAM_AT) {                                // one portfolio per pass, simple compounding, the GARCH kernel's draws
    if (variant != 0 || k.logc || k.boot) return hipErrorInvalidValue;
    MCP_GO((mc_paths_attr_kernel<MCP_NB, 1, 1>), PathArgsAT);
    return hipGetLastError();
  }
  const bool plain = k.family == FAM_PLAIN && !k.boot && !k.stt && !k.gv;
  if (k.family < FAM_PLAIN || k.family > FAM_OV || (!plain && variant != 0 && variant != VAR_KT8)) return hipErrorInvalidValue;
  switch (variant) {
    case 0: k.logc ? go<1, true>(k, a, grid, stream) : go<1, false>(k, a, grid, stream); break;
    case VAR_KT8: k.logc ? go<8, true>(k, a, grid, stream) : go<8, false>(k, a, grid, stream); break;
    case VAR_NATIVE: go_plain<1, true, false>(k.logc, a, grid, stream); break;
    case VAR_FOLD: go_plain<1, false, true>(k.logc, a, grid, stream); break;
    case VAR_KT8 | VAR_NATIVE: go_plain<8, true, false>(k.logc, a, grid, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
#undef MCP_GO

}  // namespace mcp

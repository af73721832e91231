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

template <int KT, int PPT, bool NATIVE, bool FOLD = false>
static hipError_t go(const PathArgs& args, int grid, hipStream_t stream) {
  if (args.compounding == MCP_COMPOUND_LOG)
    mc_paths_kernel<MCP_NB, KT, PPT, NATIVE, FOLD, true><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
  else
    mc_paths_kernel<MCP_NB, KT, PPT, NATIVE, FOLD, false><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
  return hipGetLastError();
}

hipError_t MCP_CAT(launch_paths_nb, MCP_NB)(int variant, const PathArgs& args, int grid, hipStream_t stream) {
  switch (variant) {
    case 0: return go<1, 1, false>(args, grid, stream);
    case VAR_NATIVE: return go<1, 1, true>(args, grid, stream);
    case VAR_FOLD: return go<1, 1, false, true>(args, grid, stream);
    case VAR_KT8: return go<8, 1, false>(args, grid, stream);
    case VAR_KT8 | VAR_NATIVE: return go<8, 1, true>(args, grid, stream);
#if MCP_NB <= 4 && defined(MCP_EXP_PPT2)      // two paths per lane: measured 3 % slower (129 VGPRs), kept behind a build flag
    case VAR_PPT2: return go<1, 2, false>(args, grid, stream);
    case VAR_PPT2 | VAR_NATIVE: return go<1, 2, true>(args, grid, stream);
#endif
    default: return hipErrorInvalidValue;
  }
}

// The drawdown kernel (mcp_launch_paths_drawdown): one portfolio or KT = 8 passes, both compounding modes.
hipError_t MCP_CAT(launch_paths_dd_nb, MCP_NB)(int variant, const PathArgsDD& args, int grid, hipStream_t stream) {
  const bool lg = args.compounding == MCP_COMPOUND_LOG;
  switch (variant) {
    case 0:
      if (lg) mc_paths_dd_kernel<MCP_NB, 1, 1, true><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
      else mc_paths_dd_kernel<MCP_NB, 1, 1, false><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
      break;
    case VAR_KT8:
      if (lg) mc_paths_dd_kernel<MCP_NB, 8, 1, true><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
      else mc_paths_dd_kernel<MCP_NB, 8, 1, false><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// The horizon kernel (mcp_launch_paths_horizons): one portfolio or KT = 8 passes, both compounding modes.
hipError_t MCP_CAT(launch_paths_hz_nb, MCP_NB)(int variant, const PathArgsHZ& args, int grid, hipStream_t stream) {
  const bool lg = args.compounding == MCP_COMPOUND_LOG;
  switch (variant) {
    case 0:
      if (lg) mc_paths_hz_kernel<MCP_NB, 1, 1, true><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
      else mc_paths_hz_kernel<MCP_NB, 1, 1, false><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
      break;
    case VAR_KT8:
      if (lg) mc_paths_hz_kernel<MCP_NB, 8, 1, true><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
      else mc_paths_hz_kernel<MCP_NB, 8, 1, false><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// The bootstrap kernels (mcp_simulate_bootstrap[_horizons]): one portfolio or KT = 8 passes, both compounding modes, the row
// table in LDS or in global memory.
template <int KT, bool LG, bool LDS>
static void go_bt(const PathArgsBT& args, int grid, hipStream_t stream) {
  mc_paths_boot_kernel<MCP_NB, KT, 1, LG, LDS><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
}
template <int KT, bool LG, bool LDS>
static void go_bt(const PathArgsBTHZ& args, int grid, hipStream_t stream) {
  mc_paths_boot_hz_kernel<MCP_NB, KT, 1, LG, LDS><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
}
template <class A>
static hipError_t go_bt_any(int variant, bool lds, const A& args, int grid, hipStream_t stream) {
  const bool lg = args.compounding == MCP_COMPOUND_LOG;
  if (variant != 0 && variant != VAR_KT8) return hipErrorInvalidValue;
  const bool kt8 = variant == VAR_KT8;
  if (kt8) {
    if (lg) lds ? go_bt<8, true, true>(args, grid, stream) : go_bt<8, true, false>(args, grid, stream);
    else lds ? go_bt<8, false, true>(args, grid, stream) : go_bt<8, false, false>(args, grid, stream);
  } else {
    if (lg) lds ? go_bt<1, true, true>(args, grid, stream) : go_bt<1, true, false>(args, grid, stream);
    else lds ? go_bt<1, false, true>(args, grid, stream) : go_bt<1, false, false>(args, grid, stream);
  }
  return hipGetLastError();
}

hipError_t MCP_CAT(launch_paths_bt_nb, MCP_NB)(int variant, bool lds, const PathArgsBT& args, int grid, hipStream_t stream) {
  return go_bt_any(variant, lds, args, grid, stream);
}

hipError_t MCP_CAT(launch_paths_bthz_nb, MCP_NB)(int variant, bool lds, const PathArgsBTHZ& args, int grid, hipStream_t stream) {
  return go_bt_any(variant, lds, args, grid, stream);
}

// The rebalancing kernel (mcp_simulate_rebalanced, SPEC.md 4.5): one portfolio or KT = 8 passes, simple compounding, Gaussian
// draws or the bootstrap's row table in LDS or in global memory.
template <int KT>
static void go_rb(bool boot, bool lds, const PathArgsRB& args, int grid, hipStream_t stream) {
  if (!boot) mc_paths_reb_kernel<MCP_NB, KT, 1, false, false><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
  else if (lds) mc_paths_reb_kernel<MCP_NB, KT, 1, true, true><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
  else mc_paths_reb_kernel<MCP_NB, KT, 1, true, false><<<grid, PATH_BLOCK, lds_pad(), stream>>>(args);
}

hipError_t MCP_CAT(launch_paths_rb_nb, MCP_NB)(int variant, bool boot, bool lds, const PathArgsRB& args, int grid, hipStream_t stream) {
  if (variant != 0 && variant != VAR_KT8) return hipErrorInvalidValue;
  if (variant == VAR_KT8) go_rb<8>(boot, lds, args, grid, stream);
  else go_rb<1>(boot, lds, args, grid, stream);
  return hipGetLastError();
}

// The Student-t kernels (mcp_simulate_student_t, SPEC.md 2.2 / 4.6): one portfolio or KT = 8 passes, simple compounding; exactly
// one of the three argument blocks is given (terminal values only, with the drawdown, with horizons).
template <int KT>
static void go_t(const PathArgsT* at, const PathArgsTDD* ad, const PathArgsTHZ* ah, int grid, hipStream_t stream) {
  if (ad) mc_paths_t_dd_kernel<MCP_NB, KT, 1><<<grid, PATH_BLOCK, lds_pad(), stream>>>(*ad);
  else if (ah) mc_paths_t_hz_kernel<MCP_NB, KT, 1><<<grid, PATH_BLOCK, lds_pad(), stream>>>(*ah);
  else mc_paths_t_kernel<MCP_NB, KT, 1><<<grid, PATH_BLOCK, lds_pad(), stream>>>(*at);
}

hipError_t MCP_CAT(launch_paths_t_nb, MCP_NB)(int variant, const PathArgsT* at, const PathArgsTDD* ad, const PathArgsTHZ* ah, int grid,
                                              hipStream_t stream) {
  if (variant != 0 && variant != VAR_KT8) return hipErrorInvalidValue;
  if ((at != nullptr) + (ad != nullptr) + (ah != nullptr) != 1) return hipErrorInvalidValue;
  if (variant == VAR_KT8) go_t<8>(at, ad, ah, grid, stream);
  else go_t<1>(at, ad, ah, grid, stream);
  return hipGetLastError();
}

}  // namespace mcp

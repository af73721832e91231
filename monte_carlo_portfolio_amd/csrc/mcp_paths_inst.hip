// mcp_paths_inst.hip -- the path kernels of mcp_paths.h for ONE value of NB (= ceil(N/4), -DMCP_NB=n) and their one entry point,
// launch_paths_nb<n>: the ladder below is the only place that maps a selector (PathKernel) to a kernel, and what it names is
// what this unit instantiates.  Built once per NB in 1..16 so the 16 translation units compile in parallel (see Makefile).
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
#define MCP_ROW(cond, ...) \
  if (cond) return run<KT>(__VA_ARGS__, s, stream)

// The kernels on the spec's normals or the bootstrap's rows and the unfolded recurrence, and the plain Gaussian kernel on native
// math, in passes of KT = 1 or 8 portfolios.  The predicates name the draw source alone; every row states its compounding, and
// only the plain, drawdown, horizon and bootstrap kernels compound in logs.
template <int KT>
static hipError_t ladder(const PathKernel& k, const PathLaunchArgs& s, hipStream_t stream) {
  constexpr int NB = MCP_NB;
  const bool lg = k.logc;
  const bool gauss = !k.boot && !k.stt && !k.gv && !k.jp && !k.rs;             // Gaussian draws
  const bool j = k.jp && !k.rs && !k.boot && !k.stt && !k.gv;                  // Gaussian draws and the market jump (SPEC.md 2.5)
  const bool r = k.rs && !k.jp && !k.boot && !k.stt && !k.gv;                  // Gaussian draws on the regime's drift and factor (SPEC.md 2.6)
  const bool t = k.stt && !k.gv && !k.boot, g = k.gv && !k.boot;                // Student-t draws; GARCH (nu = 0: Gaussian draws)
  const bool bl = k.boot && k.blds && !k.stt && !k.gv && !k.fh, bg = k.boot && !k.blds && !k.stt && !k.gv && !k.fh;   // rows from LDS / global memory
  if (k.fh) {                                             // SPEC.md 4.11: filtered rows, with or without horizons (H = 0: one segment)
    const bool ok = (k.family == FAM_PLAIN || k.family == FAM_HZ) && k.boot && !k.stt && !k.gv && !k.jp && !k.rs && !k.native && !k.anti && !lg;
    MCP_ROW(ok && k.blds, mc_paths_fhs_kernel<NB, KT, 1, true>);
    MCP_ROW(ok && !k.blds, mc_paths_fhs_kernel<NB, KT, 1, false>);
    return hipErrorInvalidValue;
  }
  if (k.pi) {                                             // SPEC.md 4.15: the GARCH walk (also Gaussian and Student-t requests) or the jump walk
    const bool ok = (k.family == FAM_DD || k.family == FAM_HZ) && !k.boot && !k.rs && !k.native && !k.anti && !lg;
    const bool gw = ok && k.stt && k.gv && !k.jp, jw = ok && k.jp && !k.stt && !k.gv, dd = k.family == FAM_DD;
    MCP_ROW(gw && !dd, mc_paths_pi_kernel<NB, KT, 1, false, false>);
    MCP_ROW(gw && dd, mc_paths_pi_kernel<NB, KT, 1, false, true>);
    MCP_ROW(jw && !dd, mc_paths_pi_kernel<NB, KT, 1, true, false>);
    MCP_ROW(jw && dd, mc_paths_pi_kernel<NB, KT, 1, true, true>);
    return hipErrorInvalidValue;
  }
  if (k.anti) {                                           // SPEC.md 2.3: gv names the GARCH walk, which also serves Student-t requests
    const bool lean = gauss && !k.native, gw = k.stt && k.gv && !k.jp && !k.rs && !k.boot && !k.native && !lg;
    switch (k.family) {
      case FAM_PLAIN:
        MCP_ROW(lean && lg, mc_paths_anti_kernel<NB, KT, 1, true, PathArgsA>);
        MCP_ROW(lean && !lg, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsA>);
        MCP_ROW(gw, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsGA>);
        break;
      case FAM_DD:
        MCP_ROW(lean && lg, mc_paths_anti_kernel<NB, KT, 1, true, PathArgsADD>);
        MCP_ROW(lean && !lg, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsADD>);
        MCP_ROW(gw, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsGADD>);
        break;
      case FAM_HZ:
        MCP_ROW(lean && lg, mc_paths_anti_kernel<NB, KT, 1, true, PathArgsAHZ>);
        MCP_ROW(lean && !lg, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsAHZ>);
        MCP_ROW(gw, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsGAHZ>);
        break;
    }
    return hipErrorInvalidValue;
  }
  if (k.native) {
    MCP_ROW(k.family == FAM_PLAIN && gauss && lg, mc_paths_kernel<NB, KT, 1, true, false, true>);
    MCP_ROW(k.family == FAM_PLAIN && gauss && !lg, mc_paths_kernel<NB, KT, 1, true, false, false>);
    return hipErrorInvalidValue;
  }
  switch (k.family) {
    case FAM_PLAIN:
      MCP_ROW(gauss && lg, mc_paths_kernel<NB, KT, 1, false, false, true>);
      MCP_ROW(gauss && !lg, mc_paths_kernel<NB, KT, 1, false, false, false>);
      MCP_ROW(t && !lg, mc_paths_t_kernel<NB, KT, 1>);
      MCP_ROW(g && !lg, mc_paths_g_kernel<NB, KT, 1>);
      MCP_ROW(j && !lg, mc_paths_j_kernel<NB, KT, 1>);
      MCP_ROW(r && !lg, mc_paths_r_kernel<NB, KT, 1>);
      MCP_ROW(bl && lg, mc_paths_boot_kernel<NB, KT, 1, true, true>);
      MCP_ROW(bl && !lg, mc_paths_boot_kernel<NB, KT, 1, false, true>);
      MCP_ROW(bg && lg, mc_paths_boot_kernel<NB, KT, 1, true, false>);
      MCP_ROW(bg && !lg, mc_paths_boot_kernel<NB, KT, 1, false, false>);
      break;
    case FAM_DD:
      MCP_ROW(gauss && lg, mc_paths_dd_kernel<NB, KT, 1, true>);
      MCP_ROW(gauss && !lg, mc_paths_dd_kernel<NB, KT, 1, false>);
      MCP_ROW(t && !lg, mc_paths_t_dd_kernel<NB, KT, 1>);
      MCP_ROW(g && !lg, mc_paths_g_dd_kernel<NB, KT, 1>);
      MCP_ROW(j && !lg, mc_paths_j_dd_kernel<NB, KT, 1>);
      MCP_ROW(r && !lg, mc_paths_r_dd_kernel<NB, KT, 1>);
      break;
    case FAM_HZ:
      MCP_ROW(gauss && lg, mc_paths_hz_kernel<NB, KT, 1, true>);
      MCP_ROW(gauss && !lg, mc_paths_hz_kernel<NB, KT, 1, false>);
      MCP_ROW(t && !lg, mc_paths_t_hz_kernel<NB, KT, 1>);
      MCP_ROW(g && !lg, mc_paths_g_hz_kernel<NB, KT, 1>);
      MCP_ROW(j && !lg, mc_paths_j_hz_kernel<NB, KT, 1>);
      MCP_ROW(r && !lg, mc_paths_r_hz_kernel<NB, KT, 1>);
      MCP_ROW(bl && lg, mc_paths_boot_hz_kernel<NB, KT, 1, true, true>);
      MCP_ROW(bl && !lg, mc_paths_boot_hz_kernel<NB, KT, 1, false, true>);
      MCP_ROW(bg && lg, mc_paths_boot_hz_kernel<NB, KT, 1, true, false>);
      MCP_ROW(bg && !lg, mc_paths_boot_hz_kernel<NB, KT, 1, false, false>);
      break;
    case FAM_REB:
      MCP_ROW(gauss && !lg && !k.tb, mc_paths_reb_kernel<NB, KT, 1, false, false>);
      MCP_ROW(bl && !lg && !k.tb, mc_paths_reb_kernel<NB, KT, 1, true, true>);
      MCP_ROW(bg && !lg && !k.tb, mc_paths_reb_kernel<NB, KT, 1, true, false>);
      if constexpr (KT == 1) {                             // SPEC.md 4.18: tolerance bands, every K as passes of one portfolio
        MCP_ROW(gauss && !lg && k.tb, mc_paths_band_kernel<NB, 1, 1, false, false>);
        MCP_ROW(bl && !lg && k.tb, mc_paths_band_kernel<NB, 1, 1, true, true>);
        MCP_ROW(bg && !lg && k.tb, mc_paths_band_kernel<NB, 1, 1, true, false>);
      }
      break;
    case FAM_CF:
      MCP_ROW(gauss && !lg && !k.gp && !k.sp && !k.lt, mc_paths_cf_kernel<NB, KT, 1, false, false, false>);
      MCP_ROW(t && !lg && !k.gp && !k.sp && !k.lt, mc_paths_cf_kernel<NB, KT, 1, false, false, true>);
      MCP_ROW(bl && !lg && !k.gp && !k.sp && !k.lt, mc_paths_cf_kernel<NB, KT, 1, true, true, false>);
      MCP_ROW(bg && !lg && !k.gp && !k.sp && !k.lt, mc_paths_cf_kernel<NB, KT, 1, true, false, false>);
      MCP_ROW(gauss && !lg && k.sp && !k.lt, mc_paths_spend_kernel<NB, KT, 1, false, false, false>);   // SPEC.md 4.16: the path's own withdrawal
      MCP_ROW(t && !lg && k.sp && !k.lt, mc_paths_spend_kernel<NB, KT, 1, false, false, true>);
      MCP_ROW(bl && !lg && k.sp && !k.lt, mc_paths_spend_kernel<NB, KT, 1, true, true, false>);
      MCP_ROW(bg && !lg && k.sp && !k.lt, mc_paths_spend_kernel<NB, KT, 1, true, false, false>);
      MCP_ROW(gauss && !lg && k.gp && !k.lt, mc_paths_glide_kernel<NB, KT, 1, false, false, false>);   // SPEC.md 4.14: the weights on a schedule
      MCP_ROW(t && !lg && k.gp && !k.lt, mc_paths_glide_kernel<NB, KT, 1, false, false, true>);
      MCP_ROW(bl && !lg && k.gp && !k.lt, mc_paths_glide_kernel<NB, KT, 1, true, true, false>);
      MCP_ROW(bg && !lg && k.gp && !k.lt, mc_paths_glide_kernel<NB, KT, 1, true, false, false>);
      MCP_ROW(gauss && !lg && k.sp && k.lt, mc_paths_spend_life_kernel<NB, KT, 1, false, false, false>);   // SPEC.md 4.17: the lifetime twins
      MCP_ROW(t && !lg && k.sp && k.lt, mc_paths_spend_life_kernel<NB, KT, 1, false, false, true>);
      MCP_ROW(bl && !lg && k.sp && k.lt, mc_paths_spend_life_kernel<NB, KT, 1, true, true, false>);
      MCP_ROW(bg && !lg && k.sp && k.lt, mc_paths_spend_life_kernel<NB, KT, 1, true, false, false>);
      MCP_ROW(gauss && !lg && k.gp && k.lt, mc_paths_glide_life_kernel<NB, KT, 1, false, false, false>);   // G = 0: the cash-flow walk
      MCP_ROW(t && !lg && k.gp && k.lt, mc_paths_glide_life_kernel<NB, KT, 1, false, false, true>);
      MCP_ROW(bl && !lg && k.gp && k.lt, mc_paths_glide_life_kernel<NB, KT, 1, true, true, false>);
      MCP_ROW(bg && !lg && k.gp && k.lt, mc_paths_glide_life_kernel<NB, KT, 1, true, false, false>);
      break;
    case FAM_OV:
      MCP_ROW(gauss && !lg && !k.dd, mc_paths_ov_kernel<NB, KT, 1, false, false>);
      MCP_ROW(gauss && !lg && k.dd, mc_paths_ov_kernel<NB, KT, 1, false, true>);
      MCP_ROW(t && !lg && !k.dd, mc_paths_ov_kernel<NB, KT, 1, true, false>);
      MCP_ROW(t && !lg && k.dd, mc_paths_ov_kernel<NB, KT, 1, true, true>);
      break;
  }
  return hipErrorInvalidValue;
}

hipError_t MCP_CAT(launch_paths_nb, MCP_NB)(const PathKernel& k, const PathLaunchArgs& s, hipStream_t stream) {
  constexpr int NB = MCP_NB, KT = 1;                       // the folded step and the attribution walk: one portfolio per pass
  if (k.anti && (k.fold || k.family == FAM_AT)) return hipErrorInvalidValue;
  if (k.fh && (k.fold || k.family == FAM_AT)) return hipErrorInvalidValue;
  if (k.jp && (k.fold || k.uhi || k.native || k.anti || k.fh || k.family == FAM_AT)) return hipErrorInvalidValue;
  if (k.rs && (k.fold || k.uhi || k.native || k.anti || k.fh || k.family == FAM_AT)) return hipErrorInvalidValue;
  if (k.gp && (k.family != FAM_CF || k.fold || k.uhi || k.native || k.anti || k.fh || k.jp || k.rs || k.gv)) return hipErrorInvalidValue;
  if (k.pi && (k.fold || k.uhi || k.native || k.anti || k.fh || k.rs || k.gp || k.family == FAM_AT)) return hipErrorInvalidValue;
  if (k.sp && (k.family != FAM_CF || k.fold || k.uhi || k.native || k.anti || k.fh || k.jp || k.rs || k.gv || k.gp || k.pi)) return hipErrorInvalidValue;
  if (k.lt && (k.family != FAM_CF || k.gp == k.sp || k.fold || k.uhi || k.native || k.anti || k.fh || k.jp || k.rs || k.gv || k.pi)) return hipErrorInvalidValue;
  if (k.tb && (k.family != FAM_REB || k.kt8 || k.fold || k.uhi || k.native || k.anti || k.fh || k.jp || k.rs || k.gv || k.stt || k.gp || k.pi || k.sp || k.lt))
    return hipErrorInvalidValue;
  if (k.fold) {                                            // rho = c + v.z: the plain Gaussian walk on the spec's normals
    const bool ok = k.family == FAM_PLAIN && !k.boot && !k.stt && !k.gv && !k.native && !k.kt8;
    MCP_ROW(ok && k.logc, mc_paths_kernel<NB, 1, 1, false, true, true>);
    MCP_ROW(ok && !k.logc, mc_paths_kernel<NB, 1, 1, false, true, false>);
    return hipErrorInvalidValue;
  }
  if (k.uhi) {                                             // one p_hi for the whole launch (lean_range): the plain Gaussian walk, lean
    if constexpr (NB <= LEAN_MAX_NB) {
      const bool ok = k.family == FAM_PLAIN && !k.boot && !k.stt && !k.gv && !k.native && !k.kt8 && !k.anti && !k.fh;
      MCP_ROW(ok && k.logc, mc_paths_lean_kernel<NB, true>);
      MCP_ROW(ok && !k.logc, mc_paths_lean_kernel<NB, false>);
    }
    return hipErrorInvalidValue;
  }
  if (k.family == FAM_AT) {                                // simple compounding, the GARCH kernel's draws
    MCP_ROW(!k.kt8 && !k.native && !k.logc && !k.boot, mc_paths_attr_kernel<NB, 1, 1>);
    return hipErrorInvalidValue;
  }
  return k.kt8 ? ladder<8>(k, s, stream) : ladder<1>(k, s, stream);
}
#undef MCP_ROW

}  // namespace mcp

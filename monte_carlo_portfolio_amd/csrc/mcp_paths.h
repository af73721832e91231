// mcp_paths.h -- the fused Monte Carlo path kernel (template; instantiated per NB in mcp_paths_inst.hip).
//
//   mc_paths_kernel   N1+N2+N3 of SURVEY.md section 8(a): Philox4x32-10 -> normals (inverse CDF) -> r = mu + L z ->
//                     rho = w.r -> V <- V(1+rho) over T steps, entirely in registers; writes V_T
//                     (4 B/path, coalesced).  Epilogue (when the launch carries a statistics workspace): with V still in
//                     registers, x = V/v0 - 1, the shifted moments {n, sum (x-c), sum (x-c)^2, min, max} in fp64 by
//                     wavefront shuffle reduction -> ONE partial per workgroup and portfolio, and the digit-0 histogram
//                     of the radix select in LDS -> global.  The select's two remaining digits are streaming passes.
//                     Conventions inherited from the reference: fixed-weight portfolio return
//                     `returns_df @ ws` (app.py:710), compounding prod(1+r) (app.py:249, app.py:253).
//
// Layout: one lane = one path (PPT independent paths per lane for ILP); the Cholesky factor, drift
// and weights are wave-uniform and are read with scalar loads (s_load_dword*) straight into SGPR
// operands of the FMAs -- they never occupy VGPRs or LDS bandwidth.  Roofline: VALU issue
// (DESIGN.md section 4); HBM traffic is 4 B per path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mcport.h"
#include "mcp_device.h"
#include "mcp_stats_kernels.h"

#ifndef MCP_MIN_WAVES
#define MCP_MIN_WAVES 6     // __launch_bounds__ 2nd argument for N <= 16, one portfolio: at least 6 waves/SIMD (the kernel needs 74
                            // VGPRs; forced into 72 for 7 waves it spills 24 B per lane outside the loop and is 0.5 % slower)
#endif
#ifndef MCP_MIN_WAVES_BIG
#define MCP_MIN_WAVES_BIG 1 // the same for 16 < N <= 64, one portfolio.  4 (<= 128 VGPRs) was measured: the 64 live normals plus the
                            // Philox / transform state do not fit, 108-148 B per lane spill into the step loop, -10 % (profiles/r03_lab_n64.txt)
#endif
#ifndef MCP_MIN_WAVES_REB
#define MCP_MIN_WAVES_REB 5 // the rebalancing kernel (N <= 16, one portfolio) holds the N4 returns B since the last rebalance on top: at
                            // 6 waves (80 VGPRs) it spilled 20 dwords into its step loop; at 5 it gets 96, no scratch in the loop
#endif
#ifndef MCP_MIN_WAVES_REB8
#define MCP_MIN_WAVES_REB8 4 // the same for 8 portfolios, N <= 16: unbounded it took 137 VGPRs (3 waves); at 4 it gets 128, no scratch in the loop
#endif
#ifndef MCP_MIN_WAVES_CF8
#define MCP_MIN_WAVES_CF8 5 // the cash-flow kernel for 8 portfolios, N <= 16: unbounded it took 102 VGPRs (4 waves) where its twin without cash
                            // flows runs 5; at 5 it gets 93, no scratch, and measured 1.10x the twin instead of 1.12x
#endif
#ifndef MCP_MIN_WAVES_OV
#define MCP_MIN_WAVES_OV 4  // the overlay kernel (N <= 16, one portfolio) holds the N4 prices P on top, as the rebalancing kernel holds B: at
                            // 5 waves (96 VGPRs) the N = 16 kernels spilled 2 to 15 dwords to scratch outside the walk; at 4 none does
#endif
#ifndef MCP_MIN_WAVES_OV8
#define MCP_MIN_WAVES_OV8 4 // the same for 8 portfolios, N <= 16
#endif
#ifndef MCP_MIN_WAVES_AT
#define MCP_MIN_WAVES_AT 5  // the attribution kernel (N <= 16, one portfolio) holds the N4 contributions A on top of the GARCH kernel's state, as
                            // the rebalancing kernel holds B: at 5 waves it gets 96 VGPRs, no scratch (profiles/attribution_isa.txt)
#endif
#ifndef MCP_MIN_WAVES_PI
#define MCP_MIN_WAVES_PI 5  // the floor-protection kernel on the jump walk (N <= 16, one portfolio) carries the peak M on top of the jump kernel's
                            // state: at 6 waves (80 VGPRs) the N = 16 kernels reloaded one spilled pair inside the step loop; at 5 none does.  On
                            // the GARCH walk it fits in 80 and keeps MCP_MIN_WAVES (profiles/protect_isa.txt)
#endif
#ifndef MCP_MIN_WAVES_SP
#define MCP_MIN_WAVES_SP 6  // the spending kernel (N <= 16, one portfolio) carries the withdrawal w and the payout Y on top of the cash-flow
                            // kernel's state: unbounded it took 83 VGPRs (5 waves); at 6, the most the 25 KiB of LDS admit, it gets 80 and no listing shows
                            // scratch in the loop over t (profiles/spend_isa.txt)
#endif
#ifndef MCP_MIN_WAVES_SP8
#define MCP_MIN_WAVES_SP8 4 // the same for 8 portfolios, N <= 16, 16 registers on top of the cash-flow kernel's: unbounded it took 110-115
                            // VGPRs (4 waves); at 5 (96) the Student-t kernel reloads spilled registers inside the loop over t, at 4 nothing spills
#endif
#ifndef MCP_MIN_WAVES_ANTI
#define MCP_MIN_WAVES_ANTI 5 // the antithetic kernels (N <= 16, one portfolio) carry the second member's V, row-pair accumulator and rho (and
                            // peak and drawdown) next to the first's: see profiles/antithetic_isa.txt
#endif
#ifndef MCP_MIN_WAVES_PU
#define MCP_MIN_WAVES_PU 5  // the drift-uncertainty kernels (N <= 16, one portfolio) hold the path's own drift, N4 registers, on top of their
#endif                      // twins' state, as the rebalancing kernel holds B: 5 waves (<= 96 VGPRs), no scratch in a walk (profiles/uncertain_isa.txt)
#ifndef MCP_MIN_WAVES_PU8
#define MCP_MIN_WAVES_PU8 4 // the same for 8 portfolios, N <= 16: 4 waves (<= 128 VGPRs), no scratch in a walk
#endif
#ifndef MCP_MIN_WAVES_UW8
#define MCP_MIN_WAVES_UW8 4 // the under-water twins for 8 portfolios, N <= 16, simple compounding, 16 counters on top of the drawdown kernel's
                            // state: unbounded the Gaussian twin took 129 VGPRs at N = 16 and the jump twin 134 (3 waves) where their parents
                            // run 4; at 4 they get 128 and no listing shows scratch in a loop over t (profiles/underwater_isa.txt)
#endif
#ifndef MCP_EXP_VKEYS
#define MCP_EXP_VKEYS 1
#endif
#ifndef MCP_EXP_BOOT_SWIZZLE  // 1: the bootstrap's LDS row table is XOR-swizzled (BootSwizzle); 0: plain layout (lab builds)
#define MCP_EXP_BOOT_SWIZZLE 1
#endif
#ifndef MCP_EXP_LDSPAR      // 1: drift from LDS (default); 2: drift and (one portfolio) weights from LDS; 0: both from SGPRs.  2 was priced at
#define MCP_EXP_LDSPAR 1    // -2 % by the issue model and measured within +-0.5 % of 1 (profiles/r02_lab5.txt): not to be tried again
#endif
#ifndef MCP_EXP_GEMV2       // the lean kernel's factor: 1: row pairs (m, m + 1) in flight together, two accumulators interleaved column by
#define MCP_EXP_GEMV2 1     // column, every row's own chain kept (bit-identical); 0: one row pair after another (tools/kernel_lab.py arm `feed_base`)
#endif
#ifndef MCP_EXP_PRIO        // the lean kernel's wave priority: 1: raised over the factor and the weight dot of every step (s_setprio, two per
#define MCP_EXP_PRIO 1      // step); 0: never changed (tools/kernel_lab.py arm `gemv2`).  Raised over Philox and the normals instead it cost 4 %,
#endif                      // and factor loads issued a Philox block ahead gained nothing (profiles/gemv_feed_probe.json): not to be tried again

namespace mcp {

#ifdef MCP_DIAG_CLOCK
// Diagnostic build only (tools/clock_probe.py; MI355X_MICROARCH.md, DVFS give-back item 6): every workgroup of mc_paths_kernel
// stamps s_memtime (shader cycles) and s_memrealtime (100 MHz) around its step loops into a buffer of its own that nothing
// else reads; in-kernel clock = d(memtime) / d(memrealtime) x 100 MHz.  No stamp executes in the product build.
extern __device__ unsigned long long mcp_diag_stamps[2 * 8192];
#endif

// The kernel arguments as struct A, through the kernel-argument pointer and the constant address space: what is read through it is
// wave-uniform (scalar loads) and is loaded where it is used -- the compiler cannot see through the pointer, so nothing is held
// in SGPRs across the walk (the Cholesky factor lives there).
template <class A>
__device__ __forceinline__ const __attribute__((address_space(4))) A* kernarg() {
  typedef const __attribute__((address_space(4))) A* cst_p;
  cst_p k = (cst_p)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}
// has_<m><A>: the argument struct A carries the member (block) m.  The block accessors below and make_args ask it inside a
// template on A: in a kernel the type of `a` is not dependent, so `if constexpr (BOOT) bt = a.bt;` would still be checked there.
#define MCP_HAS_MEMBER(m)                                                 \
  template <class A, class = void> struct has_##m : std::false_type {}; \
  template <class A> struct has_##m<A, std::void_t<decltype(A::m)>> : std::true_type {};
MCP_HAS_MEMBER(hz) MCP_HAS_MEMBER(mdd) MCP_HAS_MEMBER(bt) MCP_HAS_MEMBER(st) MCP_HAS_MEMBER(gv) MCP_HAS_MEMBER(cf)
MCP_HAS_MEMBER(ov) MCP_HAS_MEMBER(at) MCP_HAS_MEMBER(period) MCP_HAS_MEMBER(pr)
MCP_HAS_MEMBER(fh) MCP_HAS_MEMBER(p_hi) MCP_HAS_MEMBER(jp) MCP_HAS_MEMBER(rs) MCP_HAS_MEMBER(gp)
MCP_HAS_MEMBER(pi) MCP_HAS_MEMBER(sp) MCP_HAS_MEMBER(lf) MCP_HAS_MEMBER(tb) MCP_HAS_MEMBER(vt) MCP_HAS_MEMBER(uw) MCP_HAS_MEMBER(pu)
#undef MCP_HAS_MEMBER

struct PathArgs {
  const float* __restrict__ packed;   // [mu N4][L row pairs N4(N4/2+1)][W Kpad*N4]  (mcp_pack_params)
  float* __restrict__ terminal;       // [K][stride]
  const float4* __restrict__ tables;  // [ICDF_ENTRIES] inverse-CDF coefficient table (device copy of mcp_icdf_table.inc)
  // fused statistics epilogue (all three NULL: terminal values only)
  const double* __restrict__ pivot;   // [K] shift c of the moments (mcp_pivots), NULL = 0
  MomentPartial* __restrict__ partials;   // [K][slots]
  unsigned long long* __restrict__ hist;  // [K][2][MCP_SELECT_BINS]: digit-0 histogram into [k][0] (K <= 16 kernels only)
  uint64_t slots;                     // MomentPartial slots per portfolio (= gridDim.x of mc_paths_kernel, n/64 tiles of the sweeps)
  double v0d;                         // (double)(float)v0
  double inv_v0d;                     // 1 / v0d; exact when v0 is a power of two (v0_pow2), then x = fma(V, inv_v0d, -1) IS V/v0 - 1
  int32_t v0_pow2;
  uint64_t seed, path_begin, n_paths, stride;
  int32_t n_steps, n_portfolios, k_begin, compounding;
  int32_t k_count;                    // sweep kernels: portfolios [k_begin, k_begin + k_count) belong to this launch
  float v0;
  uint32_t fold_offset;               // float index of [c, v_0 .. v_{N4-1}] (portfolio 0 folded through L, SPEC.md 4.1)
};

// Arguments of mc_paths_lean_kernel: PathArgs and the high counter word that every path of the launch shares,
// p_hi = path_begin >> 32 = (path_begin + n_paths - 1) >> 32 (lean_range in mcp_route.h decides it on the host).
struct PathArgsLean : PathArgs {
  uint32_t p_hi;
  uint32_t pad;
};
// p_hi of a lean launch, a kernel argument (an SGPR for the whole walk); the argument also selects the kernel's argument type.
template <class A>
__device__ __forceinline__ uint32_t uniform_hi(const A& a) {
  if constexpr (has_p_hi<A>::value) return a.p_hi;
  else return 0u;
}

// Arguments of mc_paths_dd_kernel: PathArgs (at offset 0, where the epilogue reads it through the kernarg pointer) and the
// per-path drawdown output of SPEC.md 4.2.
struct PathArgsDD : PathArgs {
  float* __restrict__ mdd;            // [K][mdd_stride]: q (simple) or d (log) per path
  uint64_t mdd_stride;
};

// Arguments of mc_paths_hz_kernel: PathArgs and the values at the horizons of SPEC.md 4.3.
struct PathArgsHZ : PathArgs {
  float* __restrict__ hz;             // [H][K][hz_stride]: V_h (simple) / S_h (log), row h*K + k
  uint64_t hz_stride;
  int32_t n_horizons;                 // H in [1, MCP_MAX_HORIZONS]
  int32_t steps[MCP_MAX_HORIZONS];    // strictly increasing, in [1, n_steps]
};

// The observed return rows of the bootstrap kernels (SPEC.md 2.1 / 4.4).
struct BootArgs {
  const float4* __restrict__ rows;    // [R][NB] float4: row j zero-padded to N4 floats (device copy, not swizzled)
  uint64_t thr;                       // restart when (uint64)x1 < thr; in [0, 2^32] (SPEC.md 2.1)
  uint32_t n_rows;                    // R in [1, MCP_MAX_BOOT_ROWS]
  uint32_t pad;
};
// Arguments of mc_paths_boot_kernel / mc_paths_boot_hz_kernel: PathArgs (PathArgsHZ) first, as for the drawdown kernel.
struct PathArgsBT : PathArgs { BootArgs bt; };
struct PathArgsBTHZ : PathArgsHZ { BootArgs bt; };
template <class A>
__device__ __forceinline__ BootArgs boot_args(const A& a) {
  if constexpr (has_bt<A>::value) return a.bt;
  else return BootArgs{};
}
// Arguments of mc_paths_reb_kernel (SPEC.md 4.5): the horizons of PathArgsHZ (n_horizons = 0: none), the row table of the
// bootstrap (read only when BOOT) and the rebalancing rule.
struct PathArgsRB : PathArgsHZ {
  BootArgs bt;
  int32_t period;                     // m >= 0: a rebalance after every step s with s mod m == 0 and s < T (0: never)
  float cost;                         // kappa32 = fl32(kappa), in [0, 1)
};
// The Student-t draws of SPEC.md 2.2 / 4.6: the degrees of freedom nu in [3, MCP_MAX_T_DOF], wave-uniform.  Appended to the
// arguments of the plain, drawdown and horizon kernels (mc_paths_t_kernel, mc_paths_t_dd_kernel, mc_paths_t_hz_kernel).
struct StudentArgs {
  int32_t dof;
  int32_t pad;
};
struct PathArgsT : PathArgs { StudentArgs st; };
struct PathArgsTDD : PathArgsDD { StudentArgs st; };
struct PathArgsTHZ : PathArgsHZ { StudentArgs st; };
// nu of a launch whose arguments carry the Student-t block, read where it is needed (kernarg); the argument only selects the
// kernel's argument type.
template <class A>
__device__ __forceinline__ int32_t student_dof(const A&) {
  if constexpr (has_st<A>::value) return kernarg<A>()->st.dof;
  else return 0;
}

// GARCH(1,1) on the covariance (SPEC.md 4.9): the host constants a_N = fl32(a / N), b, omega = fl32(1 - a - b), the start h0 of the
// per-path variance ratio h, and N (the padding normals j >= N stay out of the step's shock q).  Appended, after the degrees of
// freedom (0: Gaussian draws), to the arguments of the plain, drawdown and horizon kernels (mc_paths_g_kernel,
// mc_paths_g_dd_kernel, mc_paths_g_hz_kernel).
struct GarchArgs {
  float a_n, b, omega, h0;
  int32_t n_assets;
  int32_t pad;
};
struct PathArgsG : PathArgs { StudentArgs st; GarchArgs gv; };
struct PathArgsGDD : PathArgsDD { StudentArgs st; GarchArgs gv; };
struct PathArgsGHZ : PathArgsHZ { StudentArgs st; GarchArgs gv; };
// The GARCH block of a g kernel's launch, read where it is used (kernarg).
typedef const __attribute__((address_space(4))) GarchArgs* cgarch_p;
template <class A>
__device__ __forceinline__ cgarch_p garch_args(const A&) {
  if constexpr (has_gv<A>::value) return &kernarg<A>()->gv;
  else return nullptr;
}

// Merton jump-diffusion (SPEC.md 2.5 / 4.12): one market jump J per path and step, drawn from one Philox block on counter stream 3
// -- the count n = #{k : x0 < thr[k]} (thr[k] = floor(2^32 P(Poisson >= k + 1)), at most MCP_MAX_JUMPS = 8 jumps), the size from
// Z(x1) -- and added to every asset through its loading: row i starts at fma(b_i, J, mu'_i), mu' the compensated drift the host
// packs in place of mu.  `loading` is zero-padded to N4.  Appended to the arguments of the plain, drawdown and horizon kernels
// (mc_paths_j_kernel, mc_paths_j_dd_kernel, mc_paths_j_hz_kernel).
struct JumpArgs {
  const float* __restrict__ loading;  // [N4] device copy
  uint32_t thr[8];
  float m, s;                         // m32 = fl32(mean), s32 = fl32(std) of one jump
};
struct PathArgsJ : PathArgs { JumpArgs jp; };
struct PathArgsJDD : PathArgsDD { JumpArgs jp; };
struct PathArgsJHZ : PathArgsHZ { JumpArgs jp; };
// The jump block of a j kernel's launch, read where it is used (kernarg).
typedef const __attribute__((address_space(4))) JumpArgs* cjump_p;
template <class A>
__device__ __forceinline__ cjump_p jump_args(const A&) {
  if constexpr (has_jp<A>::value) return &kernarg<A>()->jp;
  else return nullptr;
}

// Two-regime Markov switching (SPEC.md 2.6 / 4.13): every path carries a regime s_t in {0, 1}, moved once per step by one Philox
// block on counter stream 4 -- s_0 = x1 < thr_start (the block of t = 0), s_{t+1} = s_t == 0 ? x0 < thr01 : !(x0 < thr10), uint64
// compares against thresholds in [0, 2^32] -- and step t walks on (mu, L) of regime s_t: the packed block's for regime 0, `block1`
// ([mu1 N4][L1 row pairs N4(N4/2+1)], the layout of mcp_pack_params, behind the launch's packed block) for regime 1.  Appended to
// the arguments of the plain, drawdown and horizon kernels (mc_paths_r_kernel, mc_paths_r_dd_kernel, mc_paths_r_hz_kernel).
struct RegimeArgs {
  const float* __restrict__ block1;   // [N4 + N4(N4/2+1)] device copy
  uint64_t thr01, thr10, thr_start;
};
struct PathArgsR : PathArgs { RegimeArgs rs; };
struct PathArgsRDD : PathArgsDD { RegimeArgs rs; };
struct PathArgsRHZ : PathArgsHZ { RegimeArgs rs; };
// The regime block of an r kernel's launch, read where it is used (kernarg).
typedef const __attribute__((address_space(4))) RegimeArgs* cregime_p;
template <class A>
__device__ __forceinline__ cregime_p regime_args(const A&) {
  if constexpr (has_rs<A>::value) return &kernarg<A>()->rs;
  else return nullptr;
}

// Filtered historical simulation (SPEC.md 2.4 / 4.11): the rows of BootArgs are the filtered residuals E, `shock` holds the rows'
// shocks s_j ([R] floats behind the rows, padded to a multiple of 4), and a, b, omega, h0 are the binary32 constants of SPEC.md 4.9
// -- a itself, not a_N: the shock is already per asset.
struct FiltArgs {
  const float* __restrict__ shock;    // [4 ceil(R/4)] device copy
  float a, b, omega, h0;
};
// Arguments of mc_paths_fhs_kernel: the horizons of PathArgsHZ (n_horizons = 0: none), the residual rows and the filter block.
struct PathArgsFH : PathArgsHZ {
  BootArgs bt;
  FiltArgs fh;
};
// The filter block of an fhs kernel's launch, read where it is used (kernarg).
typedef const __attribute__((address_space(4))) FiltArgs* cfilt_p;
template <class A>
__device__ __forceinline__ cfilt_p filt_args(const A&) {
  if constexpr (has_fh<A>::value) return &kernarg<A>()->fh;
  else return nullptr;
}

// Risk attribution (SPEC.md 4.10 / 5.9): the second walk of one portfolio per pass that carries the assets' contributions A_i.
// var: the VaR of every portfolio from the call's statistics (the tail is x <= var); partials: one record of ATTR_HEAD + 3 N4
// binary64 sums per portfolio and workgroup, {n, n_tail, S1, then per asset sum A, sum_tail A, sum A (x - c)}; contrib: the
// per-path contributions, or NULL.  The pivot c is PathArgs::pivot.
constexpr int ATTR_HEAD = 3;
__host__ __device__ constexpr int attr_record_len(int n4) { return ATTR_HEAD + 3 * n4; }
struct AttrArgs {
  const double* __restrict__ var;     // [K]
  double* __restrict__ partials;      // [K][gridDim.x][attr_record_len(N4)]
  float* __restrict__ contrib;        // NULL or [K][n_assets][contrib_stride]
  uint64_t contrib_stride;
  int32_t n_assets;
  int32_t pad;
};
// Arguments of mc_paths_attr_kernel: those of mc_paths_g_kernel (student_dof and garch_args read them at the same offsets) and the
// attribution block.
struct PathArgsAT : PathArgsG { AttrArgs at; };
// The per-wave accumulators of the attribution epilogue: PATH_BLOCK / 64 records in LDS (mc_paths_attr_kernel only).
template <int N4>
__device__ __forceinline__ double* attr_wave_slots() {
  __shared__ double s_attr[4 * attr_record_len(N4)];
  return s_attr;
}

// Antithetic pairs (SPEC.md 2.3 / 5.10): a lane walks both members of one pair; in such a launch PathArgs::path_begin and n_paths
// count PAIRS (the Philox counters carry the pair id), the members 2j and 2j + 1 are adjacent in every output row (strides even,
// one 8-byte store per lane), and the epilogue leaves sum (x_2j - c)(x_2j+1 - c) per workgroup and portfolio in `cross`.
struct PairArgs {
  double* __restrict__ cross;         // [K][gridDim.x], NULL exactly when PathArgs::partials is
};
// Arguments of mc_paths_anti_kernel: those of the plain, drawdown or horizon kernel, or of their GARCH twins, and the pair block.
struct PathArgsA : PathArgs { PairArgs pr; };
struct PathArgsADD : PathArgsDD { PairArgs pr; };
struct PathArgsAHZ : PathArgsHZ { PairArgs pr; };
struct PathArgsGA : PathArgsG { PairArgs pr; };
struct PathArgsGADD : PathArgsGDD { PairArgs pr; };
struct PathArgsGAHZ : PathArgsGHZ { PairArgs pr; };
// The cross-product partials of an antithetic launch, read where they are written (kernarg).
template <class A>
__device__ __forceinline__ double* pair_cross(const A&) {
  if constexpr (has_pr<A>::value) return kernarg<A>()->pr.cross;
  else return nullptr;
}
// The per-wave accumulators of the cross products: PATH_BLOCK / 64 slots per portfolio of the pass in LDS (antithetic kernels only).
template <int KT>
__device__ __forceinline__ double* pair_wave_slots() {
  __shared__ double s_cross[4 * KT];
  return s_cross;
}

// Cash flows and ruin (SPEC.md 4.7): the schedule c_1 .. c_T, one binary32 flow per step, the same for every portfolio.
struct CashArgs {
  const float* __restrict__ flows;    // [n_steps] device copy; flows[t] = c_{t+1} arrives at the end of step t
};
// Arguments of mc_paths_cf_kernel: the horizons of PathArgsHZ (n_horizons = 0: none), the row table of the bootstrap (read only
// when BOOT), nu (read only when STT) and the schedule.
struct PathArgsCF : PathArgsHZ {
  BootArgs bt;
  StudentArgs st;
  CashArgs cf;
};
// c_{t+1} of a cash-flow kernel's launch, read where it is used (kernarg): two scalar loads per step.
template <class A>
__device__ __forceinline__ float cash_flow(const A&, int t) {
  typedef const __attribute__((address_space(4))) float* cflow_p;
  if constexpr (has_cf<A>::value) return ((cflow_p)kernarg<A>()->cf.flows)[t];
  else return 0.0f;
}

// The glide path of SPEC.md 4.14: the weights of the walk change at the breaks b_1 < .. < b_G (steps in [1, n_steps - 1]).  Step s
// walks on block g = #{j : b_j < s}: block 0 is the packed weights of the launch, block g >= 1 is `targets + (g - 1) stride`, in the
// packed weights' own layout -- rows of N4 floats, the columns i >= N and the rows up to the end of the last pass of 8 zero.
struct GlideArgs {
  const float* __restrict__ targets;  // [n_breaks][stride] device copy
  uint32_t stride;                    // floats between consecutive target blocks (padded rows x N4)
  int32_t n_breaks;                   // G in [0, MCP_MAX_GLIDE]
  int32_t breaks[MCP_MAX_GLIDE];      // strictly increasing, in [1, n_steps - 1]
};
// Arguments of mc_paths_glide_kernel: those of mc_paths_cf_kernel and the glide block, read where it is needed (kernarg).
struct PathArgsGP : PathArgsCF { GlideArgs gp; };

// The spending rule of SPEC.md 4.16: per path and portfolio the walk carries the per-step withdrawal w (from w0) and the total paid out
// Y (from +0) next to V.  Every step pays w out of U0 = fma(V, rho, V), the step of ruin what is left; after every `every`-th step the
// review moves w to p32 V, held between lo32 and hi32 times the inflated w.  The constants are wave-uniform and read inside the
// review, w0 once per tile, the output where it is written.
struct SpendArgs {
  float p32, g32, lo32, hi32, w0;     // binary32: rate, 1 + inflation, 1 - down, 1 + up (may be +inf), the first withdrawal
  int32_t every;                      // review after the steps s with s mod every == 0; 0: never
  float* __restrict__ wd;             // [K][wd_stride] Y_T
  uint64_t wd_stride;
};
// Arguments of mc_paths_spend_kernel: those of mc_paths_cf_kernel (the schedule is not read) and the spending block.
struct PathArgsSP : PathArgsCF { SpendArgs sp; };
// The spending block of a spend kernel's launch, read where it is used (kernarg).
typedef const __attribute__((address_space(4))) SpendArgs* cspend_p;
template <class A>
__device__ __forceinline__ cspend_p spend_args(const A&) {
  if constexpr (has_sp<A>::value) return &kernarg<A>()->sp;
  else return nullptr;
}

// The lifetime of SPEC.md 4.17: per path and portfolio the walks with absorbing ruin may carry the number of steps l that stored a
// positive V, a uint32 from 0, and store it next to V_T.  The output is read from the kernel arguments where it is written.
struct LifeArgs {
  uint32_t* __restrict__ life;        // [K][life_stride] l
  uint64_t life_stride;
};
// Arguments of the lifetime twins: those of mc_paths_glide_kernel and mc_paths_spend_kernel, and the lifetime block behind them.
struct PathArgsGPL : PathArgsGP { LifeArgs lf; };
struct PathArgsSPL : PathArgsSP { LifeArgs lf; };
typedef const __attribute__((address_space(4))) LifeArgs* clife_p;
template <class A>
__device__ __forceinline__ clife_p life_args(const A&) {
  if constexpr (has_lf<A>::value) return &kernarg<A>()->lf;
  else return nullptr;
}

// Tolerance bands (SPEC.md 4.18): the rebalancing walk reviews every `period` steps and trades a path back to W only when a watched
// asset of that path has drifted out of its band.  `tol` is the table of the pass's portfolios in the packed weights' layout ([K][N4],
// behind the launch's packed block; an unwatched entry is +0), `watch` the 64-bit masks of the watched assets as [K][2] words (low,
// high).  Both, and the outputs, are read from the kernel arguments where they are used, as scalar loads.
struct BandArgs {
  const float* __restrict__ tol;      // [K][N4]
  const uint32_t* __restrict__ watch; // [K][2]: bit i of the mask is set iff i < N and tol[k][i] < +inf
  uint32_t* __restrict__ trades;      // [K][trades_stride] c
  uint64_t trades_stride;
  float* __restrict__ turnover;       // [K][turnover_stride] Y
  uint64_t turnover_stride;
};
// Arguments of mc_paths_band_kernel: those of mc_paths_reb_kernel (period: the review period) and the band block behind them.
struct PathArgsTB : PathArgsRB { BandArgs tb; };
typedef const __attribute__((address_space(4))) BandArgs* cband_p;
template <class A>
__device__ __forceinline__ cband_p band_args(const A&) {
  if constexpr (has_tb<A>::value) return &kernarg<A>()->tb;
  else return nullptr;
}

// Floor protection (SPEC.md 4.15): CPPI with an exposure cap and a drawdown ratchet.  Per path and portfolio the walk carries V and the
// peak M (both from v0); step t holds E = fmaxf(fminf(fl32(m (V - F)), fl32(b V)), +0) in the risky portfolio, F = fmaxf(S_t,
// fl32(theta M)), and V - E at the riskless rate: V' = fma(E, rho, fma(V - E, rf, V)).  `floor` is the schedule S_0 .. S_T behind the
// launch's packed block; S_t is wave-uniform and read inside the step, as the cash flow is.
struct ProtectArgs {
  const float* __restrict__ floor;    // [n_steps + 1] device copy
  float m, b, rf, theta;              // binary32: multiplier >= 0, cap > 0, riskless rate > -1, ratchet in [0, 1)
};
// Arguments of mc_paths_pi_kernel: the horizons of PathArgsHZ (n_horizons = 0: none), the drawdown output (written only when DD),
// then the draws' block -- nu and the GARCH constants (the GARCH walk, which also serves Gaussian and Student-t requests), or the
// jump block -- and the protection rule.
struct PathArgsPI : PathArgsHZ {
  float* __restrict__ mdd;
  uint64_t mdd_stride;
};
struct PathArgsPG : PathArgsPI { StudentArgs st; GarchArgs gv; ProtectArgs pi; };
struct PathArgsPJ : PathArgsPI { JumpArgs jp; ProtectArgs pi; };
// The protection block of a pi kernel's launch, read where it is used (kernarg).
typedef const __attribute__((address_space(4))) ProtectArgs* cprotect_p;
template <class A>
__device__ __forceinline__ cprotect_p protect_args(const A&) {
  if constexpr (has_pi<A>::value) return &kernarg<A>()->pi;
  else return nullptr;
}

// Volatility targeting (SPEC.md 4.19): per path and portfolio the walk carries V, the EWMA variance estimate s (from s0_k) and, without the
// drawdown, the summed exposure Y (from +0); step t holds E = fl32(e V), e = fminf(tgt / sqrtf(s), b), in the risky portfolio, V - E at the
// rate rf, pays sp on what it borrows, and ruin is absorbing as in SPEC.md 4.7.  `s0` sits behind the launch's packed block, one value per
// portfolio, padded to whole passes of 8.  The constants are wave-uniform and read inside the step, s0 once per tile, the output where it
// is written.
struct VolTargetArgs {
  float tgt, lam, oml, b, rf, sp;     // binary32: target, decay, fl32(1 - lam), cap > 0, rate > -1, spread >= 0
  const float* __restrict__ s0;       // [Kpad] device copy
  float* __restrict__ exposure;       // [K][exposure_stride] Y_T (written only without DD)
  uint64_t exposure_stride;
};
// Arguments of mc_paths_vt_kernel: those of mc_paths_pi_kernel with the targeting rule in place of the protection rule.
struct PathArgsVG : PathArgsPI { StudentArgs st; GarchArgs gv; VolTargetArgs vt; };
struct PathArgsVJ : PathArgsPI { JumpArgs jp; VolTargetArgs vt; };
// The targeting block of a vt kernel's launch, read where it is used (kernarg).
typedef const __attribute__((address_space(4))) VolTargetArgs* cvoltarget_p;
template <class A>
__device__ __forceinline__ cvoltarget_p vol_target_args(const A&) {
  if constexpr (has_vt<A>::value) return &kernarg<A>()->vt;
  else return nullptr;
}

// The time under water of SPEC.md 4.20: per path and portfolio the drawdown walk may carry two uint32 counters from 0 -- the current
// spell c, the steps since the value last stood at its running peak, and the longest spell m -- and store both next to V_T and q.  The
// outputs are read from the kernel arguments where they are written.
struct UnderwaterArgs {
  uint32_t* __restrict__ longest;     // [K][uw_stride] m
  uint32_t* __restrict__ current;     // [K][uw_stride] c_T
  uint64_t uw_stride;
};
// Arguments of the under-water twins: those of mc_paths_dd_kernel, mc_paths_g_dd_kernel and mc_paths_j_dd_kernel, and the counters'
// block behind them.
struct PathArgsUW : PathArgsDD { UnderwaterArgs uw; };
struct PathArgsGUW : PathArgsGDD { UnderwaterArgs uw; };
struct PathArgsJUW : PathArgsJDD { UnderwaterArgs uw; };
typedef const __attribute__((address_space(4))) UnderwaterArgs* cunderwater_p;
template <class A>
__device__ __forceinline__ cunderwater_p underwater_args(const A&) {
  if constexpr (has_uw<A>::value) return &kernarg<A>()->uw;
  else return nullptr;
}

// Drift uncertainty (SPEC.md 2.7 / 4.21): every path draws its own drift once, before step 0 -- nb Philox blocks on counter stream 5
// give g, and m_i = mu_i, then m_i = fma(M[i,j], g_j, m_i) for j = 0 .. i -- and every step of the path starts row i of its chain at
// m_i.  `factor` is M in the row-pair layout of the Cholesky factor (mcp_pack_params), behind the launch's packed block; it is read
// through the kernel arguments where it is used, by scalar loads, once per tile, and nothing of it is held across the walk.
struct DriftArgs {
  const float* __restrict__ factor;   // [N4 (N4/2 + 1)] device copy
};
// Arguments of the mc_paths_pu_* kernels: those of the plain, drawdown, horizon and cash-flow kernels and the drift block behind them.
struct PathArgsPU : PathArgs { DriftArgs pu; };
struct PathArgsPUDD : PathArgsDD { DriftArgs pu; };
struct PathArgsPUHZ : PathArgsHZ { DriftArgs pu; };
struct PathArgsPUCF : PathArgsCF { DriftArgs pu; };
template <class A>
__device__ __forceinline__ const __attribute__((address_space(4))) float* drift_factor(const A&) {
  typedef const __attribute__((address_space(4))) float* cfactor_p;
  if constexpr (has_pu<A>::value) return (cfactor_p)kernarg<A>()->pu.factor;
  else return nullptr;
}

// The option overlay of SPEC.md 4.8: per asset a run of rows (kind, strike, premium, qty) that turns the raw return r_i of a step
// into the strategy's return r'_i at the asset's price level P_i.  rows, row_begin [N4 + 1] (assets >= N own no rows) and spot [N4]
// are device copies; bit i of `mask` is set when asset i owns rows.
struct OverlayArgs {
  const mcp_overlay_row* __restrict__ rows;
  const int32_t* __restrict__ row_begin;
  const float* __restrict__ spot;
  uint64_t mask;
};
// Arguments of mc_paths_ov_kernel: the horizons of PathArgsHZ (n_horizons = 0: none), the drawdown output (written only when DD),
// nu (read only when STT) and the overlay.
struct PathArgsOV : PathArgsHZ {
  float* __restrict__ mdd;
  uint64_t mdd_stride;
  StudentArgs st;
  OverlayArgs ov;
};
// r'_i of SPEC.md 4.8 for an asset that owns the rows [rb, re): price = fma(prev, r, prev); num = fma(q_j, leg_j, num) over the
// rows in order from +0; r' = prev != 0 ? num / prev : +0 (IEEE division); P_i = price.  The loop over the rows is a run-time loop
// on wave-uniform bounds; every row is four scalar loads.
__device__ __forceinline__ float overlay_return(float r, float& P, int rb, int re) {
  typedef const __attribute__((address_space(4))) mcp_overlay_row* crow_p;
  const float prev = P;
  const float price = fma32(prev, r, prev);
  float num = 0.0f;
#pragma unroll 1
  for (int j = rb; j < re; j++) {
    const crow_p row = (crow_p)kernarg<PathArgsOV>()->ov.rows + j;
    const int32_t kind = row->kind;
    const float strike = row->strike, premium = row->premium, qty = row->qty;
    float leg;
    if (kind == MCP_OVERLAY_LINEAR) {
      leg = price - prev;
    } else {
      const float d = kind == MCP_OVERLAY_CALL ? price - strike : strike - price;
      leg = (d > 0.0f ? d : 0.0f) - premium;
    }
    num = fma32(qty, leg, num);
  }
  P = price;
  return prev != 0.0f ? num / prev : 0.0f;
}

// Everything a launch of a path kernel may carry: mcp_api.cpp fills it once per launch, and a block the request does not have
// stays zero.  make_args builds the argument struct A of one kernel from it by value: PathArgs, then the blocks A has.
struct PathLaunchArgs {
  PathArgsHZ hz;                      // PathArgs and the horizons (n_horizons = 0: none)
  float* mdd;                         // the drawdown output
  uint64_t mdd_stride;
  BootArgs bt;
  StudentArgs st;
  GarchArgs gv;
  CashArgs cf;
  OverlayArgs ov;
  AttrArgs at;
  int32_t period;                     // the rebalancing rule of PathArgsRB
  float cost;
  PairArgs pr;
  FiltArgs fh;
  JumpArgs jp;
  RegimeArgs rs;
  GlideArgs gp;
  ProtectArgs pi;
  SpendArgs sp;
  LifeArgs lf;
  BandArgs tb;
  VolTargetArgs vt;
  UnderwaterArgs uw;
  DriftArgs pu;
};
template <class A>
inline A make_args(const PathLaunchArgs& s) {
  A x;
  if constexpr (has_hz<A>::value) static_cast<PathArgsHZ&>(x) = s.hz;
  else static_cast<PathArgs&>(x) = s.hz;
  if constexpr (has_mdd<A>::value) { x.mdd = s.mdd; x.mdd_stride = s.mdd_stride; }
  if constexpr (has_bt<A>::value) x.bt = s.bt;
  if constexpr (has_st<A>::value) x.st = s.st;
  if constexpr (has_gv<A>::value) x.gv = s.gv;
  if constexpr (has_cf<A>::value) x.cf = s.cf;
  if constexpr (has_ov<A>::value) x.ov = s.ov;
  if constexpr (has_at<A>::value) x.at = s.at;
  if constexpr (has_period<A>::value) { x.period = s.period; x.cost = s.cost; }
  if constexpr (has_pr<A>::value) x.pr = s.pr;
  if constexpr (has_fh<A>::value) x.fh = s.fh;
  if constexpr (has_jp<A>::value) x.jp = s.jp;
  if constexpr (has_rs<A>::value) x.rs = s.rs;
  if constexpr (has_gp<A>::value) x.gp = s.gp;
  if constexpr (has_pi<A>::value) x.pi = s.pi;
  if constexpr (has_sp<A>::value) x.sp = s.sp;
  if constexpr (has_lf<A>::value) x.lf = s.lf;
  if constexpr (has_tb<A>::value) x.tb = s.tb;
  if constexpr (has_vt<A>::value) x.vt = s.vt;
  if constexpr (has_uw<A>::value) x.uw = s.uw;
  if constexpr (has_pu<A>::value) x.pu = s.pu;
  if constexpr (has_p_hi<A>::value) { x.p_hi = (uint32_t)(s.hz.path_begin >> 32); x.pad = 0u; }
  return x;
}

// (boot_fits_lds / filt_fits_lds, mcp_route.h: when the row table takes the LDS slot of the inverse-CDF table)
// LDS banking of the gather (ds_read_b128: 16 slots of 16 B, bank slot = float4 index mod 16).  Row j starts at slot
// (j NB) mod 16, a multiple of G = the largest power of two dividing NB, so a fixed chunk q of random rows would fall on only
// 16 / G slots.  Chunk q of row j is stored at j NB + (q ^ s(j)), s(j) = (j >> log2(16 / G)) & (G - 1): the bits of j that
// the row start does not already spread, XORed into the chunk index inside its aligned group of G (which stays inside the
// row since G divides NB).  A fixed q then spreads over all 16 slots.  No padding: the slot would outgrow the table's.
template <int NB>
struct BootSwizzle {
  static constexpr int G = (NB & -NB) > 16 ? 16 : (NB & -NB);
  static constexpr int SHIFT = G == 16 ? 0 : G == 8 ? 1 : G == 4 ? 2 : G == 2 ? 3 : 4;
  static constexpr uint32_t MASK = (uint32_t)G - 1u;
  __device__ static __forceinline__ uint32_t of(uint32_t j) { return MCP_EXP_BOOT_SWIZZLE ? (j >> SHIFT) & MASK : 0u; }
};

// h[digit] += 1 for the active lanes.  Terminal values cluster (V_T ~ 1 +- 0.2 hits a handful of digit-0 bins), and 64
// lanes on one LDS address serialise; so up to four distinct digits per wave are counted by ballot and added once.
// Every lane of the wave must call it (ballots inside).
__device__ __forceinline__ void lds_hist_add(uint32_t* h, uint32_t digit, bool active) {
  unsigned long long todo = __ballot(active);
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int it = 0; it < 4 && todo; it++) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)digit, leader);
    const bool same = active && digit == d0;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll(m));
    todo &= ~m;
    active = active && !same;
  }
  if (active) atomicAdd(&h[digit], 1u);
}

// x = V_T/V0 - 1 (simple) or expm1(S_T) (log); double, as the host computes it (mcp_terminal_to_x).
__device__ __forceinline__ double terminal_to_x(float term, double v0, int compounding) {
  return compounding == MCP_COMPOUND_LOG ? expm1((double)term) : (double)term / v0 - 1.0;
}

constexpr int PATH_BLOCK = 256;

// NB = N4/4 Philox blocks per path-step; KT portfolios per pass; PPT paths per lane; FOLD: rho = c + v.z with
// v = L^T w precomputed on the host (SPEC.md 4.1, one portfolio) instead of the triangular GEMV.
// LOGC: compounding mode at compile time (as a run-time flag the compiler if-converts the step into fma + add + select).
// DD: also track the running peak and the max drawdown of every (path, portfolio) through the step loop (SPEC.md 4.2) and
// store q (simple: min V_t/P_t) or d (log: min S_t - P_t) next to V_T.  HZ: also store V_h at the horizons (SPEC.md 4.3).
// BOOT: r is row j_t of the observed returns (SPEC.md 2.1 / 4.4) instead of mu + L z; BLDS: that table is read from LDS.
// REB: the step updates the assets' returns since the last rebalance B instead of V; V moves at the rebalance dates only
// (SPEC.md 4.5).  STT: every normal of the step is scaled by s = sqrt((nu - 2) / chi), chi the sum of nu squared normals of
// counter stream 2 (SPEC.md 2.2 / 4.6).  CF: the step's cash flow c_s is added to V after the update and ruin (V <= 0) is absorbing
// (SPEC.md 4.7).  OV: the step carries the price P_i of every asset and replaces r_i by the return r'_i of the asset's option rows before
// the weight dot (SPEC.md 4.8).  GV: the step's normals are scaled by u = sqrt(h) (STT: times s), h the path's GARCH(1,1) variance
// ratio, and h is updated from the scaled normals (SPEC.md 4.9); in a GV kernel STT is set and nu = 0 at run time means Gaussian
// draws.  AT: the step also carries every asset's contribution A_i = fma(V, fl32(w_i r_i), A_i) and the epilogue reduces them
// (SPEC.md 4.10 / 5.9).  FH (with BOOT): the row is a filtered residual, r_i = fma(sqrt(h), E_ji, mu_i), and h is updated from the
// row's shock, h = fminf(fma(b, h, fma(a, h s_j, omega)), 2^40) (SPEC.md 2.4 / 4.11).  ANTI: a lane walks the two members of an antithetic pair on one set of draws: everything up to the step's
// normals z (Philox, the transform, the chi blocks, h) runs once, everything downstream of z -- the row-pair accumulators, rho, V,
// the peak and drawdown, the stores and the epilogue -- carries a second member that sees -z (SPEC.md 2.3 / 5.10).  UHI: the high
// counter word p_hi is one value for the whole launch, a kernel argument: Philox rounds 1 and 2 run on the SALU where their operands
// are wave-uniform (philox4x32_10_uhi), the drift's LDS address and the transform's two scaling constants sit in VGPRs across the walk
// instead of being formed every step; the draws, and every result, are those of the kernel without it.  JP: before the asset normals one
// more Philox block on counter stream 3 gives the step's market jump J (SPEC.md 2.5), and every row pair's accumulator starts at
// fma(b, J, mu') instead of mu, one packed fma with the loadings b from the LDS slot behind the drift (SPEC.md 4.12).  RS: before the
// asset normals one more Philox block on counter stream 4 moves the path's regime (SPEC.md 2.6), and every row pair's chain runs once per
// regime under that regime's lanes -- a divergent if / else, skipped where the wave has no lane in the regime -- with that regime's
// drift and Cholesky factor, the factor still a scalar operand (SPEC.md 4.13).  GP (with CF and HZ): the
// walk's weight pointer moves to the next target block at the breaks of the glide path, wave-uniform events merged with the horizons
// as the rebalancing walk merges its dates; the step itself is the cash-flow kernel's (SPEC.md 4.14).  PI (with HZ): the walk also
// carries the peak M of V, and the update of V holds only the exposure E of the floor rule in the risky portfolio, the rest at the
// riskless rate (SPEC.md 4.15).  SP (with CF and HZ): the flow of the step is the path's own withdrawal w instead of the schedule's c_s,
// the walk also carries w and the total paid out Y, and the reviews of w are wave-uniform events merged with the horizons as the glide
// walk merges its breaks (SPEC.md 4.16).  LT (with CF): the step also counts, on the mask it already forms, the steps that stored a
// positive V -- the lifetime l of SPEC.md 4.17 -- and l is stored next to V_T.  TB (with REB, one portfolio): a rebalance date is a
// review, at which only the lanes with a watched asset out of its band trade; the walk also carries the trade count c and the turnover
// Y and stores them next to V_T (SPEC.md 4.18).  VT (with HZ): the walk also carries the variance estimate s and, without DD, the summed
// exposure Y; the update of V holds the exposure e = fminf(tgt / sqrtf(s), b) in the risky portfolio, the rest at the riskless rate, what
// is borrowed at the spread on top, ruin absorbing; s then moves on the step's rho (SPEC.md 4.19).  UW (with DD): behind the update of the
// peak the step also counts the current spell below it and keeps the longest, one compare against the peak just written, one add, one
// select and one integer max per path and portfolio; both counters are stored next to V_T (SPEC.md 4.20).  PU: before step 0 every path
// draws its own drift m = mu + M g from nb Philox blocks on counter stream 5 and holds it in N4 registers across the walk; every step's
// row pair starts from the path's m pair instead of the launch's drift, and nothing else in the step changes (SPEC.md 2.7 / 4.21).  Every kernel
// below is the body in mcp_paths_body.inc under its own flags F: it names the flags it sets, the rest are PathFlagsOff's.  F is a
// local class, which may not have static data members, so it sets its flags as enumerators of an `enum : bool`; they hide the
// defaults' names and read as the same constant expressions.
struct PathFlagsOff {
  static constexpr bool NATIVE = false, FOLD = false, LOGC = false, DD = false, HZ = false, BOOT = false, BLDS = false, REB = false,
                        STT = false, CF = false, OV = false, GV = false, AT = false, ANTI = false, FH = false, UHI = false, JP = false, RS = false,
                        GP = false, PI = false, SP = false, LT = false, TB = false, VT = false, UW = false, PU = false;
};

// __launch_bounds__ 2nd argument of a path kernel: the MCP_MIN_WAVES* above for N <= 16 and one path per lane, by the kind of
// state the kernel carries; MCP_MIN_WAVES_BIG for 16 < N <= 64 and one portfolio; otherwise unbounded.
enum BoundsKind { BK_PATHS, BK_REB, BK_CF, BK_OV, BK_AT, BK_ANTI, BK_PI, BK_SP, BK_UW, BK_UWJ, BK_PU };
constexpr int min_waves(BoundsKind kind, int NB, int KT, int PPT) {
  if (kind == BK_PU)                          // the kernels that hold the path's own drift, N4 registers on top of their twins'
    return (NB <= 4 && PPT == 1) ? (KT == 1 ? MCP_MIN_WAVES_PU : MCP_MIN_WAVES_PU8) : (KT == 1 && PPT == 1) ? MCP_MIN_WAVES_BIG : 1;
  if (kind == BK_UW || kind == BK_UWJ) {      // the under-water twins (simple compounding); BK_UWJ: on the jump walk, which from N = 5 on
                                              // takes the protection kernel's 5 waves (at 6 the N = 16 kernel had scratch in its step loop)
    if (NB <= 4 && PPT == 1 && KT == 1) return (kind == BK_UWJ && NB >= 2) ? MCP_MIN_WAVES_PI : MCP_MIN_WAVES;
    if (NB <= 4 && PPT == 1) return MCP_MIN_WAVES_UW8;
    return (KT == 1 && PPT == 1) ? MCP_MIN_WAVES_BIG : 1;
  }
  if (kind == BK_SP) return (NB <= 4 && PPT == 1) ? (KT == 1 ? MCP_MIN_WAVES_SP : MCP_MIN_WAVES_SP8) : (KT == 1 && PPT == 1) ? MCP_MIN_WAVES_BIG : 1;
  if (kind == BK_ANTI) return (NB <= 4 && PPT == 1 && KT == 1) ? MCP_MIN_WAVES_ANTI : 1;
  if (NB <= 4 && PPT == 1 && KT == 1)
    return kind == BK_REB ? MCP_MIN_WAVES_REB : kind == BK_OV ? MCP_MIN_WAVES_OV : kind == BK_AT ? MCP_MIN_WAVES_AT
           : kind == BK_PI ? MCP_MIN_WAVES_PI : MCP_MIN_WAVES;
  if (NB <= 4 && PPT == 1 && kind != BK_PATHS && kind != BK_AT && kind != BK_PI)
    return kind == BK_REB ? MCP_MIN_WAVES_REB8 : kind == BK_CF ? MCP_MIN_WAVES_CF8 : MCP_MIN_WAVES_OV8;
  return (KT == 1 && PPT == 1) ? MCP_MIN_WAVES_BIG : 1;
}
#define MCP_BOUNDS(kind) __launch_bounds__(PATH_BLOCK, min_waves(kind, NB, KT, PPT))

template <int NB, int KT, int PPT, bool NATIVE_, bool FOLD_ = false, bool LOGC_ = false>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_kernel(const PathArgs a) {
  struct F : PathFlagsOff { enum : bool { NATIVE = NATIVE_, FOLD = FOLD_, LOGC = LOGC_ }; };
#include "mcp_paths_body.inc"
}

// The lean Gaussian kernel: mc_paths_kernel<NB, 1, 1, false, false, LOGC> for a launch whose paths share the high counter word
// (UHI above) -- the same walk, terminal values and fused epilogue bit for bit, with the step loop's wave-uniform work taken off
// the VALU.  A launch whose path range crosses a multiple of 2^32 stays on mc_paths_kernel.
template <int NB, bool LOGC_>
__global__ void __launch_bounds__(PATH_BLOCK, min_waves(BK_PATHS, NB, 1, 1)) mc_paths_lean_kernel(const PathArgsLean a) {
  constexpr int KT = 1, PPT = 1;
  struct F : PathFlagsOff { enum : bool { LOGC = LOGC_, UHI = true }; };
#include "mcp_paths_body.inc"
}

// The drawdown kernel (SPEC.md 4.2; spec normals, unfolded recurrence only).  Its arguments are PathArgs plus the drawdown
// array: appended to PathArgs itself they would move the hidden kernel arguments (grid size) of every plain kernel.
template <int NB, int KT, int PPT, bool LOGC_>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_dd_kernel(const PathArgsDD a) {
  struct F : PathFlagsOff { enum : bool { DD = true, LOGC = LOGC_ }; };
#include "mcp_paths_body.inc"
}

// The horizon kernel (SPEC.md 4.3; spec normals, unfolded recurrence only): the walk of mc_paths_kernel in segments that end
// at the horizons, V_h stored after each; V_T and the fused epilogue as in mc_paths_kernel.
template <int NB, int KT, int PPT, bool LOGC_>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_hz_kernel(const PathArgsHZ a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, LOGC = LOGC_ }; };
#include "mcp_paths_body.inc"
}

// The bootstrap kernel (SPEC.md 2.1 / 4.4): the walk of mc_paths_kernel on resampled rows of observed returns, one Philox
// block per path-step for the row index, no normals, no Cholesky GEMV.  V_T and the fused epilogue as in mc_paths_kernel.
template <int NB, int KT, int PPT, bool LOGC_, bool BLDS_>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_boot_kernel(const PathArgsBT a) {
  struct F : PathFlagsOff { enum : bool { BOOT = true, LOGC = LOGC_, BLDS = BLDS_ }; };
#include "mcp_paths_body.inc"
}

// The bootstrap kernel with the horizons of SPEC.md 4.3 (the segmented walk of mc_paths_hz_kernel).
template <int NB, int KT, int PPT, bool LOGC_, bool BLDS_>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_boot_hz_kernel(const PathArgsBTHZ a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, BOOT = true, LOGC = LOGC_, BLDS = BLDS_ }; };
#include "mcp_paths_body.inc"
}
// The rebalancing kernel (SPEC.md 4.5; simple compounding, Gaussian draws or, BOOT, the bootstrap's rows): the walk in segments
// that end at the events -- rebalance dates, horizons, T -- where V^ = V (1 + W.B) is marked.  H = 0 is one segment, so one
// kernel serves terminal-only and horizon calls.  V_T and the fused epilogue as in mc_paths_kernel.
template <int NB, int KT, int PPT, bool BOOT_, bool BLDS_>
__global__ void MCP_BOUNDS(BK_REB) mc_paths_reb_kernel(const PathArgsRB a) {
  struct F : PathFlagsOff { enum : bool { REB = true, BOOT = BOOT_, BLDS = BLDS_ }; };
#include "mcp_paths_body.inc"
}

// The tolerance-band kernel (SPEC.md 4.18): mc_paths_reb_kernel's walk with the trade of a date decided per path.  The returns B since
// a path's last trade belong to one portfolio -- under section 4.5 every portfolio of a pass trades on the same dates and shares them,
// under bands each trades on its own -- so there is no 8-portfolio instance: K portfolios run as K passes of this kernel, K walks of
// the draws.  It keeps the rebalancing kernel's launch bounds: c, Y and the hit mask fit the 96 VGPRs of 5 waves, and no listing
// shows scratch in a loop over t (profiles/band_isa.txt).
template <int NB, int KT, int PPT, bool BOOT_, bool BLDS_>
__global__ void MCP_BOUNDS(BK_REB) mc_paths_band_kernel(const PathArgsTB a) {
  struct F : PathFlagsOff { enum : bool { REB = true, TB = true, BOOT = BOOT_, BLDS = BLDS_ }; };
#include "mcp_paths_body.inc"
}

// The Student-t kernels (SPEC.md 2.2 / 4.6; simple compounding, unfolded recurrence): mc_paths_kernel, mc_paths_dd_kernel and
// mc_paths_hz_kernel with every step's normals scaled by the step's s.  V_T, the drawdown, the horizons and the fused epilogue as
// there.
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_t_kernel(const PathArgsT a) {
  struct F : PathFlagsOff { enum : bool { STT = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_t_dd_kernel(const PathArgsTDD a) {
  struct F : PathFlagsOff { enum : bool { DD = true, STT = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_t_hz_kernel(const PathArgsTHZ a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, STT = true }; };
#include "mcp_paths_body.inc"
}

// The GARCH kernels (SPEC.md 4.9; simple compounding, unfolded recurrence; Gaussian draws, or Student-t draws when the launch
// carries nu != 0, a wave-uniform branch around the chi blocks): mc_paths_kernel, mc_paths_dd_kernel and mc_paths_hz_kernel with
// every step's normals scaled by u = sqrt(h) (times the step's s), h the path's variance ratio, updated from the step's shock.
// V_T, the drawdown, the horizons and the fused epilogue as there.  They keep the plain kernel's launch bounds: no listing shows
// scratch in a step loop (profiles/garch_isa.txt).
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_g_kernel(const PathArgsG a) {
  struct F : PathFlagsOff { enum : bool { STT = true, GV = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_g_dd_kernel(const PathArgsGDD a) {
  struct F : PathFlagsOff { enum : bool { DD = true, STT = true, GV = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_g_hz_kernel(const PathArgsGHZ a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, STT = true, GV = true }; };
#include "mcp_paths_body.inc"
}

// The jump-diffusion kernels (SPEC.md 2.5 / 4.12; simple compounding, unfolded recurrence, Gaussian draws): mc_paths_kernel,
// mc_paths_dd_kernel and mc_paths_hz_kernel with the step's market jump added to every asset through its loading.  V_T, the
// drawdown, the horizons and the fused epilogue as there.  They keep the plain kernel's launch bounds: no listing shows scratch in
// a step loop (profiles/jump_isa.txt).
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_j_kernel(const PathArgsJ a) {
  struct F : PathFlagsOff { enum : bool { JP = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_j_dd_kernel(const PathArgsJDD a) {
  struct F : PathFlagsOff { enum : bool { JP = true, DD = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_j_hz_kernel(const PathArgsJHZ a) {
  struct F : PathFlagsOff { enum : bool { JP = true, HZ = true }; };
#include "mcp_paths_body.inc"
}

// The regime-switching kernels (SPEC.md 2.6 / 4.13; simple compounding, unfolded recurrence, Gaussian draws): mc_paths_kernel,
// mc_paths_dd_kernel and mc_paths_hz_kernel with one regime in {0, 1} per path, step t on the drift and factor of the path's regime.
// V_T, the drawdown, the horizons and the fused epilogue as there.  They keep the plain kernel's launch bounds
// (profiles/regime_isa.txt).
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_r_kernel(const PathArgsR a) {
  struct F : PathFlagsOff { enum : bool { RS = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_r_dd_kernel(const PathArgsRDD a) {
  struct F : PathFlagsOff { enum : bool { RS = true, DD = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_r_hz_kernel(const PathArgsRHZ a) {
  struct F : PathFlagsOff { enum : bool { RS = true, HZ = true }; };
#include "mcp_paths_body.inc"
}

// The cash-flow kernel (SPEC.md 4.7; simple compounding, unfolded recurrence; Gaussian draws, BOOT: the bootstrap's rows, STT:
// Student-t draws): the segmented walk of mc_paths_hz_kernel with U = fma(V, rho, V) + c_s after every step and V = U while both
// V and U are positive, +0 from then on.  H = 0 is one segment, so one kernel serves terminal-only and horizon calls.  V_T, the
// horizons and the fused epilogue as in mc_paths_hz_kernel.
template <int NB, int KT, int PPT, bool BOOT_, bool BLDS_, bool STT_>
__global__ void MCP_BOUNDS(BK_CF) mc_paths_cf_kernel(const PathArgsCF a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, CF = true, BOOT = BOOT_, BLDS = BLDS_, STT = STT_ }; };
#include "mcp_paths_body.inc"
}

// The glide-path kernel (SPEC.md 4.14): mc_paths_cf_kernel with the weights of the dot taken from the target block of the step's
// segment.  The segmented walk ends a segment at the next horizon, the next break or T; at a break the scalar weight pointer moves
// on, at a horizon V is stored, both when they share a step.  G = 0 is the cash-flow kernel's walk.  It keeps that kernel's launch
// bounds: the step loop is its twin's and no listing shows scratch in it (profiles/glide_isa.txt).
template <int NB, int KT, int PPT, bool BOOT_, bool BLDS_, bool STT_>
__global__ void MCP_BOUNDS(BK_CF) mc_paths_glide_kernel(const PathArgsGP a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, CF = true, GP = true, BOOT = BOOT_, BLDS = BLDS_, STT = STT_ }; };
#include "mcp_paths_body.inc"
}

// The spending kernel (SPEC.md 4.16): mc_paths_cf_kernel with the path's own withdrawal in place of the schedule.  The segmented walk
// ends a segment at the next horizon, the next review or T; at a horizon V is stored, at a review w moves, the store first when they
// share a step.  every = 0 is the cash-flow kernel's walk on c_s = -w0.  V_T keeps the fused epilogue; Y_T is stored next to it and
// reduced by the non-fused passes.  Launch bounds of its own: the kernel carries 2 KT registers more than its twin
// (profiles/spend_isa.txt).
template <int NB, int KT, int PPT, bool BOOT_, bool BLDS_, bool STT_>
__global__ void MCP_BOUNDS(BK_SP) mc_paths_spend_kernel(const PathArgsSP a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, CF = true, SP = true, BOOT = BOOT_, BLDS = BLDS_, STT = STT_ }; };
#include "mcp_paths_body.inc"
}

// The lifetime twins (SPEC.md 4.17): mc_paths_glide_kernel and mc_paths_spend_kernel with the counter l carried next to V and stored
// next to V_T; everything else those kernels compute is theirs bit for bit.  G = 0 on the glide twin is the cash-flow walk, so a plain
// cash-flow request with a lifetime runs there and has no third set of instances.  Both keep their originals' launch bounds: the KT
// counters fit -- the 8-portfolio glide twin at N <= 16 takes the 96 VGPRs of its 5 waves where the original takes 93; unbounded it took
// 103 (4 waves) and 76 more VALU per step -- and no listing shows scratch in a loop over t (profiles/lifetime_isa.txt).
template <int NB, int KT, int PPT, bool BOOT_, bool BLDS_, bool STT_>
__global__ void MCP_BOUNDS(BK_CF) mc_paths_glide_life_kernel(const PathArgsGPL a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, CF = true, GP = true, LT = true, BOOT = BOOT_, BLDS = BLDS_, STT = STT_ }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT, bool BOOT_, bool BLDS_, bool STT_>
__global__ void MCP_BOUNDS(BK_SP) mc_paths_spend_life_kernel(const PathArgsSPL a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, CF = true, SP = true, LT = true, BOOT = BOOT_, BLDS = BLDS_, STT = STT_ }; };
#include "mcp_paths_body.inc"
}

// The floor-protection kernel (SPEC.md 4.15; simple compounding, unfolded recurrence): the segmented walk of mc_paths_hz_kernel with
// the CPPI / ratchet rule in the update of V.  H = 0 is one segment, so one kernel serves terminal-only and horizon calls; DD adds
// the drawdown state of mc_paths_dd_kernel, which sees the protected V.  JP_ = false: the GARCH walk, which serves Gaussian (nu = 0,
// alpha = beta = 0, h0 = 1) and Student-t requests at run time as mc_paths_attr_kernel does; JP_ = true: the jump walk.  V_T, the
// horizons, the drawdown and the fused epilogue as in those kernels.  On the GARCH walk it keeps the plain kernel's launch bounds, on
// the jump walk it takes MCP_MIN_WAVES_PI: so no listing shows scratch in a step loop (profiles/protect_isa.txt).
template <int NB, int KT, int PPT, bool JP_, bool DD_>
__global__ void MCP_BOUNDS(JP_ ? BK_PI : BK_PATHS) mc_paths_pi_kernel(const std::conditional_t<JP_, PathArgsPJ, PathArgsPG> a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, PI = true, DD = DD_, STT = !JP_, GV = !JP_, JP = JP_ }; };
#include "mcp_paths_body.inc"
}

// The volatility-targeting kernel (SPEC.md 4.19; simple compounding, unfolded recurrence): mc_paths_pi_kernel's walks -- the segmented
// GARCH walk (JP_ = false: Gaussian, Student-t and GARCH requests) or jump walk (JP_ = true), H = 0 one segment, DD the drawdown state,
// which sees the targeted V -- with the targeting rule in the update of V.  Per portfolio of the pass one IEEE square root and one IEEE
// division per step.  V_T, the horizons, the drawdown and the fused epilogue as in those kernels; without DD the summed exposure Y is
// stored next to V_T and reduced by the non-fused passes.  It takes the protection kernel's launch bounds (profiles/voltarget_isa.txt).
template <int NB, int KT, int PPT, bool JP_, bool DD_>
__global__ void MCP_BOUNDS(JP_ ? BK_PI : BK_PATHS) mc_paths_vt_kernel(const std::conditional_t<JP_, PathArgsVJ, PathArgsVG> a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, VT = true, DD = DD_, STT = !JP_, GV = !JP_, JP = JP_ }; };
#include "mcp_paths_body.inc"
}

// The under-water twins (SPEC.md 4.20): mc_paths_dd_kernel (simple or log compounding), mc_paths_g_dd_kernel (the GARCH walk, which
// also serves Student-t requests: alpha = beta = 0, h0 = 1) and mc_paths_j_dd_kernel with the two counters c and m carried next to the
// peak and stored next to V_T and q; everything else those kernels compute is theirs bit for bit.  Launch bounds: their originals',
// but for N <= 16 the jump twin of one portfolio takes 5 waves from N = 5 on (one fewer than mc_paths_j_dd_kernel: at 6 its step loop
// at N = 16 held a scratch access) and the 8-portfolio twins under simple compounding are held at their parents' 4 (MCP_MIN_WAVES_UW8).
// What the 2 KT counters cost in registers and occupancy is listed in profiles/underwater_isa.txt; no listing shows scratch in a
// step loop.
template <int NB, int KT, int PPT, bool LOGC_>
__global__ void MCP_BOUNDS(LOGC_ ? BK_PATHS : BK_UW) mc_paths_uw_kernel(const PathArgsUW a) {
  struct F : PathFlagsOff { enum : bool { DD = true, UW = true, LOGC = LOGC_ }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_UW) mc_paths_g_uw_kernel(const PathArgsGUW a) {
  struct F : PathFlagsOff { enum : bool { DD = true, UW = true, STT = true, GV = true }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_UWJ) mc_paths_j_uw_kernel(const PathArgsJUW a) {
  struct F : PathFlagsOff { enum : bool { DD = true, UW = true, JP = true }; };
#include "mcp_paths_body.inc"
}

// The drift-uncertainty kernels (SPEC.md 2.7 / 4.21; spec normals, unfolded recurrence, Gaussian draws): mc_paths_kernel,
// mc_paths_dd_kernel and mc_paths_hz_kernel (simple or log compounding) and mc_paths_cf_kernel on Gaussian draws, each with the drift
// of every path drawn once inside the tile loop and held in N4 registers: the step's row pairs start from it, so the drift is not
// read from LDS.  V_T, the drawdown, the horizons, ruin and the fused epilogue as in those kernels; with M = 0 their stored values bit
// for bit.  Launch bounds of their own (MCP_MIN_WAVES_PU, MCP_MIN_WAVES_PU8): no listing shows scratch in a loop over t
// (profiles/uncertain_isa.txt).
template <int NB, int KT, int PPT, bool LOGC_>
__global__ void MCP_BOUNDS(BK_PU) mc_paths_pu_kernel(const PathArgsPU a) {
  struct F : PathFlagsOff { enum : bool { PU = true, LOGC = LOGC_ }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT, bool LOGC_>
__global__ void MCP_BOUNDS(BK_PU) mc_paths_pu_dd_kernel(const PathArgsPUDD a) {
  struct F : PathFlagsOff { enum : bool { PU = true, DD = true, LOGC = LOGC_ }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT, bool LOGC_>
__global__ void MCP_BOUNDS(BK_PU) mc_paths_pu_hz_kernel(const PathArgsPUHZ a) {
  struct F : PathFlagsOff { enum : bool { PU = true, HZ = true, LOGC = LOGC_ }; };
#include "mcp_paths_body.inc"
}
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_PU) mc_paths_pu_cf_kernel(const PathArgsPUCF a) {
  struct F : PathFlagsOff { enum : bool { PU = true, HZ = true, CF = true }; };
#include "mcp_paths_body.inc"
}

// The filtered-historical-simulation kernel (SPEC.md 2.4 / 4.11; simple compounding): the segmented walk of mc_paths_boot_hz_kernel
// on the residual rows, every row scaled by sqrt(h) and added to the drift, h updated from the row's shock.  H = 0 is one segment, so
// one kernel serves terminal-only and horizon calls.  V_T, the horizons and the fused epilogue as in mc_paths_boot_hz_kernel.
template <int NB, int KT, int PPT, bool BLDS_>
__global__ void MCP_BOUNDS(BK_PATHS) mc_paths_fhs_kernel(const PathArgsFH a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, BOOT = true, BLDS = BLDS_, FH = true }; };
#include "mcp_paths_body.inc"
}

// The overlay kernel (SPEC.md 4.8; simple compounding, unfolded recurrence; Gaussian draws, STT: Student-t draws): the segmented
// walk of mc_paths_hz_kernel with every asset's return replaced by its option rows' return at the price level the kernel carries.
// H = 0 is one segment, so one kernel serves terminal-only and horizon calls; DD adds the drawdown state of mc_paths_dd_kernel.
// V_T, the horizons, the drawdown and the fused epilogue as in those kernels.
template <int NB, int KT, int PPT, bool STT_, bool DD_>
__global__ void MCP_BOUNDS(BK_OV) mc_paths_ov_kernel(const PathArgsOV a) {
  struct F : PathFlagsOff { enum : bool { HZ = true, OV = true, STT = STT_, DD = DD_ }; };
#include "mcp_paths_body.inc"
}

// The attribution kernel (SPEC.md 4.10 / 5.9; simple compounding, unfolded recurrence, one portfolio per pass): the walk of
// mc_paths_g_kernel again -- the same draws and the same V, Gaussian (nu = 0, alpha = beta = 0, h0 = 1), Student-t or GARCH -- with
// the contribution A_i of every asset carried next to V: per pair of assets one packed multiply (w r) and one packed fma (V
// broadcast).  No terminal store and no fused statistics epilogue; its own epilogue reduces A, A over the tail x <= var and
// A (x - c) to one record per workgroup, in a fixed order, and stores A when asked to.
template <int NB, int KT, int PPT>
__global__ void MCP_BOUNDS(BK_AT) mc_paths_attr_kernel(const PathArgsAT a) {
  static_assert(KT == 1, "one portfolio per pass");
  struct F : PathFlagsOff { enum : bool { STT = true, GV = true, AT = true }; };
#include "mcp_paths_body.inc"
}

// The antithetic kernels (SPEC.md 2.3 / 5.10; spec normals, unfolded recurrence): one lane walks the pair (2j, 2j + 1) -- member 2j
// is path j of the call without pairs, member 2j + 1 the same walk on -z.  The argument struct A selects the walk: PathArgsA,
// PathArgsADD, PathArgsAHZ are mc_paths_kernel, mc_paths_dd_kernel and mc_paths_hz_kernel (simple or log compounding), PathArgsGA,
// PathArgsGADD, PathArgsGAHZ their GARCH twins, which also serve Student-t and GARCH-free requests at run time as
// mc_paths_attr_kernel does.  V_T, the drawdown, the horizons and the fused epilogue as there, over both members; the epilogue
// also leaves the pair cross products.
template <int NB, int KT, int PPT, bool LOGC_, class A>
__global__ void MCP_BOUNDS(BK_ANTI) mc_paths_anti_kernel(const A a) {
  static_assert(!(LOGC_ && has_gv<A>::value), "GARCH and Student-t paths compound simply");
  struct F : PathFlagsOff {
    enum : bool { ANTI = true, LOGC = LOGC_, DD = has_mdd<A>::value, HZ = has_hz<A>::value, STT = has_gv<A>::value, GV = has_gv<A>::value };
  };
#include "mcp_paths_body.inc"
}
#undef MCP_BOUNDS

}  // namespace mcp

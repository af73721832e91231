// mcp_api.cpp -- the C ABI of libmcport.so (include/mcport.h): argument checking, parameter packing,
// enqueue-only launch entry points, and the host-level mcp_simulate() that strings them together on
// one device.  No torch types, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mcport.h"
#include "../../include/mcport_protect.h"
#include "mcp_device.h"
#include "mcp_paths.h"
#include "mcp_stats_kernels.h"

#ifndef MCP_EXP_LEAN        // 1: launches that pass mcp::lean_range run mc_paths_lean_kernel; 0: every launch stays on mc_paths_kernel
#define MCP_EXP_LEAN 1      // (tools/kernel_lab.py arms `lean` and `nolean`; profiles/lean_probe.json)
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(MCP_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

constexpr int KT_WIDE = 8;           // portfolios per pass of the KT=8 kernel
constexpr int K_PAD = 512;           // W rows are zero-padded to a multiple of this (MFMA sweep tile: 32*MT)
using mcp::SWEEP_MIN_K;              // from this many portfolios on the MFMA sweep kernels run

// MCP_SWEEP_MT: 0 (default) = automatic tile count, 1/2/4 = force the per-wave kernel with that many 32-portfolio tiles,
// -1 = no MFMA kernels at all (K > 16 then runs as passes of the 8-portfolio kernel)
int env_sweep_mt() {
  static const int v = [] { const char* e = getenv("MCP_SWEEP_MT"); return e ? atoi(e) : 0; }();
  return v;
}
// does a launch for K portfolios go to the MFMA sweep kernels?  (decides the MomentPartial slot count)
bool uses_sweep(int K) { return K >= SWEEP_MIN_K && env_sweep_mt() >= 0; }

// How a sweep of K portfolios is cut into launches.  Two kernel families, both bit-identical to the oracle:
//   shared-draw (mc_sweep_shared_kernel): the four waves of a workgroup share one draw and own 128 MT portfolios;
//                MT = 4 | 2 for N <= 16 (512 | 256 portfolios), MT = 2 | 1 for 16 < N <= 64 (256 | 128)
//   per-wave    (mc_sweep_kernel, N <= 16): every wave draws for itself and owns 32 MT portfolios, MT = 1 | 2 | 4
// Whole big shared workgroups first; the remainder r goes to the smallest tiling that covers it:
//   N <= 16:  r <= 128 per-wave (32 / 64 / 128)   r <= 256 shared MT 2   r <= 384 shared MT 2 + per-wave   else shared MT 4
//   N  > 16:  r <= 128 shared MT 1                 else shared MT 2
// (K = 1,250 per GPU when configs[4] is sharded over 8: 2 x 512 + 226 -> one 256-portfolio workgroup row instead of a third 512.)
struct SweepSeg { bool shared; int mt, k_begin, k_count; };
int sweep_plan(int K, int nb, SweepSeg* out) {
  int n = 0;
  const int env_mt = env_sweep_mt();
  if (nb <= 4 && env_mt > 0) {                       // forced: per-wave kernel with that many tiles for everything
    out[n++] = {false, env_mt, 0, K};
    return n;
  }
  const int big = nb <= 4 ? 4 : 2, W = 128 * big;
  const int full = (K / W) * W;
  if (full) out[n++] = {true, big, 0, full};
  const int r = K - full;
  if (r == 0) return n;
  if (nb <= 4) {
    const auto per_wave = [](int k) { return k > 64 ? 4 : (k > 32 ? 2 : 1); };
    if (r <= 128) out[n++] = {false, per_wave(r), full, r};
    else if (r <= 256) out[n++] = {true, 2, full, r};
    else if (r <= 384) { out[n++] = {true, 2, full, 256}; out[n++] = {false, per_wave(r - 256), full + 256, r - 256}; }
    else out[n++] = {true, 4, full, r};
  } else {
    out[n++] = {true, r <= 128 ? 1 : 2, full, r};
  }
  return n;
}

inline int n4_of(int n) { return 4 * ((n + 3) / 4); }
// floats of the regime-1 block [mu1 N4][L1 row pairs N4(N4/2+1)] (SPEC.md 4.13)
inline size_t regime_block_len(int n) { const size_t n4 = (size_t)n4_of(n); return n4 + n4 * (n4 / 2 + 1); }
// W rows are zero-padded to whole MFMA workgroups for a sweep, to whole KT_WIDE passes otherwise
inline int kpad_of(int k) { return k >= SWEEP_MIN_K ? K_PAD * ((k + K_PAD - 1) / K_PAD) : KT_WIDE * ((k + KT_WIDE - 1) / KT_WIDE); }

int check_params(const mcp_params* p) {
  if (!p) return fail(MCP_E_ARG, "params is NULL");
  if (p->n_assets < 1 || p->n_assets > MCP_MAX_ASSETS)
    return fail(MCP_E_ARG, "n_assets=%d outside [1,%d]", p->n_assets, MCP_MAX_ASSETS);
  if (p->n_steps < 0) return fail(MCP_E_ARG, "n_steps=%d < 0", p->n_steps);
  if (p->n_portfolios < 1) return fail(MCP_E_ARG, "n_portfolios=%d < 1", p->n_portfolios);
  if (p->compounding != MCP_COMPOUND_SIMPLE && p->compounding != MCP_COMPOUND_LOG)
    return fail(MCP_E_ARG, "compounding=%d unknown", p->compounding);
  if (!(p->alpha > 0.0 && p->alpha < 1.0)) return fail(MCP_E_ARG, "alpha=%g outside (0,1)", p->alpha);
  if (!(p->v0 > 0.0) || !std::isfinite(p->v0)) return fail(MCP_E_ARG, "v0=%g must be positive", p->v0);
  return MCP_OK;
}

const mcp::launch_paths_fn k_launch[16] = {
    mcp::launch_paths_nb1,  mcp::launch_paths_nb2,  mcp::launch_paths_nb3,  mcp::launch_paths_nb4,
    mcp::launch_paths_nb5,  mcp::launch_paths_nb6,  mcp::launch_paths_nb7,  mcp::launch_paths_nb8,
    mcp::launch_paths_nb9,  mcp::launch_paths_nb10, mcp::launch_paths_nb11, mcp::launch_paths_nb12,
    mcp::launch_paths_nb13, mcp::launch_paths_nb14, mcp::launch_paths_nb15, mcp::launch_paths_nb16};

// SPEC.md 4.3: 1..MCP_MAX_HORIZONS strictly increasing steps in [1, n_steps]
int check_horizons(int n_steps, int H, const int32_t* steps) {
  if (H < 1 || H > MCP_MAX_HORIZONS) return fail(MCP_E_ARG, "n_horizons=%d outside [1,%d]", H, MCP_MAX_HORIZONS);
  if (!steps) return fail(MCP_E_ARG, "horizons is NULL");
  for (int i = 0; i < H; i++) {
    if (steps[i] < 1 || steps[i] > n_steps) return fail(MCP_E_ARG, "horizon %d = %d outside [1, n_steps=%d]", i, steps[i], n_steps);
    if (i && steps[i] <= steps[i - 1]) return fail(MCP_E_ARG, "horizons must be strictly increasing (%d after %d)", steps[i], steps[i - 1]);
  }
  return MCP_OK;
}

// SPEC.md 5.2: 0..MCP_MAX_LEVELS percentages in [0, 100]
int check_levels(int L, const double* levels) {
  if (L < 0 || L > MCP_MAX_LEVELS) return fail(MCP_E_ARG, "n_levels=%d outside [0,%d]", L, MCP_MAX_LEVELS);
  if (L && !levels) return fail(MCP_E_ARG, "levels is NULL");
  for (int i = 0; i < L; i++)
    if (!(levels[i] >= 0.0 && levels[i] <= 100.0)) return fail(MCP_E_ARG, "level %d = %g outside [0, 100]", i, levels[i]);
  return MCP_OK;
}

// SPEC.md 2.1: the bootstrap request -- 1..MCP_MAX_BOOT_ROWS rows of n_assets finite binary32 values, 1 <= b <= +inf
int check_boot(const mcp_params* prm, const mcp_bootstrap* boot) {
  if (!boot) return fail(MCP_E_ARG, "bootstrap is NULL");
  if (!boot->rows) return fail(MCP_E_ARG, "bootstrap rows is NULL");
  if (boot->n_rows < 1 || boot->n_rows > MCP_MAX_BOOT_ROWS)
    return fail(MCP_E_ARG, "n_rows=%d outside [1,%d]", boot->n_rows, MCP_MAX_BOOT_ROWS);
  const double b = boot->mean_block;
  if (!(b >= 1.0)) return fail(MCP_E_ARG, "mean_block=%g must be >= 1 (or +inf)", b);
  const size_t n = (size_t)boot->n_rows * (size_t)prm->n_assets;
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(boot->rows[i]))
      return fail(MCP_E_ARG, "bootstrap row %zu, asset %zu is not finite", i / (size_t)prm->n_assets, i % (size_t)prm->n_assets);
  return MCP_OK;
}

// SPEC.md 2.1: the restart threshold thr = b == +inf ? 0 : min(2^32, floor(fl64(2^32 / b)))
uint64_t boot_threshold(double b) {
  const double q = 4294967296.0 / b;                   // fl64(2^32 / b); 0 for b = +inf
  return q >= 4294967296.0 ? (uint64_t)1 << 32 : (uint64_t)q;
}

// SPEC.md 5.3: per portfolio the mean m and variance s2 (population) of rho_j = sum_i w_i rows[j,i] over the R rows, binary64.
void boot_moments(int N, const mcp_bootstrap* boot, const float* W, int K, double* m_out, double* s2_out) {
  const int R = boot->n_rows;
  std::vector<double> rho((size_t)R);
  for (int k = 0; k < K; k++) {
    const float* w = W + (size_t)k * N;
    double sum = 0.0;
    for (int j = 0; j < R; j++) {
      const float* r = boot->rows + (size_t)j * N;
      double v = 0.0;
      for (int i = 0; i < N; i++) v += (double)w[i] * (double)r[i];
      rho[(size_t)j] = v;
      sum += v;
    }
    const double m = sum / (double)R;
    double ss = 0.0;
    for (int j = 0; j < R; j++) { const double d = rho[(size_t)j] - m; ss += d * d; }
    m_out[k] = m;
    s2_out[k] = ss / (double)R;
  }
}

// SPEC.md 5.3: the pivot at T steps from the row moments
double boot_pivot(int compounding, int T, double m, double s2) {
  const double c = compounding == MCP_COMPOUND_LOG ? std::expm1((double)T * (m + 0.5 * s2))
                                                   : (m > -1.0 ? std::expm1((double)T * std::log1p(m)) : 0.0);
  return std::isfinite(c) ? c : 0.0;
}

// SPEC.md 4.5: period >= 0, reserved == 0, cost in [0, 1) (not NaN)
int check_reb(const mcp_rebalance* reb) {
  if (!reb) return fail(MCP_E_ARG, "rebalance is NULL");
  if (reb->period < 0) return fail(MCP_E_ARG, "rebalance period=%d < 0", reb->period);
  if (reb->reserved != 0) return fail(MCP_E_ARG, "rebalance reserved=%d must be 0", reb->reserved);
  if (!(reb->cost >= 0.0 && reb->cost < 1.0)) return fail(MCP_E_ARG, "rebalance cost=%g outside [0, 1)", reb->cost);
  return MCP_OK;
}

// SPEC.md 2.2: 3 <= nu <= MCP_MAX_T_DOF, reserved == 0, (uint64)T ceil(nu/4) < 2^32 (the counter of stream 2)
int check_student_t(const mcp_params* prm, const mcp_student_t* st) {
  if (!st) return fail(MCP_E_ARG, "student_t is NULL");
  if (st->dof < 3 || st->dof > MCP_MAX_T_DOF) return fail(MCP_E_ARG, "dof=%d outside [3,%d]", st->dof, MCP_MAX_T_DOF);
  if (st->reserved != 0) return fail(MCP_E_ARG, "student_t reserved=%d must be 0", st->reserved);
  if ((uint64_t)prm->n_steps * (uint64_t)((st->dof + 3) / 4) > 0xFFFFFFFFull)
    return fail(MCP_E_ARG, "n_steps * ceil(dof/4) = %llu exceeds the 32-bit Philox block counter of stream 2",
                (unsigned long long)((uint64_t)prm->n_steps * (uint64_t)((st->dof + 3) / 4)));
  return MCP_OK;
}

// SPEC.md 4.9: the binary32 constants of a GARCH request -- a = fl32(alpha), b = fl32(beta), g = fl32(h0), omega = fl32(1 - a - b)
// and a_N = fl32(a / N), the last two from binary64 arithmetic on a and b
struct GarchConsts { float a, b, g, omega, a_n; };
GarchConsts garch_consts(const mcp_garch* g, int N) {
  GarchConsts c;
  c.a = (float)g->alpha;
  c.b = (float)g->beta;
  c.g = (float)g->h0;
  c.omega = (float)(1.0 - (double)c.a - (double)c.b);
  c.a_n = (float)((double)c.a / (double)N);
  return c;
}

// SPEC.md 4.9: alpha, beta, h0 finite; a >= 0, b >= 0, a + b < 1 (binary64 sum of the rounded values), omega > 0, g > 0; reserved == 0
int check_garch(const mcp_params* prm, const mcp_garch* g) {
  if (!g) return fail(MCP_E_ARG, "garch is NULL");
  if (g->reserved != 0) return fail(MCP_E_ARG, "garch reserved=%llu must be 0", (unsigned long long)g->reserved);
  if (!std::isfinite(g->alpha) || !std::isfinite(g->beta) || !std::isfinite(g->h0))
    return fail(MCP_E_ARG, "garch alpha=%g, beta=%g, h0=%g must be finite", g->alpha, g->beta, g->h0);
  const GarchConsts c = garch_consts(g, prm->n_assets);
  if (!std::isfinite(c.a) || !std::isfinite(c.b) || !std::isfinite(c.g))
    return fail(MCP_E_ARG, "garch alpha=%g, beta=%g, h0=%g must be finite in binary32", g->alpha, g->beta, g->h0);
  if (!(c.a >= 0.0f) || !(c.b >= 0.0f)) return fail(MCP_E_ARG, "garch alpha=%g and beta=%g must be >= 0", g->alpha, g->beta);
  if (!((double)c.a + (double)c.b < 1.0) || !(c.omega > 0.0f))
    return fail(MCP_E_ARG, "garch alpha + beta = %.9g must be < 1 in binary32", (double)c.a + (double)c.b);
  if (!(c.g > 0.0f)) return fail(MCP_E_ARG, "garch h0=%g must be > 0 in binary32", g->h0);
  return MCP_OK;
}

// SPEC.md 2.5: the host constants of a jump request, binary64 in the spec's order -- thr[k-1] = clamp(floor((1 - cum_k) 2^32), 0,
// 2^32 - 1) with cum_k the Poisson(lambda) mass below k, E = sum_k thr_k / 2^32 (the exact mean of the truncated count the kernel
// draws), m = fl32(mean), s = fl32(std)
struct JumpConsts { uint32_t thr[MCP_MAX_JUMPS]; double mean_count; float m, s; };
JumpConsts jump_consts(const mcp_jumps* j) {
  JumpConsts c;
  double p = std::exp(-j->intensity), cum = 0.0;
  c.mean_count = 0.0;
  for (int k = 1; k <= MCP_MAX_JUMPS; k++) {
    cum = cum + p;
    double v = std::floor((1.0 - cum) * 4294967296.0);
    v = v < 0.0 ? 0.0 : v > 4294967295.0 ? 4294967295.0 : v;
    c.thr[k - 1] = (uint32_t)v;
    c.mean_count += (double)c.thr[k - 1] / 4294967296.0;
    p = p * j->intensity / (double)k;
  }
  c.m = (float)j->mean;
  c.s = (float)j->std;
  return c;
}
// SPEC.md 2.5: the compensated drift mu'_i = (d == 0 or b_i == 0) ? mu_i : fl32(mu_i - b_i d), d = (double)m E: E[r] stays mu
void jump_drift(const mcp_jumps* j, const JumpConsts& c, int N, const float* mu, float* out) {
  const double d = (double)c.m * c.mean_count;
  for (int i = 0; i < N; i++) {
    const float b = j->loading ? j->loading[i] : 1.0f;
    out[i] = (d == 0.0 || b == 0.0f) ? mu[i] : (float)((double)mu[i] - (double)b * d);
  }
}

// SPEC.md 2.5: intensity, mean, std and the loadings finite, before and after rounding to binary32; 0 <= intensity <= 1; std >= 0;
// reserved == 0
int check_jumps(int n_assets, const mcp_jumps* j) {
  if (!j) return fail(MCP_E_ARG, "jumps is NULL");
  if (j->reserved != 0) return fail(MCP_E_ARG, "jumps reserved=%d must be 0", j->reserved);
  if (!std::isfinite(j->intensity) || !std::isfinite(j->mean) || !std::isfinite(j->std))
    return fail(MCP_E_ARG, "jumps intensity=%g, mean=%g, std=%g must be finite", j->intensity, j->mean, j->std);
  if (!std::isfinite((float)j->intensity) || !std::isfinite((float)j->mean) || !std::isfinite((float)j->std))
    return fail(MCP_E_ARG, "jumps intensity=%g, mean=%g, std=%g must be finite in binary32", j->intensity, j->mean, j->std);
  if (!(j->intensity >= 0.0 && j->intensity <= 1.0)) return fail(MCP_E_ARG, "jumps intensity=%g outside [0, 1]", j->intensity);
  if (!(j->std >= 0.0)) return fail(MCP_E_ARG, "jumps std=%g must be >= 0", j->std);
  for (int i = 0; j->loading && i < n_assets; i++)
    if (!std::isfinite(j->loading[i])) return fail(MCP_E_ARG, "jumps loading, asset %d is not finite", i);
  return MCP_OK;
}

// SPEC.md 2.6: the host constants of a regime request, binary64 -- thr_x = min(2^32, floor(p_x 2^32)) (the product an exact scaling)
// and the probabilities the kernel really uses, p^_x = thr_x / 2^32, for x = 01, 10, start
struct RegimeConsts { uint64_t thr01, thr10, thr_start; double p01, p10, start; };
inline uint64_t regime_thr(double p) {
  const double v = std::floor(p * 4294967296.0);
  return v >= 4294967296.0 ? (uint64_t)1 << 32 : (uint64_t)v;
}
RegimeConsts regime_consts(const mcp_regimes* r) {
  RegimeConsts c;
  c.thr01 = regime_thr(r->p01);
  c.thr10 = regime_thr(r->p10);
  c.thr_start = regime_thr(r->start);
  c.p01 = (double)c.thr01 / 4294967296.0;
  c.p10 = (double)c.thr10 / 4294967296.0;
  c.start = (double)c.thr_start / 4294967296.0;
  return c;
}

// SPEC.md 2.6: the three probabilities finite and in [0, 1], mu1 [N] and chol1 [N][N] not NULL and finite, reserved == 0
int check_regimes(int n_assets, const mcp_regimes* r) {
  if (!r) return fail(MCP_E_ARG, "regimes is NULL");
  if (r->reserved != 0) return fail(MCP_E_ARG, "regimes reserved=%d must be 0", r->reserved);
  if (!std::isfinite(r->p01) || !std::isfinite(r->p10) || !std::isfinite(r->start))
    return fail(MCP_E_ARG, "regimes p01=%g, p10=%g, start=%g must be finite", r->p01, r->p10, r->start);
  if (!(r->p01 >= 0.0 && r->p01 <= 1.0) || !(r->p10 >= 0.0 && r->p10 <= 1.0) || !(r->start >= 0.0 && r->start <= 1.0))
    return fail(MCP_E_ARG, "regimes p01=%g, p10=%g, start=%g outside [0, 1]", r->p01, r->p10, r->start);
  if (!r->mu1 || !r->chol1) return fail(MCP_E_ARG, "regimes mu1 or chol1 is NULL");
  for (int i = 0; i < n_assets; i++)
    if (!std::isfinite(r->mu1[i])) return fail(MCP_E_ARG, "regimes mu1, asset %d is not finite", i);
  for (size_t i = 0; i < (size_t)n_assets * n_assets; i++)
    if (!std::isfinite(r->chol1[i])) return fail(MCP_E_ARG, "regimes chol1, entry %zu is not finite", i);
  return MCP_OK;
}

// SPEC.md 5.13: the exact mean of x after h steps, c_k(h) = pi' D_k (P^ D_k)^(h-1) 1 - 1 with d_ks = 1 + sum_i W[k,i] mu^(s)_i (i
// ascending, binary64 from the binary32 inputs), as one row-vector recursion over h = 1 .. T: v = pi D, then v = (v P^) D;
// out_T[k] = c_k(T), out_hz[h*K + k] = c_k(steps[h]); 0 for h = 0 and where c is not finite.  Where the walk of portfolio k has one
// drift only -- m_k0 == m_k1, or the chain never leaves the regime it starts in (p^start = 0 and p^01 = 0: regime 0; p^start = 1 and
// p^10 = 0: regime 1) -- c_k(h) is mcp_pivots' own expm1(h log1p(m)) on that drift, the same mean in the Gaussian call's rounding, so
// that such a call has the Gaussian call's statistics bit for bit.
void regime_pivots(int N, int K, int T, const float* mu0, const float* mu1, const RegimeConsts& c, const float* W, int H, const int32_t* steps,
                   double* out_T, double* out_hz) {
  for (int k = 0; k < K; k++) {
    const float* w = W + (size_t)k * N;
    double d0 = 0.0, d1 = 0.0;
    for (int i = 0; i < N; i++) d0 += (double)w[i] * (double)(mu0[i] + 0.0f);
    for (int i = 0; i < N; i++) d1 += (double)w[i] * (double)(mu1[i] + 0.0f);
    const bool only0 = c.thr_start == 0 && c.thr01 == 0, only1 = c.thr_start == ((uint64_t)1 << 32) && c.thr10 == 0;
    const bool one_drift = d0 == d1 || only0 || only1;
    const double m = only1 ? d1 : d0;
    d0 = 1.0 + d0;
    d1 = 1.0 + d1;
    double v0 = (1.0 - c.start) * d0, v1 = c.start * d1;
    int hi = 0;
    if (out_T) out_T[k] = 0.0;
    for (int h = 1; h <= T; h++) {
      if (h > 1) {
        const double u0 = v0 * (1.0 - c.p01) + v1 * c.p10, u1 = v0 * c.p01 + v1 * (1.0 - c.p10);
        v0 = u0 * d0;
        v1 = u1 * d1;
      }
      const double ch = one_drift ? (m > -1.0 ? std::expm1((double)h * std::log1p(m)) : 0.0) : (v0 + v1) - 1.0;
      const double piv = std::isfinite(ch) ? ch : 0.0;
      if (hi < H && steps[hi] == h) out_hz[(size_t)hi++ * K + k] = piv;
      if (h == T && out_T) out_T[k] = piv;
    }
  }
}

// SPEC.md 2.4: the filtered rows -- mu [N], resid [R][N] and shock [R] finite binary32 values, every shock >= 0, 1..MCP_MAX_BOOT_ROWS
// rows, 1 <= b <= +inf, reserved == 0
int check_filtered(const mcp_params* prm, const mcp_filtered* f) {
  if (!f) return fail(MCP_E_ARG, "filtered is NULL");
  if (!f->mu) return fail(MCP_E_ARG, "filtered mu is NULL");
  if (!f->resid) return fail(MCP_E_ARG, "filtered resid is NULL");
  if (!f->shock) return fail(MCP_E_ARG, "filtered shock is NULL");
  if (f->n_rows < 1 || f->n_rows > MCP_MAX_BOOT_ROWS) return fail(MCP_E_ARG, "filtered n_rows=%d outside [1,%d]", f->n_rows, MCP_MAX_BOOT_ROWS);
  if (f->reserved != 0) return fail(MCP_E_ARG, "filtered reserved=%d must be 0", f->reserved);
  if (!(f->mean_block >= 1.0)) return fail(MCP_E_ARG, "filtered mean_block=%g must be >= 1 (or +inf)", f->mean_block);
  const size_t N = (size_t)prm->n_assets, R = (size_t)f->n_rows;
  for (size_t i = 0; i < N; i++)
    if (!std::isfinite(f->mu[i])) return fail(MCP_E_ARG, "filtered mu, asset %zu is not finite", i);
  for (size_t i = 0; i < R * N; i++)
    if (!std::isfinite(f->resid[i])) return fail(MCP_E_ARG, "filtered resid row %zu, asset %zu is not finite", i / N, i % N);
  for (size_t j = 0; j < R; j++) {
    if (!std::isfinite(f->shock[j])) return fail(MCP_E_ARG, "filtered shock, row %zu is not finite", j);
    if (!(f->shock[j] >= 0.0f)) return fail(MCP_E_ARG, "filtered shock, row %zu = %g is negative", j, (double)f->shock[j]);
  }
  return MCP_OK;
}

// SPEC.md 5.11: mu_i + e_i of the pivot of filtered paths, binary64 -- e_i the mean of column i of the residual rows, j ascending
void filt_means(int N, const mcp_filtered* f, double* out) {
  for (int i = 0; i < N; i++) {
    double sum = 0.0;
    for (int j = 0; j < f->n_rows; j++) sum += (double)f->resid[(size_t)j * N + i];
    out[i] = (double)f->mu[i] + sum / (double)f->n_rows;
  }
}

// SPEC.md 5.11: m_k = sum_i W[k,i] (mu_i + e_i) (i ascending), c_k = expm1(T log1p(m_k)), 0 if m_k <= -1 or not finite
void filt_pivots(int N, int K, int T, const double* me, const float* W, double* out) {
  for (int k = 0; k < K; k++) {
    const float* w = W + (size_t)k * N;
    double m = 0.0;
    for (int i = 0; i < N; i++) m += (double)w[i] * me[i];
    const double c = m > -1.0 ? std::expm1((double)T * std::log1p(m)) : 0.0;
    out[k] = std::isfinite(c) ? c : 0.0;
  }
}

// SPEC.md 4.7: n_flows == n_steps finite flows, has_target 0 / 1 with a finite target, fl32(v0) > 0
int check_cashflow(const mcp_params* prm, const mcp_cashflow* cf) {
  if (!cf) return fail(MCP_E_ARG, "cashflow is NULL");
  if (cf->n_flows != prm->n_steps) return fail(MCP_E_ARG, "n_flows=%d must equal n_steps=%d", cf->n_flows, prm->n_steps);
  if (prm->n_steps > 0 && !cf->flows) return fail(MCP_E_ARG, "cashflow flows is NULL");
  for (int s = 0; s < cf->n_flows; s++)
    if (!std::isfinite(cf->flows[s])) return fail(MCP_E_ARG, "cash flow %d is not finite", s + 1);
  if (cf->has_target != 0 && cf->has_target != 1) return fail(MCP_E_ARG, "has_target=%d must be 0 or 1", cf->has_target);
  if (cf->has_target && !std::isfinite(cf->target)) return fail(MCP_E_ARG, "target=%g is not finite", cf->target);
  if (!((float)prm->v0 > 0.0f)) return fail(MCP_E_ARG, "v0=%g rounds to zero in binary32", prm->v0);
  return MCP_OK;
}

// SPEC.md 4.14: 0..MCP_MAX_GLIDE strictly increasing breaks in [1, n_steps - 1], n_breaks blocks of [K][N] finite targets, reserved == 0
int check_glide(const mcp_params* prm, const mcp_glide* gl) {
  if (!gl) return fail(MCP_E_ARG, "glide is NULL");
  if (gl->reserved != 0) return fail(MCP_E_ARG, "glide reserved=%d must be 0", gl->reserved);
  if (gl->n_breaks < 0 || gl->n_breaks > MCP_MAX_GLIDE) return fail(MCP_E_ARG, "n_breaks=%d outside [0,%d]", gl->n_breaks, MCP_MAX_GLIDE);
  if (gl->n_breaks > 0 && (!gl->breaks || !gl->targets)) return fail(MCP_E_ARG, "glide breaks or targets is NULL");
  for (int g = 0; g < gl->n_breaks; g++) {
    if (gl->breaks[g] < 1 || gl->breaks[g] > prm->n_steps - 1)
      return fail(MCP_E_ARG, "glide break %d = %d outside [1, n_steps - 1 = %d]", g, gl->breaks[g], prm->n_steps - 1);
    if (g && gl->breaks[g] <= gl->breaks[g - 1])
      return fail(MCP_E_ARG, "glide breaks must be strictly increasing (%d after %d)", gl->breaks[g], gl->breaks[g - 1]);
  }
  const size_t KN = (size_t)prm->n_portfolios * (size_t)prm->n_assets;
  for (size_t i = 0; i < (size_t)gl->n_breaks * KN; i++)
    if (!std::isfinite(gl->targets[i]))
      return fail(MCP_E_ARG, "glide target %zu, portfolio %zu, asset %zu is not finite", i / KN + 1, i % KN / (size_t)prm->n_assets,
                  i % (size_t)prm->n_assets);
  return MCP_OK;
}

// SPEC.md 4.14: the device copy of the target blocks of the portfolios [k0, k0 + kt) -- per block glide_rows(kt) rows of N4 floats, the
// packed weights' layout with the rows padded to whole passes of 8 (the glide kernels run no MFMA sweep)
inline size_t glide_rows(int kt) { return (size_t)KT_WIDE * (size_t)((kt + KT_WIDE - 1) / KT_WIDE); }
inline size_t glide_len(int N, int kt, const mcp_glide* gl) { return (size_t)gl->n_breaks * glide_rows(kt) * (size_t)n4_of(N); }
void glide_pack(int N, int K, int k0, int kt, const mcp_glide* gl, float* out) {
  const size_t n4 = (size_t)n4_of(N), blk = glide_rows(kt) * n4;
  std::fill(out, out + (size_t)gl->n_breaks * blk, 0.0f);
  for (int g = 0; g < gl->n_breaks; g++)
    for (int k = 0; k < kt; k++)
      memcpy(out + (size_t)g * blk + (size_t)k * n4, gl->targets + ((size_t)g * K + (size_t)(k0 + k)) * N, (size_t)N * sizeof(float));
}

// SPEC.md 4.15: the binary32 constants of a protection request
struct ProtectConsts { float m, b, rf, theta; };
ProtectConsts protect_consts(const mcp_protect* pt) {
  return ProtectConsts{(float)pt->multiplier, (float)pt->cap, (float)pt->rate, (float)pt->ratchet};
}
// SPEC.md 4.15: a finite floor >= +0 at every step 0 .. n_steps; multiplier >= 0, cap > 0, rate > -1, ratchet in [0, 1), each finite
// before and after rounding to binary32 and inside its range after it; a finite target; reserved == 0
int check_protect(const mcp_params* prm, const mcp_protect* pt) {
  if (!pt) return fail(MCP_E_ARG, "protect is NULL");
  if (pt->reserved != 0) return fail(MCP_E_ARG, "protect reserved=%d must be 0", pt->reserved);
  if (!pt->floor) return fail(MCP_E_ARG, "protect floor is NULL");
  const double v[4] = {pt->multiplier, pt->cap, pt->rate, pt->ratchet};
  for (int i = 0; i < 4; i++)
    if (!std::isfinite(v[i]) || !std::isfinite((float)v[i]))
      return fail(MCP_E_ARG, "protect multiplier=%g, cap=%g, rate=%g, ratchet=%g must be finite, also in binary32", v[0], v[1], v[2], v[3]);
  const ProtectConsts c = protect_consts(pt);
  if (!(pt->multiplier >= 0.0)) return fail(MCP_E_ARG, "protect multiplier=%g must be >= 0", pt->multiplier);
  if (!(pt->cap > 0.0) || !(c.b > 0.0f)) return fail(MCP_E_ARG, "protect cap=%g must be > 0 in binary32", pt->cap);
  if (!(pt->rate > -1.0) || !(c.rf > -1.0f)) return fail(MCP_E_ARG, "protect rate=%g must be > -1 in binary32", pt->rate);
  if (!(pt->ratchet >= 0.0 && pt->ratchet < 1.0) || !(c.theta < 1.0f))
    return fail(MCP_E_ARG, "protect ratchet=%g outside [0, 1) in binary32", pt->ratchet);
  if (pt->target && (!std::isfinite(*pt->target) || !std::isfinite((float)*pt->target)))
    return fail(MCP_E_ARG, "protect target=%g must be finite, also in binary32", *pt->target);
  for (int t = 0; t <= prm->n_steps; t++)
    if (!std::isfinite(pt->floor[t]) || !(pt->floor[t] >= 0.0f))
      return fail(MCP_E_ARG, "protect floor, step %d = %g must be finite and >= 0", t, (double)pt->floor[t]);
  if (!((float)prm->v0 > 0.0f)) return fail(MCP_E_ARG, "v0=%g rounds to zero in binary32", prm->v0);
  return MCP_OK;
}
// What follows the packed block (and the jump loadings) of a protected launch: the schedule S_0 .. S_T, then per stored row -- the kt
// terminal rows, then the H*kt horizon rows -- the two thresholds {S_h, target or -inf} of the counts (SPEC.md 5.15)
inline size_t protect_len(int T, int kt, int H) { return (size_t)T + 1 + 2 * (size_t)kt * (size_t)(1 + H); }
void protect_pack(int T, int kt, int H, const int32_t* steps, const mcp_protect* pt, float* out) {
  memcpy(out, pt->floor, ((size_t)T + 1) * sizeof(float));
  float* thr = out + T + 1;
  const float tg = pt->target ? (float)*pt->target : -HUGE_VALF;
  for (int h = -1; h < H; h++)
    for (int k = 0; k < kt; k++) {
      *thr++ = pt->floor[h < 0 ? T : steps[h]];
      *thr++ = tg;
    }
}

// SPEC.md 4.8: row_begin ascending from 0 to n_rows, at most MCP_MAX_OVERLAY_ROWS rows per asset, kinds 0..2, finite numbers, a
// positive spot on every asset that owns rows, reserved == 0
int check_overlay(const mcp_params* prm, const mcp_overlay* ov) {
  if (!ov) return fail(MCP_E_ARG, "overlay is NULL");
  if (ov->reserved != 0) return fail(MCP_E_ARG, "overlay reserved=%d must be 0", ov->reserved);
  const int N = prm->n_assets;
  if (ov->n_rows < 0 || ov->n_rows > N * MCP_MAX_OVERLAY_ROWS)
    return fail(MCP_E_ARG, "overlay n_rows=%d outside [0,%d]", ov->n_rows, N * MCP_MAX_OVERLAY_ROWS);
  if (!ov->row_begin || !ov->spot || (ov->n_rows > 0 && !ov->rows)) return fail(MCP_E_ARG, "overlay rows, row_begin or spot is NULL");
  if (ov->row_begin[0] != 0 || ov->row_begin[N] != ov->n_rows)
    return fail(MCP_E_ARG, "overlay row_begin must run from 0 to n_rows=%d (got %d .. %d)", ov->n_rows, ov->row_begin[0], ov->row_begin[N]);
  for (int i = 0; i < N; i++) {
    const int cnt = ov->row_begin[i + 1] - ov->row_begin[i];
    if (cnt < 0) return fail(MCP_E_ARG, "overlay row_begin is not ascending at asset %d", i);
    if (cnt > MCP_MAX_OVERLAY_ROWS) return fail(MCP_E_ARG, "asset %d owns %d overlay rows, at most %d", i, cnt, MCP_MAX_OVERLAY_ROWS);
    if (!std::isfinite(ov->spot[i])) return fail(MCP_E_ARG, "spot of asset %d is not finite", i);
    if (cnt > 0 && !(ov->spot[i] > 0.0f)) return fail(MCP_E_ARG, "spot of asset %d = %g must be positive (it owns overlay rows)", i, ov->spot[i]);
  }
  for (int j = 0; j < ov->n_rows; j++) {
    const mcp_overlay_row& r = ov->rows[j];
    if (r.kind < MCP_OVERLAY_LINEAR || r.kind > MCP_OVERLAY_PUT) return fail(MCP_E_ARG, "overlay row %d: kind=%d outside 0..2", j, r.kind);
    if (!std::isfinite(r.strike) || !std::isfinite(r.premium) || !std::isfinite(r.qty))
      return fail(MCP_E_ARG, "overlay row %d: strike, premium or qty is not finite", j);
  }
  return MCP_OK;
}

// SPEC.md 5.7: the rule of SPEC.md 4.8 in binary64 on the deterministic prices P_i,t = P_i,t-1 (1 + mu_i) from spot_i; the return of
// an asset without rows is mu_i.  rho_k,t = sum_i W[k,i] r'_i,t (i ascending), A_k,t = A_k,t-1 (1 + rho_k,t) from 1; the pivot
// A - 1 (0 where not finite) after step T into out_T[k] and after the steps of the H horizons into out_hz[h*K + k].
void overlay_pivots(int N, int K, int T, const mcp_overlay* ov, const float* mu, const float* W, int H, const int32_t* steps,
                    double* out_T, double* out_hz) {
  const auto pivot = [](double A) {
    const double c = A - 1.0;
    return std::isfinite(c) ? c : 0.0;
  };
  std::vector<double> P((size_t)N), g((size_t)N), r((size_t)N), A((size_t)K, 1.0);
  for (int i = 0; i < N; i++) {
    P[(size_t)i] = (double)ov->spot[i];
    r[(size_t)i] = (double)(mu[i] + 0.0f);
    g[(size_t)i] = 1.0 + r[(size_t)i];
  }
  int hi = 0;
  for (int t = 1; t <= T; t++) {
    for (int i = 0; i < N; i++) {
      const int rb = ov->row_begin[i], re = ov->row_begin[i + 1];
      if (rb == re) continue;
      const double prev = P[(size_t)i], price = prev * g[(size_t)i];
      double num = 0.0;
      for (int j = rb; j < re; j++) {
        const mcp_overlay_row& row = ov->rows[j];
        double leg;
        if (row.kind == MCP_OVERLAY_LINEAR) {
          leg = price - prev;
        } else {
          const double d = row.kind == MCP_OVERLAY_CALL ? price - (double)row.strike : (double)row.strike - price;
          leg = (d > 0.0 ? d : 0.0) - (double)row.premium;
        }
        num = num + (double)row.qty * leg;
      }
      r[(size_t)i] = prev != 0.0 ? num / prev : 0.0;
      P[(size_t)i] = price;
    }
    for (int k = 0; k < K; k++) {
      const float* w = W + (size_t)k * N;
      double rho = 0.0;
      for (int i = 0; i < N; i++) rho += (double)w[i] * r[(size_t)i];
      A[(size_t)k] = A[(size_t)k] * (1.0 + rho);
    }
    if (hi < H && steps[hi] == t) {
      for (int k = 0; k < K; k++) out_hz[(size_t)hi * K + k] = pivot(A[(size_t)k]);
      hi++;
    }
  }
  for (int k = 0; k < K; k++) out_T[k] = pivot(A[(size_t)k]);
}

// SPEC.md 4.8: the device copy of an overlay -- [rows n_rows][row_begin N4 + 1][spot N4]; the assets >= N own no rows
size_t overlay_bytes(int N, int n_rows) { return (size_t)n_rows * sizeof(mcp_overlay_row) + (size_t)(2 * n4_of(N) + 1) * 4; }
void overlay_pack(int N, const mcp_overlay* ov, char* out) {
  const int n4 = n4_of(N);
  if (ov->n_rows) memcpy(out, ov->rows, (size_t)ov->n_rows * sizeof(mcp_overlay_row));
  int32_t* rb = (int32_t*)(out + (size_t)ov->n_rows * sizeof(mcp_overlay_row));
  float* sp = (float*)(rb + n4 + 1);
  for (int i = 0; i <= n4; i++) rb[i] = i <= N ? ov->row_begin[i] : ov->n_rows;
  for (int i = 0; i < n4; i++) sp[i] = i < N ? ov->spot[i] : 1.0f;
}

// The draws of a walk (SPEC.md 2): Gaussian steps mu + L z, rows of the bootstrap, Student-t steps mu + L s z, or filtered residual
// rows scaled by the path's GARCH variance ratio (SPEC.md 2.4).
enum Source { SRC_GAUSS, SRC_BOOT, SRC_T, SRC_FHS };

// What one call asks of the walk: the draw source, optionally a rebalancing rule, the drawdown or horizons, and the host arrays
// of an mcp_simulate* call (an mcp_launch_paths* call gives its device arrays in a Launch instead).
struct Request {
  Source src = SRC_GAUSS;
  const float* mu = nullptr;            // SRC_GAUSS, SRC_T: the drift and the Cholesky factor
  const float* chol = nullptr;
  const mcp_bootstrap* boot = nullptr;  // SRC_BOOT (SPEC.md 2.1)
  const mcp_student_t* st = nullptr;    // SRC_T (SPEC.md 2.2)
  const mcp_filtered* filt = nullptr;   // SRC_FHS (SPEC.md 2.4): the rows, with the triple of SPEC.md 4.9 in `gv` (`garch` stays false)
  bool rebalanced = false;              // SPEC.md 4.5: the rule `reb`
  const mcp_rebalance* reb = nullptr;
  bool cash = false;                    // SPEC.md 4.7: the schedule `cf`
  const mcp_cashflow* cf = nullptr;
  bool glide = false;                   // SPEC.md 4.14: the weight schedule `gl`, always with `cf` (mcp_simulate_glide)
  const mcp_glide* gl = nullptr;
  bool protect = false;                 // SPEC.md 4.15: the floor rule `pi` (mcp_simulate_protected)
  const mcp_protect* pi = nullptr;
  bool overlay = false;                 // SPEC.md 4.8: the option rows `ov`
  const mcp_overlay* ov = nullptr;
  bool garch = false;                   // SPEC.md 4.9: the variance recurrence `gv` (SRC_GAUSS or SRC_T)
  const mcp_garch* gv = nullptr;
  bool jumps = false;                   // SPEC.md 2.5 / 4.12: the market jump `jp` on top of SRC_GAUSS
  const mcp_jumps* jp = nullptr;
  bool regimes = false;                 // SPEC.md 2.6 / 4.13: two regimes `rs`, regime 0 on (mu, chol), on top of SRC_GAUSS
  const mcp_regimes* rs = nullptr;
  bool dd = false;                      // SPEC.md 4.2 / 5.1: the drawdown of every path
  bool hz = false;                      // SPEC.md 4.3 / 5.2: the values after H steps, statistics at alpha and at L levels
  int H = 0, L = 0;
  const int32_t* steps = nullptr;
  const double* levels = nullptr;
  const float* W = nullptr;             // [K][N]
  float* terminal_out = nullptr;        // outputs; the optional ones NULL when not asked for
  mcp_stats* stats_out = nullptr;
  float* mdd_out = nullptr;
  mcp_stats* dd_stats_out = nullptr;
  float* hz_out = nullptr;              // [H*K*n], row h*K + k
  mcp_stats* hz_stats_out = nullptr;    // [H*K]
  double* bands_out = nullptr;          // [H*K*L]
  uint64_t* counts_out = nullptr;       // cash flows: [K][2] {n_ruined, n_short} (SPEC.md 5.6); protection: {n_gap, n_short} (5.15)
  uint64_t* hz_counts_out = nullptr;    // [H*K][2]
  bool attr = false;                    // SPEC.md 4.10 / 5.9: the second walk that attributes the risk to the assets
  float* contrib_out = nullptr;         // NULL or host [K][N][n]
  mcp_attr* attr_out = nullptr;         // [K][N]
  uint64_t* attr_counts_out = nullptr;  // [K][2] {n, n_tail}
  bool anti = false;                    // SPEC.md 2.3 / 5.10: antithetic pairs
  mcp_pair* pair_out = nullptr;         // [K]
  double* cross_out = nullptr;          // [K] the call's cross sums: every tile adds its shards' in shard order
};

// The row table of a request that walks rows: the bootstrap's own, or the residual rows of SRC_FHS.
mcp_bootstrap rows_of(const Request& rq) {
  if (rq.src == SRC_FHS) return mcp_bootstrap{rq.filt->resid, rq.filt->n_rows, 0, rq.filt->mean_block};
  return *rq.boot;
}

Request host_request(Source src, const float* mu, const float* chol, const float* W, float* terminal_out, mcp_stats* stats_out) {
  Request rq;
  rq.src = src;
  rq.mu = mu;
  rq.chol = chol;
  rq.W = W;
  rq.terminal_out = terminal_out;
  rq.stats_out = stats_out;
  return rq;
}

void ask_horizons(Request& rq, bool on, int H, const int32_t* steps, int L, const double* levels, float* out, mcp_stats* stats,
                  double* bands) {
  rq.hz = on;
  rq.H = H;
  rq.steps = steps;
  rq.L = L;
  rq.levels = levels;
  rq.hz_out = out;
  rq.hz_stats_out = stats;
  rq.bands_out = bands;
}

// One launch of the path kernels for a request: the device arrays of an mcp_launch_paths* call or of one shard's part of a tile.
struct Launch {
  const float* d_packed = nullptr;
  const double* d_pivot = nullptr;
  uint64_t seed = 0, path_begin = 0, n_paths = 0;
  float* d_terminal = nullptr;
  uint64_t stride = 0;
  float* d_mdd = nullptr;               // drawdown: [K][mdd_stride]
  uint64_t mdd_stride = 0;
  float* d_hz = nullptr;                // horizons: [H][K][hz_stride]
  uint64_t hz_stride = 0;
  const float* d_rows = nullptr;        // bootstrap: [R][N4], zero-padded
  const float* d_flows = nullptr;       // cash flows: [n_steps]
  const float* d_floor = nullptr;       // protection: [n_steps + 1] the floor schedule
  const float* d_targets = nullptr;     // glide path: [n_breaks][glide_rows(K)][N4] target blocks (glide_pack)
  const char* d_overlay = nullptr;      // overlay: [rows][row_begin N4 + 1][spot N4] (overlay_pack)
  const float* d_loading = nullptr;     // jumps: [N4] loadings, zero-padded
  const float* d_block1 = nullptr;      // regimes: [mu1 N4][L1 row pairs], the layout of mcp_pack_params
  bool attr = false;                    // the attribution walk (SPEC.md 4.10): FAM_AT instead of the request's own family
  const double* d_var = nullptr;        // attribution: [K] VaRs
  double* d_cross = nullptr;            // antithetic pairs: [K][path_grid(n_paths / 2)] cross partials
  double* d_attr_partials = nullptr;    // attribution: [K][path_grid(n_paths)][attr_record_len(N4)]
  float* d_contrib = nullptr;           // attribution: NULL or [K][N][contrib_stride]
  uint64_t contrib_stride = 0;
  void* d_partials = nullptr;
  void* d_hist = nullptr;
  hipStream_t stream = nullptr;
};

// Every rule a request meets: each feature's own arguments, then which features combine (MCP_E_UNSUPPORTED), then the outputs.
// `ln`: an mcp_launch_paths* call, whose device arrays are checked instead of the host arrays of an mcp_simulate* call.
int check_request(const mcp_params* prm, const Request& rq, uint64_t n_paths, const Launch* ln = nullptr, uint64_t path_begin = 0) {
  int rc;
  if ((rc = check_params(prm))) return rc;
  if (rq.rebalanced) {
    if ((rc = check_reb(rq.reb))) return rc;
    if (rq.src == SRC_BOOT ? rq.mu || rq.chol : !rq.mu || !rq.chol) return fail(MCP_E_ARG, "exactly one draw source: mu and chol, or boot");
  }
  if (rq.src == SRC_BOOT && (rc = check_boot(prm, rq.boot))) return rc;
  if (rq.src == SRC_T && (rc = check_student_t(prm, rq.st))) return rc;
  if (rq.cash) {
    if ((rc = check_cashflow(prm, rq.cf))) return rc;
    if (rq.src == SRC_BOOT ? rq.mu || rq.chol : !rq.mu || !rq.chol)
      return fail(MCP_E_ARG, "exactly one draw source: mu and chol (with or without student_t), or boot");
    if (!rq.counts_out) return fail(MCP_E_ARG, "counts_out is NULL");
    if ((rq.hz_counts_out == nullptr) != !rq.hz) return fail(MCP_E_ARG, "hz_counts_out must be NULL exactly when n_horizons == 0");
  }
  if (rq.glide) {                                              // SPEC.md 4.14: the rules, then what a glide path is not combined with
    if ((rc = check_glide(prm, rq.gl))) return rc;
    if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "glide paths compound simply (no log compounding)");
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH))
      return fail(MCP_E_UNSUPPORTED, "glide paths run on the unfolded recurrence and the spec's normals (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)");
    if (!rq.cash || rq.src == SRC_FHS || rq.rebalanced || rq.overlay || rq.garch || rq.jumps || rq.regimes || rq.dd || rq.attr || rq.anti)
      return fail(MCP_E_UNSUPPORTED, "a glide path is not combined with the drawdown, rebalancing, the overlay, GARCH, jumps, regimes, "
                                     "filtered rows, the attribution or antithetic pairs");
    if (ln) return fail(MCP_E_UNSUPPORTED, "glide paths are not wired into mcp_launch_paths*");
  }
  if (rq.protect) {                                            // SPEC.md 4.15: the rules, then what the protection is not combined with
    if ((rc = check_protect(prm, rq.pi))) return rc;
    if (!rq.counts_out) return fail(MCP_E_ARG, "counts_out is NULL");
    if ((rq.hz_counts_out == nullptr) != !rq.hz) return fail(MCP_E_ARG, "hz_counts_out must be NULL exactly when n_horizons == 0");
    if (rq.src == SRC_T && (rc = check_student_t(prm, rq.st))) return rc;
    if (rq.garch && (rc = check_garch(prm, rq.gv))) return rc;
    if (rq.jumps && (rc = check_jumps(prm->n_assets, rq.jp))) return rc;
    if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "protected paths compound simply (no log compounding)");
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH))
      return fail(MCP_E_UNSUPPORTED, "protected paths run on the unfolded recurrence and the spec's normals (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)");
    if (rq.src == SRC_BOOT || rq.src == SRC_FHS || rq.regimes || rq.rebalanced || rq.cash || rq.glide || rq.overlay || rq.attr || rq.anti)
      return fail(MCP_E_UNSUPPORTED, "floor protection is not combined with bootstrap or filtered rows, regimes, rebalancing, cash flows, "
                                     "glide paths, the overlay, the attribution or antithetic pairs");
    if (ln) return fail(MCP_E_UNSUPPORTED, "floor protection is not wired into mcp_launch_paths*");
  }
  if (rq.overlay && (rc = check_overlay(prm, rq.ov))) return rc;
  if (rq.garch && (rc = check_garch(prm, rq.gv))) return rc;
  if (rq.jumps && (rc = check_jumps(prm->n_assets, rq.jp))) return rc;
  const bool logc = prm->compounding != MCP_COMPOUND_SIMPLE;
  if (rq.jumps) {                                              // SPEC.md 4.12: what the jump-diffusion is not combined with
    if (logc) return fail(MCP_E_UNSUPPORTED, "jump-diffusion paths compound simply (no log compounding)");
    if (rq.src != SRC_GAUSS || rq.st || rq.garch)
      return fail(MCP_E_UNSUPPORTED, "jumps are not combined with Student-t draws, GARCH, bootstrap or filtered rows");
    if (rq.rebalanced || rq.cash || rq.overlay || rq.attr || rq.anti)
      return fail(MCP_E_UNSUPPORTED, "jumps are not combined with rebalancing, cash flows, the overlay, the attribution or antithetic pairs");
    if (ln) return fail(MCP_E_UNSUPPORTED, "jumps are not wired into mcp_launch_paths*");
  }
  if (rq.regimes) {                                            // SPEC.md 2.6 / 4.13: the rules, then what the regimes are not combined with
    if ((rc = check_regimes(prm->n_assets, rq.rs))) return rc;
    for (int i = 0; rq.mu && i < prm->n_assets; i++)
      if (!std::isfinite(rq.mu[i])) return fail(MCP_E_ARG, "regimes: mu, asset %d is not finite", i);
    for (size_t i = 0; rq.chol && i < (size_t)prm->n_assets * prm->n_assets; i++)
      if (!std::isfinite(rq.chol[i])) return fail(MCP_E_ARG, "regimes: chol, entry %zu is not finite", i);
    if (logc) return fail(MCP_E_UNSUPPORTED, "regime-switching paths compound simply (no log compounding)");
    if (rq.src != SRC_GAUSS || rq.st || rq.garch || rq.jumps)
      return fail(MCP_E_UNSUPPORTED, "regimes are not combined with Student-t draws, GARCH, jumps, bootstrap or filtered rows");
    if (rq.rebalanced || rq.cash || rq.overlay || rq.attr || rq.anti)
      return fail(MCP_E_UNSUPPORTED, "regimes are not combined with rebalancing, cash flows, the overlay, the attribution or antithetic pairs");
    if (ln) return fail(MCP_E_UNSUPPORTED, "regimes are not wired into mcp_launch_paths*");
  }
  if (rq.src == SRC_FHS) {                                     // SPEC.md 2.4 / 4.11: the rows, the triple, then what it is not combined with
    if ((rc = check_filtered(prm, rq.filt))) return rc;
    if ((rc = check_garch(prm, rq.gv))) return rc;
    if (logc) return fail(MCP_E_UNSUPPORTED, "filtered paths compound simply (no log compounding)");
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH))
      return fail(MCP_E_UNSUPPORTED, "filtered paths draw no normals (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)");
    if (rq.st || rq.garch || rq.rebalanced || rq.cash || rq.overlay || rq.dd || rq.attr || rq.anti)
      return fail(MCP_E_UNSUPPORTED, "filtered rows are not combined with Student-t draws, rebalancing, cash flows, the overlay, the drawdown, "
                                     "the attribution or antithetic pairs");
    if (ln) return fail(MCP_E_UNSUPPORTED, "filtered rows are not wired into mcp_launch_paths*");
  }
  if (rq.garch && logc)
    return fail(MCP_E_UNSUPPORTED, "GARCH paths compound simply (log compounding: expm1(S) has no finite mean under GARCH tails)");
  if (rq.garch && (rq.src == SRC_BOOT || rq.rebalanced || rq.cash || rq.overlay))
    return fail(MCP_E_UNSUPPORTED, "GARCH is not combined with bootstrap rows, rebalancing, cash flows or the overlay");
  if (rq.overlay && logc) return fail(MCP_E_UNSUPPORTED, "overlaid paths compound simply (no log compounding)");
  if (rq.overlay && (rq.src == SRC_BOOT || rq.rebalanced || rq.cash))
    return fail(MCP_E_UNSUPPORTED, "the overlay is not combined with bootstrap rows, rebalancing or cash flows");
  if (rq.rebalanced && logc) return fail(MCP_E_UNSUPPORTED, "rebalanced paths compound simply (no log compounding)");
  if (rq.cash && logc) return fail(MCP_E_UNSUPPORTED, "paths with cash flows compound simply (no log compounding)");
  if (rq.src == SRC_T && logc)
    return fail(MCP_E_UNSUPPORTED, "Student-t paths compound simply (log compounding: expm1(S) has no finite mean under t steps)");
  if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH)) {   // the fast steps exist for plain Gaussian walks only
    const char* who = rq.regimes           ? "regime-switching paths run on the spec's normals and the unfolded recurrence"
                      : rq.jumps           ? "jump-diffusion paths run on the spec's normals and the unfolded recurrence"
                      : rq.garch           ? "GARCH paths run on the spec's normals and the unfolded recurrence"
                      : rq.overlay         ? "overlaid paths run on the unfolded recurrence and the spec's normals"
                      : rq.cash            ? "paths with cash flows run on the unfolded recurrence and the spec's normals"
                      : rq.rebalanced      ? "rebalanced paths run on the unfolded recurrence and the spec's normals"
                      : rq.src == SRC_T    ? "Student-t paths run on the spec's normals and the unfolded recurrence"
                      : rq.src == SRC_BOOT ? "bootstrap paths draw no normals"
                      : rq.dd              ? "the drawdown runs on the spec's normals and the unfolded recurrence"
                      : rq.hz              ? "the horizons run on the spec's normals and the unfolded recurrence"
                                           : nullptr;
    if (who) return fail(MCP_E_UNSUPPORTED, "%s (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)", who);
    if ((prm->flags & MCP_FLAG_FOLD) && (prm->n_portfolios != 1 || (prm->flags & MCP_FLAG_NATIVE_MATH)))
      return fail(MCP_E_UNSUPPORTED, "MCP_FLAG_FOLD needs one portfolio and the spec's normals");
  }
  if (rq.attr) {                                               // SPEC.md 4.10: constant weights, simple compounding, the spec's step
    if (logc) return fail(MCP_E_UNSUPPORTED, "the attribution compounds simply (no log compounding)");
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH | MCP_FLAG_SHARD_PORTFOLIOS))
      return fail(MCP_E_UNSUPPORTED, "the attribution runs on the spec's normals, the unfolded recurrence and path shards (no MCP_FLAG_FOLD / "
                                     "MCP_FLAG_NATIVE_MATH / MCP_FLAG_SHARD_PORTFOLIOS)");
    if (rq.src == SRC_BOOT || rq.rebalanced || rq.cash || rq.overlay)
      return fail(MCP_E_UNSUPPORTED, "the attribution is not combined with bootstrap rows, rebalancing, cash flows or the overlay");
    if (rq.dd || rq.hz) return fail(MCP_E_UNSUPPORTED, "the attribution is not combined with the drawdown or horizons");
    if (prm->n_portfolios > MCP_MAX_ATTR_PORTFOLIOS)
      return fail(MCP_E_UNSUPPORTED, "the attribution takes at most %d portfolios, got %d", MCP_MAX_ATTR_PORTFOLIOS, prm->n_portfolios);
    if (!ln && (!rq.attr_out || !rq.attr_counts_out)) return fail(MCP_E_ARG, "attr_out or attr_counts_out is NULL");
  }
  if (rq.anti) {                                               // SPEC.md 2.3: whole pairs of the spec's step on Gaussian, t or GARCH draws
    if ((path_begin | n_paths) & 1)
      return fail(MCP_E_ARG, "antithetic pairs: path_begin=%llu and n_paths=%llu must both be even", (unsigned long long)path_begin,
                  (unsigned long long)n_paths);
    if (!ln && !rq.pair_out) return fail(MCP_E_ARG, "pair_out is NULL");
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH | MCP_FLAG_SHARD_PORTFOLIOS))
      return fail(MCP_E_UNSUPPORTED, "antithetic pairs run on the spec's normals, the unfolded recurrence and path shards (no MCP_FLAG_FOLD / "
                                     "MCP_FLAG_NATIVE_MATH / MCP_FLAG_SHARD_PORTFOLIOS)");
    if (rq.src == SRC_BOOT || rq.rebalanced || rq.cash || rq.overlay || rq.attr)
      return fail(MCP_E_UNSUPPORTED, "antithetic pairs are not combined with bootstrap rows, rebalancing, cash flows, the overlay or the attribution");
  }
  if (rq.dd && rq.hz) return fail(MCP_E_UNSUPPORTED, "horizons and the drawdown are not tracked in one walk");
  if (rq.dd && (rq.src == SRC_BOOT || rq.rebalanced))
    return fail(MCP_E_UNSUPPORTED, "the drawdown is not tracked on bootstrap or rebalanced paths");
  if (rq.src == SRC_T && rq.rebalanced) return fail(MCP_E_UNSUPPORTED, "Student-t draws are not combined with rebalancing");
  if (rq.cash && (rq.dd || rq.rebalanced))
    return fail(MCP_E_UNSUPPORTED, "cash flows are not combined with the drawdown or with rebalancing");
  if (rq.src != SRC_BOOT && rq.src != SRC_FHS && (uint64_t)prm->n_steps * (uint64_t)((prm->n_assets + 3) / 4) > 0xFFFFFFFFull)
    return fail(MCP_E_UNSUPPORTED, "n_steps * ceil(N/4) exceeds the 32-bit Philox block counter");
  if (!rq.dd && rq.mdd_out) return fail(MCP_E_ARG, "mdd_out needs dd_stats_out");
  if (!rq.hz) {
    if (rq.L != 0 || rq.hz_out || rq.hz_stats_out || rq.bands_out)
      return fail(MCP_E_ARG, "n_horizons = 0: n_levels must be 0 and horizon_out, hz_stats_out, bands_out NULL");
  } else {
    if ((rc = check_horizons(prm->n_steps, rq.H, rq.steps))) return rc;
    if ((rc = check_levels(rq.L, rq.levels))) return rc;
    if (!ln && !rq.hz_stats_out) return fail(MCP_E_ARG, "hz_stats_out is NULL");
    if ((rq.bands_out == nullptr) != (rq.L == 0)) return fail(MCP_E_ARG, "bands_out must be NULL exactly when n_levels == 0");
  }
  if (!ln) {
    if ((rq.src != SRC_BOOT && rq.src != SRC_FHS && (!rq.mu || !rq.chol)) || !rq.W || !rq.stats_out || (rq.dd && !rq.dd_stats_out))
      return fail(MCP_E_ARG, "NULL pointer");
    if (n_paths < 1) return fail(MCP_E_ARG, "n_paths must be >= 1");
    return MCP_OK;
  }
  if (!ln->d_packed || !ln->d_terminal) return fail(MCP_E_ARG, "NULL device pointer");
  if (rq.dd && !ln->d_mdd) return fail(MCP_E_ARG, "d_mdd is NULL");
  if (rq.hz && !ln->d_hz) return fail(MCP_E_ARG, "d_horizon is NULL");
  if ((ln->d_partials == nullptr) != (ln->d_hist == nullptr)) return fail(MCP_E_ARG, "d_partials and d_hist go together (both or neither)");
  if (n_paths < 1) return fail(MCP_E_ARG, "n_paths must be >= 1");
  const uint64_t need[3] = {ln->stride, rq.dd ? ln->mdd_stride : n_paths, rq.hz ? ln->hz_stride : n_paths};
  const char* name[3] = {"terminal_stride", "mdd_stride", "horizon_stride"};
  for (int i = 0; i < 3; i++)
    if (need[i] < n_paths) return fail(MCP_E_ARG, "%s %llu < n_paths %llu", name[i], (unsigned long long)need[i], (unsigned long long)n_paths);
  return MCP_OK;
}

// SPEC.md 5.4: mu_i of the pivot of rebalanced paths, binary64 -- the drift (Gaussian) or the mean of column i of the rows
// (bootstrap, j ascending)
void reb_means(int N, const float* mu, const mcp_bootstrap* boot, double* out) {
  for (int i = 0; i < N; i++) {
    if (boot) {
      double sum = 0.0;
      for (int j = 0; j < boot->n_rows; j++) sum += (double)boot->rows[(size_t)j * N + i];
      out[i] = sum / (double)boot->n_rows;
    } else {
      out[i] = (double)mu[i];
    }
  }
}

// SPEC.md 5.4: the pivots at T steps of period m for K portfolios.  The dates m, 2m, .. < T cut [0, T] into F = floor((T-1)/m)
// segments of length m and a last one of length T - F m (m = 0 or m >= T: one segment of length T); with
// a_i(l) = expm1(l log1p(mu_i)) and g(l) = sum_i W[k,i] a_i(l) (i ascending), c = expm1(F log1p(g(m)) + log1p(g(l_last))),
// 0 where it is not finite (0 for T = 0).
void reb_pivots(int N, int K, int T, int m, const double* mu, const float* W, double* out) {
  if (T <= 0) {
    for (int k = 0; k < K; k++) out[k] = 0.0;
    return;
  }
  const int64_t F = (m >= 1 && m < T) ? (int64_t)(T - 1) / m : 0;
  const double l_last = (double)((int64_t)T - F * m);
  std::vector<double> af((size_t)N), al((size_t)N);
  for (int i = 0; i < N; i++) {
    const double lp = std::log1p(mu[i]);
    al[(size_t)i] = std::expm1(l_last * lp);
    af[(size_t)i] = F ? std::expm1((double)m * lp) : 0.0;
  }
  for (int k = 0; k < K; k++) {
    const float* w = W + (size_t)k * N;
    double gf = 0.0, gl = 0.0;
    for (int i = 0; i < N; i++) {
      gf += (double)w[i] * af[(size_t)i];
      gl += (double)w[i] * al[(size_t)i];
    }
    double e = std::log1p(gl);
    if (F) e = (double)F * std::log1p(gf) + e;
    const double c = std::expm1(e);
    out[k] = std::isfinite(c) ? c : 0.0;
  }
}

// SPEC.md 5.6: the per-step mean m_k of the draws, binary64 -- sum_i W[k,i] mu_i (i ascending) or the row mean of SPEC.md 5.3
void cash_means(int N, int K, const float* mu, const mcp_bootstrap* boot, const float* W, double* out) {
  if (boot) {
    std::vector<double> s2((size_t)K);
    boot_moments(N, boot, W, K, out, s2.data());
    return;
  }
  for (int k = 0; k < K; k++) {
    const float* w = W + (size_t)k * N;
    double m = 0.0;
    for (int i = 0; i < N; i++) m += (double)w[i] * (double)(mu[i] + 0.0f);
    out[k] = m;
  }
}

// SPEC.md 5.6: one Horner walk A_s = A_{s-1} (1 + m) + c_s from A_0 = fl32(v0) per portfolio; the pivot max(A, 0) / fl32(v0) - 1
// (0 where not finite) after step T into out_T[k] and after the steps of the H horizons into out_hz[h*K + k].
void cash_pivots(int K, int T, const double* m, const float* flows, double v0, int H, const int32_t* steps, double* out_T, double* out_hz) {
  const auto pivot = [v0](double A) {
    const double c = (A > 0.0 ? A : 0.0) / v0 - 1.0;
    return std::isfinite(A) && std::isfinite(c) ? c : 0.0;
  };
  for (int k = 0; k < K; k++) {
    const double g = 1.0 + m[k];
    double A = v0;
    int hi = 0;
    for (int s = 1; s <= T; s++) {
      A = A * g;
      A = A + (double)flows[s - 1];
      if (hi < H && steps[hi] == s) out_hz[(size_t)(hi++) * K + k] = pivot(A);
    }
    out_T[k] = pivot(A);
  }
}

// SPEC.md 5.14: cash_pivots with the per-step mean of the step's segment.  m[g*K + k]: the mean of portfolio k on the weights of
// block g = 0 .. G (block 0: the call's W); step s walks on block #{j : breaks[j] < s}.  flows NULL: c_s = +0.  G = 0, or equal
// means in every block, is cash_pivots operation for operation.
void glide_pivots(int K, int T, int G, const int32_t* breaks, const double* m, const float* flows, double v0, int H, const int32_t* steps,
                  double* out_T, double* out_hz) {
  const auto pivot = [v0](double A) {
    const double c = (A > 0.0 ? A : 0.0) / v0 - 1.0;
    return std::isfinite(A) && std::isfinite(c) ? c : 0.0;
  };
  for (int k = 0; k < K; k++) {
    double A = v0;
    int hi = 0, gi = 0;
    double g = 1.0 + m[k];
    for (int s = 1; s <= T; s++) {
      A = A * g;
      A = A + (flows ? (double)flows[s - 1] : 0.0);
      if (hi < H && steps[hi] == s) out_hz[(size_t)(hi++) * K + k] = pivot(A);
      if (gi < G && breaks[gi] == s) g = 1.0 + m[(size_t)(++gi) * K + k];
    }
    out_T[k] = pivot(A);
  }
}
// The means m[g*kt + k] of glide_pivots for the portfolios [k0, k0 + kt) of a call with K portfolios (cash_means per block)
void glide_means(int N, int K, int k0, int kt, const float* mu, const mcp_bootstrap* boot, const float* W, const mcp_glide* gl, double* out) {
  cash_means(N, kt, mu, boot, W + (size_t)k0 * N, out);
  for (int g = 0; g < gl->n_breaks; g++)
    cash_means(N, kt, mu, boot, gl->targets + ((size_t)g * K + (size_t)k0) * N, out + (size_t)(g + 1) * kt);
}

// Inverse-CDF coefficient table (SPEC.md section 3; DATA of the spec, generated by tools/fit_icdf_table.py): one
// device-resident copy per device, uploaded on first use on the caller's stream.  The first call on a device
// allocates and synchronises: do it once before capturing launches into a hipGraph.
const float k_icdf_table[mcp::ICDF_ENTRIES][4] = {
#include "mcp_icdf_table.inc"
};
constexpr int MAX_DEVICES = 64;
std::mutex g_tab_mu;
float4* g_tables[MAX_DEVICES] = {nullptr};

// Device that owns `stream` (the current device for the NULL stream).
int stream_device(hipStream_t stream, int* dev) {
  if (stream) {
    hipDevice_t d = 0;
    if (hipStreamGetDevice(stream, &d) == hipSuccess) { *dev = (int)d; return MCP_OK; }
  }
  HIP_TRY(hipGetDevice(dev));
  return MCP_OK;
}

// Makes `dev` current for the lifetime of the object (launches go to the current device; a caller may hand over a
// stream of another device than the thread's current one).
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); changed = err == hipSuccess; }
  }
  ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};

int device_tables(int dev, hipStream_t stream, const float4** out) {
  if (dev < 0 || dev >= MAX_DEVICES) return fail(MCP_E_UNSUPPORTED, "device index %d", dev);
  std::lock_guard<std::mutex> lock(g_tab_mu);
  if (!g_tables[dev]) {
    float4* t = nullptr;
    if (hipMalloc((void**)&t, sizeof k_icdf_table) != hipSuccess) return fail(MCP_E_NOMEM, "hipMalloc of the inverse-CDF table failed");
    hipError_t e = hipMemcpyAsync(t, k_icdf_table, sizeof k_icdf_table, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);     // other streams may use the table next
    if (e != hipSuccess) { (void)hipFree(t); return fail(MCP_E_HIP, "inverse-CDF table upload: %s", hipGetErrorString(e)); }
    g_tables[dev] = t;
  }
  *out = g_tables[dev];
  return MCP_OK;
}

// Device memory (hipMalloc) and pinned host memory (hipHostMalloc, portable; `dev` is the device address of a mapped one), grown
// by grow() / grow_mapped() and released by release().
template <class T> struct DevBuf { T* p = nullptr; size_t cap = 0; };
template <class T> struct HostBuf { T* p = nullptr; size_t cap = 0; void* dev = nullptr; };

// One shard of a context: a device, its stream and every buffer a pass needs there.
struct Shard {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;                 // same-device exchange: "my step is enqueued"
  void* ws[MCP_WS_COUNT] = {nullptr};      // ws[MCP_WS_STATS] is stats.dev
  size_t ws_cap[MCP_WS_COUNT] = {0};
  DevBuf<float> packed;
  DevBuf<float> terminal;
  DevBuf<mcp_record> gather;               // [shards][K tile] records of all shards (shard 0 finishes the statistics)
  HostBuf<float> h_packed;                 // pinned staging
  HostBuf<double> h_pivot;                 // pinned staging of the [K tile] pivots
  HostBuf<mcp_stats> stats;                // mapped: the last kernel of a pass writes the [K] records straight into host memory
  struct {                                 // drawdown calls
    DevBuf<float> mdd;                     // [K tile][paths] q / d of SPEC.md 4.2
    HostBuf<mcp_stats> stats;              // the drawdown statistics, mapped
  } dd;
  struct {                                 // horizon calls
    DevBuf<float> values;                  // [H][K tile][paths] V_h / S_h of SPEC.md 4.3
    DevBuf<double> pivot;                  // [H][K tile] pivots (mcp_pivots at n_steps = h)
    HostBuf<double> h_pivot;               // pinned staging of pivot
    HostBuf<mcp_stats> stats;              // [1 + L][H][K tile] records of the alpha select and of every level's select, mapped
  } hz;
  DevBuf<float> boot;                      // bootstrap calls: [R][N4] observed rows, zero-padded (SPEC.md 2.1)
  DevBuf<char> overlay;                    // overlay calls: the table of overlay_pack (SPEC.md 4.8)
  struct {                                 // cash-flow calls (SPEC.md 4.7 / 5.6)
    DevBuf<float> flows;                   // [n_steps] the schedule
    DevBuf<unsigned long long> counts;     // [(1 + H) K tile][2] {n_ruined, n_short}: the terminal rows, then the horizon rows
    HostBuf<unsigned long long> h_counts;  // pinned copy of counts
  } cf;
  struct {                                 // attribution calls (SPEC.md 4.10 / 5.9)
    DevBuf<double> in;                     // [2][K]: the VaRs, then the pivots
    HostBuf<double> h_in;                  // pinned staging of `in`
    DevBuf<double> partials;               // [K][path_grid(paths)][attr_record_len(N4)]: one record per workgroup
    DevBuf<double> records;                // [K][attr_record_len(N4)]: the workgroups' records summed in block order
    HostBuf<double> h_records;             // pinned copy of records
    DevBuf<float> contrib;                 // [K][N][paths] A_ki, when the caller asks for them
  } at;
  struct {                                 // antithetic calls (SPEC.md 5.10)
    DevBuf<double> partials;               // [K tile][path_grid(pairs)] cross partials, one per workgroup
    DevBuf<double> cross;                  // [K tile] the workgroups' partials summed in block order
    HostBuf<double> h_cross;               // pinned copy of cross
  } pr;
};

int grow_dev(void** p, size_t* cap, size_t need, hipStream_t zero_on = nullptr, bool zero = false) {
  if (need <= *cap) return MCP_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t bytes = (need + 7) & ~(size_t)7;
  if (hipMalloc(p, bytes) != hipSuccess) return fail(MCP_E_NOMEM, "hipMalloc(%zu) failed", bytes);
  *cap = need;
  if (zero) HIP_TRY(mcp::launch_zero(*p, bytes, zero_on));
  return MCP_OK;
}

int grow_host(void** p, size_t* cap, size_t need, bool mapped = false) {
  if (need <= *cap) return MCP_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  if (hipHostMalloc(p, need, mapped ? (hipHostMallocMapped | hipHostMallocPortable) : hipHostMallocPortable) != hipSuccess)   // portable: every device of a multi-device context copies from / writes to it
    return fail(MCP_E_NOMEM, "hipHostMalloc(%zu) failed", need);
  *cap = need;
  return MCP_OK;
}

// `count` elements of T
template <class T> int grow(DevBuf<T>& b, size_t count) { return grow_dev((void**)&b.p, &b.cap, count * sizeof(T)); }
template <class T> int grow(HostBuf<T>& b, size_t count) { return grow_host((void**)&b.p, &b.cap, count * sizeof(T)); }
template <class T> int grow_mapped(HostBuf<T>& b, size_t count) {
  if (count * sizeof(T) <= b.cap) return MCP_OK;
  if (int rc = grow_host((void**)&b.p, &b.cap, count * sizeof(T), true)) return rc;
  HIP_TRY(hipHostGetDevicePointer(&b.dev, b.p, 0));
  return MCP_OK;
}

template <class T> void release(DevBuf<T>& b) { if (b.p) (void)hipFree(b.p); }
template <class T> void release(HostBuf<T>& b) { if (b.p) (void)hipHostFree(b.p); }

// RCCL entry points, resolved at run time (no link-time dependency: a single-device user never loads librccl).
// Prototypes as in /opt/rocm/include/rccl/rccl.h:236 (ncclCommInitAll), :260 (ncclCommDestroy), :339
// (ncclGetErrorString), :611 (ncclAllReduce), :678 (ncclAllGather), group calls; enum values :448 (ncclSum = 0),
// :459-467 (ncclUint64 = 5, ncclFloat64 = 8).
struct Rccl {
  void* handle = nullptr;
  int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
  int (*CommDestroy)(void* comm) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*AllReduce)(const void* send, void* recv, size_t count, int dtype, int op, void* comm, hipStream_t s) = nullptr;
  int (*AllGather)(const void* send, void* recv, size_t sendcount, int dtype, void* comm, hipStream_t s) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
};
constexpr int NCCL_SUM = 0, NCCL_UINT64 = 5, NCCL_FLOAT64 = 8;
std::mutex g_rccl_mu;
Rccl g_rccl;

int load_rccl(const Rccl** out) {
  std::lock_guard<std::mutex> lock(g_rccl_mu);
  if (!g_rccl.handle) {
    const char* cands[3] = {getenv("MCP_RCCL_LIB"), "librccl.so.1", "librccl.so"};
    void* h = nullptr;
    for (const char* c : cands)
      if (c && *c && (h = dlopen(c, RTLD_NOW | RTLD_LOCAL))) break;   // LOCAL: every entry point is taken with dlsym; a GLOBAL librccl
                                                                      // interposes symbols of a torch imported later (abort at exit)
    if (!h) return fail(MCP_E_COMM, "cannot load librccl (set MCP_RCCL_LIB): %s", dlerror());
    Rccl r;
    r.handle = h;
#define MCP_SYM(field, name) \
    *(void**)(&r.field) = dlsym(h, name); \
    if (!r.field) { dlclose(h); return fail(MCP_E_COMM, "librccl lacks %s", name); }
    MCP_SYM(CommInitAll, "ncclCommInitAll") MCP_SYM(CommDestroy, "ncclCommDestroy") MCP_SYM(GetErrorString, "ncclGetErrorString")
    MCP_SYM(AllReduce, "ncclAllReduce") MCP_SYM(AllGather, "ncclAllGather") MCP_SYM(GroupStart, "ncclGroupStart")
    MCP_SYM(GroupEnd, "ncclGroupEnd")
#undef MCP_SYM
    g_rccl = r;
  }
  *out = &g_rccl;
  return MCP_OK;
}

}  // namespace

struct mcp_ctx {
  std::vector<Shard> sh;
  std::mutex mu;
  bool all_same = false;             // every shard on ONE device (logical shards)
  bool same_device = false;          // exchange through a kernel of shard 0 that reads / writes every shard's buffer: shards
                                     // of ONE device, or distinct devices with peer access (the fallback when RCCL is unavailable)
  bool exchange_always = false;      // MCP_FORCE_RCCL=1: run the collectives with one device too (a 1-rank communicator)
  int exchange_mode = MCP_EXCHANGE_UNSET;
  std::string exchange_note;         // why RCCL was not used, when the peer-access kernel stands in for it
  const Rccl* rccl = nullptr;
  std::vector<void*> comms;          // one ncclComm_t per shard (distinct devices only)
  size_t terminal_budget = (size_t)8 << 30;
  double* d_sweep = nullptr;         // inputs then outputs of mcp_sweep_historical (shard 0)
  size_t sweep_cap = 0;
  float* h_boot = nullptr;           // bootstrap calls: pinned, portable [R][N4] padded rows, uploaded to every shard's boot buffer
  size_t h_boot_cap = 0;
  float* h_flows = nullptr;          // cash-flow calls: pinned, portable [n_steps] schedule, uploaded to every shard's flows buffer
  size_t h_flows_cap = 0;
  char* h_overlay = nullptr;         // overlay calls: pinned, portable table of overlay_pack, uploaded to every shard's overlay buffer
  size_t h_overlay_cap = 0;
};


extern "C" {

int mcp_abi_version(void) { return MCP_ABI_VERSION; }

int mcp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* mcp_last_error(void) { return g_err.c_str(); }

size_t mcp_packed_len(int n_assets, int n_portfolios) {
  if (n_assets < 1 || n_assets > MCP_MAX_ASSETS || n_portfolios < 1) return 0;
  const size_t n4 = (size_t)n4_of(n_assets);
  return n4 + n4 * (n4 / 2 + 1) + (size_t)kpad_of(n_portfolios) * n4 + 4 + n4;   // ... + fold block [c, v] (+3 pad)
}

int mcp_pack_params(int n_assets, int n_portfolios, const float* mu, const float* chol, const float* W,
                    float* out, size_t out_len) {
  const size_t need = mcp_packed_len(n_assets, n_portfolios);
  if (need == 0) return fail(MCP_E_ARG, "bad shape N=%d K=%d", n_assets, n_portfolios);
  if (!mu || !chol || !W || !out) return fail(MCP_E_ARG, "NULL pointer");
  if (out_len < need) return fail(MCP_E_ARG, "packed buffer too small: %zu < %zu", out_len, need);
  const int N = n_assets, n4 = n4_of(N);
  memset(out, 0, need * sizeof(float));
  for (int i = 0; i < N; i++) out[i] = mu[i] + 0.0f;   // -0 -> +0 (SPEC.md section 4)
  // lower triangle in row pairs: pair m = rows (2m, 2m+1), columns j = 0..2m+1 interleaved as
  // (L[2m][j], L[2m+1][j]); L[2m][2m+1] is a structural zero.  Offset of pair m: 2m(m+1).
  float* L = out + n4;
  for (int i = 0; i < N; i++)
    for (int j = 0; j <= i; j++) L[2 * (i / 2) * (i / 2 + 1) + 2 * j + (i & 1)] = chol[(size_t)i * N + j];
  float* Wp = L + (size_t)n4 * (n4 / 2 + 1);
  for (int k = 0; k < n_portfolios; k++)
    for (int i = 0; i < N; i++) Wp[(size_t)k * n4 + i] = W[(size_t)k * N + i];
  // fold block of portfolio 0 (SPEC.md section 4.1): c = w.mu, v = L^T w, accumulated in binary64 (i ascending)
  // from the binary32 inputs, rounded once to binary32
  float* F = Wp + (size_t)kpad_of(n_portfolios) * n4;
  double c = 0.0;
  for (int i = 0; i < N; i++) c += (double)W[i] * (double)out[i];
  F[0] = (float)c;
  for (int j = 0; j < N; j++) {
    double v = 0.0;
    for (int i = j; i < N; i++) v += (double)W[i] * (double)chol[(size_t)i * N + j];
    F[1 + j] = (float)v;
  }
  return MCP_OK;
}

uint64_t mcp_moment_slots(int K, uint64_t n_paths) { return K < 1 ? 0 : mcp::moment_slots(uses_sweep(K), n_paths); }

size_t mcp_ws_bytes(int which, int K, uint64_t n_paths) {
  if (K < 1) return 0;
  switch (which) {
    case MCP_WS_PARTIALS: return (size_t)K * (size_t)mcp_moment_slots(K, n_paths) * sizeof(mcp::MomentPartial);
    case MCP_WS_RECORD: return (size_t)K * sizeof(mcp_record);
    case MCP_WS_STATE: return (size_t)K * 2 * sizeof(mcp::SelectState);
    case MCP_WS_HIST: return (size_t)K * 2 * MCP_SELECT_BINS * sizeof(unsigned long long);
    case MCP_WS_QUANT: return (size_t)K * sizeof(mcp::Quantile);
    case MCP_WS_STATS: return (size_t)K * sizeof(mcp_stats);
    case MCP_WS_BELOW: return (size_t)K * mcp::stream_slots(K) * sizeof(double);
    case MCP_WS_PIVOT: return (size_t)K * sizeof(double);
    default: return 0;
  }
}

int mcp_pivots(const mcp_params* prm, const float* mu, const float* chol, const float* W, double* out) {
  if (int rc = check_params(prm)) return rc;
  if (!mu || !chol || !W || !out) return fail(MCP_E_ARG, "NULL pointer");
  const int N = prm->n_assets, K = prm->n_portfolios;
  const double T = (double)prm->n_steps;
  for (int k = 0; k < K; k++) {
    const float* w = W + (size_t)k * N;
    double m = 0.0;
    for (int i = 0; i < N; i++) m += (double)w[i] * (double)(mu[i] + 0.0f);
    double c;
    if (prm->compounding == MCP_COMPOUND_LOG) {
      double s2 = 0.0;                                   // |L^T w|^2 = w' Sigma w
      for (int j = 0; j < N; j++) {
        double v = 0.0;
        for (int i = j; i < N; i++) v += (double)w[i] * (double)chol[(size_t)i * N + j];
        s2 += v * v;
      }
      c = std::expm1(T * (m + 0.5 * s2));
    } else {
      c = m > -1.0 ? std::expm1(T * std::log1p(m)) : 0.0;
    }
    out[k] = std::isfinite(c) ? c : 0.0;
  }
  return MCP_OK;
}

int mcp_rebalance_pivots(const mcp_params* prm, const mcp_rebalance* reb, const float* mu, const mcp_bootstrap* boot, const float* W,
                         double* out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_reb(reb)) return rc;
  if ((mu == nullptr) == (boot == nullptr)) return fail(MCP_E_ARG, "exactly one of mu and boot");
  if (boot)
    if (int rc = check_boot(prm, boot)) return rc;
  if (!W || !out) return fail(MCP_E_ARG, "NULL pointer");
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "rebalanced paths compound simply (no log compounding)");
  std::vector<double> m((size_t)prm->n_assets);
  reb_means(prm->n_assets, mu, boot, m.data());
  reb_pivots(prm->n_assets, prm->n_portfolios, prm->n_steps, reb->period, m.data(), W, out);
  return MCP_OK;
}

int mcp_bootstrap_pivots(const mcp_params* prm, const mcp_bootstrap* boot, const float* W, double* out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_boot(prm, boot)) return rc;
  if (!W || !out) return fail(MCP_E_ARG, "NULL pointer");
  const int K = prm->n_portfolios;
  std::vector<double> m((size_t)K), s2((size_t)K);
  boot_moments(prm->n_assets, boot, W, K, m.data(), s2.data());
  for (int k = 0; k < K; k++) out[k] = boot_pivot(prm->compounding, prm->n_steps, m[(size_t)k], s2[(size_t)k]);
  return MCP_OK;
}

}  // extern "C"

// The blocks that the family kernels add to PathArgs (mcp_paths.h), filled from the request and its launch; a block the request
// does not carry is empty.
static void fill_hz(mcp::PathArgsHZ& x, const Request& rq, const Launch& ln) {
  x.hz = rq.hz ? ln.d_hz : nullptr;
  x.hz_stride = rq.hz ? ln.hz_stride : 0;
  x.n_horizons = rq.hz ? rq.H : 0;
  for (int i = 0; i < MCP_MAX_HORIZONS; i++) x.steps[i] = i < x.n_horizons ? rq.steps[i] : 0;
}
static mcp::BootArgs boot_block(const Request& rq, const Launch& ln) {
  mcp::BootArgs bt;
  const bool on = rq.src == SRC_BOOT || rq.src == SRC_FHS;
  bt.rows = on ? (const float4*)ln.d_rows : nullptr;
  bt.thr = on ? boot_threshold(rows_of(rq).mean_block) : 0;
  bt.n_rows = on ? (uint32_t)rows_of(rq).n_rows : 0;
  bt.pad = 0;
  return bt;
}
// SPEC.md 4.11: the shocks sit behind the [R][N4] rows of the launch's row buffer; a itself, not a_N
static mcp::FiltArgs filt_block(const Request& rq, const Launch& ln, int n_assets) {
  const GarchConsts c = garch_consts(rq.gv, n_assets);
  mcp::FiltArgs fh;
  fh.shock = ln.d_rows + (size_t)rq.filt->n_rows * (size_t)n4_of(n_assets);
  fh.a = c.a;
  fh.b = c.b;
  fh.omega = c.omega;
  fh.h0 = c.g;
  return fh;
}
static mcp::StudentArgs student_block(const Request& rq) {
  mcp::StudentArgs st;
  st.dof = rq.src == SRC_T ? rq.st->dof : 0;                   // 0: Gaussian draws
  st.pad = 0;
  return st;
}
static mcp::GarchArgs garch_block(const mcp_garch* g, int n_assets) {
  const GarchConsts c = garch_consts(g, n_assets);
  mcp::GarchArgs gv;
  gv.a_n = c.a_n;
  gv.b = c.b;
  gv.omega = c.omega;
  gv.h0 = c.g;
  gv.n_assets = n_assets;
  gv.pad = 0;
  return gv;
}
// SPEC.md 2.5: the thresholds and the binary32 jump law; the loadings sit behind the launch's packed block
static mcp::JumpArgs jump_block(const Request& rq, const Launch& ln) {
  const JumpConsts c = jump_consts(rq.jp);
  mcp::JumpArgs jp;
  jp.loading = ln.d_loading;
  for (int k = 0; k < MCP_MAX_JUMPS; k++) jp.thr[k] = c.thr[k];
  jp.m = c.m;
  jp.s = c.s;
  return jp;
}
// SPEC.md 2.6: the thresholds; the regime-1 block sits behind the launch's packed block
static mcp::RegimeArgs regime_block(const Request& rq, const Launch& ln) {
  const RegimeConsts c = regime_consts(rq.rs);
  mcp::RegimeArgs rs;
  rs.block1 = ln.d_block1;
  rs.thr01 = c.thr01;
  rs.thr10 = c.thr10;
  rs.thr_start = c.thr_start;
  return rs;
}
// SPEC.md 4.14: the breaks; the target blocks sit behind the launch's packed block
static mcp::GlideArgs glide_block(const Request& rq, const Launch& ln, int n_assets, int n_portfolios) {
  mcp::GlideArgs gp;
  gp.targets = ln.d_targets;
  gp.stride = (uint32_t)(glide_rows(n_portfolios) * (size_t)n4_of(n_assets));
  gp.n_breaks = rq.gl->n_breaks;
  for (int g = 0; g < MCP_MAX_GLIDE; g++) gp.breaks[g] = g < gp.n_breaks ? rq.gl->breaks[g] : 0;
  return gp;
}
// SPEC.md 4.15: the binary32 constants; the schedule sits behind the launch's packed block
static mcp::ProtectArgs protect_block(const Request& rq, const Launch& ln) {
  const ProtectConsts c = protect_consts(rq.pi);
  mcp::ProtectArgs pi;
  pi.floor = ln.d_floor;
  pi.m = c.m;
  pi.b = c.b;
  pi.rf = c.rf;
  pi.theta = c.theta;
  return pi;
}
static mcp::OverlayArgs overlay_block(const Request& rq, const Launch& ln, int n_assets) {
  mcp::OverlayArgs ov;
  const size_t row_bytes = (size_t)rq.ov->n_rows * sizeof(mcp_overlay_row);
  ov.rows = (const mcp_overlay_row*)ln.d_overlay;
  ov.row_begin = (const int32_t*)(ln.d_overlay + row_bytes);
  ov.spot = (const float*)(ln.d_overlay + row_bytes) + n4_of(n_assets) + 1;
  ov.mask = 0;
  for (int i = 0; i < n_assets; i++)                           // the padding assets >= N own no rows
    if (rq.ov->row_begin[i + 1] > rq.ov->row_begin[i]) ov.mask |= (uint64_t)1 << i;
  return ov;
}
static mcp::AttrArgs attr_block(const Launch& ln, int n_assets) {
  mcp::AttrArgs at;
  at.var = ln.d_var;
  at.partials = ln.d_attr_partials;
  at.contrib = ln.d_contrib;
  at.contrib_stride = ln.contrib_stride;
  at.n_assets = n_assets;
  at.pad = 0;
  return at;
}

// Enqueues the path kernels of a checked request (check_request).  Plain Gaussian walks with K >= 17 run on the MFMA sweep
// kernels; every other request runs its family's kernel, K >= 17 as passes of the 8-portfolio kernel (the sweep kernels track
// neither the path's peak, its intermediate values, rows nor t draws).  Its moment partials keep the layout mcp_moment_slots(K, n)
// gives (what mcp_launch_scan reads): where that is one slot per 64-path tile (K >= 17), an empty pass 0 first pads every slot,
// and the path kernel's workgroups overwrite the first path_grid(n) of them.
static int launch_paths_impl(const mcp_params* prm, const Request& rq, const Launch& ln) {
  const int N = prm->n_assets, nb = (N + 3) / 4;
  const int K = prm->n_portfolios;
  const bool plain = rq.src == SRC_GAUSS && !rq.dd && !rq.hz && !rq.rebalanced && !rq.cash && !rq.overlay && !rq.garch && !rq.jumps && !rq.regimes &&
                     !rq.protect;
  mcp::PathLaunchArgs s = {};             // every block the request does not carry stays empty
  mcp::PathArgs& a = s.hz;
  const float4* tables = nullptr;
  int dev = 0;
  if (int rc = stream_device(ln.stream, &dev)) return rc;
  DeviceGuard guard(dev);                 // the stream may belong to another device than the thread's current one
  if (guard.err != hipSuccess) return fail(MCP_E_HIP, "hipSetDevice(%d): %s", dev, hipGetErrorString(guard.err));
  if (int rc = device_tables(dev, ln.stream, &tables)) return rc;
  const bool sweep = plain && !ln.attr && !rq.anti && uses_sweep(K);
  a.tables = tables;
  a.packed = ln.d_packed;
  a.terminal = ln.d_terminal;
  a.pivot = ln.d_pivot;
  a.partials = (mcp::MomentPartial*)ln.d_partials;
  a.hist = sweep ? nullptr : (unsigned long long*)ln.d_hist;     // the sweep kernels leave digit 0 to hist(0) below
  a.slots = mcp_moment_slots(K, ln.n_paths);
  a.v0d = (double)(float)prm->v0;
  a.inv_v0d = 1.0 / a.v0d;
  { int e = 0; a.v0_pow2 = std::frexp(a.v0d, &e) == 0.5; }
  a.seed = ln.seed;
  a.path_begin = ln.path_begin;
  a.n_paths = ln.n_paths;
  a.stride = ln.stride;
  a.n_steps = prm->n_steps;
  a.n_portfolios = K;
  a.compounding = prm->compounding;
  a.v0 = (float)prm->v0;
  a.k_count = K;
  a.fold_offset = (uint32_t)(n4_of(N) + n4_of(N) * (n4_of(N) / 2 + 1) + kpad_of(K) * n4_of(N));
  if (rq.anti) {
    // SPEC.md 2.3: one lane per pair -- the kernel counts pairs and stores the members 2j, 2j + 1 of every row with one 8-byte store
    if ((ln.path_begin | ln.n_paths | ln.stride | (rq.dd ? ln.mdd_stride : 0) | (rq.hz ? ln.hz_stride : 0)) & 1)
      return fail(MCP_E_ARG, "antithetic pairs: a launch begins, ends and strides at even path ids");
    a.path_begin = ln.path_begin / 2;
    a.n_paths = ln.n_paths / 2;
    s.pr.cross = ln.d_partials ? ln.d_cross : nullptr;
  }
  if (sweep) {
    const bool native = (prm->flags & MCP_FLAG_NATIVE_MATH) != 0;
    SweepSeg segs[4];
    const int n_seg = sweep_plan(K, nb, segs);
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_seg && e == hipSuccess; i++) {
      a.k_begin = segs[i].k_begin;
      a.k_count = segs[i].k_count;
      e = segs[i].shared ? mcp::launch_sweep_shared(nb, segs[i].mt, native, a, ln.stream)
                         : mcp::launch_sweep_paths(nb, segs[i].mt, native, a, ln.stream);
    }
    if (e != hipSuccess) return fail(MCP_E_HIP, "mc_sweep_kernel launch: %s", hipGetErrorString(e));
    if (ln.d_hist) {                           // digit 0 of the select: one lean read of the terminal values just written
      e = mcp::launch_hist(*prm, K, 0, ln.d_terminal, ln.stride, ln.n_paths, nullptr, ln.d_pivot, nullptr, (unsigned long long*)ln.d_hist,
                           ln.stream);
      if (e != hipSuccess) return fail(MCP_E_HIP, "hist_kernel<0> launch: %s", hipGetErrorString(e));
    }
    return MCP_OK;
  }
  if ((!plain || rq.anti) && ln.d_partials && a.slots > (uint64_t)mcp::path_grid(a.n_paths))
    HIP_TRY(mcp::launch_pass0(*prm, K, ln.d_terminal, ln.stride, 0, nullptr, a.slots, (mcp::MomentPartial*)ln.d_partials,
                              (unsigned long long*)ln.d_hist, ln.stream));
  fill_hz(s.hz, rq, ln);
  s.mdd = rq.dd ? ln.d_mdd : nullptr;
  s.mdd_stride = rq.dd ? ln.mdd_stride : 0;
  s.bt = boot_block(rq, ln);
  s.st = student_block(rq);
  if (rq.garch) s.gv = garch_block(rq.gv, N);
  if (rq.cash) s.cf.flows = ln.d_flows;
  if (rq.glide) s.gp = glide_block(rq, ln, N, K);
  if (rq.overlay) s.ov = overlay_block(rq, ln, N);
  if (rq.rebalanced) { s.period = rq.reb->period; s.cost = (float)rq.reb->cost; }
  if (rq.src == SRC_FHS) s.fh = filt_block(rq, ln, N);
  if (rq.jumps) s.jp = jump_block(rq, ln);
  if (rq.regimes) s.rs = regime_block(rq, ln);
  if (rq.protect) s.pi = protect_block(rq, ln);
  mcp::PathKernel k = {};
  k.logc = prm->compounding == MCP_COMPOUND_LOG;
  k.fh = rq.src == SRC_FHS;
  k.boot = rq.src == SRC_BOOT || k.fh;
  k.blds = k.fh ? mcp::filt_fits_lds((uint64_t)rq.filt->n_rows, nb) : k.boot && mcp::boot_fits_lds((uint64_t)rq.boot->n_rows, nb);
  k.stt = rq.src == SRC_T;
  if (ln.attr) {
    // SPEC.md 4.10: one portfolio per pass, no terminal store, its own epilogue.  The walk draws as the GARCH kernel does: without
    // GARCH on alpha = beta = 0, h0 = 1, which is the Gaussian or Student-t call bit for bit (SPEC.md 4.9).
    static const mcp_garch none = {0.0, 0.0, 1.0, 0};
    k.family = mcp::FAM_AT;
    k.stt = k.gv = true;
    a.partials = nullptr;
    a.hist = nullptr;
    if (!rq.garch) s.gv = garch_block(&none, N);
    s.at = attr_block(ln, N);
  } else {
    k.family = rq.overlay ? mcp::FAM_OV : rq.cash ? mcp::FAM_CF : rq.rebalanced ? mcp::FAM_REB : rq.dd ? mcp::FAM_DD : rq.hz ? mcp::FAM_HZ : mcp::FAM_PLAIN;
    k.dd = rq.overlay && rq.dd;
    k.gv = rq.garch;
    k.jp = rq.jumps;
    k.rs = rq.regimes;
    k.gp = rq.glide;
    if (rq.protect) {
      // SPEC.md 4.15: one segmented kernel serves terminal-only and horizon calls.  Gaussian, Student-t and GARCH requests share the
      // GARCH walk, as the attribution does: without GARCH on alpha = beta = 0, h0 = 1
      static const mcp_garch none = {0.0, 0.0, 1.0, 0};
      k.pi = true;
      k.family = rq.dd ? mcp::FAM_DD : mcp::FAM_HZ;
      if (!rq.jumps) {
        k.stt = k.gv = true;
        if (!rq.garch) s.gv = garch_block(&none, N);
      }
    }
    k.kt8 = K > 1;
    k.native = (prm->flags & MCP_FLAG_NATIVE_MATH) != 0;
    k.fold = (prm->flags & MCP_FLAG_FOLD) != 0;
    // the plain Gaussian walk of one portfolio whose paths share the high counter word runs the lean step loop (mcp_paths.h, UHI)
    k.uhi = MCP_EXP_LEAN && plain && !rq.anti && !k.kt8 && !k.native && !k.fold && nb <= mcp::LEAN_MAX_NB && mcp::lean_range(a.path_begin, a.n_paths);
    if (rq.anti) {
      // Student-t and GARCH requests share the GARCH walk, as the attribution does: without GARCH on alpha = beta = 0, h0 = 1
      static const mcp_garch none = {0.0, 0.0, 1.0, 0};
      k.anti = true;
      if (k.stt || k.gv) {
        k.stt = k.gv = true;
        if (!rq.garch) s.gv = garch_block(&none, N);
      }
    }
  }
  const hipError_t e = k_launch[nb - 1](k, s, ln.stream);
  if (e != hipSuccess) return fail(MCP_E_HIP, "path kernel launch (family %d): %s", k.family, hipGetErrorString(e));
  return MCP_OK;
}

static Launch make_launch(const float* d_packed, const double* d_pivot, uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                          float* d_terminal, uint64_t stride, void* d_partials, void* d_hist, void* stream) {
  Launch ln;
  ln.d_packed = d_packed;
  ln.d_pivot = d_pivot;
  ln.seed = seed;
  ln.path_begin = path_begin;
  ln.n_paths = n_paths;
  ln.d_terminal = d_terminal;
  ln.stride = stride;
  ln.d_partials = d_partials;
  ln.d_hist = d_hist;
  ln.stream = (hipStream_t)stream;
  return ln;
}

static int launch_checked(const mcp_params* prm, const Request& rq, const Launch& ln) {
  if (int rc = check_request(prm, rq, ln.n_paths, &ln)) return rc;
  return launch_paths_impl(prm, rq, ln);
}

extern "C" {

int mcp_launch_paths(const mcp_params* prm, const float* d_packed, const double* d_pivot, uint64_t seed, uint64_t path_begin,
                     uint64_t n_paths, float* d_terminal, uint64_t stride, void* d_partials, void* d_hist, void* stream) {
  return launch_checked(prm, Request(), make_launch(d_packed, d_pivot, seed, path_begin, n_paths, d_terminal, stride, d_partials, d_hist, stream));
}

int mcp_launch_paths_drawdown(const mcp_params* prm, const float* d_packed, const double* d_pivot, uint64_t seed, uint64_t path_begin,
                              uint64_t n_paths, float* d_terminal, uint64_t terminal_stride, float* d_mdd, uint64_t mdd_stride,
                              void* d_partials, void* d_hist, void* stream) {
  Request rq;
  rq.dd = true;
  Launch ln = make_launch(d_packed, d_pivot, seed, path_begin, n_paths, d_terminal, terminal_stride, d_partials, d_hist, stream);
  ln.d_mdd = d_mdd;
  ln.mdd_stride = mdd_stride;
  return launch_checked(prm, rq, ln);
}

int mcp_launch_paths_horizons(const mcp_params* prm, const float* d_packed, const double* d_pivot, uint64_t seed, uint64_t path_begin,
                              uint64_t n_paths, float* d_terminal, uint64_t terminal_stride, int n_horizons, const int32_t* horizons,
                              float* d_horizon, uint64_t horizon_stride, void* d_partials, void* d_hist, void* stream) {
  Request rq;
  ask_horizons(rq, true, n_horizons, horizons, 0, nullptr, nullptr, nullptr, nullptr);
  Launch ln = make_launch(d_packed, d_pivot, seed, path_begin, n_paths, d_terminal, terminal_stride, d_partials, d_hist, stream);
  ln.d_hz = d_horizon;
  ln.hz_stride = horizon_stride;
  return launch_checked(prm, rq, ln);
}

// Launches below go to the device that owns the stream.
#define MCP_ON_STREAM_DEVICE(stream)                                                                     \
  int dev_ = 0;                                                                                          \
  if (int rc_ = stream_device((hipStream_t)(stream), &dev_)) return rc_;                                 \
  DeviceGuard guard_(dev_);                                                                              \
  if (guard_.err != hipSuccess) return fail(MCP_E_HIP, "hipSetDevice(%d): %s", dev_, hipGetErrorString(guard_.err))

int mcp_percentile_rank(uint64_t n, double alpha, uint64_t* rank_lo, uint64_t* rank_hi, double* gamma) {
  if (n < 1 || !rank_lo || !rank_hi || !gamma) return fail(MCP_E_ARG, "bad argument");
  // app.py:259  np.percentile(returns, (1-alpha)*100); numpy divides by 100 again, then method
  // 'linear' takes virtual_index = (n - 1) * q  (numpy 2.2 _QuantileMethods['linear']).
  const double pct = (1.0 - alpha) * 100.0;
  const double q = pct / 100.0;
  const double vi = (double)(n - 1) * q;
  if (vi >= (double)(n - 1)) { *rank_lo = *rank_hi = n - 1; *gamma = 0.0; return MCP_OK; }
  if (vi < 0.0) { *rank_lo = *rank_hi = 0; *gamma = 0.0; return MCP_OK; }
  const double fl = std::floor(vi);
  *rank_lo = (uint64_t)fl;
  *rank_hi = *rank_lo + 1;
  *gamma = vi - fl;
  return MCP_OK;
}

int mcp_percentile_rank_q(uint64_t n, double q, uint64_t* rank_lo, uint64_t* rank_hi, double* gamma) {
  if (n < 1 || !rank_lo || !rank_hi || !gamma || !(q >= 0.0 && q <= 100.0)) return fail(MCP_E_ARG, "bad argument");
  // np.percentile(x, q): numpy divides q by 100, then method 'linear' as in mcp_percentile_rank
  const double qq = q / 100.0;
  const double vi = (double)(n - 1) * qq;
  if (vi >= (double)(n - 1)) { *rank_lo = *rank_hi = n - 1; *gamma = 0.0; return MCP_OK; }
  if (vi < 0.0) { *rank_lo = *rank_hi = 0; *gamma = 0.0; return MCP_OK; }
  const double fl = std::floor(vi);
  *rank_lo = (uint64_t)fl;
  *rank_hi = *rank_lo + 1;
  *gamma = vi - fl;
  return MCP_OK;
}

int mcp_launch_pass0(const mcp_params* prm, const float* d_terminal, uint64_t stride, uint64_t n, const double* d_pivot,
                     void* d_partials, void* d_hist, void* stream) {
  if (int rc = check_params(prm)) return rc;
  if (!d_terminal || !d_partials || !d_hist || stride < n) return fail(MCP_E_ARG, "bad argument");
  MCP_ON_STREAM_DEVICE(stream);
  HIP_TRY(mcp::launch_pass0(*prm, prm->n_portfolios, d_terminal, stride, n, d_pivot, mcp_moment_slots(prm->n_portfolios, n),
                            (mcp::MomentPartial*)d_partials, (unsigned long long*)d_hist, (hipStream_t)stream));
  return MCP_OK;
}

int mcp_launch_scan(const mcp_params* prm, int pass, uint64_t n, uint64_t rank_lo, uint64_t rank_hi, const void* d_partials,
                    const void* d_below, const double* d_pivot, void* d_hist, void* d_state, void* d_record, void* stream) {
  if (int rc = check_params(prm)) return rc;
  if (!d_partials || !d_below || !d_hist || !d_state || !d_record || pass < 0 || pass > 1) return fail(MCP_E_ARG, "bad argument");
  MCP_ON_STREAM_DEVICE(stream);
  HIP_TRY(mcp::launch_scan(*prm, prm->n_portfolios, pass, n, rank_lo, rank_hi, mcp_moment_slots(prm->n_portfolios, n),
                           (const mcp::MomentPartial*)d_partials, (const double*)d_below, d_pivot, (unsigned long long*)d_hist,
                           (mcp::SelectState*)d_state, (mcp_record*)d_record, (hipStream_t)stream));
  return MCP_OK;
}

int mcp_launch_hist(const mcp_params* prm, int pass, const float* d_terminal, uint64_t stride, uint64_t n,
                    const void* d_state, const double* d_pivot, void* d_below, void* d_hist, void* stream) {
  if (int rc = check_params(prm)) return rc;
  if (!d_terminal || !d_hist || pass < 0 || pass > 2 || stride < n || (pass > 0 && (!d_state || !d_below)))
    return fail(MCP_E_ARG, "bad argument");
  MCP_ON_STREAM_DEVICE(stream);
  HIP_TRY(mcp::launch_hist(*prm, prm->n_portfolios, pass, d_terminal, stride, n, (const mcp::SelectState*)d_state, d_pivot,
                           (double*)d_below, (unsigned long long*)d_hist, (hipStream_t)stream));
  return MCP_OK;
}

int mcp_launch_final(const mcp_params* prm, uint64_t n, double gamma, uint64_t rank_lo, uint64_t rank_hi,
                     const void* d_below, void* d_hist, const void* d_state, void* d_record, void* d_quant,
                     void* d_stats, void* stream) {
  if (int rc = check_params(prm)) return rc;
  if (!d_below || !d_hist || !d_state || !d_record || !d_quant) return fail(MCP_E_ARG, "NULL device pointer");
  MCP_ON_STREAM_DEVICE(stream);
  HIP_TRY(mcp::launch_final(*prm, prm->n_portfolios, n, gamma, rank_lo, rank_hi, (const double*)d_below,
                            (unsigned long long*)d_hist, (const mcp::SelectState*)d_state, (mcp_record*)d_record,
                            (mcp::Quantile*)d_quant, (mcp_stats*)d_stats, (hipStream_t)stream));
  return MCP_OK;
}

int mcp_launch_stats(const mcp_params* prm, int world, const void* d_gathered, const void* d_quant, void* d_stats,
                     void* stream) {
  if (int rc = check_params(prm)) return rc;
  if (world < 1 || !d_gathered || !d_quant || !d_stats) return fail(MCP_E_ARG, "bad argument");
  MCP_ON_STREAM_DEVICE(stream);
  HIP_TRY(mcp::launch_stats(*prm, prm->n_portfolios, world, (const mcp_record*)d_gathered, (const mcp::Quantile*)d_quant,
                            (mcp_stats*)d_stats, (hipStream_t)stream));
  return MCP_OK;
}

int mcp_launch_sum_u64(void* const* d_bufs, int n_bufs, size_t words, void* stream) {
  if (!d_bufs || n_bufs < 1 || n_bufs > 8) return fail(MCP_E_ARG, "n_bufs=%d outside [1,8]", n_bufs);
  for (int i = 0; i < n_bufs; i++)
    if (!d_bufs[i]) return fail(MCP_E_ARG, "NULL device pointer");
  MCP_ON_STREAM_DEVICE(stream);
  HIP_TRY(mcp::launch_sum_u64((unsigned long long* const*)d_bufs, n_bufs, words, (hipStream_t)stream));
  return MCP_OK;
}

int mcp_stream_create(int device, int reserve_cus, void** out) {
  if (!out) return fail(MCP_E_ARG, "stream_out is NULL");
  *out = nullptr;
  const int n = mcp_device_count();
  if (n <= 0) return fail(MCP_E_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return fail(MCP_E_ARG, "device %d outside [0,%d)", device, n);
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return fail(MCP_E_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(guard.err));
  hipStream_t s = nullptr;
  if (reserve_cus <= 0) {
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  } else {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int cus = prop.multiProcessorCount;
    if (reserve_cus >= cus) return fail(MCP_E_ARG, "reserve_cus=%d leaves none of the %d compute units", reserve_cus, cus);
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
    for (int i = 0; i < cus - reserve_cus; i++) mask[(size_t)i / 32] |= 1u << (i % 32);
    HIP_TRY(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
  }
  *out = (void*)s;
  return MCP_OK;
}

int mcp_stream_destroy(void* stream) {
  if (!stream) return fail(MCP_E_ARG, "stream is NULL");
  HIP_TRY(hipStreamDestroy((hipStream_t)stream));
  return MCP_OK;
}

int mcp_launch_normals(const uint32_t* d_x, uint64_t n, float* d_z, void* stream) {
  if (!d_x || !d_z) return fail(MCP_E_ARG, "NULL device pointer");
  MCP_ON_STREAM_DEVICE(stream);
  const float4* tables = nullptr;
  if (int rc = device_tables(dev_, (hipStream_t)stream, &tables)) return rc;
  HIP_TRY(mcp::launch_normals(d_x, n, tables, d_z, (hipStream_t)stream));
  return MCP_OK;
}

int mcp_icdf_table(float* out, size_t out_len) {
  if (!out || out_len < (size_t)mcp::ICDF_ENTRIES * 4) return fail(MCP_E_ARG, "buffer too small for %d x 4 floats", mcp::ICDF_ENTRIES);
  memcpy(out, k_icdf_table, sizeof k_icdf_table);
  return MCP_OK;
}

uint32_t mcp_float_to_key(float v) { return mcp::float_to_key(v); }
float mcp_key_to_float(uint32_t key) { return mcp::key_to_float(key); }

double mcp_terminal_to_x(const mcp_params* prm, float terminal) {
  if (prm->compounding == MCP_COMPOUND_LOG) return std::expm1((double)terminal);
  return (double)terminal / (double)(float)prm->v0 - 1.0;
}

// ---- host-level context -----------------------------------------------------------------------------

static void free_shard(Shard& sh) {
  (void)hipSetDevice(sh.device);
  if (sh.stream) { (void)hipStreamSynchronize(sh.stream); (void)hipStreamDestroy(sh.stream); }
  if (sh.ev) (void)hipEventDestroy(sh.ev);
  for (int i = 0; i < MCP_WS_COUNT; i++)
    if (sh.ws[i] && i != MCP_WS_STATS) (void)hipFree(sh.ws[i]);
  release(sh.packed);
  release(sh.terminal);
  release(sh.gather);
  release(sh.h_packed);
  release(sh.h_pivot);
  release(sh.stats);
  release(sh.dd.mdd);
  release(sh.dd.stats);
  release(sh.hz.values);
  release(sh.hz.pivot);
  release(sh.hz.h_pivot);
  release(sh.hz.stats);
  release(sh.boot);
  release(sh.cf.flows);
  release(sh.overlay);
  release(sh.cf.counts);
  release(sh.cf.h_counts);
  release(sh.at.in);
  release(sh.at.h_in);
  release(sh.at.partials);
  release(sh.at.records);
  release(sh.at.h_records);
  release(sh.at.contrib);
  release(sh.pr.partials);
  release(sh.pr.cross);
  release(sh.pr.h_cross);
}

int mcp_ctx_create_multi(const int* devices, int ndev, mcp_ctx** out) {
  if (!out) return fail(MCP_E_ARG, "out is NULL");
  *out = nullptr;
  if (!devices || ndev < 1 || ndev > MAX_DEVICES) return fail(MCP_E_ARG, "ndev=%d outside [1,%d]", ndev, MAX_DEVICES);
  const int n = mcp_device_count();
  if (n <= 0) return fail(MCP_E_NODEVICE, "no HIP device visible (the product path has no CPU fallback)");
  bool all_same = true, all_distinct = true;
  for (int i = 0; i < ndev; i++) {
    if (devices[i] < 0 || devices[i] >= n) return fail(MCP_E_ARG, "device %d outside [0,%d)", devices[i], n);
    if (devices[i] != devices[0]) all_same = false;
    for (int j = 0; j < i; j++)
      if (devices[j] == devices[i]) all_distinct = false;
  }
  if (ndev > 1 && !all_same && !all_distinct)
    return fail(MCP_E_UNSUPPORTED, "devices must be all distinct (RCCL) or all the same (logical shards of one GPU)");
  if (ndev > 1 && all_same && ndev > 8) return fail(MCP_E_UNSUPPORTED, "at most 8 logical shards on one device");
  mcp_ctx* c = new (std::nothrow) mcp_ctx;
  if (!c) return fail(MCP_E_NOMEM, "out of host memory");
  struct Restore { int dev = 0; Restore() { (void)hipGetDevice(&dev); } ~Restore() { (void)hipSetDevice(dev); } } restore;   // leave the caller's current device as it was
  c->all_same = ndev > 1 && all_same;
  c->sh.resize((size_t)ndev);
  for (int i = 0; i < ndev; i++) {
    Shard& sh = c->sh[(size_t)i];
    sh.device = devices[i];
    if (hipSetDevice(sh.device) != hipSuccess || hipStreamCreateWithFlags(&sh.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&sh.ev, hipEventDisableTiming) != hipSuccess) {
      mcp_ctx_destroy(c);
      return fail(MCP_E_HIP, "cannot create a stream on device %d", devices[i]);
    }
  }
  const char* force = getenv("MCP_FORCE_RCCL");      // exercise the RCCL path on a one-GPU box
  c->exchange_always = ndev == 1 && force && *force == '1';
  // The communicator / peer mapping is set up by the first path-sharded mcp_simulate (ensure_exchange): a context that
  // only ever shards the PORTFOLIOS needs neither RCCL nor peer access.
  *out = c;
  return MCP_OK;
}

// First path-sharded call of a context with several shards (or MCP_FORCE_RCCL=1): decide how they exchange.
static int ensure_exchange(mcp_ctx* c) {
  if (c->exchange_mode != MCP_EXCHANGE_UNSET) return MCP_OK;
  const int ndev = (int)c->sh.size();
  if (ndev == 1 && !c->exchange_always) { c->exchange_mode = MCP_EXCHANGE_NONE; return MCP_OK; }
  if (c->all_same) { c->same_device = true; c->exchange_mode = MCP_EXCHANGE_KERNEL; return MCP_OK; }
  // RCCL (north_star: the sufficient statistics travel over xGMI through RCCL).  MCP_EXCHANGE=p2p, or a librccl that
  // cannot be loaded / initialised, falls back to the kernel exchange over peer access: device 0 reads and writes the
  // (<= 32 KiB per portfolio) buffers of its peers directly -- the choreography the one-device shards exercise.  The
  // fallback is reported: mcp_ctx_exchange_mode() / mcp_ctx_exchange_note().
  std::vector<int> devices((size_t)ndev);
  for (int i = 0; i < ndev; i++) devices[(size_t)i] = c->sh[(size_t)i].device;
  const char* mode = getenv("MCP_EXCHANGE");
  int rc = (mode && !strcmp(mode, "p2p") && !c->exchange_always) ? fail(MCP_E_COMM, "MCP_EXCHANGE=p2p") : load_rccl(&c->rccl);
  if (rc == MCP_OK) {
    c->comms.assign((size_t)ndev, nullptr);
    const int r = c->rccl->CommInitAll(c->comms.data(), ndev, devices.data());
    if (r != 0) {
      c->comms.clear();
      rc = fail(MCP_E_COMM, "ncclCommInitAll over %d devices: %s", ndev, c->rccl->GetErrorString(r));
      c->rccl = nullptr;
    }
  }
  if (rc == MCP_OK) { c->exchange_mode = MCP_EXCHANGE_RCCL; return MCP_OK; }
  const std::string why = g_err;
  bool peers = ndev > 1 && ndev <= 8 && hipSetDevice(devices[0]) == hipSuccess;
  for (int i = 1; peers && i < ndev; i++) {
    int can = 0;
    peers = hipDeviceCanAccessPeer(&can, devices[0], devices[(size_t)i]) == hipSuccess && can;
    if (peers) {
      const hipError_t e = hipDeviceEnablePeerAccess(devices[(size_t)i], 0);
      peers = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
      (void)hipGetLastError();
    }
  }
  if (!peers) return fail(MCP_E_COMM, "%s; and no peer access from device %d to the others for the kernel exchange", why.c_str(), devices[0]);
  c->rccl = nullptr;
  c->same_device = true;                               // kernel exchange
  c->exchange_mode = MCP_EXCHANGE_P2P;
  c->exchange_note = why;
  return MCP_OK;
}

int mcp_ctx_exchange_mode(const mcp_ctx* c) { return c ? c->exchange_mode : MCP_EXCHANGE_UNSET; }
const char* mcp_ctx_exchange_note(const mcp_ctx* c) { return c ? c->exchange_note.c_str() : ""; }

int mcp_ctx_create(int device, mcp_ctx** out) { return mcp_ctx_create_multi(&device, 1, out); }

int mcp_ctx_device_count(const mcp_ctx* c) { return c ? (int)c->sh.size() : 0; }

int mcp_ctx_set_terminal_budget(mcp_ctx* c, size_t bytes) {
  if (!c || bytes < 4096) return fail(MCP_E_ARG, "bad argument");
  std::lock_guard<std::mutex> lock(c->mu);
  c->terminal_budget = bytes;
  return MCP_OK;
}

void mcp_ctx_destroy(mcp_ctx* c) {
  if (!c) return;
  int prev_dev = 0;
  const bool have_prev = hipGetDevice(&prev_dev) == hipSuccess;
  for (Shard& sh : c->sh)                                  // drain every stream, then the communicators, then the streams
    if (sh.stream) { (void)hipSetDevice(sh.device); (void)hipStreamSynchronize(sh.stream); }
  if (c->rccl)
    for (void* comm : c->comms)
      if (comm) (void)c->rccl->CommDestroy(comm);
  for (Shard& sh : c->sh) free_shard(sh);
  if (c->d_sweep && !c->sh.empty()) { (void)hipSetDevice(c->sh[0].device); (void)hipFree(c->d_sweep); }
  if (c->h_boot) (void)hipHostFree(c->h_boot);
  if (c->h_flows) (void)hipHostFree(c->h_flows);
  if (c->h_overlay) (void)hipHostFree(c->h_overlay);
  if (have_prev) (void)hipSetDevice(prev_dev);
  delete c;
}

namespace {

// What one shard does in one tile of portfolios.
struct Job {
  int k0 = 0, kt = 0;            // portfolios [k0, k0+kt) of the caller's W
  uint64_t p0 = 0, pn = 0;       // paths [p0, p0+pn) relative to path_begin
  bool active = false;
};

#define RCCL_TRY(c, expr)                                                                            \
  do {                                                                                               \
    int r_ = (expr);                                                                                 \
    if (r_ != 0) return fail(MCP_E_COMM, "%s: %s", #expr, (c)->rccl->GetErrorString(r_));            \
  } while (0)

// histogram all-reduce (SUM, u64) over the shards of a path-sharded tile
int exchange_hist(mcp_ctx* c, int kt) {
  const size_t words = (size_t)kt * 2 * MCP_SELECT_BINS;
  const size_t S = c->sh.size();
  if (c->same_device) {
    Shard& s0 = c->sh[0];
    HIP_TRY(hipSetDevice(s0.device));
    unsigned long long* bufs[8];
    for (size_t s = 0; s < S; s++) {
      bufs[s] = (unsigned long long*)c->sh[s].ws[MCP_WS_HIST];
      if (s) { HIP_TRY(hipEventRecord(c->sh[s].ev, c->sh[s].stream)); HIP_TRY(hipStreamWaitEvent(s0.stream, c->sh[s].ev, 0)); }
    }
    HIP_TRY(mcp::launch_sum_u64(bufs, (int)S, words, s0.stream));
    HIP_TRY(hipEventRecord(s0.ev, s0.stream));
    for (size_t s = 1; s < S; s++) HIP_TRY(hipStreamWaitEvent(c->sh[s].stream, s0.ev, 0));
    return MCP_OK;
  }
  RCCL_TRY(c, c->rccl->GroupStart());
  for (size_t s = 0; s < S; s++) {
    void* h = c->sh[s].ws[MCP_WS_HIST];
    const int r = c->rccl->AllReduce(h, h, words, NCCL_UINT64, NCCL_SUM, c->comms[s], c->sh[s].stream);
    if (r != 0) { (void)c->rccl->GroupEnd(); return fail(MCP_E_COMM, "ncclAllReduce (shard %zu): %s", s, c->rccl->GetErrorString(r)); }   // never leave the group open
  }
  RCCL_TRY(c, c->rccl->GroupEnd());
  return MCP_OK;
}

// all-gather of the [kt] records into every shard's d_gather [S][kt] (same device: only shard 0 needs them)
int exchange_records(mcp_ctx* c, int kt) {
  const size_t S = c->sh.size();
  const size_t bytes = (size_t)kt * sizeof(mcp_record);
  if (c->same_device) {
    Shard& s0 = c->sh[0];
    HIP_TRY(hipSetDevice(s0.device));
    for (size_t s = 0; s < S; s++) {
      if (s) { HIP_TRY(hipEventRecord(c->sh[s].ev, c->sh[s].stream)); HIP_TRY(hipStreamWaitEvent(s0.stream, c->sh[s].ev, 0)); }
      HIP_TRY(hipMemcpyAsync((char*)s0.gather.p + s * bytes, c->sh[s].ws[MCP_WS_RECORD], bytes, hipMemcpyDeviceToDevice, s0.stream));
    }
    return MCP_OK;
  }
  RCCL_TRY(c, c->rccl->GroupStart());
  for (size_t s = 0; s < S; s++) {
    const int r = c->rccl->AllGather(c->sh[s].ws[MCP_WS_RECORD], c->sh[s].gather.p, (size_t)kt * (sizeof(mcp_record) / sizeof(double)),
                                     NCCL_FLOAT64, c->comms[s], c->sh[s].stream);
    if (r != 0) { (void)c->rccl->GroupEnd(); return fail(MCP_E_COMM, "ncclAllGather (shard %zu): %s", s, c->rccl->GetErrorString(r)); }
  }
  RCCL_TRY(c, c->rccl->GroupEnd());
  return MCP_OK;
}

// What a select phase reduces: the terminal values, the drawdown array (SPEC.md 5.1; tp carries v0 = 1, rf = 0, no pivot) or
// the horizon array (SPEC.md 5.2; tp carries n_portfolios = H * kt rows, one pivot per row).
enum SelectOf { SEL_TERMINAL, SEL_DRAWDOWN, SEL_HORIZON };

// The select / exchange / record phase of one tile, over the [rows][pn] array of every active shard (rows = tp[s].n_portfolios)
// whose moment partials and digit-0 histogram are in the shard's work buffers: three descents of the radix select, exchanges
// between the steps when the tile is path-sharded (`exchange`), and the [rows] statistics into each shard's mapped host buffer
// (merged on shard 0 when path-sharded); SEL_HORIZON writes them to slot `slot` of h_hz_stats.  When it runs again, on the
// drawdown or the horizons, the histogram exchange that opens it also orders every shard's work after shard 0's copies of the
// previous phase's records (same-device exchange).
int run_select(mcp_ctx* c, const std::vector<mcp_params>& tp, const std::vector<Job>& jobs, bool exchange, uint64_t lo, uint64_t hi,
               double gamma, SelectOf what, int slot = 0) {
  const size_t S = c->sh.size();
  int rc;
  const int kt_x = tp[0].n_portfolios;         // path-sharded tiles: the same rows on every shard
  const auto stats_of = [&](Shard& sh, int rows) -> void* {
    if (what == SEL_DRAWDOWN) return sh.dd.stats.dev;
    if (what == SEL_HORIZON) return (mcp_stats*)sh.hz.stats.dev + (size_t)slot * rows;
    return sh.ws[MCP_WS_STATS];
  };
  for (int pass = 0; pass < 3; pass++) {
    if (exchange && (rc = exchange_hist(c, kt_x))) return rc;
    for (size_t s = 0; s < S; s++) {
      const Job& j = jobs[s];
      if (!j.active) continue;
      Shard& sh = c->sh[s];
      HIP_TRY(hipSetDevice(sh.device));
      const uint64_t stride = j.pn ? j.pn : 1;
      const double* piv = what == SEL_DRAWDOWN ? nullptr : what == SEL_HORIZON ? sh.hz.pivot.p : (const double*)sh.ws[MCP_WS_PIVOT];
      const float* src = what == SEL_DRAWDOWN ? sh.dd.mdd.p : what == SEL_HORIZON ? sh.hz.values.p : sh.terminal.p;
      if (pass < 2) {
        if ((rc = mcp_launch_scan(&tp[s], pass, j.pn, lo, hi, sh.ws[MCP_WS_PARTIALS], sh.ws[MCP_WS_BELOW], piv, sh.ws[MCP_WS_HIST],
                                  sh.ws[MCP_WS_STATE], sh.ws[MCP_WS_RECORD], sh.stream))) return rc;
        if ((rc = mcp_launch_hist(&tp[s], pass + 1, src, stride, j.pn, sh.ws[MCP_WS_STATE], piv, sh.ws[MCP_WS_BELOW],
                                  sh.ws[MCP_WS_HIST], sh.stream))) return rc;
      } else {
        void* stats = exchange ? nullptr : stats_of(sh, tp[s].n_portfolios);
        if ((rc = mcp_launch_final(&tp[s], j.pn, gamma, lo, hi, sh.ws[MCP_WS_BELOW], sh.ws[MCP_WS_HIST], sh.ws[MCP_WS_STATE],
                                   sh.ws[MCP_WS_RECORD], sh.ws[MCP_WS_QUANT], stats, sh.stream)))
          return rc;
      }
    }
  }
  // finish: merged records on shard 0 (path-sharded) or each shard's own records (portfolio-sharded / one shard)
  if (exchange) {
    if ((rc = exchange_records(c, kt_x))) return rc;
    Shard& s0 = c->sh[0];
    HIP_TRY(hipSetDevice(s0.device));
    if ((rc = mcp_launch_stats(&tp[0], (int)S, s0.gather.p, s0.ws[MCP_WS_QUANT], stats_of(s0, kt_x), s0.stream)))
      return rc;
  }
  return MCP_OK;
}

// SPEC.md 5.15: c_k(h) = (S_h + (v0 - S_0) g_k^h) / v0 - 1, g_k = 1 + rf + m (mu_k - rf), mu_k = sum_i W_ki mu_i (i ascending), binary64
// from the binary32 inputs; where g_k <= 0 or the result is not finite, the pivot of the plain call at h steps (mcp_pivots).  K
// portfolios W[0, K); h = T into out_T[k], the H horizons into out_hz[h*K + k].
void protect_pivots(const mcp_params& prm, const mcp_protect* pt, const float* mu, const float* W, int K, int H, const int32_t* steps,
                    double* out_T, double* out_hz) {
  const ProtectConsts pc = protect_consts(pt);
  const double v0 = (double)(float)prm.v0, rf = (double)pc.rf, m = (double)pc.m, s0 = (double)pt->floor[0];
  const int N = prm.n_assets;
  for (int k = 0; k < K; k++) {
    double mk = 0.0;
    for (int i = 0; i < N; i++) mk += (double)W[(size_t)k * N + i] * (double)mu[i];
    const double g = 1.0 + rf + m * (mk - rf);
    for (int h = -1; h < H; h++) {
      const int st = h < 0 ? prm.n_steps : steps[h];
      double c = (((double)pt->floor[st] + (v0 - s0) * std::pow(g, (double)st)) / v0) - 1.0;
      if (!(g > 0.0) || !std::isfinite(c)) {
        c = mk > -1.0 ? std::expm1((double)st * std::log1p(mk)) : 0.0;
        if (!std::isfinite(c)) c = 0.0;
      }
      (h < 0 ? out_T[k] : out_hz[(size_t)h * K + k]) = c;
    }
  }
}

// The [kt] pivots of the portfolios W[0, kt) of a tile (tp.n_portfolios = kt) at T steps (SPEC.md 5): of rebalanced paths from
// the draws' per-asset means rmu (5.4), of bootstrap paths from the row moments bm, bs2 (5.3), else mcp_pivots.
int tile_pivots(const mcp_params& tp, const Request& rq, int T, const float* W, const double* rmu, const double* bm, const double* bs2,
                double* out) {
  if (rq.rebalanced) {
    reb_pivots(tp.n_assets, tp.n_portfolios, T, rq.reb->period, rmu, W, out);
    return MCP_OK;
  }
  if (rq.src == SRC_BOOT) {
    for (int k = 0; k < tp.n_portfolios; k++) out[k] = boot_pivot(tp.compounding, T, bm[k], bs2[k]);
    return MCP_OK;
  }
  if (rq.src == SRC_FHS) {                                   // SPEC.md 5.11: rmu holds mu_i + e_i
    filt_pivots(tp.n_assets, tp.n_portfolios, T, rmu, W, out);
    return MCP_OK;
  }
  mcp_params p = tp;
  p.n_steps = T;
  return mcp_pivots(&p, rq.mu, rq.chol, W, out);
}

// One tile: every active shard simulates its (portfolios x paths) block -- the kernels' epilogue leaves the moment partials
// and the digit-0 histogram -- and the rest of the statistics pipeline runs (run_select).  Drawdown: the path kernels also leave
// the drawdown array, and after the terminal values a pass 0 over it and a second run_select reduce it to dd_stats_out.
// Horizons: the path kernels also leave the [H][kt][pn] horizon array; after the terminal values it is reduced as H*kt rows, once
// at alpha (pass 0 + run_select) and once per level at that level's rank, whose records contribute only their `var`.
int run_tile(mcp_ctx* c, const mcp_params* prm, const Request& rq, uint64_t seed, uint64_t path_begin, uint64_t n_total,
             const std::vector<Job>& jobs, bool exchange) {
  const size_t S = c->sh.size();
  const int N = prm->n_assets;
  uint64_t lo, hi;
  double gamma;
  if (int rc = mcp_percentile_rank(n_total, prm->alpha, &lo, &hi, &gamma)) return rc;
  std::vector<mcp_params> tp(S, *prm);
  int rc;
  // 1a. buffers (steady state: nothing to do)
  for (size_t s = 0; s < S; s++) {
    const Job& j = jobs[s];
    if (!j.active) continue;
    Shard& sh = c->sh[s];
    HIP_TRY(hipSetDevice(sh.device));
    tp[s].n_portfolios = j.kt;
    // jumps: the loadings behind the packed block; regimes: [mu1][L1 row pairs] there
    // glide path: the target blocks of the tile's portfolios there
    const size_t plen = mcp_packed_len(N, j.kt) + (rq.jumps ? (size_t)n4_of(N) : 0) + (rq.regimes ? regime_block_len(N) : 0) +
                        (rq.glide ? glide_len(N, j.kt, rq.gl) : 0) + (rq.protect ? protect_len(prm->n_steps, j.kt, rq.hz ? rq.H : 0) : 0),
                 pn = j.pn ? j.pn : 1;   // protection: the floor schedule and the counts' thresholds there (protect_pack)
    const int rows = rq.hz ? rq.H * j.kt : j.kt;  // horizon calls: the work buffers also serve the H*kt rows of the horizon selects
    for (int w = 0; w < MCP_WS_COUNT; w++) {      // only the histogram and the select state must start zeroed
      const size_t need = std::max(mcp_ws_bytes(w, j.kt, pn), mcp_ws_bytes(w, rows, pn));
      if (w != MCP_WS_STATS && (rc = grow_dev(&sh.ws[w], &sh.ws_cap[w], need, sh.stream, w == MCP_WS_HIST || w == MCP_WS_STATE)))
        return rc;
    }
    if ((rc = grow(sh.packed, plen)) || (rc = grow(sh.terminal, (size_t)j.kt * pn))) return rc;
    if (exchange && (rc = grow(sh.gather, S * (size_t)std::max(j.kt, rows)))) return rc;
    if ((rc = grow(sh.h_packed, plen)) || (rc = grow(sh.h_pivot, (size_t)j.kt)) || (rc = grow_mapped(sh.stats, (size_t)j.kt))) return rc;
    sh.ws[MCP_WS_STATS] = sh.stats.dev;
    if (rq.dd && ((rc = grow(sh.dd.mdd, (size_t)j.kt * pn)) || (rc = grow_mapped(sh.dd.stats, (size_t)j.kt)))) return rc;
    if (rq.hz && ((rc = grow(sh.hz.values, (size_t)rows * pn)) || (rc = grow(sh.hz.pivot, (size_t)rows)) ||
                  (rc = grow(sh.hz.h_pivot, (size_t)rows)) || (rc = grow_mapped(sh.hz.stats, (size_t)(1 + rq.L) * rows))))
      return rc;
    if ((rq.cash || rq.protect) && ((rc = grow(sh.cf.counts, 2 * (size_t)(j.kt + rows))) || (rc = grow(sh.cf.h_counts, 2 * (size_t)(j.kt + rows))))) return rc;
    if (rq.anti && ((rc = grow(sh.pr.partials, (size_t)j.kt * (size_t)mcp::path_grid(pn / 2))) || (rc = grow(sh.pr.cross, (size_t)j.kt)) ||
                    (rc = grow(sh.pr.h_cross, (size_t)j.kt))))
      return rc;
  }
  // 1b. parameters up and the path kernels out, device after device with nothing else in between: every GPU should be
  //     simulating as early as possible.  Shards of a path-sharded tile share one packed block and one pivot vector
  //     (packed once; the pivot is a function of the inputs, identical on every shard by construction).
  const float* shared_packed = nullptr;
  const double* shared_pivot = nullptr;
  const double* shared_hz_pivot = nullptr;
  // bootstrap: no drift and no Cholesky factor in the packed block (only W is read), the pivots of SPEC.md 5.3 from the row
  // moments (computed once per tile); rebalancing: the per-asset means of the draws (SPEC.md 5.4), once per tile
  // filtered rows (SPEC.md 4.11): their drift in the packed block, the Cholesky factor zero
  const bool boot = rq.src == SRC_BOOT, fhs = rq.src == SRC_FHS;
  const std::vector<float> zmu(boot ? N : 0, 0.0f), zchol(boot || fhs ? (size_t)N * N : 0, 0.0f);
  // jumps (SPEC.md 2.5): the compensated drift in the packed block (the pivots keep the drift itself), the loadings behind the block
  std::vector<float> jmu(rq.jumps ? N : 0);
  if (rq.jumps) jump_drift(rq.jp, jump_consts(rq.jp), N, rq.mu, jmu.data());
  // regimes (SPEC.md 2.6): (mu1, chol1) packed as (mu, chol) are, the head of that block behind the packed block
  const size_t n_load = rq.jumps ? (size_t)n4_of(N) : rq.regimes ? regime_block_len(N) : 0;
  std::vector<float> blk1;
  if (rq.regimes) {
    blk1.resize(mcp_packed_len(N, 1));
    if ((rc = mcp_pack_params(N, 1, rq.rs->mu1, rq.rs->chol1, rq.W, blk1.data(), blk1.size()))) return rc;
  }
  const float* mu = boot ? zmu.data() : fhs ? rq.filt->mu : rq.jumps ? jmu.data() : rq.mu;
  const float* chol = boot || fhs ? zchol.data() : rq.chol;
  std::vector<double> bm, bs2, rmu(rq.rebalanced || fhs ? N : 0), cm;
  if (rq.rebalanced) reb_means(N, rq.mu, boot ? rq.boot : nullptr, rmu.data());
  if (fhs) filt_means(N, rq.filt, rmu.data());
  const bool ov_walk = rq.overlay && rq.ov->n_rows > 0;    // no rows: the pivots of the plain call (SPEC.md 5.7)
  for (size_t s = 0; s < S; s++) {
    const Job& j = jobs[s];
    if (!j.active) continue;
    Shard& sh = c->sh[s];
    HIP_TRY(hipSetDevice(sh.device));
    const size_t plen = mcp_packed_len(N, j.kt);
    const size_t n_prot = rq.protect ? protect_len(prm->n_steps, j.kt, rq.hz ? rq.H : 0) : 0;
    const size_t n_tail = rq.glide ? glide_len(N, j.kt, rq.gl) : n_load + n_prot;   // what follows the packed block: loadings, regime 1 or targets; then the floor
    const float* src = sh.h_packed.p;
    const double* psrc = sh.h_pivot.p;
    const double* hpsrc = sh.hz.h_pivot.p;
    if (exchange && shared_packed) {
      src = shared_packed;                                   // same portfolios on every shard: pinned + portable
      psrc = shared_pivot;
      hpsrc = shared_hz_pivot;
    } else {
      const float* Wt = rq.W + (size_t)j.k0 * N;
      if ((rc = mcp_pack_params(N, j.kt, mu, chol, Wt, sh.h_packed.p, plen))) return rc;
      for (size_t i = 0; rq.jumps && i < n_load; i++) sh.h_packed.p[plen + i] = (int)i < N ? (rq.jp->loading ? rq.jp->loading[i] : 1.0f) : 0.0f;
      for (size_t i = 0; rq.regimes && i < n_load; i++) sh.h_packed.p[plen + i] = blk1[i];
      if (boot && !rq.rebalanced) {
        bm.resize((size_t)j.kt);
        bs2.resize((size_t)j.kt);
        boot_moments(N, rq.boot, Wt, j.kt, bm.data(), bs2.data());
      }
      if (rq.protect) {                                      // SPEC.md 4.15 / 5.15: the schedule and thresholds; every pivot in closed form
        protect_pack(prm->n_steps, j.kt, rq.hz ? rq.H : 0, rq.steps, rq.pi, sh.h_packed.p + plen + n_load);
        protect_pivots(*prm, rq.pi, rq.mu, Wt, j.kt, rq.hz ? rq.H : 0, rq.steps, sh.h_pivot.p, sh.hz.h_pivot.p);
      } else if (rq.glide) {                                 // SPEC.md 4.14 / 5.14: the tile's target blocks; one walk gives every pivot
        glide_pack(N, prm->n_portfolios, j.k0, j.kt, rq.gl, sh.h_packed.p + plen);
        cm.resize((size_t)(rq.gl->n_breaks + 1) * j.kt);
        glide_means(N, prm->n_portfolios, j.k0, j.kt, rq.mu, boot ? rq.boot : nullptr, rq.W, rq.gl, cm.data());
        glide_pivots(j.kt, prm->n_steps, rq.gl->n_breaks, rq.gl->breaks, cm.data(), rq.cf->flows, (double)(float)prm->v0, rq.hz ? rq.H : 0,
                     rq.steps, sh.h_pivot.p, sh.hz.h_pivot.p);
      } else if (rq.cash) {                                  // SPEC.md 5.6: one Horner walk gives T and every horizon
        cm.resize((size_t)j.kt);
        cash_means(N, j.kt, rq.mu, boot ? rq.boot : nullptr, Wt, cm.data());
        cash_pivots(j.kt, prm->n_steps, cm.data(), rq.cf->flows, (double)(float)prm->v0, rq.hz ? rq.H : 0, rq.steps, sh.h_pivot.p,
                    sh.hz.h_pivot.p);
      } else if (ov_walk) {                                  // SPEC.md 5.7: one walk gives T and every horizon
        overlay_pivots(N, j.kt, prm->n_steps, rq.ov, rq.mu, Wt, rq.hz ? rq.H : 0, rq.steps, sh.h_pivot.p, sh.hz.h_pivot.p);
      } else if (rq.regimes) {                               // SPEC.md 5.13: one recursion gives T and every horizon
        regime_pivots(N, j.kt, prm->n_steps, rq.mu, rq.rs->mu1, regime_consts(rq.rs), Wt, rq.hz ? rq.H : 0, rq.steps, sh.h_pivot.p,
                      sh.hz.h_pivot.p);
      } else if ((rc = tile_pivots(tp[s], rq, prm->n_steps, Wt, rmu.data(), bm.data(), bs2.data(), sh.h_pivot.p))) return rc;
      for (int h = 0; rq.hz && !rq.cash && !ov_walk && !rq.regimes && !rq.protect && h < rq.H; h++)                // SPEC.md 5.2 / 5.3: row h*kt + k is pivoted with n_steps = h
        if ((rc = tile_pivots(tp[s], rq, rq.steps[h], Wt, rmu.data(), bm.data(), bs2.data(), sh.hz.h_pivot.p + (size_t)h * j.kt)))
          return rc;
      if (exchange) { shared_packed = sh.h_packed.p; shared_pivot = sh.h_pivot.p; shared_hz_pivot = sh.hz.h_pivot.p; }
    }
    HIP_TRY(hipMemcpyAsync(sh.packed.p, src, (plen + n_tail) * sizeof(float), hipMemcpyHostToDevice, sh.stream));
    HIP_TRY(hipMemcpyAsync(sh.ws[MCP_WS_PIVOT], psrc, (size_t)j.kt * sizeof(double), hipMemcpyHostToDevice, sh.stream));
    if (rq.hz) HIP_TRY(hipMemcpyAsync(sh.hz.pivot.p, hpsrc, (size_t)rq.H * j.kt * sizeof(double), hipMemcpyHostToDevice, sh.stream));
    if (j.pn) {
      Launch ln = make_launch(sh.packed.p, (const double*)sh.ws[MCP_WS_PIVOT], seed, path_begin + j.p0, j.pn, sh.terminal.p, j.pn,
                              sh.ws[MCP_WS_PARTIALS], sh.ws[MCP_WS_HIST], sh.stream);
      ln.d_mdd = sh.dd.mdd.p;
      ln.mdd_stride = j.pn;
      ln.d_hz = sh.hz.values.p;
      ln.hz_stride = j.pn;
      ln.d_rows = sh.boot.p;
      ln.d_flows = sh.cf.flows.p;
      ln.d_overlay = sh.overlay.p;
      ln.d_loading = sh.packed.p + plen;
      ln.d_block1 = sh.packed.p + plen;
      ln.d_targets = sh.packed.p + plen;
      ln.d_floor = sh.packed.p + plen + n_load;
      ln.d_cross = sh.pr.partials.p;
      if ((rc = launch_paths_impl(&tp[s], rq, ln))) return rc;
      if (rq.anti) {                                         // SPEC.md 5.10: the workgroups' cross partials in block order
        HIP_TRY(mcp::launch_attr_merge(sh.pr.partials.p, j.kt, mcp::path_grid(j.pn / 2), 1, sh.pr.cross.p, sh.stream));
        HIP_TRY(hipMemcpyAsync(sh.pr.h_cross.p, sh.pr.cross.p, (size_t)j.kt * sizeof(double), hipMemcpyDeviceToHost, sh.stream));
      }
      if (rq.cash) {                                         // SPEC.md 5.6: the ruined and the short paths of every stored row
        const size_t rows_hz = rq.hz ? (size_t)rq.H * j.kt : 0;
        const bool tg = rq.cf->has_target != 0;
        const float g32 = tg ? (float)rq.cf->target : 0.0f;
        HIP_TRY(mcp::launch_zero(sh.cf.counts.p, 2 * ((size_t)j.kt + rows_hz) * sizeof(unsigned long long), sh.stream));
        HIP_TRY(mcp::launch_count_rows(sh.terminal.p, j.pn, j.pn, j.kt, tg, g32, sh.cf.counts.p, sh.stream));
        if (rows_hz)
          HIP_TRY(mcp::launch_count_rows(sh.hz.values.p, j.pn, j.pn, (int)rows_hz, tg, g32, sh.cf.counts.p + 2 * (size_t)j.kt, sh.stream));
      }
      if (rq.protect) {                                      // SPEC.md 5.15: the paths below the floor and below the target, every stored row
        const size_t rows_hz = rq.hz ? (size_t)rq.H * j.kt : 0;
        const float* thr = ln.d_floor + prm->n_steps + 1;
        HIP_TRY(mcp::launch_zero(sh.cf.counts.p, 2 * ((size_t)j.kt + rows_hz) * sizeof(unsigned long long), sh.stream));
        HIP_TRY(mcp::launch_count_below(sh.terminal.p, j.pn, j.pn, j.kt, thr, sh.cf.counts.p, sh.stream));
        if (rows_hz)
          HIP_TRY(mcp::launch_count_below(sh.hz.values.p, j.pn, j.pn, (int)rows_hz, thr + 2 * (size_t)j.kt, sh.cf.counts.p + 2 * (size_t)j.kt,
                                          sh.stream));
      }
    } else {
      // a shard without paths (fewer paths than shards): empty moment partials, nothing in the histogram
      if ((rc = mcp_launch_pass0(&tp[s], sh.terminal.p, 1, 0, (const double*)sh.ws[MCP_WS_PIVOT], sh.ws[MCP_WS_PARTIALS],
                                 sh.ws[MCP_WS_HIST], sh.stream))) return rc;
    }
  }
  // 2. the terminal values' select, exchanges and records
  if ((rc = run_select(c, tp, jobs, exchange, lo, hi, gamma, SEL_TERMINAL))) return rc;
  // 3. drawdown (SPEC.md 5.1): the same pipeline over q / d -- x = q - 1 (simple, v0 = 1) or expm1(d) (log), no pivot, no rf
  if (rq.dd) {
    std::vector<mcp_params> tpd(tp);
    for (size_t s = 0; s < S; s++) {
      tpd[s].v0 = 1.0;
      tpd[s].rf = 0.0;
      const Job& j = jobs[s];
      if (!j.active) continue;
      Shard& sh = c->sh[s];
      HIP_TRY(hipSetDevice(sh.device));
      if ((rc = mcp_launch_pass0(&tpd[s], sh.dd.mdd.p, j.pn ? j.pn : 1, j.pn, nullptr, sh.ws[MCP_WS_PARTIALS], sh.ws[MCP_WS_HIST],
                                 sh.stream)))
        return rc;
    }
    if ((rc = run_select(c, tpd, jobs, exchange, lo, hi, gamma, SEL_DRAWDOWN))) return rc;
  }
  // 4. horizons (SPEC.md 5.2): the H*kt rows of the horizon array, at alpha and at every level's rank
  if (rq.hz) {
    std::vector<mcp_params> tph(tp);
    for (size_t s = 0; s < S; s++)
      if (jobs[s].active) tph[s].n_portfolios = rq.H * jobs[s].kt;
    for (int l = -1; l < rq.L; l++) {
      uint64_t qlo = lo, qhi = hi;
      double qg = gamma;
      if (l >= 0 && (rc = mcp_percentile_rank_q(n_total, rq.levels[l], &qlo, &qhi, &qg))) return rc;
      for (size_t s = 0; s < S; s++) {
        const Job& j = jobs[s];
        if (!j.active) continue;
        Shard& sh = c->sh[s];
        HIP_TRY(hipSetDevice(sh.device));
        if ((rc = mcp_launch_pass0(&tph[s], sh.hz.values.p, j.pn ? j.pn : 1, j.pn, sh.hz.pivot.p, sh.ws[MCP_WS_PARTIALS],
                                   sh.ws[MCP_WS_HIST], sh.stream))) return rc;
      }
      if ((rc = run_select(c, tph, jobs, exchange, qlo, qhi, qg, SEL_HORIZON, l + 1))) return rc;
    }
  }
  for (size_t s = 0; s < S; s++) {
    const Job& j = jobs[s];
    if (!j.active || !j.pn) continue;
    Shard& sh = c->sh[s];
    HIP_TRY(hipSetDevice(sh.device));
    // the records are already in host memory when the stream drains: ws[MCP_WS_STATS] is the mapped sh.stats
    const auto copy_out = [&](float* out, const float* d) {   // [kt][pn] block -> rows k0.. of the [K][n_total] array at column p0
      return hipMemcpy2DAsync(out + (size_t)j.k0 * n_total + j.p0, n_total * sizeof(float), d, j.pn * sizeof(float),
                              j.pn * sizeof(float), (size_t)j.kt, hipMemcpyDeviceToHost, sh.stream);
    };
    if (rq.terminal_out) HIP_TRY(copy_out(rq.terminal_out, sh.terminal.p));
    if (rq.dd && rq.mdd_out) HIP_TRY(copy_out(rq.mdd_out, sh.dd.mdd.p));
    if (rq.hz && rq.hz_out)
      for (int h = 0; h < rq.H; h++)
        HIP_TRY(copy_out(rq.hz_out + (size_t)h * prm->n_portfolios * n_total, sh.hz.values.p + (size_t)h * j.kt * j.pn));
    if (rq.cash || rq.protect)
      HIP_TRY(hipMemcpyAsync(sh.cf.h_counts.p, sh.cf.counts.p, 2 * (size_t)((rq.hz ? 1 + rq.H : 1) * j.kt) * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, sh.stream));
  }
  for (size_t s = 0; s < S; s++)
    if (jobs[s].active) { HIP_TRY(hipSetDevice(c->sh[s].device)); HIP_TRY(hipStreamSynchronize(c->sh[s].stream)); }
  for (size_t s = 0; (rq.cash || rq.protect) && s < S; s++) {   // the counts of every shard that walked paths add up (zeroed per call)
    const Job& j = jobs[s];
    if (!j.active || !j.pn) continue;
    const unsigned long long* hc = c->sh[s].cf.h_counts.p;
    for (int k = 0; k < j.kt; k++)
      for (int i = 0; i < 2; i++) {
        rq.counts_out[2 * (size_t)(j.k0 + k) + i] += hc[2 * (size_t)k + i];
        for (int h = 0; rq.hz && h < rq.H; h++)
          rq.hz_counts_out[2 * ((size_t)h * prm->n_portfolios + j.k0 + k) + i] += hc[2 * ((size_t)j.kt + (size_t)h * j.kt + k) + i];
      }
  }
  for (size_t s = 0; rq.anti && s < S; s++) {              // the cross sums of every shard that walked pairs, in shard order
    const Job& j = jobs[s];
    if (!j.active || !j.pn) continue;
    for (int k = 0; k < j.kt; k++) rq.cross_out[j.k0 + k] += c->sh[s].pr.h_cross.p[k];
  }
  for (size_t s = 0; s < S; s++) {
    const Job& j = jobs[s];
    if (!j.active || (exchange && s != 0)) continue;
    const Shard& sh = c->sh[s];
    memcpy(rq.stats_out + j.k0, sh.stats.p, (size_t)j.kt * sizeof(mcp_stats));
    if (rq.dd) {
      memcpy(rq.dd_stats_out + j.k0, sh.dd.stats.p, (size_t)j.kt * sizeof(mcp_stats));
      for (int k = 0; k < j.kt; k++) rq.dd_stats_out[j.k0 + k].sharpe = 0.0;
    }
    if (rq.hz) {                                         // slot 0: the records at alpha; slot 1 + l: level l's quantile (var)
      const int rows = rq.H * j.kt;
      for (int h = 0; h < rq.H; h++)
        for (int k = 0; k < j.kt; k++) {
          const size_t o = (size_t)h * prm->n_portfolios + j.k0 + k, r = (size_t)h * j.kt + k;
          rq.hz_stats_out[o] = sh.hz.stats.p[r];
          rq.hz_stats_out[o].sharpe = 0.0;
          for (int l = 0; l < rq.L; l++) rq.bands_out[o * rq.L + l] = sh.hz.stats.p[(size_t)(1 + l) * rows + r].var;
        }
    }
  }
  return MCP_OK;
}

// Portfolios per tile so that kt * n_paths * bytes_per_path fits the budget (4 B of V_T, 8 B with the drawdown array,
// 4 (1 + H) B with H horizons): whole
// 512-portfolio workgroups of the MFMA sweep kernel when K is tiled at all.
int tile_portfolios(size_t budget, uint64_t n_paths, int K, size_t bytes_per_path = sizeof(float)) {
  const uint64_t fit = budget / (bytes_per_path * (n_paths ? n_paths : 1));
  if (fit >= (uint64_t)K) return K;
  if (fit >= (uint64_t)K_PAD) return (int)(fit / K_PAD) * K_PAD;
  return fit >= 1 ? (int)fit : 1;
}

// SPEC.md 4.10 / 5.9: the second walk of an attribution call, after the call's statistics are in rq.stats_out.  Every shard walks
// its path range again, one portfolio per pass, and leaves one record of sums per workgroup; a small kernel adds them in block order,
// the host adds the shards' records in shard order and divides once.
int run_attribution(mcp_ctx* c, const mcp_params* prm, const Request& rq, uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                    const std::vector<Job>& jobs) {
  const size_t S = c->sh.size();
  const int N = prm->n_assets, K = prm->n_portfolios, n4 = n4_of(N), RL = mcp::attr_record_len(n4);
  const size_t plen = mcp_packed_len(N, K);
  int rc;
  for (size_t s = 0; s < S; s++) {
    const Job& j = jobs[s];
    if (!j.pn) continue;
    Shard& sh = c->sh[s];
    HIP_TRY(hipSetDevice(sh.device));
    const size_t grid = (size_t)mcp::path_grid(j.pn);
    if ((rc = grow(sh.packed, plen)) || (rc = grow(sh.h_packed, plen)) || (rc = grow(sh.at.in, 2 * (size_t)K)) ||
        (rc = grow(sh.at.h_in, 2 * (size_t)K)) || (rc = grow(sh.at.partials, (size_t)K * grid * RL)) ||
        (rc = grow(sh.at.records, (size_t)K * RL)) || (rc = grow(sh.at.h_records, (size_t)K * RL)))
      return rc;
    if (rq.contrib_out && (rc = grow(sh.at.contrib, (size_t)K * N * j.pn))) return rc;
    if ((rc = mcp_pack_params(N, K, rq.mu, rq.chol, rq.W, sh.h_packed.p, plen))) return rc;
    for (int k = 0; k < K; k++) sh.at.h_in.p[k] = rq.stats_out[k].var;
    if ((rc = mcp_pivots(prm, rq.mu, rq.chol, rq.W, sh.at.h_in.p + K))) return rc;
    HIP_TRY(hipMemcpyAsync(sh.packed.p, sh.h_packed.p, plen * sizeof(float), hipMemcpyHostToDevice, sh.stream));
    HIP_TRY(hipMemcpyAsync(sh.at.in.p, sh.at.h_in.p, 2 * (size_t)K * sizeof(double), hipMemcpyHostToDevice, sh.stream));
    Launch ln = make_launch(sh.packed.p, sh.at.in.p + K, seed, path_begin + j.p0, j.pn, nullptr, j.pn, nullptr, nullptr, sh.stream);
    ln.attr = true;
    ln.d_var = sh.at.in.p;
    ln.d_attr_partials = sh.at.partials.p;
    ln.d_contrib = rq.contrib_out ? sh.at.contrib.p : nullptr;
    ln.contrib_stride = j.pn;
    if ((rc = launch_paths_impl(prm, rq, ln))) return rc;
    HIP_TRY(mcp::launch_attr_merge(sh.at.partials.p, K, (int)grid, RL, sh.at.records.p, sh.stream));
    HIP_TRY(hipMemcpyAsync(sh.at.h_records.p, sh.at.records.p, (size_t)K * RL * sizeof(double), hipMemcpyDeviceToHost, sh.stream));
    if (rq.contrib_out)                                    // [K N][pn] block -> the [K][N][n_paths] array at column p0
      HIP_TRY(hipMemcpy2DAsync(rq.contrib_out + j.p0, n_paths * sizeof(float), sh.at.contrib.p, j.pn * sizeof(float), j.pn * sizeof(float),
                               (size_t)K * N, hipMemcpyDeviceToHost, sh.stream));
  }
  for (size_t s = 0; s < S; s++)
    if (jobs[s].pn) { HIP_TRY(hipSetDevice(c->sh[s].device)); HIP_TRY(hipStreamSynchronize(c->sh[s].stream)); }
  const double v0d = (double)(float)prm->v0;
  std::vector<double> rec((size_t)RL);
  for (int k = 0; k < K; k++) {
    std::fill(rec.begin(), rec.end(), 0.0);
    for (size_t s = 0; s < S; s++)                         // shard order
      if (jobs[s].pn)
        for (int i = 0; i < RL; i++) rec[i] += c->sh[s].at.h_records.p[(size_t)k * RL + i];
    const double n = rec[0], n_tail = rec[1], s1 = rec[2], sd = rq.stats_out[k].std;
    rq.attr_counts_out[2 * k] = (uint64_t)n;
    rq.attr_counts_out[2 * k + 1] = (uint64_t)n_tail;
    for (int i = 0; i < N; i++) {
      mcp_attr& o = rq.attr_out[(size_t)k * N + i];
      o.sum = rec[mcp::ATTR_HEAD + 3 * i];
      o.sum_tail = rec[mcp::ATTR_HEAD + 3 * i + 1];
      o.sum_xc = rec[mcp::ATTR_HEAD + 3 * i + 2];
      o.mean = n > 0 ? o.sum / (v0d * n) : 0.0;
      o.cvar = n_tail > 0 ? o.sum_tail / (v0d * n_tail) : 0.0;
      const double cov = n > 1 ? (o.sum_xc - o.sum * s1 / n) / (v0d * (n - 1.0)) : 0.0;
      o.vol = sd > 0.0 ? cov / sd : 0.0;
    }
  }
  return MCP_OK;
}

// A checked request (check_request) on the shards of a context.
int simulate_impl(mcp_ctx* c, const mcp_params* prm, const Request& rq, uint64_t seed, uint64_t path_begin, uint64_t n_paths) {
  if (!c) return fail(MCP_E_ARG, "ctx is NULL");
  const size_t bytes_per_path = rq.hz ? (1 + (size_t)rq.H) * sizeof(float) : rq.dd ? 2 * sizeof(float) : sizeof(float);
  std::lock_guard<std::mutex> lock(c->mu);
  const size_t S = c->sh.size();
  const int K = prm->n_portfolios;
  int prev_dev = 0;
  (void)hipGetDevice(&prev_dev);
  int rc = MCP_OK;
  std::vector<Job> jobs(S);
  const bool by_portfolio = S > 1 && (prm->flags & MCP_FLAG_SHARD_PORTFOLIOS);
  if (rq.src == SRC_BOOT || rq.src == SRC_FHS) {
    // SPEC.md 2.1: the rows, zero-padded to N4, into one pinned staging copy and from there once into the boot buffer of every
    // shard that walks paths in this call (the tiles of the call share it).  SPEC.md 2.4: the shocks of filtered rows behind them,
    // zero-padded to a multiple of 4
    const int N = prm->n_assets, n4 = n4_of(N);
    const mcp_bootstrap tab = rows_of(rq);
    const size_t R = tab.n_rows, n_shock = rq.src == SRC_FHS ? (R + 3) / 4 * 4 : 0, bytes = (R * (size_t)n4 + n_shock) * sizeof(float);
    rc = grow_host((void**)&c->h_boot, &c->h_boot_cap, bytes);
    if (rc == MCP_OK) {
      memset(c->h_boot, 0, bytes);
      for (size_t j = 0; j < R; j++) memcpy(c->h_boot + j * n4, tab.rows + j * N, (size_t)N * sizeof(float));
      if (n_shock) memcpy(c->h_boot + R * n4, rq.filt->shock, R * sizeof(float));
    }
    for (size_t s = 0; s < S && rc == MCP_OK; s++) {
      const bool works = by_portfolio ? (int64_t)K * (int64_t)(s + 1) / (int64_t)S > (int64_t)K * (int64_t)s / (int64_t)S
                                      : n_paths / S + (s < n_paths % S ? 1 : 0) > 0;
      if (!works) continue;
      Shard& sh = c->sh[s];
      if (hipSetDevice(sh.device) != hipSuccess) { rc = fail(MCP_E_HIP, "hipSetDevice(%d)", sh.device); break; }
      if ((rc = grow(sh.boot, R * (size_t)n4 + n_shock))) break;
      const hipError_t e = hipMemcpyAsync(sh.boot.p, c->h_boot, bytes, hipMemcpyHostToDevice, sh.stream);
      if (e != hipSuccess) rc = fail(MCP_E_HIP, "bootstrap rows upload: %s", hipGetErrorString(e));
    }
  }
  if (rc == MCP_OK && rq.cash) {
    // SPEC.md 4.7: the schedule into one pinned staging copy and from there once into the flows buffer of every shard (the tiles
    // of the call share it); the counts of the call start at zero, every tile and shard adds its own
    const size_t T = (size_t)prm->n_steps, bytes = T * sizeof(float);
    memset(rq.counts_out, 0, 2 * (size_t)K * sizeof(uint64_t));
    if (rq.hz) memset(rq.hz_counts_out, 0, 2 * (size_t)rq.H * K * sizeof(uint64_t));
    rc = grow_host((void**)&c->h_flows, &c->h_flows_cap, bytes ? bytes : sizeof(float));
    if (rc == MCP_OK && bytes) memcpy(c->h_flows, rq.cf->flows, bytes);
    for (size_t s = 0; s < S && rc == MCP_OK; s++) {
      Shard& sh = c->sh[s];
      if (hipSetDevice(sh.device) != hipSuccess) { rc = fail(MCP_E_HIP, "hipSetDevice(%d)", sh.device); break; }
      if ((rc = grow(sh.cf.flows, T ? T : 1)) || !bytes) continue;
      const hipError_t e = hipMemcpyAsync(sh.cf.flows.p, c->h_flows, bytes, hipMemcpyHostToDevice, sh.stream);
      if (e != hipSuccess) rc = fail(MCP_E_HIP, "cash-flow schedule upload: %s", hipGetErrorString(e));
    }
  }
  if (rc == MCP_OK && rq.protect) {                          // SPEC.md 5.15: the counts of the call start at zero, every tile and shard adds its own
    memset(rq.counts_out, 0, 2 * (size_t)K * sizeof(uint64_t));
    if (rq.hz) memset(rq.hz_counts_out, 0, 2 * (size_t)rq.H * K * sizeof(uint64_t));
  }
  if (rc == MCP_OK && rq.overlay) {
    // SPEC.md 4.8: the table into one pinned staging copy and from there once into the overlay buffer of every shard (the tiles
    // of the call share it)
    const size_t bytes = overlay_bytes(prm->n_assets, rq.ov->n_rows);
    rc = grow_host((void**)&c->h_overlay, &c->h_overlay_cap, bytes);
    if (rc == MCP_OK) overlay_pack(prm->n_assets, rq.ov, c->h_overlay);
    for (size_t s = 0; s < S && rc == MCP_OK; s++) {
      Shard& sh = c->sh[s];
      if (hipSetDevice(sh.device) != hipSuccess) { rc = fail(MCP_E_HIP, "hipSetDevice(%d)", sh.device); break; }
      if ((rc = grow(sh.overlay, bytes))) break;
      const hipError_t e = hipMemcpyAsync(sh.overlay.p, c->h_overlay, bytes, hipMemcpyHostToDevice, sh.stream);
      if (e != hipSuccess) rc = fail(MCP_E_HIP, "overlay table upload: %s", hipGetErrorString(e));
    }
  }
  if (rc == MCP_OK && by_portfolio) {
    // every shard walks all paths for its slice of W; slices are tiled independently; no exchange
    std::vector<int> kb(S + 1);
    for (size_t s = 0; s <= S; s++) kb[s] = (int)((int64_t)K * (int64_t)s / (int64_t)S);
    std::vector<int> done(S, 0);
    for (bool more = true; more && rc == MCP_OK;) {
      more = false;
      for (size_t s = 0; s < S; s++) {
        const int left = kb[s + 1] - kb[s] - done[s];
        jobs[s] = Job();
        if (left <= 0) continue;
        const int kt = std::min(left, tile_portfolios(c->terminal_budget, n_paths, left, bytes_per_path));
        jobs[s].k0 = kb[s] + done[s]; jobs[s].kt = kt; jobs[s].p0 = 0; jobs[s].pn = n_paths; jobs[s].active = true;
        done[s] += kt;
        more = true;
      }
      if (more) rc = run_tile(c, prm, rq, seed, path_begin, n_paths, jobs, false);
    }
  } else if (rc == MCP_OK) {
    // the path range is sharded; all shards see the same tile of portfolios
    uint64_t pn_max = 0;
    const uint64_t unit = rq.anti ? 2 : 1, n_units = n_paths / unit;   // antithetic pairs: the range is cut at even ids (SPEC.md 2.3)
    for (size_t s = 0; s < S; s++) {
      jobs[s].p0 = unit * (n_units / S * s + std::min<uint64_t>(s, n_units % S));
      jobs[s].pn = unit * (n_units / S + (s < n_units % S ? 1 : 0));
      jobs[s].active = true;
      pn_max = std::max(pn_max, jobs[s].pn);
    }
    const int kt_max = tile_portfolios(c->terminal_budget, pn_max, K, bytes_per_path);
    rc = ensure_exchange(c);
    for (int k0 = 0; k0 < K && rc == MCP_OK; k0 += kt_max) {
      for (size_t s = 0; s < S; s++) { jobs[s].k0 = k0; jobs[s].kt = std::min(kt_max, K - k0); }
      rc = run_tile(c, prm, rq, seed, path_begin, n_paths, jobs, S > 1 || c->exchange_always);
    }
    if (rc == MCP_OK && rq.attr) rc = run_attribution(c, prm, rq, seed, path_begin, n_paths, jobs);
  }
  if (rc != MCP_OK) {
    // Leave no work in flight behind a failed call, and restore the invariant of the read-and-clear protocol: a pass that
    // stopped half way may have left counts in the histograms, and the next call would add to them.  (Every select of a
    // drawdown or horizon call -- terminal values, drawdowns, horizon rows -- shares these buffers.)
    const std::string why = g_err;
    for (Shard& sh : c->sh) { (void)hipSetDevice(sh.device); (void)hipStreamSynchronize(sh.stream); }
    for (Shard& sh : c->sh) {
      (void)hipSetDevice(sh.device);
      for (int w : {MCP_WS_HIST, MCP_WS_STATE})
        if (sh.ws[w]) (void)mcp::launch_zero(sh.ws[w], (sh.ws_cap[w] + 7) & ~(size_t)7, sh.stream);
      (void)hipStreamSynchronize(sh.stream);
    }
    (void)hipGetLastError();
    g_err = why;
  }
  (void)hipSetDevice(prev_dev);
  return rc;
}

// Every public simulate entry point: the request is checked in full before the context is looked at.
int simulate_checked(mcp_ctx* c, const mcp_params* prm, const Request& rq, uint64_t seed, uint64_t path_begin, uint64_t n_paths) {
  if (int rc = check_request(prm, rq, n_paths, nullptr, path_begin)) return rc;
  return simulate_impl(c, prm, rq, seed, path_begin, n_paths);
}

}  // namespace

int mcp_simulate(mcp_ctx* c, const mcp_params* prm, const float* mu, const float* chol, const float* W,
                 uint64_t seed, uint64_t path_begin, uint64_t n_paths, float* terminal_out, mcp_stats* stats_out) {
  if (!c) return fail(MCP_E_ARG, "ctx is NULL");   // mcp_simulate and mcp_simulate_drawdown look at the context first (ABI 1)
  return simulate_checked(c, prm, host_request(SRC_GAUSS, mu, chol, W, terminal_out, stats_out), seed, path_begin, n_paths);
}

int mcp_simulate_drawdown(mcp_ctx* c, const mcp_params* prm, const float* mu, const float* chol, const float* W, uint64_t seed,
                          uint64_t path_begin, uint64_t n_paths, float* terminal_out, mcp_stats* stats_out, float* mdd_out,
                          mcp_stats* dd_stats_out) {
  if (!c) return fail(MCP_E_ARG, "ctx is NULL");
  Request rq = host_request(SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.dd = true;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_horizons(mcp_ctx* c, const mcp_params* prm, const float* mu, const float* chol, const float* W, uint64_t seed,
                          uint64_t path_begin, uint64_t n_paths, int n_horizons, const int32_t* horizons, int n_levels,
                          const double* levels, float* terminal_out, mcp_stats* stats_out, float* horizon_out,
                          mcp_stats* hz_stats_out, double* bands_out) {
  Request rq = host_request(SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  ask_horizons(rq, true, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_bootstrap(mcp_ctx* c, const mcp_params* prm, const mcp_bootstrap* boot, const float* W, uint64_t seed,
                           uint64_t path_begin, uint64_t n_paths, float* terminal_out, mcp_stats* stats_out) {
  Request rq = host_request(SRC_BOOT, nullptr, nullptr, W, terminal_out, stats_out);
  rq.boot = boot;
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_bootstrap_horizons(mcp_ctx* c, const mcp_params* prm, const mcp_bootstrap* boot, const float* W, uint64_t seed,
                                    uint64_t path_begin, uint64_t n_paths, int n_horizons, const int32_t* horizons, int n_levels,
                                    const double* levels, float* terminal_out, mcp_stats* stats_out, float* horizon_out,
                                    mcp_stats* hz_stats_out, double* bands_out) {
  Request rq = host_request(SRC_BOOT, nullptr, nullptr, W, terminal_out, stats_out);
  rq.boot = boot;
  ask_horizons(rq, true, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_rebalanced(mcp_ctx* c, const mcp_params* prm, const mcp_rebalance* reb, const float* mu, const float* chol,
                            const mcp_bootstrap* boot, const float* W, uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                            int n_horizons, const int32_t* horizons, int n_levels, const double* levels, float* terminal_out,
                            mcp_stats* stats_out, float* horizon_out, mcp_stats* hz_stats_out, double* bands_out) {
  Request rq = host_request(boot ? SRC_BOOT : SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.boot = boot;
  rq.rebalanced = true;
  rq.reb = reb;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_student_t(mcp_ctx* c, const mcp_params* prm, const mcp_student_t* st, const float* mu, const float* chol,
                           const float* W, uint64_t seed, uint64_t path_begin, uint64_t n_paths, int n_horizons, const int32_t* horizons,
                           int n_levels, const double* levels, float* terminal_out, mcp_stats* stats_out, float* mdd_out,
                           mcp_stats* dd_stats_out, float* horizon_out, mcp_stats* hz_stats_out, double* bands_out) {
  Request rq = host_request(SRC_T, mu, chol, W, terminal_out, stats_out);
  rq.st = st;
  rq.dd = dd_stats_out != nullptr;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_garch(mcp_ctx* c, const mcp_params* prm, const mcp_garch* g, const mcp_student_t* st, const float* mu,
                       const float* chol, const float* W, uint64_t seed, uint64_t path_begin, uint64_t n_paths, int n_horizons,
                       const int32_t* horizons, int n_levels, const double* levels, float* terminal_out, mcp_stats* stats_out,
                       float* mdd_out, mcp_stats* dd_stats_out, float* horizon_out, mcp_stats* hz_stats_out, double* bands_out) {
  Request rq = host_request(st ? SRC_T : SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.st = st;
  rq.garch = true;
  rq.gv = g;
  rq.dd = dd_stats_out != nullptr;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_jumps(mcp_ctx* c, const mcp_params* prm, const mcp_jumps* j, const float* mu, const float* chol, const float* W,
                       uint64_t seed, uint64_t path_begin, uint64_t n_paths, int n_horizons, const int32_t* horizons, int n_levels,
                       const double* levels, float* terminal_out, mcp_stats* stats_out, float* mdd_out, mcp_stats* dd_stats_out,
                       float* horizon_out, mcp_stats* hz_stats_out, double* bands_out) {
  Request rq = host_request(SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.jumps = true;
  rq.jp = j;
  rq.dd = dd_stats_out != nullptr;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_regimes(mcp_ctx* c, const mcp_params* prm, const mcp_regimes* r, const float* mu, const float* chol, const float* W,
                         uint64_t seed, uint64_t path_begin, uint64_t n_paths, int n_horizons, const int32_t* horizons, int n_levels,
                         const double* levels, float* terminal_out, mcp_stats* stats_out, float* mdd_out, mcp_stats* dd_stats_out,
                         float* horizon_out, mcp_stats* hz_stats_out, double* bands_out) {
  Request rq = host_request(SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.regimes = true;
  rq.rs = r;
  rq.dd = dd_stats_out != nullptr;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_regime_consts(const mcp_regimes* r, uint64_t* thr_out, double* p_out) {
  if (!r) return fail(MCP_E_ARG, "regimes is NULL");
  if (r->reserved != 0) return fail(MCP_E_ARG, "regimes reserved=%d must be 0", r->reserved);
  if (!std::isfinite(r->p01) || !std::isfinite(r->p10) || !std::isfinite(r->start))
    return fail(MCP_E_ARG, "regimes p01=%g, p10=%g, start=%g must be finite", r->p01, r->p10, r->start);
  if (!(r->p01 >= 0.0 && r->p01 <= 1.0) || !(r->p10 >= 0.0 && r->p10 <= 1.0) || !(r->start >= 0.0 && r->start <= 1.0))
    return fail(MCP_E_ARG, "regimes p01=%g, p10=%g, start=%g outside [0, 1]", r->p01, r->p10, r->start);
  if (!thr_out || !p_out) return fail(MCP_E_ARG, "NULL pointer");
  const RegimeConsts c = regime_consts(r);
  thr_out[0] = c.thr01; thr_out[1] = c.thr10; thr_out[2] = c.thr_start;
  p_out[0] = c.p01; p_out[1] = c.p10; p_out[2] = c.start;
  return MCP_OK;
}

int mcp_regime_pivots(const mcp_params* prm, const mcp_regimes* r, const float* mu, const float* W, int n_horizons,
                      const int32_t* horizons, double* pivots_out, double* hz_pivots_out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_regimes(prm->n_assets, r)) return rc;
  if (!mu || !W || !pivots_out) return fail(MCP_E_ARG, "NULL pointer");
  for (int i = 0; i < prm->n_assets; i++)
    if (!std::isfinite(mu[i])) return fail(MCP_E_ARG, "regimes: mu, asset %d is not finite", i);
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "regime-switching paths compound simply (no log compounding)");
  if (n_horizons != 0) {
    if (int rc = check_horizons(prm->n_steps, n_horizons, horizons)) return rc;
    if (!hz_pivots_out) return fail(MCP_E_ARG, "hz_pivots_out is NULL");
  }
  regime_pivots(prm->n_assets, prm->n_portfolios, prm->n_steps, mu, r->mu1, regime_consts(r), W, n_horizons, horizons, pivots_out, hz_pivots_out);
  return MCP_OK;
}

int mcp_jump_consts(const mcp_jumps* j, int n_assets, const float* mu, uint32_t* thr_out, double* mean_count_out, float* drift_out) {
  if (n_assets < 1 || n_assets > MCP_MAX_ASSETS) return fail(MCP_E_ARG, "n_assets=%d outside [1,%d]", n_assets, MCP_MAX_ASSETS);
  if (int rc = check_jumps(n_assets, j)) return rc;
  if (!thr_out || !mean_count_out || (drift_out && !mu)) return fail(MCP_E_ARG, "NULL pointer");
  const JumpConsts c = jump_consts(j);
  for (int k = 0; k < MCP_MAX_JUMPS; k++) thr_out[k] = c.thr[k];
  *mean_count_out = c.mean_count;
  if (drift_out) jump_drift(j, c, n_assets, mu, drift_out);
  return MCP_OK;
}

int mcp_simulate_filtered(mcp_ctx* c, const mcp_params* prm, const mcp_filtered* filt, const mcp_garch* g, const float* W, uint64_t seed,
                          uint64_t path_begin, uint64_t n_paths, int n_horizons, const int32_t* horizons, int n_levels,
                          const double* levels, float* terminal_out, mcp_stats* stats_out, float* horizon_out, mcp_stats* hz_stats_out,
                          double* bands_out) {
  Request rq = host_request(SRC_FHS, nullptr, nullptr, W, terminal_out, stats_out);
  rq.filt = filt;
  rq.gv = g;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_filtered_pivots(const mcp_params* prm, const mcp_filtered* filt, const float* W, double* out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_filtered(prm, filt)) return rc;
  if (!W || !out) return fail(MCP_E_ARG, "NULL pointer");
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "filtered paths compound simply (no log compounding)");
  std::vector<double> me((size_t)prm->n_assets);
  filt_means(prm->n_assets, filt, me.data());
  filt_pivots(prm->n_assets, prm->n_portfolios, prm->n_steps, me.data(), W, out);
  return MCP_OK;
}

// SPEC.md 5.10: the pair record of one portfolio from the call's statistics, its pivot c and cross = sum (x_2j - c)(x_2j+1 - c)
static void pair_record(const mcp_stats& st, double c, double cross, mcp_pair* out) {
  const double n = (double)st.n, np = (double)(st.n / 2);
  const double s1 = (st.mean - c) * n;
  const double C = n > 0.0 ? cross - s1 * s1 / (2.0 * n) : 0.0;
  out->n_pairs = st.n / 2;
  out->reserved = 0;
  out->cross = cross;
  out->pair_cov = np >= 2.0 ? C / (np - 1.0) : 0.0;
  out->pair_corr = st.m2 > 0.0 ? 2.0 * C / st.m2 : 0.0;
  out->mean_se = np >= 2.0 ? std::sqrt(std::max(st.m2 + 2.0 * C, 0.0) / (n * (n - 2.0))) : 0.0;
  out->mean_se_iid = n > 0.0 ? st.std / std::sqrt(n) : 0.0;
}

int mcp_simulate_antithetic(mcp_ctx* c, const mcp_params* prm, const mcp_garch* g, const mcp_student_t* st, const float* mu,
                            const float* chol, const float* W, uint64_t seed, uint64_t path_begin, uint64_t n_paths, int n_horizons,
                            const int32_t* horizons, int n_levels, const double* levels, float* terminal_out, mcp_stats* stats_out,
                            float* mdd_out, mcp_stats* dd_stats_out, float* horizon_out, mcp_stats* hz_stats_out, double* bands_out,
                            mcp_pair* pair_out) {
  Request rq = host_request(st ? SRC_T : SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.st = st;
  rq.garch = g != nullptr;
  rq.gv = g;
  rq.dd = dd_stats_out != nullptr;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
  rq.anti = true;
  rq.pair_out = pair_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  if (int rc = check_request(prm, rq, n_paths, nullptr, path_begin)) return rc;
  const size_t K = (size_t)prm->n_portfolios;
  std::vector<double> cross(K, 0.0), pivot(K);
  rq.cross_out = cross.data();
  if (int rc = simulate_impl(c, prm, rq, seed, path_begin, n_paths)) return rc;
  if (int rc = mcp_pivots(prm, mu, chol, W, pivot.data())) return rc;
  for (size_t k = 0; k < K; k++) pair_record(stats_out[k], pivot[k], cross[k], pair_out + k);
  return MCP_OK;
}

int mcp_simulate_attribution(mcp_ctx* c, const mcp_params* prm, const mcp_garch* g, const mcp_student_t* st, const float* mu,
                             const float* chol, const float* W, uint64_t seed, uint64_t path_begin, uint64_t n_paths, float* terminal_out,
                             mcp_stats* stats_out, float* contrib_out, mcp_attr* attr_out, uint64_t* attr_counts_out) {
  Request rq = host_request(st ? SRC_T : SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.st = st;
  rq.garch = g != nullptr;
  rq.gv = g;
  rq.attr = true;
  rq.contrib_out = contrib_out;
  rq.attr_out = attr_out;
  rq.attr_counts_out = attr_counts_out;
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_simulate_cashflow(mcp_ctx* c, const mcp_params* prm, const mcp_cashflow* cf, const float* mu, const float* chol,
                          const mcp_bootstrap* boot, const mcp_student_t* st, const float* W, uint64_t seed, uint64_t path_begin,
                          uint64_t n_paths, int n_horizons, const int32_t* horizons, int n_levels, const double* levels,
                          float* terminal_out, mcp_stats* stats_out, uint64_t* counts_out, float* horizon_out, mcp_stats* hz_stats_out,
                          double* bands_out, uint64_t* hz_counts_out) {
  if (boot && st) return fail(MCP_E_ARG, "exactly one draw source: mu and chol (with or without student_t), or boot");
  Request rq = host_request(boot ? SRC_BOOT : st ? SRC_T : SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.boot = boot;
  rq.st = st;
  rq.cash = true;
  rq.cf = cf;
  rq.counts_out = counts_out;
  rq.hz_counts_out = hz_counts_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_cashflow_pivots(const mcp_params* prm, const mcp_cashflow* cf, const float* mu, const mcp_bootstrap* boot, const float* W,
                        double* out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_cashflow(prm, cf)) return rc;
  if ((mu == nullptr) == (boot == nullptr)) return fail(MCP_E_ARG, "exactly one of mu and boot");
  if (boot)
    if (int rc = check_boot(prm, boot)) return rc;
  if (!W || !out) return fail(MCP_E_ARG, "NULL pointer");
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "paths with cash flows compound simply (no log compounding)");
  std::vector<double> m((size_t)prm->n_portfolios);
  cash_means(prm->n_assets, prm->n_portfolios, mu, boot, W, m.data());
  cash_pivots(prm->n_portfolios, prm->n_steps, m.data(), cf->flows, (double)(float)prm->v0, 0, nullptr, out, nullptr);
  return MCP_OK;
}

int mcp_simulate_glide(mcp_ctx* c, const mcp_params* prm, const mcp_glide* gl, const mcp_cashflow* cf, const float* mu, const float* chol,
                       const mcp_bootstrap* boot, const mcp_student_t* st, const float* W, uint64_t seed, uint64_t path_begin,
                       uint64_t n_paths, int n_horizons, const int32_t* horizons, int n_levels, const double* levels, float* terminal_out,
                       mcp_stats* stats_out, uint64_t* counts_out, float* horizon_out, mcp_stats* hz_stats_out, double* bands_out,
                       uint64_t* hz_counts_out) {
  if (boot && st) return fail(MCP_E_ARG, "exactly one draw source: mu and chol (with or without student_t), or boot");
  // cf NULL: the all-zero schedule without a target, so that one request and one kernel serve both
  const std::vector<float> zeros(!cf && prm && prm->n_steps > 0 ? (size_t)prm->n_steps : 0, 0.0f);
  const mcp_cashflow none = {zeros.data(), prm ? prm->n_steps : 0, 0, 0.0};
  Request rq = host_request(boot ? SRC_BOOT : st ? SRC_T : SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.boot = boot;
  rq.st = st;
  rq.cash = true;
  rq.cf = cf ? cf : &none;
  rq.glide = true;
  rq.gl = gl;
  rq.counts_out = counts_out;
  rq.hz_counts_out = hz_counts_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_glide_pivots(const mcp_params* prm, const mcp_glide* gl, const mcp_cashflow* cf, const float* mu, const mcp_bootstrap* boot,
                     const float* W, int n_horizons, const int32_t* horizons, double* pivots_out, double* hz_pivots_out) {
  if (int rc = check_params(prm)) return rc;
  if (cf)
    if (int rc = check_cashflow(prm, cf)) return rc;
  if (!((float)prm->v0 > 0.0f)) return fail(MCP_E_ARG, "v0=%g rounds to zero in binary32", prm->v0);
  if (int rc = check_glide(prm, gl)) return rc;
  if ((mu == nullptr) == (boot == nullptr)) return fail(MCP_E_ARG, "exactly one of mu and boot");
  if (boot)
    if (int rc = check_boot(prm, boot)) return rc;
  if (!W || !pivots_out) return fail(MCP_E_ARG, "NULL pointer");
  if (n_horizons != 0) {
    if (int rc = check_horizons(prm->n_steps, n_horizons, horizons)) return rc;
    if (!hz_pivots_out) return fail(MCP_E_ARG, "hz_pivots_out is NULL");
  }
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "glide paths compound simply (no log compounding)");
  const int K = prm->n_portfolios;
  std::vector<double> m((size_t)(gl->n_breaks + 1) * K);
  glide_means(prm->n_assets, K, 0, K, mu, boot, W, gl, m.data());
  glide_pivots(K, prm->n_steps, gl->n_breaks, gl->breaks, m.data(), cf ? cf->flows : nullptr, (double)(float)prm->v0, n_horizons, horizons,
               pivots_out, hz_pivots_out);
  return MCP_OK;
}

int mcp_simulate_protected(mcp_ctx* c, const mcp_params* prm, const mcp_protect* pt, const mcp_garch* gv, const mcp_student_t* st,
                           const mcp_jumps* jp, const float* mu, const float* chol, const float* W, uint64_t seed, uint64_t path_begin,
                           uint64_t n_paths, int n_horizons, const int32_t* horizons, int n_levels, const double* levels, float* terminal_out,
                           mcp_stats* stats_out, float* mdd_out, mcp_stats* dd_stats_out, uint64_t* counts_out, float* horizon_out,
                           mcp_stats* hz_stats_out, double* bands_out, uint64_t* hz_counts_out) {
  Request rq = host_request(st ? SRC_T : SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.st = st;
  rq.garch = gv != nullptr;
  rq.gv = gv;
  rq.jumps = jp != nullptr;
  rq.jp = jp;
  rq.protect = true;
  rq.pi = pt;
  rq.dd = dd_stats_out != nullptr;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
  rq.counts_out = counts_out;
  rq.hz_counts_out = hz_counts_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_protect_pivots(const mcp_params* prm, const mcp_protect* pt, const float* mu, const float* W, int n_horizons,
                       const int32_t* horizons, double* pivots_out, double* hz_pivots_out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_protect(prm, pt)) return rc;
  if (!mu || !W || !pivots_out) return fail(MCP_E_ARG, "NULL pointer");
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "protected paths compound simply (no log compounding)");
  if (n_horizons != 0) {
    if (int rc = check_horizons(prm->n_steps, n_horizons, horizons)) return rc;
    if (!hz_pivots_out) return fail(MCP_E_ARG, "hz_pivots_out is NULL");
  }
  protect_pivots(*prm, pt, mu, W, prm->n_portfolios, n_horizons, horizons, pivots_out, hz_pivots_out);
  return MCP_OK;
}

int mcp_protect_floor(double floor0, double rate, int n_steps, float* out) {
  if (!std::isfinite(floor0) || !std::isfinite(rate) || !std::isfinite((float)floor0) || !std::isfinite((float)rate))
    return fail(MCP_E_ARG, "floor0=%g and rate=%g must be finite, also in binary32", floor0, rate);
  if (!(floor0 >= 0.0)) return fail(MCP_E_ARG, "floor0=%g must be >= 0", floor0);
  if (!(rate > -1.0) || !((float)rate > -1.0f)) return fail(MCP_E_ARG, "rate=%g must be > -1 in binary32", rate);
  if (n_steps < 1) return fail(MCP_E_ARG, "n_steps=%d must be >= 1", n_steps);
  if (!out) return fail(MCP_E_ARG, "out is NULL");
  const float r = (float)rate;
  out[0] = (float)floor0;
  for (int t = 0; t < n_steps; t++) {
    out[t + 1] = std::fmaf(out[t], r, out[t]);
    if (!std::isfinite(out[t + 1])) return fail(MCP_E_ARG, "the floor schedule overflows binary32 at step %d", t + 1);
  }
  return MCP_OK;
}

int mcp_simulate_overlay(mcp_ctx* c, const mcp_params* prm, const mcp_overlay* ov, const float* mu, const float* chol,
                         const mcp_student_t* st, const float* W, uint64_t seed, uint64_t path_begin, uint64_t n_paths, int n_horizons,
                         const int32_t* horizons, int n_levels, const double* levels, float* terminal_out, mcp_stats* stats_out,
                         float* mdd_out, mcp_stats* dd_stats_out, float* horizon_out, mcp_stats* hz_stats_out, double* bands_out) {
  Request rq = host_request(st ? SRC_T : SRC_GAUSS, mu, chol, W, terminal_out, stats_out);
  rq.st = st;
  rq.overlay = true;
  rq.ov = ov;
  rq.dd = dd_stats_out != nullptr;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
  ask_horizons(rq, n_horizons != 0, n_horizons, horizons, n_levels, levels, horizon_out, hz_stats_out, bands_out);
  return simulate_checked(c, prm, rq, seed, path_begin, n_paths);
}

int mcp_overlay_pivots(const mcp_params* prm, const mcp_overlay* ov, const float* mu, const float* W, double* out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_overlay(prm, ov)) return rc;
  if (!mu || !W || !out) return fail(MCP_E_ARG, "NULL pointer");
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "overlaid paths compound simply (no log compounding)");
  if (ov->n_rows == 0) {                                   // every asset passes through: the plain pivots, which read no factor
    const std::vector<float> eye((size_t)prm->n_assets * prm->n_assets, 0.0f);
    return mcp_pivots(prm, mu, eye.data(), W, out);
  }
  overlay_pivots(prm->n_assets, prm->n_portfolios, prm->n_steps, ov, mu, W, 0, nullptr, out, nullptr);
  return MCP_OK;
}

int mcp_sweep_historical(mcp_ctx* c, int N, int R, int P, const double* returns, const double* mean, const double* cov,
                         const double* W, double rf, double alpha, double* o_ret, double* o_std, double* o_sharpe,
                         double* o_var, double* o_cvar) {
  if (!c) return fail(MCP_E_ARG, "ctx is NULL");
  if (N < 1 || N > MCP_MAX_ASSETS) return fail(MCP_E_ARG, "n_assets=%d outside [1,%d]", N, MCP_MAX_ASSETS);
  if (R < 1 || R > MCP_SWEEP_MAX_ROWS) return fail(MCP_E_ARG, "n_rows=%d outside [1,%d]", R, MCP_SWEEP_MAX_ROWS);
  if (P < 1) return fail(MCP_E_ARG, "n_portfolios=%d < 1", P);
  if (!(alpha > 0.0 && alpha < 1.0)) return fail(MCP_E_ARG, "alpha=%g outside (0,1)", alpha);
  const void* const ptrs[9] = {returns, mean, cov, W, o_ret, o_std, o_sharpe, o_var, o_cvar};
  static const char* const ptr_names[9] = {"returns", "mean", "cov", "W", "port_return", "port_std", "sharpe", "var", "cvar"};
  for (int i = 0; i < 9; i++)
    if (!ptrs[i]) return fail(MCP_E_ARG, "%s is NULL", ptr_names[i]);
  // Finite input only, the rule of bootstrap rows (check_bootstrap): the kernels order the series with plain compares, under
  // which a NaN has no rank, and would answer with a finite number.  A host scan of (R + 1 + N + P) * N doubles, at most
  // 4096 * 64 + P * 64 for returns and W, before any copy or launch.
  const auto first_bad = [](const double* a, size_t n) {
    size_t i = 0;
    while (i < n && std::isfinite(a[i])) i++;
    return i;
  };
  const size_t n = (size_t)N;
  size_t i;
  if ((i = first_bad(returns, (size_t)R * n)) < (size_t)R * n)
    return fail(MCP_E_ARG, "returns[%zu] (row %zu, asset %zu) is not finite", i, i / n, i % n);
  if ((i = first_bad(W, (size_t)P * n)) < (size_t)P * n)
    return fail(MCP_E_ARG, "W[%zu] (portfolio %zu, asset %zu) is not finite", i, i / n, i % n);
  if ((i = first_bad(mean, n)) < n) return fail(MCP_E_ARG, "mean[%zu] is not finite", i);
  if ((i = first_bad(cov, n * n)) < n * n) return fail(MCP_E_ARG, "cov[%zu] (row %zu, column %zu) is not finite", i, i / n, i % n);
  std::lock_guard<std::mutex> lock(c->mu);
  Shard& sh = c->sh[0];
  DeviceGuard guard(sh.device);
  if (guard.err != hipSuccess) return fail(MCP_E_HIP, "hipSetDevice(%d): %s", sh.device, hipGetErrorString(guard.err));
  uint64_t lo, hi;
  double gamma;
  if (int rc = mcp_percentile_rank((uint64_t)R, alpha, &lo, &hi, &gamma)) return rc;
  const size_t n_ret = (size_t)R * N, n_cov = (size_t)N * N, n_w = (size_t)P * N, n_out = 5 * (size_t)P;
  const size_t total = n_ret + (size_t)N + n_cov + n_w + n_out;
  if (int rc = grow_dev((void**)&c->d_sweep, &c->sweep_cap, total * sizeof(double))) return rc;
  double* d_ret = c->d_sweep;
  double* d_mean = d_ret + n_ret;
  double* d_cov = d_mean + N;
  double* d_w = d_cov + n_cov;
  double* d_out = d_w + n_w;
  hipStream_t s = sh.stream;
  HIP_TRY(hipMemcpyAsync(d_ret, returns, n_ret * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_mean, mean, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_cov, cov, n_cov * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_w, W, n_w * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(mcp::launch_sweep_hist(N, R, P, d_ret, d_mean, d_cov, d_w, rf, lo, hi, gamma, d_out, s));
  double* outs[5] = {o_ret, o_std, o_sharpe, o_var, o_cvar};
  for (int i = 0; i < 5; i++)
    HIP_TRY(hipMemcpyAsync(outs[i], d_out + (size_t)i * P, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MCP_OK;
}

}  // extern "C"

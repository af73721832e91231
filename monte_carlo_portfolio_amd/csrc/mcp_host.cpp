// mcp_host.cpp -- the host code of libmcport.so that touches no device (mcp_host.h): argument checking, every feature's host
// constants and closed-form pivots, parameter packing, the layout of a tile's parameter block, the choice of the path kernel
// (route_kernel), and the entry points of include/mcport.h that need nothing else.  No device header: make host-selftest builds
// this file with a plain C++ compiler.
#include "mcp_host.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

namespace mcph {

namespace {
thread_local std::string g_err;
}


int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

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
size_t glide_rows(int kt) { return (size_t)KT_WIDE * (size_t)((kt + KT_WIDE - 1) / KT_WIDE); }
size_t glide_len(int N, int kt, const mcp_glide* gl) { return (size_t)gl->n_breaks * glide_rows(kt) * (size_t)n4_of(N); }
void glide_pack(int N, int K, int k0, int kt, const mcp_glide* gl, float* out) {
  const size_t n4 = (size_t)n4_of(N), blk = glide_rows(kt) * n4;
  std::fill(out, out + (size_t)gl->n_breaks * blk, 0.0f);
  for (int g = 0; g < gl->n_breaks; g++)
    for (int k = 0; k < kt; k++)
      memcpy(out + (size_t)g * blk + (size_t)k * n4, gl->targets + ((size_t)g * K + (size_t)(k0 + k)) * N, (size_t)N * sizeof(float));
}

// SPEC.md 4.15: the binary32 constants of a protection request
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
// SPEC.md 4.19: the binary32 constants of a volatility-targeting request; oml = fl32(1 - (double)lam)
VolTargetConsts vol_target_consts(const mcp_vol_target* vt) {
  const float lam = (float)vt->decay;
  return VolTargetConsts{(float)vt->target, lam, (float)(1.0 - (double)lam), (float)vt->cap, (float)vt->rate, (float)vt->spread};
}
// SPEC.md 4.19: the caller's s0_k, or fl32(sum_j (sum_i W[k,i] L[i,j])^2) in binary64 from the binary32 inputs, i and j ascending over
// the lower triangle the walk reads, rounded once
float vol_target_s0(int N, const mcp_vol_target* vt, const float* chol, const float* W, int k) {
  if (vt->s0) return (float)vt->s0[k];
  double q = 0.0;
  for (int j = 0; j < N; j++) {
    double v = 0.0;
    for (int i = j; i < N; i++) v += (double)W[(size_t)k * N + i] * (double)chol[(size_t)i * N + j];
    q += v * v;
  }
  return (float)q;
}
// SPEC.md 4.19: target > 0, decay in [0, 1], cap > 0, rate > -1, spread >= 0, each finite before and after rounding to binary32 and
// inside its range after it; s0 finite and > 0 in binary32, given or formed; a finite target_value; reserved == 0; fl32(v0) > 0
int check_vol_target(const mcp_params* prm, const mcp_vol_target* vt, const float* chol, const float* W) {
  if (!vt) return fail(MCP_E_ARG, "vol_target is NULL");
  if (vt->reserved != 0) return fail(MCP_E_ARG, "vol_target reserved=%d must be 0", vt->reserved);
  const double v[5] = {vt->target, vt->decay, vt->cap, vt->rate, vt->spread};
  for (int i = 0; i < 5; i++)
    if (!std::isfinite(v[i]) || !std::isfinite((float)v[i]))
      return fail(MCP_E_ARG, "vol_target target=%g, decay=%g, cap=%g, rate=%g, spread=%g must be finite, also in binary32", v[0], v[1], v[2], v[3],
                  v[4]);
  const VolTargetConsts c = vol_target_consts(vt);
  if (!(vt->target > 0.0) || !(c.tgt > 0.0f)) return fail(MCP_E_ARG, "vol_target target=%g must be > 0 in binary32", vt->target);
  if (!(vt->decay >= 0.0 && vt->decay <= 1.0) || !(c.lam >= 0.0f && c.lam <= 1.0f))
    return fail(MCP_E_ARG, "vol_target decay=%g outside [0, 1]", vt->decay);
  if (!(vt->cap > 0.0) || !(c.b > 0.0f)) return fail(MCP_E_ARG, "vol_target cap=%g must be > 0 in binary32", vt->cap);
  if (!(vt->rate > -1.0) || !(c.rf > -1.0f)) return fail(MCP_E_ARG, "vol_target rate=%g must be > -1 in binary32", vt->rate);
  if (!(vt->spread >= 0.0)) return fail(MCP_E_ARG, "vol_target spread=%g must be >= 0", vt->spread);
  if (vt->target_value && (!std::isfinite(*vt->target_value) || !std::isfinite((float)*vt->target_value)))
    return fail(MCP_E_ARG, "vol_target target_value=%g must be finite, also in binary32", *vt->target_value);
  if (!((float)prm->v0 > 0.0f)) return fail(MCP_E_ARG, "v0=%g rounds to zero in binary32", prm->v0);
  if (!vt->s0 && (!chol || !W)) return fail(MCP_E_ARG, "NULL pointer");
  for (int k = 0; k < prm->n_portfolios; k++) {
    const float s0 = vol_target_s0(prm->n_assets, vt, chol, W, k);
    if ((vt->s0 && !(std::isfinite(vt->s0[k]) && vt->s0[k] > 0.0)) || !std::isfinite(s0) || !(s0 > 0.0f))
      return fail(MCP_E_ARG, "vol_target s0, portfolio %d = %g must be finite and > 0 in binary32", k, vt->s0 ? vt->s0[k] : (double)s0);
  }
  return MCP_OK;
}
// SPEC.md 4.21: the struct, reserved == 0, and every entry of M finite (binary32 already: before and after rounding are one test)
int check_drift_uncertainty(int n_assets, const mcp_drift_uncertainty* du) {
  if (!du) return fail(MCP_E_ARG, "drift_uncertainty is NULL");
  if (!du->factor) return fail(MCP_E_ARG, "drift_uncertainty factor is NULL");
  if (du->reserved != 0) return fail(MCP_E_ARG, "drift_uncertainty reserved=%d must be 0", du->reserved);
  for (size_t i = 0; i < (size_t)n_assets * (size_t)n_assets; i++)
    if (!std::isfinite(du->factor[i]))
      return fail(MCP_E_ARG, "drift_uncertainty factor, entry (%zu, %zu) is not finite", i / (size_t)n_assets, i % (size_t)n_assets);
  return MCP_OK;
}
size_t drift_len(int N) { const size_t n4 = (size_t)n4_of(N); return n4 * (n4 / 2 + 1); }
// M's lower triangle as mcp_pack_params lays out the Cholesky factor: pair m = rows (2m, 2m+1) at offset 2m(m+1), columns j = 0 ..
// 2m+1 interleaved as (M[2m][j], M[2m+1][j]); the padding and M[2m][2m+1] are +0; -0 -> +0
void drift_pack(int N, const mcp_drift_uncertainty* du, float* out) {
  std::fill(out, out + drift_len(N), 0.0f);
  for (int i = 0; i < N; i++)
    for (int j = 0; j <= i; j++) out[2 * (i / 2) * (i / 2 + 1) + 2 * j + (i & 1)] = du->factor[(size_t)i * N + j] + 0.0f;
}
// SPEC.md 4.16: the binary32 constants of a spending request; w0 without `first` is fl32(p32 fl32(v0)), the product in binary64 (exact)
SpendConsts spend_consts(const mcp_spending* sp, double v0) {
  const float p = (float)sp->rate;
  return SpendConsts{p, (float)(1.0 + sp->inflation), (float)(1.0 - sp->down), (float)(1.0 + sp->up),
                     sp->has_first ? (float)sp->first : (float)((double)p * (double)(float)v0)};
}
// SPEC.md 4.16: rate finite >= 0, every >= 0, down in [0, 1], up in [0, +inf] (+inf allowed), inflation finite > -1, first finite >= 0,
// a finite target, each rule before and after rounding to binary32; flags 0 / 1, reserved == 0, fl32(v0) > 0
int check_spending(double v0, const mcp_spending* sp) {
  if (!sp) return fail(MCP_E_ARG, "spending is NULL");
  if (sp->reserved != 0) return fail(MCP_E_ARG, "spending reserved=%d must be 0", sp->reserved);
  if (sp->has_first != 0 && sp->has_first != 1) return fail(MCP_E_ARG, "has_first=%d must be 0 or 1", sp->has_first);
  if (sp->has_target != 0 && sp->has_target != 1) return fail(MCP_E_ARG, "has_target=%d must be 0 or 1", sp->has_target);
  if (sp->every < 0) return fail(MCP_E_ARG, "spending every=%d must be >= 0", sp->every);
  if (!((float)v0 > 0.0f) || !std::isfinite((float)v0)) return fail(MCP_E_ARG, "v0=%g must be positive and finite in binary32", v0);
  const SpendConsts c = spend_consts(sp, v0);
  if (!std::isfinite(sp->rate) || !(sp->rate >= 0.0) || !std::isfinite(c.p)) return fail(MCP_E_ARG, "spending rate=%g must be finite and >= 0, also in binary32", sp->rate);
  if (!(sp->down >= 0.0 && sp->down <= 1.0) || !(c.lo >= 0.0f && c.lo <= 1.0f)) return fail(MCP_E_ARG, "spending down=%g outside [0, 1]", sp->down);
  if (!(sp->up >= 0.0) || !(c.hi >= 1.0f)) return fail(MCP_E_ARG, "spending up=%g must be >= 0 (+inf allowed)", sp->up);
  if (!std::isfinite(sp->inflation) || !(sp->inflation > -1.0) || !((float)sp->inflation > -1.0f) || !(c.g > 0.0f) || !std::isfinite(c.g))
    return fail(MCP_E_ARG, "spending inflation=%g must be finite and > -1, also in binary32", sp->inflation);
  if (sp->has_first && (!std::isfinite(sp->first) || !(sp->first >= 0.0) || !std::isfinite(c.w0)))
    return fail(MCP_E_ARG, "spending first=%g must be finite and >= 0, also in binary32", sp->first);
  if (!std::isfinite(c.w0)) return fail(MCP_E_ARG, "spending rate=%g times v0=%g overflows binary32", sp->rate, v0);
  if (sp->has_target && (!std::isfinite(sp->target) || !std::isfinite((float)sp->target)))
    return fail(MCP_E_ARG, "spending target=%g must be finite, also in binary32", sp->target);
  return MCP_OK;
}

// What follows the packed block (and the jump loadings) of a protected launch: the schedule S_0 .. S_T, then per stored row -- the kt
// terminal rows, then the H*kt horizon rows -- the two thresholds {S_h, target or -inf} of the counts (SPEC.md 5.15)
size_t protect_len(int T, int kt, int H) { return (size_t)T + 1 + 2 * (size_t)kt * (size_t)(1 + H); }
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

// SPEC.md 4.18: the rule's arguments.  tol is [K][N]: every entry >= 0 (finite or +inf); a NaN fails the compare too
int check_band(const mcp_params* prm, const mcp_band* bd) {
  if (!bd) return fail(MCP_E_ARG, "band is NULL");
  if (bd->every < 0) return fail(MCP_E_ARG, "band every=%d < 0", bd->every);
  if (bd->reserved != 0) return fail(MCP_E_ARG, "band reserved=%d must be 0", bd->reserved);
  if (!(bd->cost >= 0.0 && bd->cost < 1.0)) return fail(MCP_E_ARG, "band cost=%g outside [0, 1)", bd->cost);
  if (!bd->tol) return fail(MCP_E_ARG, "band tol is NULL");
  const size_t n = (size_t)prm->n_portfolios * (size_t)prm->n_assets;
  for (size_t i = 0; i < n; i++)
    if (!(bd->tol[i] >= 0.0f))
      return fail(MCP_E_ARG, "band tol[%zu]=%g (portfolio %zu, asset %zu) must be >= 0 or +inf", i, (double)bd->tol[i], i / (size_t)prm->n_assets,
                  i % (size_t)prm->n_assets);
  return MCP_OK;
}
int band_reviews(int T, int e) { return (e >= 1 && e < T) ? (T - 1) / e : 0; }
size_t count_bins(const mcp_params* prm, const Request& rq) {
  return (size_t)(rq.band ? band_reviews(prm->n_steps, rq.bd->every) : prm->n_steps) + 1;
}
// SPEC.md 4.18: the device copy of the tolerances of the portfolios [k0, k0 + kt) -- [kt][N4] floats, an entry of an unwatched asset
// (+inf, or padding) stored as +0, then per portfolio the two 32-bit words (low, high) of the mask of the watched assets
size_t band_len(int N, int kt) { return (size_t)kt * ((size_t)n4_of(N) + 2); }
void band_pack(int N, int k0, int kt, const mcp_band* bd, float* out) {
  const size_t n4 = (size_t)n4_of(N);
  uint32_t* words = (uint32_t*)(out + (size_t)kt * n4);
  for (int k = 0; k < kt; k++) {
    uint64_t watch = 0;
    for (size_t i = 0; i < n4; i++) {
      const float t = i < (size_t)N ? bd->tol[(size_t)(k0 + k) * N + i] : __builtin_inff();
      const bool on = t < __builtin_inff();
      out[(size_t)k * n4 + i] = on ? t : 0.0f;
      if (on) watch |= (uint64_t)1 << i;
    }
    words[2 * k] = (uint32_t)watch;
    words[2 * k + 1] = (uint32_t)(watch >> 32);
  }
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

void ask_drawdown(Request& rq, float* mdd_out, mcp_stats* dd_stats_out) {
  rq.dd = dd_stats_out != nullptr;
  rq.mdd_out = mdd_out;
  rq.dd_stats_out = dd_stats_out;
}

// Every rule a request meets: each feature's own arguments, then which features combine (MCP_E_UNSUPPORTED), then the outputs.
// `ln`: an mcp_launch_paths* call, whose device arrays are checked instead of the host arrays of an mcp_simulate* call.
int check_request(const mcp_params* prm, const Request& rq, uint64_t n_paths, const Launch* ln, uint64_t path_begin) {
  int rc;
  if ((rc = check_params(prm))) return rc;
  if (rq.band) {                                               // SPEC.md 4.18: the rules, then what the bands are not combined with
    if ((rc = check_band(prm, rq.bd))) return rc;
    if (!rq.trade_hist_out || !rq.turnover_stats_out) return fail(MCP_E_ARG, "trade_hist_out or turnover_stats_out is NULL");
    if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "banded paths compound simply (no log compounding)");
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH))
      return fail(MCP_E_UNSUPPORTED, "banded paths run on the unfolded recurrence and the spec's normals (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)");
    if (band_reviews(prm->n_steps, rq.bd->every) > MCP_MAX_LIFE_STEPS)
      return fail(MCP_E_UNSUPPORTED, "bands: %d reviews above MCP_MAX_LIFE_STEPS=%d", band_reviews(prm->n_steps, rq.bd->every), MCP_MAX_LIFE_STEPS);
    if (!rq.rebalanced || rq.src == SRC_T || rq.src == SRC_FHS || rq.cash || rq.glide || rq.protect || rq.spend || rq.life || rq.overlay ||
        rq.garch || rq.jumps || rq.regimes || rq.dd || rq.attr || rq.anti)
      return fail(MCP_E_UNSUPPORTED, "tolerance bands are not combined with Student-t draws, filtered rows, cash flows, glide paths, floor protection, "
                                     "spending rules, the drawdown, the overlay, GARCH, jumps, regimes, the attribution or antithetic pairs");
    if (ln) return fail(MCP_E_UNSUPPORTED, "tolerance bands are not wired into mcp_launch_paths*");
  }
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
  if (rq.spend) {                                              // SPEC.md 4.16: the rules, then what a spending rule is not combined with
    if ((rc = check_spending(prm->v0, rq.sp))) return rc;
    if (!ln && !rq.wd_stats_out) return fail(MCP_E_ARG, "wd_stats_out is NULL");
    if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "paths with a spending rule compound simply (no log compounding)");
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH))
      return fail(MCP_E_UNSUPPORTED, "paths with a spending rule run on the unfolded recurrence and the spec's normals (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)");
    if (!rq.cash || rq.glide || rq.protect || rq.src == SRC_FHS || rq.rebalanced || rq.overlay || rq.garch || rq.jumps || rq.regimes || rq.dd ||
        rq.attr || rq.anti)
      return fail(MCP_E_UNSUPPORTED, "a spending rule is not combined with a cash-flow schedule, a glide path, floor protection, the drawdown, "
                                     "rebalancing, the overlay, GARCH, jumps, regimes, filtered rows, the attribution or antithetic pairs");
    if (ln) return fail(MCP_E_UNSUPPORTED, "spending rules are not wired into mcp_launch_paths*");
  }
  if (rq.life) {                                               // SPEC.md 4.17: a counter on the walks with absorbing ruin
    if (!rq.cash) return fail(MCP_E_UNSUPPORTED, "the lifetime needs a walk with ruin: a cash-flow schedule, with or without a glide path, or a spending rule");
    if (prm->n_steps > MCP_MAX_LIFE_STEPS) return fail(MCP_E_UNSUPPORTED, "lifetime: n_steps=%d above MCP_MAX_LIFE_STEPS=%d", prm->n_steps, MCP_MAX_LIFE_STEPS);
    if (ln) return fail(MCP_E_UNSUPPORTED, "the lifetime is not wired into mcp_launch_paths*");
    if (!rq.life_hist_out) return fail(MCP_E_ARG, "life_hist_out is NULL");
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
  if (rq.vol_target) {                                         // SPEC.md 4.19: the rules, then what the volatility target is not combined with
    if ((rc = check_vol_target(prm, rq.vt, rq.chol, rq.W))) return rc;
    if (!rq.counts_out) return fail(MCP_E_ARG, "counts_out is NULL");
    if ((rq.hz_counts_out == nullptr) != !rq.hz) return fail(MCP_E_ARG, "hz_counts_out must be NULL exactly when n_horizons == 0");
    if (!rq.exposure_stats_out && rq.exposure_out) return fail(MCP_E_ARG, "exposure_out needs exposure_stats_out");
    if (!rq.exposure_stats_out && !rq.dd) return fail(MCP_E_ARG, "exposure_stats_out is NULL (it may be only where dd_stats_out is not)");
    if (rq.src == SRC_T && (rc = check_student_t(prm, rq.st))) return rc;
    if (rq.garch && (rc = check_garch(prm, rq.gv))) return rc;
    if (rq.jumps && (rc = check_jumps(prm->n_assets, rq.jp))) return rc;
    if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "volatility-targeted paths compound simply (no log compounding)");
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH))
      return fail(MCP_E_UNSUPPORTED, "volatility-targeted paths run on the unfolded recurrence and the spec's normals (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)");
    if (rq.exposure_stats_out && rq.dd)
      return fail(MCP_E_UNSUPPORTED, "a call leaves one second array: the exposure record is not combined with the drawdown");
    if (rq.src == SRC_BOOT || rq.src == SRC_FHS || rq.regimes || rq.rebalanced || rq.cash || rq.glide || rq.protect || rq.spend || rq.life ||
        rq.band || rq.overlay || rq.attr || rq.anti)
      return fail(MCP_E_UNSUPPORTED, "a volatility target is not combined with bootstrap or filtered rows, regimes, rebalancing, cash flows, "
                                     "glide paths, floor protection, spending rules, tolerance bands, the overlay, the attribution or "
                                     "antithetic pairs");
    if (ln) return fail(MCP_E_UNSUPPORTED, "volatility targeting is not wired into mcp_launch_paths*");
  }
  if (rq.underwater) {                                         // SPEC.md 4.20: two counters on the drawdown walk
    if (!rq.dd) return fail(MCP_E_ARG, "the time under water needs the drawdown walk: dd_stats_out is NULL");
    if (!rq.uw_longest_hist_out || !rq.uw_current_hist_out) return fail(MCP_E_ARG, "longest_hist_out or current_hist_out is NULL");
    if (rq.src == SRC_T && (rc = check_student_t(prm, rq.st))) return rc;
    if (rq.garch && (rc = check_garch(prm, rq.gv))) return rc;
    if (rq.jumps && (rc = check_jumps(prm->n_assets, rq.jp))) return rc;
    if (prm->n_steps > MCP_MAX_LIFE_STEPS)
      return fail(MCP_E_UNSUPPORTED, "time under water: n_steps=%d above MCP_MAX_LIFE_STEPS=%d", prm->n_steps, MCP_MAX_LIFE_STEPS);
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH))
      return fail(MCP_E_UNSUPPORTED, "the time under water runs on the unfolded recurrence and the spec's normals (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)");
    if (rq.src == SRC_BOOT || rq.src == SRC_FHS || rq.regimes || rq.rebalanced || rq.cash || rq.glide || rq.protect || rq.spend || rq.life ||
        rq.band || rq.vol_target || rq.overlay || rq.attr || rq.anti || rq.hz)
      return fail(MCP_E_UNSUPPORTED, "the time under water is not combined with bootstrap or filtered rows, regimes, rebalancing, cash flows, "
                                     "glide paths, floor protection, spending rules, tolerance bands, volatility targeting, the overlay, the "
                                     "attribution, antithetic pairs or horizons");
    if (ln) return fail(MCP_E_UNSUPPORTED, "the time under water is not wired into mcp_launch_paths*");
  }
  if (rq.uncertain) {                                          // SPEC.md 4.21: the factor, then what the per-path drift is not combined with
    if ((rc = check_drift_uncertainty(prm->n_assets, rq.du))) return rc;
    if (prm->flags & (MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH))
      return fail(MCP_E_UNSUPPORTED, "paths with drift uncertainty run on the unfolded recurrence and the spec's normals (no MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH)");
    if (rq.src != SRC_GAUSS || rq.st || rq.garch || rq.jumps || rq.regimes || rq.rebalanced || rq.band || rq.glide || rq.spend || rq.life ||
        rq.protect || rq.vol_target || rq.overlay || rq.attr || rq.anti || rq.underwater)
      return fail(MCP_E_UNSUPPORTED, "drift uncertainty is not combined with Student-t draws, GARCH, jumps, regimes, bootstrap or filtered rows, "
                                     "rebalancing, tolerance bands, glide paths, spending rules, the lifetime, floor protection, volatility "
                                     "targeting, the overlay, the attribution, antithetic pairs or the time under water");
    if (ln) return fail(MCP_E_UNSUPPORTED, "drift uncertainty is not wired into mcp_launch_paths*");
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

#ifndef MCP_EXP_LEAN        // 1: launches that pass mcp::lean_range run mc_paths_lean_kernel; 0: every launch stays on mc_paths_kernel
#define MCP_EXP_LEAN 1      // (tools/kernel_lab.py arms `lean` and `nolean`; profiles/lean_probe.json)
#endif

// Which kernel walks the paths of a checked request (mcp_route.h; the rows are mcp_paths_ladder.inc).  Every other request than a
// plain Gaussian walk of K >= 17 portfolios, which goes to the MFMA sweep kernels before this is asked (mcp_api.cpp), runs its
// family's kernel, K >= 2 as passes of the 8-portfolio kernel.
mcp::PathKernel route_kernel(const mcp_params* prm, const Request& rq, bool attr_walk, uint64_t path_begin, uint64_t n_paths) {
  using namespace mcp;
  const int nb = (prm->n_assets + 3) / 4;
  // Gaussian, Student-t and GARCH requests of a family with one walk run the GARCH walk on Student-t draws: without GARCH on
  // alpha = beta = 0, h0 = 1, which is the Gaussian or Student-t call bit for bit (SPEC.md 4.9)
  const auto share_garch_walk = [](uint32_t flags) { return (flags & ~(uint32_t)PK_STT) | PK_GV; };
  PathKernel k = {FAM_PLAIN, 0};
  if (prm->compounding == MCP_COMPOUND_LOG) k.flags |= PK_LOGC;
  if (rq.src == SRC_BOOT) k.flags |= PK_BOOT;
  if (rq.src == SRC_FHS) k.flags |= PK_BOOT | PK_FH;
  if (rq.src == SRC_FHS ? filt_fits_lds((uint64_t)rq.filt->n_rows, nb) : rq.src == SRC_BOOT && boot_fits_lds((uint64_t)rq.boot->n_rows, nb))
    k.flags |= PK_BLDS;
  if (rq.src == SRC_T) k.flags |= PK_STT;
  if (attr_walk) {                        // SPEC.md 4.10: one portfolio per pass.  The walk draws as the GARCH kernel does
    k.family = FAM_AT;
    k.flags = share_garch_walk(k.flags);
    return k;
  }
  k.family = rq.overlay ? FAM_OV : rq.cash ? FAM_CF : rq.rebalanced ? FAM_REB : rq.dd ? FAM_DD : rq.hz ? FAM_HZ : FAM_PLAIN;
  if (rq.src == SRC_FHS) k.family = FAM_HZ;            // SPEC.md 4.11: one segmented kernel serves terminal-only and horizon calls
  if (rq.overlay && rq.dd) k.flags |= PK_DD;
  if (rq.garch) k.flags = share_garch_walk(k.flags);   // the GARCH kernels draw Student-t, nu = 0 for Gaussian draws
  if (rq.jumps) k.flags |= PK_JP;
  if (rq.regimes) k.flags |= PK_RS;
  if (rq.glide) k.flags |= PK_GP;
  if (rq.spend) k.flags |= PK_SP;
  if (rq.life) k.flags |= PK_LT;
  if (rq.life && !rq.spend) k.flags |= PK_GP;          // SPEC.md 4.17: a plain cash-flow request runs the glide twin on G = 0 (no targets)
  if (rq.protect) {                       // SPEC.md 4.15: one segmented kernel serves terminal-only and horizon calls, on the GARCH or the jump walk
    k.family = rq.dd ? FAM_DD : FAM_HZ;
    k.flags |= PK_PI;
    if (!rq.jumps) k.flags = share_garch_walk(k.flags);
  }
  if (rq.vol_target) {                    // SPEC.md 4.19: the protection's two walks and families, with the targeting rule
    k.family = rq.dd ? FAM_DD : FAM_HZ;
    k.flags |= PK_VT;
    if (!rq.jumps) k.flags = share_garch_walk(k.flags);
  }
  if (rq.underwater) {                    // SPEC.md 4.20: the twins of the Gaussian, the GARCH and the jump drawdown kernels; a Student-t
    k.flags |= PK_UW;                     // request shares the GARCH walk
    if (k.flags & PK_STT) k.flags = share_garch_walk(k.flags);
  }
  if (rq.uncertain) k.flags |= PK_PU;     // SPEC.md 4.21: the request's own family; the flag also keeps the launch off the lean step loop below
  if (rq.band) k.flags |= PK_TB;          // SPEC.md 4.18: B is per portfolio, so every portfolio of a banded call is a pass of its own
  if (prm->n_portfolios > 1 && !rq.band) k.flags |= PK_KT8;
  if (prm->flags & MCP_FLAG_NATIVE_MATH) k.flags |= PK_NATIVE;
  if (prm->flags & MCP_FLAG_FOLD) k.flags |= PK_FOLD;
  if (rq.anti) {                          // SPEC.md 2.3: Student-t and GARCH requests share the GARCH walk, as the attribution does
    k.flags |= PK_ANTI;
    if (k.flags & (PK_STT | PK_GV)) k.flags = share_garch_walk(k.flags);
  }
  // the plain Gaussian walk of one portfolio whose paths share the high counter word runs the lean step loop (mcp_paths.h, UHI)
  if (MCP_EXP_LEAN && k.family == FAM_PLAIN && (k.flags & ~(uint32_t)PK_LOGC) == 0 && nb <= LEAN_MAX_NB && lean_range(path_begin, n_paths))
    k.flags |= PK_UHI;
  return k;
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

// SPEC.md 5.16: the spending rule on the mean path -- cash_pivots with the flow -wbar, wbar reviewed as the walk reviews w, on the
// doubles of the binary32 constants; out_wd[k] is the pivot of the total paid out (NULL: not asked for).  every = 0, or g = lo = hi = 1,
// is cash_pivots on c_s = -w0 operation for operation.
void spend_pivots(int K, int T, const double* m, const SpendConsts& c, int every, double v0, int H, const int32_t* steps, double* out_T,
                  double* out_hz, double* out_wd) {
  const auto pivot = [v0](double A) {
    const double x = (A > 0.0 ? A : 0.0) / v0 - 1.0;
    return std::isfinite(A) && std::isfinite(x) ? x : 0.0;
  };
  const double p = (double)c.p, gi = (double)c.g, lo = (double)c.lo, hi = (double)c.hi;
  for (int k = 0; k < K; k++) {
    const double g = 1.0 + m[k];
    double A = v0, w = (double)c.w0, Y = 0.0;
    int h = 0, nr = every >= 1 ? every : 0;
    for (int s = 1; s <= T; s++) {
      A = A * g;
      A = A + (-w);
      Y = Y + w;
      if (h < H && steps[h] == s) out_hz[(size_t)(h++) * K + k] = pivot(A);
      if (nr && s == nr) {
        const double wp = w * gi;
        w = std::fmin(std::fmax(p * (A > 0.0 ? A : 0.0), wp * lo), wp * hi);
        nr += every;
      }
    }
    if (out_T) out_T[k] = pivot(A);
    if (out_wd) {
      const double x = Y / v0 - 1.0;
      out_wd[k] = std::isfinite(x) ? x : 0.0;
    }
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

// SPEC.md 5.19: c_k(h) = g_k^h - 1, g_k = 1 + rf + e_k (mu_k - rf) - sp max(e_k - 1, 0), e_k = min(tgt / sqrt(s0_k), b), mu_k = sum_i W_ki mu_i
// (i ascending), binary64 from the binary32 constants; where g_k <= 0 or the result is not finite, the pivot of the plain call at h
// steps (mcp_pivots).  The portfolios [k0, k0 + K) of the call's W; h = T into out_T[k], the H horizons into out_hz[h*K + k].
void vol_target_pivots(const mcp_params& prm, const mcp_vol_target* vt, const float* mu, const float* chol, const float* W, int k0, int K,
                       int H, const int32_t* steps, double* out_T, double* out_hz) {
  const VolTargetConsts vc = vol_target_consts(vt);
  const double rf = (double)vc.rf, sp = (double)vc.sp;
  const int N = prm.n_assets;
  for (int k = 0; k < K; k++) {
    double mk = 0.0;
    for (int i = 0; i < N; i++) mk += (double)W[(size_t)(k0 + k) * N + i] * (double)mu[i];
    const double e = std::fmin((double)vc.tgt / std::sqrt((double)vol_target_s0(N, vt, chol, W, k0 + k)), (double)vc.b);
    const double g = 1.0 + rf + e * (mk - rf) - sp * std::fmax(e - 1.0, 0.0);
    for (int h = -1; h < H; h++) {
      const int st = h < 0 ? prm.n_steps : steps[h];
      double c = std::pow(g, (double)st) - 1.0;
      if (!(g > 0.0) || !std::isfinite(c)) {
        c = mk > -1.0 ? std::expm1((double)st * std::log1p(mk)) : 0.0;
        if (!std::isfinite(c)) c = 0.0;
      }
      (h < 0 ? out_T[k] : out_hz[(size_t)h * K + k]) = c;
    }
  }
}

// What follows the packed block of a tile of kt portfolios.  Jumps: the [N4] loadings; regimes: [mu1][L1 row pairs]; glide path: the
// target blocks of the tile's portfolios; bands: the tolerance table and the masks; drift uncertainty: M in the factor's row-pair layout
// (check_request lets at most one of the five through).  Protection: behind them the floor
// schedule and the counts' thresholds (protect_pack), or, volatility target, s0 of the tile's portfolios padded with ones to whole
// passes of 8.
TileLayout tile_layout(const mcp_params* prm, const Request& rq, int kt) {
  const int N = prm->n_assets;
  TileLayout t;
  t.base = t.load = mcp_packed_len(N, kt);
  t.floor = t.load + (rq.jumps ? (size_t)n4_of(N) : rq.regimes ? regime_block_len(N) : rq.glide ? glide_len(N, kt, rq.gl)
                       : rq.band ? band_len(N, kt) : rq.uncertain ? drift_len(N) : 0);
  t.total = t.floor + (rq.protect ? protect_len(prm->n_steps, kt, rq.hz ? rq.H : 0)
                       : rq.vol_target ? (size_t)KT_WIDE * (size_t)((kt + KT_WIDE - 1) / KT_WIDE) : 0);
  return t;
}

int tile_inputs(const mcp_params* prm, const Request& rq, TileInputs* in) {
  const int N = prm->n_assets;
  const bool boot = rq.src == SRC_BOOT, fhs = rq.src == SRC_FHS;
  in->zmu.assign(boot ? (size_t)N : 0, 0.0f);
  in->zchol.assign(boot || fhs ? (size_t)N * N : 0, 0.0f);
  in->jmu.resize(rq.jumps ? (size_t)N : 0);
  if (rq.jumps) jump_drift(rq.jp, jump_consts(rq.jp), N, rq.mu, in->jmu.data());
  in->blk1.clear();
  if (rq.regimes) {
    in->blk1.resize(mcp_packed_len(N, 1));
    if (int rc = mcp_pack_params(N, 1, rq.rs->mu1, rq.rs->chol1, rq.W, in->blk1.data(), in->blk1.size())) return rc;
  }
  in->rmu.resize(rq.rebalanced || fhs ? (size_t)N : 0);
  if (rq.rebalanced) reb_means(N, rq.mu, boot ? rq.boot : nullptr, in->rmu.data());
  if (fhs) filt_means(N, rq.filt, in->rmu.data());
  return MCP_OK;
}

// The packed block by the draw source -- bootstrap: no drift and no Cholesky factor (only W is read); filtered rows (SPEC.md 4.11):
// their drift, the factor zero; jumps: the compensated drift (the pivots keep the drift itself) -- then the layout's tail.
int pack_tile(const mcp_params* prm, const Request& rq, const TileInputs& in, int k0, int kt, float* out) {
  const int N = prm->n_assets, H = rq.hz ? rq.H : 0;
  const bool boot = rq.src == SRC_BOOT, fhs = rq.src == SRC_FHS;
  const TileLayout lay = tile_layout(prm, rq, kt);
  const float* mu = boot ? in.zmu.data() : fhs ? rq.filt->mu : rq.jumps ? in.jmu.data() : rq.mu;
  const float* chol = boot || fhs ? in.zchol.data() : rq.chol;
  if (int rc = mcp_pack_params(N, kt, mu, chol, rq.W + (size_t)k0 * N, out, lay.base)) return rc;
  float* load = out + lay.load;
  for (int i = 0; rq.jumps && i < n4_of(N); i++) load[i] = i < N ? (rq.jp->loading ? rq.jp->loading[i] : 1.0f) : 0.0f;
  if (rq.regimes) std::copy(in.blk1.begin(), in.blk1.begin() + (ptrdiff_t)regime_block_len(N), load);
  if (rq.glide) glide_pack(N, prm->n_portfolios, k0, kt, rq.gl, load);
  if (rq.band) band_pack(N, k0, kt, rq.bd, load);
  if (rq.uncertain) drift_pack(N, rq.du, load);
  if (rq.protect) protect_pack(prm->n_steps, kt, H, rq.steps, rq.pi, out + lay.floor);
  for (size_t k = 0; rq.vol_target && k < lay.total - lay.floor; k++)
    out[lay.floor + k] = k < (size_t)kt ? vol_target_s0(N, rq.vt, rq.chol, rq.W, k0 + (int)k) : 1.0f;
  return MCP_OK;
}

// One ordered choice of the pivot rule (SPEC.md 5); every arm writes T and all H horizons.
int request_pivots(const mcp_params* prm, const Request& rq, const TileInputs& in, int k0, int kt, double* out_T, double* out_hz) {
  const int N = prm->n_assets, T = prm->n_steps, H = rq.hz ? rq.H : 0;
  const float* Wt = rq.W + (size_t)k0 * N;
  const mcp_bootstrap* boot = rq.src == SRC_BOOT ? rq.boot : nullptr;
  const double v0 = (double)(float)prm->v0;
  if (rq.vol_target) {                                         // SPEC.md 5.19: every pivot in closed form
    vol_target_pivots(*prm, rq.vt, rq.mu, rq.chol, rq.W, k0, kt, H, rq.steps, out_T, out_hz);
  } else if (rq.protect) {                                     // SPEC.md 5.15: every pivot in closed form
    protect_pivots(*prm, rq.pi, rq.mu, Wt, kt, H, rq.steps, out_T, out_hz);
  } else if (rq.spend) {                                       // SPEC.md 5.16: the rule on the mean path gives T and every horizon
    std::vector<double> cm((size_t)kt);
    cash_means(N, kt, rq.mu, boot, Wt, cm.data());
    spend_pivots(kt, T, cm.data(), spend_consts(rq.sp, prm->v0), rq.sp->every, v0, H, rq.steps, out_T, out_hz, nullptr);
  } else if (rq.glide) {                                       // SPEC.md 5.14: one walk gives T and every horizon
    std::vector<double> cm((size_t)(rq.gl->n_breaks + 1) * kt);
    glide_means(N, prm->n_portfolios, k0, kt, rq.mu, boot, rq.W, rq.gl, cm.data());
    glide_pivots(kt, T, rq.gl->n_breaks, rq.gl->breaks, cm.data(), rq.cf->flows, v0, H, rq.steps, out_T, out_hz);
  } else if (rq.cash) {                                        // SPEC.md 5.6: one Horner walk gives T and every horizon
    std::vector<double> cm((size_t)kt);
    cash_means(N, kt, rq.mu, boot, Wt, cm.data());
    cash_pivots(kt, T, cm.data(), rq.cf->flows, v0, H, rq.steps, out_T, out_hz);
  } else if (rq.overlay && rq.ov->n_rows > 0) {                // SPEC.md 5.7: one walk; no rows: the pivots of the plain call
    overlay_pivots(N, kt, T, rq.ov, rq.mu, Wt, H, rq.steps, out_T, out_hz);
  } else if (rq.regimes) {                                     // SPEC.md 5.13: one recursion gives T and every horizon
    regime_pivots(N, kt, T, rq.mu, rq.rs->mu1, regime_consts(rq.rs), Wt, H, rq.steps, out_T, out_hz);
  } else {                                                     // SPEC.md 5.2 / 5.3: row h*kt + k is pivoted with n_steps = steps[h]
    std::vector<double> bm, bs2;
    if (boot && !rq.rebalanced) {                              // SPEC.md 5.3: the row moments, once per tile
      bm.resize((size_t)kt);
      bs2.resize((size_t)kt);
      boot_moments(N, boot, Wt, kt, bm.data(), bs2.data());
    }
    for (int h = -1; h < H; h++) {
      const int t = h < 0 ? T : rq.steps[h];
      double* out = h < 0 ? out_T : out_hz + (size_t)h * kt;
      if (rq.rebalanced) {                                     // SPEC.md 5.4: from the draws' per-asset means
        reb_pivots(N, kt, t, rq.reb->period, in.rmu.data(), Wt, out);
      } else if (boot) {
        for (int k = 0; k < kt; k++) out[k] = boot_pivot(prm->compounding, t, bm[(size_t)k], bs2[(size_t)k]);
      } else if (rq.src == SRC_FHS) {                          // SPEC.md 5.11: rmu holds mu_i + e_i
        filt_pivots(N, kt, t, in.rmu.data(), Wt, out);
      } else {
        mcp_params p = *prm;
        p.n_portfolios = kt;
        p.n_steps = t;
        if (int rc = mcp_pivots(&p, rq.mu, rq.chol, Wt, out)) return rc;
      }
    }
  }
  return MCP_OK;
}

void request_wd_pivots(const mcp_params* prm, const Request& rq, int k0, int kt, double* out_wd) {
  std::vector<double> cm((size_t)kt);
  cash_means(prm->n_assets, kt, rq.mu, rq.src == SRC_BOOT ? rq.boot : nullptr, rq.W + (size_t)k0 * prm->n_assets, cm.data());
  spend_pivots(kt, prm->n_steps, cm.data(), spend_consts(rq.sp, prm->v0), rq.sp->every, (double)(float)prm->v0, 0, nullptr, nullptr, nullptr, out_wd);
}

Second second_of(const Request& rq) {
  if (rq.dd) return {true, true, false, rq.mdd_out, rq.dd_stats_out};
  if (rq.band) return {true, true, false, rq.turnover_out, rq.turnover_stats_out};
  if (rq.spend) return {true, false, true, rq.wd_out, rq.wd_stats_out};
  if (rq.vol_target) return {true, true, false, rq.exposure_out, rq.exposure_stats_out};   // SPEC.md 5.19: x = Y - 1, without the drawdown only
  return {false, false, false, nullptr, nullptr};
}

Counted counted_of(const mcp_params* prm, const Request& rq) {
  if (rq.band) return {true, count_bins(prm, rq), rq.trades_out, rq.trade_hist_out, 1, nullptr, nullptr};
  if (rq.underwater)                                           // SPEC.md 5.20: m, then c_T
    return {true, count_bins(prm, rq), rq.uw_longest_out, rq.uw_longest_hist_out, 2, rq.uw_current_out, rq.uw_current_hist_out};
  return {rq.life, count_bins(prm, rq), rq.life ? rq.life_out : nullptr, rq.life ? rq.life_hist_out : nullptr, rq.life ? 1 : 0, nullptr, nullptr};
}

// A banded call is budgeted at 4 bytes more per path than its arrays hold (V_T, the horizon rows, Y and c): the figure it was
// introduced with, which decides the tile sizes of every banded call under a small budget.
constexpr size_t BAND_BUDGET_SLACK = sizeof(float);
size_t tile_bytes_per_path(const Request& rq) {
  return (1 + (rq.hz ? (size_t)rq.H : 0)) * sizeof(float) + (second_of(rq).on ? sizeof(float) : 0) +
         (rq.life || rq.band ? sizeof(uint32_t) : 0) + (rq.band ? BAND_BUDGET_SLACK : 0) + (rq.underwater ? 2 * sizeof(uint32_t) : 0) +
         (rq.rl.on ? sizeof(float) : 0);
}

int tile_portfolios(size_t budget, uint64_t n_paths, int K, size_t bytes_per_path) {
  const uint64_t fit = budget / (bytes_per_path * (n_paths ? n_paths : 1));
  if (fit >= (uint64_t)K) return K;
  if (fit >= (uint64_t)K_PAD) return (int)(fit / K_PAD) * K_PAD;
  return fit >= 1 ? (int)fit : 1;
}

bool TilePlan::walks(size_t s) const {
  for (size_t t = 0; t < tiles(); t++)
    if (tile(t)[s].active && tile(t)[s].pn) return true;
  return false;
}

TilePlan plan_tiles(size_t S, int K, uint64_t n_paths, bool by_portfolio, uint64_t unit, size_t budget, size_t bytes_per_path) {
  TilePlan plan;
  plan.S = S;
  std::vector<Job> jobs(S);
  if (by_portfolio) {
    const auto kb = [&](size_t s) { return (int)((int64_t)K * (int64_t)s / (int64_t)S); };
    std::vector<int> done(S, 0);
    for (bool more = true; more;) {
      more = false;
      for (size_t s = 0; s < S; s++) {
        const int left = kb(s + 1) - kb(s) - done[s];
        jobs[s] = Job();
        if (left <= 0) continue;
        const int kt = std::min(left, tile_portfolios(budget, n_paths, left, bytes_per_path));
        jobs[s].k0 = kb(s) + done[s]; jobs[s].kt = kt; jobs[s].p0 = 0; jobs[s].pn = n_paths; jobs[s].active = true;
        done[s] += kt;
        more = true;
      }
      if (more) plan.jobs.insert(plan.jobs.end(), jobs.begin(), jobs.end());
    }
    return plan;
  }
  uint64_t pn_max = 0;
  const uint64_t n_units = n_paths / unit;
  for (size_t s = 0; s < S; s++) {
    jobs[s].p0 = unit * (n_units / S * s + std::min<uint64_t>(s, n_units % S));
    jobs[s].pn = unit * (n_units / S + (s < n_units % S ? 1 : 0));
    jobs[s].active = true;
    pn_max = std::max(pn_max, jobs[s].pn);
  }
  const int kt_max = tile_portfolios(budget, pn_max, K, bytes_per_path);
  plan.jobs.reserve(S * (size_t)((K + kt_max - 1) / kt_max));
  for (int k0 = 0; k0 < K; k0 += kt_max) {
    for (size_t s = 0; s < S; s++) { jobs[s].k0 = k0; jobs[s].kt = std::min(kt_max, K - k0); }
    plan.jobs.insert(plan.jobs.end(), jobs.begin(), jobs.end());
  }
  return plan;
}

// SPEC.md 5.17: one pass over the cumulated histogram.  n = sum hist; level q's value is the smallest s with cum(s) > lo
int life_summary(const uint64_t* hist, int T, int n_levels, const double* levels, uint64_t* sum_out, uint32_t* q_out) {
  uint64_t n = 0, sum = 0;
  for (int s = 0; s <= T; s++) { n += hist[s]; sum += (uint64_t)s * hist[s]; }
  if (sum_out) *sum_out = sum;
  for (int l = 0; l < n_levels; l++) {
    if (n == 0) { q_out[l] = 0u; continue; }
    uint64_t lo, hi, cum = 0;
    double gamma;
    if (int rc = mcp_percentile_rank_q(n, levels[l], &lo, &hi, &gamma)) return rc;
    int s = 0;
    for (; s < T; s++) {
      cum += hist[s];
      if (cum > lo) break;
    }
    q_out[l] = (uint32_t)s;
  }
  return MCP_OK;
}

// SPEC.md 5.22: the request's own rules, the context aside
int check_downside(const mcp_downside* req, const mcp_downside_stats* stats_out) {
  if (!req) return fail(MCP_E_ARG, "downside request is NULL");
  if (!stats_out) return fail(MCP_E_ARG, "downside stats_out is NULL");
  if (!std::isfinite(req->tau)) return fail(MCP_E_ARG, "downside tau=%g is not finite", req->tau);
  if (req->reserved != 0) return fail(MCP_E_ARG, "downside reserved=%d must be 0", req->reserved);
  return MCP_OK;
}

void DownsideArm::arm(const mcp_downside& req, mcp_downside_sums* sums, mcp_downside_stats* stats, mcp_downside_stats* hz_stats) {
  on = true;
  tau = req.tau;
  use_rf = req.use_rf != 0;
  sums_out = sums;
  stats_out = stats;
  hz_stats_out = hz_stats;
}

DownsideArm DownsideArm::take() {
  const DownsideArm t = *this;
  *this = DownsideArm();
  return t;
}

// SPEC.md 5.23: the request's own rules, the context and the call aside
int check_relative(const mcp_relative* req, const mcp_relative_stats* stats_out) {
  if (!req) return fail(MCP_E_ARG, "relative request is NULL");
  if (!stats_out) return fail(MCP_E_ARG, "relative stats_out is NULL");
  if (req->bench < 0) return fail(MCP_E_ARG, "relative bench=%d is negative", req->bench);
  if (req->reserved != 0) return fail(MCP_E_ARG, "relative reserved=%d must be 0", req->reserved);
  return MCP_OK;
}

void RelativeArm::arm(const mcp_relative& req, mcp_relative_sums* sums, mcp_relative_stats* stats, mcp_stats* active_stats, float* active,
                      mcp_relative_stats* hz_stats) {
  on = true;
  bench = req.bench;
  sums_out = sums;
  stats_out = stats;
  active_stats_out = active_stats;
  active_out = active;
  hz_stats_out = hz_stats;
}

RelativeArm RelativeArm::take() {
  const RelativeArm t = *this;
  *this = RelativeArm();
  return t;
}

int check_relative_plan(const TilePlan& plan, int K, bool by_portfolio) {
  if (by_portfolio && plan.S > 1)
    return fail(MCP_E_ARG, "a relative request needs the benchmark's row on every shard: shard by paths, not by portfolios");
  for (const Job& j : plan.jobs)
    if (j.active && (j.k0 != 0 || j.kt != K))
      return fail(MCP_E_ARG, "a relative request needs all %d portfolios in one tile, the terminal budget holds %d: raise the budget or "
                  "shard by paths", K, j.kt);
  return MCP_OK;
}

int check_sweep_perf(int N, int R, int P, const double* returns, const double* W, double risk_free, double ann_factor,
                     const mcp_sweep_perf_stats* stats_out) {
  if (N < 1 || N > MCP_MAX_ASSETS) return fail(MCP_E_ARG, "n_assets=%d outside [1,%d]", N, MCP_MAX_ASSETS);
  if (R < 2 || R > MCP_SWEEP_MAX_ROWS) return fail(MCP_E_ARG, "n_rows=%d outside [2,%d]", R, MCP_SWEEP_MAX_ROWS);
  if (P < 0) return fail(MCP_E_ARG, "n_portfolios=%d < 0", P);
  if (!(ann_factor > 0.0) || !std::isfinite(ann_factor)) return fail(MCP_E_ARG, "ann_factor=%g is not finite and > 0", ann_factor);
  if (!std::isfinite(risk_free)) return fail(MCP_E_ARG, "risk_free=%g is not finite", risk_free);
  if (!returns) return fail(MCP_E_ARG, "returns is NULL");
  if (P == 0) return MCP_OK;
  if (!W) return fail(MCP_E_ARG, "W is NULL");
  if (!stats_out) return fail(MCP_E_ARG, "stats_out is NULL");
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
  return MCP_OK;
}

// SPEC.md 5.25: the replicate range and the block of a resampled sweep
int check_boot_replicates(uint64_t replicate_begin, int B, int R, double block) {
  if (R < 2 || R > MCP_SWEEP_MAX_ROWS) return fail(MCP_E_ARG, "n_rows=%d outside [2,%d]", R, MCP_SWEEP_MAX_ROWS);
  if (B < 0 || B > MCP_SWEEP_MAX_REPLICATES) return fail(MCP_E_ARG, "n_replicates=%d outside [0,%d]", B, MCP_SWEEP_MAX_REPLICATES);
  if (!(block >= 1.0)) return fail(MCP_E_ARG, "block=%g must be >= 1 (or +inf)", block);
  if (replicate_begin + (uint64_t)B < replicate_begin)
    return fail(MCP_E_ARG, "replicate_begin=%llu + n_replicates=%d wraps", (unsigned long long)replicate_begin, B);
  return MCP_OK;
}

int check_sweep_boot(int N, int R, int P, const double* returns, const double* W, double rf, double ann_factor, double alpha,
                     uint64_t replicate_begin, int B, double block, const double* scores_out, const int32_t* opt_out) {
  if (N < 1 || N > MCP_MAX_ASSETS) return fail(MCP_E_ARG, "n_assets=%d outside [1,%d]", N, MCP_MAX_ASSETS);
  if (R < 2 || R > MCP_SWEEP_MAX_ROWS) return fail(MCP_E_ARG, "n_rows=%d outside [2,%d]", R, MCP_SWEEP_MAX_ROWS);
  if (P < 0) return fail(MCP_E_ARG, "n_portfolios=%d < 0", P);
  if (int rc = check_boot_replicates(replicate_begin, B, R, block)) return rc;
  if ((uint64_t)P * (uint64_t)B > ((uint64_t)1 << 27))
    return fail(MCP_E_ARG, "n_portfolios=%d * n_replicates=%d exceeds 2^27 scores per figure", P, B);
  if (!(ann_factor > 0.0) || !std::isfinite(ann_factor)) return fail(MCP_E_ARG, "ann_factor=%g is not finite and > 0", ann_factor);
  if (!std::isfinite(rf)) return fail(MCP_E_ARG, "rf=%g is not finite", rf);
  if (!(alpha > 0.0 && alpha < 1.0)) return fail(MCP_E_ARG, "alpha=%g outside (0,1)", alpha);
  if (!returns) return fail(MCP_E_ARG, "returns is NULL");
  if (P == 0 || B == 0) return MCP_OK;
  if (!W) return fail(MCP_E_ARG, "W is NULL");
  if (!scores_out) return fail(MCP_E_ARG, "scores_out is NULL");
  if (!opt_out) return fail(MCP_E_ARG, "opt_out is NULL");
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
  return MCP_OK;
}

namespace {
// Philox4x32-10 (SPEC.md 2), the words x0 and x1 of the block on counter (c0, c1, c2, c3) under key (k0, k1)
inline void philox_x01(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* x0, uint32_t* x1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  *x0 = c0;
  *x1 = c1;
}
}  // namespace

}  // namespace mcph

using namespace mcph;

// SPEC.md 5.25: the rows of replicate g are those of path g of SPEC.md 2.1 with T = R steps on R rows; only their counts leave
int mcp_sweep_boot_counts(uint64_t seed, uint64_t replicate_begin, int B, int R, double block, uint16_t* counts_out) {
  if (int rc = check_boot_replicates(replicate_begin, B, R, block)) return rc;
  if (B == 0) return MCP_OK;
  if (!counts_out) return fail(MCP_E_ARG, "counts_out is NULL");
  const uint64_t thr = boot_threshold(block);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int q = 0; q < B; q++) {
    const uint64_t g = replicate_begin + (uint64_t)q;
    uint16_t* c = counts_out + (size_t)q * (size_t)R;
    for (int r = 0; r < R; r++) c[r] = 0;
    uint32_t j = 0;
    for (int t = 0; t < R; t++) {
      uint32_t x0, x1;
      philox_x01((uint32_t)t, 1u, (uint32_t)g, (uint32_t)(g >> 32), k0, k1, &x0, &x1);
      const uint32_t start = (uint32_t)(((uint64_t)x0 * (uint64_t)R) >> 32), next = j + 1u;
      j = (t == 0 || (uint64_t)x1 < thr) ? start : (next == (uint32_t)R ? 0u : next);
      c[j] = (uint16_t)(c[j] + 1);
    }
  }
  return MCP_OK;
}

// SPEC.md 5.24: every operation below is one binary64 operation in the reference's order (-ffp-contract=off); sweep.performance_finish
// repeats it.  n_neg == 1 divides 0 by 0 and a zero downside_std divides by IEEE rules, both as the reference does.
int mcp_sweep_perf_finish(const mcp_sweep_perf_sums* s, double ann_factor, mcp_sweep_perf_stats* out) {
  if (!s || !out) return fail(MCP_E_ARG, "NULL pointer");
  if (!(ann_factor > 0.0) || !std::isfinite(ann_factor)) return fail(MCP_E_ARG, "ann_factor=%g is not finite and > 0", ann_factor);
  const double n = (double)s->n, nn = (double)s->n_neg, root = std::sqrt(ann_factor);
  mcp_sweep_perf_stats o;
  const double mean_excess = s->S / n;
  const double sd = std::sqrt(s->M2 / (n - 1.0));
  o.sharpe_ratio = sd == 0.0 ? 0.0 : mean_excess / sd * root;
  const double downside_std = s->n_neg == 0 ? 1e-4 : std::sqrt(s->M2_neg / (nn - 1.0));
  o.sortino_ratio = mean_excess / downside_std * root;
  o.annual_volatility = sd * root;
  o.annual_return = std::pow(s->prod, ann_factor / n) - 1.0;
  o.max_drawdown = s->mdd;
  o.calmar = s->mdd == 0.0 ? 0.0 : o.annual_return / std::fabs(s->mdd);
  o.peak_row = s->peak_row;
  o.trough_row = s->trough_row;
  *out = o;
  return MCP_OK;
}

// SPEC.md 5.23: every operation below is one binary64 operation in the order written (-ffp-contract=off); relative.finish repeats it
int mcp_relative_finish(const mcp_relative_sums* s, double pivot, double bench_pivot, mcp_relative_stats* out) {
  if (!s || !out) return fail(MCP_E_ARG, "NULL pointer");
  const double n = (double)s->n, nu = (double)s->n_under, no = (double)s->n_over;
  mcp_relative_stats o;
  const double el = s->n ? s->e1 / n : 0.0;
  o.active_mean = (pivot - bench_pivot) + el;
  const double q = s->e2 - s->e1 * el;
  o.tracking_error = s->n >= 2 ? std::sqrt((q > 0.0 ? q : 0.0) / (n - 1.0)) : 0.0;
  o.information_ratio = o.tracking_error > 0.0 ? o.active_mean / o.tracking_error : 0.0;
  o.p_under = s->n ? nu / n : 0.0;
  o.p_over = s->n ? no / n : 0.0;
  o.mean_underperformance = s->n_under ? s->u1 / nu : 0.0;
  o.relative_downside_deviation = s->n ? std::sqrt(s->u2 / n) : 0.0;
  const double kl = s->n ? s->k1 / n : 0.0, bl = s->n ? s->b1 / n : 0.0;
  const double vk = s->k2 - s->k1 * kl, vb = s->b2 - s->b1 * bl, ckb = s->kb - s->k1 * bl;
  o.beta = vb > 0.0 ? ckb / vb : 0.0;
  const double mk = pivot + kl, mb = bench_pivot + bl;
  o.alpha = mk - o.beta * mb;
  const double vv = vk > 0.0 && vb > 0.0 ? vk * vb : 0.0;
  const double rho = vv > 0.0 ? ckb / std::sqrt(vv) : 0.0;
  o.correlation = rho > 1.0 ? 1.0 : (rho < -1.0 ? -1.0 : rho);
  o.up_capture = s->n_up && s->up_b != 0.0 ? s->up_k / s->up_b : 0.0;
  o.down_capture = s->n_down && s->down_b != 0.0 ? s->down_k / s->down_b : 0.0;
  o.pivot = pivot;
  o.bench_pivot = bench_pivot;
  *out = o;
  return MCP_OK;
}

// SPEC.md 5.22: every operation below is one binary64 operation in the order written (-ffp-contract=off); downside.finish repeats it
int mcp_downside_finish(const mcp_downside_sums* s, double tau, double pivot, mcp_downside_stats* out) {
  if (!s || !out) return fail(MCP_E_ARG, "NULL pointer");
  const double n = (double)s->n, nb = (double)s->n_below;
  const double dl = s->n ? s->s1 / n : 0.0;
  mcp_downside_stats o;
  o.mean = pivot + dl;
  const double dl2 = dl * dl;
  const double m2 = s->s2 - s->s1 * dl;
  const double m3 = (s->s3 - (3.0 * dl) * s->s2) + ((2.0 * n) * dl) * dl2;
  const double m4 = ((s->s4 - (4.0 * dl) * s->s3) + (6.0 * dl2) * s->s2) - ((3.0 * n) * dl2) * dl2;
  if (m2 > 0.0) {
    const double v = m2 / n;
    o.skewness = (m3 / n) / (v * std::sqrt(v));
    o.excess_kurtosis = (n * m4) / (m2 * m2) - 3.0;
  } else {
    o.skewness = 0.0;
    o.excess_kurtosis = 0.0;
  }
  if (s->n_below >= 2) {
    const double q = s->b2 - (s->b1 * s->b1) / nb;
    o.downside_std = std::sqrt((q > 0.0 ? q : 0.0) / (nb - 1.0));
  } else {
    o.downside_std = s->n_below == 1 ? std::nan("") : 1e-4;
  }
  const double ex = o.mean - tau;
  o.sortino = ex / o.downside_std;
  o.downside_deviation = s->n ? std::sqrt(s->l2 / n) : 0.0;
  o.sortino_target = o.downside_deviation > 0.0 ? ex / o.downside_deviation : 0.0;
  o.p_below = s->n ? nb / n : 0.0;
  o.mean_shortfall = s->n_below ? s->l1 / nb : 0.0;
  o.omega = s->l1 == 0.0 ? HUGE_VAL : s->u1 / (-s->l1);
  o.pivot = pivot;
  *out = o;
  return MCP_OK;
}

int mcp_lifetime_summary(const uint64_t* hist, int n_steps, int n_levels, const double* levels, uint64_t* sum_out, uint32_t* q_out) {
  if (!hist || !sum_out) return fail(MCP_E_ARG, "NULL pointer");
  if (n_steps < 0 || n_steps > MCP_MAX_LIFE_STEPS) return fail(MCP_E_ARG, "n_steps=%d outside [0,%d]", n_steps, MCP_MAX_LIFE_STEPS);
  if (int rc = check_levels(n_levels, levels)) return rc;
  if ((q_out == nullptr) != (n_levels == 0)) return fail(MCP_E_ARG, "q_out must be NULL exactly when n_levels == 0");
  uint64_t n = 0;
  for (int s = 0; s <= n_steps; s++) {
    if (hist[s] > UINT64_MAX - n) return fail(MCP_E_ARG, "the histogram's total overflows 64 bits");
    n += hist[s];
  }
  if (n_levels && n == 0) return fail(MCP_E_ARG, "an empty histogram has no quantile");
  if (n > UINT64_MAX / (uint64_t)(n_steps > 0 ? n_steps : 1)) return fail(MCP_E_ARG, "life_sum overflows 64 bits");
  return life_summary(hist, n_steps, n_levels, levels, sum_out, q_out);
}

int mcp_band_reviews(const mcp_params* prm, const mcp_band* bd) {
  if (!prm || !bd) { (void)fail(MCP_E_ARG, "NULL pointer"); return -1; }
  if (prm->n_steps < 0 || bd->every < 0) { (void)fail(MCP_E_ARG, "n_steps=%d or every=%d < 0", prm->n_steps, bd->every); return -1; }
  return band_reviews(prm->n_steps, bd->every);
}

extern "C" {

int mcp_abi_version(void) { return MCP_ABI_VERSION; }

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

int mcp_vol_target_pivots(const mcp_params* prm, const mcp_vol_target* vt, const float* mu, const float* chol, const float* W, int n_horizons,
                          const int32_t* horizons, double* pivots_out, double* hz_pivots_out) {
  if (int rc = check_params(prm)) return rc;
  if (!mu || !chol || !W || !pivots_out) return fail(MCP_E_ARG, "NULL pointer");
  if (int rc = check_vol_target(prm, vt, chol, W)) return rc;
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "volatility-targeted paths compound simply (no log compounding)");
  if (n_horizons != 0) {
    if (int rc = check_horizons(prm->n_steps, n_horizons, horizons)) return rc;
    if (!hz_pivots_out) return fail(MCP_E_ARG, "hz_pivots_out is NULL");
  }
  vol_target_pivots(*prm, vt, mu, chol, W, 0, prm->n_portfolios, n_horizons, horizons, pivots_out, hz_pivots_out);
  return MCP_OK;
}

int mcp_vol_target_consts(const mcp_params* prm, const mcp_vol_target* vt, const float* chol, const float* W, float* out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_vol_target(prm, vt, chol, W)) return rc;
  if (!out) return fail(MCP_E_ARG, "out is NULL");
  const VolTargetConsts c = vol_target_consts(vt);
  out[0] = c.tgt; out[1] = c.lam; out[2] = c.oml; out[3] = c.b; out[4] = c.rf; out[5] = c.sp;
  for (int k = 0; k < prm->n_portfolios; k++) out[6 + k] = vol_target_s0(prm->n_assets, vt, chol, W, k);
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

int mcp_spending_pivots(const mcp_params* prm, const mcp_spending* sp, const float* mu, const mcp_bootstrap* boot, const float* W,
                        int n_horizons, const int32_t* horizons, double* pivots_out, double* hz_pivots_out, double* wd_pivots_out) {
  if (int rc = check_params(prm)) return rc;
  if (int rc = check_spending(prm->v0, sp)) return rc;
  if ((mu == nullptr) == (boot == nullptr)) return fail(MCP_E_ARG, "exactly one of mu and boot");
  if (boot)
    if (int rc = check_boot(prm, boot)) return rc;
  if (!W || !pivots_out || !wd_pivots_out) return fail(MCP_E_ARG, "NULL pointer");
  if (n_horizons != 0) {
    if (int rc = check_horizons(prm->n_steps, n_horizons, horizons)) return rc;
    if (!hz_pivots_out) return fail(MCP_E_ARG, "hz_pivots_out is NULL");
  }
  if (prm->compounding != MCP_COMPOUND_SIMPLE) return fail(MCP_E_UNSUPPORTED, "paths with a spending rule compound simply (no log compounding)");
  std::vector<double> m((size_t)prm->n_portfolios);
  cash_means(prm->n_assets, prm->n_portfolios, mu, boot, W, m.data());
  spend_pivots(prm->n_portfolios, prm->n_steps, m.data(), spend_consts(sp, prm->v0), sp->every, (double)(float)prm->v0, n_horizons, horizons,
               pivots_out, hz_pivots_out, wd_pivots_out);
  return MCP_OK;
}

int mcp_spending_consts(const mcp_spending* sp, double v0, float* out) {
  if (int rc = check_spending(v0, sp)) return rc;
  if (!out) return fail(MCP_E_ARG, "out is NULL");
  const SpendConsts c = spend_consts(sp, v0);
  out[0] = c.p; out[1] = c.g; out[2] = c.lo; out[3] = c.hi; out[4] = c.w0;
  return MCP_OK;
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

}  // extern "C"

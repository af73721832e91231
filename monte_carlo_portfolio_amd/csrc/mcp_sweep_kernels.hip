// mcp_sweep_kernels.hip -- the reference's own "Monte Carlo": the random-weight sweep over HISTORICAL
// returns, loop body of app.py:708-713 evaluated for P weight vectors at once, in binary64 like the
// reference (NumPy/pandas defaults).
//
//   port_return = w . mean_returns                     app.py:708
//   port_std    = sqrt(w^T (cov w))                    app.py:709
//   port_series = returns_df @ w                       app.py:710   [R]
//   sharpe      = (port_return - rf)/port_std or 0     app.py:711   (rf in the reference's units, Q2)
//   var_95      = np.percentile(port_series, (1-a)*100) app.py:712 -> 258-259
//   cvar_95     = port_series[port_series <= var].mean() app.py:713 -> 261-263
//
// Up to 256 rows (the reference's own sizes: 13 monthly ... 252 daily rows): one 64-lane wave per portfolio, the series in
// LDS, the two order statistics by rank counting (O(R^2) compares, a few microseconds for 2,500 portfolios x 13 rows).
// Beyond: one 256-thread workgroup per portfolio and an in-LDS bitonic sort of the series (O(R log^2 R)): 2,500 portfolios x
// 4,096 rows in milliseconds instead of 16 M compares per portfolio.  Same values either way (order statistics are exact;
// the tail sum differs in association only).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcport.h"
#include "mcp_reduce.h"
#include "mcp_stats_kernels.h"

namespace mcp {

// The tail sum as an unevaluated pair s + c: c collects what every addition rounds away (Knuth's TwoSum, exact here because the
// build neither contracts nor reassociates), so the sum is the exact one rounded once, in whatever order the lanes add.  A plain
// tree of R / 256 + 8 additions is off by up to that many roundings of the running sum, which a tail of equal or nearly equal
// values shows in the last digits of the mean.
struct Sum2 {
  double s, c;
};
__device__ __forceinline__ void add2(Sum2& a, double x) {
  const double t = a.s + x, bp = t - a.s;
  a.c += (a.s - (t - bp)) + (x - bp);
  a.s = t;
}
__device__ __forceinline__ Sum2 wsum2(Sum2 a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_xor(a.s, o, 64), oc = __shfl_xor(a.c, o, 64);
    add2(a, os);
    a.c += oc;
  }
  return a;
}
// The tail mean, kept inside its range [smallest tail element, VaR]: even the exact sum, rounded and divided by the count, can leave
// it by an ulp when the tail is one value repeated (three times 0.1, over 3, is above 0.1), and CVaR <= VaR is what callers rely on.
__device__ __forceinline__ double tail_mean(Sum2 sum, double cnt, double lo, double v) {
  return cnt > 0.0 ? fmin(fmax((sum.s + sum.c) / cnt, lo), v) : v;
}

// grid = P, block = 64, dynamic LDS = (R + N) doubles
__global__ void __launch_bounds__(64) sweep_hist_kernel(int N, int R, const double* __restrict__ returns,
                                                        const double* __restrict__ mean, const double* __restrict__ cov,
                                                        const double* __restrict__ W, double rf, uint64_t rank_lo,
                                                        uint64_t rank_hi, double gamma, double* __restrict__ out_ret,
                                                        double* __restrict__ out_std, double* __restrict__ out_sharpe,
                                                        double* __restrict__ out_var, double* __restrict__ out_cvar) {
  extern __shared__ double lds[];
  double* series = lds;        // [R]
  double* w = lds + R;         // [N]
  const int p = blockIdx.x, lane = threadIdx.x;
  for (int i = lane; i < N; i += 64) w[i] = W[(size_t)p * N + i];
  __syncthreads();

  // analytic moments
  double pr = 0.0, pv = 0.0;
  for (int i = lane; i < N; i += 64) {
    pr += w[i] * mean[i];
    double cw = 0.0;
    for (int j = 0; j < N; j++) cw += cov[(size_t)i * N + j] * w[j];
    pv += w[i] * cw;
  }
  pr = wave_sum(pr);
  pv = wave_sum(pv);
  const double sd = sqrt(pv);

  // historical portfolio return series
  for (int r = lane; r < R; r += 64) {
    double s = 0.0;
    for (int i = 0; i < N; i++) s += returns[(size_t)r * N + i] * w[i];
    series[r] = s;
  }
  __syncthreads();

  // order statistics rank_lo / rank_hi by (stable) rank counting
  double a_part = 0.0, b_part = 0.0;
  for (int r = lane; r < R; r += 64) {
    const double x = series[r];
    uint64_t rk = 0;
    for (int q = 0; q < R; q++) {
      const double y = series[q];
      rk += (y < x) || (y == x && q < r);
    }
    if (rk == rank_lo) a_part = x;
    if (rk == rank_hi) b_part = x;
  }
  // exactly one lane holds each; all others contribute +0.0 (x + 0.0 == x, also for -0.0 + 0.0 -> +0.0: harmless)
  const double a = wave_sum(a_part), b = wave_sum(b_part);
  const double diff = b - a;
  double v = a + diff * gamma;                    // numpy _lerp
  if (gamma >= 0.5) v = b - diff * (1.0 - gamma);

  double cnt = 0.0, lo = v;
  Sum2 sum = {0.0, 0.0};
  for (int r = lane; r < R; r += 64) {
    const double x = series[r];
    if (x <= v) { cnt += 1.0; add2(sum, x); lo = fmin(lo, x); }
  }
  cnt = wave_sum(cnt);
  sum = wsum2(sum);
  lo = wave_min(lo);
  if (lane == 0) {
    out_ret[p] = pr;
    out_std[p] = sd;
    out_sharpe[p] = sd > 0.0 ? (pr - rf) / sd : 0.0;
    out_var[p] = v;
    out_cvar[p] = tail_mean(sum, cnt, lo, v);
  }
}

// ---- R > 256: sort instead of counting ranks ---------------------------------------------------------------------------
constexpr int SORT_BLOCK = 256;
__device__ __forceinline__ Sum2 bsum2(Sum2 a, double* red /* [8] LDS */) {
  a = wsum2(a);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a.s; red[4 + (threadIdx.x >> 6)] = a.c; }
  __syncthreads();
  Sum2 r = {red[0], red[4]};
  for (int i = 1; i < 4; i++) { add2(r, red[i]); r.c += red[4 + i]; }
  return r;
}

// grid = P, block = 256, dynamic LDS = (R2 + N) doubles, R2 = R rounded up to a power of two
__global__ void __launch_bounds__(SORT_BLOCK) sweep_hist_sorted_kernel(int N, int R, int R2, const double* __restrict__ returns,
                                                                       const double* __restrict__ mean, const double* __restrict__ cov,
                                                                       const double* __restrict__ W, double rf, uint64_t rank_lo,
                                                                       uint64_t rank_hi, double gamma, double* __restrict__ out_ret,
                                                                       double* __restrict__ out_std, double* __restrict__ out_sharpe,
                                                                       double* __restrict__ out_var, double* __restrict__ out_cvar) {
  extern __shared__ double lds[];
  __shared__ double red[8];
  double* series = lds;        // [R2], sorted in place
  double* w = lds + R2;        // [N]
  const int p = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < N; i += SORT_BLOCK) w[i] = W[(size_t)p * N + i];
  __syncthreads();

  // analytic moments (the same per-lane expressions as the one-wave kernel)
  double pr = 0.0, pv = 0.0;
  for (int i = tid; i < N; i += SORT_BLOCK) {
    pr += w[i] * mean[i];
    double cw = 0.0;
    for (int j = 0; j < N; j++) cw += cov[(size_t)i * N + j] * w[j];
    pv += w[i] * cw;
  }
  pr = block_sum(pr, red);
  pv = block_sum(pv, red);
  const double sd = sqrt(pv);

  // historical portfolio return series (app.py:710), padded with +inf up to the power of two
  for (int r = tid; r < R2; r += SORT_BLOCK) {
    double x = __builtin_inf();
    if (r < R) {
      x = 0.0;
      for (int i = 0; i < N; i++) x += returns[(size_t)r * N + i] * w[i];
    }
    series[r] = x;
  }
  __syncthreads();

  // bitonic sort, ascending
  for (int k = 2; k <= R2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < R2 / 2; t += SORT_BLOCK) {
        const int i = 2 * t - (t & (j - 1));           // lower index of the t-th pair at distance j
        const int l = i + j;
        const bool up = (i & k) == 0;
        const double a = series[i], b = series[l];
        if ((a > b) == up) { series[i] = b; series[l] = a; }
      }
      __syncthreads();
    }
  }
  const double a = series[rank_lo], b = series[rank_hi];
  const double diff = b - a;
  double v = a + diff * gamma;                    // numpy _lerp
  if (gamma >= 0.5) v = b - diff * (1.0 - gamma);

  double cnt = 0.0;
  Sum2 sum = {0.0, 0.0};
  for (int r = tid; r < R; r += SORT_BLOCK) {
    const double x = series[r];
    if (x <= v) { cnt += 1.0; add2(sum, x); }
  }
  cnt = block_sum(cnt, red);
  sum = bsum2(sum, red);
  if (tid == 0) {
    out_ret[p] = pr;
    out_std[p] = sd;
    out_sharpe[p] = sd > 0.0 ? (pr - rf) / sd : 0.0;
    out_var[p] = v;
    out_cvar[p] = tail_mean(sum, cnt, series[0], v);   // sorted: series[0] is the smallest
  }
}

hipError_t launch_sweep_hist(int N, int R, int P, const double* returns, const double* mean, const double* cov,
                             const double* W, double rf, uint64_t rank_lo, uint64_t rank_hi, double gamma,
                             double* out5 /* [5][P] */, hipStream_t s) {
  if (R > 256) {
    int R2 = 512;
    while (R2 < R) R2 <<= 1;
    const size_t lds = (size_t)(R2 + N) * sizeof(double);          // <= (4096 + 64) * 8 = 33,280 B
    sweep_hist_sorted_kernel<<<P, SORT_BLOCK, lds, s>>>(N, R, R2, returns, mean, cov, W, rf, rank_lo, rank_hi, gamma, out5, out5 + P,
                                                        out5 + 2 * (size_t)P, out5 + 3 * (size_t)P, out5 + 4 * (size_t)P);
    return hipGetLastError();
  }
  const size_t lds = (size_t)(R + N) * sizeof(double);
  sweep_hist_kernel<<<P, 64, lds, s>>>(N, R, returns, mean, cov, W, rf, rank_lo, rank_hi, gamma, out5, out5 + P,
                                       out5 + 2 * (size_t)P, out5 + 3 * (size_t)P, out5 + 4 * (size_t)P);
  return hipGetLastError();
}

// ---- series statistics of every portfolio (SPEC.md 5.24, include/mcport_sweep_perf.h) ----------------------------------------
// The order of the sums is the definition (rows ascending, one binary64 operation at a time), so the parallelism is across
// portfolios: one lane per portfolio, 64 portfolios per wave, every lane walking the rows itself.  A row of `returns` is the same
// for the whole wave (a uniform address: scalar loads); a lane's weights sit in LDS transposed, wt[i * 64 + lane], so lane l reads
// bank pair l -- no conflict, no register array, no scratch.  The series is formed twice with the same expression, hence the same
// bits: pass 1 takes the sums and the wealth recurrence, pass 2 the squared deviations about the means of pass 1 (two passes, as
// np.std takes them).
constexpr int PERF_LANES = 64;
__device__ __forceinline__ double perf_x(const double* __restrict__ row, const double* __restrict__ wt, int N) {
  double x = 0.0;
  for (int i = 0; i < N; i++) x += row[i] * wt[i * PERF_LANES];
  return x;
}

// grid = ceil(P / 64), block = 64, dynamic LDS = N * 64 doubles (<= 32 KiB)
__global__ void __launch_bounds__(PERF_LANES) sweep_perf_kernel(int N, int R, int P, const double* __restrict__ returns,
                                                                const double* __restrict__ W, double rf_step,
                                                                mcp_sweep_perf_sums* __restrict__ out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int p0 = blockIdx.x * PERF_LANES;
  const int live = min(PERF_LANES, P - p0);          // portfolios of this wave: the ragged last wave has fewer than 64
  // the wave's weight rows are one contiguous block of `live` * N doubles: coalesced reads, transposed on the way into LDS;
  // the columns of absent portfolios are 0.0, so their lanes walk finite numbers and write nothing
  for (int t = lane; t < PERF_LANES * N; t += PERF_LANES) {
    const int q = t / N, i = t - q * N;
    lds[i * PERF_LANES + q] = q < live ? W[(size_t)p0 * N + t] : 0.0;
  }
  __syncthreads();
  const double* wt = lds + lane;

  // pass 1: S, n_neg, S_neg, and the wealth recurrence of max_drawdown
  double S = 0.0, S_neg = 0.0;
  int n_neg = 0;
  double c, peak, mdd;
  int peak_cur = 0, peak_row = 0, trough_row = 0;
  bool dd_nan;
  {
    const double x = perf_x(returns, wt, N);
    const double e = x - rf_step;
    S += e;
    if (e < 0.0) { n_neg++; S_neg += e; }
    c = 1.0 + x;
    peak = c;
    mdd = (c - peak) / peak;
    dd_nan = mdd != mdd;
  }
  for (int r = 1; r < R; r++) {
    const double x = perf_x(returns + (size_t)r * N, wt, N);
    const double e = x - rf_step;
    S += e;
    if (e < 0.0) { n_neg++; S_neg += e; }
    c = c * (1.0 + x);
    if (c > peak) { peak = c; peak_cur = r; }
    const double dd = (c - peak) / peak;
    dd_nan |= dd != dd;
    if (dd < mdd) { mdd = dd; trough_row = r; peak_row = peak_cur; }
  }

  // pass 2: squared deviations about the means of pass 1
  const double mean = S / (double)R, mean_neg = S_neg / (double)n_neg;
  double M2 = 0.0, M2_neg = 0.0;
  for (int r = 0; r < R; r++) {
    const double e = perf_x(returns + (size_t)r * N, wt, N) - rf_step;
    const double d = e - mean;
    M2 += d * d;
    if (e < 0.0) { const double dn = e - mean_neg; M2_neg += dn * dn; }
  }

  if (lane < live) {
    mcp_sweep_perf_sums o;
    o.n = R;
    o.n_neg = n_neg;
    o.peak_row = dd_nan ? -1 : peak_row;
    o.trough_row = dd_nan ? -1 : trough_row;
    o.S = S;
    o.S_neg = S_neg;
    o.M2 = M2;
    o.M2_neg = M2_neg;
    o.prod = c;
    o.mdd = dd_nan ? __builtin_nan("") : mdd;
    out[p0 + lane] = o;
  }
}

hipError_t launch_sweep_perf(int N, int R, int P, const double* returns, const double* W, double rf_step,
                             mcp_sweep_perf_sums* out, hipStream_t s) {
  const int grid = (P + PERF_LANES - 1) / PERF_LANES;
  const size_t lds = (size_t)N * PERF_LANES * sizeof(double);        // <= 64 * 64 * 8 = 32,768 B
  sweep_perf_kernel<<<grid, PERF_LANES, lds, s>>>(N, R, P, returns, W, rf_step, out);
  return hipGetLastError();
}

}  // namespace mcp

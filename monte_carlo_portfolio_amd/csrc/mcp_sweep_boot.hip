// mcp_sweep_boot.hip -- the resampled historical sweep (SPEC.md 5.25, include/mcport_sweep_boot.h): the rows of the sweep's sample
// redrawn B times by the stationary block bootstrap of SPEC.md 2.1, all P portfolios scored on every resample, in binary64.
//
// A resample enters every figure through its row counts c[r] alone, so no resampled series is ever formed:
//   boot_counts_kernel   one lane per replicate walks t = 0 .. R-1 as the path kernels' bootstrap step does and counts the rows it
//                        visits; counts [R][B] (uint16), column beta owned by one lane -- no atomics.
//   boot_score_kernel    one workgroup per (portfolio, slice of the replicates).  Once per workgroup: the series y[r] into LDS and the
//                        stable ascending order perm[] of its rows by a bitonic network over (value, row) keys.  Then one lane per
//                        replicate: two passes over r for the moments, a walk over the sorted order for the two order statistics that
//                        stops as soon as every lane of the wave has passed rank_hi, a second short walk for the tail sum.  y[r] and
//                        perm[k] are wave-uniform LDS reads (broadcasts); the only per-lane memory traffic is the count, one coalesced
//                        2-byte gather per (replicate, row) and pass, from a matrix that every workgroup shares (L2).
//   boot_argmax_kernel   per criterion (sharpe, var, cvar) one lane per replicate and 16 waves over slices of the portfolios, each in
//                        order; the first maximum wins.
// The order of every sum is the definition (r or k ascending, one binary64 operation at a time; the build neither contracts nor
// reassociates), so the bytes do not depend on how the replicates are cut into workgroups or calls.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcport.h"
#include "mcp_device.h"
#include "mcp_stats_kernels.h"

namespace mcp {

constexpr int BOOT_BLOCK = 256;
constexpr int WALK = 8;              // sorted rows per trip of the score kernel's two walks

// grid = ceil(B / 256), block = 256; counts [R][B] zeroed before the launch
__global__ void __launch_bounds__(BOOT_BLOCK) boot_counts_kernel(int R, int B, uint64_t seed, uint64_t begin, uint64_t thr,
                                                                 uint16_t* __restrict__ counts) {
  const int q = blockIdx.x * BOOT_BLOCK + threadIdx.x;
  if (q >= B) return;
  const PhiloxKeys ks = philox_keys((uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t g = begin + (uint64_t)q;
  const uint32_t glo = (uint32_t)g, ghi = (uint32_t)(g >> 32), n_rows = (uint32_t)R;
  uint32_t j = 0;
  for (int t = 0; t < R; t++) {
    uint32_t x[4];
    philox4x32_10((uint32_t)t, 1u, glo, ghi, ks, x);
    const uint32_t start = __umulhi(x[0], n_rows), next = j + 1u;
    j = (t == 0 || (uint64_t)x[1] < thr) ? start : (next == n_rows ? 0u : next);       // j < R always
    uint16_t* c = counts + (size_t)j * B + q;
    *c = (uint16_t)(*c + 1);
  }
}

// is the row pair (value ya, row a) after (yb, b) in the stable ascending order?  rows >= R are padding, after every real row
__device__ __forceinline__ bool boot_after(const double* __restrict__ y, int R, uint32_t a, uint32_t b) {
  const bool pa = a >= (uint32_t)R, pb = b >= (uint32_t)R;
  if (pa || pb) return pa && (!pb || a > b);
  const double ya = y[a], yb = y[b];
  return ya > yb || (ya == yb && a > b);            // -0.0 == +0.0: the row decides
}

// grid = (P, slices), block = 256, dynamic LDS = (R + N) doubles + R2 uint32, R2 = R rounded up to a power of two (<= 49,664 B).
// Slice s of a portfolio scores the replicates of the 256-wide chunks s, s + slices, ...
__global__ void __launch_bounds__(BOOT_BLOCK) boot_score_kernel(int N, int R, int R2, int P, int B, const double* __restrict__ returns,
                                                                const double* __restrict__ W, const uint16_t* __restrict__ counts,
                                                                double rf, double ann, uint32_t rank_lo, uint32_t rank_hi, double gamma,
                                                                double* __restrict__ scores /* [5][P][B] */) {
  extern __shared__ double lds[];
  double* y = lds;                               // [R], in row order
  double* w = lds + R;                           // [N]
  uint32_t* perm = (uint32_t*)(lds + R + N);     // [R2]: perm[k] = the row of the k-th smallest value
  const int p = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < N; i += BOOT_BLOCK) w[i] = W[(size_t)p * N + i];
  for (int k = tid; k < R2; k += BOOT_BLOCK) perm[k] = (uint32_t)k;
  __syncthreads();
  for (int r = tid; r < R; r += BOOT_BLOCK) {
    double s = 0.0;
    for (int i = 0; i < N; i++) s += returns[(size_t)r * N + i] * w[i];
    y[r] = s;
  }
  __syncthreads();
  // bitonic network over the rows, ascending by (value, row): a total order, so the result is the stable order whatever the network
  for (int k = 2; k <= R2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < R2 / 2; t += BOOT_BLOCK) {
        const int i = 2 * t - (t & (j - 1));           // lower index of the t-th pair at distance j
        const int l = i + j;
        const bool up = (i & k) == 0;
        const uint32_t a = perm[i], b = perm[l];
        if (boot_after(y, R, a, b) == up) { perm[i] = b; perm[l] = a; }
      }
      __syncthreads();
    }
  }

  const double dR = (double)R, dR1 = (double)(R - 1);
  const size_t PB = (size_t)P * B;
  for (int q0 = blockIdx.y * BOOT_BLOCK; q0 < B; q0 += gridDim.y * BOOT_BLOCK) {
    const int q = q0 + tid;
    const bool live = q < B;
    const uint16_t* c = counts + (live ? q : B - 1);       // an absent lane walks the last column and stores nothing

    double S = 0.0;
    for (int r = 0; r < R; r++) S += (double)c[(size_t)r * B] * y[r];
    const double m = S / dR;
    double M2 = 0.0;
    for (int r = 0; r < R; r++) {
      const double d = y[r] - m;
      M2 += (double)c[(size_t)r * B] * (d * d);
    }
    const double pret = m * ann;
    const double psd = sqrt(M2 / dR1 * ann);
    const double sharpe = psd > 0.0 ? (pret - rf) / psd : 0.0;

    // the order statistics rank_lo <= rank_hi of the resample: the first k at which the accumulated count passes the rank.  WALK
    // sorted rows per trip: their counts are gathered together, ahead of the chain of compares, and the wave asks once per trip
    // whether every lane has passed rank_hi.  A row past the end counts 0 and moves nothing.
    uint32_t cum = 0;
    double lo = 0.0, a = 0.0, b = 0.0;
    for (int k0 = 0; k0 < R; k0 += WALK) {
      double v[WALK];
      uint32_t cr[WALK];
#pragma unroll
      for (int u = 0; u < WALK; u++) {
        const bool ok = k0 + u < R;
        const uint32_t row = perm[ok ? k0 + u : 0];
        v[u] = y[row];
        cr[u] = ok ? (uint32_t)c[(size_t)row * B] : 0u;
      }
#pragma unroll
      for (int u = 0; u < WALK; u++) {
        const uint32_t before = cum;
        cum += cr[u];
        if (before == 0u && cum > 0u) lo = v[u];
        if (before <= rank_lo && cum > rank_lo) a = v[u];
        if (before <= rank_hi && cum > rank_hi) b = v[u];
      }
      if (__all(cum > rank_hi)) break;
    }
    const double diff = b - a;
    double var = a + diff * gamma;                    // numpy _lerp
    if (gamma >= 0.5) var = b - diff * (1.0 - gamma);

    // the tail: every sorted value <= var, weighted by its count (lo <= a <= var, so tc >= 1); the values ascend, so the wave stops
    // after the first trip whose last row is above every lane's var
    double ts = 0.0;
    uint32_t tc = 0;
    for (int k0 = 0; k0 < R; k0 += WALK) {
      double v[WALK];
      uint32_t cr[WALK];
      bool in[WALK];
#pragma unroll
      for (int u = 0; u < WALK; u++) {
        const bool ok = k0 + u < R;
        const uint32_t row = perm[ok ? k0 + u : 0];
        v[u] = y[row];
        cr[u] = (uint32_t)c[(size_t)row * B];
        in[u] = ok && v[u] <= var;
      }
#pragma unroll
      for (int u = 0; u < WALK; u++)
        if (in[u]) {
          ts += (double)cr[u] * v[u];
          tc += cr[u];
        }
      if (!__any(in[WALK - 1])) break;
    }
    double cvar = ts / (double)tc;
    if (cvar < lo) cvar = lo;
    if (cvar > var) cvar = var;

    if (live) {
      double* o = scores + (size_t)p * B + q;
      o[0] = pret;
      o[PB] = psd;
      o[2 * PB] = sharpe;
      o[3 * PB] = var;
      o[4 * PB] = cvar;
    }
  }
}

// grid = (ceil(B / 64), 3), block = 64 x ARGMAX_WAVES: lane = replicate, wave = a contiguous slice of the portfolios.  A wave runs over
// its slice in order and keeps the first maximum; wave 0 then takes the slices in order, again by a strict compare, so the winner is
// the first portfolio attaining the maximum whatever the number of waves.
constexpr int ARGMAX_WAVES = 16;
__global__ void __launch_bounds__(64 * ARGMAX_WAVES) boot_argmax_kernel(int P, int B, const double* __restrict__ scores,
                                                                        int32_t* __restrict__ opt) {
  __shared__ double best_s[ARGMAX_WAVES][64];
  __shared__ int32_t at_s[ARGMAX_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.y;
  const int q = blockIdx.x * 64 + lane;
  const int per = (P + ARGMAX_WAVES - 1) / ARGMAX_WAVES;
  const int p0 = wave * per, p1 = min(P, p0 + per);
  const double* s = scores + (size_t)(2 + f) * P * B + (q < B ? q : B - 1);       // an absent lane reads the last column
  double best = 0.0;
  int32_t at = -1;                                                                // an empty slice: no candidate
  if (p0 < p1) {
    best = s[(size_t)p0 * B];
    at = p0;
    for (int p = p0 + 1; p < p1; p++) {
      const double v = s[(size_t)p * B];
      if (v > best) { best = v; at = p; }
    }
  }
  best_s[wave][lane] = best;
  at_s[wave][lane] = at;
  __syncthreads();
  if (wave == 0 && q < B) {                                                       // slice 0 holds portfolio 0: never empty
    for (int w = 1; w < ARGMAX_WAVES; w++) {
      const double v = best_s[w][lane];
      const int32_t a = at_s[w][lane];
      if (a >= 0 && v > best) { best = v; at = a; }
    }
    opt[(size_t)f * B + q] = at;
  }
}

// grid = (ceil(R / 32), ceil(B / 32)), block = (32, 8): counts [R][B] -> out [B][R] through a padded LDS tile
__global__ void __launch_bounds__(256) boot_transpose_kernel(int R, int B, const uint16_t* __restrict__ counts, uint16_t* __restrict__ out) {
  __shared__ uint16_t tile[32][33];
  const int r0 = blockIdx.x * 32, q0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = r0 + i, q = q0 + threadIdx.x;
    if (r < R && q < B) tile[i][threadIdx.x] = counts[(size_t)r * B + q];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int q = q0 + i, r = r0 + threadIdx.x;
    if (r < R && q < B) out[(size_t)q * R + r] = tile[threadIdx.x][i];
  }
}

hipError_t launch_boot_counts(int R, int B, uint64_t seed, uint64_t begin, uint64_t thr, uint16_t* counts /* [R][B] */,
                              uint16_t* counts_t /* NULL or [B][R] */, hipStream_t s) {
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)R * B * sizeof(uint16_t), s);
  if (e != hipSuccess) return e;
  boot_counts_kernel<<<(B + BOOT_BLOCK - 1) / BOOT_BLOCK, BOOT_BLOCK, 0, s>>>(R, B, seed, begin, thr, counts);
  if ((e = hipGetLastError()) != hipSuccess || !counts_t) return e;
  boot_transpose_kernel<<<dim3((R + 31) / 32, (B + 31) / 32), dim3(32, 8), 0, s>>>(R, B, counts, counts_t);
  return hipGetLastError();
}

hipError_t launch_boot_score(int N, int R, int P, int B, const double* returns, const double* W, const uint16_t* counts, double rf,
                             double ann, uint64_t rank_lo, uint64_t rank_hi, double gamma, double* scores, int32_t* opt, hipStream_t s) {
  int R2 = 2;
  while (R2 < R) R2 <<= 1;
  const size_t lds = (size_t)(R + N) * sizeof(double) + (size_t)R2 * sizeof(uint32_t);    // <= (4096 + 64) * 8 + 4096 * 4 = 49,664 B
  // a few portfolios: cut the replicates of each over several workgroups (each sorts again) until about 1,024 are in flight
  const int chunks = (B + BOOT_BLOCK - 1) / BOOT_BLOCK;
  int slices = (1024 + P - 1) / P;
  slices = slices < 1 ? 1 : (slices > chunks ? chunks : slices);
  boot_score_kernel<<<dim3(P, slices), BOOT_BLOCK, lds, s>>>(N, R, R2, P, B, returns, W, counts, rf, ann, (uint32_t)rank_lo,
                                                            (uint32_t)rank_hi, gamma, scores);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  boot_argmax_kernel<<<dim3((B + 63) / 64, 3), 64 * ARGMAX_WAVES, 0, s>>>(P, B, scores, opt);
  return hipGetLastError();
}

}  // namespace mcp

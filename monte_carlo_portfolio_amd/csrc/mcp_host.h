// mcp_host.h -- the host code of libmcport.so that touches no device (mcp_host.cpp): every argument rule, every feature's host
// constants, every closed-form pivot, the packers, the layout of a tile's parameter block, the plan of a call and the choice of the
// path kernel.  Internal, not installed.  It includes no device header, so that mcp_host.cpp also builds with a plain C++ compiler
// (make host-selftest).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/mcport.h"
#include "../../include/mcport_protect.h"
#include "../../include/mcport_spend.h"
#include "../../include/mcport_life.h"
#include "../../include/mcport_band.h"
#include "../../include/mcport_voltarget.h"
#include "../../include/mcport_underwater.h"
#include "../../include/mcport_uncertain.h"
#include "../../include/mcport_downside.h"
#include "../../include/mcport_relative.h"
#include "../../include/mcport_sweep_perf.h"
#include "../../include/mcport_sweep_boot.h"
#include "mcp_route.h"

namespace mcp {
constexpr int SWEEP_MIN_K = 17;      // from this many portfolios on the MFMA sweep kernels run

// The raw record of a row-sum pass (SPEC.md 5.22, 5.23), declared once for the kernels and the host: WORDS 8-byte words, the COUNTS
// leading ones unsigned integers, the rest binary64 sums.
template <class T> struct RowSumLayout;
template <> struct RowSumLayout<mcp_downside_sums> { static constexpr int WORDS = 12, COUNTS = 3; };
template <> struct RowSumLayout<mcp_relative_sums> { static constexpr int WORDS = 18, COUNTS = 5; };
static_assert(sizeof(mcp_downside_sums) == 12 * 8, "mcp_downside_sums is twelve 8-byte words");
static_assert(sizeof(mcp_relative_sums) == 18 * 8, "mcp_relative_sums is eighteen 8-byte words");
}

namespace mcph {

using mcp::SWEEP_MIN_K;
constexpr int KT_WIDE = 8;           // portfolios per pass of the KT=8 kernel
constexpr int K_PAD = 512;           // W rows are zero-padded to a multiple of this (MFMA sweep tile: 32*MT)

// Records the thread's last error (mcp_last_error) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

inline int n4_of(int n) { return 4 * ((n + 3) / 4); }
// floats of the regime-1 block [mu1 N4][L1 row pairs N4(N4/2+1)] (SPEC.md 4.13)
inline size_t regime_block_len(int n) { const size_t n4 = (size_t)n4_of(n); return n4 + n4 * (n4 / 2 + 1); }
// W rows are zero-padded to whole MFMA workgroups for a sweep, to whole KT_WIDE passes otherwise
inline int kpad_of(int k) { return k >= SWEEP_MIN_K ? K_PAD * ((k + K_PAD - 1) / K_PAD) : KT_WIDE * ((k + KT_WIDE - 1) / KT_WIDE); }

// A row-sum request riding a call (SPEC.md 5.22, 5.23): where the call's raw records of T gather, and the pivots they are about
template <class T>
struct RowSumRequest {
  bool on = false;                      // the context was armed; set by the call that takes the request
  bool hz = false;                      // the request also covers the horizon rows
  T* sums = nullptr;                    // [K] the call's raw records: every tile adds its shards' in shard order
  T* hz_sums = nullptr;                 // [H*K], row h*K + k
  double* pivot = nullptr;              // [K] the pivots the records are about, as the tiles computed them
  double* hz_pivot = nullptr;           // [H*K]
};

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
  bool spend = false;                   // SPEC.md 4.16: the spending rule `sp`, always with `cash` on an all-zero `cf` that carries the
  const mcp_spending* sp = nullptr;     // rule's target (mcp_simulate_spending)
  bool life = false;                    // SPEC.md 4.17: the lifetime l of every path, always with `cash` (mcp_simulate_lifetime)
  bool band = false;                    // SPEC.md 4.18: the tolerance bands `bd`, always with `rebalanced` on a rule `reb` of the same
  const mcp_band* bd = nullptr;         // period and cost (mcp_simulate_banded)
  bool vol_target = false;              // SPEC.md 4.19: the targeting rule `vt` (mcp_simulate_vol_target)
  const mcp_vol_target* vt = nullptr;
  bool overlay = false;                 // SPEC.md 4.8: the option rows `ov`
  const mcp_overlay* ov = nullptr;
  bool garch = false;                   // SPEC.md 4.9: the variance recurrence `gv` (SRC_GAUSS or SRC_T)
  const mcp_garch* gv = nullptr;
  bool jumps = false;                   // SPEC.md 2.5 / 4.12: the market jump `jp` on top of SRC_GAUSS
  const mcp_jumps* jp = nullptr;
  bool regimes = false;                 // SPEC.md 2.6 / 4.13: two regimes `rs`, regime 0 on (mu, chol), on top of SRC_GAUSS
  const mcp_regimes* rs = nullptr;
  bool dd = false;                      // SPEC.md 4.2 / 5.1: the drawdown of every path
  bool underwater = false;              // SPEC.md 4.20 / 5.20: the longest and the current spell under water, always with `dd`
                                        // (mcp_simulate_underwater)
  bool uncertain = false;               // SPEC.md 2.7 / 4.21: the drift of every path drawn once, m = mu + M g, on top of SRC_GAUSS
  const mcp_drift_uncertainty* du = nullptr;   // (mcp_simulate_uncertain)
  bool hz = false;                     // SPEC.md 4.3 / 5.2: the values after H steps, statistics at alpha and at L levels
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
  uint64_t* counts_out = nullptr;       // cash flows, volatility target: [K][2] {n_ruined, n_short} (SPEC.md 5.6 / 5.19); protection: {n_gap, n_short} (5.15)
  uint64_t* hz_counts_out = nullptr;    // [H*K][2]
  float* wd_out = nullptr;              // spending rule: NULL or host [K*n] Y_T (SPEC.md 4.16)
  mcp_stats* wd_stats_out = nullptr;    // [K]
  float* exposure_out = nullptr;        // volatility target without the drawdown: NULL or host [K*n] Y_T (SPEC.md 4.19)
  mcp_stats* exposure_stats_out = nullptr;   // [K]
  uint32_t* life_out = nullptr;         // lifetime: NULL or host [K*n] l (SPEC.md 4.17)
  uint64_t* life_hist_out = nullptr;    // [K][n_steps + 1] (SPEC.md 5.17)
  uint32_t* trades_out = nullptr;       // bands: NULL or host [K*n] c (SPEC.md 4.18)
  uint64_t* trade_hist_out = nullptr;   // [K][n_reviews + 1] (SPEC.md 5.18)
  uint32_t* uw_longest_out = nullptr;   // time under water: NULL or host [K*n] m (SPEC.md 4.20)
  uint32_t* uw_current_out = nullptr;   // NULL or host [K*n] c_T
  uint64_t* uw_longest_hist_out = nullptr;   // [K][n_steps + 1] (SPEC.md 5.20)
  uint64_t* uw_current_hist_out = nullptr;   // [K][n_steps + 1]
  float* turnover_out = nullptr;        // NULL or host [K*n] Y
  mcp_stats* turnover_stats_out = nullptr;   // [K]
  bool attr = false;                    // SPEC.md 4.10 / 5.9: the second walk that attributes the risk to the assets
  float* contrib_out = nullptr;         // NULL or host [K][N][n]
  mcp_attr* attr_out = nullptr;         // [K][N]
  uint64_t* attr_counts_out = nullptr;  // [K][2] {n, n_tail}
  bool anti = false;                    // SPEC.md 2.3 / 5.10: antithetic pairs
  mcp_pair* pair_out = nullptr;         // [K]
  double* cross_out = nullptr;          // [K] the call's cross sums: every tile adds its shards' in shard order
  RowSumRequest<mcp_downside_sums> ds;  // SPEC.md 5.22: mcp_ctx_request_downside
  double ds_tau = 0.0;                  // the threshold, prm->rf when the request says so
  RowSumRequest<mcp_relative_sums> rl;  // SPEC.md 5.23: mcp_ctx_request_relative
  int rl_bench = 0;                     // the benchmark's row of W
  float* rl_active_out = nullptr;       // NULL or host [K*n] Y = fl32(1 + a)
  mcp_stats* rl_active_stats_out = nullptr;  // NULL or [K] the records of Y
};

// The row table of a request that walks rows: the bootstrap's own, or the residual rows of SRC_FHS.
mcp_bootstrap rows_of(const Request& rq);
Request host_request(Source src, const float* mu, const float* chol, const float* W, float* terminal_out, mcp_stats* stats_out);
void ask_horizons(Request& rq, bool on, int H, const int32_t* steps, int L, const double* levels, float* out, mcp_stats* stats,
                  double* bands);
// The drawdown is asked for by its statistics: dd_stats_out != NULL
void ask_drawdown(Request& rq, float* mdd_out, mcp_stats* dd_stats_out);

// One launch of the path kernels for a request: the device arrays of an mcp_launch_paths* call or of one shard's part of a tile.
struct Launch {
  const float* d_packed = nullptr;
  const double* d_pivot = nullptr;
  uint64_t seed = 0, path_begin = 0, n_paths = 0;
  float* d_terminal = nullptr;
  uint64_t stride = 0;
  float* d_mdd = nullptr;               // drawdown: [K][mdd_stride]
  uint64_t mdd_stride = 0;
  float* d_wd = nullptr;                // spending rule: [K][wd_stride] Y_T; volatility target: the summed exposure Y_T
  uint64_t wd_stride = 0;
  uint32_t* d_life = nullptr;           // lifetime: [K][life_stride] l; time under water: the longest spell m
  uint64_t life_stride = 0;
  uint32_t* d_life2 = nullptr;          // time under water: [K][life_stride] the current spell c_T
  float* d_hz = nullptr;                // horizons: [H][K][hz_stride]
  uint64_t hz_stride = 0;
  const float* d_rows = nullptr;        // bootstrap: [R][N4], zero-padded
  const float* d_flows = nullptr;       // cash flows: [n_steps]
  const float* d_floor = nullptr;       // protection: [n_steps + 1] the floor schedule
  const float* d_s0 = nullptr;          // volatility target: [8 ceil(K/8)] the initial variance estimates
  const float* d_band = nullptr;        // bands: [K][N4] tolerances, then [K][2] mask words (band_pack); c goes to d_life, Y to d_wd
  const float* d_targets = nullptr;     // glide path: [n_breaks][glide_rows(K)][N4] target blocks (glide_pack)
  const char* d_overlay = nullptr;      // overlay: [rows][row_begin N4 + 1][spot N4] (overlay_pack)
  const float* d_loading = nullptr;     // jumps: [N4] loadings, zero-padded
  const float* d_block1 = nullptr;      // regimes: [mu1 N4][L1 row pairs], the layout of mcp_pack_params
  const float* d_drift = nullptr;       // drift uncertainty: [N4 (N4/2 + 1)] M in the factor's row-pair layout (drift_pack)
  bool attr = false;                   // the attribution walk (SPEC.md 4.10): FAM_AT instead of the request's own family
  const double* d_var = nullptr;        // attribution: [K] VaRs
  double* d_cross = nullptr;            // antithetic pairs: [K][path_grid(n_paths / 2)] cross partials
  double* d_attr_partials = nullptr;    // attribution: [K][path_grid(n_paths)][attr_record_len(N4)]
  float* d_contrib = nullptr;           // attribution: NULL or [K][N][contrib_stride]
  uint64_t contrib_stride = 0;
  void* d_partials = nullptr;
  void* d_hist = nullptr;
  void* stream = nullptr;               // the device side casts it to its stream type
};

// ---- each feature's argument rules (SPEC.md sections as in mcp_host.cpp) ----
int check_params(const mcp_params* p);
int check_horizons(int n_steps, int H, const int32_t* steps);
int check_levels(int L, const double* levels);
int check_boot(const mcp_params* prm, const mcp_bootstrap* boot);
int check_reb(const mcp_rebalance* reb);
int check_student_t(const mcp_params* prm, const mcp_student_t* st);
int check_garch(const mcp_params* prm, const mcp_garch* g);
int check_jumps(int n_assets, const mcp_jumps* j);
int check_regimes(int n_assets, const mcp_regimes* r);
int check_filtered(const mcp_params* prm, const mcp_filtered* f);
int check_cashflow(const mcp_params* prm, const mcp_cashflow* cf);
int check_glide(const mcp_params* prm, const mcp_glide* gl);
int check_protect(const mcp_params* prm, const mcp_protect* pt);
int check_spending(double v0, const mcp_spending* sp);
int check_overlay(const mcp_params* prm, const mcp_overlay* ov);
int check_band(const mcp_params* prm, const mcp_band* bd);
// `chol`, `W`: what the default s0_k is formed from (read only when vt->s0 is NULL)
int check_vol_target(const mcp_params* prm, const mcp_vol_target* vt, const float* chol, const float* W);
int check_drift_uncertainty(int n_assets, const mcp_drift_uncertainty* du);
int check_downside(const mcp_downside* req, const mcp_downside_stats* stats_out);
int check_relative(const mcp_relative* req, const mcp_relative_stats* stats_out);
// SPEC.md 5.24: every rule of mcp_sweep_historical_perf but the context's, the finiteness scan of mcp_sweep_historical included
int check_sweep_perf(int N, int R, int P, const double* returns, const double* W, double risk_free, double ann_factor,
                     const mcp_sweep_perf_stats* stats_out);
// SPEC.md 5.25: every rule of mcp_sweep_resampled but the context's (the scan above included), and those of mcp_sweep_boot_counts
int check_sweep_boot(int N, int R, int P, const double* returns, const double* W, double rf, double ann_factor, double alpha,
                     uint64_t replicate_begin, int B, double block, const double* scores_out, const int32_t* opt_out);
int check_boot_replicates(uint64_t replicate_begin, int B, int R, double block);
// Every rule a request meets: each feature's own arguments, then which features combine (MCP_E_UNSUPPORTED), then the outputs.
// `ln`: an mcp_launch_paths* call, whose device arrays are checked instead of the host arrays of an mcp_simulate* call.
int check_request(const mcp_params* prm, const Request& rq, uint64_t n_paths, const Launch* ln = nullptr, uint64_t path_begin = 0);
// The path kernel of one launch of a checked request on the paths [path_begin, path_begin + n_paths): its selector, with no flag
// set that the kernel does not consume, so that it equals one row of mcp_paths_ladder.inc (host_selftest.cpp proves both for every
// request check_request accepts).  `attr_walk`: the second walk of an attribution call (Launch::attr) instead of the request's own.
mcp::PathKernel route_kernel(const mcp_params* prm, const Request& rq, bool attr_walk, uint64_t path_begin, uint64_t n_paths);

// ---- each feature's host constants ----
uint64_t boot_threshold(double b);
void boot_moments(int N, const mcp_bootstrap* boot, const float* W, int K, double* m_out, double* s2_out);
double boot_pivot(int compounding, int T, double m, double s2);
struct GarchConsts { float a, b, g, omega, a_n; };
GarchConsts garch_consts(const mcp_garch* g, int N);
struct JumpConsts { uint32_t thr[MCP_MAX_JUMPS]; double mean_count; float m, s; };
JumpConsts jump_consts(const mcp_jumps* j);
void jump_drift(const mcp_jumps* j, const JumpConsts& c, int N, const float* mu, float* out);
struct RegimeConsts { uint64_t thr01, thr10, thr_start; double p01, p10, start; };
RegimeConsts regime_consts(const mcp_regimes* r);
struct ProtectConsts { float m, b, rf, theta; };
ProtectConsts protect_consts(const mcp_protect* pt);
struct SpendConsts { float p, g, lo, hi, w0; };
struct VolTargetConsts { float tgt, lam, oml, b, rf, sp; };
VolTargetConsts vol_target_consts(const mcp_vol_target* vt);
// SPEC.md 4.19: s0_k of portfolio k of W -- the caller's, or fl32(sum_j (sum_i W[k,i] L[i,j])^2)
float vol_target_s0(int N, const mcp_vol_target* vt, const float* chol, const float* W, int k);
SpendConsts spend_consts(const mcp_spending* sp, double v0);

// ---- the closed-form pivots and their means ----
void regime_pivots(int N, int K, int T, const float* mu0, const float* mu1, const RegimeConsts& c, const float* W, int H, const int32_t* steps,
                   double* out_T, double* out_hz);
void filt_means(int N, const mcp_filtered* f, double* out);
void filt_pivots(int N, int K, int T, const double* me, const float* W, double* out);
void overlay_pivots(int N, int K, int T, const mcp_overlay* ov, const float* mu, const float* W, int H, const int32_t* steps,
                    double* out_T, double* out_hz);
void reb_means(int N, const float* mu, const mcp_bootstrap* boot, double* out);
void reb_pivots(int N, int K, int T, int m, const double* mu, const float* W, double* out);
void cash_means(int N, int K, const float* mu, const mcp_bootstrap* boot, const float* W, double* out);
void cash_pivots(int K, int T, const double* m, const float* flows, double v0, int H, const int32_t* steps, double* out_T, double* out_hz);
void glide_means(int N, int K, int k0, int kt, const float* mu, const mcp_bootstrap* boot, const float* W, const mcp_glide* gl, double* out);
void glide_pivots(int K, int T, int G, const int32_t* breaks, const double* m, const float* flows, double v0, int H, const int32_t* steps,
                  double* out_T, double* out_hz);
void protect_pivots(const mcp_params& prm, const mcp_protect* pt, const float* mu, const float* W, int K, int H, const int32_t* steps,
                    double* out_T, double* out_hz);
void vol_target_pivots(const mcp_params& prm, const mcp_vol_target* vt, const float* mu, const float* chol, const float* W, int k0, int K,
                       int H, const int32_t* steps, double* out_T, double* out_hz);
void spend_pivots(int K, int T, const double* m, const SpendConsts& c, int every, double v0, int H, const int32_t* steps, double* out_T,
                  double* out_hz, double* out_wd);

// SPEC.md 5.17: life_sum and the order statistics at the levels' ranks `lo` (mcp_percentile_rank_q) of one histogram hist[0 .. T]
int life_summary(const uint64_t* hist, int T, int n_levels, const double* levels, uint64_t* sum_out, uint32_t* q_out);

// SPEC.md 4.18: the reviews of a walk of T steps reviewed every e steps, floor((T - 1) / e) for 1 <= e < T, else 0
int band_reviews(int T, int e);
// The bins of the exact histogram of a request's integer records: the lifetime's and the time under water's n_steps + 1 (SPEC.md 5.17 /
// 5.20), the bands' n_reviews + 1 (5.18)
size_t count_bins(const mcp_params* prm, const Request& rq);

// ---- the packers of what a launch reads besides the packed block of mcp_pack_params ----
size_t glide_rows(int kt);
size_t glide_len(int N, int kt, const mcp_glide* gl);
void glide_pack(int N, int K, int k0, int kt, const mcp_glide* gl, float* out);
size_t band_len(int N, int kt);
void band_pack(int N, int k0, int kt, const mcp_band* bd, float* out);
size_t protect_len(int T, int kt, int H);
void protect_pack(int T, int kt, int H, const int32_t* steps, const mcp_protect* pt, float* out);
// SPEC.md 4.21: M's lower triangle in the row-pair layout of the Cholesky factor (mcp_pack_params), every entry through + 0.0f
size_t drift_len(int N);
void drift_pack(int N, const mcp_drift_uncertainty* du, float* out);
size_t overlay_bytes(int N, int n_rows);
void overlay_pack(int N, const mcp_overlay* ov, char* out);

// ---- one tile of a checked request: the portfolios [k0, k0 + kt) of the call's W ----
// Float offsets into the parameter block of a tile.  This is the only place that knows what follows the packed block.
struct TileLayout {
  size_t base;     // mcp_packed_len(N, kt): the end of the packed block
  size_t load;     // where the jump loadings, the regime-1 block, the glide targets, the tolerance table or the drift factor M begin
  size_t floor;    // where the protection schedule and the counts' thresholds begin (protect_pack), or the volatility target's s0
  size_t total;    // floats of the whole block
};
TileLayout tile_layout(const mcp_params* prm, const Request& rq, int kt);

// What pack_tile and request_pivots need of the request that no tile changes; filled once per call by tile_inputs.
struct TileInputs {
  std::vector<float> zmu, zchol;   // bootstrap: no drift and no Cholesky factor in the packed block; filtered rows: no factor
  std::vector<float> jmu;          // jumps: the compensated drift (SPEC.md 2.5)
  std::vector<float> blk1;         // regimes: (mu1, chol1) packed as (mu, chol) are (SPEC.md 2.6)
  std::vector<double> rmu;         // rebalancing: the draws' per-asset means (SPEC.md 5.4); filtered rows: mu_i + e_i (5.11)
};
int tile_inputs(const mcp_params* prm, const Request& rq, TileInputs* in);
// The host block of one tile, out[tile_layout(prm, rq, kt).total]
int pack_tile(const mcp_params* prm, const Request& rq, const TileInputs& in, int k0, int kt, float* out);
// The tile's pivots at n_steps into out_T[kt] and at the request's horizons into out_hz[H*kt] (row h*kt + k; NULL without horizons)
int request_pivots(const mcp_params* prm, const Request& rq, const TileInputs& in, int k0, int kt, double* out_T, double* out_hz);
// SPEC.md 5.16: the tile's pivots of the total paid out into out_wd[kt] (a spending request only)
void request_wd_pivots(const mcp_params* prm, const Request& rq, int k0, int kt, double* out_wd);

// ---- what a request leaves per path besides V_T and the horizon rows ----
// The one second float array: the drawdown q / d (SPEC.md 5.1), the turnover Y of the bands (5.18), the total paid out Y_T of a
// spending rule (5.16) or, in a call without the drawdown, the summed exposure Y_T of a volatility target (5.19); check_request lets
// at most one of them through.  It is reduced as the terminal values are, at rf = 0.
struct Second {
  bool on;                // the request has one
  bool unit_v0;           // its select runs at v0 = 1: x = q - 1, expm1(d) or Y - 1 (turnover, summed exposure); the total paid out keeps v0: x = Y / fl32(v0) - 1
  bool pivoted;           // its select takes the pivots of request_wd_pivots (spending only); the other two take none
  float* out;             // the caller's [K*n] array, or NULL
  mcp_stats* stats_out;   // the caller's [K] records
};
Second second_of(const Request& rq);
// The integer records: the lifetime l (SPEC.md 4.17 / 5.17), the bands' trade count c (4.18 / 5.18), or the two counters of the time
// under water, m then c_T (4.20 / 5.20), each with its exact histogram.  A shard holds record r of a tile of kt portfolios as the rows
// [r kt, (r + 1) kt) of one array, and its histograms likewise.
struct Counted {
  bool on;
  size_t bins;            // count_bins
  uint32_t* out;          // the caller's [K*n] array, or NULL
  uint64_t* hist_out;     // the caller's [K][bins] histogram
  int records;            // 1, or 2 for the time under water (0 when off)
  uint32_t* out2;         // the second record's, as `out` and `hist_out`
  uint64_t* hist_out2;
};
Counted counted_of(const mcp_params* prm, const Request& rq);

// ---- downside and shape statistics (SPEC.md 5.22) ----
// What mcp_ctx_request_downside leaves on a context.  The next call that walks paths takes it, and taking disarms: whatever becomes of
// that call, the one after it finds nothing and writes nothing.
struct DownsideArm {
  bool on = false;
  double tau = 0.0;
  bool use_rf = false;
  mcp_downside_sums* sums_out = nullptr;
  mcp_downside_stats* stats_out = nullptr;
  mcp_downside_stats* hz_stats_out = nullptr;
  void arm(const mcp_downside& req, mcp_downside_sums* sums, mcp_downside_stats* stats, mcp_downside_stats* hz_stats);
  DownsideArm take();
};
// a += b, word by word over the record's layout, the counts as integers and the sums as doubles: how the records of shards add up,
// in shard order
template <class T>
inline void rowsum_add(T& a, const T& b) {
  using L = mcp::RowSumLayout<T>;
  uint64_t n[L::COUNTS], m[L::COUNTS];
  double x[L::WORDS - L::COUNTS], y[L::WORDS - L::COUNTS];
  memcpy(n, &a, sizeof n); memcpy(m, &b, sizeof m);
  memcpy(x, (const char*)&a + sizeof n, sizeof x); memcpy(y, (const char*)&b + sizeof m, sizeof y);
  for (int i = 0; i < L::COUNTS; i++) n[i] += m[i];
  for (int i = 0; i < L::WORDS - L::COUNTS; i++) x[i] += y[i];
  memcpy(&a, n, sizeof n); memcpy((char*)&a + sizeof n, x, sizeof x);
}

// ---- benchmark-relative statistics (SPEC.md 5.23) ----
// What mcp_ctx_request_relative leaves on a context: the next call that walks paths takes it, and taking disarms.  Both requests may
// be armed at once; the same call serves both.
struct RelativeArm {
  bool on = false;
  int bench = 0;
  mcp_relative_sums* sums_out = nullptr;
  mcp_relative_stats* stats_out = nullptr;
  mcp_stats* active_stats_out = nullptr;
  float* active_out = nullptr;
  mcp_relative_stats* hz_stats_out = nullptr;
  void arm(const mcp_relative& req, mcp_relative_sums* sums, mcp_relative_stats* stats, mcp_stats* active_stats, float* active,
           mcp_relative_stats* hz_stats);
  RelativeArm take();
};

// ---- the plan of a call: which shard does what in which tile ----
// Bytes per path and portfolio that the tile budget counts: 4 of V_T, 4 per horizon row, 4 of the second array, 4 per integer record,
// 4 of the active returns Y of a relative request
size_t tile_bytes_per_path(const Request& rq);
// Portfolios per tile so that kt * n_paths * bytes_per_path fits the budget: whole 512-portfolio workgroups of the MFMA sweep kernel
// when K is tiled at all.
int tile_portfolios(size_t budget, uint64_t n_paths, int K, size_t bytes_per_path);
// What one shard does in one tile of portfolios.
struct Job {
  int k0 = 0, kt = 0;            // portfolios [k0, k0+kt) of the caller's W
  uint64_t p0 = 0, pn = 0;       // paths [p0, p0+pn) relative to path_begin
  bool active = false;
};
struct TilePlan {
  size_t S = 0;                  // shards
  std::vector<Job> jobs;         // [tiles][S], in the order the tiles run
  size_t tiles() const { return jobs.size() / S; }
  const Job* tile(size_t t) const { return jobs.data() + t * S; }
  bool walks(size_t s) const;    // does shard s walk paths in this call?
};
// The tiles of a call of K portfolios and n_paths paths on S shards under `budget` bytes per device.  Portfolio shards: shard s takes
// the slice [K*s/S, K*(s+1)/S) of W and walks all paths; the slices are tiled independently, round after round until every shard is
// done, a finished shard inactive.  Path shards: all shards see the same tile of portfolios and shard s walks its part of the path
// range, cut at multiples of `unit` (2 for antithetic pairs, SPEC.md 2.3); with fewer units than shards the last ones are active on
// no paths.
TilePlan plan_tiles(size_t S, int K, uint64_t n_paths, bool by_portfolio, uint64_t unit, size_t budget, size_t bytes_per_path);
// SPEC.md 5.23: a relative request needs row `bench` beside every row, so the plan must hold all K portfolios in one tile on every
// shard -- MCP_E_ARG for portfolio shards on several shards and for a budget that cuts K
int check_relative_plan(const TilePlan& plan, int K, bool by_portfolio);

}  // namespace mcph

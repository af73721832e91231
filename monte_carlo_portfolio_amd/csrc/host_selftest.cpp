// host_selftest.cpp -- drives mcp_host.cpp on heap buffers of exactly the documented lengths, for `make host-selftest`: built
// with a plain C++ compiler under AddressSanitizer + UBSan, so an overrun of a packer or a pivot rule is a sanitizer report.  It
// asserts return codes and finiteness only; the values are pinned bit for bit by the CPU tests against their NumPy restatements.
// The plan of a call (second_of, counted_of, tile_bytes_per_path, plan_tiles) has no other CPU test: it is asserted in full here.
// So is the routing: every combination of features goes through check_request, route_kernel and the rows of mcp_paths_ladder.inc,
// the text the device build compiles (run_routes).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "mcp_host.h"

using namespace mcph;

#define EXPECT(cond)                                                                                           \
  do {                                                                                                         \
    if (!(cond)) {                                                                                             \
      fprintf(stderr, "host_selftest:%d: %s  [%s; last error: %s]\n", __LINE__, #cond, g_case, mcp_last_error()); \
      exit(1);                                                                                                 \
    }                                                                                                          \
  } while (0)

static char g_case[96] = "";
template <class T> static bool finite(const std::vector<T>& v) {
  for (const T& x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

// Minimal valid arguments of every feature for N assets, K portfolios, T steps and row tables of R rows, with the outputs a request
// must carry, and the request of one combination of features over them.
enum Bit { B_DD = 1, B_HZ = 2, B_REB = 4, B_BAND = 8, B_CASH = 16, B_GLIDE = 32, B_SPEND = 64, B_LIFE = 128, B_PROTECT = 256, B_OVERLAY = 512,
           B_GARCH = 1024, B_JUMPS = 2048, B_REGIMES = 4096, B_ANTI = 8192, B_ATTR = 16384, B_VT = 32768, B_UW = 65536, N_BITS = 17 };
enum { B_PU = 1 << N_BITS, N_BITS_PU = N_BITS + 1 };     // SPEC.md 4.21: the per-path drift, the bit behind them (131072; 18 bits in all)
struct Payloads {
  static constexpr int G = 2, H = 2;
  const int N, K, T, R;
  const int32_t steps[H], breaks[G] = {3, 7};
  std::vector<float> mu, mu1, chol, chol1, W, rows, shock, loading, targets, flows, zero_flows, floor_s, spot, tol, drift_m;
  std::vector<int32_t> row_begin;
  const std::vector<mcp_overlay_row> ov_rows;
  mcp_bootstrap boot;
  mcp_filtered filt;
  const mcp_student_t st = {5, 0};
  const mcp_garch gv = {0.05, 0.9, 1.0, 0};
  mcp_jumps jp;
  mcp_regimes rs;
  mcp_glide gl;
  mcp_cashflow cf, no_cf;
  mcp_protect pt;
  const mcp_vol_target vt = {0.01, 0.94, 1.5, 0.001, 0.0005, nullptr, nullptr, 0};
  mcp_overlay ov;
  const mcp_rebalance reb = {5, 0, 0.001};
  mcp_band bd;
  mcp_rebalance bd_reb;
  const mcp_spending sp = {0.01, 0.1, HUGE_VAL, 0.02, 0.015, 0.9, 5, 1, 1, 0};
  mcp_drift_uncertainty du;
  std::vector<mcp_stats> stats, hz_stats, second_stats;
  std::vector<uint64_t> counts, hz_counts, trade_hist, life_hist, uw_longest_hist, uw_current_hist, attr_counts;
  std::vector<mcp_attr> attr;
  std::vector<mcp_pair> pair;

  Payloads(int N_, int K_, int T_, int R_)
      : N(N_), K(K_), T(T_), R(R_), steps{1, T_}, mu(N), mu1(N), chol((size_t)N * N, 0.0f), chol1((size_t)N * N, 0.0f), W((size_t)K * N),
        rows((size_t)R * N), shock(R), loading(N), targets((size_t)G * K * N), flows(T, -0.01f), zero_flows(T, 0.0f), floor_s(T + 1),
        spot(N, 100.0f), tol((size_t)K * N, 0.05f), drift_m((size_t)N * N, 0.0f), row_begin(N + 1, 1), ov_rows(1, mcp_overlay_row{MCP_OVERLAY_PUT, 95.0f, 1.0f, 0.01f}),
        stats(K), hz_stats((size_t)H * K), second_stats(K), counts(2 * (size_t)K), hz_counts(2 * (size_t)H * K),
        trade_hist((size_t)K * ((size_t)(T - 1) / 5 + 1)), life_hist((size_t)K * ((size_t)T + 1)), uw_longest_hist((size_t)K * ((size_t)T + 1)),
        uw_current_hist((size_t)K * ((size_t)T + 1)), attr_counts(2 * (size_t)K),
        attr((size_t)K * N), pair(K) {
    for (int i = 0; i < N; i++) {
      mu[i] = 0.001f * (float)(i + 1) / (float)N;
      mu1[i] = -2.0f * mu[i];
      loading[i] = 0.5f + 0.5f * (float)(i & 1);
      for (int j = 0; j <= i; j++) chol[(size_t)i * N + j] = i == j ? 0.01f : 0.001f;
      for (int j = 0; j <= i; j++) chol1[(size_t)i * N + j] = 3.0f * chol[(size_t)i * N + j];
      for (int j = 0; j <= i; j++) drift_m[(size_t)i * N + j] = i == j ? 0.002f : -0.0005f;
    }
    for (size_t i = 0; i < W.size(); i++) W[i] = (1.0f + 0.1f * (float)(i % 3)) / (float)N;
    for (size_t i = 0; i < targets.size(); i++) targets[i] = (1.0f + 0.1f * (float)(i % 5)) / (float)N;
    for (size_t i = 0; i < rows.size(); i++) rows[i] = 0.002f * (float)((int)(i % 7) - 3);
    for (int j = 0; j < R; j++) shock[j] = 0.5f + 0.25f * (float)(j % 6);
    EXPECT(mcp_protect_floor(0.8, 0.001, T, floor_s.data()) == MCP_OK && finite(floor_s));
    row_begin[0] = 0;
    for (int k = 0; k < K; k++) tol[(size_t)k * N + N - 1] = HUGE_VALF;     // SPEC.md 4.18: the last asset of every portfolio not watched
    boot = {rows.data(), R, 0, 3.0};
    filt = {mu.data(), rows.data(), shock.data(), R, 0, 2.0};
    jp = {0.1, -0.05, 0.02, (N & 1) ? loading.data() : nullptr, 0};
    rs = {0.05, 0.2, 0.1, mu1.data(), chol1.data(), 0};
    gl = {breaks, targets.data(), G, 0};
    cf = {flows.data(), T, 1, 1.0};
    no_cf = {zero_flows.data(), T, 0, 0.0};
    pt = {floor_s.data(), 3.0, 1.0, 0.001, 0.1, nullptr, 0};
    ov = {ov_rows.data(), row_begin.data(), spot.data(), 1, 0};
    bd = {5, 0, 0.001, tol.data()};
    bd_reb = {bd.every, 0, bd.cost};
    du = {drift_m.data(), 0};
  }
  Payloads(const Payloads&) = delete;

  // The request of an mcp_simulate* call with the draw source `src` and the features `bits`, every output it must carry on this
  // object's buffers and none of the optional ones.  A spending rule comes on the all-zero schedule, as mcp_simulate_spending asks it.
  Request request(Source src, int bits) {
    const bool rows_only = src == SRC_BOOT || src == SRC_FHS;
    Request rq = host_request(src, rows_only ? nullptr : mu.data(), rows_only ? nullptr : chol.data(), W.data(), nullptr, stats.data());
    if (src == SRC_BOOT) rq.boot = &boot;
    if (src == SRC_T) rq.st = &st;
    if (src == SRC_FHS) { rq.filt = &filt; rq.gv = &gv; }
    if (bits & B_DD) ask_drawdown(rq, nullptr, second_stats.data());
    if (bits & B_HZ) ask_horizons(rq, true, H, steps, 0, nullptr, nullptr, hz_stats.data(), nullptr);
    if (bits & B_REB) { rq.rebalanced = true; rq.reb = (bits & B_BAND) ? &bd_reb : &reb; }
    if (bits & B_BAND) { rq.band = true; rq.bd = &bd; rq.trade_hist_out = trade_hist.data(); rq.turnover_stats_out = second_stats.data(); }
    if (bits & B_CASH) { rq.cash = true; rq.cf = (bits & B_SPEND) ? &no_cf : &cf; }
    if (bits & B_GLIDE) { rq.glide = true; rq.gl = &gl; }
    if (bits & B_SPEND) { rq.spend = true; rq.sp = &sp; rq.wd_stats_out = second_stats.data(); }
    if (bits & B_LIFE) { rq.life = true; rq.life_hist_out = life_hist.data(); }
    if (bits & B_PROTECT) { rq.protect = true; rq.pi = &pt; }
    if (bits & B_VT) { rq.vol_target = true; rq.vt = &vt; rq.exposure_stats_out = (bits & B_DD) ? nullptr : second_stats.data(); }
    if (bits & B_UW) { rq.underwater = true; rq.uw_longest_hist_out = uw_longest_hist.data(); rq.uw_current_hist_out = uw_current_hist.data(); }
    if (bits & B_PU) { rq.uncertain = true; rq.du = &du; }
    if (bits & B_OVERLAY) { rq.overlay = true; rq.ov = &ov; }
    if (bits & B_GARCH) { rq.garch = true; rq.gv = &gv; }
    if (bits & B_JUMPS) { rq.jumps = true; rq.jp = &jp; }
    if (bits & B_REGIMES) { rq.regimes = true; rq.rs = &rs; }
    if (bits & B_ANTI) { rq.anti = true; rq.pair_out = pair.data(); }
    if (bits & B_ATTR) { rq.attr = true; rq.attr_out = attr.data(); rq.attr_counts_out = attr_counts.data(); }
    if (rq.cash || rq.protect || rq.vol_target) { rq.counts_out = counts.data(); rq.hz_counts_out = rq.hz ? hz_counts.data() : nullptr; }
    return rq;
  }
};

enum Feature { PLAIN, BOOT, FILTERED, JUMPS, REGIMES, GLIDE_CF, GLIDE, PROTECT, CASH, OVERLAY, SPEND, SPEND_BOOT, BAND, BAND_BOOT, VOL_TARGET, UNDERWATER,
               UNCERTAIN, UNCERTAIN_CASH, N_FEATURES };
static const struct { const char* name; Source src; int bits; } k_features[N_FEATURES] = {
    {"plain", SRC_GAUSS, 0}, {"bootstrap", SRC_BOOT, 0}, {"filtered", SRC_FHS, 0}, {"jumps", SRC_GAUSS, B_JUMPS}, {"regimes", SRC_GAUSS, B_REGIMES},
    {"glide+flows", SRC_GAUSS, B_CASH | B_GLIDE}, {"glide", SRC_GAUSS, B_CASH | B_GLIDE}, {"protect", SRC_GAUSS, B_PROTECT},
    {"cash", SRC_GAUSS, B_CASH}, {"overlay", SRC_GAUSS, B_OVERLAY}, {"spend", SRC_GAUSS, B_CASH | B_SPEND},
    {"spend+bootstrap", SRC_BOOT, B_CASH | B_SPEND}, {"band", SRC_GAUSS, B_REB | B_BAND}, {"band+bootstrap", SRC_BOOT, B_REB | B_BAND},
    {"vol_target", SRC_GAUSS, B_VT}, {"underwater", SRC_GAUSS, B_DD | B_UW},
    {"uncertain", SRC_GAUSS, B_PU}, {"uncertain+flows", SRC_GAUSS, B_PU | B_CASH}};

static void run_shape(int N, int K, int T, int H) {
  Payloads p(N, K, T, 6);
  mcp_params prm = {N, T, K, MCP_COMPOUND_SIMPLE, 0, 0, 1.0, 0.95, 0.0};
  const int32_t* hs = H ? p.steps : nullptr;

  // every pure entry point, outputs of exactly the documented length
  snprintf(g_case, sizeof g_case, "entry points, N=%d K=%d T=%d H=%d", N, K, T, H);
  std::vector<double> pv(K), hz((size_t)H * K), p3(3), mean_count(1);
  std::vector<float> packed(mcp_packed_len(N, K)), drift(N);
  std::vector<uint64_t> thr3(3), rank(2);
  std::vector<uint32_t> jthr(MCP_MAX_JUMPS);
  double* hzp = H ? hz.data() : nullptr;
  EXPECT(mcp_abi_version() == MCP_ABI_VERSION && !packed.empty());
  EXPECT(mcp_pack_params(N, K, p.mu.data(), p.chol.data(), p.W.data(), packed.data(), packed.size()) == MCP_OK && finite(packed));
  EXPECT(mcp_pivots(&prm, p.mu.data(), p.chol.data(), p.W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_rebalance_pivots(&prm, &p.reb, p.mu.data(), nullptr, p.W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_rebalance_pivots(&prm, &p.reb, nullptr, &p.boot, p.W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_bootstrap_pivots(&prm, &p.boot, p.W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_filtered_pivots(&prm, &p.filt, p.W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_cashflow_pivots(&prm, &p.cf, p.mu.data(), nullptr, p.W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_overlay_pivots(&prm, &p.ov, p.mu.data(), p.W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_regime_pivots(&prm, &p.rs, p.mu.data(), p.W.data(), H, hs, pv.data(), hzp) == MCP_OK && finite(pv) && finite(hz));
  EXPECT(mcp_glide_pivots(&prm, &p.gl, &p.cf, p.mu.data(), nullptr, p.W.data(), H, hs, pv.data(), hzp) == MCP_OK && finite(pv) && finite(hz));
  EXPECT(mcp_protect_pivots(&prm, &p.pt, p.mu.data(), p.W.data(), H, hs, pv.data(), hzp) == MCP_OK && finite(pv) && finite(hz));
  {                                       // SPEC.md 4.19 / 5.19: the pivots, and the six constants with s0_k behind them
    std::vector<float> vc(6 + (size_t)K);
    EXPECT(mcp_vol_target_pivots(&prm, &p.vt, p.mu.data(), p.chol.data(), p.W.data(), H, hs, pv.data(), hzp) == MCP_OK && finite(pv) && finite(hz));
    EXPECT(mcp_vol_target_consts(&prm, &p.vt, p.chol.data(), p.W.data(), vc.data()) == MCP_OK && finite(vc) && vc[0] == 0.01f && vc[1] == 0.94f &&
           vc[2] == (float)(1.0 - (double)0.94f) && vc[3] == 1.5f && vc[6] > 0.0f);
    EXPECT(mcp_vol_target_consts(&prm, &p.vt, nullptr, p.W.data(), vc.data()) == MCP_E_ARG);   // the default s0 needs the factor
  }
  std::vector<double> wdp(K);
  std::vector<float> c5(5);
  EXPECT(mcp_spending_pivots(&prm, &p.sp, p.mu.data(), nullptr, p.W.data(), H, hs, pv.data(), hzp, wdp.data()) == MCP_OK && finite(pv) && finite(hz) && finite(wdp));
  EXPECT(mcp_spending_pivots(&prm, &p.sp, nullptr, &p.boot, p.W.data(), H, hs, pv.data(), hzp, wdp.data()) == MCP_OK && finite(pv) && finite(hz) && finite(wdp));
  EXPECT(mcp_spending_consts(&p.sp, prm.v0, c5.data()) == MCP_OK && std::isinf(c5[3]) && c5[4] == 0.015f);
  {                                       // SPEC.md 5.17 on an exactly sized histogram: T + 1 bins, one level per quartile
    std::vector<uint64_t> lh((size_t)T + 1, 1);
    std::vector<double> lq = {0.0, 25.0, 50.0, 100.0};
    std::vector<uint32_t> got(lq.size());
    uint64_t total = 0;
    EXPECT(mcp_lifetime_summary(lh.data(), T, (int)lq.size(), lq.data(), &total, got.data()) == MCP_OK && total == (uint64_t)T * (T + 1) / 2 &&
           got[0] == 0 && got[1] == (uint32_t)(T / 4) && got[2] == (uint32_t)(T / 2) && got[3] == (uint32_t)T);
    EXPECT(mcp_lifetime_summary(lh.data(), T, 0, nullptr, &total, nullptr) == MCP_OK);
  }
  EXPECT(mcp_band_reviews(&prm, &p.bd) == (T - 1) / 5 && mcp_band_reviews(&prm, nullptr) == -1);
  EXPECT(mcp_regime_consts(&p.rs, thr3.data(), p3.data()) == MCP_OK && finite(p3));
  EXPECT(mcp_jump_consts(&p.jp, N, p.mu.data(), jthr.data(), mean_count.data(), drift.data()) == MCP_OK && finite(mean_count) && finite(drift));
  EXPECT(mcp_percentile_rank(1000, 0.95, &rank[0], &rank[1], p3.data()) == MCP_OK && rank[1] == rank[0] + 1 && finite(p3));
  EXPECT(mcp_percentile_rank_q(1000, 2.5, &rank[0], &rank[1], p3.data()) == MCP_OK && rank[1] == rank[0] + 1 && finite(p3));

  // every feature: the request's rules, then the block and the pivots of every tile on exactly sized buffers
  for (int f = 0; f < N_FEATURES; f++) {
    snprintf(g_case, sizeof g_case, "%s, N=%d K=%d T=%d H=%d", k_features[f].name, N, K, T, H);
    Request rq = p.request(k_features[f].src, k_features[f].bits | (H ? B_HZ : 0));
    if (f == GLIDE) rq.cf = &p.no_cf;
    std::vector<float> second((size_t)K * 4);                // [K][4 paths] the optional per-path outputs
    std::vector<uint32_t> record((size_t)K * 4), record2((size_t)K * 4);
    std::vector<mcp_stats> second_stats(K);
    if (f == UNDERWATER && H) {           // SPEC.md 4.20: the drawdown walk stores no horizons, with or without the counters
      EXPECT(check_request(&prm, rq, 4) == MCP_E_UNSUPPORTED);
      continue;
    }
    if (rq.underwater) {
      ask_drawdown(rq, second.data(), second_stats.data());
      rq.uw_longest_out = record.data();
      rq.uw_current_out = record2.data();
    }
    if (rq.band) { rq.turnover_out = second.data(); rq.turnover_stats_out = second_stats.data(); rq.trades_out = record.data(); }
    if (rq.spend) { rq.wd_out = second.data(); rq.wd_stats_out = second_stats.data(); }
    if (rq.vol_target) { rq.exposure_out = second.data(); rq.exposure_stats_out = second_stats.data(); }
    EXPECT(check_request(&prm, rq, 4) == MCP_OK);
    {                                     // the one second array and the integer records of the request, on the request's own outputs
      const Second sec = second_of(rq);
      const Counted cnt = counted_of(&prm, rq);
      EXPECT(sec.on == (rq.band || rq.spend || rq.vol_target || rq.underwater) && cnt.on == (rq.band || rq.underwater) && cnt.bins == count_bins(&prm, rq));
      EXPECT(sec.out == (sec.on ? second.data() : nullptr) && sec.stats_out == (sec.on ? second_stats.data() : nullptr));
      EXPECT(cnt.out == (cnt.on ? record.data() : nullptr) &&
             cnt.hist_out == (rq.band ? p.trade_hist.data() : rq.underwater ? p.uw_longest_hist.data() : nullptr));
      EXPECT(cnt.records == (rq.underwater ? 2 : cnt.on ? 1 : 0) && cnt.out2 == (rq.underwater ? record2.data() : nullptr) &&
             cnt.hist_out2 == (rq.underwater ? p.uw_current_hist.data() : nullptr));
      if (rq.underwater) EXPECT(cnt.bins == (size_t)T + 1 && sec.unit_v0 && !sec.pivoted);   // SPEC.md 5.20: the lifetime's bins; 5.1's record
      if (rq.band) EXPECT(sec.unit_v0 && !sec.pivoted);   // SPEC.md 5.18: x = Y - 1, no pivot
      if (rq.spend) EXPECT(!sec.unit_v0 && sec.pivoted);  // SPEC.md 5.16: x = Y / fl32(v0) - 1, the pivots of request_wd_pivots
      if (rq.vol_target) EXPECT(sec.unit_v0 && !sec.pivoted);   // SPEC.md 5.19: x = Y - 1, no pivot
      Request dr = rq;                                    // SPEC.md 5.1: the drawdown, where the request may carry it
      ask_drawdown(dr, second.data(), second_stats.data());
      if (check_request(&prm, dr, 4) == MCP_OK) {
        const Second dd = second_of(dr);
        EXPECT(dd.on && dd.unit_v0 && !dd.pivoted && dd.out == second.data() && dd.stats_out == second_stats.data());
      }
    }
    {                                     // SPEC.md 4.17: the lifetime is taken by the walks with ruin and refused by every other
      std::vector<uint64_t> lh((size_t)K * (T + 1));
      Request lr = rq;
      lr.life = true;
      lr.life_hist_out = lh.data();
      lr.life_out = record.data();
      const Counted cnt = counted_of(&prm, lr);
      if (rq.cash) EXPECT(cnt.on && cnt.bins == (size_t)T + 1 && cnt.bins == count_bins(&prm, lr) && cnt.out == record.data() && cnt.hist_out == lh.data());
      lr.life_out = nullptr;
      EXPECT(check_request(&prm, lr, 4) == (rq.cash && !rq.uncertain ? MCP_OK : MCP_E_UNSUPPORTED));   // SPEC.md 4.21: not with the per-path drift
      lr.life_hist_out = nullptr;
      EXPECT(check_request(&prm, lr, 4) == (rq.cash ? MCP_E_ARG : MCP_E_UNSUPPORTED));
    }
    if (rq.vol_target) {                  // SPEC.md 4.19 / 5.19: one second array; a bad constant; s0 behind the block, padded with ones
      Request vr = rq;
      ask_drawdown(vr, nullptr, p.second_stats.data());
      EXPECT(check_request(&prm, vr, 4) == MCP_E_UNSUPPORTED);             // the exposure record together with the drawdown
      vr.exposure_out = nullptr;
      vr.exposure_stats_out = nullptr;
      EXPECT(check_request(&prm, vr, 4) == (H ? MCP_E_UNSUPPORTED : MCP_OK) && second_of(vr).stats_out == p.second_stats.data());
      vr = rq;
      vr.exposure_stats_out = nullptr;
      EXPECT(check_request(&prm, vr, 4) == MCP_E_ARG);
      std::vector<double> s0(K, 1e-4);
      mcp_vol_target bad_vt = p.vt;
      bad_vt.s0 = s0.data();
      vr = rq;
      vr.vt = &bad_vt;
      EXPECT(check_request(&prm, vr, 4) == MCP_OK);
      s0.back() = 0.0;
      EXPECT(check_request(&prm, vr, 4) == MCP_E_ARG);
      bad_vt = p.vt;
      bad_vt.decay = 1.0000001;
      EXPECT(check_request(&prm, vr, 4) == MCP_E_ARG);
      bad_vt = p.vt;
      bad_vt.spread = -1e-9;
      EXPECT(check_request(&prm, vr, 4) == MCP_E_ARG);
      const TileLayout lay = tile_layout(&prm, rq, K);
      EXPECT(lay.total - lay.floor == 8 * (((size_t)K + 7) / 8));
    }
    if (rq.underwater) {                  // SPEC.md 4.20: a missing histogram; no drawdown; what the counters are not combined with; the step limit
      Request ur = rq;
      ur.uw_current_hist_out = nullptr;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_ARG);
      ur = rq;
      ask_drawdown(ur, nullptr, nullptr);
      EXPECT(check_request(&prm, ur, 4) == MCP_E_ARG);
      ur = rq;
      ur.regimes = true;
      ur.rs = &p.rs;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_UNSUPPORTED);
      ur = rq;
      ur.anti = true;
      ur.pair_out = p.pair.data();
      EXPECT(check_request(&prm, ur, 4) == MCP_E_UNSUPPORTED);
      mcp_params big = prm;
      big.n_steps = MCP_MAX_LIFE_STEPS + 1;
      EXPECT(check_request(&big, rq, 4) == MCP_E_UNSUPPORTED);
      mcp_params lg = prm;
      lg.compounding = MCP_COMPOUND_LOG;  // Gaussian draws compound either way; the GARCH, Student-t and jump walks simply
      EXPECT(check_request(&lg, rq, 4) == MCP_OK);
      ur = rq;
      ur.garch = true;
      ur.gv = &p.gv;
      EXPECT(check_request(&prm, ur, 4) == MCP_OK && check_request(&lg, ur, 4) == MCP_E_UNSUPPORTED);
      ur.jumps = true;
      ur.jp = &p.jp;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_UNSUPPORTED);
    }
    if (rq.uncertain) {                   // SPEC.md 4.21: the struct's rules, the refusals, M behind the block, never the lean step loop
      Request ur = rq;
      ur.du = nullptr;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_ARG);
      mcp_drift_uncertainty bad_du = p.du;
      ur.du = &bad_du;
      bad_du.factor = nullptr;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_ARG);
      bad_du = p.du;
      bad_du.reserved = 1;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_ARG);
      std::vector<float> inf_m(p.drift_m);
      inf_m.back() = HUGE_VALF;
      bad_du = {inf_m.data(), 0};
      EXPECT(check_request(&prm, ur, 4) == MCP_E_ARG);
      inf_m.back() = NAN;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_ARG);
      std::vector<float> zero_m(p.drift_m.size(), 0.0f);
      bad_du = {zero_m.data(), 0};
      EXPECT(check_request(&prm, ur, 4) == MCP_OK);        // all-zero is allowed
      mcp_params lg = prm;
      lg.compounding = MCP_COMPOUND_LOG;
      EXPECT(check_request(&lg, rq, 4) == (rq.cash ? MCP_E_UNSUPPORTED : MCP_OK));
      mcp_params fold = prm;
      fold.flags = MCP_FLAG_FOLD;
      EXPECT(check_request(&fold, rq, 4) == MCP_E_UNSUPPORTED);
      ur = rq;
      ask_drawdown(ur, nullptr, p.second_stats.data());
      EXPECT(check_request(&prm, ur, 4) == (H || rq.cash ? MCP_E_UNSUPPORTED : MCP_OK));
      ur = rq;
      ur.garch = true;
      ur.gv = &p.gv;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_UNSUPPORTED);
      ur = rq;
      ur.src = SRC_T;
      ur.st = &p.st;
      EXPECT(check_request(&prm, ur, 4) == MCP_E_UNSUPPORTED);
      const TileLayout lay = tile_layout(&prm, rq, K);
      EXPECT(lay.floor - lay.load == drift_len(N) && lay.total == lay.floor);
      for (uint64_t begin : {(uint64_t)0, ((uint64_t)1 << 32) - 2}) {
        const mcp::PathKernel k = route_kernel(&prm, rq, false, begin, 4);
        EXPECT((k.flags & mcp::PK_PU) && !(k.flags & mcp::PK_UHI));
      }
    }
    if (rq.band) {                        // SPEC.md 4.18: a negative entry, a missing histogram, and the size of the histogram
      Request br = rq;
      std::vector<float> neg(p.tol);
      neg.back() = -0.01f;
      const mcp_band bad_bd = {5, 0, 0.001, neg.data()};
      br.bd = &bad_bd;
      EXPECT(check_request(&prm, br, 4) == MCP_E_ARG);
      br = rq;
      br.trade_hist_out = nullptr;
      EXPECT(check_request(&prm, br, 4) == MCP_E_ARG);
      EXPECT(count_bins(&prm, rq) * (size_t)K == p.trade_hist.size());
    }
    TileInputs in;
    EXPECT(tile_inputs(&prm, rq, &in) == MCP_OK);
    const int tiles[3][2] = {{0, K}, {0, K < 8 ? K : 8}, {8, K - 8}};     // the whole call; K = 9 also as tiles of 8 and 1
    for (int t = 0; t < (K == 9 ? 3 : 1); t++) {
      const int k0 = tiles[t][0], kt = tiles[t][1];
      const TileLayout lay = tile_layout(&prm, rq, kt);
      EXPECT(lay.base == mcp_packed_len(N, kt) && lay.base <= lay.load && lay.load <= lay.floor && lay.floor <= lay.total);
      std::vector<float> block(lay.total);
      std::vector<double> piv(kt), piv_hz((size_t)H * kt);
      EXPECT(pack_tile(&prm, rq, in, k0, kt, block.data()) == MCP_OK);
      block.resize(lay.floor + (rq.protect ? (size_t)T + 1 : 0));         // the thresholds behind the schedule may be -inf (no target)
      if (rq.band) {                                                      // the table is finite (+0 where not watched); behind it the mask words
        EXPECT(lay.floor - lay.load == band_len(N, kt));
        const uint32_t* words = (const uint32_t*)(block.data() + lay.load + (size_t)kt * (4 * ((N + 3) / 4)));
        for (int k = 0; k < kt; k++) {
          const uint64_t watch = (uint64_t)words[2 * k] | (uint64_t)words[2 * k + 1] << 32;
          EXPECT(watch == (N == 1 ? 0 : (N - 1 == 64 ? ~0ull : (1ull << (N - 1)) - 1)));
        }
        block.resize(lay.load + (size_t)kt * (4 * ((N + 3) / 4)));
      }
      EXPECT(finite(block));
      EXPECT(request_pivots(&prm, rq, in, k0, kt, piv.data(), H ? piv_hz.data() : nullptr) == MCP_OK && finite(piv) && finite(piv_hz));
      if (rq.spend) {
        request_wd_pivots(&prm, rq, k0, kt, piv.data());
        EXPECT(finite(piv));
      }
    }
    // one invalid request per feature and its documented code
    mcp_params bad = prm;
    mcp_bootstrap bad_boot = p.boot;
    if (f == PLAIN) bad.flags = MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH;      // the folded step needs the spec's normals
    else if (f == BOOT) { bad_boot.mean_block = 0.5; rq.boot = &bad_boot; }  // the bootstrap compounds either way; b < 1 does not
    else if (f == UNDERWATER) bad.flags = MCP_FLAG_NATIVE_MATH;          // the drawdown walk runs on the spec's normals
    else if (f == UNCERTAIN) bad.flags = MCP_FLAG_NATIVE_MATH;           // the per-path drift compounds either way, on the spec's normals only
    else bad.compounding = MCP_COMPOUND_LOG;                              // every other feature compounds simply
    EXPECT(check_request(&bad, rq, 4) == (f == BOOT ? MCP_E_ARG : MCP_E_UNSUPPORTED) && mcp_last_error()[0] != '\0');
  }
}

// The plan of one call (plan_tiles) against what it promises: every (portfolio, path) cell once, the shape of either sharding, the
// budget, whole K_PAD tiles, and which shards walk paths.
static void check_plan(size_t S, int K, uint64_t n, bool by_portfolio, uint64_t unit, size_t budget, size_t bytes) {
  snprintf(g_case, sizeof g_case, "plan S=%zu K=%d n=%llu %s unit=%llu budget=%zu", S, K, (unsigned long long)n,
           by_portfolio ? "portfolios" : "paths", (unsigned long long)unit, budget);
  const TilePlan plan = plan_tiles(S, K, n, by_portfolio, unit, budget, bytes);
  EXPECT(plan.S == S && plan.tiles() >= 1 && plan.jobs.size() == plan.tiles() * S);
  std::vector<unsigned char> seen((size_t)K * n, 0);
  std::vector<int> next(S);                                  // portfolio shards: where shard s goes on
  for (size_t s = 0; s < S; s++) next[s] = (int)((int64_t)K * (int64_t)s / (int64_t)S);
  for (size_t t = 0; t < plan.tiles(); t++) {
    const Job* jobs = plan.tile(t);
    bool any = false;
    for (size_t s = 0; s < S; s++) {
      const Job& j = jobs[s];
      const int slice_end = (int)((int64_t)K * (int64_t)(s + 1) / (int64_t)S);
      if (by_portfolio) {
        EXPECT(j.active == (next[s] < slice_end));           // active until its slice is done, never on an empty slice
        if (!j.active) continue;
        EXPECT(j.k0 == next[s] && j.kt >= 1 && j.k0 + j.kt <= slice_end && j.p0 == 0 && j.pn == n);
        const uint64_t fit = budget / (bytes * n);
        if (j.kt < slice_end - next[s] && fit >= (uint64_t)K_PAD) EXPECT(j.kt % K_PAD == 0);
        next[s] += j.kt;
      } else {
        EXPECT(j.active && j.k0 == jobs[0].k0 && j.kt == jobs[0].kt && j.kt >= 1 && j.k0 + j.kt <= K);
        EXPECT(j.p0 == (s ? jobs[s - 1].p0 + jobs[s - 1].pn : 0) && j.p0 % unit == 0 && j.pn % unit == 0);
        if (s) EXPECT(j.pn <= jobs[s - 1].pn);               // the remainder goes to the first shards: pn = 0 only at the end
        if (s + 1 == S) EXPECT(j.p0 + j.pn == n);
        EXPECT(j.k0 == (t ? plan.tile(t - 1)[s].k0 + plan.tile(t - 1)[s].kt : 0));
        const uint64_t fit = budget / (bytes * (jobs[0].pn ? jobs[0].pn : 1));   // shard 0 holds the largest range
        if (j.kt < K && j.k0 + j.kt < K && fit >= (uint64_t)K_PAD) EXPECT(j.kt % K_PAD == 0);
      }
      any = true;
      if (j.kt > 1) EXPECT((uint64_t)j.kt * j.pn * bytes <= budget);
      for (int k = j.k0; k < j.k0 + j.kt; k++)
        for (uint64_t p = j.p0; p < j.p0 + j.pn; p++) seen[(size_t)k * n + p]++;
    }
    EXPECT(any);                                             // no tile without work
    if (!by_portfolio && t + 1 == plan.tiles()) EXPECT(jobs[0].k0 + jobs[0].kt == K);
  }
  for (unsigned char c : seen) EXPECT(c == 1);
  for (size_t s = 0; s < S && unit == 1; s++) {              // the shards that take the row table of a bootstrap call (never antithetic)
    const bool walks = by_portfolio ? (int64_t)K * (int64_t)(s + 1) / (int64_t)S > (int64_t)K * (int64_t)s / (int64_t)S
                                    : n / S + (s < n % S ? 1 : 0) > 0;
    EXPECT(plan.walks(s) == walks);
  }
}

static void run_plans() {
  const size_t Ss[4] = {1, 2, 3, 8}, bytes = sizeof(float);
  const int Ks[5] = {1, 3, 17, 600, 1700};
  const uint64_t ns[4] = {1, 2, 5, 4098};
  for (size_t S : Ss)
    for (int K : Ks)
      for (uint64_t n : ns)
        for (int mode = 0; mode < 3; mode++) {               // path shards, path shards of antithetic pairs, portfolio shards
          const bool by_portfolio = mode == 2;
          const uint64_t unit = mode == 1 ? 2 : 1;
          if (unit == 2 && (n & 1)) continue;
          const uint64_t units = n / unit, pn_max = by_portfolio ? n : unit * (units / S + (units % S ? 1 : 0));
          const size_t per = bytes * (size_t)(pn_max ? pn_max : 1);
          for (size_t fit : {(size_t)K, (size_t)1100, (size_t)3, (size_t)1})   // tiles of K, of 1024 (K = 1700), of 3 and of 1 portfolio
            check_plan(S, K, n, by_portfolio, unit, fit * per, bytes);
        }
  // tests/test_gpu_round2.py::test_terminal_budget_tiles_the_portfolios, one shard: room for 600 portfolios of 8192 paths
  snprintf(g_case, sizeof g_case, "pinned plan, 1700 portfolios");
  {
    const TilePlan plan = plan_tiles(1, 1700, 8192, false, 1, (size_t)600 * 8192 * 4, 4);
    const int want[4][2] = {{0, 512}, {512, 512}, {1024, 512}, {1536, 164}};
    EXPECT(plan.tiles() == 4);
    for (size_t t = 0; t < 4; t++) {
      const Job& j = plan.tile(t)[0];
      EXPECT(j.active && j.k0 == want[t][0] && j.kt == want[t][1] && j.p0 == 0 && j.pn == 8192);
    }
  }
  // tests/test_gpu_band.py::test_property_d_shards_and_tiles, one shard: 5 banded portfolios with two horizons, two per tile
  snprintf(g_case, sizeof g_case, "pinned plan, banded call");
  {
    const int32_t steps[2] = {10, 30};
    const uint64_t n = 30001;
    Request rq;
    rq.rebalanced = rq.band = true;
    ask_horizons(rq, true, 2, steps, 0, nullptr, nullptr, nullptr, nullptr);
    const TilePlan plan = plan_tiles(1, 5, n, false, 1, 2 * n * (4 * (1 + 2) + 12), tile_bytes_per_path(rq));
    const int want[3][2] = {{0, 2}, {2, 2}, {4, 1}};
    EXPECT(plan.tiles() == 3);
    for (size_t t = 0; t < 3; t++) {
      const Job& j = plan.tile(t)[0];
      EXPECT(j.active && j.k0 == want[t][0] && j.kt == want[t][1] && j.p0 == 0 && j.pn == n);
    }
  }
  // what the budget counts per path and portfolio
  snprintf(g_case, sizeof g_case, "tile_bytes_per_path");
  const int32_t steps[2] = {1, 2};
  for (int H : {0, 2}) {
    Request rq;
    ask_horizons(rq, H != 0, H, steps, 0, nullptr, nullptr, nullptr, nullptr);
    const size_t hz = 4 * (size_t)H;
    Request dd = rq, spend = rq, life = rq, spend_life = rq, band = rq, uw = rq;
    dd.dd = true;
    uw.dd = uw.underwater = true;
    spend.cash = spend.spend = true;
    life.cash = life.life = true;
    spend_life.cash = spend_life.spend = spend_life.life = true;
    band.rebalanced = band.band = true;
    EXPECT(tile_bytes_per_path(rq) == 4 + hz && tile_bytes_per_path(spend) == 8 + hz && tile_bytes_per_path(life) == 8 + hz);
    EXPECT(tile_bytes_per_path(spend_life) == 12 + hz && tile_bytes_per_path(band) == 16 + hz);
    if (!H) EXPECT(tile_bytes_per_path(dd) == 8 && tile_bytes_per_path(uw) == 16);   // the drawdown and horizons are never asked together
  }
}

// ---- the routing: check_request -> route_kernel -> the rows of mcp_paths_ladder.inc ----
// Every combination of draw source, features, compounding, flags, view (mcp_simulate* or mcp_launch_paths*) and path range (one that
// passes lean_range, one that crosses 2^32; even, so that pairs stay legal) goes to visit(prm, rq, ln or NULL, path_begin, n_paths) on
// minimal valid arguments, for NB = 1, 4, 5, 16 (the smallest N of each) and K = 1, 2, and for K = 20 at NB = 1: K meets the limits
// of the folded step and the attribution and sets the pass width, none of which looks at N.  `visit` says whether check_request
// accepts; a request on rows that it accepts on a table that fits LDS (8 rows) comes again on the first table that does not --
// check_request scans the table, and sees its size in check_boot's and check_filtered's own rules only.
template <class Visit>
static void for_each_request(Visit&& visit) {
  static float d_array[1];                                   // an mcp_launch_paths* call's device arrays are only tested against NULL
  const int T = 12, shapes[9][2] = {{1, 1}, {1, 2}, {1, 20}, {4, 1}, {4, 2}, {5, 1}, {5, 2}, {16, 1}, {16, 2}};   // (NB, K)
  const uint64_t ranges[2][2] = {{0, 66}, {(1ull << 32) - 64, 66}};
  for (const auto& shape : shapes) {
    const int nb = shape[0], N = 4 * nb - 3, K = shape[1];
    int r_boot = 8, r_filt = 8;
    while (mcp::boot_fits_lds((uint64_t)r_boot, nb)) r_boot++;
    while (mcp::filt_fits_lds((uint64_t)r_filt, nb)) r_filt++;
    Payloads fits(N, K, T, 8), big_boot(N, K, T, r_boot), big_filt(N, K, T, r_filt);
    for (int src = SRC_GAUSS; src <= SRC_FHS; src++)
      for (int bits = 0; bits < 1 << N_BITS_PU; bits++) {
        // SPEC.md 4.21: the per-path drift comes with every set of up to three other features -- what it combines with (the drawdown,
        // horizons, cash flows) has no larger set, and every other feature is refused alone and in every pair and triple; the larger
        // sets would double the run for refusals that the rule's one sentence already states
        if ((bits & B_PU) && __builtin_popcount((unsigned)(bits & ~B_PU)) > 3) continue;
        const Request rq = fits.request((Source)src, bits);
        for (int compounding : {MCP_COMPOUND_SIMPLE, MCP_COMPOUND_LOG})
          for (int flags : {0, (int)MCP_FLAG_NATIVE_MATH, (int)MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH | MCP_FLAG_FOLD}) {
            const mcp_params prm = {N, T, K, compounding, flags, 0, 1.0, 0.95, 0.0};
            for (const auto& range : ranges) {
              Launch ln;
              ln.d_packed = ln.d_terminal = d_array;
              ln.path_begin = range[0];
              ln.n_paths = ln.stride = ln.mdd_stride = ln.hz_stride = range[1];
              if (rq.dd) ln.d_mdd = d_array;
              if (rq.hz) ln.d_hz = d_array;
              for (const Launch* view : {(const Launch*)nullptr, (const Launch*)&ln})
                if (visit(prm, rq, view, range[0], range[1]) && (src == SRC_BOOT || src == SRC_FHS)) {
                  snprintf(g_case, sizeof g_case, "the table that does not fit LDS: nb=%d K=%d src=%d bits=0x%x", nb, K, src, bits);
                  EXPECT(visit(prm, (src == SRC_BOOT ? big_boot : big_filt).request((Source)src, bits), view, range[0], range[1]));
                }
            }
          }
      }
  }
}

// The rows of mcp_paths_ladder.inc that exist at (NB, KT), the text the device build compiles, with the kernel's name for the launch
struct Row { int family; uint32_t mask; const char* kernel; };
template <int NB, int KT>
static std::vector<Row> ladder_rows() {
  using namespace mcp;
  std::vector<Row> rows;
#define MCP_ROW_IF(cond, family, mask, ...) \
  if constexpr (cond) rows.push_back(Row{family, mask, #__VA_ARGS__});
#include "mcp_paths_ladder.inc"
#undef MCP_ROW_IF
  return rows;
}
static const std::vector<Row>& rows_at(int nb, bool kt8) {
  static const std::vector<Row> at[4][2] = {{ladder_rows<1, 1>(), ladder_rows<1, 8>()}, {ladder_rows<4, 1>(), ladder_rows<4, 8>()},
                                            {ladder_rows<5, 1>(), ladder_rows<5, 8>()}, {ladder_rows<16, 1>(), ladder_rows<16, 8>()}};
  return at[nb == 1 ? 0 : nb == 4 ? 1 : nb == 5 ? 2 : 3][kt8];
}
// The row that `k` selects at `nb`, as launch_paths_nb<nb> finds it; *n_out: how many rows it equals
static const Row* select_row(int nb, const mcp::PathKernel& k, int* n_out = nullptr) {
  const Row* hit = nullptr;
  int n = 0;
  for (const Row& r : rows_at(nb, (k.flags & mcp::PK_KT8) != 0))
    if (mcp::selects(k, r.family, r.mask)) { if (!hit) hit = &r; n++; }
  if (n_out) *n_out = n;
  return hit;
}

static long run_routes() {
  using namespace mcp;
  // (d) the table: 93 rows for NB <= LEAN_MAX_NB (the two lean kernels), 91 above; at KT = 8 without the folded step, the lean kernels,
  // the bands and the attribution
  for (int nb : {1, 4, 5, 16}) {
    snprintf(g_case, sizeof g_case, "row counts, nb=%d", nb);
    EXPECT(rows_at(nb, false).size() == (nb <= LEAN_MAX_NB ? 93u : 91u) && rows_at(nb, true).size() == 85u);
  }
  // (a) every accepted request has exactly one row; (b) its selector is canonical: with any one flag set or cleared it is another
  // kernel's or nobody's -- under equality that is (a) again, asserted all the same, once per selector and nb; (c) every row is
  // reached, at KT = 1 and where it exists at KT = 8
  std::set<std::pair<int, uint32_t>> reached[2];             // (family, mask) by kt8
  std::set<std::pair<int, std::pair<int, uint32_t>>> canonical;
  long n_requests = 0, n_accepted = 0;
  for_each_request([&](const mcp_params& prm, const Request& rq, const Launch* ln, uint64_t path_begin, uint64_t n_paths) {
    n_requests++;
    if (check_request(&prm, rq, n_paths, ln, path_begin) != MCP_OK) return false;
    n_accepted++;
    const int nb = (prm.n_assets + 3) / 4;
    for (int attr_walk = 0; attr_walk <= (rq.attr ? 1 : 0); attr_walk++) {
      const PathKernel k = route_kernel(&prm, rq, attr_walk != 0, path_begin, n_paths);
      if (!canonical.insert({nb, {k.family, k.flags}}).second) continue;
      snprintf(g_case, sizeof g_case, "route nb=%d K=%d src=%d family=%d flags=0x%x", nb, prm.n_portfolios, (int)rq.src, k.family, k.flags);
      int n = 0;
      const Row* row = select_row(nb, k, &n);
      EXPECT(n == 1);
      for (int b = 0; b < N_PATH_FLAGS_PU; b++) {
        const PathKernel other = {k.family, k.flags ^ (1u << b)};
        EXPECT(select_row(nb, other) != row);               // PK_KT8: the row of the table at the other KT, another kernel
      }
      reached[(k.flags & PK_KT8) != 0].insert({row->family, row->mask});
    }
    return true;
  });
  for (int kt8 = 0; kt8 < 2; kt8++)
    for (const Row& r : rows_at(1, kt8 != 0)) {
      snprintf(g_case, sizeof g_case, "no accepted request reaches %s (family %d, mask 0x%x) at KT = %d", r.kernel, r.family, r.mask, kt8 ? 8 : 1);
      EXPECT(reached[kt8].count({r.family, r.mask}) == 1);
    }
  snprintf(g_case, sizeof g_case, "accepted requests");
  EXPECT(n_accepted > 0 && n_accepted < n_requests);
  return n_requests;
}

// (e) the kernel of the named requests, literally: what runs what.  NB and KT stand for ceil(N / 4) and for 8 (K >= 2) or 1.
static void run_named_routes() {
  const uint64_t far = (1ull << 32) - 64;
  const struct { const char* what; Source src; int bits, compounding, flags, K, N; uint64_t path_begin; bool attr_walk; const char* kernel; } named[] = {
      {"plain, one portfolio", SRC_GAUSS, 0, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_lean_kernel<NB, false>"},
      {"plain, log", SRC_GAUSS, 0, MCP_COMPOUND_LOG, 0, 1, 16, 0, false, "mc_paths_lean_kernel<NB, true>"},
      {"plain, N > 16", SRC_GAUSS, 0, MCP_COMPOUND_SIMPLE, 0, 1, 17, 0, false, "mc_paths_kernel<NB, KT, 1, false, false, false>"},
      {"plain, across 2^32", SRC_GAUSS, 0, MCP_COMPOUND_SIMPLE, 0, 1, 16, far, false, "mc_paths_kernel<NB, KT, 1, false, false, false>"},
      {"plain, K = 2", SRC_GAUSS, 0, MCP_COMPOUND_LOG, 0, 2, 16, 0, false, "mc_paths_kernel<NB, KT, 1, false, false, true>"},
      {"plain, native math", SRC_GAUSS, 0, MCP_COMPOUND_SIMPLE, MCP_FLAG_NATIVE_MATH, 2, 16, 0, false, "mc_paths_kernel<NB, KT, 1, true, false, false>"},
      {"plain, folded", SRC_GAUSS, 0, MCP_COMPOUND_LOG, MCP_FLAG_FOLD, 1, 16, 0, false, "mc_paths_kernel<NB, 1, 1, false, true, true>"},
      {"drawdown", SRC_GAUSS, B_DD, MCP_COMPOUND_LOG, 0, 1, 16, 0, false, "mc_paths_dd_kernel<NB, KT, 1, true>"},
      {"horizons", SRC_GAUSS, B_HZ, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_hz_kernel<NB, KT, 1, false>"},
      {"bootstrap", SRC_BOOT, 0, MCP_COMPOUND_LOG, 0, 1, 16, 0, false, "mc_paths_boot_kernel<NB, KT, 1, true, true>"},
      {"bootstrap, horizons", SRC_BOOT, B_HZ, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_boot_hz_kernel<NB, KT, 1, false, true>"},
      {"filtered", SRC_FHS, 0, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_fhs_kernel<NB, KT, 1, true>"},
      {"filtered, horizons", SRC_FHS, B_HZ, MCP_COMPOUND_SIMPLE, 0, 2, 16, 0, false, "mc_paths_fhs_kernel<NB, KT, 1, true>"},
      {"Student-t", SRC_T, 0, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_t_kernel<NB, KT, 1>"},
      {"Student-t, drawdown", SRC_T, B_DD, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_t_dd_kernel<NB, KT, 1>"},
      {"GARCH", SRC_GAUSS, B_GARCH, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_g_kernel<NB, KT, 1>"},
      {"GARCH, Student-t, horizons", SRC_T, B_GARCH | B_HZ, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_g_hz_kernel<NB, KT, 1>"},
      {"jumps", SRC_GAUSS, B_JUMPS, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_j_kernel<NB, KT, 1>"},
      {"regimes, drawdown", SRC_GAUSS, B_REGIMES | B_DD, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_r_dd_kernel<NB, KT, 1>"},
      {"antithetic", SRC_GAUSS, B_ANTI, MCP_COMPOUND_LOG, 0, 1, 16, 0, false, "mc_paths_anti_kernel<NB, KT, 1, true, PathArgsA>"},
      {"antithetic, Student-t, drawdown", SRC_T, B_ANTI | B_DD, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_anti_kernel<NB, KT, 1, false, PathArgsGADD>"},
      {"attribution, first walk", SRC_GAUSS, B_ATTR, MCP_COMPOUND_SIMPLE, 0, 1, 17, 0, false, "mc_paths_kernel<NB, KT, 1, false, false, false>"},
      {"attribution, second walk", SRC_GAUSS, B_ATTR, MCP_COMPOUND_SIMPLE, 0, 2, 16, 0, true, "mc_paths_attr_kernel<NB, 1, 1>"},
      {"rebalanced", SRC_GAUSS, B_REB, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_reb_kernel<NB, KT, 1, false, false>"},
      {"band", SRC_GAUSS, B_REB | B_BAND, MCP_COMPOUND_SIMPLE, 0, 2, 16, 0, false, "mc_paths_band_kernel<NB, 1, 1, false, false>"},
      {"band, bootstrap", SRC_BOOT, B_REB | B_BAND, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_band_kernel<NB, 1, 1, true, true>"},
      {"cash", SRC_GAUSS, B_CASH, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_cf_kernel<NB, KT, 1, false, false, false>"},
      {"cash, Student-t", SRC_T, B_CASH, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_cf_kernel<NB, KT, 1, false, false, true>"},
      {"cash, lifetime", SRC_GAUSS, B_CASH | B_LIFE, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_glide_life_kernel<NB, KT, 1, false, false, false>"},
      {"glide", SRC_GAUSS, B_CASH | B_GLIDE, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_glide_kernel<NB, KT, 1, false, false, false>"},
      {"glide, lifetime", SRC_GAUSS, B_CASH | B_GLIDE | B_LIFE, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_glide_life_kernel<NB, KT, 1, false, false, false>"},
      {"spend", SRC_GAUSS, B_CASH | B_SPEND, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_spend_kernel<NB, KT, 1, false, false, false>"},
      {"spend, bootstrap", SRC_BOOT, B_CASH | B_SPEND, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_spend_kernel<NB, KT, 1, true, true, false>"},
      {"spend, lifetime", SRC_GAUSS, B_CASH | B_SPEND | B_LIFE, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_spend_life_kernel<NB, KT, 1, false, false, false>"},
      {"overlay", SRC_GAUSS, B_OVERLAY, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_ov_kernel<NB, KT, 1, false, false>"},
      {"overlay, Student-t, drawdown", SRC_T, B_OVERLAY | B_DD, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_ov_kernel<NB, KT, 1, true, true>"},
      {"protect", SRC_GAUSS, B_PROTECT, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_pi_kernel<NB, KT, 1, false, false>"},
      {"protect, GARCH, drawdown", SRC_GAUSS, B_PROTECT | B_GARCH | B_DD, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_pi_kernel<NB, KT, 1, false, true>"},
      {"protect, jumps, horizons", SRC_GAUSS, B_PROTECT | B_JUMPS | B_HZ, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_pi_kernel<NB, KT, 1, true, false>"},
      {"vol target", SRC_GAUSS, B_VT, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_vt_kernel<NB, KT, 1, false, false>"},
      {"vol target, Student-t, GARCH, drawdown", SRC_T, B_VT | B_GARCH | B_DD, MCP_COMPOUND_SIMPLE, 0, 2, 16, 0, false, "mc_paths_vt_kernel<NB, KT, 1, false, true>"},
      {"vol target, jumps, horizons", SRC_GAUSS, B_VT | B_JUMPS | B_HZ, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_vt_kernel<NB, KT, 1, true, false>"},
      {"under water", SRC_GAUSS, B_DD | B_UW, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_uw_kernel<NB, KT, 1, false>"},
      {"under water, log", SRC_GAUSS, B_DD | B_UW, MCP_COMPOUND_LOG, 0, 2, 17, 0, false, "mc_paths_uw_kernel<NB, KT, 1, true>"},
      {"under water, Student-t", SRC_T, B_DD | B_UW, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_g_uw_kernel<NB, KT, 1>"},
      {"under water, GARCH", SRC_GAUSS, B_DD | B_UW | B_GARCH, MCP_COMPOUND_SIMPLE, 0, 2, 16, 0, false, "mc_paths_g_uw_kernel<NB, KT, 1>"},
      {"under water, jumps", SRC_GAUSS, B_DD | B_UW | B_JUMPS, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_j_uw_kernel<NB, KT, 1>"},
      {"uncertain: never the lean kernel", SRC_GAUSS, B_PU, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_pu_kernel<NB, KT, 1, false>"},
      {"uncertain, log, K = 2", SRC_GAUSS, B_PU, MCP_COMPOUND_LOG, 0, 2, 17, 0, false, "mc_paths_pu_kernel<NB, KT, 1, true>"},
      {"uncertain, drawdown", SRC_GAUSS, B_PU | B_DD, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_pu_dd_kernel<NB, KT, 1, false>"},
      {"uncertain, drawdown, log", SRC_GAUSS, B_PU | B_DD, MCP_COMPOUND_LOG, 0, 1, 16, far, false, "mc_paths_pu_dd_kernel<NB, KT, 1, true>"},
      {"uncertain, horizons", SRC_GAUSS, B_PU | B_HZ, MCP_COMPOUND_SIMPLE, 0, 2, 16, 0, false, "mc_paths_pu_hz_kernel<NB, KT, 1, false>"},
      {"uncertain, horizons, log", SRC_GAUSS, B_PU | B_HZ, MCP_COMPOUND_LOG, 0, 1, 16, 0, false, "mc_paths_pu_hz_kernel<NB, KT, 1, true>"},
      {"uncertain, cash, horizons", SRC_GAUSS, B_PU | B_CASH | B_HZ, MCP_COMPOUND_SIMPLE, 0, 1, 16, 0, false, "mc_paths_pu_cf_kernel<NB, KT, 1>"},
  };
  for (const auto& c : named) {
    snprintf(g_case, sizeof g_case, "named route: %s", c.what);
    Payloads p(c.N, c.K, 12, 8);
    const mcp_params prm = {c.N, 12, c.K, c.compounding, c.flags, 0, 1.0, 0.95, 0.0};
    const Request rq = p.request(c.src, c.bits);
    EXPECT(check_request(&prm, rq, 66, nullptr, c.path_begin) == MCP_OK);
    const mcp::PathKernel k = route_kernel(&prm, rq, c.attr_walk, c.path_begin, 66);
    const Row* row = select_row(c.N == 16 ? 4 : 5, k);
    EXPECT(row && strcmp(row->kernel, c.kernel) == 0 && ((k.flags & mcp::PK_KT8) != 0) == (c.K > 1 && !(c.bits & B_BAND) && !c.attr_walk));
  }
}

// SPEC.md 5.22: mcp_downside_finish on hand-made records -- the three cases of downside_std, the empty sets, a constant sample -- the
// request's rules, and the arm / disarm rule: armed, a failing call (which takes the request), then a plain call finds nothing.
static void run_downside() {
  snprintf(g_case, sizeof g_case, "downside finish");
  mcp_downside_stats o;
  // x = {-2, -1, 1, 4} about c = 0 at tau = 0: d = e
  const mcp_downside_sums four = {4, 2, 2, 2.0, 22.0, 56.0, 274.0, -3.0, 5.0, -3.0, 5.0, 5.0};
  EXPECT(mcp_downside_finish(&four, 0.0, 0.0, &o) == MCP_OK);
  EXPECT(o.mean == 0.5 && o.p_below == 0.5 && o.mean_shortfall == -1.5 && o.omega == 5.0 / 3.0);
  EXPECT(o.downside_std == std::sqrt(0.5) && o.sortino == 0.5 / std::sqrt(0.5) && o.downside_deviation == std::sqrt(1.25));
  EXPECT(o.sortino_target == 0.5 / std::sqrt(1.25) && std::isfinite(o.skewness) && std::isfinite(o.excess_kurtosis));
  EXPECT(mcp_downside_finish(&four, 0.0, 10.0, &o) == MCP_OK && o.mean == 10.5);     // the pivot moves the mean alone
  const mcp_downside_sums one_below = {2, 1, 1, 0.0, 2.0, 0.0, 2.0, -1.0, 1.0, -1.0, 1.0, 1.0};   // x = {-1, 1}
  EXPECT(mcp_downside_finish(&one_below, 0.0, 0.0, &o) == MCP_OK && std::isnan(o.downside_std) && std::isnan(o.sortino) && o.omega == 1.0);
  EXPECT(o.skewness == 0.0 && o.excess_kurtosis == -2.0);
  const mcp_downside_sums none_below = {2, 0, 2, 3.0, 5.0, 9.0, 17.0, 0.0, 0.0, 0.0, 0.0, 3.0};  // x = {1, 2}
  EXPECT(mcp_downside_finish(&none_below, 0.0, 0.0, &o) == MCP_OK && o.downside_std == 1e-4 && o.sortino == 1.5 / 1e-4);
  EXPECT(o.omega == HUGE_VAL && o.mean_shortfall == 0.0 && o.sortino_target == 0.0 && o.p_below == 0.0 && o.downside_deviation == 0.0);
  const mcp_downside_sums constant = {3, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // x = tau = c three times: neither set
  EXPECT(mcp_downside_finish(&constant, 0.25, 0.25, &o) == MCP_OK && o.skewness == 0.0 && o.excess_kurtosis == 0.0 && o.mean == 0.25);
  EXPECT(o.sortino == 0.0 && o.omega == HUGE_VAL && o.p_below == 0.0);
  const mcp_downside_sums empty = {};
  EXPECT(mcp_downside_finish(&empty, 0.0, 0.5, &o) == MCP_OK && o.mean == 0.5 && o.p_below == 0.0 && o.downside_deviation == 0.0);
  EXPECT(mcp_downside_finish(nullptr, 0.0, 0.0, &o) == MCP_E_ARG && mcp_downside_finish(&four, 0.0, 0.0, nullptr) == MCP_E_ARG);

  snprintf(g_case, sizeof g_case, "downside request");
  mcp_downside req = {0.01, 0, 0};
  EXPECT(check_downside(&req, &o) == MCP_OK);
  EXPECT(check_downside(nullptr, &o) == MCP_E_ARG && check_downside(&req, nullptr) == MCP_E_ARG);
  req.reserved = 1;
  EXPECT(check_downside(&req, &o) == MCP_E_ARG);
  req.reserved = 0;
  for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
    req.tau = bad;
    EXPECT(check_downside(&req, &o) == MCP_E_ARG);
  }
  req.tau = 0.01;
  req.use_rf = 1;

  snprintf(g_case, sizeof g_case, "downside arm / disarm");
  DownsideArm arm;
  mcp_downside_sums sums;
  mcp_downside_stats hz;
  EXPECT(!arm.on && !arm.take().on);
  arm.arm(req, &sums, &o, &hz);
  EXPECT(arm.on && arm.use_rf && arm.tau == 0.01 && arm.sums_out == &sums && arm.stats_out == &o && arm.hz_stats_out == &hz);
  const DownsideArm failing = arm.take();                  // the call that takes it may fail: the request is spent either way
  EXPECT(failing.on && failing.stats_out == &o && !arm.on && !arm.stats_out && !arm.sums_out && !arm.hz_stats_out);
  const DownsideArm plain = arm.take();                    // the plain call after it: nothing to write to
  EXPECT(!plain.on && !plain.stats_out && !plain.sums_out && !plain.hz_stats_out);
  req.use_rf = 0;
  arm.arm(req, nullptr, &o, nullptr);
  arm.arm(req, &sums, &o, nullptr);                        // a second request replaces the first
  EXPECT(arm.take().sums_out == &sums && !arm.on);

  mcp_downside_sums a = four;
  rowsum_add(a, one_below);
  EXPECT(a.n == 6 && a.n_below == 3 && a.n_above == 3 && a.s2 == 24.0 && a.b1 == -4.0 && a.l2 == 6.0 && a.u1 == 6.0 && a.s4 == 276.0);
}

int main() {
  run_downside();
  const int Ns[3] = {1, 5, MCP_MAX_ASSETS}, Ks[4] = {1, 8, 9, 17}, Hs[2] = {0, 2};
  int n = 0;
  for (int N : Ns)
    for (int K : Ks)
      for (int H : Hs) { run_shape(N, K, 12, H); n++; }
  run_plans();
  run_named_routes();
  const long n_routed = run_routes();
  printf("host_selftest ok: %d shapes x %d requests, the plans, the routes of %ld requests\n", n, (int)N_FEATURES, n_routed);
  return 0;
}

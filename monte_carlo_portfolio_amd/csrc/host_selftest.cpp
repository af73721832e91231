// host_selftest.cpp -- drives mcp_host.cpp on heap buffers of exactly the documented lengths, for `make host-selftest`: built
// with a plain C++ compiler under AddressSanitizer + UBSan, so an overrun of a packer or a pivot rule is a sanitizer report.  It
// asserts return codes and finiteness only; the values are pinned bit for bit by the CPU tests against their NumPy restatements.
// The plan of a call (second_of, counted_of, tile_bytes_per_path, plan_tiles) has no other CPU test: it is asserted in full here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

enum Feature { PLAIN, BOOT, FILTERED, JUMPS, REGIMES, GLIDE_CF, GLIDE, PROTECT, CASH, OVERLAY, SPEND, SPEND_BOOT, BAND, BAND_BOOT, N_FEATURES };
static const char* const k_names[N_FEATURES] = {"plain", "bootstrap", "filtered", "jumps", "regimes", "glide+flows", "glide",
                                                "protect", "cash", "overlay", "spend", "spend+bootstrap", "band", "band+bootstrap"};

static void run_shape(int N, int K, int T, int H) {
  const int R = 6, G = 2;
  const int32_t steps_v[2] = {1, T}, breaks_v[G] = {3, 7};
  const std::vector<int32_t> steps(steps_v, steps_v + H), breaks(breaks_v, breaks_v + G);
  std::vector<float> mu(N), mu1(N), chol((size_t)N * N, 0.0f), chol1((size_t)N * N, 0.0f), W((size_t)K * N), rows((size_t)R * N), shock(R),
      loading(N), targets((size_t)G * K * N), flows(T, -0.01f), zero_flows(T, 0.0f), floor_s(T + 1), spot(N, 100.0f);
  for (int i = 0; i < N; i++) {
    mu[i] = 0.001f * (float)(i + 1) / (float)N;
    mu1[i] = -2.0f * mu[i];
    loading[i] = 0.5f + 0.5f * (float)(i & 1);
    for (int j = 0; j <= i; j++) chol[(size_t)i * N + j] = i == j ? 0.01f : 0.001f;
    for (int j = 0; j <= i; j++) chol1[(size_t)i * N + j] = 3.0f * chol[(size_t)i * N + j];
  }
  for (size_t i = 0; i < W.size(); i++) W[i] = (1.0f + 0.1f * (float)(i % 3)) / (float)N;
  for (size_t i = 0; i < targets.size(); i++) targets[i] = (1.0f + 0.1f * (float)(i % 5)) / (float)N;
  for (size_t i = 0; i < rows.size(); i++) rows[i] = 0.002f * (float)((int)(i % 7) - 3);
  for (int j = 0; j < R; j++) shock[j] = 0.5f + 0.25f * (float)j;
  EXPECT(mcp_protect_floor(0.8, 0.001, T, floor_s.data()) == MCP_OK && finite(floor_s));
  std::vector<int32_t> row_begin(N + 1, 1);
  row_begin[0] = 0;
  const std::vector<mcp_overlay_row> ov_rows(1, mcp_overlay_row{MCP_OVERLAY_PUT, 95.0f, 1.0f, 0.01f});

  mcp_params prm = {N, T, K, MCP_COMPOUND_SIMPLE, 0, 0, 1.0, 0.95, 0.0};
  const mcp_bootstrap boot = {rows.data(), R, 0, 3.0};
  const mcp_filtered filt = {mu.data(), rows.data(), shock.data(), R, 0, 2.0};
  const mcp_garch gv = {0.05, 0.9, 1.0, 0};
  const mcp_jumps jp = {0.1, -0.05, 0.02, (N & 1) ? loading.data() : nullptr, 0};
  const mcp_regimes rs = {0.05, 0.2, 0.1, mu1.data(), chol1.data(), 0};
  const mcp_glide gl = {breaks.data(), targets.data(), G, 0};
  const mcp_cashflow cf = {flows.data(), T, 1, 1.0}, no_cf = {zero_flows.data(), T, 0, 0.0};
  const mcp_protect pt = {floor_s.data(), 3.0, 1.0, 0.001, 0.1, nullptr, 0};
  const mcp_overlay ov = {ov_rows.data(), row_begin.data(), spot.data(), 1, 0};
  const mcp_rebalance reb = {5, 0, 0.001};
  std::vector<float> tol((size_t)K * N, 0.05f);          // SPEC.md 4.18: bands, the last asset of every portfolio not watched
  for (int k = 0; k < K; k++) tol[(size_t)k * N + N - 1] = HUGE_VALF;
  const mcp_band bd = {5, 0, 0.001, tol.data()};
  const mcp_rebalance bd_reb = {bd.every, 0, bd.cost};
  const mcp_spending sp = {0.01, 0.1, HUGE_VAL, 0.02, 0.015, 0.9, 5, 1, 1, 0};
  const int32_t* hs = H ? steps.data() : nullptr;

  // every pure entry point, outputs of exactly the documented length
  snprintf(g_case, sizeof g_case, "entry points, N=%d K=%d T=%d H=%d", N, K, T, H);
  std::vector<double> pv(K), hz((size_t)H * K), p3(3), mean_count(1);
  std::vector<float> packed(mcp_packed_len(N, K)), drift(N);
  std::vector<uint64_t> thr3(3), rank(2);
  std::vector<uint32_t> jthr(MCP_MAX_JUMPS);
  double* hzp = H ? hz.data() : nullptr;
  EXPECT(mcp_abi_version() == MCP_ABI_VERSION && !packed.empty());
  EXPECT(mcp_pack_params(N, K, mu.data(), chol.data(), W.data(), packed.data(), packed.size()) == MCP_OK && finite(packed));
  EXPECT(mcp_pivots(&prm, mu.data(), chol.data(), W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_rebalance_pivots(&prm, &reb, mu.data(), nullptr, W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_rebalance_pivots(&prm, &reb, nullptr, &boot, W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_bootstrap_pivots(&prm, &boot, W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_filtered_pivots(&prm, &filt, W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_cashflow_pivots(&prm, &cf, mu.data(), nullptr, W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_overlay_pivots(&prm, &ov, mu.data(), W.data(), pv.data()) == MCP_OK && finite(pv));
  EXPECT(mcp_regime_pivots(&prm, &rs, mu.data(), W.data(), H, hs, pv.data(), hzp) == MCP_OK && finite(pv) && finite(hz));
  EXPECT(mcp_glide_pivots(&prm, &gl, &cf, mu.data(), nullptr, W.data(), H, hs, pv.data(), hzp) == MCP_OK && finite(pv) && finite(hz));
  EXPECT(mcp_protect_pivots(&prm, &pt, mu.data(), W.data(), H, hs, pv.data(), hzp) == MCP_OK && finite(pv) && finite(hz));
  std::vector<double> wdp(K);
  std::vector<float> c5(5);
  EXPECT(mcp_spending_pivots(&prm, &sp, mu.data(), nullptr, W.data(), H, hs, pv.data(), hzp, wdp.data()) == MCP_OK && finite(pv) && finite(hz) && finite(wdp));
  EXPECT(mcp_spending_pivots(&prm, &sp, nullptr, &boot, W.data(), H, hs, pv.data(), hzp, wdp.data()) == MCP_OK && finite(pv) && finite(hz) && finite(wdp));
  EXPECT(mcp_spending_consts(&sp, prm.v0, c5.data()) == MCP_OK && std::isinf(c5[3]) && c5[4] == 0.015f);
  {                                       // SPEC.md 5.17 on an exactly sized histogram: T + 1 bins, one level per quartile
    std::vector<uint64_t> lh((size_t)T + 1, 1);
    std::vector<double> lq = {0.0, 25.0, 50.0, 100.0};
    std::vector<uint32_t> got(lq.size());
    uint64_t total = 0;
    EXPECT(mcp_lifetime_summary(lh.data(), T, (int)lq.size(), lq.data(), &total, got.data()) == MCP_OK && total == (uint64_t)T * (T + 1) / 2 &&
           got[0] == 0 && got[1] == (uint32_t)(T / 4) && got[2] == (uint32_t)(T / 2) && got[3] == (uint32_t)T);
    EXPECT(mcp_lifetime_summary(lh.data(), T, 0, nullptr, &total, nullptr) == MCP_OK);
  }
  EXPECT(mcp_band_reviews(&prm, &bd) == (T - 1) / 5 && mcp_band_reviews(&prm, nullptr) == -1);
  EXPECT(mcp_regime_consts(&rs, thr3.data(), p3.data()) == MCP_OK && finite(p3));
  EXPECT(mcp_jump_consts(&jp, N, mu.data(), jthr.data(), mean_count.data(), drift.data()) == MCP_OK && finite(mean_count) && finite(drift));
  EXPECT(mcp_percentile_rank(1000, 0.95, &rank[0], &rank[1], p3.data()) == MCP_OK && rank[1] == rank[0] + 1 && finite(p3));
  EXPECT(mcp_percentile_rank_q(1000, 2.5, &rank[0], &rank[1], p3.data()) == MCP_OK && rank[1] == rank[0] + 1 && finite(p3));

  // every feature: the request's rules, then the block and the pivots of every tile on exactly sized buffers
  std::vector<mcp_stats> stats(K), hz_stats((size_t)H * K);
  std::vector<uint64_t> counts(2 * (size_t)K), hz_counts(2 * (size_t)H * K);
  for (int f = 0; f < N_FEATURES; f++) {
    snprintf(g_case, sizeof g_case, "%s, N=%d K=%d T=%d H=%d", k_names[f], N, K, T, H);
    const Source src = f == BOOT || f == SPEND_BOOT || f == BAND_BOOT ? SRC_BOOT : f == FILTERED ? SRC_FHS : SRC_GAUSS;
    const bool rows_only = src != SRC_GAUSS;
    Request rq = host_request(src, rows_only ? nullptr : mu.data(), rows_only ? nullptr : chol.data(), W.data(), nullptr, stats.data());
    ask_horizons(rq, H != 0, H, hs, 0, nullptr, nullptr, H ? hz_stats.data() : nullptr, nullptr);
    if (f == BOOT || f == SPEND_BOOT || f == BAND_BOOT) rq.boot = &boot;
    std::vector<uint64_t> trade_hist((size_t)K * ((size_t)(T - 1) / 5 + 1));
    if (f == BAND || f == BAND_BOOT) {
      rq.rebalanced = rq.band = true; rq.reb = &bd_reb; rq.bd = &bd;
      rq.trade_hist_out = trade_hist.data(); rq.turnover_stats_out = stats.data();
    }
    if (f == FILTERED) { rq.filt = &filt; rq.gv = &gv; }
    if (f == JUMPS) { rq.jumps = true; rq.jp = &jp; }
    if (f == REGIMES) { rq.regimes = true; rq.rs = &rs; }
    if (f == GLIDE || f == GLIDE_CF) { rq.glide = true; rq.gl = &gl; }
    if (f == GLIDE || f == GLIDE_CF || f == CASH) { rq.cash = true; rq.cf = f == GLIDE ? &no_cf : &cf; }
    if (f == PROTECT) { rq.protect = true; rq.pi = &pt; }
    if (f == SPEND || f == SPEND_BOOT) { rq.cash = rq.spend = true; rq.cf = &no_cf; rq.sp = &sp; rq.wd_stats_out = stats.data(); }
    if (f == OVERLAY) { rq.overlay = true; rq.ov = &ov; }
    if (rq.cash || rq.protect) { rq.counts_out = counts.data(); rq.hz_counts_out = H ? hz_counts.data() : nullptr; }
    std::vector<float> second((size_t)K * 4);                // [K][4 paths] the optional per-path outputs
    std::vector<uint32_t> record((size_t)K * 4);
    std::vector<mcp_stats> second_stats(K);
    if (rq.band) { rq.turnover_out = second.data(); rq.turnover_stats_out = second_stats.data(); rq.trades_out = record.data(); }
    if (rq.spend) { rq.wd_out = second.data(); rq.wd_stats_out = second_stats.data(); }
    EXPECT(check_request(&prm, rq, 4) == MCP_OK);
    {                                     // the one second array and the one integer record of the request, on the request's own outputs
      const Second sec = second_of(rq);
      const Counted cnt = counted_of(&prm, rq);
      EXPECT(sec.on == (rq.band || rq.spend) && cnt.on == rq.band && cnt.bins == count_bins(&prm, rq));
      EXPECT(sec.out == (sec.on ? second.data() : nullptr) && sec.stats_out == (sec.on ? second_stats.data() : nullptr));
      EXPECT(cnt.out == (cnt.on ? record.data() : nullptr) && cnt.hist_out == (cnt.on ? trade_hist.data() : nullptr));
      if (rq.band) EXPECT(sec.unit_v0 && !sec.pivoted);   // SPEC.md 5.18: x = Y - 1, no pivot
      if (rq.spend) EXPECT(!sec.unit_v0 && sec.pivoted);  // SPEC.md 5.16: x = Y / fl32(v0) - 1, the pivots of request_wd_pivots
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
      EXPECT(check_request(&prm, lr, 4) == (rq.cash ? MCP_OK : MCP_E_UNSUPPORTED));
      lr.life_hist_out = nullptr;
      EXPECT(check_request(&prm, lr, 4) == (rq.cash ? MCP_E_ARG : MCP_E_UNSUPPORTED));
    }
    if (rq.band) {                        // SPEC.md 4.18: a negative entry, a missing histogram, and the size of the histogram
      Request br = rq;
      std::vector<float> neg(tol);
      neg.back() = -0.01f;
      const mcp_band bad_bd = {5, 0, 0.001, neg.data()};
      br.bd = &bad_bd;
      EXPECT(check_request(&prm, br, 4) == MCP_E_ARG);
      br = rq;
      br.trade_hist_out = nullptr;
      EXPECT(check_request(&prm, br, 4) == MCP_E_ARG);
      EXPECT(count_bins(&prm, rq) * (size_t)K == trade_hist.size());
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
    mcp_bootstrap bad_boot = boot;
    if (f == PLAIN) bad.flags = MCP_FLAG_FOLD | MCP_FLAG_NATIVE_MATH;      // the folded step needs the spec's normals
    else if (f == BOOT) { bad_boot.mean_block = 0.5; rq.boot = &bad_boot; }  // the bootstrap compounds either way; b < 1 does not
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
    Request dd = rq, spend = rq, life = rq, spend_life = rq, band = rq;
    dd.dd = true;
    spend.cash = spend.spend = true;
    life.cash = life.life = true;
    spend_life.cash = spend_life.spend = spend_life.life = true;
    band.rebalanced = band.band = true;
    EXPECT(tile_bytes_per_path(rq) == 4 + hz && tile_bytes_per_path(spend) == 8 + hz && tile_bytes_per_path(life) == 8 + hz);
    EXPECT(tile_bytes_per_path(spend_life) == 12 + hz && tile_bytes_per_path(band) == 16 + hz);
    if (!H) EXPECT(tile_bytes_per_path(dd) == 8);            // the drawdown and horizons are never asked together
  }
}

int main() {
  const int Ns[3] = {1, 5, MCP_MAX_ASSETS}, Ks[4] = {1, 8, 9, 17}, Hs[2] = {0, 2};
  int n = 0;
  for (int N : Ns)
    for (int K : Ks)
      for (int H : Hs) { run_shape(N, K, 12, H); n++; }
  run_plans();
  printf("host_selftest ok: %d shapes x %d requests, the plans\n", n, (int)N_FEATURES);
  return 0;
}

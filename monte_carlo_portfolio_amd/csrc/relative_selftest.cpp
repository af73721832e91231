// relative_selftest.cpp -- the pure-host side of SPEC.md 5.23 for `make relative-selftest`: built with mcp_host.cpp by a plain C++
// compiler under AddressSanitizer + UBSan, no device.  mcp_relative_finish on hand-made records whose every figure is a dyadic
// rational (so == is the right comparison), every zero denominator and the benchmark's own row; the request's rules; arm / take /
// disarm; the one-tile rule against plan_tiles; what the request adds to the bytes the tile budget counts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mcp_host.h"

using namespace mcph;

static char g_case[96] = "";
#define EXPECT(cond)                                                                                               \
  do {                                                                                                             \
    if (!(cond)) {                                                                                                 \
      fprintf(stderr, "relative_selftest:%d: %s  [%s; last error: %s]\n", __LINE__, #cond, g_case, mcp_last_error()); \
      exit(1);                                                                                                     \
    }                                                                                                              \
  } while (0)

static void run_finish() {
  snprintf(g_case, sizeof g_case, "relative finish");
  mcp_relative_stats o;
  // x_k = {1/2, -1/4, 3/4, 0} against x_b = {1/4, -1/8, 3/4, -1/2} about c = 0: a = e = {1/4, -1/8, 0, 1/2}
  const mcp_relative_sums four = {4, 1, 2, 2, 2, 0.625, 0.328125, 1.0, 0.375, 0.875, 0.890625, 0.71875, -0.125, 0.015625, 1.25, 1.0, -0.25, -0.625};
  EXPECT(mcp_relative_finish(&four, 0.0, 0.0, &o) == MCP_OK);
  const double te = std::sqrt(0.23046875 / 3.0), beta = 0.625 / 0.85546875;
  EXPECT(o.active_mean == 0.15625 && o.tracking_error == te && o.information_ratio == 0.15625 / te);
  EXPECT(o.p_under == 0.25 && o.p_over == 0.5 && o.mean_underperformance == -0.125 && o.relative_downside_deviation == 0.0625);
  EXPECT(o.beta == beta && o.alpha == 0.25 - beta * 0.09375 && o.correlation == 0.625 / std::sqrt(0.625 * 0.85546875));
  EXPECT(o.up_capture == 1.25 && o.down_capture == 0.4 && o.pivot == 0.0 && o.bench_pivot == 0.0);
  // the pivots move the means alone: c_k = 1/2, c_b = 1/4
  EXPECT(mcp_relative_finish(&four, 0.5, 0.25, &o) == MCP_OK && o.active_mean == 0.40625 && o.tracking_error == te && o.beta == beta);
  EXPECT(o.alpha == 0.75 - beta * 0.34375 && o.pivot == 0.5 && o.bench_pivot == 0.25);

  // the benchmark's own row: d_k = d_b, e = a = 0 on every path
  const mcp_relative_sums own = {4, 0, 0, 2, 2, 0.0, 0.0, 0.375, 0.375, 0.890625, 0.890625, 0.890625, 0.0, 0.0, 1.0, 1.0, -0.625, -0.625};
  EXPECT(mcp_relative_finish(&own, 0.25, 0.25, &o) == MCP_OK);
  EXPECT(o.active_mean == 0.0 && o.tracking_error == 0.0 && o.information_ratio == 0.0 && o.p_under == 0.0 && o.p_over == 0.0);
  EXPECT(o.beta == 1.0 && o.correlation == 1.0 && o.alpha == 0.0 && o.up_capture == 1.0 && o.down_capture == 1.0);
  EXPECT(o.mean_underperformance == 0.0 && o.relative_downside_deviation == 0.0);

  // a benchmark that does not move, x_b = c_b = 1/4 twice, x_k = {1/2, 0}: var(x_b) = 0, no path with x_b < 0
  const mcp_relative_sums flat = {2, 1, 1, 2, 0, 0.0, 0.125, 0.0, 0.0, 0.125, 0.0, 0.0, -0.25, 0.0625, 0.5, 0.5, 0.0, 0.0};
  EXPECT(mcp_relative_finish(&flat, 0.25, 0.25, &o) == MCP_OK);
  EXPECT(o.beta == 0.0 && o.correlation == 0.0 && o.alpha == 0.25 && o.down_capture == 0.0 && o.up_capture == 1.0);
  EXPECT(o.tracking_error == std::sqrt(0.125) && o.p_under == 0.5 && o.mean_underperformance == -0.25);
  // its own row: correlation 0 where var(x_b) is 0, beta 0 by the same rule
  const mcp_relative_sums flat_own = {2, 0, 0, 2, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.5, 0.0, 0.0};
  EXPECT(mcp_relative_finish(&flat_own, 0.25, 0.25, &o) == MCP_OK && o.correlation == 0.0 && o.tracking_error == 0.0 && o.up_capture == 1.0);

  // one path: no sample deviation; nobody behind; no path with x_b > 0
  const mcp_relative_sums one = {1, 0, 1, 0, 1, 0.5, 0.25, 0.25, -0.25, 0.0625, 0.0625, -0.0625, 0.0, 0.0, 0.0, 0.0, 0.25, -0.25};
  EXPECT(mcp_relative_finish(&one, 0.0, 0.0, &o) == MCP_OK && o.tracking_error == 0.0 && o.information_ratio == 0.0 && o.active_mean == 0.5);
  EXPECT(o.mean_underperformance == 0.0 && o.up_capture == 0.0 && o.down_capture == -1.0 && o.beta == 0.0 && o.correlation == 0.0);
  EXPECT(o.p_over == 1.0 && o.p_under == 0.0);

  const mcp_relative_sums empty = {};
  EXPECT(mcp_relative_finish(&empty, 0.5, 0.25, &o) == MCP_OK && o.active_mean == 0.25 && o.tracking_error == 0.0 && o.p_under == 0.0);
  EXPECT(o.p_over == 0.0 && o.relative_downside_deviation == 0.0 && o.beta == 0.0 && o.alpha == 0.5 && o.correlation == 0.0);
  EXPECT(o.up_capture == 0.0 && o.down_capture == 0.0 && o.mean_underperformance == 0.0 && o.information_ratio == 0.0);
  EXPECT(mcp_relative_finish(nullptr, 0.0, 0.0, &o) == MCP_E_ARG && mcp_relative_finish(&four, 0.0, 0.0, nullptr) == MCP_E_ARG);

  mcp_relative_sums a = four;
  rowsum_add(a, one);
  EXPECT(a.n == 5 && a.n_under == 1 && a.n_over == 3 && a.n_up == 2 && a.n_down == 3 && a.e1 == 1.125 && a.e2 == 0.578125);
  EXPECT(a.k1 == 1.25 && a.b1 == 0.125 && a.k2 == 0.9375 && a.b2 == 0.953125 && a.kb == 0.65625 && a.u1 == -0.125 && a.u2 == 0.015625);
  EXPECT(a.up_k == 1.25 && a.up_b == 1.0 && a.down_k == 0.0 && a.down_b == -0.875);
}

static void run_request() {
  snprintf(g_case, sizeof g_case, "relative request");
  mcp_relative_stats o, hz;
  mcp_relative req = {2, 0};
  EXPECT(check_relative(&req, &o) == MCP_OK);
  EXPECT(check_relative(nullptr, &o) == MCP_E_ARG && check_relative(&req, nullptr) == MCP_E_ARG);
  req.reserved = 1;
  EXPECT(check_relative(&req, &o) == MCP_E_ARG);
  req.reserved = 0;
  req.bench = -1;
  EXPECT(check_relative(&req, &o) == MCP_E_ARG);
  req.bench = 0;
  EXPECT(check_relative(&req, &o) == MCP_OK);
  req.bench = 2;

  snprintf(g_case, sizeof g_case, "relative arm / disarm");
  RelativeArm arm;
  mcp_relative_sums sums;
  mcp_stats as;
  float y;
  EXPECT(!arm.on && !arm.take().on);
  arm.arm(req, &sums, &o, &as, &y, &hz);
  EXPECT(arm.on && arm.bench == 2 && arm.sums_out == &sums && arm.stats_out == &o && arm.active_stats_out == &as && arm.active_out == &y &&
         arm.hz_stats_out == &hz);
  const RelativeArm failing = arm.take();                  // the call that takes it may fail: the request is spent either way
  EXPECT(failing.on && failing.stats_out == &o && failing.bench == 2 && !arm.on && !arm.stats_out && !arm.sums_out && !arm.hz_stats_out);
  EXPECT(!arm.active_stats_out && !arm.active_out && arm.bench == 0);
  const RelativeArm plain = arm.take();                    // the plain call after it: nothing to write to
  EXPECT(!plain.on && !plain.stats_out && !plain.sums_out && !plain.active_out);
  arm.arm(req, nullptr, &o, nullptr, nullptr, nullptr);
  req.bench = 1;
  arm.arm(req, &sums, &o, nullptr, nullptr, nullptr);      // a second request replaces the first
  const RelativeArm second = arm.take();
  EXPECT(second.sums_out == &sums && second.bench == 1 && !arm.on);
  // a downside request beside it is another arm: taking one leaves the other
  DownsideArm ds;
  mcp_downside_stats dso;
  const mcp_downside dreq = {0.0, 0, 0};
  ds.arm(dreq, nullptr, &dso, nullptr);
  arm.arm(req, nullptr, &o, nullptr, nullptr, nullptr);
  EXPECT(arm.take().on && ds.on && ds.take().on && !arm.on);
}

static void run_plan() {
  snprintf(g_case, sizeof g_case, "relative bytes per path");
  Request rq;
  const size_t base = tile_bytes_per_path(rq);
  EXPECT(base == 4);
  rq.rl.on = true;
  EXPECT(tile_bytes_per_path(rq) == base + 4);
  rq.hz = true;
  rq.H = 2;
  EXPECT(tile_bytes_per_path(rq) == 16);                   // V_T, two horizon rows, Y: no Y at the horizons
  rq.dd = true;
  EXPECT(tile_bytes_per_path(rq) == 20);                   // the second array and Y are two arrays
  rq.rl.on = false;
  EXPECT(tile_bytes_per_path(rq) == 16);
  rq.ds.on = true;                                      // the downside request stores nothing per path
  EXPECT(tile_bytes_per_path(rq) == 16);

  snprintf(g_case, sizeof g_case, "relative one-tile rule");
  const int K = 5;
  const uint64_t n = 1000;
  const size_t bpp = 8;
  const TilePlan whole = plan_tiles(1, K, n, false, 1, (size_t)K * n * bpp, bpp);
  EXPECT(whole.tiles() == 1 && check_relative_plan(whole, K, false) == MCP_OK);
  const TilePlan cut = plan_tiles(1, K, n, false, 1, (size_t)K * n * bpp - 1, bpp);            // one byte short: 4 portfolios per tile
  EXPECT(cut.tiles() == 2 && check_relative_plan(cut, K, false) == MCP_E_ARG && strstr(mcp_last_error(), "raise the budget or shard by paths"));
  const TilePlan paths2 = plan_tiles(2, K, n, false, 1, (size_t)K * n * bpp, bpp);             // path shards: all K rows on both
  EXPECT(paths2.tiles() == 1 && check_relative_plan(paths2, K, false) == MCP_OK);
  const TilePlan paths2_cut = plan_tiles(2, K, n, false, 1, (size_t)2 * (n / 2) * bpp, bpp);
  EXPECT(paths2_cut.tiles() == 3 && check_relative_plan(paths2_cut, K, false) == MCP_E_ARG);
  const TilePlan ports2 = plan_tiles(2, K, n, true, 1, (size_t)K * n * bpp, bpp);              // portfolio shards: the rows are split
  EXPECT(check_relative_plan(ports2, K, true) == MCP_E_ARG && strstr(mcp_last_error(), "shard by paths"));
  const TilePlan anti = plan_tiles(3, K, n, false, 2, (size_t)K * n * bpp, bpp);               // antithetic pairs: members are paths
  EXPECT(check_relative_plan(anti, K, false) == MCP_OK);
}

int main() {
  run_finish();
  run_request();
  run_plan();
  printf("relative_selftest ok\n");
  return 0;
}

// sweep_perf_selftest.cpp -- the pure-host side of SPEC.md 5.24 for `make sweep-perf-selftest`: built with mcp_host.cpp by a plain
// C++ compiler under AddressSanitizer + UBSan, no device.  mcp_sweep_perf_finish on hand-made records whose every figure is a dyadic
// rational (so == is the right comparison) through every branch of the finish -- n_neg 0, 1 and 2, a zero std, a zero downside_std,
// a zero and a NaN drawdown -- and the rules of mcp_sweep_historical_perf on exactly sized heap arrays.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "mcp_host.h"

using namespace mcph;

static char g_case[96] = "";
#define EXPECT(cond)                                                                                                 \
  do {                                                                                                               \
    if (!(cond)) {                                                                                                   \
      fprintf(stderr, "sweep_perf_selftest:%d: %s  [%s; last error: %s]\n", __LINE__, #cond, g_case, mcp_last_error()); \
      exit(1);                                                                                                       \
    }                                                                                                                \
  } while (0)

static void run_finish() {
  snprintf(g_case, sizeof g_case, "sweep perf finish");
  mcp_sweep_perf_stats o;
  // n = 4 at ann_factor 4: mean_excess 1/4, std sqrt(3/4 / 3) = 1/2, downside_std sqrt(1/16 / 1) = 1/4, pow(3/2, 1) - 1 = 1/2
  const mcp_sweep_perf_sums two = {4, 2, 1, 3, 1.0, -0.75, 0.75, 0.0625, 1.5, -0.25};
  EXPECT(mcp_sweep_perf_finish(&two, 4.0, &o) == MCP_OK);
  EXPECT(o.sharpe_ratio == 1.0 && o.sortino_ratio == 2.0 && o.annual_volatility == 1.0 && o.annual_return == 0.5);
  EXPECT(o.max_drawdown == -0.25 && o.calmar == 2.0 && o.peak_row == 1 && o.trough_row == 3);
  // ann_factor 16 over the same record: sqrt(16) = 4, pow(3/2, 4) - 1 = 65/16
  EXPECT(mcp_sweep_perf_finish(&two, 16.0, &o) == MCP_OK);
  EXPECT(o.sharpe_ratio == 2.0 && o.sortino_ratio == 4.0 && o.annual_volatility == 2.0);
  EXPECT(std::fabs(o.annual_return - 4.0625) <= 1e-12 * 4.0625 && std::fabs(o.calmar - 16.25) <= 1e-12 * 16.25);

  // no negative excess return: the reference's 1e-4
  const mcp_sweep_perf_sums none = {4, 0, 0, 0, 1.0, 0.0, 0.75, 0.0, 1.5, 0.0};
  EXPECT(mcp_sweep_perf_finish(&none, 4.0, &o) == MCP_OK);
  EXPECT(o.sortino_ratio == 0.25 / 1e-4 * 2.0 && o.sharpe_ratio == 1.0);
  EXPECT(o.max_drawdown == 0.0 && o.calmar == 0.0 && o.annual_return == 0.5);       // a zero drawdown: Calmar 0, not a division

  // exactly one: np.std of one value at ddof 1 is 0 / 0
  const mcp_sweep_perf_sums one = {4, 1, 0, 1, 1.0, -0.25, 0.75, 0.0, 1.5, -0.5};
  EXPECT(mcp_sweep_perf_finish(&one, 4.0, &o) == MCP_OK);
  EXPECT(std::isnan(o.sortino_ratio) && o.sharpe_ratio == 1.0 && o.calmar == 1.0);

  // a zero std: Sharpe 0 by the reference's test, volatility 0; a zero downside_std divides by IEEE rules
  const mcp_sweep_perf_sums flat = {4, 4, 0, 3, -1.0, -1.0, 0.0, 0.0, 0.5, -0.5};
  EXPECT(mcp_sweep_perf_finish(&flat, 4.0, &o) == MCP_OK);
  EXPECT(o.sharpe_ratio == 0.0 && o.annual_volatility == 0.0 && o.sortino_ratio == -std::numeric_limits<double>::infinity());
  EXPECT(o.annual_return == -0.5 && o.calmar == -1.0);
  const mcp_sweep_perf_sums flat_up = {4, 2, 0, 3, 1.0, -0.5, 0.75, 0.0, 1.5, -0.5};
  EXPECT(mcp_sweep_perf_finish(&flat_up, 4.0, &o) == MCP_OK && o.sortino_ratio == std::numeric_limits<double>::infinity());
  const mcp_sweep_perf_sums flat_zero = {4, 2, 0, 3, 0.0, -0.5, 0.75, 0.0, 1.5, -0.5};
  EXPECT(mcp_sweep_perf_finish(&flat_zero, 4.0, &o) == MCP_OK && std::isnan(o.sortino_ratio) && o.sharpe_ratio == 0.0);

  // a NaN drawdown (wealth 0 at the first row): it propagates to Calmar, the rows are -1
  const mcp_sweep_perf_sums lost = {4, 1, -1, -1, -0.5, -1.0, 0.75, 0.0, 0.0, std::nan("")};
  EXPECT(mcp_sweep_perf_finish(&lost, 4.0, &o) == MCP_OK);
  EXPECT(std::isnan(o.max_drawdown) && std::isnan(o.calmar) && o.annual_return == -1.0 && o.peak_row == -1 && o.trough_row == -1);

  snprintf(g_case, sizeof g_case, "sweep perf finish rules");
  EXPECT(mcp_sweep_perf_finish(nullptr, 4.0, &o) == MCP_E_ARG && mcp_sweep_perf_finish(&two, 4.0, nullptr) == MCP_E_ARG);
  EXPECT(mcp_sweep_perf_finish(&two, 0.0, &o) == MCP_E_ARG && mcp_sweep_perf_finish(&two, -1.0, &o) == MCP_E_ARG);
  EXPECT(mcp_sweep_perf_finish(&two, std::nan(""), &o) == MCP_E_ARG && mcp_sweep_perf_finish(&two, HUGE_VAL, &o) == MCP_E_ARG);
}

static void run_rules() {
  snprintf(g_case, sizeof g_case, "sweep perf rules");
  const int N = 3, R = 5, P = 4;
  std::vector<double> ret((size_t)R * N, 0.01), W((size_t)P * N, 0.25);
  std::vector<mcp_sweep_perf_stats> out((size_t)P);
  EXPECT(check_sweep_perf(N, R, P, ret.data(), W.data(), 0.03, 12.0, out.data()) == MCP_OK);
  EXPECT(check_sweep_perf(N, R, 0, ret.data(), nullptr, 0.03, 12.0, nullptr) == MCP_OK);        // P = 0 reads neither
  EXPECT(check_sweep_perf(0, R, P, ret.data(), W.data(), 0.0, 12.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_assets=0"));
  EXPECT(check_sweep_perf(MCP_MAX_ASSETS + 1, R, P, ret.data(), W.data(), 0.0, 12.0, out.data()) == MCP_E_ARG);
  EXPECT(check_sweep_perf(N, 1, P, ret.data(), W.data(), 0.0, 12.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_rows=1"));
  EXPECT(check_sweep_perf(N, MCP_SWEEP_MAX_ROWS + 1, P, ret.data(), W.data(), 0.0, 12.0, out.data()) == MCP_E_ARG);
  EXPECT(check_sweep_perf(N, R, -1, ret.data(), W.data(), 0.0, 12.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_portfolios=-1"));
  EXPECT(check_sweep_perf(N, R, P, ret.data(), W.data(), 0.0, 0.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "ann_factor"));
  EXPECT(check_sweep_perf(N, R, P, ret.data(), W.data(), 0.0, HUGE_VAL, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "ann_factor"));
  EXPECT(check_sweep_perf(N, R, P, ret.data(), W.data(), std::nan(""), 12.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "risk_free"));
  EXPECT(check_sweep_perf(N, R, P, nullptr, W.data(), 0.0, 12.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "returns is NULL"));
  EXPECT(check_sweep_perf(N, R, P, ret.data(), nullptr, 0.0, 12.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "W is NULL"));
  EXPECT(check_sweep_perf(N, R, P, ret.data(), W.data(), 0.0, 12.0, nullptr) == MCP_E_ARG && strstr(mcp_last_error(), "stats_out is NULL"));
  ret[(size_t)R * N - 1] = std::nan("");                                                      // the last value the scan reads
  EXPECT(check_sweep_perf(N, R, P, ret.data(), W.data(), 0.0, 12.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "returns[14] (row 4, asset 2)"));
  ret[(size_t)R * N - 1] = 0.01;
  W[(size_t)P * N - 2] = HUGE_VAL;
  EXPECT(check_sweep_perf(N, R, P, ret.data(), W.data(), 0.0, 12.0, out.data()) == MCP_E_ARG && strstr(mcp_last_error(), "W[10] (portfolio 3, asset 1)"));
}

int main() {
  run_finish();
  run_rules();
  printf("sweep_perf_selftest ok\n");
  return 0;
}

// sweep_boot_selftest.cpp -- the pure-host side of SPEC.md 5.25 for `make sweep-boot-selftest`: built with mcp_host.cpp by a plain C++
// compiler under AddressSanitizer + UBSan, no device.  mcp_sweep_boot_counts on exactly sized heap buffers at the row limits (R = 2 and
// R = 4096), at both extremes of the block (1 and +inf) and on a replicate range across 2^32, and every argument rule of it and of
// mcp_sweep_resampled.
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
      fprintf(stderr, "sweep_boot_selftest:%d: %s  [%s; last error: %s]\n", __LINE__, #cond, g_case, mcp_last_error()); \
      exit(1);                                                                                                       \
    }                                                                                                                \
  } while (0)

static const double INF = std::numeric_limits<double>::infinity();

// the counts of B replicates on an exactly sized heap buffer; every row must sum to R
static std::vector<uint16_t> counts_of(uint64_t seed, uint64_t begin, int B, int R, double block) {
  std::vector<uint16_t> c((size_t)B * (size_t)R, (uint16_t)0xFFFF);
  EXPECT(mcp_sweep_boot_counts(seed, begin, B, R, block, c.data()) == MCP_OK);
  for (int q = 0; q < B; q++) {
    long sum = 0;
    for (int r = 0; r < R; r++) sum += c[(size_t)q * R + r];
    EXPECT(sum == R);
  }
  return c;
}

static void run_counts() {
  const uint64_t seed = 0x9E3779B97F4A7C15ull;
  snprintf(g_case, sizeof g_case, "counts R = 2");
  {
    const int B = 64;
    const std::vector<uint16_t> c = counts_of(seed, 0, B, 2, 1.0);
    int seen[3] = {0, 0, 0};                                   // block 1 on two rows: counts (0,2), (1,1) and (2,0) all occur
    for (int q = 0; q < B; q++) seen[c[(size_t)q * 2]]++;
    EXPECT(seen[0] > 0 && seen[1] > 0 && seen[2] > 0 && seen[0] + seen[1] + seen[2] == B);
    const std::vector<uint16_t> whole = counts_of(seed, 0, B, 2, INF);
    for (size_t i = 0; i < whole.size(); i++) EXPECT(whole[i] == 1);
  }
  snprintf(g_case, sizeof g_case, "counts R = 4096");
  {
    const int R = MCP_SWEEP_MAX_ROWS, B = 3;
    const std::vector<uint16_t> whole = counts_of(seed, 5, B, R, INF);      // one circular block: every row exactly once
    for (size_t i = 0; i < whole.size(); i++) EXPECT(whole[i] == 1);
    const std::vector<uint16_t> iid = counts_of(seed, 5, B, R, 1.0);        // i.i.d.: about R / e rows are never drawn
    for (int q = 0; q < B; q++) {
      int zero = 0;
      for (int r = 0; r < R; r++) zero += iid[(size_t)q * R + r] == 0;
      EXPECT(zero > R / 4 && zero < R / 2);
    }
    const std::vector<uint16_t> mid = counts_of(seed, 5, B, R, 4.0);
    EXPECT(memcmp(mid.data(), iid.data(), mid.size() * sizeof(uint16_t)) != 0);
  }
  snprintf(g_case, sizeof g_case, "counts across 2^32");
  {
    const int R = 13, B = 6;
    const uint64_t begin = ((uint64_t)1 << 32) - 3;
    const std::vector<uint16_t> all = counts_of(seed, begin, B, R, 4.0);
    const std::vector<uint16_t> head = counts_of(seed, begin, 2, R, 4.0), tail = counts_of(seed, begin + 2, 4, R, 4.0);
    EXPECT(memcmp(all.data(), head.data(), head.size() * sizeof(uint16_t)) == 0);            // any partition, the same bytes
    EXPECT(memcmp(all.data() + head.size(), tail.data(), tail.size() * sizeof(uint16_t)) == 0);
    const std::vector<uint16_t> low = counts_of(seed, begin - ((uint64_t)1 << 32) + 3, 1, R, 4.0);   // replicate 0 is not replicate 2^32
    EXPECT(memcmp(low.data(), all.data() + 3 * (size_t)R, (size_t)R * sizeof(uint16_t)) != 0);
    const std::vector<uint16_t> other = counts_of(seed + 1, begin, B, R, 4.0);              // the seed is the key
    EXPECT(memcmp(other.data(), all.data(), all.size() * sizeof(uint16_t)) != 0);
    const std::vector<uint16_t> last = counts_of(seed, ~(uint64_t)0 - 1, 1, R, 4.0);         // the last replicate that does not wrap
    (void)last;
  }
  snprintf(g_case, sizeof g_case, "counts rules");
  {
    std::vector<uint16_t> c(2 * 5, (uint16_t)7);
    EXPECT(mcp_sweep_boot_counts(1, 0, 0, 5, 1.0, nullptr) == MCP_OK);                        // no replicate: nothing is read
    EXPECT(mcp_sweep_boot_counts(1, 0, 2, 1, 1.0, c.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_rows=1 outside [2,4096]"));
    EXPECT(mcp_sweep_boot_counts(1, 0, 2, MCP_SWEEP_MAX_ROWS + 1, 1.0, c.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_rows=4097"));
    EXPECT(mcp_sweep_boot_counts(1, 0, -1, 5, 1.0, c.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_replicates=-1 outside [0,4096]"));
    EXPECT(mcp_sweep_boot_counts(1, 0, MCP_SWEEP_MAX_REPLICATES + 1, 5, 1.0, c.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_replicates=4097"));
    EXPECT(mcp_sweep_boot_counts(1, 0, 2, 5, 0.5, c.data()) == MCP_E_ARG && strstr(mcp_last_error(), "block=0.5"));
    EXPECT(mcp_sweep_boot_counts(1, 0, 2, 5, std::nan(""), c.data()) == MCP_E_ARG && strstr(mcp_last_error(), "block="));
    EXPECT(mcp_sweep_boot_counts(1, ~(uint64_t)0, 2, 5, 1.0, c.data()) == MCP_E_ARG && strstr(mcp_last_error(), "wraps"));
    EXPECT(mcp_sweep_boot_counts(1, ~(uint64_t)0, 1, 5, 1.0, c.data()) == MCP_E_ARG && strstr(mcp_last_error(), "wraps"));
    EXPECT(mcp_sweep_boot_counts(1, 0, 2, 5, 1.0, nullptr) == MCP_E_ARG && strstr(mcp_last_error(), "counts_out is NULL"));
    for (size_t i = 0; i < c.size(); i++) EXPECT(c[i] == 7);                                  // a refused call writes nothing
  }
}

static void run_rules() {
  snprintf(g_case, sizeof g_case, "sweep boot rules");
  const int N = 3, R = 5, P = 4, B = 6;
  std::vector<double> ret((size_t)R * N, 0.01), W((size_t)P * N, 0.25), sc((size_t)5 * P * B);
  std::vector<int32_t> opt((size_t)3 * B);
  const auto call = [&](int n, int r, int p, const double* rt, const double* w, double rf, double ann, double alpha, uint64_t begin, int b,
                        double block, const double* s, const int32_t* o) {
    return check_sweep_boot(n, r, p, rt, w, rf, ann, alpha, begin, b, block, s, o);
  };
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.03, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_OK);
  EXPECT(call(N, R, 0, ret.data(), nullptr, 0.03, 12.0, 0.95, 0, B, 1.0, nullptr, nullptr) == MCP_OK);       // no work: W and the outputs unread
  EXPECT(call(N, R, P, ret.data(), nullptr, 0.03, 12.0, 0.95, 0, 0, 1.0, nullptr, nullptr) == MCP_OK);
  EXPECT(call(N, 2, P, ret.data(), W.data(), 0.03, 12.0, 0.95, 0, B, INF, sc.data(), opt.data()) == MCP_OK);
  EXPECT(call(0, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_assets=0"));
  EXPECT(call(MCP_MAX_ASSETS + 1, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG);
  EXPECT(call(N, 1, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_rows=1"));
  EXPECT(call(N, MCP_SWEEP_MAX_ROWS + 1, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG);
  EXPECT(call(N, R, -1, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_portfolios=-1"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, -1, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "n_replicates=-1"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, MCP_SWEEP_MAX_REPLICATES + 1, 1.0, sc.data(), opt.data()) == MCP_E_ARG);
  EXPECT(call(N, R, (1 << 15) + 1, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, 4096, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "2^27"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 0.99, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "block=0.99"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, ~(uint64_t)0 - 4, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "wraps"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, ~(uint64_t)0 - 6, B, 1.0, sc.data(), opt.data()) == MCP_OK);
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 0.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "ann_factor"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, INF, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "ann_factor"));
  EXPECT(call(N, R, P, ret.data(), W.data(), std::nan(""), 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "rf="));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.0, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "alpha=0 outside (0,1)"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 1.0, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "alpha=1"));
  EXPECT(call(N, R, P, nullptr, W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "returns is NULL"));
  EXPECT(call(N, R, P, ret.data(), nullptr, 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "W is NULL"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, nullptr, opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "scores_out is NULL"));
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), nullptr) == MCP_E_ARG && strstr(mcp_last_error(), "opt_out is NULL"));
  ret[(size_t)R * N - 1] = std::nan("");                                                      // the last value the scan reads
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "returns[14] (row 4, asset 2)"));
  ret[(size_t)R * N - 1] = 0.01;
  W[(size_t)P * N - 2] = HUGE_VAL;
  EXPECT(call(N, R, P, ret.data(), W.data(), 0.0, 12.0, 0.95, 0, B, 1.0, sc.data(), opt.data()) == MCP_E_ARG && strstr(mcp_last_error(), "W[10] (portfolio 3, asset 1)"));
}

int main() {
  run_counts();
  run_rules();
  printf("sweep_boot_selftest ok\n");
  return 0;
}

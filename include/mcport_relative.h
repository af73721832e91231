/* mcport_relative.h -- benchmark-relative statistics of a call's portfolios (SPEC.md 5.23): the active return of every portfolio
 * against one of the call's own rows on the same paths -- tracking error, information ratio, the probability and mean size of ending
 * behind, beta, alpha and correlation to the benchmark, up and down capture, and the order statistics of the active return (relative
 * VaR / CVaR) -- one more streaming reduction over the values every call already keeps on the device, over two rows at a time.  An
 * extension of include/mcport.h: the entry points below are additive, detected by symbol, and MCP_ABI_VERSION stays what mcport.h
 * says.  C99-clean. */
#ifndef MCPORT_RELATIVE_H
#define MCPORT_RELATIVE_H

#include "mcport.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The raw record of one row k against its benchmark row b (SPEC.md 5.23).  x_k and x_b are mcp_terminal_to_x of the two rows' stored
 * values of the same path, c_k and c_b the rows' pivots; d_k = x_k - c_k, d_b = x_b - c_b, e = d_k - d_b, a = x_k - x_b, every
 * difference and product rounded once in binary64.  A summand outside its set enters as + 0.0.  Summation order: lane, wave,
 * workgroup, the row's workgroups (record g on lane g mod 64 of one wave, in increasing g, then the wave's butterfly), shard (shard
 * order); no floating-point atomic, so a call repeats its bytes.  Across partitions the counts are exact and the sums agree to
 * association. */
typedef struct {
    uint64_t n, n_under, n_over;    /* #paths, #{a < 0}, #{a > 0}; a tie is in neither set */
    uint64_t n_up, n_down;          /* #{x_b > 0}, #{x_b < 0} */
    double   e1, e2;                /* sum e, sum e e */
    double   k1, b1;                /* sum d_k, sum d_b */
    double   k2, b2, kb;            /* sum d_k d_k, sum d_b d_b, sum d_k d_b */
    double   u1, u2;                /* sum a, sum a a over {a < 0} */
    double   up_k, up_b;            /* sum x_k, sum x_b over {x_b > 0} */
    double   down_k, down_b;        /* sum x_k, sum x_b over {x_b < 0} */
} mcp_relative_sums;

/* The finished record: mcp_relative_finish of the raw record, in binary64, by the formulas of SPEC.md 5.23 in the order written
 * there (monte_carlo_portfolio_amd/relative.py repeats them bit for bit).  Every quotient whose denominator is 0 is 0. */
typedef struct {
    double active_mean;             /* (c_k - c_b) + E1 / n */
    double tracking_error;          /* np.std(a, ddof = 1), from E1 and E2; 0 for n < 2 */
    double information_ratio;       /* active_mean / tracking_error; 0 when the tracking error is 0 */
    double p_under, p_over;         /* n_under / n, n_over / n */
    double mean_underperformance;   /* U1 / n_under; 0 when no path ends behind */
    double relative_downside_deviation;   /* sqrt(U2 / n) */
    double beta;                    /* cov(x_k, x_b) / var(x_b); 0 when var(x_b) is 0 */
    double alpha;                   /* mean_k - beta mean_b */
    double correlation;             /* in [-1, 1]; 0 when either variance is 0 */
    double up_capture;              /* UP_K / UP_B; 0 when no path has x_b > 0 */
    double down_capture;            /* DOWN_K / DOWN_B; 0 when no path has x_b < 0 */
    double pivot, bench_pivot;      /* c_k and c_b: whoever holds both records can finish again */
} mcp_relative_stats;

/* What a call is asked for: the row of the call's W that every portfolio is compared with.  reserved must be 0. */
typedef struct {
    int32_t bench;
    int32_t reserved;
} mcp_relative;

/* Workgroups per row of mcp_launch_relative over n values, a function of n alone, and the bytes of its d_partials for `rows`
 * rows (one mcp_relative_sums per row and workgroup). */
uint64_t mcp_relative_grid(uint64_t n);
size_t mcp_relative_ws_bytes(int rows, uint64_t n);
/* The smallest n at which the workgroups of a row that starts 16-byte aligned go through their load loop a second time. */
uint64_t mcp_relative_trip_n(void);

/* Enqueue-only, on the device that owns `stream`: the raw records of the `rows` rows of the binary32 array d_values
 * [rows][stride], n <= stride live values each, x formed by prm->compounding and prm->v0 as mcp_terminal_to_x forms it.  The rows
 * come in groups of `group`: row r is compared with row (r / group) group + bench.  d_pivot: device [rows] binary64, or NULL for
 * c = 0.  d_partials: mcp_relative_ws_bytes(rows, n) bytes.  d_sums: device [rows] mcp_relative_sums.  d_active: device
 * [rows][stride] binary32, Y = fl32(1 + a) of every live value, or NULL, and then nothing is written.  Rows and d_active may start at
 * any 4-byte boundary, whatever the stride.  MCP_E_ARG: a NULL prm, d_values, d_partials or d_sums, rows < 1, group < 1, rows not a
 * multiple of group, bench outside [0, group), stride < n, and the rules of prm. */
int mcp_launch_relative(const mcp_params *prm, const float *d_values, uint64_t stride, uint64_t n, int rows, int group, int bench,
                        const double *d_pivot, void *d_partials, void *d_sums, float *d_active, void *stream);

/* Pure host arithmetic: the finished record of one raw record about the pivots c_k and c_b.  MCP_E_ARG: a NULL pointer. */
int mcp_relative_finish(const mcp_relative_sums *sums, double pivot, double bench_pivot, mcp_relative_stats *out);

/* Arms the context: the next mcp_simulate_* call on it that walks paths fills the arrays -- stats_out [K] (and sums_out [K] when
 * given) over the terminal values against row req->bench, active_stats_out [K] (when given) the statistics of the stored
 * Y = fl32(1 + a) reduced as the turnover of SPEC.md 5.18 is (x = Y - 1, rf 0, no pivot, the call's alpha; sharpe 0), active_out
 * [K*n] (when given) that array itself, hz_stats_out [H*K] (row h*K + k) over the horizon rows against the benchmark's row of the
 * same horizon, at their own pivots -- and disarms the context, whether that call succeeds or fails.  A call that its own argument
 * rules refuse returns before the context is looked at and leaves the request in place: withdraw it, or let the next call take it.
 * The caller keeps the arrays alive until the request is spent or withdrawn.  A second request before such a call replaces the
 * first; req == NULL withdraws the request in place and reads no other argument.  Calls on one context are serialised by the
 * library.  The records cover every combination the call itself covers that keeps all K portfolios in one tile on every shard:
 * passes of 8 portfolios, the MFMA sweep kernels, several devices, logical shards, antithetic pairs (whose members count as paths).
 * Argument errors (MCP_E_ARG) are found before any device is touched: a NULL ctx or stats_out, bench < 0, reserved != 0.  The next
 * call fails with MCP_E_ARG before it walks if bench is not below its n_portfolios, if hz_stats_out is given and it has no
 * horizons, or if its plan cuts the K portfolios (portfolio shards on several shards, a terminal budget below all K rows: raise the
 * budget or shard by paths).  mcp_sweep_historical walks no paths: it neither reads nor disarms the request.  The second walk of
 * mcp_simulate_attribution stores no values: the request is served by that call's first walk alone. */
int mcp_ctx_request_relative(mcp_ctx *ctx, const mcp_relative *req, mcp_relative_sums *sums_out, mcp_relative_stats *stats_out,
                             mcp_stats *active_stats_out, float *active_out, mcp_relative_stats *hz_stats_out);

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_RELATIVE_H */

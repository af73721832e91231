/* mcport_downside.h -- downside and shape statistics of a simulated distribution (SPEC.md 5.22): the Sortino ratio the reference
 * reports (app.py:238-243), the target semideviation, the probability and the mean size of a shortfall below a threshold, Omega, and
 * the skewness and excess kurtosis of x -- one more streaming reduction over the values every call already keeps on the device.  An
 * extension of include/mcport.h: the entry points below are additive, detected by symbol, and MCP_ABI_VERSION stays what mcport.h
 * says.  C99-clean. */
#ifndef MCPORT_DOWNSIDE_H
#define MCPORT_DOWNSIDE_H

#include "mcport.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The raw record of one row (SPEC.md 5.22).  A row is a portfolio's terminal values or a (horizon, portfolio) row of SPEC.md 4.3;
 * x is mcp_terminal_to_x of every value, c the row's pivot, tau the threshold; d = x - c, e = x - tau, every product below rounded
 * once: d2 = d d, d3 = d2 d, d4 = d2 d2, e2 = e e.  Summation order: lane, wave, workgroup, the row's workgroups (record b
 * on lane b mod 64 of one wave, in increasing b, then the wave's butterfly), shard (shard order); no floating-point atomic, so a call
 * repeats its bytes.  Across partitions the counts are exact and the sums agree to association. */
typedef struct {
    uint64_t n, n_below, n_above;   /* #values, #{e < 0}, #{e > 0}; a value equal to tau is in neither set */
    double   s1, s2, s3, s4;        /* sum d, sum d2, sum d3, sum d4 */
    double   b1, b2;                /* sum d, sum d2 over {e < 0}: the reference's std of the negative excess returns, about c */
    double   l1, l2;                /* sum e, sum e2 over {e < 0}: the lower partial moments about tau */
    double   u1;                    /* sum e over {e > 0} */
} mcp_downside_sums;

/* The finished record: mcp_downside_finish of the raw record, in binary64, by the formulas of SPEC.md 5.22 in the order written
 * there (monte_carlo_portfolio_amd/downside.py repeats them bit for bit). */
typedef struct {
    double mean;                    /* c + S1 / n */
    double skewness;                /* population form (scipy.stats.skew); 0 when the central second moment is 0 */
    double excess_kurtosis;         /* population form (scipy.stats.kurtosis); 0 when the central second moment is 0 */
    double downside_std;            /* np.std(e[e < 0], ddof = 1); NaN for one such value, 1e-4 for none (app.py:241-242) */
    double sortino;                 /* (mean - tau) / downside_std: the reference's ratio, not annualised */
    double downside_deviation;      /* sqrt(L2 / n): the target semideviation */
    double sortino_target;          /* (mean - tau) / downside_deviation; 0 when that deviation is 0 */
    double p_below;                 /* n_below / n */
    double mean_shortfall;          /* L1 / n_below; 0 when the below-set is empty */
    double omega;                   /* U1 / (-L1); +inf when L1 == 0 */
    double pivot;                   /* c, what the raw record's d is about: whoever holds both records can finish again */
} mcp_downside_stats;

/* What a call is asked for.  use_rf != 0: the threshold is the call's prm->rf and tau is not read (it must still be finite).
 * reserved must be 0. */
typedef struct {
    double  tau;
    int32_t use_rf;
    int32_t reserved;
} mcp_downside;

/* Workgroups per row of mcp_launch_downside over n values, a function of n alone, and the bytes of its d_partials for `rows`
 * rows (one mcp_downside_sums per row and workgroup). */
uint64_t mcp_downside_grid(uint64_t n);
size_t mcp_downside_ws_bytes(int rows, uint64_t n);
/* The smallest n at which the workgroups of a row that starts 16-byte aligned go through their load loop a second time. */
uint64_t mcp_downside_trip_n(void);

/* Enqueue-only, on the device that owns `stream`: the raw records of the `rows` rows of the binary32 array d_values
 * [rows][stride], n <= stride live values each, x formed by prm->compounding and prm->v0 as mcp_terminal_to_x forms it.
 * d_pivot: device [rows] binary64, or NULL for c = 0.  d_partials: mcp_downside_ws_bytes(rows, n) bytes.  d_sums: device [rows]
 * mcp_downside_sums.  Rows may start at any 4-byte boundary.  MCP_E_ARG: a NULL prm, d_values, d_partials or d_sums, rows < 1,
 * stride < n, a tau that is not finite, and the rules of prm. */
int mcp_launch_downside(const mcp_params *prm, const float *d_values, uint64_t stride, uint64_t n, int rows,
                        const double *d_pivot, double tau, void *d_partials, void *d_sums, void *stream);

/* Pure host arithmetic: the finished record of one raw record.  MCP_E_ARG: a NULL pointer. */
int mcp_downside_finish(const mcp_downside_sums *sums, double tau, double pivot, mcp_downside_stats *out);

/* Arms the context: the next mcp_simulate_* call on it that walks paths fills the arrays -- stats_out [K] (and sums_out [K] when
 * given) over the terminal values, hz_stats_out [H*K] (row h*K + k) over the horizon rows at their own pivots -- and disarms the
 * context, whether that call succeeds or fails.  A call that its own argument rules refuse returns before the context is looked at
 * and leaves the request in place: withdraw it, or let the next call take it.  The caller keeps the arrays alive until the request is
 * spent or withdrawn.  A second request before such a call replaces the first; req == NULL withdraws the request in place and reads
 * no other argument.  Calls on one context are serialised by the library.  The records cover every combination the call
 * itself covers: passes of 8 portfolios, the MFMA sweep kernels, tiles, several devices, logical shards, portfolio shards,
 * antithetic pairs (whose members count as paths).  Argument errors (MCP_E_ARG) are found before any device is touched: a NULL ctx
 * or stats_out, a tau that is not finite, reserved != 0.  If hz_stats_out is given and the next call has no horizons, that call
 * fails with MCP_E_ARG before it walks.  mcp_sweep_historical walks no paths: it neither reads nor disarms the request.  The second
 * walk of mcp_simulate_attribution stores no values: the request is served by that call's first walk alone. */
int mcp_ctx_request_downside(mcp_ctx *ctx, const mcp_downside *req, mcp_downside_sums *sums_out,
                             mcp_downside_stats *stats_out, mcp_downside_stats *hz_stats_out);

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_DOWNSIDE_H */

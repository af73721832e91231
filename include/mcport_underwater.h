/* mcport_underwater.h -- the time under water of the drawdown walk of libmcport.so (SPEC.md 4.20 / 5.20): how long a path stays
 * below its running peak -- the longest such spell and the spell it is in at the horizon -- per path, as histograms over every length,
 * and as order statistics.  An extension of include/mcport.h: the entry point below is additive, detected by symbol, and
 * MCP_ABI_VERSION stays what mcport.h says.  C99-clean. */
#ifndef MCPORT_UNDERWATER_H
#define MCPORT_UNDERWATER_H

#include "mcport.h"
#include "mcport_life.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule (SPEC.md 4.20).  Per path and portfolio the drawdown walk of SPEC.md 4.2 carries two uint32 counters from 0, the current
 * spell c and the longest spell m.  After step t = 1 .. n_steps it updates the peak as section 4.2 says, P = fmaxf(P, X_t) with X = V
 * (simple compounding) or S (log), and then
 *     w = X_t < P                      binary32 compare against the peak just updated; false on a NaN
 *     c = w ? c + 1 : 0
 *     m = max(m, c)
 * The outputs are m and c_T.  The peak starts at X_1, so step 1 is never under water and 0 <= c_T <= m <= max(n_steps - 1, 0); a
 * return to the peak exactly ends a spell; c_T == 0 is a path that ends at its high-water mark.
 *
 * mcp_simulate_underwater is mcp_simulate_drawdown (gv, st and jp NULL), mcp_simulate_student_t (st), mcp_simulate_garch (gv, with or
 * without st) or mcp_simulate_jumps (jp) with the drawdown and these counters switched on: every argument up to dd_stats_out is that
 * call's, with that call's rules and results bit for bit (terminal_out, mdd_out and both records); dd_stats_out is required.  On top:
 *   longest_out       NULL or host [K*n_paths]: m of every path, row k at k*n_paths
 *   current_out       NULL or host [K*n_paths]: c_T likewise
 *   longest_hist_out  [K][n_steps + 1]: hist[k][s] = #{m == s}; every row sums to n_paths; the entry at n_steps is always 0 (it keeps
 *                     the layout of mcp_lifetime_summary)
 *   current_hist_out  [K][n_steps + 1]: the same for c_T
 *   sums_out          [K][2]: sum over s of s hist[k][s], of m then of c_T
 *   q_out             [K][2][n_uw_levels], NULL exactly when n_uw_levels == 0: for every level q in percent (0 <= q <= 100, at most
 *                     MCP_MAX_LEVELS) the order statistic of m, then of c_T, at rank `lo` of mcp_percentile_rank_q(n_paths, q) --
 *                     np.percentile(., q, method="lower")
 * All exact integers, independent of how the path range is cut over tiles, shards and devices.  Argument errors (MCP_E_ARG: a NULL
 * dd_stats_out, longest_hist_out, current_hist_out or sums_out; a bad level; q_out against n_uw_levels; and every rule of the draws'
 * own structs) are found before any device is touched.  MCP_E_UNSUPPORTED: n_steps > MCP_MAX_LIFE_STEPS, MCP_FLAG_FOLD,
 * MCP_FLAG_NATIVE_MATH, log compounding with gv, st or jp, jumps together with gv or st.  Not built: the time under water with
 * regimes, antithetic pairs, the overlay, floor protection or volatility targeting, on bootstrap or filtered rows (which have no
 * drawdown walk), with horizons, at the mcp_launch_* level or in engine.PathEngine.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_underwater(mcp_ctx *ctx, const mcp_params *prm,
                            const mcp_garch *gv,             /* NULL: no GARCH                                  */
                            const mcp_student_t *st,         /* NULL: Gaussian draws                            */
                            const mcp_jumps *jp,             /* NULL: no jumps; not with gv or st               */
                            const float *mu, const float *chol, const float *W,
                            uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                            float *terminal_out,             /* NULL or host [K*n_paths] */
                            mcp_stats *stats_out,            /* [K] */
                            float *mdd_out,                  /* NULL or host [K*n_paths] q / d of SPEC.md 4.2 */
                            mcp_stats *dd_stats_out,         /* [K], required */
                            uint32_t *longest_out,           /* NULL or host [K*n_paths] */
                            uint32_t *current_out,           /* NULL or host [K*n_paths] */
                            uint64_t *longest_hist_out,      /* [K][n_steps + 1] */
                            uint64_t *current_hist_out,      /* [K][n_steps + 1] */
                            uint64_t *sums_out,              /* [K][2] */
                            int n_uw_levels, const double *uw_levels,
                            uint32_t *q_out);                /* [K][2][n_uw_levels], NULL iff n_uw_levels == 0 */

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_UNDERWATER_H */

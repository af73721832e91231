/* mcport_life.h -- the time of ruin and the survival curve of the walks with absorbing ruin of libmcport.so (SPEC.md 4.17 / 5.17): how
 * long the money lasts, per path, as a histogram over every step, and as order statistics.  An extension of include/mcport.h: the
 * entry points below are additive, detected by symbol, and MCP_ABI_VERSION stays what mcport.h says.  C99-clean. */
#ifndef MCPORT_LIFE_H
#define MCPORT_LIFE_H

#include "mcport.h"
#include "mcport_spend.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The lifetime needs 1 <= n_steps + 1 <= MCP_MAX_LIFE_STEPS + 1; beyond that the call returns MCP_E_UNSUPPORTED. */
#define MCP_MAX_LIFE_STEPS 1048576

/* The lifetime (SPEC.md 4.17).  Per path and portfolio the walk carries one uint32 l from 0; after the update of step s = 1 .. n_steps
 *     l = l + (V_s > 0 ? 1 : 0)
 * with V_s the value that step stores (+0 from the step of ruin on; a NaN U is ruin).  Ruin is absorbing, so V_s > 0 exactly when
 * s <= l: l == n_steps is a path that was not ruined inside the horizon (censored), l < n_steps one that was ruined in step l + 1.
 *
 * mcp_simulate_lifetime is mcp_simulate_cashflow (cf alone), mcp_simulate_glide (cf and gl) or mcp_simulate_spending (sp alone) with
 * that counter switched on: exactly one of cf and sp is not NULL, gl needs cf.  Every argument up to wd_stats_out is that call's, with
 * that call's rules, refusals and results bit for bit (terminal_out, horizon_out, withdrawn_out, the counts, records and bands);
 * withdrawn_out and wd_stats_out are NULL without sp.  On top:
 *   life_out       NULL or host [K*n_paths]: l of every path, row k at k*n_paths
 *   life_hist_out  [K][n_steps + 1]: hist[k][s] = #{l == s}; every row sums to n_paths
 *   life_sum_out   [K]: sum over s of s hist[k][s]
 *   life_q_out     [K][n_life_levels], NULL exactly when n_life_levels == 0: for every level q in percent (0 <= q <= 100, at most
 *                  MCP_MAX_LEVELS) the order statistic of l at rank `lo` of mcp_percentile_rank_q(n_paths, q) -- np.percentile(l, q,
 *                  method="lower")
 * All exact integers, independent of how the path range is cut over tiles, shards and devices.  Argument errors (MCP_E_ARG: both or
 * neither of cf and sp; gl without cf; withdrawn_out or wd_stats_out without sp; life_hist_out or life_sum_out NULL; a bad level;
 * life_q_out against n_life_levels) are found before any device is touched.  MCP_E_UNSUPPORTED: n_steps > MCP_MAX_LIFE_STEPS.  Not
 * built: the lifetime at the mcp_launch_* level, and on floor protection, which has no ruin rule.  K >= 17 runs as passes of 8. */
int mcp_simulate_lifetime(mcp_ctx *ctx, const mcp_params *prm,
                          const mcp_cashflow *cf,                /* the schedule ...                               */
                          const mcp_glide *gl,                   /* ... NULL or, with cf, the glide path           */
                          const mcp_spending *sp,                /* ... or the spending rule: exactly one of cf, sp */
                          const float *mu, const float *chol, const mcp_bootstrap *boot, const mcp_student_t *st,
                          const float *W, uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                          int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                          float *terminal_out, mcp_stats *stats_out, uint64_t *counts_out, float *horizon_out,
                          mcp_stats *hz_stats_out, double *bands_out, uint64_t *hz_counts_out,
                          float *withdrawn_out, mcp_stats *wd_stats_out,
                          uint32_t *life_out,         /* NULL or host [K*n_paths] */
                          uint64_t *life_hist_out,    /* [K][n_steps + 1] */
                          uint64_t *life_sum_out,     /* [K] */
                          int n_life_levels, const double *life_levels,
                          uint32_t *life_q_out);      /* [K][n_life_levels], NULL iff n_life_levels == 0 */

/* The reduction of SPEC.md 5.17 of one histogram hist[0 .. n_steps] (host only): *sum_out = sum of s hist[s], q_out[i] the order
 * statistic at rank `lo` of mcp_percentile_rank_q(sum of hist, levels[i]).  0 <= n_steps <= MCP_MAX_LIFE_STEPS; q_out NULL exactly
 * when n_levels == 0; an empty histogram has no quantile (MCP_E_ARG when n_levels > 0). */
int mcp_lifetime_summary(const uint64_t *hist, int n_steps, int n_levels, const double *levels, uint64_t *sum_out, uint32_t *q_out);

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_LIFE_H */

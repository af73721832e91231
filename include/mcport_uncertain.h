/* mcport_uncertain.h -- drift uncertainty (estimation risk) for the path engine of libmcport.so (SPEC.md 2.7 / 4.21 / 5.21): every
 * path draws its own drift once, m = mu + M g with g ~ N(0, I), and walks on it.  mu is a sample mean; M is the factor of the
 * covariance of that mean.  An extension of include/mcport.h: the entry point below is additive, detected by symbol, and
 * MCP_ABI_VERSION stays what mcport.h says.  C99-clean. */
#ifndef MCPORT_UNCERTAIN_H
#define MCPORT_UNCERTAIN_H

#include "mcport.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule (SPEC.md 2.7 / 4.21).  factor: M [N*N], binary32, row-major, used as lower triangular (the entries above the diagonal
 * take no part); every entry of the array must be finite; all-zero is allowed.  It is zero-padded to N4 and passed through + 0.0f as the
 * Cholesky factor is.  Once per path p, before step 0, nb = ceil(N/4) Philox blocks on counter stream 5
 *     x(q) = Philox(counter = (q, 5, p & 0xffffffff, p >> 32)),  q = 0 .. nb - 1,     g[m nb + q] = Z(x_m(q))
 * (the transform of SPEC.md 3, the assignment to assets of SPEC.md 2) and, in binary32,
 *     m_i = mu_i;  for j = 0 .. i:  m_i = fma(M[i,j], g_j, m_i)                       j ascending
 * Every step of the path then starts row i of its chain at m_i in place of mu_i; nothing else changes.  The counter depends neither
 * on n_steps nor on the step, the asset normals stay on stream 0, all portfolios of a path share m.  M = 0 gives the stored values
 * of the call without uncertainty bit for bit.  reserved must be 0. */
typedef struct {
    const float *factor;            /* [N*N] */
    int32_t      reserved;          /* must be 0 */
} mcp_drift_uncertainty;

/* mcp_simulate (cf NULL, no horizons, no drawdown), mcp_simulate_drawdown (dd_stats_out given), mcp_simulate_horizons (n_horizons > 0)
 * or mcp_simulate_cashflow on Gaussian draws (cf given, with or without horizons; cf->target as that call has it) with the per-path
 * drift above: the outputs, records, bands and counts are those calls', pivoted as those calls are (SPEC.md 5.21: mcp_pivots, or the
 * cash-flow pivot of SPEC.md 5.6).  Simple or log compounding; the spec's normals and the unfolded recurrence.  counts_out and
 * hz_counts_out belong to cf: counts_out NULL exactly when cf is, hz_counts_out given exactly when cf is and n_horizons > 0.
 * Argument errors (MCP_E_ARG: a NULL struct or factor, an entry that is not finite before or after rounding, reserved != 0, and
 * every rule of the underlying call) are found before any device is touched.  MCP_E_UNSUPPORTED: MCP_FLAG_FOLD,
 * MCP_FLAG_NATIVE_MATH, the drawdown together with horizons or with cash flows, log compounding with cash flows.  Not built: drift
 * uncertainty with any other feature (Student-t draws, GARCH, jumps, regimes, bootstrap or filtered rows, rebalancing, bands, glide
 * paths, spending rules, the lifetime, floor protection, volatility targeting, the overlay, the attribution, antithetic pairs, the
 * time under water), at the mcp_launch_* level or in engine.PathEngine.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_uncertain(mcp_ctx *ctx, const mcp_params *prm, const mcp_drift_uncertainty *du,
                           const mcp_cashflow *cf,          /* NULL: no cash flows */
                           const float *mu, const float *chol, const float *W,
                           uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                           int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                           float *terminal_out,             /* NULL or host [K*n_paths] */
                           mcp_stats *stats_out,            /* [K] */
                           float *mdd_out,                  /* NULL or host [K*n_paths] q / d of SPEC.md 4.2; needs dd_stats_out */
                           mcp_stats *dd_stats_out,         /* NULL: no drawdown; else [K] */
                           uint64_t *counts_out,            /* [K][2] {n_ruined, n_short}; NULL iff cf is NULL */
                           float *horizon_out,              /* NULL or host [H*K*n_paths], row h*K + k */
                           mcp_stats *hz_stats_out,         /* [H*K], NULL iff n_horizons == 0 */
                           double *bands_out,               /* [H*K*L], NULL iff n_levels == 0 */
                           uint64_t *hz_counts_out);        /* [H*K][2], given iff cf and n_horizons > 0 */

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_UNCERTAIN_H */

/* mcport_sweep_boot.h -- the resampled historical sweep (SPEC.md 5.25): the rows of the sweep's return sample are redrawn n_replicates
 * times by the stationary block bootstrap of SPEC.md 2.1, every portfolio of the sweep is scored on every resample with the figures of
 * mcp_sweep_historical's loop (port_return, port_std, sharpe, var, cvar, here all five from the resampled series), and every replicate
 * names its optimum by each of the loop's three criteria.  An extension of include/mcport.h: the entry points below are additive,
 * detected by symbol, and MCP_ABI_VERSION stays what mcport.h says.  C99-clean. */
#ifndef MCPORT_SWEEP_BOOT_H
#define MCPORT_SWEEP_BOOT_H

#include "mcport.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCP_SWEEP_MAX_REPLICATES 4096

/* Replicate g = replicate_begin + beta resamples the rows that path g of a bootstrap call with n_steps = n_rows on n_rows rows walks
 * (counter (t, 1, g_lo, g_hi), key from seed, start = mulhi(x0, R), a restart at t = 0 or when x1 < thr(block)); a resample enters the
 * figures through its row counts c_g[r] = #{t : j_t = r} alone, and any partition of a replicate range gives the same bytes per
 * replicate.  With y_p[r] = sum_i returns[r,i] W[p,i] (i ascending from 0.0, product and sum rounded separately) and all sums over r
 * ascending, one binary64 operation at a time:  S = sum c[r] y[r], m = S / R, M2 = sum c[r] ((y[r] - m) (y[r] - m)), port_return =
 * m ann_factor, port_std = sqrt(M2 / (R - 1) ann_factor), sharpe = port_std > 0 ? (port_return - rf) / port_std : 0; var is NumPy's
 * percentile (method 'linear', ranks of mcp_percentile_rank(R, alpha)) of the resampled series, taken by walking the stable ascending
 * order of y_p with the counts accumulated; cvar is the count-weighted mean of the sorted values <= var, kept inside [smallest value of
 * the resample, var].
 * scores_out: [5][P][B], the figures in the order above.  opt_out: [3][B], per replicate the first portfolio attaining the largest
 * sharpe, var and cvar.  counts_out: NULL or [B][R].  The call runs on shard 0 of the context.  n_portfolios == 0 or n_replicates == 0
 * returns MCP_OK at once and touches neither a device nor an output.  Argument errors are MCP_E_ARG, found before any device is
 * touched, mcp_last_error() naming the argument: n_assets outside [1, MCP_MAX_ASSETS], n_rows outside [2, MCP_SWEEP_MAX_ROWS],
 * n_portfolios < 0, n_replicates outside [0, MCP_SWEEP_MAX_REPLICATES], n_portfolios * n_replicates > 2^27, an ann_factor that is not
 * finite and > 0, an rf that is not finite, an alpha outside (0, 1), a block that is not >= 1 (+inf is allowed), a replicate range that
 * wraps, a NULL returns, and for a call with work a NULL W, scores_out or opt_out, a value of returns or W that is not finite (the scan
 * of mcp_sweep_historical_perf), and last a NULL ctx.  A failed device allocation is MCP_E_NOMEM.  The call walks no paths: it neither
 * reads nor disarms a pending downside or relative request. */
int mcp_sweep_resampled(mcp_ctx *ctx, int n_assets, int n_rows, int n_portfolios, const double *returns, const double *W,
                        double rf, double ann_factor, double alpha, uint64_t seed, uint64_t replicate_begin, int n_replicates,
                        double block, double *scores_out, int32_t *opt_out, uint16_t *counts_out);

/* Pure host arithmetic: the row counts of the same replicates, counts_out [B][R], every row summing to n_rows.  MCP_E_ARG: n_rows
 * outside [2, MCP_SWEEP_MAX_ROWS], n_replicates outside [0, MCP_SWEEP_MAX_REPLICATES], a block that is not >= 1, a replicate range
 * that wraps, and for n_replicates > 0 a NULL counts_out. */
int mcp_sweep_boot_counts(uint64_t seed, uint64_t replicate_begin, int n_replicates, int n_rows, double block, uint16_t *counts_out);

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_SWEEP_BOOT_H */

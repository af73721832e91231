/* mcport_band.h -- tolerance-band rebalancing of libmcport.so (SPEC.md 4.18 / 5.18): the portfolio is looked at on a schedule and traded
 * back to its weights only when an asset has drifted out of its band; per path the number of trades and the turnover.  An extension of
 * include/mcport.h: the entry points below are additive, detected by symbol, and MCP_ABI_VERSION stays what mcport.h says.  C99-clean. */
#ifndef MCPORT_BAND_H
#define MCPORT_BAND_H

#include "mcport.h"
#include "mcport_life.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule (SPEC.md 4.18).  every: the review period e >= 0 in steps -- a review after every step s with s mod e == 0 and s < n_steps
 * (0: never); cost: kappa in [0, 1), the proportional cost of mcp_rebalance; tol: host [K][N] floats, every entry finite and >= 0, or
 * +inf for an asset that is not watched.  At a review a path marks rho^ = W.B as mcp_simulate_rebalanced does and trades when a watched
 * asset i has  fl32(|W[k,i]| fl32(|B_i - rho^|)) >= fma(tol[k,i], rho^, tol[k,i])  -- its weight is off target by tol[k,i] or more.  The
 * trade is mcp_simulate_rebalanced's, operation for operation; a path that does not trade changes nothing.  n_reviews =
 * floor((n_steps - 1) / every) for 1 <= every < n_steps, else 0; it must not exceed MCP_MAX_LIFE_STEPS (MCP_E_UNSUPPORTED). */
typedef struct mcp_band {
  int32_t every;
  int32_t reserved;    /* must be 0 */
  double cost;
  const float *tol;    /* [K][N] */
} mcp_band;

/* mcp_simulate_rebalanced with the trade of every date decided per path (SPEC.md 4.18; simple compounding only).  Draws, horizon inputs
 * and the outputs up to bands_out are that call's, with that call's rules; the pivot of the moments is mcp_rebalance_pivots at period =
 * every.  With every tol = 0 the values are that call's bit for bit; with every tol = +inf, or every = 0, they are buy-and-hold's.
 * On top:
 *   trades_out          NULL or host [K*n_paths]: the trade count c of every path, row k at k*n_paths
 *   trade_hist_out      [K][n_reviews + 1]: hist[k][s] = #{c == s}; every row sums to n_paths
 *   trade_sum_out       [K]: sum over s of s hist[k][s]
 *   trade_q_out         [K][n_trade_levels], NULL exactly when n_trade_levels == 0: for every level q in percent (0 <= q <= 100, at most
 *                       MCP_MAX_LEVELS) np.percentile(c, q, method="lower"), read off the histogram as mcp_lifetime_summary does
 *   turnover_out        NULL or host [K*n_paths]: the turnover Y of every path, the sum over its trades of tau = sum_i |W_i| |B_i - rho^|
 *   turnover_stats_out  [K]: one mcp_stats record over x = (double)Y - 1 (pivot 0, sharpe 0); its var is np.percentile(x, 100 (1 - alpha))
 *                       bit for bit
 * The counts are exact integers and every output is independent of how the path range is cut over tiles, shards and devices.  Argument
 * errors (MCP_E_ARG: bd or bd->tol NULL; an entry of tol negative or NaN; reserved != 0; every < 0; cost outside [0, 1); trade_hist_out,
 * trade_sum_out or turnover_stats_out NULL; a bad level; trade_q_out against n_trade_levels) are found before any device is touched.
 * MCP_E_UNSUPPORTED: log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH, n_reviews > MCP_MAX_LIFE_STEPS.  Every portfolio is a pass
 * of its own over the draws: the cost of K portfolios is K walks.  Not built: bands at the mcp_launch_* level. */
int mcp_simulate_banded(mcp_ctx *ctx, const mcp_params *prm, const mcp_band *bd,
                        const float *mu, const float *chol,   /* Gaussian draws ...                       */
                        const mcp_bootstrap *boot,             /* ... or bootstrap draws: exactly one        */
                        const float *W, uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                        int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                        float *terminal_out, mcp_stats *stats_out, float *horizon_out,
                        mcp_stats *hz_stats_out, double *bands_out,
                        uint32_t *trades_out,          /* NULL or host [K*n_paths] */
                        uint64_t *trade_hist_out,      /* [K][n_reviews + 1] */
                        uint64_t *trade_sum_out,       /* [K] */
                        int n_trade_levels, const double *trade_levels,
                        uint32_t *trade_q_out,         /* [K][n_trade_levels], NULL iff n_trade_levels == 0 */
                        float *turnover_out,           /* NULL or host [K*n_paths] */
                        mcp_stats *turnover_stats_out);/* [K] */

/* n_reviews of a call (host only, no device is touched): floor((n_steps - 1) / every) for 1 <= every < n_steps, else 0; -1 and
 * mcp_last_error() for NULL arguments, n_steps < 0 or every < 0. */
int mcp_band_reviews(const mcp_params *prm, const mcp_band *bd);

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_BAND_H */

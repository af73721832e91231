/* mcport_spend.h -- spending rules for the path engine of libmcport.so (SPEC.md 4.16 / 5.16): withdrawals that depend on the path --
 * a constant inflation-adjusted amount, a fixed percentage of the current value, or a floor-and-ceiling rule between the two.  An
 * extension of include/mcport.h: the entry points below are additive, detected by symbol, and MCP_ABI_VERSION stays what mcport.h
 * says.  C99-clean. */
#ifndef MCPORT_SPEND_H
#define MCPORT_SPEND_H

#include "mcport.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule (SPEC.md 4.16; simple compounding, binary32 with IEEE fminf / fmaxf and correctly rounded fma, nothing fused across
 * lines).  Per path and portfolio the walk carries the value V from fl32(v0), the per-step withdrawal w from w0 and the total paid out
 * Y from +0.  Step s = 1 .. n_steps, on the step's portfolio return rho exactly as mcp_simulate_cashflow forms it:
 *     U0   = fma(V, rho, V)
 *     U    = U0 - w
 *     live = V > 0 and U > 0
 *     paid = live ? w : ((V > 0 and U0 > 0) ? U0 : +0)      the step of ruin pays out what is left
 *     V    = live ? U : +0                                   ruin is absorbing; a NaN U0 is ruin and pays +0
 *     Y    = Y + paid
 *     (the horizon store of V)
 *     if every >= 1 and s mod every == 0:                    the review, after the store
 *         w' = fl32(w g32)
 *         w  = fminf(fmaxf(fl32(p32 V), fl32(w' lo32)), fl32(w' hi32))
 * with p32 = fl32(rate), g32 = fl32(1 + inflation), lo32 = fl32(1 - down), hi32 = fl32(1 + up) and w0 = fl32(first) or, has_first
 * == 0, fl32((double)p32 (double)fl32(v0)) (mcp_spending_consts).  A NaN bound (0 inf) is ignored; w is never negative and never
 * NaN.  rate: finite, >= 0, the fraction of the current value aimed at per step; every: >= 0, 0 never reviews; down in [0, 1], the
 * largest cut per review; up in [0, +inf], +inf allowed, the largest raise per review; inflation: finite, > -1, applied per review;
 * first: finite, >= 0 (read only when has_first == 1); target: finite (read only when has_target == 1), for the second count, as
 * mcp_cashflow's.  Every rule holds before and after rounding to binary32.  has_first and has_target are 0 or 1; reserved must be
 * 0; fl32(v0) > 0. */
typedef struct {
    double  rate, down, up, inflation, first, target;
    int32_t every, has_first, has_target, reserved;
} mcp_spending;

/* mcp_simulate_cashflow with the rule above in place of the schedule: the draws, the horizons, records, bands and the counts
 * {n_ruined, n_short} are that call's.  withdrawn_out: Y_T of every path; wd_stats_out[k]: the record of x_Y = (double)Y_T /
 * (double)fl32(v0) - 1 at the call's alpha with sharpe = 0, reduced as the drawdown array of mcp_simulate_drawdown is (VaR is
 * np.percentile of the stored values), moments pivoted at SPEC.md 5.16 (mcp_spending_pivots).  With every = 0, or down = up =
 * inflation = 0, w stays w0 and terminal_out, horizon_out, the counts, records and bands are those of mcp_simulate_cashflow on the
 * schedule c_s = -w0, bit for bit.  Argument errors (MCP_E_ARG: a NULL struct, counts_out, wd_stats_out or required output; a value
 * outside its range or not finite, before or after rounding to binary32; every < 0; has_first or has_target not 0 / 1; reserved != 0;
 * fl32(v0) not positive; hz_counts_out NULL exactly when n_horizons == 0 is required; and every rule of the draws' own structs) are
 * found before any device is touched.  MCP_E_UNSUPPORTED: log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH.  Not built: a spending
 * rule with a cash-flow schedule, a glide path, floor protection, the drawdown, rebalancing, the overlay, GARCH, jumps, regimes,
 * filtered rows, the attribution, antithetic pairs, or at the mcp_launch_* level.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_spending(mcp_ctx *ctx, const mcp_params *prm, const mcp_spending *sp,
                          const float *mu, const float *chol,   /* Gaussian or Student-t draws ...                */
                          const mcp_bootstrap *boot,             /* ... or bootstrap rows: exactly one             */
                          const mcp_student_t *st,               /* NULL: Gaussian; needs mu and chol              */
                          const float *W, uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                          int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                          float *terminal_out,        /* NULL or host [K*n_paths] */
                          mcp_stats *stats_out,       /* [K] */
                          uint64_t *counts_out,       /* [K][2] {n_ruined, n_short} */
                          float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                          mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                          double *bands_out,          /* [H*K*L], NULL iff n_levels == 0 */
                          uint64_t *hz_counts_out,    /* [H*K][2], NULL iff n_horizons == 0 */
                          float *withdrawn_out,       /* NULL or host [K*n_paths] Y_T */
                          mcp_stats *wd_stats_out);   /* [K] */

/* The shifts of the moments (SPEC.md 5.16; host side, binary64 from the binary32 inputs): the rule on the mean path.  With m_k the
 * per-step mean of mcp_cashflow_pivots, A_0 = fl32(v0), wbar = (double)w0, Ybar = 0; per step A = A (1 + m_k) (a sum, a product), A =
 * A + (-wbar), Ybar = Ybar + wbar; at a review wbar' = wbar g, wbar = fmin(fmax(p max(A, 0), wbar' lo), wbar' hi) on the doubles of
 * the binary32 constants.  max(A, 0) / fl32(v0) - 1 after step n_steps into pivots_out[k] and after the steps of the n_horizons
 * horizons into hz_pivots_out[h*K + k] (n_horizons = 0: horizons and hz_pivots_out ignored); Ybar / fl32(v0) - 1 after step n_steps
 * into wd_pivots_out[k]; each 0 where it is not finite.  Exactly one of mu and boot. */
int mcp_spending_pivots(const mcp_params *prm, const mcp_spending *sp, const float *mu, const mcp_bootstrap *boot,
                        const float *W, int n_horizons, const int32_t *horizons, double *pivots_out /* [K] */,
                        double *hz_pivots_out /* NULL or [H*K] */, double *wd_pivots_out /* [K] */);

/* The five binary32 constants of the rule as the walk uses them: out = {p32, g32, lo32, hi32, w0}.  Checks sp and v0 as
 * mcp_simulate_spending does; touches no device. */
int mcp_spending_consts(const mcp_spending *sp, double v0, float *out /* [5] */);

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_SPEND_H */

/* mcport_voltarget.h -- volatility targeting for the path engine of libmcport.so (SPEC.md 4.19 / 5.19): the exposure to the risky
 * portfolio is target / estimated volatility, the estimate an EWMA of the path's own squared returns, the rest in cash or borrowed
 * up to a cap.  An extension of include/mcport.h: the entry points below are additive, detected by symbol, and MCP_ABI_VERSION stays
 * what mcport.h says.  C99-clean. */
#ifndef MCPORT_VOLTARGET_H
#define MCPORT_VOLTARGET_H

#include "mcport.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule (SPEC.md 4.19; simple compounding, binary32 with IEEE fminf / fmaxf, correctly rounded fma, sqrtf and division).  Per
 * path and portfolio the walk carries the value V from fl32(v0), the variance estimate s from s0_k and, without the drawdown, the
 * summed exposure Y from +0.  Step t = 0 .. n_steps - 1, on the step's portfolio return rho exactly as the call without targeting
 * forms it:
 *     e  = fminf(tgt / sqrtf(s), b)                  the exposure, decided before the step's return is seen
 *     E  = fl32(e V)
 *     u  = fma(V - E, rf, V)
 *     U  = fma(E, rho, u)
 *     D  = fmaxf(E - V, +0)                          the currency borrowed
 *     U  = fma(D, -sp, U)
 *     V' = (V > +0 and U > +0) ? U : +0              absorbing ruin, as SPEC.md 4.7
 *     Y' = Y + e                                     on every lane, ruined or not
 *     s' = fminf(fma(oml, fl32(rho rho), fl32(lam s)), 2^40)
 * with tgt, lam, b, rf, sp the binary32 roundings of target, decay, cap, rate and spread and oml = fl32(1 - (double)lam).  target > 0,
 * per step; decay in [0, 1]; cap > 0, a multiple of V (1: no leverage); rate > -1, per step; spread >= 0, per step, paid on top of
 * rate on what is borrowed; every rule holds before and after rounding.  s0: NULL, or n_portfolios finite values > 0; NULL takes
 * s0_k = fl32(sum_j (sum_i W[k,i] L[i,j])^2), binary64 from the binary32 inputs, i and j ascending -- w'Sigma w of the Gaussian part
 * -- which must come out finite and > 0.  target_value: NULL, or one finite value for the second count.  reserved must be 0. */
typedef struct {
    double        target, decay, cap, rate, spread;
    const double *s0;               /* NULL or [n_portfolios] */
    const double *target_value;     /* NULL or one value */
    int32_t       reserved;         /* must be 0 */
} mcp_vol_target;

/* mcp_simulate_garch / mcp_simulate_jumps with the rule above in the update of V: the draws, the drawdown (which sees V'), the
 * horizons, records and bands are those calls'.  gv NULL: no GARCH; st NULL: Gaussian draws; jp NULL: no jumps; all three NULL is
 * the Gaussian walk.  counts_out[k] = {#(V_T == +0), target_value ? #(V_T < fl32(*target_value)) : 0}; hz_counts_out[h*K + k] the
 * same for V_h.  Without the drawdown exposure_stats_out[k] is the record of x_Y = (double)Y_T - 1 (pivot 0, rf 0, sharpe 0: add 1 and
 * divide by n_steps for the path's average exposure) and exposure_out, when given, receives Y_T; with the drawdown the second array
 * of the call is the drawdown and there is no exposure record.  The moments are pivoted at SPEC.md 5.19 (mcp_vol_target_pivots).
 * With cap 1 and target 2^60 every V' is fma(V, rho, V) while the values stay positive: the stored values of the call without
 * targeting, bit for bit.  Argument errors (MCP_E_ARG: a NULL struct, counts_out or required output; a value that is not finite
 * before or after rounding to binary32 or outside its range; an s0 entry that is not finite and > 0, or a default that is not;
 * reserved != 0; exposure_out without exposure_stats_out; hz_counts_out NULL exactly when n_horizons == 0 is required; and every
 * rule of the draws' own structs) are found before any device is touched.  MCP_E_UNSUPPORTED: log compounding, MCP_FLAG_FOLD,
 * MCP_FLAG_NATIVE_MATH, the drawdown together with horizons, jumps together with gv or st, exposure_stats_out together with
 * dd_stats_out.  Not built: targeting on bootstrap or filtered rows, with regimes, rebalancing, cash flows, glide paths, floor
 * protection, spending rules or tolerance bands, with the overlay, the attribution or antithetic pairs, at the mcp_launch_* level or
 * in engine.PathEngine.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_vol_target(mcp_ctx *ctx, const mcp_params *prm, const mcp_vol_target *vt,
                            const mcp_garch *gv,             /* NULL: no GARCH                                  */
                            const mcp_student_t *st,         /* NULL: Gaussian draws                            */
                            const mcp_jumps *jp,             /* NULL: no jumps; not with gv or st               */
                            const float *mu, const float *chol, const float *W,
                            uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                            int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                            float *terminal_out,           /* NULL or host [K*n_paths] */
                            mcp_stats *stats_out,          /* [K] */
                            float *mdd_out,                /* NULL or host [K*n_paths] q of SPEC.md 4.2; needs dd_stats_out */
                            mcp_stats *dd_stats_out,       /* NULL: no drawdown; else [K] */
                            float *exposure_out,           /* NULL or host [K*n_paths] Y_T; needs exposure_stats_out */
                            mcp_stats *exposure_stats_out, /* [K], NULL exactly when dd_stats_out is not */
                            uint64_t *counts_out,          /* [K][2] {n_ruined, n_short} */
                            float *horizon_out,            /* NULL or host [H*K*n_paths], row h*K + k */
                            mcp_stats *hz_stats_out,       /* [H*K], NULL iff n_horizons == 0 */
                            double *bands_out,             /* [H*K*L], NULL iff n_levels == 0 */
                            uint64_t *hz_counts_out);      /* [H*K][2], NULL iff n_horizons == 0 */

/* The shifts of the moments of targeted paths (SPEC.md 5.19; host side, binary64 from the binary32 constants): with mu_k = sum_i
 * W_ki mu_i (i ascending), e_k = min(tgt / sqrt(s0_k), b) and g_k = 1 + rf + e_k (mu_k - rf) - sp max(e_k - 1, 0), c_k(h) = g_k^h - 1
 * after h steps; where g_k <= 0 or the result is not finite, the value of mcp_pivots at h steps.  h = n_steps into pivots_out[k], the
 * n_horizons horizons into hz_pivots_out[h*K + k] (n_horizons = 0: horizons and hz_pivots_out ignored). */
int mcp_vol_target_pivots(const mcp_params *prm, const mcp_vol_target *vt, const float *mu, const float *chol, const float *W,
                          int n_horizons, const int32_t *horizons, double *pivots_out /* [K] */,
                          double *hz_pivots_out /* NULL or [H*K] */);

/* The binary32 constants of a request as the kernel uses them: out[0 .. 5] = {tgt, lam, oml, b, rf, sp}, out[6 + k] = s0_k. */
int mcp_vol_target_consts(const mcp_params *prm, const mcp_vol_target *vt, const float *chol, const float *W,
                          float *out /* [6 + K] */);

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_VOLTARGET_H */

/* mcport_protect.h -- floor protection for the path engine of libmcport.so (SPEC.md 4.15 / 5.15): CPPI with an exposure cap and
 * an optional drawdown ratchet (TIPP).  An extension of include/mcport.h: the entry points below are additive, detected by symbol,
 * and MCP_ABI_VERSION stays what mcport.h says.  C99-clean. */
#ifndef MCPORT_PROTECT_H
#define MCPORT_PROTECT_H

#include "mcport.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule (SPEC.md 4.15; simple compounding, binary32 with IEEE fminf / fmaxf and correctly rounded fma).  Per path and portfolio
 * the walk carries the value V and its peak M, both from fl32(v0).  Step t = 0 .. n_steps - 1, on the step's portfolio return rho
 * exactly as the call without protection forms it:
 *     F  = fmaxf(S_t, fl32(theta M))
 *     C  = V - F
 *     E  = fmaxf(fminf(fl32(m C), fl32(b V)), +0)       the currency held in the risky portfolio
 *     u  = fma(V - E, rf, V)
 *     V' = fma(E, rho, u)
 *     M' = fmaxf(M, V')
 * with m, b, rf, theta the binary32 roundings of multiplier, cap, rate and ratchet.  floor: the schedule S_0 .. S_T, n_steps + 1
 * finite values >= +0 (mcp_protect_floor builds a compounding one); multiplier >= 0; cap > 0, a multiple of V (1: no leverage);
 * rate > -1, per step; ratchet in [0, 1) (0: no ratchet).  target: NULL, or one finite value for the second count.  reserved must
 * be 0. */
typedef struct {
    const float  *floor;            /* [n_steps + 1] */
    double        multiplier, cap, rate, ratchet;
    const double *target;           /* NULL or one value */
    int32_t       reserved;         /* must be 0 */
} mcp_protect;

/* mcp_simulate_garch / mcp_simulate_jumps with the rule above in the update of V: the draws, the drawdown (which sees V'), the
 * horizons, records and bands are those calls'.  gv NULL: no GARCH; st NULL: Gaussian draws; jp NULL: no jumps; all three NULL is
 * the Gaussian walk.  counts_out[k] = {#(V_T < S_T), target ? #(V_T < fl32(*target)) : 0}; hz_counts_out[h*K + k] the same for V_h
 * against S_h.  The moments are pivoted at SPEC.md 5.15 (mcp_protect_pivots).  With floor = 0, ratchet 0, cap 1 and multiplier >= 1
 * every V' is fma(V, rho, V): the stored values of the call without protection, bit for bit.  Argument errors (MCP_E_ARG: a NULL
 * struct, floor, counts_out or required output; a value that is not finite before or after rounding to binary32; a negative floor
 * entry; multiplier < 0; cap <= 0; rate <= -1; ratchet outside [0, 1); reserved != 0; hz_counts_out NULL exactly when n_horizons ==
 * 0 is required; and every rule of the draws' own structs) are found before any device is touched.  MCP_E_UNSUPPORTED: log
 * compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH, the drawdown together with horizons, jumps together with gv or st.  Not built:
 * protection on bootstrap or filtered rows, with regimes, rebalancing, cash flows, glide paths, the overlay, the attribution or
 * antithetic pairs, or at the mcp_launch_* level.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_protected(mcp_ctx *ctx, const mcp_params *prm, const mcp_protect *pt,
                           const mcp_garch *gv,             /* NULL: no GARCH                                  */
                           const mcp_student_t *st,         /* NULL: Gaussian draws                            */
                           const mcp_jumps *jp,             /* NULL: no jumps; not with gv or st               */
                           const float *mu, const float *chol, const float *W,
                           uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                           int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                           float *terminal_out,        /* NULL or host [K*n_paths] */
                           mcp_stats *stats_out,       /* [K] */
                           float *mdd_out,             /* NULL or host [K*n_paths] q of SPEC.md 4.2; needs dd_stats_out */
                           mcp_stats *dd_stats_out,    /* NULL: no drawdown; else [K] */
                           uint64_t *counts_out,       /* [K][2] {n_gap, n_short} */
                           float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                           mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                           double *bands_out,          /* [H*K*L], NULL iff n_levels == 0 */
                           uint64_t *hz_counts_out);   /* [H*K][2], NULL iff n_horizons == 0 */

/* The shifts of the moments of protected paths (SPEC.md 5.15; host side, binary64 from the binary32 inputs): with mu_k = sum_i
 * W_ki mu_i (i ascending) and g_k = 1 + rf + m (mu_k - rf), c_k(h) = (S_h + (v0 - S_0) g_k^h) / v0 - 1 after h steps; where g_k <= 0
 * or the result is not finite, the value of mcp_pivots at h steps.  h = n_steps into pivots_out[k], the n_horizons horizons into
 * hz_pivots_out[h*K + k] (n_horizons = 0: horizons and hz_pivots_out ignored). */
int mcp_protect_pivots(const mcp_params *prm, const mcp_protect *pt, const float *mu, const float *W,
                       int n_horizons, const int32_t *horizons, double *pivots_out /* [K] */,
                       double *hz_pivots_out /* NULL or [H*K] */);

/* A floor that compounds at a per-step rate: out[0] = fl32(floor0), out[t + 1] = fma(out[t], fl32(rate), out[t]), n_steps + 1 values.
 * MCP_E_ARG: floor0 or rate not finite (before or after rounding), floor0 < 0, rate <= -1, n_steps < 1, out NULL, or a schedule that
 * overflows binary32. */
int mcp_protect_floor(double floor0, double rate, int n_steps, float *out /* [n_steps + 1] */);

#ifdef __cplusplus
}
#endif

#endif /* MCPORT_PROTECT_H */

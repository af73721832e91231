/*
 * mcport.h -- C ABI of libmcport.so, the MI355X (gfx950) Monte Carlo portfolio path engine.
 *
 * The reference (mohammadmarghzari/monte-carlo-portfolio, app.py) has no FFI / plugin interface: it
 * is a flat Streamlit script.  This ABI is therefore the boundary SURVEY.md section 8(b) defines; each
 * entry point names the reference lines whose role it takes over.  Bound from Python with ctypes
 * (monte_carlo_portfolio_amd/_ffi.py); INTEGRATION.md shows the stub a maintainer of app.py would add.
 *
 * Conventions: every function returns 0 on success or a negative MCP_E_* code and never throws;
 * mcp_last_error() returns a thread-local message.  Host pointers are caller-owned and only need to
 * stay valid for the call.  "d_" pointers are DEVICE pointers (hipMalloc / torch CUDA tensors) and
 * "stream" is a hipStream_t passed as void* (NULL = the default stream); the *_launch_* functions only
 * enqueue work on that stream, they never allocate, synchronise or copy to the host, so they may be
 * captured in a hipGraph.
 */
#ifndef MCPORT_H
#define MCPORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCP_ABI_VERSION 4        /* 4: + mcp_simulate_drawdown, mcp_launch_paths_drawdown (additive); + mcp_simulate_horizons,
                                    mcp_launch_paths_horizons, mcp_percentile_rank_q (additive, detected by symbol);
                                    + mcp_simulate_bootstrap[_horizons], mcp_bootstrap_pivots (additive, detected by symbol);
                                    + mcp_simulate_rebalanced, mcp_rebalance_pivots (additive, detected by symbol);
                                    + mcp_simulate_student_t (additive, detected by symbol);
                                    + mcp_simulate_overlay, mcp_overlay_pivots (additive, detected by symbol);
                                    + mcp_simulate_garch (additive, detected by symbol);
                                    + mcp_simulate_attribution (additive, detected by symbol);
                                    + mcp_simulate_antithetic (additive, detected by symbol);
                                    + mcp_simulate_filtered, mcp_filtered_pivots (additive, detected by symbol);
                                    + mcp_simulate_jumps, mcp_jump_consts (additive, detected by symbol);
                                    + mcp_simulate_regimes, mcp_regime_consts, mcp_regime_pivots (additive, detected by symbol);
                                    + mcp_simulate_glide, mcp_glide_pivots (additive, detected by symbol) */
#define MCP_MAX_ASSETS 64        /* thread-per-path kernels are instantiated for N4 = 4..64 */
#define MCP_SELECT_BINS 2048     /* radix-select digit: 11 + 11 + 10 bits */
#define MCP_MAX_HORIZONS 64      /* mcp_simulate_horizons: horizon steps per call */
#define MCP_MAX_LEVELS 16        /* mcp_simulate_horizons: band levels per call */
#define MCP_MAX_BOOT_ROWS (1 << 20) /* mcp_simulate_bootstrap, mcp_simulate_filtered: observed return rows per call */
#define MCP_MAX_OVERLAY_ROWS 8   /* mcp_simulate_overlay: option rows per asset */
#define MCP_MAX_T_DOF 32         /* mcp_simulate_student_t: degrees of freedom in [3, MCP_MAX_T_DOF] */
#define MCP_MAX_ATTR_PORTFOLIOS 16 /* mcp_simulate_attribution: portfolios per call */
#define MCP_MAX_JUMPS 8          /* mcp_simulate_jumps: market jumps per path-step (the Poisson count is truncated there) */
#define MCP_MAX_GLIDE 64         /* mcp_simulate_glide: breaks (changes of the target weights) per call */

enum {
    MCP_OK = 0,
    MCP_E_ARG = -1,        /* bad argument (shape, NULL, range) */
    MCP_E_NODEVICE = -2,   /* no HIP device visible (the product has no CPU fallback) */
    MCP_E_NOMEM = -3,
    MCP_E_UNSUPPORTED = -4,
    MCP_E_HIP = -5,        /* a HIP runtime call or kernel launch failed; mcp_last_error() has the call and the HIP error string */
    MCP_E_COMM = -6        /* RCCL could not be loaded or a collective failed (multi-device contexts only) */
};

enum {
    MCP_COMPOUND_SIMPLE = 0,   /* V <- V*(1+rho): np.cumprod(1+r) idiom, app.py:249, app.py:253 */
    MCP_COMPOUND_LOG = 1       /* S <- S+rho, x = expm1(S) */
};

enum {
    MCP_FLAG_NATIVE_MATH = 1,  /* normals by Box-Muller on the v_log/v_sqrt/v_sin/v_cos hardware approximations instead
                                  of the spec's inverse-CDF table: statistically equivalent draws from the same Philox
                                  stream, NOT comparable to the oracle value by value */
    MCP_FLAG_FOLD = 2,         /* one portfolio only: rho = w.mu + (L^T w).z with L^T w folded on the host (SPEC.md 4.1)
                                  instead of the triangular GEMV + weight dot.  A separately reported fast path: same
                                  normals, other rounding than the unfolded recurrence (agrees to ~1e-7 relative) */
    MCP_FLAG_SHARD_PORTFOLIOS = 4  /* multi-device contexts: every device walks ALL paths for its slice of the K weight
                                  vectors (BASELINE configs[4]; no collective at all) instead of sharding the path range */
};

typedef struct mcp_ctx mcp_ctx;

/* Problem description.  mu/Sigma play the role of app.py:679-680 (per STEP, i.e. already divided by
 * the annualisation factor), W rows are portfolios as drawn at app.py:702. */
typedef struct {
    int32_t n_assets;       /* N in [1, MCP_MAX_ASSETS] */
    int32_t n_steps;        /* T >= 0 */
    int32_t n_portfolios;   /* K >= 1; all K portfolios see the same normals (common random numbers) */
    int32_t compounding;    /* MCP_COMPOUND_* */
    int32_t flags;          /* MCP_FLAG_* */
    int32_t reserved;
    double v0;              /* initial value; rounded to binary32 on the device */
    double alpha;           /* VaR/CVaR confidence, reference default 0.95 (app.py:258, app.py:684) */
    double rf;              /* risk-free rate over the horizon, subtracted as at app.py:711 */
} mcp_params;

/* Per-portfolio result on x = V_T/V0 - 1 (or expm1(S_T)), semantics of app.py:258-263, app.py:711. */
typedef struct {
    uint64_t n;             /* number of paths */
    uint64_t n_tail;        /* #{x <= VaR} */
    double mean;
    double m2;              /* sum (x - mean)^2 */
    double std;             /* ddof = 1, as np.std(ddof=1) at app.py:234 */
    double sharpe;          /* (mean - rf)/std, 0 if std == 0 (app.py:711) */
    double var;             /* np.percentile(x, (1-alpha)*100), linear interpolation (app.py:259) */
    double cvar;            /* mean of x[x <= var], var if empty (app.py:263) */
    double min, max;
    double sum_tail;        /* sum of x[x <= var] */
    double x_lo, x_hi;      /* the two order statistics np.percentile interpolates between */
} mcp_stats;

/* Raw sufficient statistics of one portfolio on one device: what ranks exchange (one all-gather, merged in rank
 * order: SUM on n, sum, sumsq, below; MIN on min; MAX on max).  SHIFTED sums: sum = sum (x - pivot),
 * sumsq = sum (x - pivot)^2 with the same pivot on every rank (mcp_pivots: the analytic mean of x), so that
 * mean = pivot + sum/n and sum (x - mean)^2 = sumsq - sum^2/n do not cancel for a low-volatility portfolio
 * (np.std(ddof=1), app.py:234, is two-pass).  `below` = this device's paths that sort strictly below the bucket of the low
 * order statistic of the radix select (the CVaR tail, app.py:261-263), as sum (V - v0) (simple compounding;
 * sum x = below / v0) or sum x (log). */
typedef struct {
    double n, sum, sumsq, min, max, below;
    double pivot;
    double pad;
} mcp_record;

int mcp_abi_version(void);
int mcp_device_count(void);                 /* 0 when no GPU is visible; never fails */
const char *mcp_last_error(void);

/* ---- host-level API: NumPy in, NumPy out (replaces the script lines app.py:699-717 for a simulated
 *      terminal distribution).  Owns its device buffers; calls on one ctx are serialised. ---------- */
int mcp_ctx_create(int device, mcp_ctx **out);
/* one context over `ndev` devices, one stream per device, the path range (or, with
 * MCP_FLAG_SHARD_PORTFOLIOS, the weight matrix) sharded over them.  Distinct devices exchange through RCCL
 * (ncclCommInitAll; librccl is loaded at run time).  If librccl cannot be loaded or initialised -- or MCP_EXCHANGE=p2p is
 * set -- and the first device has peer access to the others (at most 8 devices), the exchange runs as a kernel of the
 * first device over peer access instead; MCP_E_COMM if neither is possible.  A device listed more than once holds
 * several logical shards that exchange through that same kernel (what a one-GPU box can exercise).  ndev = 1 is
 * mcp_ctx_create.  Results equal the one-device results: order statistics, counts and argmax exactly, fp64 sums up to
 * association. */
int mcp_ctx_create_multi(const int *devices, int ndev, mcp_ctx **out);
int mcp_ctx_device_count(const mcp_ctx *ctx);   /* number of shards of the context */
/* How the shards of the context exchange histograms and records.  The communicator (or the peer mapping) is set up on the
 * first path-sharded mcp_simulate, not at creation: a portfolio-sharded call (MCP_FLAG_SHARD_PORTFOLIOS) needs neither.
 * MCP_EXCHANGE_UNSET until then.  When RCCL could not be used and the context fell back to the peer-access kernel,
 * mcp_ctx_exchange_note() says why (empty string otherwise). */
enum {
    MCP_EXCHANGE_UNSET = 0,    /* nothing exchanged yet */
    MCP_EXCHANGE_NONE = 1,     /* one shard */
    MCP_EXCHANGE_RCCL = 2,     /* distinct devices, ncclAllReduce / ncclAllGather over xGMI */
    MCP_EXCHANGE_KERNEL = 3,   /* logical shards of ONE device: a kernel sums the shards' buffers */
    MCP_EXCHANGE_P2P = 4       /* distinct devices, RCCL unavailable (or MCP_EXCHANGE=p2p): the same kernel over peer access */
};
int mcp_ctx_exchange_mode(const mcp_ctx *ctx);
const char *mcp_ctx_exchange_note(const mcp_ctx *ctx);
void mcp_ctx_destroy(mcp_ctx *ctx);

/* Large K: the terminal values are produced and reduced in tiles of portfolios so that at most about
 * `bytes` of V_T are resident per device (default 8 GiB; SURVEY.md section 8a N2: V_T[K x paths] is never
 * materialised whole unless terminal_out asks for it). */
int mcp_ctx_set_terminal_budget(mcp_ctx *ctx, size_t bytes);

int mcp_simulate(mcp_ctx *ctx, const mcp_params *prm,
                 const float *mu,      /* [N] */
                 const float *chol,    /* [N*N] row-major, lower triangular (upper ignored) */
                 const float *W,       /* [K*N] */
                 uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                 float *terminal_out,  /* NULL or host [K*n_paths] */
                 mcp_stats *stats_out  /* [K] */);

/* mcp_simulate plus the max drawdown of every path (SPEC.md 4.2) reduced per portfolio as the reference's VaR / CVaR reduce
 * a sample (SPEC.md 5.1): dd_stats_out[k] is an mcp_stats over mdd (var = DaR, cvar = CDaR, n_tail, mean, std, min = worst,
 * max = best, x_lo / x_hi; sharpe = 0).  mdd_out: NULL or host [K*n_paths] floats, the kernels' raw per-path q (simple
 * compounding: mdd = q - 1) or d (log: mdd = expm1(d)).  terminal_out / stats_out are what mcp_simulate returns, with the
 * same V_T; for K >= 17 the moments (mean, m2, std, sharpe) agree with mcp_simulate's to fp64 association only, everything
 * else exactly.  Costs: the path kernels keep the running peak in registers (one IEEE division per step and portfolio),
 * K >= 17 runs as passes of the 8-portfolio kernel instead of the MFMA sweep kernels, a second select pipeline reduces the
 * drawdowns, and the terminal budget counts 8 B per path and portfolio.  MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH:
 * MCP_E_UNSUPPORTED. */
int mcp_simulate_drawdown(mcp_ctx *ctx, const mcp_params *prm, const float *mu, const float *chol, const float *W,
                          uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                          float *terminal_out,     /* NULL or host [K*n_paths] */
                          mcp_stats *stats_out,    /* [K] */
                          float *mdd_out,          /* NULL or host [K*n_paths]: q or d */
                          mcp_stats *dd_stats_out  /* [K] */);

/* mcp_simulate plus the values at intermediate horizons (SPEC.md 4.3) and their statistics and bands (SPEC.md 5.2).
 * horizons: n_horizons in [1, MCP_MAX_HORIZONS] strictly increasing steps in [1, n_steps] (n_steps itself allowed); the
 * value after step h of this walk is bit for bit the terminal value of the same call with n_steps = h.  levels: n_levels in
 * [0, MCP_MAX_LEVELS] percentages in [0, 100].  Per (horizon h, portfolio k), over x_h = V_h/v0 - 1 (simple) or expm1(S_h)
 * (log): hz_stats_out[h*K + k] is an mcp_stats record at the call's alpha (pivot of n_steps = h, sharpe = 0), and
 * bands_out[(h*K + k)*L + l] = np.percentile(x_h, levels[l]) bit for bit.  horizon_out: NULL or host [H*K*n_paths] floats,
 * row h*K + k, the raw V_h / S_h.  terminal_out / stats_out are what mcp_simulate returns, with the same V_T; for K >= 17 the
 * moments agree with mcp_simulate's to fp64 association only, everything else exactly.  Costs: one 4 B store per path,
 * portfolio and horizon; K >= 17 runs as passes of the 8-portfolio kernel; 1 + L selects over the H*K rows; the terminal
 * budget counts 4 (1 + H) B per path and portfolio.  Argument errors (MCP_E_ARG) are found before any device is touched;
 * MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED. */
int mcp_simulate_horizons(mcp_ctx *ctx, const mcp_params *prm, const float *mu, const float *chol, const float *W,
                          uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                          int n_horizons, const int32_t *horizons,
                          int n_levels, const double *levels,
                          float *terminal_out,        /* NULL or host [K*n_paths] */
                          mcp_stats *stats_out,       /* [K] */
                          float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                          mcp_stats *hz_stats_out,    /* [H*K] */
                          double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */

/* Stationary block bootstrap of observed return rows (Politis & Romano 1994; SPEC.md 2.1 / 4.4 / 5.3).  rows: [n_rows * N]
 * row-major binary32 (returns_df.values, app.py:667, rounded to nearest by the caller), every entry finite, 1 <= n_rows <=
 * MCP_MAX_BOOT_ROWS.  mean_block: the mean block length b in [1, +inf]: b = 1 draws every step's row independently, b = +inf
 * walks consecutive rows (circularly) from one random start. */
typedef struct {
    const float *rows;      /* [n_rows * N] */
    int32_t n_rows;
    int32_t reserved;
    double mean_block;
} mcp_bootstrap;

/* mcp_simulate on bootstrap paths: step t of path p uses row j_t of the table (SPEC.md 2.1, one Philox block per step on a
 * counter stream of its own), rho_k = w_k . row, and V or S is updated as in SPEC.md 4 (SPEC.md 4.4).  All K portfolios see
 * the same rows.  stats_out / terminal_out as mcp_simulate, with the moments pivoted at SPEC.md 5.3.  The n_assets of prm is the
 * row width.  Argument errors (MCP_E_ARG) are found before any device is touched; MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH:
 * MCP_E_UNSUPPORTED.  Costs: the row table is uploaded once per device and call (4 N4 B per row); it is read from LDS when
 * n_rows * ceil(N/4) <= 1088 (N = 16: 272 rows), else from global memory; K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_bootstrap(mcp_ctx *ctx, const mcp_params *prm, const mcp_bootstrap *boot, const float *W, uint64_t seed,
                           uint64_t path_begin, uint64_t n_paths, float *terminal_out, mcp_stats *stats_out);
/* mcp_simulate_horizons on bootstrap paths: the horizons, records and bands of SPEC.md 4.3 / 5.2 over the walk of
 * mcp_simulate_bootstrap (the value after step h is bit for bit the terminal value of the same call with n_steps = h). */
int mcp_simulate_bootstrap_horizons(mcp_ctx *ctx, const mcp_params *prm, const mcp_bootstrap *boot, const float *W,
                                    uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                                    int n_horizons, const int32_t *horizons,
                                    int n_levels, const double *levels,
                                    float *terminal_out,        /* NULL or host [K*n_paths] */
                                    mcp_stats *stats_out,       /* [K] */
                                    float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                                    mcp_stats *hz_stats_out,    /* [H*K] */
                                    double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */
/* The shift of the moments of bootstrap paths (SPEC.md 5.3; host side, binary64): with rho_jk = sum_i W[k,i] rows[j,i],
 * m_k = sum_j rho_jk / R and s2_k = sum_j (rho_jk - m_k)^2 / R,
 *   simple: c_k = (1 + m_k)^T - 1 (as expm1(T log1p(m_k)), 0 if m_k <= -1)     log: c_k = expm1(T (m_k + s2_k / 2)).
 * 0 where it is not finite. */
int mcp_bootstrap_pivots(const mcp_params *prm, const mcp_bootstrap *boot, const float *W, double *pivots_out /* [K] */);

/* Buy-and-hold and periodic rebalancing (SPEC.md 4.5 / 5.4).  period m >= 0: the portfolio is traded back to its weights after
 * every step s with s mod m == 0 and s < T; m = 0 (or m >= T) is buy-and-hold.  cost: the proportional cost kappa in [0, 1) of
 * the fraction traded, paid out of the portfolio.  reserved must be 0. */
typedef struct {
    int32_t period;
    int32_t reserved;
    double cost;
} mcp_rebalance;

/* mcp_simulate / mcp_simulate_horizons / mcp_simulate_bootstrap[_horizons] with the weights held between rebalance dates
 * instead of kept constant (SPEC.md 4.5; simple compounding only).  Draws: exactly one source -- mu and chol (SPEC.md 2-4,
 * boot NULL) or boot (SPEC.md 2.1 / 4.4, mu and chol NULL).  n_horizons = 0: no horizons (horizons ignored, n_levels = 0,
 * horizon_out, hz_stats_out and bands_out NULL); otherwise the horizons, records and bands of mcp_simulate_horizons, V_h taken
 * before any trade of step h.  Period 1 without cost is bit for bit the constant-weight call.  The moments are pivoted at
 * SPEC.md 5.4.  Argument errors (MCP_E_ARG) are found before any device is touched; log compounding, MCP_FLAG_FOLD,
 * MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_rebalanced(mcp_ctx *ctx, const mcp_params *prm, const mcp_rebalance *reb,
                            const float *mu, const float *chol,   /* Gaussian draws ...                       */
                            const mcp_bootstrap *boot,             /* ... or bootstrap draws: exactly one        */
                            const float *W, uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                            int n_horizons, const int32_t *horizons,
                            int n_levels, const double *levels,
                            float *terminal_out,        /* NULL or host [K*n_paths] */
                            mcp_stats *stats_out,       /* [K] */
                            float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                            mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                            double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */
/* The shift of the moments of rebalanced paths at prm->n_steps (SPEC.md 5.4; host side, binary64): with the segments l_1..l_S
 * between the rebalance dates, mu_i = mu[i] (Gaussian) or the mean of column i of the rows (bootstrap; exactly one of mu and boot),
 * a_i(l) = expm1(l log1p(mu_i)), g_s = sum_i W[k,i] a_i(l_s):  c_k = expm1(sum_s log1p(g_s)), 0 where it is not finite.  The cost
 * is ignored. */
int mcp_rebalance_pivots(const mcp_params *prm, const mcp_rebalance *reb, const float *mu, const mcp_bootstrap *boot,
                         const float *W, double *pivots_out /* [K] */);

/* Fat-tailed draws: the multivariate Student-t with nu degrees of freedom, a normal variance mixture (SPEC.md 2.2 / 4.6).  dof:
 * an integer nu in [3, MCP_MAX_T_DOF]; reserved must be 0. */
typedef struct {
    int32_t dof;
    int32_t reserved;
} mcp_student_t;

/* mcp_simulate / mcp_simulate_drawdown / mcp_simulate_horizons with every step's normals z scaled by s = sqrt((nu - 2) / chi),
 * chi the sum of nu squared normals of a counter stream of its own (SPEC.md 2.2 / 4.6; simple compounding only): r = mu + L s z
 * has the mean mu and the covariance L L^T of the Gaussian call, fat tails (excess kurtosis 6 / (nu - 4) for nu > 4) and
 * assets that crash together.  The asset normals are the Gaussian call's own (common random numbers with the same seed).
 * dd_stats_out non-NULL: the drawdown of mcp_simulate_drawdown (mdd_out NULL or host [K*n_paths] q); n_horizons > 0: the
 * horizons, records and bands of mcp_simulate_horizons (n_horizons = 0: horizons ignored, n_levels = 0, horizon_out,
 * hz_stats_out and bands_out NULL); not both (MCP_E_UNSUPPORTED).  The moments are pivoted as mcp_pivots (SPEC.md 5).
 * Argument errors (MCP_E_ARG: nu out of range, reserved != 0, n_steps * ceil(nu/4) >= 2^32, NULL pointers) are found before
 * any device is touched; log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.  Costs: ceil(nu/4) more
 * Philox blocks and normals per step; K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_student_t(mcp_ctx *ctx, const mcp_params *prm, const mcp_student_t *st,
                           const float *mu, const float *chol, const float *W,
                           uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                           int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                           float *terminal_out,        /* NULL or host [K*n_paths] */
                           mcp_stats *stats_out,       /* [K] */
                           float *mdd_out,             /* NULL or host [K*n_paths]; needs dd_stats_out */
                           mcp_stats *dd_stats_out,    /* [K], or NULL: no drawdown */
                           float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                           mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                           double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */

/* Volatility clustering: a scalar GARCH(1,1) on the covariance, Sigma_t = h_t Sigma (SPEC.md 4.9 / 5.8).  One variance ratio h per
 * path, shared by all assets and portfolios: h_{t+1} = (1 - alpha - beta) + alpha (eps_t' Sigma^-1 eps_t / N) + beta h_t from h0, in
 * units of the unconditional variance.  alpha, beta, h0: finite, rounded to binary32 (a, b, g) with a >= 0, b >= 0, a + b < 1 and
 * g > 0; reserved must be 0. */
typedef struct {
    double alpha, beta, h0;
    uint64_t reserved;
} mcp_garch;

/* mcp_simulate / mcp_simulate_drawdown / mcp_simulate_horizons / mcp_simulate_student_t with every step's normals scaled by
 * u = sqrt(h) (st: u = s sqrt(h), s of SPEC.md 2.2) and h updated from the step's scaled normals (SPEC.md 4.9; simple compounding
 * only): the conditional mean of every step is mu, so the moments are pivoted as mcp_pivots; with h0 = 1 the per-step covariance is
 * the Gaussian call's, with h0 != 1 it reverts to it as 1 + (alpha + beta)^t (h0 - 1).  alpha = 0 and h0 = 1 is the call without
 * GARCH bit for bit.  st NULL: Gaussian draws.  The horizon inputs and the outputs are those of mcp_simulate_student_t (the
 * drawdown or the horizons, not both: MCP_E_UNSUPPORTED).  Argument errors (MCP_E_ARG: the rules above, those of st, NULL pointers)
 * are found before any device is touched; log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.  Costs: one
 * square root, N + 2 fused multiply-adds and N multiplies per path-step; K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_garch(mcp_ctx *ctx, const mcp_params *prm, const mcp_garch *g,
                       const mcp_student_t *st,            /* NULL: Gaussian draws */
                       const float *mu, const float *chol, const float *W,
                       uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                       int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                       float *terminal_out,        /* NULL or host [K*n_paths] */
                       mcp_stats *stats_out,       /* [K] */
                       float *mdd_out,             /* NULL or host [K*n_paths]; needs dd_stats_out */
                       mcp_stats *dd_stats_out,    /* [K], or NULL: no drawdown */
                       float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                       mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                       double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */

/* Filtered historical simulation (Barone-Adesi, Giannopoulos & Vosper 1999; SPEC.md 2.4 / 4.11 / 5.11): the bootstrap on rows that
 * were de-volatilised with a fitted GARCH(1,1) variance path, every draw re-scaled by the path's own simulated variance ratio.
 * mu: [N] the level the residuals are added to; resid: [n_rows * N] row-major residual rows E; shock: [n_rows] the rows' shocks
 * s_j >= 0 (the row's Mahalanobis shock over its fitted variance ratio); all binary32 and finite, 1 <= n_rows <= MCP_MAX_BOOT_ROWS.
 * mean_block: the mean block length b in [1, +inf] of mcp_bootstrap (b = 1: classical FHS).  reserved must be 0. */
typedef struct {
    const float *mu, *resid, *shock;
    int32_t n_rows;
    int32_t reserved;
    double mean_block;
} mcp_filtered;

/* mcp_simulate_bootstrap[_horizons] on filtered rows (SPEC.md 4.11; simple compounding only): step t of path p draws the row j_t
 * of SPEC.md 2.1, r_i = fma(sqrt(h), E[j_t, i], mu_i), rho_k = w_k . r, V = fma(V, rho_k, V), and then
 * h = min(fma(b, h, fma(a, fl32(h s[j_t]), omega)), 2^40) from h = g, with (a, b, g, omega) of the mcp_garch triple as in SPEC.md 4.9.
 * alpha = 0 and h0 = 1 is mcp_simulate_bootstrap on the rows fl32(E + mu) bit for bit.  n_horizons = 0: no horizons (horizons ignored,
 * n_levels = 0, horizon_out, hz_stats_out and bands_out NULL); otherwise the horizons, records and bands of mcp_simulate_horizons.
 * The moments are pivoted at SPEC.md 5.11.  Argument errors (MCP_E_ARG: a NULL struct or member, n_rows out of range, reserved != 0,
 * mean_block < 1 or NaN, a non-finite entry, a negative shock -- the message names the array and the first offending index -- and the
 * rules of g) are found before any device is touched; log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.
 * Costs: the rows and shocks are uploaded once per device and call (4 N4 + 4 B per row); they are read from LDS when
 * n_rows * ceil(N/4) + ceil(n_rows/4) <= 1088 (N = 16: 256 rows), else from global memory; one square root and N4 + 3 fused
 * multiply-adds or multiplies per path-step on top of the bootstrap; K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_filtered(mcp_ctx *ctx, const mcp_params *prm, const mcp_filtered *filt, const mcp_garch *g, const float *W,
                          uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                          int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                          float *terminal_out,        /* NULL or host [K*n_paths] */
                          mcp_stats *stats_out,       /* [K] */
                          float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                          mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                          double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */
/* The shift of the moments of filtered paths at prm->n_steps (SPEC.md 5.11; host side, binary64): with e_i the mean of column i of
 * resid (rows ascending), m_k = sum_i W[k,i] (mu_i + e_i): c_k = expm1(T log1p(m_k)), 0 if m_k <= -1 or where it is not finite. */
int mcp_filtered_pivots(const mcp_params *prm, const mcp_filtered *filt, const float *W, double *pivots_out /* [K] */);

/* Merton jump-diffusion (Merton 1976; SPEC.md 2.5 / 4.12 / 5.12): on top of the Gaussian step every path-step takes a compound-Poisson
 * market jump J = sum of n normal(mean, std^2) jumps, n ~ Poisson(intensity) truncated at MCP_MAX_JUMPS, that asset i takes part in
 * through its loading: r_i = mu'_i + b_i J + (L z)_i.  intensity: expected jumps per step, in [0, 1]; mean, std >= 0: of one jump, rounded
 * to binary32; loading: [N] binary32 (NULL: all ones).  Everything finite, before and after rounding to binary32; reserved must be 0. */
typedef struct {
    double intensity, mean, std;
    const float *loading;
    int32_t reserved;
} mcp_jumps;

/* mcp_simulate / mcp_simulate_drawdown / mcp_simulate_horizons with the market jump of SPEC.md 2.5 added to every step (simple
 * compounding only): one more Philox block per path-step on counter stream 3 gives the count n (uint32 compares of its first word
 * against the thresholds of mcp_jump_consts) and the size J = fma(fl32(sqrt(n) s32), Z(second word), fl32(n m32)); row i of the
 * step starts at fma(b_i, J, mu'_i) with mu' the compensated drift of mcp_jump_consts, so the mean of every step stays mu and
 * the moments are pivoted as mcp_pivots on mu.  chol is the DIFFUSIVE factor: the per-step covariance is L L' + Var(J) b b'.  The
 * asset normals are those of the call without jumps (common random numbers); intensity = 0, mean = std = 0 or loading = 0 is that
 * call bit for bit for a drift without zero entries.  The horizon inputs and the outputs are those of mcp_simulate_garch (the
 * drawdown or the horizons, not both: MCP_E_UNSUPPORTED).  Argument errors (MCP_E_ARG: the rules above, NULL pointers) are found
 * before any device is touched; log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.  Not built: jumps with
 * Student-t draws, GARCH, bootstrap or filtered rows, rebalancing, cash flows, the overlay, the attribution or antithetic pairs, and
 * at the mcp_launch_paths* level.  Costs: one Philox block, one normal, 8 compares and N4/2 packed fused multiply-adds per path-step;
 * the loadings are uploaded once per device and tile behind the packed parameters; K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_jumps(mcp_ctx *ctx, const mcp_params *prm, const mcp_jumps *j,
                       const float *mu, const float *chol, const float *W,
                       uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                       int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                       float *terminal_out,        /* NULL or host [K*n_paths] */
                       mcp_stats *stats_out,       /* [K] */
                       float *mdd_out,             /* NULL or host [K*n_paths]; needs dd_stats_out */
                       mcp_stats *dd_stats_out,    /* [K], or NULL: no drawdown */
                       float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                       mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                       double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */
/* The host constants of a jump request (SPEC.md 2.5; no device is touched): thr_out[k-1] = floor(2^32 P(Poisson(intensity) >= k)) for
 * k = 1 .. MCP_MAX_JUMPS (binary64, libm exp), *mean_count_out = sum_k thr_k / 2^32 -- the exact mean of the count the kernel draws
 * -- and, when drift_out is not NULL, the compensated drift mu'_i = fl32(mu_i - b_i fl32(mean) mean_count) of the [n_assets] drift
 * mu (mu_i itself where b_i or the product is 0). */
int mcp_jump_consts(const mcp_jumps *j, int n_assets, const float *mu,
                    uint32_t *thr_out /* [MCP_MAX_JUMPS] */, double *mean_count_out, float *drift_out /* NULL or [n_assets] */);

/* Two-regime Markov switching (Hamilton 1989; SPEC.md 2.6 / 4.13 / 5.13): every path carries a regime s_t in {0 (calm), 1 (crisis)}
 * that moves once per step with P(0 -> 1) = p01 and P(1 -> 0) = p10, and step t draws r = mu^(s_t) + L^(s_t) z: the call's mu and
 * chol are regime 0, mu1 [N] and chol1 [N*N, lower Cholesky factor, row-major] regime 1.  start = P(regime 1 in step 0).  Everything
 * finite, the three probabilities in [0, 1], no NULL pointer, reserved 0. */
typedef struct {
    double p01, p10, start;
    const float *mu1;
    const float *chol1;
    int32_t reserved;
} mcp_regimes;

/* mcp_simulate / mcp_simulate_drawdown / mcp_simulate_horizons on the two regimes of SPEC.md 2.6 (simple compounding only): one more
 * Philox block per path-step on counter stream 4 moves the regime -- s_0 = x1 < thr_start (block of t = 0), s_{t+1} = s_t == 0 ?
 * x0 < thr01 : !(x0 < thr10), uint64 compares against the thresholds of mcp_regime_consts -- and row i of step t is mu^(s)_i then
 * fma(L^(s)_ij, z_j, acc), j ascending, s = s_t, each regime a whole chain of its own.  All portfolios and assets of a path share the
 * regime.  The asset normals are those of the call without regimes (common random numbers): mu1 = mu and chol1 = chol, or start = 0
 * and p01 = 0, is mcp_simulate* on (mu, chol) bit for bit, start = 1 and p10 = 0 that call on (mu1, chol1).  The moments are pivoted
 * on the exact mean of mcp_regime_pivots, horizon row h on the h-step one.  The horizon inputs and the outputs are those of
 * mcp_simulate_jumps (the drawdown or the horizons, not both: MCP_E_UNSUPPORTED).  Argument errors (MCP_E_ARG: the rules above,
 * NULL pointers) are found before any device is touched; log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.  Not
 * built: regimes with Student-t draws, GARCH, jumps, bootstrap or filtered rows, rebalancing, cash flows, the overlay, the attribution
 * or antithetic pairs, and at the mcp_launch_paths* level.  Costs: one Philox block and three compares per path-step, and a second
 * chain of N4 (N4/2 + 1) / 2 packed fused multiply-adds in every wave whose 64 paths are not all in one regime; (mu1, chol1) are
 * uploaded once per device and tile behind the packed parameters; K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_regimes(mcp_ctx *ctx, const mcp_params *prm, const mcp_regimes *r,
                         const float *mu, const float *chol, const float *W,
                         uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                         int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                         float *terminal_out,        /* NULL or host [K*n_paths] */
                         mcp_stats *stats_out,       /* [K] */
                         float *mdd_out,             /* NULL or host [K*n_paths]; needs dd_stats_out */
                         mcp_stats *dd_stats_out,    /* [K], or NULL: no drawdown */
                         float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                         mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                         double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */
/* The host constants of a regime request (SPEC.md 2.6; no device is touched; mu1 and chol1 are not read): for x = 01, 10, start in
 * this order thr_out[x] = min(2^32, floor(p_x 2^32)) and p_out[x] = thr_x / 2^32, the probability the kernel really uses (p = 0 and
 * p = 1 are exact: never and always). */
int mcp_regime_consts(const mcp_regimes *r, uint64_t *thr_out /* [3] */, double *p_out /* [3] */);
/* The shifts of the moments of regime paths (SPEC.md 5.13; no device is touched), binary64 from the binary32 inputs: with d_ks = 1 +
 * sum_i W[k,i] mu^(s)_i (i ascending), pi = (1 - p^start, p^start), P^ the transition matrix on the p^ of mcp_regime_consts and
 * D_k = diag(d_k0, d_k1): c_k(h) = pi' D_k (P^ D_k)^(h-1) 1 - 1, the exact mean of x after h steps, by the recursion v = pi D_k, then
 * u = v P^ (u_0 = v_0 (1 - p^01) + v_1 p^10, u_1 = v_0 p^01 + v_1 (1 - p^10)), v = u D_k; c = (v_0 + v_1) - 1; 0 for h = 0 or where it
 * is not finite.  Where portfolio k walks on one drift m only (m_k0 == m_k1; p^start = 0 and p^01 = 0; p^start = 1 and p^10 = 0) c_k(h)
 * is mcp_pivots' expm1(h log1p(m)), 0 if m <= -1: the same mean, so that such a call has the Gaussian call's statistics bit for bit.
 * pivots_out[k] = c_k(n_steps); hz_pivots_out[h*K + k] = c_k(horizons[h]) (NULL iff n_horizons == 0). */
int mcp_regime_pivots(const mcp_params *prm, const mcp_regimes *r, const float *mu, const float *W,
                      int n_horizons, const int32_t *horizons, double *pivots_out /* [K] */, double *hz_pivots_out /* NULL or [H*K] */);

/* Antithetic pairs (SPEC.md 2.3 / 5.10): the pair statistics of one portfolio on the terminal x.  cross = sum_j (x_2j - c)(x_2j+1 - c)
 * with c the pivot of mcp_pivots; with C = cross - S1^2 / (2 n), S1 = (mean - c) n: pair_cov = C / (n_pairs - 1), pair_corr = 2 C / m2
 * (0 if m2 == 0), mean_se = sqrt(max(m2 + 2 C, 0) / (n (n - 2))) -- the standard error of the mean of the n / 2 independent pair
 * means -- and mean_se_iid = std / sqrt(n), what n independent paths would have given.  pair_cov and mean_se are 0 when n_pairs < 2. */
typedef struct {
    uint64_t n_pairs, reserved;
    double cross, pair_cov, pair_corr, mean_se, mean_se_iid;
} mcp_pair;

/* mcp_simulate (g and st NULL), mcp_simulate_student_t (st) or mcp_simulate_garch (g, st or NULL) on antithetic pairs: path_begin and
 * n_paths even; the global paths 2j and 2j + 1 share every draw of pair j -- the Philox counters carry j -- and path 2j + 1 sees the
 * asset normals negated (the chi blocks and the GARCH variance are shared).  Member 2j is bit for bit path j of the call without pairs
 * at (path_begin / 2, n_paths / 2), member 2j + 1 path j of that call with chol negated.  Every statistic is that of the call without
 * pairs over all n_paths values; pair_out [K] adds the pair statistics.  The horizon inputs, the outputs and their rules are those of
 * mcp_simulate_garch; log compounding with Gaussian draws only.  MCP_E_ARG (before any device is touched): odd path_begin or n_paths,
 * NULL pair_out, the rules of g and st.  MCP_E_UNSUPPORTED: MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH, MCP_FLAG_SHARD_PORTFOLIOS, log
 * compounding with g or st.  Path-sharded contexts cut the path range at even ids; the shards' cross sums are added in shard order.
 * Costs per pair: the draws of one path and the Cholesky product of two.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_antithetic(mcp_ctx *ctx, const mcp_params *prm,
                            const mcp_garch *g,                 /* NULL: no GARCH */
                            const mcp_student_t *st,            /* NULL: Gaussian draws */
                            const float *mu, const float *chol, const float *W,
                            uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                            int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                            float *terminal_out,        /* NULL or host [K*n_paths] */
                            mcp_stats *stats_out,       /* [K] */
                            float *mdd_out,             /* NULL or host [K*n_paths]; needs dd_stats_out */
                            mcp_stats *dd_stats_out,    /* [K], or NULL: no drawdown */
                            float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                            mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                            double *bands_out,          /* [H*K*L], NULL iff n_levels == 0 */
                            mcp_pair *pair_out);        /* [K] */

/* Per-asset risk attribution (SPEC.md 4.10 / 5.9): one record per (portfolio k, asset i).  A_ki is the money asset i made or lost
 * for portfolio k along a path, A_ki = sum_t V_{t-1} w_ki r_i (binary32, in the kernel); sum_i A_ki = V_T - v0 up to rounding.  sum,
 * sum_tail and sum_xc are the binary64 sums over the paths of A_ki, of A_ki over the tail {x <= VaR} and of A_ki (x - pivot); mean, cvar
 * and vol are the asset's parts of the portfolio's mean, CVaR and standard deviation (Euler: the parts add up to the whole). */
typedef struct {
    double mean;            /* sum / (v0 n) */
    double cvar;            /* sum_tail / (v0 n_tail): component CVaR */
    double vol;             /* cov(A_ki / v0, x) / std, 0 if std == 0: component volatility */
    double sum, sum_tail, sum_xc;
} mcp_attr;

/* mcp_simulate (g and st NULL), mcp_simulate_student_t (st) or mcp_simulate_garch (g, st or NULL) without drawdown or horizons, then
 * a second walk of the same paths that carries every asset's contribution next to the value (one extra walk per portfolio; nothing
 * per step is stored).  terminal_out and stats_out are bit for bit those of the call without attribution.  attr_out [K][N] and
 * attr_counts_out [K][2] = {n, n_tail} as this walk counted them (equal to the statistics' own); contrib_out, when given, receives
 * the binary32 A_ki as [K][N][n_paths].  Path-sharded contexts run the second walk on every shard; the shards' sums are added in
 * shard order and the results are run-to-run deterministic.  MCP_E_UNSUPPORTED: log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH,
 * MCP_FLAG_SHARD_PORTFOLIOS, K > MCP_MAX_ATTR_PORTFOLIOS.  MCP_E_ARG (before any device is touched): the rules of g and st, NULL
 * attr_out or attr_counts_out. */
int mcp_simulate_attribution(mcp_ctx *ctx, const mcp_params *prm,
                             const mcp_garch *g,                 /* NULL: no GARCH */
                             const mcp_student_t *st,            /* NULL: Gaussian draws */
                             const float *mu, const float *chol, const float *W,
                             uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                             float *terminal_out,        /* NULL or host [K*n_paths] */
                             mcp_stats *stats_out,       /* [K] */
                             float *contrib_out,         /* NULL or host [K*N*n_paths], row k*N + i */
                             mcp_attr *attr_out,         /* [K*N] */
                             uint64_t *attr_counts_out); /* [K][2] */

/* Contributions, withdrawals and ruin (SPEC.md 4.7 / 5.6).  flows: the schedule c_1 .. c_T, n_flows == prm->n_steps finite
 * binary32 values in the units of v0 (positive: paid in, negative: taken out), the same for every portfolio; flow c_s arrives
 * at the end of step s.  has_target (0 or 1): also count the paths whose value is below fl32(target) (finite). */
typedef struct {
    const float *flows;
    int32_t n_flows;
    int32_t has_target;
    double target;
} mcp_cashflow;

/* mcp_simulate / mcp_simulate_horizons / mcp_simulate_bootstrap[_horizons] / mcp_simulate_student_t with the schedule applied
 * inside the walk (simple compounding only): per step U = fma(V, rho, V), U = U + c_s, V = (V > 0 and U > 0) ? U : +0 -- ruin is
 * absorbing, a ruined path is stored as +0 and every other stored value is > 0.  Draws: exactly one source -- mu and chol (st
 * NULL: Gaussian; st: Student-t, SPEC.md 2.2) or boot (mu, chol and st NULL).  n_horizons = 0: no horizons (horizons ignored,
 * n_levels = 0, horizon_out, hz_stats_out, bands_out and hz_counts_out NULL); otherwise the horizons, records and bands of
 * mcp_simulate_horizons, V_h taken after the flow c_h.  The records are those of x = V/fl32(v0) - 1: terminal wealth over the
 * INITIAL value, not a return on the capital paid in.  The moments are pivoted at SPEC.md 5.6 (mcp_cashflow_pivots).
 * counts_out[k] = {#(V_T == +0), has_target ? #(V_T < fl32(target)) : 0}, hz_counts_out the same per horizon row h*K + k:
 * integers summed over the shards, exact.  Argument errors (MCP_E_ARG: a NULL struct, NULL flows with n_steps > 0, n_flows !=
 * n_steps, a flow or target that is not finite, has_target not 0 / 1, fl32(v0) == 0, NULL counts_out) are found before any
 * device is touched; log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.  K >= 17 runs as passes of 8
 * portfolios. */
int mcp_simulate_cashflow(mcp_ctx *ctx, const mcp_params *prm, const mcp_cashflow *cf,
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
                          uint64_t *hz_counts_out);   /* [H*K][2], NULL iff n_horizons == 0 */
/* The shift of the moments of paths with cash flows at prm->n_steps (SPEC.md 5.6; host side, binary64 from the binary32 inputs):
 * with m_k the per-step mean of mcp_pivots (mu) or of mcp_bootstrap_pivots (boot; exactly one of mu and boot), A_0 = fl32(v0),
 * A_s = A_{s-1} (1 + m_k) + c_s (a product, then a sum):  c_k = max(A_T, 0) / fl32(v0) - 1, 0 where it is not finite.  The
 * exact mean of x while no path is ruined. */
int mcp_cashflow_pivots(const mcp_params *prm, const mcp_cashflow *cf, const float *mu, const mcp_bootstrap *boot,
                        const float *W, double *pivots_out /* [K] */);

/* Glide paths: scheduled target weights (SPEC.md 4.14 / 5.14).  breaks: n_breaks strictly increasing steps in [1, n_steps - 1];
 * targets: n_breaks blocks of [K][N] finite binary32 weights.  Step s = 1 .. n_steps of portfolio k walks on block g = #{j : breaks[j]
 * < s}, block 0 being the call's W: W is held through step breaks[0], targets block 0 through step breaks[1], and so on.  The
 * portfolio stands at its current target at the start of every step; the trade at a break is free.  reserved must be 0. */
typedef struct {
    const int32_t *breaks;    /* [n_breaks], strictly increasing, in [1, n_steps - 1]; NULL when n_breaks == 0 */
    const float *targets;     /* [n_breaks][K][N] row-major, finite; NULL when n_breaks == 0 */
    int32_t n_breaks;         /* 0 .. MCP_MAX_GLIDE */
    int32_t reserved;         /* 0 */
} mcp_glide;

/* mcp_simulate_cashflow on the weights of a glide path: the draws, the recurrence U = fma(V, rho, V) + c_s with absorbing ruin, the
 * horizons, records, bands and counts are that call's, only the weights of the dot rho_k = sum_i w_ki r_i change at the breaks.  cf
 * NULL: the all-zero schedule without a target (V stays absorbed at +0 once it is not positive).  n_breaks = 0, or every target block
 * equal to W, is mcp_simulate_cashflow bit for bit.  The moments are pivoted at SPEC.md 5.14 (mcp_glide_pivots).  Argument errors
 * (MCP_E_ARG: a NULL struct, n_breaks outside [0, MCP_MAX_GLIDE], NULL breaks or targets with n_breaks > 0, a break outside
 * [1, n_steps - 1] or not above the one before, a target that is not finite, reserved != 0, and every rule of mcp_simulate_cashflow)
 * are found before any device is touched; log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.  Not built:
 * a glide path with the drawdown, rebalancing, the overlay, GARCH, jumps, regimes, filtered rows, the attribution, antithetic pairs,
 * or at the mcp_launch_* level.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_glide(mcp_ctx *ctx, const mcp_params *prm, const mcp_glide *gl,
                       const mcp_cashflow *cf,                /* NULL: all-zero schedule, no target              */
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
                       uint64_t *hz_counts_out);   /* [H*K][2], NULL iff n_horizons == 0 */
/* The shifts of the moments of a glide path (SPEC.md 5.14; host side, binary64 from the binary32 inputs): with m_kg the per-step
 * mean of mcp_cashflow_pivots on the weights of block g, A_0 = fl32(v0), A_s = A_{s-1} (1 + m_kg(s)) + c_s (a sum, a product, a
 * sum): max(A, 0) / fl32(v0) - 1, 0 where it is not finite, after step n_steps into pivots_out[k] and after the steps of the
 * n_horizons horizons into hz_pivots_out[h*K + k] (n_horizons = 0: horizons and hz_pivots_out ignored).  cf NULL: c_s = 0. */
int mcp_glide_pivots(const mcp_params *prm, const mcp_glide *gl, const mcp_cashflow *cf, const float *mu,
                     const mcp_bootstrap *boot, const float *W, int n_horizons, const int32_t *horizons,
                     double *pivots_out /* [K] */, double *hz_pivots_out /* NULL or [H*K] */);

/* Option and hedging overlays (SPEC.md 4.8 / 5.7).  Asset i owns the rows [row_begin[i], row_begin[i+1]) of `rows`, applied in that
 * order; kind LINEAR: leg = price - prev, CALL: leg = max(price - strike, 0) - premium, PUT: leg = max(strike - price, 0) -
 * premium (strike and premium in price units, the sign of a short row folded into qty).  spot: the assets' current prices, > 0 on
 * every asset that owns rows; reserved must be 0.  n_rows = 0: every asset passes through. */
#define MCP_OVERLAY_LINEAR 0
#define MCP_OVERLAY_CALL 1
#define MCP_OVERLAY_PUT 2
typedef struct {
    int32_t kind;
    float strike, premium, qty;
} mcp_overlay_row;
typedef struct {
    const mcp_overlay_row *rows;   /* [n_rows], NULL when n_rows == 0 */
    const int32_t *row_begin;      /* [n_assets + 1], ascending from 0 to n_rows */
    const float *spot;             /* [n_assets] */
    int32_t n_rows;
    int32_t reserved;
} mcp_overlay;

/* mcp_simulate / mcp_simulate_drawdown / mcp_simulate_horizons / mcp_simulate_student_t with the overlay applied inside the walk
 * (simple compounding only): the kernel carries the price P_i of every asset that owns rows (from fl32(spot_i), price = fma(P_i,
 * r_i, P_i) with the RAW return r_i of the step) and replaces r_i by r'_i = sum_rows qty * leg / P_i (one fma per row from +0, one
 * IEEE division; +0 where P_i == 0) before rho_k = sum_i W[k,i] r'_i.  st NULL: Gaussian draws; st: Student-t draws (SPEC.md
 * 2.2).  dd_stats_out non-NULL: the drawdown of mcp_simulate_drawdown; n_horizons > 0: the horizons, records and bands of
 * mcp_simulate_horizons (n_horizons = 0: horizons ignored, n_levels = 0, horizon_out, hz_stats_out, bands_out NULL); not both
 * (MCP_E_UNSUPPORTED).  The moments are pivoted at SPEC.md 5.7 (mcp_overlay_pivots).  Argument errors (MCP_E_ARG: a NULL struct,
 * row_begin not ascending from 0 to n_rows, more than MCP_MAX_OVERLAY_ROWS rows on an asset, a kind outside 0..2, a strike,
 * premium, qty or spot that is not finite, spot <= 0 on an asset with rows, reserved != 0) are found before any device is touched;
 * log compounding, MCP_FLAG_FOLD, MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED.  K >= 17 runs as passes of 8 portfolios. */
int mcp_simulate_overlay(mcp_ctx *ctx, const mcp_params *prm, const mcp_overlay *ov,
                         const float *mu, const float *chol,
                         const mcp_student_t *st,            /* NULL: Gaussian draws */
                         const float *W, uint64_t seed, uint64_t path_begin, uint64_t n_paths,
                         int n_horizons, const int32_t *horizons, int n_levels, const double *levels,
                         float *terminal_out,        /* NULL or host [K*n_paths] */
                         mcp_stats *stats_out,       /* [K] */
                         float *mdd_out,             /* NULL or host [K*n_paths]; needs dd_stats_out */
                         mcp_stats *dd_stats_out,    /* [K], or NULL: no drawdown */
                         float *horizon_out,         /* NULL or host [H*K*n_paths], row h*K + k */
                         mcp_stats *hz_stats_out,    /* [H*K], NULL iff n_horizons == 0 */
                         double *bands_out);         /* [H*K*L], NULL iff n_levels == 0 */
/* The shift of the moments of overlaid paths at prm->n_steps (SPEC.md 5.7; host side, binary64 from the binary32 inputs): the
 * rule of SPEC.md 4.8 on the deterministic prices P_i,t = P_i,t-1 (1 + mu_i) from P_i,0 = spot_i, rho_k,t = sum_i W[k,i] r'_i,t
 * (i ascending), A_k,t = A_k,t-1 (1 + rho_k,t) from 1:  c_k = A_k,T - 1, 0 where it is not finite.  n_rows = 0: mcp_pivots. */
int mcp_overlay_pivots(const mcp_params *prm, const mcp_overlay *ov, const float *mu, const float *W,
                       double *pivots_out /* [K] */);

/* The reference's own sweep (app.py:699-717) over HISTORICAL returns, loop body app.py:708-713 for P weight
 * vectors at once, binary64 like the reference.  returns: [R*N] row-major (returns_df.values, app.py:667),
 * mean/cov: the annualised mean_returns / cov_matrix of app.py:679-680, W: [P*N] (rows as drawn at
 * app.py:702), rf in the reference's units (user_rf, app.py:711), alpha = cvar_alpha (app.py:684).
 * Outputs are [P] each.  Limits: N <= MCP_MAX_ASSETS, R <= MCP_SWEEP_MAX_ROWS.
 * Every value of returns, W, mean and cov must be finite (the rule of mcp_bootstrap rows): a NaN or an infinity is MCP_E_ARG,
 * mcp_last_error() naming the array and the first offending index, found by a host scan before anything is copied or
 * launched -- the kernels order the series with plain compares, under which a NaN would come back as a finite VaR.  Drop such
 * rows first, as the reference's ingest does.  cvar is the tail mean from an exactly accumulated sum, kept inside
 * [smallest tail element, var], so cvar <= var always and cvar == var where the tail is one value repeated. */
#define MCP_SWEEP_MAX_ROWS 4096
int mcp_sweep_historical(mcp_ctx *ctx, int n_assets, int n_rows, int n_portfolios, const double *returns,
                         const double *mean, const double *cov, const double *W, double rf, double alpha,
                         double *port_return, double *port_std, double *sharpe, double *var, double *cvar);

/* ---- device-level API: the same kernels as separate enqueue-only steps, for a host that owns the
 *      buffers and the collectives (one process per GPU, torch.distributed over RCCL).  Work buffers
 *      are opaque device memory of the byte sizes given by mcp_ws_bytes(); MCP_WS_HIST must be ZERO when first
 *      used (the steps clear what they consume).  One pass, in this order:
 *          paths (fused: V_T, moment partials, digit-0 histogram)
 *                -> [all-reduce HIST] -> scan(0) -> hist(1) -> [all-reduce HIST] -> scan(1)
 *                -> hist(2) -> [all-reduce HIST] -> final -> [all-gather RECORD -> stats]
 *      A single-GPU host skips the bracketed exchanges and passes d_stats to mcp_launch_final.  A host that has terminal
 *      values of its own replaces `paths` by mcp_launch_pass0. -------- */

enum {
    MCP_WS_PARTIALS = 0,   /* [K][mcp_moment_slots] x 32 B {sum (x-c), sum (x-c)^2, float min V, max V, u64 n}: one per
                              workgroup (K <= 16) or per 64-path wave tile (K >= 17) of the path kernels          */
    MCP_WS_RECORD = 1,     /* [K] mcp_record: this device's sufficient statistics (all-gathered)                  */
    MCP_WS_STATE = 2,      /* [K][2] select state {u32 prefix, u32 pad, u64 rank}                                 */
    MCP_WS_HIST = 3,       /* [K][2][MCP_SELECT_BINS] uint64: all-reduce SUM after paths / hist                   */
    MCP_WS_QUANT = 4,      /* [K] {double x_lo, x_hi, var, level2; u64 n_tail, pad}: identical on all ranks       */
    MCP_WS_STATS = 5,      /* [K] mcp_stats                                                                       */
    MCP_WS_BELOW = 6,      /* [K][slots(K)] double: per-block tail partials of hist(1) / hist(2)                  */
    MCP_WS_PIVOT = 7,      /* [K] double: the shift of the moments (host: mcp_pivots, then copy to the device)    */
    MCP_WS_COUNT = 8
};
/* bytes of work buffer `which` for K portfolios and n_paths paths on this device (only MCP_WS_PARTIALS depends on n_paths) */
size_t mcp_ws_bytes(int which, int n_portfolios, uint64_t n_paths);
/* MomentPartial slots per portfolio a pass over n_paths fills (informative; mcp_ws_bytes uses it) */
uint64_t mcp_moment_slots(int n_portfolios, uint64_t n_paths);

/* Number of floats of the packed parameter block for (N, K). */
size_t mcp_packed_len(int n_assets, int n_portfolios);
/* Pack mu, lower(chol), W (and portfolio 0's fold block) into the padded device layout (host side, no GPU needed). */
int mcp_pack_params(int n_assets, int n_portfolios, const float *mu, const float *chol, const float *W,
                    float *packed_out, size_t packed_len);
/* The shift of the moments, one per portfolio (host side, binary64 from the binary32 inputs): the analytic mean of x --
 * w_k.mu is the per-step `port_return` of app.py:708, |L^T w_k|^2 the per-step `port_std`^2 of app.py:709 --
 *   simple: c_k = (1 + w_k.mu)^T - 1          log: c_k = expm1(T (w_k.mu + |L^T w_k|^2 / 2)).
 * A function of the inputs only, hence identical on every rank; 0 where it is not finite. */
int mcp_pivots(const mcp_params *prm, const float *mu, const float *chol, const float *W, double *pivots_out /* [K] */);

/* Simulate paths [path_begin, path_begin+n_paths) of all K portfolios and store the terminal values:
 * d_terminal is [K][terminal_stride] floats (terminal_stride >= n_paths), 4 B per path and portfolio.
 * With d_partials and d_hist (both or neither) the kernels' epilogue also reduces the paths while V is in registers:
 * moment partials around d_pivot ([K] doubles, NULL = 0) into d_partials and the digit-0 histogram of the radix select
 * (key bits 31..21) into d_hist -- what mcp_launch_scan(pass 0) consumes.  (K >= 17: the histogram is one lean read of
 * V_T enqueued behind the MFMA kernel, whose workgroups hold 512 portfolios.) */
int mcp_launch_paths(const mcp_params *prm, const float *d_packed, const double *d_pivot, uint64_t seed, uint64_t path_begin,
                     uint64_t n_paths, float *d_terminal, uint64_t terminal_stride, void *d_partials, void *d_hist,
                     void *stream);
/* mcp_launch_paths that also stores the per-path drawdown state of SPEC.md 4.2 into d_mdd ([K][mdd_stride] floats, q or d;
 * mdd_stride >= n_paths).  Always the one-lane-per-path kernels (K >= 17: passes of 8 portfolios, whose moment partials keep
 * the mcp_moment_slots(K, n) layout).  To reduce the drawdowns: mcp_launch_pass0 over d_mdd with a copy of the parameters
 * with v0 = 1, rf = 0 and d_pivot NULL, then the usual scan / hist / final steps (x = q - 1 or expm1(d) is then exactly the
 * drawdown).  MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED. */
int mcp_launch_paths_drawdown(const mcp_params *prm, const float *d_packed, const double *d_pivot, uint64_t seed,
                              uint64_t path_begin, uint64_t n_paths, float *d_terminal, uint64_t terminal_stride,
                              float *d_mdd, uint64_t mdd_stride, void *d_partials, void *d_hist, void *stream);
/* mcp_launch_paths that also stores the values after the steps horizons[0..n_horizons) (host array, SPEC.md 4.3) into
 * d_horizon ([n_horizons][K][horizon_stride] floats, row h*K + k; horizon_stride >= n_paths).  Kernels and moment partials
 * as in mcp_launch_paths_drawdown.  To reduce one horizon row set: mcp_launch_pass0 over d_horizon with n_portfolios =
 * H*K and the [H*K] pivots of mcp_pivots at n_steps = h, then the usual scan / hist / final steps.  Work buffers that serve
 * both this and the launch's own K rows take the LARGER of mcp_ws_bytes(w, K, n) and mcp_ws_bytes(w, H*K, n), buffer by
 * buffer: MCP_WS_BELOW does not grow with the rows (K = 9 needs 16,380 doubles, H*K = 27 only 16,362).
 * MCP_FLAG_FOLD / MCP_FLAG_NATIVE_MATH: MCP_E_UNSUPPORTED. */
int mcp_launch_paths_horizons(const mcp_params *prm, const float *d_packed, const double *d_pivot, uint64_t seed,
                              uint64_t path_begin, uint64_t n_paths, float *d_terminal, uint64_t terminal_stride,
                              int n_horizons, const int32_t *horizons, float *d_horizon, uint64_t horizon_stride,
                              void *d_partials, void *d_hist, void *stream);

/* np.percentile(x, (1-alpha)*100) bookkeeping (numpy 2.2 `_compute_virtual_index`/`_get_indexes`,
 * method 'linear'; the q of app.py:259): ranks of the two order statistics and the weight. */
int mcp_percentile_rank(uint64_t n_total, double alpha, uint64_t *rank_lo, uint64_t *rank_hi, double *gamma);
/* The same bookkeeping for np.percentile(x, q) itself, q in percent in [0, 100]: q/100, vi = (n-1)*(q/100), the same clamps. */
int mcp_percentile_rank_q(uint64_t n_total, double q, uint64_t *rank_lo, uint64_t *rank_hi, double *gamma);

/* Standalone pass 0 over CALLER-SUPPLIED terminal values (n per portfolio): the same moment partials and digit-0
 * histogram the fused epilogue of mcp_launch_paths leaves.  d_pivot: [K] doubles or NULL (= 0: raw sums). */
int mcp_launch_pass0(const mcp_params *prm, const float *d_terminal, uint64_t terminal_stride, uint64_t n,
                     const double *d_pivot, void *d_partials, void *d_hist, void *stream);
/* pass 0: partials -> d_record (with d_pivot, NULL = 0), (rank_lo, rank_hi) of the GLOBAL n -> d_state, descend into the
 * digit holding each rank; pass 1: descend again (and fold the tail partials of hist pass 1 into d_record).  Clears d_hist. */
int mcp_launch_scan(const mcp_params *prm, int pass, uint64_t n, uint64_t rank_lo, uint64_t rank_hi, const void *d_partials,
                    const void *d_below, const double *d_pivot, void *d_hist, void *d_state, void *d_record, void *stream);
/* pass 1 (key bits 20..10) / pass 2 (bits 9..0): digit histograms of the keys matching the prefixes in d_state, and the
 * tail sum below the low bucket (CVaR tail, app.py:261-263) into d_below.  pass 0: the digit-0 histogram alone (d_state
 * unused; d_pivot, if given, centres the kernel's counting window). */
int mcp_launch_hist(const mcp_params *prm, int pass, const float *d_terminal, uint64_t terminal_stride, uint64_t n,
                    const void *d_state, const double *d_pivot, void *d_below, void *d_hist, void *stream);
/* Last descent -> order statistics -> VaR (numpy `_lerp`) -> d_quant; tail count / in-bucket tail sum from the
 * (global) histogram; local `below` into d_record.  d_stats != NULL (single device): also mean, std (ddof=1), Sharpe,
 * CVaR -> d_stats [K] mcp_stats.  Clears d_hist. */
int mcp_launch_final(const mcp_params *prm, uint64_t n, double gamma, uint64_t rank_lo, uint64_t rank_hi,
                     const void *d_below, void *d_hist, const void *d_state, void *d_record, void *d_quant,
                     void *d_stats, void *stream);
/* Multi-GPU: merge the all-gathered records of `world` ranks, d_gathered [world][K] mcp_record in rank order, and
 * finish -> d_stats [K] mcp_stats. */
int mcp_launch_stats(const mcp_params *prm, int world, const void *d_gathered, const void *d_quant, void *d_stats,
                     void *stream);
/* Exchange between logical shards that live in ONE process (several shards of one device, or devices with peer access):
 * every one of the `n_bufs` (<= 8) device buffers <- their element-wise sum (u64 words).  The kernel form of the histogram
 * all-reduce; the caller orders it after the producers and before the consumers of every buffer (events). */
int mcp_launch_sum_u64(void *const *d_bufs, int n_bufs, size_t words, void *stream);

/* A stream of `device` whose kernels may run on all but `reserve_cus` compute units (hipExtStreamCreateWithCUMask; the
 * reserved ones are the highest-numbered CUs of the mask).  For hosts that pipeline batches: path kernels on such streams
 * leave a few CUs to the small statistics / exchange kernels of the batch before, which otherwise queue for wave slots
 * beside a kernel that fills the chip.  reserve_cus = 0: an ordinary non-blocking stream. */
int mcp_stream_create(int device, int reserve_cus, void **stream_out);
int mcp_stream_destroy(void *stream);

/* The normal generator on its own: d_z[i] = inverse-CDF normal (SPEC.md section 3) of the 32-bit word d_x[i]. */
int mcp_launch_normals(const uint32_t *d_x, uint64_t n, float *d_z, void *stream);

/* The inverse-CDF coefficient table the kernels use (1056 x 4 floats; pure CPU): lets a test compare it with the
 * oracle's copy. */
int mcp_icdf_table(float *out, size_t out_len);

/* Host helpers shared by both levels (pure CPU). */
uint32_t mcp_float_to_key(float v);
float mcp_key_to_float(uint32_t key);
/* x from a terminal value, in double: V/fl32(v0) - 1, or expm1(S). */
double mcp_terminal_to_x(const mcp_params *prm, float terminal);

#ifdef __cplusplus
}
#endif
#endif /* MCPORT_H */

#!/usr/bin/env python3
"""CSV-in -> (weights, stats, P/L curve): the reference's tab 0 / 1 / 2 flow, headless, on the MI355X engine.

    python examples/pipeline.py [csv ...]        (defaults to three of the CSV files the reference ships)

Mirrors app.py's order of operations with the package's drop-in functions: read_csv_file (app.py:89) ->
align / resample (app.py:466-482) -> per-asset statistics table (app.py:484-495) -> option overlay and payoff
curve of one asset (app.py:499-653) -> returns matrix (app.py:658-667) -> the five-method random-weight sweep on
historical rows (app.py:682-783, GPU) and its best-Sortino / shallowest-drawdown / best-Calmar weights -> the optimum re-scored on one million SIMULATED one-year paths (GPU).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import monte_carlo_portfolio_amd as mcp                                   # noqa: E402
from monte_carlo_portfolio_amd import ingest, options, sweep              # noqa: E402


def main(paths, resample_rule="M", user_rf=3.0, investment=10000.0, seed=12345, n_paths=1_000_000):
    files = [open(p, "rb") for p in paths]
    names, prices, resampled = mcp.load_prices(files, resample_rule=resample_rule, report=lambda m: print("skip:", m))
    af = ingest.ANNUAL_FACTOR[resample_rule]
    print("assets:", names, "| rows after alignment:", len(prices), "| periods:", len(resampled))
    print(mcp.stats_table(resampled, resample_rule, user_rf).round(4).to_string())

    a0 = names[0]                                                          # a protective put on the first asset
    S = float(resampled[a0].iloc[-1])
    rows = options.strategy_rows("Protective Put", S, premium_put=0.02)
    grid = options.payoff_grid(S)
    pay = mcp.calculate_payoff(rows, S, S, grid)
    print(f"{a0}: protective put breakeven {mcp.calculate_breakeven(rows, S):.4f}, P/L at -50 % / +50 %: {pay[0]:.3f} / {pay[-1]:.3f}")

    returns_df = mcp.returns_matrix(resampled, {a0: rows})
    res = mcp.run_all_methods(returns_df, user_rf=user_rf, annual_factor=af, seed=seed, investment_amount=investment)
    for m, r in res.items():
        print(f"{m:12s} opt_idx {r['opt_idx']:5d}  risk {r['all_risks'][r['opt_idx']] * 100:8.3f} %  "
              f"return {r['all_returns'][r['opt_idx']] * 100:8.3f} %  dollars {np.round(r['dollar_vals'], 2)}")
    # three more criteria over the weights the "Monte Carlo" method drew (SPEC.md 5.24): the reference's own series statistics of
    # returns_df @ w for every row -- best Sortino, shallowest historical drawdown, best Calmar -- beside the five optima above
    for m in sweep.EXTRA_METHODS:
        risks, rets, W, scores, opt = sweep.run_sweep(returns_df, m, user_rf=user_rf, annual_factor=af, seed=seed, risk_free=user_rf / 100)
        print(f"{m:12s} opt_idx {opt:5d}  risk {risks[opt] * 100:8.3f} %  return {rets[opt] * 100:8.3f} %  "
              f"dollars {np.round(sweep.allocation(W[opt], investment), 2)}  score {scores[opt]:+.4f}")

    # how far the Monte Carlo optimum can be trusted (SPEC.md 5.25): the same weights scored on 1,000 i.i.d. resamples of the rows
    mc = res["Monte Carlo"]
    rs = sweep.score_resampled(returns_df.to_numpy(dtype=np.float64), mc["all_weights"], user_rf, af, n_replicates=1000, block=1.0, seed=seed)
    summ = sweep.resample_summary(rs, mc["all_weights"], point=mc["opt_idx"])
    won, lo_hi = summ["Monte Carlo"], summ["sharpe"]["interval"][:, mc["opt_idx"]]
    print(f"resampled sweep (1,000 replicates): the Monte Carlo optimum wins {won['point_win_share'] * 100:.1f} % of them, is in the top "
          f"5 % in {won['point_top5_share'] * 100:.1f} %; {int((won['wins'] > 0).sum())} portfolios win at least once")
    print(f"  95 % interval of its Sharpe: {lo_hi[0]:+.4f} .. {lo_hi[1]:+.4f} (standard error {summ['sharpe']['se'][mc['opt_idx']]:.4f})")
    print(f"  resampled weights {np.round(won['resampled_weights'], 4)} beside its own {np.round(mc['weights'], 4)}")

    w = res["Monte Carlo"]["weights"]
    mu_step, cov_step = returns_df.mean().values, returns_df.cov().values  # per period, before annualising
    sim = mcp.simulate_paths(mu_step, cov_step, w, n_steps=af, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100,
                             drawdown=True, downside=0.0)
    print(f"max-Sharpe weights on {n_paths:,} simulated {af}-period paths: mean {sim['mean']:+.4f}  std {sim['std']:.4f}  "
          f"VaR95 {sim['var']:+.4f}  CVaR95 {sim['cvar']:+.4f}  Sharpe {sim['sharpe']:.4f}")

    def shape(label, o):                  # downside and shape of x at the threshold 0 (SPEC.md 5.22): what fat tails and jumps move
        d = o["downside"]
        print(f"  {label}: Sortino {d['sortino']:.4f}  P(loss) {d['p_below']:.4f}  skewness {d['skewness']:+.4f}  "
              f"excess kurtosis {d['excess_kurtosis']:+.4f}")
    shape("Gaussian draws", sim)
    # the optimum against equal weights on the same paths (SPEC.md 5.23): row 0 against row 1, the benchmark
    pair = mcp.simulate_paths(mu_step, cov_step, np.stack([w, np.full(len(w), 1.0 / len(w))]), n_steps=af, n_paths=n_paths, seed=seed,
                              v0=investment, rf=user_rf / 100, benchmark=1)
    rel = pair[0]["relative"]
    print(f"  against equal weights: tracking error {rel['tracking_error']:.4f}  IR {rel['information_ratio']:+.4f}  "
          f"P(behind) {rel['p_under']:.4f}  relative CVaR95 {rel['active']['cvar']:+.4f}  down capture {rel['down_capture']:.4f}")
    dd = sim["drawdown"]                  # max drawdown of every path before the horizon (SPEC.md 4.2 / 5.1)
    print(f"  max drawdown: mean {dd['mean']:+.4f}  DaR95 {dd['dar']:+.4f}  CDaR95 {dd['cdar']:+.4f}  worst {dd['worst']:+.4f}")
    # which holding that risk comes from (SPEC.md 4.10 / 5.9): the same paths walked a second time, every asset's part of the CVaR
    # and of the volatility -- the risk pie next to the dollar pie of the optimum
    att = mcp.simulate_paths(mu_step, cov_step, w, n_steps=af, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100,
                             attribution=True)["attribution"]
    for name, wi, cs, vs in zip(names, w, att["cvar_share"], att["vol_share"]):
        print(f"  risk attribution {name}: weight {wi * 100:6.2f} %  CVaR share {cs * 100:6.2f} %  volatility share {vs * 100:6.2f} %")
    fan = mcp.simulate_paths(mu_step, cov_step, w, n_steps=6, n_paths=n_paths, seed=seed, v0=investment, horizons=[1, 3, 6],
                             bands=(2.5, 50.0, 97.5))["horizons"]        # values at intermediate horizons (SPEC.md 4.3 / 5.2)
    for h, b in zip(fan["steps"], fan["bands"]):
        lo, mid, hi = investment * (1.0 + b)
        print(f"  forecast fan after {h} period(s): 2.5 % {lo:,.2f}  median {mid:,.2f}  97.5 % {hi:,.2f}")
    # the same fan with the estimation risk of the mean inside it (SPEC.md 2.7 / 4.21): one drift per path, drawn from drift_cov(rows)
    ufan = mcp.simulate_paths(mu_step, cov_step, w, n_steps=6, n_paths=n_paths, seed=seed, v0=investment, horizons=[1, 3, 6],
                              bands=(2.5, 50.0, 97.5), drift_uncertainty=mcp.drift_cov(returns_df))["horizons"]
    for h, b in zip(ufan["steps"], ufan["bands"]):
        lo, mid, hi = investment * (1.0 + b)
        print(f"  fan with drift uncertainty after {h} period(s): 2.5 % {lo:,.2f}  median {mid:,.2f}  97.5 % {hi:,.2f}")
    # the same weights on paths resampled from the observed rows (stationary bootstrap, SPEC.md 2.1 / 4.4): the option
    # overlay's kinks and the fat tails stay in the paths instead of being reduced to mean / cov
    boot = mcp.simulate_bootstrap(returns_df, w, n_steps=af, n_paths=n_paths, block=3.0, seed=seed, v0=investment, rf=user_rf / 100,
                                  horizons=[1, 3, 6], bands=(2.5, 50.0, 97.5))
    print(f"bootstrap (mean block 3) of the {len(returns_df)} observed rows, same weights: mean {boot['mean']:+.4f}  "
          f"std {boot['std']:.4f}  VaR95 {boot['var']:+.4f}  CVaR95 {boot['cvar']:+.4f}  Sharpe {boot['sharpe']:.4f}")
    for h, b in zip(boot["horizons"]["steps"], boot["horizons"]["bands"]):
        lo, mid, hi = investment * (1.0 + b)
        print(f"  bootstrap fan after {h} period(s): 2.5 % {lo:,.2f}  median {mid:,.2f}  97.5 % {hi:,.2f}")
    # the same weights on fat-tailed Student-t steps (SPEC.md 2.2 / 4.6): the normal model's mean and covariance, one chi-square
    # mixing variable per path and period shared by all assets, nu fitted to the observed rows (32: no evidence of fat tails)
    nu = mcp.fit_student_t_dof(returns_df)
    tsim = mcp.simulate_paths(mu_step, cov_step, w, n_steps=af, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100,
                              dof=nu, drawdown=True, downside=0.0)
    print(f"Student-t (nu = {nu}, fitted to the {len(returns_df)} observed rows), same weights: mean {tsim['mean']:+.4f}  "
          f"std {tsim['std']:.4f}  VaR95 {tsim['var']:+.4f}  CVaR95 {tsim['cvar']:+.4f}  Sharpe {tsim['sharpe']:.4f}  "
          f"DaR95 {tsim['drawdown']['dar']:+.4f}")
    shape(f"Student-t draws (6 / (nu - 4) = {6 / (nu - 4):.2f} per step)" if nu > 4 else "Student-t draws", tsim)
    # how long the optimum stays below its high-water mark on those paths (SPEC.md 4.20 / 5.20): exact integers off two histograms
    uw = mcp.simulate_paths(mu_step, cov_step, w, n_steps=af, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100, dof=nu,
                            drawdown=True, underwater=True, underwater_levels=(50, 95))["underwater"]
    print(f"  time under water: longest spell median {uw['longest']['levels'][50.0]} / 95 % {uw['longest']['levels'][95.0]} of {af} "
          f"period(s), P(under water at the end) = {uw['p_under_water_at_end']:.4f}")
    tfan = mcp.simulate_paths(mu_step, cov_step, w, n_steps=6, n_paths=n_paths, seed=seed, v0=investment, dof=nu, horizons=[1, 3, 6],
                              bands=(2.5, 50.0, 97.5))["horizons"]
    for h, b in zip(tfan["steps"], tfan["bands"]):
        lo, mid, hi = investment * (1.0 + b)
        print(f"  Student-t fan after {h} period(s): 2.5 % {lo:,.2f}  median {mid:,.2f}  97.5 % {hi:,.2f}")
    # the same weights with volatility clustering (SPEC.md 4.9): a GARCH(1,1) variance ratio on the covariance, fitted to the observed
    # rows; the fan starts from the fitted h0, the regime the rows end in (alpha = beta = 0: no evidence of clustering)
    gfit = mcp.fit_garch(returns_df)
    print(f"GARCH(1,1) fit: alpha = {gfit.alpha:.3f}  beta = {gfit.beta:.3f}  h0 = {gfit.h0:.3f}  "
          f"(log-likelihood {gfit.loglik - gfit.loglik_iid:+.2f} over constant variance)")
    gfan = mcp.simulate_paths(mu_step, cov_step, w, n_steps=6, n_paths=n_paths, seed=seed, v0=investment, garch=gfit[:3],
                              horizons=[1, 3, 6], bands=(2.5, 50.0, 97.5))["horizons"]
    for h, b in zip(gfan["steps"], gfan["bands"]):
        lo, mid, hi = investment * (1.0 + b)
        print(f"  GARCH fan after {h} period(s): 2.5 % {lo:,.2f}  median {mid:,.2f}  97.5 % {hi:,.2f}")
    # the same weights under a volatility target (SPEC.md 4.19 / 5.19) on the fitted GARCH paths: the exposure to the optimum is the
    # optimum's unconditional step volatility over an EWMA estimate of the path's own (half-life a quarter of a year), at most 1.5 times
    # the value, the rest in cash at the riskless rate -- less exposure while volatility is high, more while it is low
    sig = float(np.sqrt(np.asarray(w, np.float64) @ np.asarray(cov_step, np.float64) @ np.asarray(w, np.float64)))
    vkw = dict(n_steps=af, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100, garch=gfit[:3], drawdown=True)
    held = mcp.simulate_paths(mu_step, cov_step, w, **vkw)
    aimed = mcp.simulate_paths(mu_step, cov_step, w, vol_target=(sig, mcp.ewma_decay(max(1.0, af / 4)), 1.5, user_rf / 100 / af), **vkw)
    for label, o in (("held", held), ("volatility target", aimed)):
        print(f"  optimum under the fitted GARCH, {label}: VaR = {o['var']:+.4f}  CVaR = {o['cvar']:+.4f}  mean max drawdown = "
              f"{o['drawdown']['mean']:+.4f}")
    print(f"  (target {sig:.4f} per period, cap 1.5, first exposure {aimed['vol_target']['exposure0']:.3f}, ruined "
          f"{aimed['vol_target']['n_ruined']} of {n_paths} paths)")
    # the observed rows themselves at today's volatility (SPEC.md 2.4 / 4.11, filtered historical simulation): the rows divided by
    # the fitted variance path, resampled, and every draw scaled by the variance ratio the path carries from the same h0
    frows = mcp.filter_rows(returns_df, gfit[:2])
    ffan = mcp.simulate_filtered(frows, w, n_steps=6, n_paths=n_paths, seed=seed, v0=investment, horizons=[1, 3, 6],
                                 levels=(2.5, 50.0, 97.5))["horizons"]
    for h, b in zip(ffan["steps"], ffan["bands"]):
        lo, mid, hi = investment * (1.0 + b)
        print(f"  filtered-rows fan after {h} period(s): 2.5 % {lo:,.2f}  median {mid:,.2f}  97.5 % {hi:,.2f}")
    # the same weights under crash risk (SPEC.md 2.5 / 4.12, Merton jump-diffusion): a market jump fitted to the observed rows by a
    # threshold rule, every asset taking part through its loading; mean and covariance stay those of the rows, skew and tails move
    jfit = mcp.fit_jumps(returns_df)
    print(f"jump-diffusion fit: intensity = {jfit.intensity:.4f}  mean = {jfit.mean:+.4f}  std = {jfit.std:.4f}  "
          f"({jfit.n_jump_rows} of {len(returns_df)} rows)  loadings {np.round(jfit.loading, 2)}")
    kw = dict(n_steps=af, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100, drawdown=True, jumps=tuple(jfit[:4]), downside=0.0)
    try:
        jsim = mcp.simulate_paths(mu_step, cov_step, w, **kw)
    except ValueError:                    # the fitted jumps carry more variance than the rows' covariance leaves: keep the diffusion whole
        jsim = mcp.simulate_paths(mu_step, cov_step, w, chol=np.linalg.cholesky(cov_step), **kw)
    print(f"  optimum without jumps: VaR = {sim['var']:+.4f}  CVaR = {sim['cvar']:+.4f}  mean max drawdown = {sim['drawdown']['mean']:+.4f}")
    print(f"  optimum with jumps:    VaR = {jsim['var']:+.4f}  CVaR = {jsim['cvar']:+.4f}  mean max drawdown = "
          f"{jsim['drawdown']['mean']:+.4f}  (jump share of the variance {jsim['jumps']['variance_share'] * 100:.1f} %)")
    shape("with jumps", jsim)
    # a withdrawal plan on the same weights (SPEC.md 4.7 / 5.6): 1.5 % of the capital taken out after every period for 6 years;
    # a path whose value is used up is ruined and stays so -- the share of ruined paths per horizon is the survival curve
    T, take = 6 * af, 0.015 * investment
    plan = mcp.simulate_paths(mu_step, cov_step, w, n_steps=T, n_paths=n_paths, seed=seed, v0=investment, cashflow=-take,
                              target=investment, horizons=[2 * af, 4 * af, 6 * af], bands=(50.0,))
    cash = plan["cashflow"]
    print(f"withdrawal plan ({take:,.2f} per period over {T} periods, {-cash['contributed']:,.2f} in all): ruin probability at the end "
          f"{cash['ruin_probability']:.4f}  below the initial capital {cash['shortfall_probability']:.4f}")
    for h, p, b in zip(plan["horizons"]["steps"], plan["horizons"]["ruin_probability"], plan["horizons"]["bands"]):
        print(f"  ruined after {h} periods: {p:.4f}  median value {investment * (1.0 + b[0]):,.2f}")
    # the same plan when the drift is not taken as known (SPEC.md 2.7 / 4.21): mu_step is a mean over len(returns_df) rows, so every
    # path draws its own drift from the standard error of that mean and walks on it -- the variance this adds grows like T^2
    unsure = mcp.simulate_paths(mu_step, cov_step, w, n_steps=T, n_paths=n_paths, seed=seed, v0=investment, cashflow=-take, target=investment,
                                drift_uncertainty=mcp.drift_cov(returns_df))
    print(f"  with drift uncertainty (the mean of {len(returns_df)} rows, drift std {unsure['drift_uncertainty']['drift_std']:.5f} per period): "
          f"ruin probability {unsure['cashflow']['ruin_probability']:.4f} against {cash['ruin_probability']:.4f} with the drift known")
    # the same plan on a glide path (SPEC.md 4.14 / 5.14): the weights move once a year, in equal steps, from the optimum to the
    # minimum-variance portfolio of the same sweep -- de-risking while the capital is drawn down
    mc = res["Monte Carlo"]
    w_safe = mc["all_weights"][int(np.argmin(mc["all_risks"]))]
    glided = mcp.simulate_paths(mu_step, cov_step, w, n_steps=T, n_paths=n_paths, seed=seed, v0=investment, cashflow=-take,
                                target=investment, horizons=[2 * af, 4 * af, 6 * af], bands=(50.0,),
                                glide=mcp.glide_path(w, w_safe, T, af))
    print(f"  glide path to the minimum-variance weights ({len(glided['glide']['breaks'])} yearly moves): ruin probability "
          f"{glided['cashflow']['ruin_probability']:.4f} against {cash['ruin_probability']:.4f} held  median value at the end "
          f"{investment * (1.0 + glided['horizons']['bands'][-1][0]):,.2f} against {investment * (1.0 + plan['horizons']['bands'][-1][0]):,.2f}")
    # the same plan under a floor-and-ceiling spending rule (SPEC.md 4.16 / 5.16): once a year the withdrawal moves to 1.5 % of what
    # is there, but is cut by at most 2.5 % and raised by at most 5 % -- it spends less after a crash and more after a rally.  The
    # fixed plan as a rule (every = 0: no review) is the withdrawal plan above bit for bit, with the total paid out per path on top
    payout = {}
    for label, rule in (("fixed", mcp.spending_rule("constant", 0.015, every=0, first=take)),
                        ("dynamic", mcp.spending_rule("floor_ceiling", 0.015, every=af, down=0.025, up=0.05, first=take))):
        o = mcp.simulate_paths(mu_step, cov_step, w, n_steps=T, n_paths=n_paths, seed=seed, v0=investment, spending=rule, store=True)
        payout[label] = (o["spending"]["ruin_probability"],) + tuple(np.percentile(o["withdrawn"].astype(np.float64), (5.0, 50.0)))
    (pd_, d5, d50), (pf, f5, f50) = payout["dynamic"], payout["fixed"]
    print(f"  floor-and-ceiling spending (reviewed yearly, cut <= 2.5 %, raise <= 5 %): ruin probability {pd_:.4f} against {pf:.4f} fixed  "
          f"5 % / median payout {d5:,.2f} / {d50:,.2f} against {f5:,.2f} / {f50:,.2f}")
    # how long the money lasts (SPEC.md 4.17 / 5.17): the periods a path ended with money left, as the lifetime that 95 % of the paths
    # reach and the median one; a path that is not ruined inside the plan counts its whole length
    life = {label: mcp.simulate_paths(mu_step, cov_step, w, n_steps=T, n_paths=n_paths, seed=seed, v0=investment, lifetime=True,
                                      lifetime_levels=(5, 50), **how)["lifetime"]
            for label, how in (("fixed", dict(cashflow=-take)),
                               ("dynamic", dict(spending=mcp.spending_rule("floor_ceiling", 0.015, every=af, down=0.025, up=0.05, first=take))))}
    print(f"  lifetime of the plan, 5 % / median of {T} periods: fixed {life['fixed']['quantiles'][5.0]} / {life['fixed']['quantiles'][50.0]}  "
          f"floor-and-ceiling {life['dynamic']['quantiles'][5.0]} / {life['dynamic']['quantiles'][50.0]}  "
          f"(ruined inside the plan: {life['fixed']['n_ruined']} and {life['dynamic']['n_ruined']} of {n_paths} paths)")
    # how to rebalance (SPEC.md 4.18 / 5.18): the optimum held over the same 6 years without withdrawals, traded back to its weights
    # every quarter, or looked at every period and traded only when an asset has left its 5/25 band (5 points, or a quarter of its
    # target), at 0.2 % of what is traded either way
    quarter = max(1, af // 4)
    kw = dict(n_steps=T, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100, rebalance_cost=0.002, store=True)
    cal = mcp.simulate_paths(mu_step, cov_step, w, rebalance=quarter, tolerance=0.0, **kw)
    band = mcp.simulate_paths(mu_step, cov_step, w, rebalance=1, tolerance=mcp.tolerance_bands(w, absolute=0.05, relative=0.25), **kw)
    for label, o in (("quarterly calendar", cal), ("5/25 bands", band)):
        tb = o["tolerance"]
        print(f"  rebalancing by {label}: mean trades {tb['trades']['mean']:.2f} of {tb['n_reviews']} reviews  median turnover "
              f"{np.percentile(tb['turnover']['paths'].astype(np.float64), 50.0):.4f}  VaR = {o['var']:+.4f}  CVaR = {o['cvar']:+.4f}")
    # the same weights with the first asset held through a protective put, on simulated paths (SPEC.md 4.8 / 5.7): the put is
    # applied inside the path kernel at the price level of every path, so the floor shows in the tail and in the drawdown, and
    # the premium (2 % of the price here, in price units) in the mean.  The model is the UNHEDGED returns' mean and covariance.
    raw = mcp.returns_matrix(resampled, {})
    spots = [float(resampled[n].iloc[-1]) for n in names]
    put = options.strategy_rows("Protective Put", S, premium_put=0.02 * S)
    for label, kw in (("unhedged", {}), ("hedged", {"overlay": {0: put}, "spot": spots})):
        o = mcp.simulate_paths(raw.mean().values, raw.cov().values, w, n_steps=af, n_paths=n_paths, seed=seed, v0=investment,
                               drawdown=True, **kw)
        print(f"protective put on {a0} ( {label} ): mean {o['mean']:+.4f}  VaR95 {o['var']:+.4f}  CVaR95 {o['cvar']:+.4f}  "
              f"mean max drawdown {o['drawdown']['mean']:+.4f}")
    # the same allocation bought and held, and traded back to the weights every 3 periods at 10 bp of the amount traded
    # (SPEC.md 4.5): a dollar allocation drifts with the prices instead of being rebalanced after every period for free
    for label, kw in (("bought and held", {"rebalance": "never"}),
                      ("rebalanced every 3 periods at 10 bp", {"rebalance": 3, "rebalance_cost": 1e-3})):
        held = mcp.simulate_paths(mu_step, cov_step, w, n_steps=af, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100, **kw)
        print(f"max-Sharpe allocation {label}: mean {held['mean']:+.4f}  std {held['std']:.4f}  VaR95 {held['var']:+.4f}  "
              f"CVaR95 {held['cvar']:+.4f}  Sharpe {held['sharpe']:.4f}")
    # the same weights under two regimes (SPEC.md 2.6 / 4.13, Markov switching): a calm and a crisis regime fitted to the observed rows
    # by Baum-Welch, each with its own means and covariance; the fan starts from the regime of the last row
    from monte_carlo_portfolio_amd import regimes as rg
    rfit = mcp.fit_regimes(returns_df)
    print(f"regime fit: p01 = {rfit.p01:.4f}  p10 = {rfit.p10:.4f}  P(crisis next) = {rfit.start:.4f}  log-likelihood gain "
          f"{rfit.loglik - rfit.loglik_iid:.2f} ({'no evidence of' if rg.no_evidence(rfit, len(returns_df)) else 'evidence of'} two regimes "
          f"over {len(returns_df)} rows)")
    rsim = mcp.simulate_paths(rfit.mu0, rfit.cov0, w, n_steps=af, n_paths=n_paths, seed=seed, v0=investment, rf=user_rf / 100,
                              drawdown=True, regimes=(rfit.p01, rfit.p10, rfit.mu1, rfit.cov1, rfit.start))
    print(f"  optimum without regimes: VaR = {sim['var']:+.4f}  CVaR = {sim['cvar']:+.4f}  mean max drawdown = {sim['drawdown']['mean']:+.4f}")
    print(f"  optimum with regimes:    VaR = {rsim['var']:+.4f}  CVaR = {rsim['cvar']:+.4f}  mean max drawdown = "
          f"{rsim['drawdown']['mean']:+.4f}  (long-run share of crisis steps {rsim['regimes']['stationary'] * 100:.1f} %)")
    # downside protection three ways on the same weights and model (SPEC.md 4.15 / 5.15): left alone, the protective put above (static,
    # paid for up front), and an 80 % floor held dynamically at a multiplier of 4 (CPPI: four times the cushion above the floor in the
    # portfolio, the rest riskless).  The gap probability is the share of paths that end below 80 % of the capital: the dynamic floor
    # holds while every step stays above -1 / m, so under small Gaussian steps it is 0; steps as large as these rows', and crash
    # jumps, gap through it -- the number to read next to the put's premium
    floor_T = np.float32(0.8 * investment)
    for draws, dkw in (("Gaussian draws", {}), ("fitted jumps", {"jumps": tuple(jfit[:4])})):
        for label, kw in (("unprotected", {}), ("protective put", {"overlay": {0: put}, "spot": spots}),
                          ("80 % floor at m = 4", {"protect": (0.8, 4.0)})):
            if "overlay" in kw and dkw:
                print(f"protection on {draws} ( {label} ): not built (the overlay is not combined with jumps)")
                continue
            args = dict(n_steps=af, n_paths=n_paths, seed=seed, v0=investment, drawdown=True, store=True, **kw, **dkw)
            try:
                o = mcp.simulate_paths(raw.mean().values, raw.cov().values, w, **args)
            except ValueError:            # the fitted jumps carry more variance than the covariance leaves: keep the diffusion whole
                o = mcp.simulate_paths(raw.mean().values, raw.cov().values, w, chol=np.linalg.cholesky(raw.cov().values), **args)
            gap = o["protect"]["gap_probability"] if "protect" in o else float(np.mean(o["terminal"] < floor_T))
            print(f"protection on {draws} ( {label} ): VaR95 {o['var']:+.4f}  CVaR95 {o['cvar']:+.4f}  mean max drawdown "
                  f"{o['drawdown']['mean']:+.4f}  gap probability {gap:.4f}")
    return res, sim


if __name__ == "__main__":
    data = os.path.join(ROOT, "tests", "golden", "data")
    default = [os.path.join(data, f) for f in ("Avalanche Historical Data.csv", "Cardano Historical Data.csv",
                                               "NEAR_USD Binance Historical Data.csv")]
    main(sys.argv[1:] or default)

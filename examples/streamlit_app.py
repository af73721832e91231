#!/usr/bin/env python3
"""A thin Streamlit front end over monte_carlo_portfolio_amd: the four tabs of the reference's app.py, rebuilt on the
package's functions (optional shim).  Nothing is computed here: every number comes from the
surface the package exposes under the reference's names.

    streamlit run examples/streamlit_app.py

Tabs (reference lines they stand for): per-asset statistics (app.py:463-497), option strategy and P/L curve
(app.py:499-653), the five-method random-weight sweep on historical rows plus the optimum re-scored on simulated paths
(app.py:655-783 + the MI355X path engine), forecast (app.py:785-809: there ARIMA/GARCH; here a Monte Carlo fan from the
path engine's values at intermediate horizons, and for the selected asset a second fan with GARCH(1,1) volatility fitted to its
rows -- the tab says so).
Streamlit is not part of the test image; tests/test_gpu_shim.py runs this file under a recording stand-in module.
"""
import os
import sys

import numpy as np
import streamlit as st

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import monte_carlo_portfolio_amd as mcp                      # noqa: E402
from monte_carlo_portfolio_amd import ingest, options, sweep  # noqa: E402

st.set_page_config(page_title="Monte Carlo portfolio (MI355X engine)", layout="wide")
state = st.session_state
state.setdefault("frames", [])                               # [(asset name, DataFrame[Date, Price])]
state.setdefault("investment_amount", 10000.0)

# ---- sidebar: files and settings (app.py:378-458) -------------------------------------------------------------------
with st.sidebar:
    compat = st.checkbox("reference CSV parsing (thousands separators are NOT parsed)", value=False)
    for up in st.file_uploader("price CSV files (Date + Price/Close column)", type=["csv"], accept_multiple_files=True) or []:
        if up.name not in [n for n, _ in state["frames"]]:
            df = mcp.read_csv_file(up, compat=compat, report=st.error)
            if df is not None:
                state["frames"].append((ingest.asset_name(up.name), df))
    period = st.selectbox("analysis period", ["M", "Q", "W"], index=0)
    annual_factor = ingest.ANNUAL_FACTOR[period]
    user_rf = st.number_input("risk-free rate (the reference's units: 3.0 means '3 %', used as entered)", value=3.0)
    state["investment_amount"] = st.number_input("capital", value=float(state["investment_amount"]))
    n_paths = int(st.number_input("simulated paths for the optimum", value=1_000_000, step=100_000))

if not state["frames"]:
    st.info("upload at least one CSV file")
    st.stop()

names, prices, resampled = ingest.align_prices(state["frames"], period)
with st.sidebar:
    lo = np.array([st.number_input(f"min weight {n}", 0.0, 1.0, 0.0) for n in names])
    hi = np.array([st.number_input(f"max weight {n}", 0.0, 1.0, 1.0) for n in names])

tab_stats, tab_options, tab_sweep, tab_forecast = st.tabs(["statistics", "options", "portfolio", "forecast"])

with tab_stats:                                               # app.py:484-495
    st.dataframe(mcp.stats_table(resampled, period, user_rf))

option_rows = {}
with tab_options:                                             # app.py:499-653
    asset = st.selectbox("asset", names)
    strategy = st.selectbox("strategy", list(options.STRATEGIES))
    spot = float(resampled[asset].iloc[-1])
    if strategy != options.STRATEGIES[0]:
        rows = options.strategy_rows(strategy, spot, premium_put=st.number_input("put premium", value=0.02),
                                     premium_call=st.number_input("call premium", value=0.02))
        option_rows[asset] = rows
        grid = options.payoff_grid(spot)
        st.line_chart({"price": grid, "P/L": mcp.calculate_payoff(rows, spot, spot, grid)})
        st.write({"breakeven": mcp.calculate_breakeven(rows, spot)})
        # next to the payoff curve: the asset alone on simulated one-year paths, unhedged and held through the strategy inside
        # the path kernel (SPEC.md 4.8; the premiums, fractions of the price above, in price units here)
        r1 = mcp.returns_matrix(resampled, {})[asset]
        held = [(t, k, p * spot, q) for t, k, p, q in rows]
        hedge = {}
        for side, kw in (("unhedged", {}), ("hedged", {"overlay": {0: held}, "spot": [spot]})):
            o = mcp.simulate_paths([r1.mean()], [[r1.var()]], [1.0], n_steps=annual_factor, n_paths=n_paths, seed=12345, alpha=0.95,
                                   drawdown=True, **kw)
            hedge[side] = {"VaR 5%": o["var"], "CVaR 5%": o["cvar"], "mean max drawdown": o["drawdown"]["mean"]}
        st.write({"simulated hedge": hedge})

with tab_sweep:                                               # app.py:655-783
    returns_df = mcp.returns_matrix(resampled, option_rows)
    results = mcp.run_all_methods(returns_df, min_weights=lo, max_weights=hi, user_rf=user_rf, annual_factor=annual_factor,
                                  investment_amount=state["investment_amount"])
    for method, r in results.items():
        i = r["opt_idx"]
        st.subheader(method)
        st.scatter_chart({"risk %": r["all_risks"] * 100, "return %": r["all_returns"] * 100})
        st.write({"optimum": i, "risk %": float(r["all_risks"][i] * 100), "return %": float(r["all_returns"][i] * 100),
                  "allocation": dict(zip(names, np.round(r["dollar_vals"], 2).tolist()))})
    # three more criteria over the weights the "Monte Carlo" method drew (SPEC.md 5.24): the reference's own series statistics of
    # returns_df @ w for every row of the sweep, and for the chosen optimum the dates of its deepest historical drawdown
    criterion = st.selectbox("historical criterion over the Monte Carlo sweep's weights", list(sweep.EXTRA_METHODS), 0)
    mc = results["Monte Carlo"]
    perf = sweep.score_performance(returns_df.to_numpy(dtype=np.float64), mc["all_weights"], risk_free=user_rf / 100.0,
                                   ann_factor=annual_factor)
    key = {"Sortino": "sortino_ratio", "Max Drawdown": "max_drawdown", "Calmar": "calmar"}[criterion]
    j = sweep.select_optimum(criterion, perf[key])
    peak, trough = int(perf["peak_row"][j]), int(perf["trough_row"][j])
    st.subheader(f"best {criterion} of the sweep (historical rows)")
    st.write({"criterion": criterion, "best": j, "score": float(perf[key][j]), "Sortino": float(perf["sortino_ratio"][j]),
              "max drawdown %": float(perf["max_drawdown"][j] * 100), "Calmar": float(perf["calmar"][j]),
              "drawdown peak": str(returns_df.index[peak]) if peak >= 0 else None,
              "drawdown trough": str(returns_df.index[trough]) if trough >= 0 else None,
              "allocation": dict(zip(names, np.round(sweep.allocation(mc["all_weights"][j], state["investment_amount"]), 2).tolist()))})
    # how far the Monte Carlo optimum can be trusted (SPEC.md 5.25): the same weights scored on resamples of the rows
    block = max(1.0, float(st.number_input("mean block length of the resampled sweep (1 = i.i.d. rows)", value=1.0)))
    rs = sweep.score_resampled(returns_df.to_numpy(dtype=np.float64), mc["all_weights"], user_rf, annual_factor, n_replicates=1000,
                               block=block, seed=12345)
    summ = sweep.resample_summary(rs, mc["all_weights"], point=mc["opt_idx"])
    won, i = summ["Monte Carlo"], mc["opt_idx"]
    st.subheader("resampled sweep: 1,000 bootstrap replicates of the historical rows")
    st.write({"optimum's win share %": won["point_win_share"] * 100, "in the top 5 % of, %": won["point_top5_share"] * 100,
              "portfolios that win at least once": int((won["wins"] > 0).sum()),
              "95 % interval of its Sharpe": [float(v) for v in summ["sharpe"]["interval"][:, i]],
              "resampled weights": dict(zip(names, np.round(won["resampled_weights"], 4).tolist())),
              "its own weights": dict(zip(names, np.round(mc["weights"], 4).tolist()))})
    w = results["Monte Carlo"]["weights"]
    mu_step, cov_step = returns_df.mean().values, returns_df.cov().values          # per period (app.py:679-680 before annualising)
    sim = mcp.simulate_paths(mu_step, cov_step, w, n_steps=annual_factor, n_paths=n_paths, seed=12345,
                             v0=state["investment_amount"], rf=user_rf / 100.0, drawdown=True)
    st.subheader("max-Sharpe weights on simulated one-year paths (MI355X path engine)")
    st.write({k: sim[k] for k in ("n", "mean", "std", "sharpe", "var", "cvar", "min", "max")})
    st.write({"max drawdown: mean": sim["drawdown"]["mean"], "DaR": sim["drawdown"]["dar"], "CDaR": sim["drawdown"]["cdar"],
              "worst": sim["drawdown"]["worst"]})
    # the risk pie next to the dollar pie of the optimum (SPEC.md 4.10 / 5.9): every asset's share of the simulated CVaR and volatility
    att = mcp.simulate_paths(mu_step, cov_step, w, n_steps=annual_factor, n_paths=n_paths, seed=12345,
                             v0=state["investment_amount"], rf=user_rf / 100.0, attribution=True)["attribution"]
    st.subheader("where the risk of the max-Sharpe weights comes from (component CVaR and volatility)")
    st.write({"risk attribution": {"weight %": dict(zip(names, np.round(np.asarray(w) * 100, 2).tolist())),
                                   "CVaR share %": dict(zip(names, np.round(att["cvar_share"] * 100, 2).tolist())),
                                   "volatility share %": dict(zip(names, np.round(att["vol_share"] * 100, 2).tolist()))}})
    # the same weights on paths resampled from the observed rows (stationary bootstrap, SPEC.md 2.1 / 4.4), next to the normal
    # model: hedged (option-overlay) rows keep their floor and cap here
    boot = mcp.simulate_bootstrap(returns_df, w, n_steps=annual_factor, n_paths=n_paths, block=3.0, seed=12345,
                                  v0=state["investment_amount"], rf=user_rf / 100.0)
    # and on fat-tailed Student-t steps with the normal model's mean and covariance, nu fitted to the rows (SPEC.md 2.2 / 4.6)
    nu = mcp.fit_student_t_dof(returns_df)
    tsim = mcp.simulate_paths(mu_step, cov_step, w, n_steps=annual_factor, n_paths=n_paths, seed=12345,
                              v0=state["investment_amount"], rf=user_rf / 100.0, dof=nu)
    keys = ("mean", "std", "sharpe", "var", "cvar", "min", "max")
    st.subheader("normal model vs. bootstrap of the observed rows (mean block 3) vs. Student-t")
    st.write({"normal model (mean / cov)": {k: sim[k] for k in keys}, "bootstrap of the observed rows": {k: boot[k] for k in keys},
              f"Student-t (ν = {nu}, fitted)": {k: tsim[k] for k in keys}})
    # the same allocation as a purchase: bought and held, or traded back to the weights every few periods at a proportional cost
    # of the amount traded (SPEC.md 4.5), instead of the free rebalance after every period of the paths above
    choices = ["never (buy and hold)", "every period", "every 3 periods", "every 6 periods"]
    held_choice = st.selectbox("rebalancing of the allocation", choices, 0)
    cost_bp = float(st.number_input("trading cost (basis points of the amount traded)", value=10.0))
    held = mcp.simulate_paths(mu_step, cov_step, w, n_steps=annual_factor, n_paths=n_paths, seed=12345,
                              v0=state["investment_amount"], rf=user_rf / 100.0,
                              rebalance=dict(zip(choices, ["never", 1, 3, 6]))[held_choice], rebalance_cost=cost_bp / 1e4)
    st.write({"allocation held": {"rebalancing": held_choice, "cost (bp)": cost_bp, **{k: held[k] for k in keys}}})

with tab_forecast:                                            # app.py:785-809
    # The reference forecasts 1, 3 and 6 periods ahead with a 95 % interval.  Here: a Monte Carlo fan from the path engine
    # (values at intermediate horizons, SPEC.md 4.3 / 5.2) -- each asset on its own (one-hot weight rows, from its last
    # price) and the Monte Carlo optimum (from the capital).
    st.info("Monte Carlo forecast on simulated paths (MI355X path engine), not the reference's ARIMA/GARCH models.")
    horizons, levels = [1, 3, 6], (2.5, 50.0, 97.5)
    _, _, asset_bands = mcp.simulate_paths(mu_step, cov_step, np.eye(len(names)), n_steps=horizons[-1], n_paths=n_paths, seed=12345,
                                           horizons=horizons, bands=levels, as_array=True)
    opt_fan = mcp.simulate_paths(mu_step, cov_step, w, n_steps=horizons[-1], n_paths=n_paths, seed=12345,
                                 v0=state["investment_amount"], horizons=horizons, bands=levels)["horizons"]["bands"]
    fans = [(n, float(resampled[n].iloc[-1]), asset_bands[:, a, :]) for a, n in enumerate(names)]
    fans.append(("Monte Carlo optimum", float(state["investment_amount"]), opt_fan))
    for name, v0, b in fans:
        st.subheader(f"{name}: forecast fan")
        fan = {"horizon": horizons, **{f"{q} %": (v0 * (1.0 + b[:, j])).tolist() for j, q in enumerate(levels)}}
        st.line_chart(fan, x="horizon")
        st.write({"asset": name, **fan})
    # the reference's forecast fits a GARCH(1,1) to the selected asset's returns and builds its interval from the summed variance
    # forecast; here the same asset with the variance ratio fitted to its rows (fit_garch, N = 1) and the paths started from the
    # fitted h0, today's regime (SPEC.md 4.9), beside the constant-variance fan above
    r_sel = mcp.returns_matrix(resampled, {})[asset]
    gfit = mcp.fit_garch(r_sel)
    gfan = mcp.simulate_paths([r_sel.mean()], [[r_sel.var()]], [1.0], n_steps=horizons[-1], n_paths=n_paths, seed=12345,
                              garch=gfit[:3], horizons=horizons, bands=levels)["horizons"]["bands"]
    last = float(resampled[asset].iloc[-1])
    st.subheader(f"{asset}: forecast fan with GARCH(1,1) volatility, started from today's regime")
    gchart = {"step": horizons, **{f"{q} %": (last * (1.0 + gfan[:, j])).tolist() for j, q in enumerate(levels)}}
    st.line_chart(gchart, x="step")
    st.write({"GARCH(1,1)": {"asset": asset, "alpha": gfit.alpha, "beta": gfit.beta, "h0": gfit.h0,
                             "log-likelihood gain over constant variance": gfit.loglik - gfit.loglik_iid}, **gchart})
    # contributions or withdrawals on the optimum (SPEC.md 4.7 / 5.6): the flow arrives after every period, a path whose value is
    # used up is ruined and stays so; the ruined share per horizon stands next to the fan
    flow = st.number_input("contribution (+) or withdrawal (-) per period", value=-0.05 * float(state["investment_amount"]))
    goal = st.number_input("target value at the end", value=float(state["investment_amount"]))
    plan = mcp.simulate_paths(mu_step, cov_step, w, n_steps=horizons[-1], n_paths=n_paths, seed=12345, v0=state["investment_amount"],
                              cashflow=float(flow), target=float(goal), horizons=horizons, bands=levels)
    pb = plan["horizons"]["bands"]
    st.subheader("Monte Carlo optimum with the cash flow: forecast fan and ruin probability")
    st.line_chart({"period": horizons, **{f"{q} %": (state["investment_amount"] * (1.0 + pb[:, j])).tolist()
                                          for j, q in enumerate(levels)}}, x="period")
    st.write({"cash flow per period": float(flow), "paid in (+) / taken out (-) in all": plan["cashflow"]["contributed"],
              "ruin probability per horizon": {int(h): float(p) for h, p in zip(horizons, plan["horizons"]["ruin_probability"])},
              "shortfall probability at the end": plan["cashflow"]["shortfall_probability"]})

"""monte_carlo_portfolio_amd -- MI355X-native Monte Carlo portfolio path engine.

Host side of the hot path named by BASELINE.json: a thin ctypes layer over libmcport.so
(hand-written HIP for gfx950) with the reference's function surface (app.py) above it, under the
reference's own names so an app.py-shaped Streamlit script can import them unchanged.
"""
from ._ffi import McpError, build, lib  # noqa: F401
from . import ingest_np  # noqa: F401  (the same ingest without pandas: file -> returns matrix -> mu, Sigma)
from .ingest import align_prices, load_prices, read_csv_file, returns_matrix  # noqa: F401
from .metrics import (annual_return, annual_volatility, calc_asset_stats, cvar, max_drawdown, sharpe_ratio,  # noqa: F401
                      sortino_ratio, stats_table, var)
from .options import (calc_option_return, calc_options_series, calculate_breakeven, calculate_payoff,  # noqa: F401
                      calculate_profit_loss_percent, strategy_rows)
from .simulate import Context, simulate_bootstrap, simulate_filtered, simulate_paths, simulate_sweep  # noqa: F401
from .glide import glide_law, glide_path  # noqa: F401
from .protect import floor_schedule, protect_law  # noqa: F401
from .spending import spending_law, spending_rule  # noqa: F401
from .lifetime import lifetime_law, survival_curve  # noqa: F401
from .tolerance import band_law, tolerance_bands  # noqa: F401
from .voltarget import ewma_decay, vol_target_law  # noqa: F401
from .underwater import spell_law  # noqa: F401
from .uncertainty import check_drift_uncertainty, drift_cov, drift_factor, drift_law  # noqa: F401
from .downside import check_downside, normal_law  # noqa: F401
from .relative import check_benchmark, relative_law  # noqa: F401
from .garch import FilteredRows, GarchFit, filter_rows, fit_garch  # noqa: F401
from .jumps import JumpFit, diffusion_cov, fit_jumps, jump_law  # noqa: F401
from .regimes import RegimeFit, fit_regimes, regime_law  # noqa: F401
from .student_t import fit_student_t_dof  # noqa: F401
from .sweep import EXTRA_METHODS, allocation, efficient_frontier, performance_finish, run_all_methods, run_sweep, score_performance  # noqa: F401

__all__ = [
    "McpError", "build", "lib", "Context", "simulate_paths", "simulate_bootstrap", "simulate_filtered", "simulate_sweep", "fit_student_t_dof", "fit_garch", "GarchFit", "filter_rows", "FilteredRows", "fit_jumps", "JumpFit", "jump_law", "diffusion_cov", "fit_regimes", "RegimeFit", "regime_law", "glide_path", "glide_law", "floor_schedule", "protect_law", "spending_rule", "spending_law", "survival_curve", "lifetime_law", "tolerance_bands", "band_law", "ewma_decay", "vol_target_law", "spell_law", "drift_cov", "drift_factor", "drift_law", "check_drift_uncertainty", "check_downside", "normal_law", "check_benchmark", "relative_law", "run_sweep", "run_all_methods", "efficient_frontier", "score_performance", "performance_finish", "EXTRA_METHODS",
    "allocation", "ingest_np", "read_csv_file", "align_prices", "load_prices", "returns_matrix", "calc_asset_stats", "stats_table",
    "sharpe_ratio", "sortino_ratio", "annual_volatility", "annual_return", "max_drawdown", "var", "cvar",
    "calc_option_return", "calc_options_series", "calculate_payoff", "calculate_breakeven",
    "calculate_profit_loss_percent", "strategy_rows",
]

"""tests/sweep_ref.py against the reference's recorded run (no GPU): the restatement the GPU edge tests measure the sweep kernels
with is itself pinned to the per-portfolio arrays the reference wrote (tests/golden/ref_script_arrays.npz), at the 1e-12
relative bar tests/test_gpu_sweep.py sets for the kernels.  Also here, because they need no device: the checks
`sweep.score_portfolios` makes before it calls the library."""
import json
import os

import numpy as np
import pytest

import sweep_ref
from monte_carlo_portfolio_amd import sweep

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, "golden", "ref_script.json")))
A = np.load(os.path.join(HERE, "golden", "ref_script_arrays.npz"))
RANDOM_METHODS = ("Monte Carlo", "VaR", "CVaR", "MPT")                    # the stream order of the reference's loop (quirk Q7)
METRIC = {"Monte Carlo": "sharpe", "VaR": "var_95", "CVaR": "cvar_95", "MPT": "sharpe"}


@pytest.mark.parametrize("key,seed", [("monthly_seed12345", 12345), ("weekly_seed12345", 12345)])
def test_restatement_matches_the_reference_run(key, seed):
    e = G[key]
    R, mean, cov = sweep.sweep_inputs(A[f"{key}__returns_df"], e["annual_factor"])
    assert list(R.shape) == e["returns_shape"]
    np.random.seed(seed)
    arrays = 0
    for m in RANDOM_METHODS:
        W = sweep.draw_weights(R.shape[1], 2500)                            # every method draws, recorded or not: one stream
        want = e["methods"][m]
        s = sweep_ref.score(R, mean, cov, W, e["user_rf"], 0.95)
        metric = s["sharpe"] if METRIC[m] == "sharpe" else -s[METRIC[m]]
        # what every recorded run has: the optimum, its point, the range of the metric
        opt = sweep.select_optimum(m, metric)
        assert len(W) == want["n"] and opt == want["opt_idx"], m
        np.testing.assert_allclose([s["port_std"][opt] * 100, s["port_return"][opt] * 100],
                                   [float.fromhex(v) for v in want["opt_point_pct"]], rtol=1e-12, atol=0)
        np.testing.assert_allclose([metric.min(), metric.max()], [float.fromhex(want["metric_min"]), float.fromhex(want["metric_max"])],
                                   rtol=1e-12, atol=0)
        if f"{key}__{m}__metrics" in A:                                     # and the per-portfolio arrays where they were kept
            np.testing.assert_allclose(s["port_std"] * 100, A[f"{key}__{m}__risks_pct"], rtol=1e-12, atol=0)
            np.testing.assert_allclose(s["port_return"] * 100, A[f"{key}__{m}__returns_pct"], rtol=1e-12, atol=0)
            np.testing.assert_allclose(metric, A[f"{key}__{m}__metrics"], rtol=1e-12, atol=0)
            arrays += 1
        # the longdouble sums agree with the binary64 ones to the bounds the GPU tests use
        assert np.all(np.abs(s["ret_ld"] - s["port_return"]) <= 2 * R.shape[1] * sweep_ref.U * s["ret_abs"])
        assert np.all(np.abs(s["tail_ld"] - s["cvar_95"]) <= 2 * sweep_ref.U * (s["tail_abs"] / s["n_tail"] + np.abs(s["cvar_95"])))
    assert arrays == (4 if key == "monthly_seed12345" else 0), "the golden file's per-portfolio arrays changed"


def test_series_is_the_kernel_order_sum():
    rng = np.random.default_rng(5)
    R, W = rng.normal(0, 0.02, (9, 4)), rng.dirichlet(np.ones(4), 3)
    want = np.array([[((R[r, 0] * W[p, 0] + R[r, 1] * W[p, 1]) + R[r, 2] * W[p, 2]) + R[r, 3] * W[p, 3] for p in range(3)]
                     for r in range(9)])
    assert np.array_equal(sweep_ref.series(R, W), want)


def test_score_rules_on_a_hand_case():
    """Four rows of one asset: the order statistics, the `<=` of the tail, the empty-tail and std <= 0 rules."""
    R = np.array([[0.03], [-0.01], [0.01], [-0.02]])
    s = sweep_ref.score(R, [0.5], [[0.04]], [[1.0], [0.0]], 0.1, 0.5)
    assert s["var_95"][0] == 0.0 and s["n_tail"][0] == 2 and s["cvar_95"][0] == (-0.01 - 0.02) / 2
    assert s["port_std"][0] == np.sqrt(0.04) and s["sharpe"][0] == (0.5 - 0.1) / np.sqrt(0.04)
    assert s["port_std"][1] == 0.0 and s["sharpe"][1] == 0.0 and s["var_95"][1] == 0.0 and s["n_tail"][1] == 4
    s = sweep_ref.score(R, [0.5], [[-1.0]], [[1.0]], 0.1, 1e-300)
    assert s["var_95"][0] == 0.03 and s["n_tail"][0] == 4 and np.isnan(s["port_std"][0]) and s["sharpe"][0] == 0.0


def _case():
    rng = np.random.default_rng(11)
    R = rng.normal(4e-4, 0.02, (12, 3))
    return R, R.mean(axis=0), np.cov(R.T), rng.dirichlet(np.ones(3), 4)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("name,cell,where", [("returns", (5, 2), "row 5, asset 2"), ("W", (3, 1), "portfolio 3, asset 1"),
                                              ("mean", (2,), "asset 2"), ("cov", (1, 2), "row 1, column 2")])
def test_score_portfolios_rejects_non_finite_input(bad, name, cell, where, monkeypatch):
    """A NaN or an infinity in any input array is a ValueError naming the array and the first offending cell, raised before the
    library or a device is touched (so this passes without a GPU)."""
    monkeypatch.setattr(sweep, "default_context", lambda *a, **k: pytest.fail("the context was asked for"))
    arrays = dict(zip(("returns", "mean", "cov", "W"), _case()))
    arrays[name] = arrays[name].copy()
    arrays[name][cell] = bad
    later = tuple(min(c + 1, n - 1) for c, n in zip(cell, arrays[name].shape))
    arrays[name][later] = bad                                               # a second one further on: the first is named
    with pytest.raises(ValueError, match=rf"NaN or infinite values in {name} \(first: {where}\)"):
        sweep.score_portfolios(arrays["returns"], arrays["mean"], arrays["cov"], arrays["W"], 0.03)


def test_score_portfolios_checks_shapes_before_the_library(monkeypatch):
    monkeypatch.setattr(sweep, "default_context", lambda *a, **k: pytest.fail("the context was asked for"))
    R, mean, cov, W = _case()
    with pytest.raises(ValueError, match="returns"):
        sweep.score_portfolios(R[:, :2], mean, cov, W, 0.03)
    with pytest.raises(ValueError, match="mean"):
        sweep.score_portfolios(R, mean[:2], cov, W, 0.03)
    with pytest.raises(ValueError, match="cov"):
        sweep.score_portfolios(R, mean, cov[:2], W, 0.03)
    out = sweep.score_portfolios(R, mean, cov, np.empty((0, 3)), 0.03)     # no portfolios: five empty arrays, no library call
    assert list(out) == ["port_return", "port_std", "sharpe", "var_95", "cvar_95"] and all(v.shape == (0,) for v in out.values())

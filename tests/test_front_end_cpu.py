"""The Python front end against the parent commit's, without a GPU: Context._call and the public functions are run over a
recording stand-in for the library (tests/front_end_cases.py) and compared with tests/golden/front_end_cases.json, which
tests/golden/make_front_end_cases.py wrote from a checkout of the parent commit."""
import json
import os

import pytest

import front_end_cases

HERE = os.path.dirname(os.path.abspath(__file__))

# The pairs of Context._call keywords whose entry point has no argument group for one of the two: the parent made the call as if
# that keyword had not been given, the table-driven _call refuses it.  Beside each, the public call of the same pair.
DROPPED_BEFORE = {
    "rows+dof": "bootstrap:dof",
    "rows+drawdown": "bootstrap:drawdown",
    "rows+overlay": "bootstrap:overlay",
    "rows+garch": "bootstrap:garch",
    "dof+period": "paths:dof+rebalance",
    "period+drawdown": "paths:drawdown+rebalance",
    "period+flows": "paths:cashflow+rebalance",
    "period+overlay": "paths:overlay+rebalance",
    "period+garch": "paths:garch+rebalance",
    "drawdown+horizons": "paths:drawdown+horizons",
    "drawdown+flows": "paths:cashflow+drawdown",
    "flows+overlay": "paths:cashflow+overlay",
    "flows+garch": "paths:cashflow+garch",
    "overlay+garch": "paths:garch+overlay",
}


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(HERE, "golden", "front_end_cases.json")) as f:
        return json.load(f)


def test_call_reaches_what_the_parent_reached(parent):
    got, want = front_end_cases.call_cases(), parent["call"]
    assert sorted(got) == sorted(want) and len(got) == 106
    assert {c["raises"][0] for c in want.values() if "raises" in c} == {"ValueError"}
    for name in sorted(want):
        if name in DROPPED_BEFORE:
            assert "calls" in want[name], name                                 # the parent made the call ...
            assert "raises" in parent["public"][DROPPED_BEFORE[name]], name    # ... that no public function lets through
            assert got[name].get("raises", [None])[0] == "ValueError", (name, got[name])
            entry = want[name]["calls"][0][0]
            assert got[name]["raises"][1].startswith(f"{entry} has no argument for "), got[name]
        else:
            assert got[name] == want[name], name


def test_dropped_pairs_are_those_of_the_entry_table():
    """DROPPED_BEFORE is exactly the pairs whose chosen entry point lacks the argument group of one of the two keywords and
    carries no refusal sentence of its own."""
    from monte_carlo_portfolio_amd import _ffi, simulate
    want = set()
    for a, b in front_end_cases.subsets(front_end_cases.CALL_KEYWORDS)[15:]:
        entry, text = next((e, t) for needs, e, t in simulate._ENTRY_CHOICE if set(needs) <= {a, b})
        if text is None and any(simulate._KEYWORD_GROUP[k] not in _ffi.SIMULATE_ENTRIES[entry] for k in (a, b)):
            want.add(f"{a}+{b}")
    assert want == set(DROPPED_BEFORE)


def test_public_functions_do_what_the_parent_did(parent, mcp_lib):
    got, want = front_end_cases.public_cases(mcp_lib), parent["public"]
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name

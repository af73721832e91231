"""What the relative tests share (SPEC.md 5.23): the summands of a raw record as NumPy forms them on x of the two rows (x as
tests/downside_ref.py forms it, mcp_terminal_to_x element by element), the record of their exact sums (math.fsum), the association
bound a device record is held to -- downside_ref's, (n - 1) 2^-53 sum |summand|, widened as that file widens it for log compounding
-- and the assertions of the one-step law with the standard-error multiples that the CPU twin and the GPU test both use."""
import math

import numpy as np

from downside_ref import U, to_x  # noqa: F401
from monte_carlo_portfolio_amd import _ffi, relative

COUNTS = relative.COUNT_FIELDS
SUMS = relative.SUM_FIELDS[5:]
LAW_SE = 5.0        # every figure of the law within this many standard errors


def summands(xk, xb, ck, cb):
    """({sum: its summands}, {count: its value}): d_k = x_k - c_k, d_b = x_b - c_b, e = d_k - d_b, a = x_k - x_b, every product rounded
    once, in the order SPEC.md 5.23 writes them; a sum over a set holds that set's summands alone."""
    xk, xb = np.asarray(xk, np.float64), np.asarray(xb, np.float64)
    dk, db = xk - ck, xb - cb
    e, a = dk - db, xk - xb
    under, over, up, down = a < 0, a > 0, xb > 0, xb < 0
    s = {"e1": e, "e2": e * e, "k1": dk, "b1": db, "k2": dk * dk, "b2": db * db, "kb": dk * db, "u1": a[under], "u2": (a * a)[under],
         "up_k": xk[up], "up_b": xb[up], "down_k": xk[down], "down_b": xb[down]}
    c = {"n": xk.size, "n_under": int(under.sum()), "n_over": int(over.sum()), "n_up": int(up.sum()), "n_down": int(down.sum())}
    return s, c


def exact(xk, xb, ck, cb):
    """(counts, {sum: (math.fsum of the summands, math.fsum of their magnitudes)}): computed once per pair of rows, shared by every
    layout the rows are launched in."""
    s, c = summands(xk, xb, ck, cb)
    return c, {f: (math.fsum(s[f]), math.fsum(np.abs(s[f]))) for f in SUMS}


def raw_record(xk, xb, ck, cb):
    """The raw record with exact sums -> a RELATIVE_SUMS_DTYPE scalar."""
    c, w = exact(xk, xb, ck, cb)
    rec = np.zeros((), _ffi.RELATIVE_SUMS_DTYPE)
    for f in COUNTS:
        rec[f] = c[f]
    for f in SUMS:
        rec[f] = w[f][0]
    return rec


def check_against(got, want, per_summand=0.0, note="", quiet=False):
    """A device record against `want` = exact(...): the counts exactly; every sum within (n - 1) 2^-53 sum |summand| of math.fsum of
    NumPy's summands, widened by per_summand * sum |summand| (log compounding: 4 * 2^-53); no word is NaN.  Every figure is printed
    before it is asserted."""
    counts, sums = want
    n = counts["n"]
    have = {f: int(got[f]) for f in COUNTS}
    if not quiet:
        print(f"{note} counts {have} want {counts}")
    assert have == counts, (note, have, counts)
    for f in SUMS:
        w, mass = sums[f]
        bound = (max(n - 1, 0) * U + per_summand) * mass
        err = abs(float(got[f]) - w)
        if not quiet or not err <= bound:
            print(f"{note} {f}: got {float(got[f])!r} want {w!r} err {err:.3e} bound {bound:.3e}")
        assert not math.isnan(float(got[f])), (note, f)
        assert err <= bound, (note, f, float(got[f]), w, err, bound)


def check_record(got, xk, xb, ck, cb, per_summand=0.0, note="", quiet=False):
    check_against(got, exact(xk, xb, ck, cb), per_summand, note, quiet)


def same_to_association(a, b, xk, xb, ck, cb, note=""):
    """Two device records of the same values summed in different partitions: the counts exactly, every sum within twice the
    association bound, since each lies within one bound of the exact sum."""
    counts, sums = exact(xk, xb, ck, cb)
    for f in COUNTS:
        assert int(a[f]) == int(b[f]) == counts[f], (note, f)
    for f in SUMS:
        gap, bound = abs(float(a[f]) - float(b[f])), 2 * max(counts["n"] - 1, 0) * U * sums[f][1]
        assert gap <= bound, (note, f, gap, bound)


def record_of(block):
    """The RELATIVE_SUMS_DTYPE scalar of a result's 'relative' block."""
    rec = np.zeros((), _ffi.RELATIVE_SUMS_DTYPE)
    for f in relative.SUM_FIELDS:
        rec[f] = block["sums"][f]
    return rec


def law_assertions(rec, law, n, note=""):
    """The finished record of n one-step Gaussian pairs against relative_law: every figure within LAW_SE standard errors.  With
    r the correlation of the pair: se(tracking error) = te / sqrt(2 n); se(beta) = sqrt((1 - r^2) var_k / var_b / n); se(r) =
    (1 - r^2) / sqrt(n); se(IR) = sqrt((1 + IR^2 / 2) / n); se(p_under) = sqrt(p (1 - p) / n)."""
    r, ir, p = law["correlation"], law["information_ratio"], law["p_under"]
    figs = {"tracking_error": law["tracking_error"] / math.sqrt(2.0 * n),
            "beta": math.sqrt((1.0 - r * r) * law["var_k"] / law["var_b"] / n),
            "correlation": (1.0 - r * r) / math.sqrt(n),
            "information_ratio": math.sqrt((1.0 + 0.5 * ir * ir) / n),
            "p_under": math.sqrt(p * (1.0 - p) / n)}
    for name, se in figs.items():
        print(f"{note} {name}: got {float(rec[name])!r} law {law[name]!r} se {se:.3e} -> {(float(rec[name]) - law[name]) / se:+.2f} se")
    for name, se in figs.items():
        assert abs(float(rec[name]) - law[name]) < LAW_SE * se, (note, name, float(rec[name]), law[name], se)

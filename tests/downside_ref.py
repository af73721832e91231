"""What the downside tests share (SPEC.md 5.22): x as mcp_terminal_to_x forms it, the summands of a raw record as NumPy forms them,
the record of their exact sums (math.fsum), the association bound a device record is held to, and the assertions of the normal law."""
import ctypes
import math

import numpy as np

from monte_carlo_portfolio_amd import _ffi, downside

U = 2.0 ** -53
SUMS = ("s1", "s2", "s3", "s4", "b1", "b2", "l1", "l2", "u1")


def to_x(values, v0=1.0, compounding="simple"):
    """binary64 x of binary32 values: one division per element (simple), or the library's own expm1 element by element (log)."""
    v = np.asarray(values, np.float32)
    if compounding == "simple":
        return v.astype(np.float64) / float(np.float32(v0)) - 1.0
    prm = _ffi.make_params(1, 1, 1, "log", v0)
    fn = _ffi.lib().mcp_terminal_to_x
    return np.array([fn(ctypes.byref(prm), float(t)) for t in v.ravel()], np.float64).reshape(v.shape)


def summands(x, c, tau):
    """{sum: its summands}: d = x - c, e = x - tau, every product rounded once, in the order SPEC.md 5.22 writes them."""
    d, e = x - c, x - tau
    d2, e2 = d * d, e * e
    lo, hi = e < 0, e > 0
    return {"s1": d, "s2": d2, "s3": d2 * d, "s4": d2 * d2, "b1": d[lo], "b2": d2[lo], "l1": e[lo], "l2": e2[lo], "u1": e[hi]}, lo, hi


def raw_record(x, c, tau):
    """The raw record of x with exact sums (math.fsum) -> a DOWNSIDE_SUMS_DTYPE scalar."""
    s, lo, hi = summands(np.asarray(x, np.float64), c, tau)
    rec = np.zeros((), _ffi.DOWNSIDE_SUMS_DTYPE)
    rec["n"], rec["n_below"], rec["n_above"] = x.size, int(lo.sum()), int(hi.sum())
    for f in SUMS:
        rec[f] = math.fsum(s[f])
    return rec


def check_record(got, x, c, tau, per_summand=0.0, note=""):
    """A device record against NumPy on x: the counts exactly; every sum within (n - 1) 2^-53 sum |summand| of math.fsum of NumPy's
    summands, widened by per_summand * sum |summand| (log compounding: 4 * 2^-53).  Every figure is printed before it is asserted."""
    s, lo, hi = summands(np.asarray(x, np.float64), c, tau)
    n = x.size
    counts = (int(got["n"]), int(got["n_below"]), int(got["n_above"]))
    print(f"{note} n={n} counts {counts} want {(n, int(lo.sum()), int(hi.sum()))}")
    assert counts == (n, int(lo.sum()), int(hi.sum())), note
    for f in SUMS:
        want, mass = math.fsum(s[f]), math.fsum(np.abs(s[f]))
        bound = (max(n - 1, 0) * U + per_summand) * mass
        err = abs(float(got[f]) - want)
        print(f"{note} {f}: got {float(got[f])!r} want {want!r} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (note, f, float(got[f]), want, err, bound)
        assert bound <= 1e-12 * mass or n > 9000        # at the crafted sizes the association bound is below SPEC.md 6's


def same_to_association(a, b, x, c, tau, note=""):
    """Two device records of the same values x summed in different partitions: the counts exactly, every sum within twice the
    association bound, since each lies within one bound of the exact sum."""
    s, _, _ = summands(np.asarray(x, np.float64), c, tau)
    for f in ("n", "n_below", "n_above"):
        assert int(a[f]) == int(b[f]), (note, f)
    for f in SUMS:
        gap, bound = abs(float(a[f]) - float(b[f])), 2 * max(x.size - 1, 0) * U * math.fsum(np.abs(s[f]))
        assert gap <= bound, (note, f, gap, bound)


def law_assertions(rec, sigma, n, note=""):
    """The finished record of n draws of a normal x at tau = its mean: every figure within 5 standard errors of its law."""
    law = downside.normal_law(0.0, sigma, 0.0)
    figs = {"p_below": (rec["p_below"], 0.5, 0.5 / math.sqrt(n)),
            "L2/n": (rec["downside_deviation"] ** 2, sigma * sigma / 2, sigma * sigma * math.sqrt(1.25 / n)),
            "skewness": (rec["skewness"], 0.0, math.sqrt(6.0 / n)),
            "excess_kurtosis": (rec["excess_kurtosis"], 0.0, math.sqrt(24.0 / n)),
            "omega": (rec["omega"], 1.0, law["omega_se1"] / math.sqrt(n))}
    assert abs(law["omega"] - 1.0) < 1e-12 and abs(law["l2"] - sigma * sigma / 2) < 1e-15 * sigma * sigma + 1e-30
    for name, (got, want, se) in figs.items():
        print(f"{note} {name}: got {float(got)!r} law {want!r} se {se:.3e} -> {(float(got) - want) / se:+.2f} se")
    for name, (got, want, se) in figs.items():
        assert abs(float(got) - want) < 5 * se, (note, name, float(got), want, se)

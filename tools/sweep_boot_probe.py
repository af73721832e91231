"""Timing probe for the resampled historical sweep (mcp_sweep_resampled, SPEC.md 5.25) as whole host calls (uploads, the kernels, the
download of 5 P B scores): rows x assets x portfolios x replicates, the median, minimum and maximum of CALLS calls after WARMUP
warm-up calls, one process.  Beside them, on the host: the NumPy restatement (tests/sweep_boot_ref.py) on a few replicates, its time
per replicate scaled to the call's B (a scaled figure, said so in the output) and its scores compared bit for bit with the call's, and from the counts the device wrote what the score
kernel's early stop saves: the sorted rows a wave really walks in its two walks (whole trips of 8 until every lane has passed rank_hi,
then until a trip's last row is above every lane's var) over the 2 R rows of two full walks, on a sample of portfolios.

    python tools/sweep_boot_probe.py [out.json] [--kernels-only]     (--kernels-only: a few calls and no host work, for a kernel trace)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from monte_carlo_portfolio_amd import sweep  # noqa: E402

SHAPES = ((252, 16, 2500, 1000, 1.0), (1260, 16, 10_000, 4096, 1.0))
WARMUP, CALLS = 2, 7
WALK, WAVE, CHUNK = 8, 64, 256
P_SMALL, B_SMALL = 500, 8          # what the restatement is run on: timed and scaled, and compared with the device's scores


def walked_share(y, counts, alpha, sample=40):
    """Rows walked per wave over 2 R, for the first `sample` portfolios: the kernel's two loops replayed on the host."""
    import sweep_boot_ref as ref_
    B, R = counts.shape
    rank_lo, rank_hi, gamma = ref_.percentile_rank(R, alpha)
    c = counts.astype(np.int64)
    walked = total = 0
    for p in range(min(sample, len(y))):
        perm = np.argsort(y[p], kind="stable")
        ys = y[p][perm]
        cum = np.cumsum(c[:, perm], axis=1)                         # [B, R]
        k_hi = np.argmax(cum > rank_hi, axis=1)                     # the position at which a lane passes rank_hi
        k_lo = np.argmax(cum > rank_lo, axis=1)
        a, b = ys[k_lo], ys[k_hi]
        var = np.where(gamma >= 0.5, b - (b - a) * (1.0 - gamma), a + (b - a) * gamma)
        n_in = (ys[None, :] <= var[:, None]).sum(axis=1)            # rows of the tail per lane
        for q0 in range(0, B, CHUNK):
            for w0 in range(q0, min(q0 + CHUNK, B), WAVE):
                lanes = slice(w0, min(w0 + WAVE, B))
                t1 = k_hi[lanes].max() // WALK + 1
                t2 = min(n_in[lanes].max() // WALK + 1, -(-R // WALK))
                walked += min(t1 * WALK, R) + min(t2 * WALK, R)
                total += 2 * R
    return walked / total


def main(out_path, kernels_only):
    import sweep_boot_ref as ref_
    rows = []
    for R, N, P, B, block in SHAPES:
        rng = np.random.default_rng(R + N)
        Rc = np.ascontiguousarray(rng.normal(0.0004, 0.02, (R, N)))
        W = np.random.RandomState(7).dirichlet(np.ones(N), P)
        ts = []
        for it in range((1 + 2) if kernels_only else (WARMUP + CALLS)):
            t0 = time.perf_counter()
            out = sweep.score_resampled(Rc, W, 0.03, 252, 0.95, B, block, seed=1, counts=(it == 0))
            if it >= WARMUP:
                ts.append(time.perf_counter() - t0)
            if it == 0:
                counts = out["counts"]
                head = {k: out[k][:P_SMALL, :B_SMALL].copy() for k in sweep.RESAMPLED_KEYS}
            del out
        if kernels_only:
            continue
        row = {"rows": R, "assets": N, "portfolios": P, "replicates": B, "block": block, "calls": CALLS, "warmup": WARMUP,
               "call_ms": {"median": float(np.median(ts)) * 1e3, "min": min(ts) * 1e3, "max": max(ts) * 1e3},
               "scores_bytes": 5 * P * B * 8}
        b_small, p_small = B_SMALL, min(P, P_SMALL)
        t0 = time.perf_counter()
        want = ref_.resampled(Rc, W[:p_small], 0.03, 252, 0.95, 1, 0, b_small, block)
        per = (time.perf_counter() - t0) / b_small * (P / p_small)
        for k in sweep.RESAMPLED_KEYS:                                  # the timed call computes what the restatement computes
            assert np.ascontiguousarray(head[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (R, k)
        row["first_scores_equal_restatement"] = [p_small, b_small]
        row["numpy_restatement"] = {"measured_replicates": b_small, "measured_portfolios": p_small, "s_per_replicate_scaled_to_P": per,
                                    "s_scaled_to_call": per * B}
        row["sorted_rows_walked_over_2R"] = walked_share(ref_.series(Rc, W[:40]), counts, 0.95)
        rows.append(row)
        print(f"rows {R} x assets {N} x portfolios {P} x replicates {B}: call {row['call_ms']['median']:.2f} ms "
              f"(min {row['call_ms']['min']:.2f}, max {row['call_ms']['max']:.2f}); NumPy restatement scaled {per * B:.1f} s; "
              f"sorted rows walked {row['sorted_rows_walked_over_2R'] * 100:.1f} % of two full walks", flush=True)
    if not kernels_only:
        doc = {"what": "whole host calls, wall clock around a call that ends in a stream synchronise, one process on one MI355X; a single-box "
                       "number.  The NumPy figure is measured on few replicates and portfolios and scaled, not run in full.", "shapes": rows}
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else os.path.join(ROOT, "profiles", "sweep_boot.json"), "--kernels-only" in sys.argv)

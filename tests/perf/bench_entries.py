"""The f(A) entries estimator (kt_entries_fun) on the benchmark graph
(graphs.chung_lu(), n = 1M, nnz = 10M): every tril edge (5M pairs), N = 256
probes, m = 30, deflation by the device's leading eigenvector (k = 1).  A
script, not a test; one JSON line (also written to --out).

  * wall time per call (best of --repeat, after a warm-up call) against
    kra.diag_fun with the same arguments in the same run: the difference is
    what the pairs cost;
  * the pair kernels (profile slot 9: k_entries_accumulate per sweep and
    k_entries_e0 once) as a share of the sweeps' pass time (slot 3) in one
    profiled call, and their byte rate;
  * the A/B of the pair table in the given order against the table sorted by
    the first end's position in the sweep's row order (KT_ENTRIES_SORT=1, read
    per call; the results are the same bits);
  * the existing route to entries, kt_function_multiple_entries (one Arnoldi
    run per distinct row), timed on a 1,000-edge sample at tol 1e-12.  The
    time is reported as measured and not extrapolated;
  * the sums of the estimate over the edges and over the diagonal, against
    nothing: no trace identity exists for off-diagonal entries, so these only
    record what the run computed."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (torch's ROCm runtime first)
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import krylov_robustness_amd as kra  # noqa: E402
from krylov_robustness_amd import graphs  # noqa: E402
from krylov_robustness_amd.greedy import _tril_edges  # noqa: E402


def best(fn, repeat):
    ts, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, min(ts), ts


def stage(msg):
    print(f"[bench_entries] {msg}", file=sys.stderr, flush=True)


def profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    out = fn()
    ctx.profile(False)
    return out, {s: ctx.profile_read(s) for s in (3, 7, 8, 9)}, {s: ctx.profile_busy(s) for s in (3, 9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--probes", type=int, default=256)
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entries", "bench_entries.json"))
    a = ap.parse_args()
    N, m, P = a.probes, a.m, 16
    A = graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0)
    n = A.shape[0]
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    lam, u = kra.eigs_leading(D, ctx=ctx)
    Q = np.asfortranarray(u[:, None])
    I, J = _tril_edges(A.tocsc())
    pairs = np.stack([I, J], axis=1)
    npairs = len(pairs)
    out = {"workload": f"entries exp, chung_lu n={n} nnz={A.nnz}, all tril edges", "npairs": npairs, "probes": N,
           "lanczos_m": m, "kdef": 1, "lambda1": lam, "source_digest": kra._lib.source_digest()}
    run_e = lambda pr=pairs: kra.entries_fun(D, pr, N, m=m, seed=0, deflate=Q, ctx=ctx)
    run_d = lambda: kra.diag_fun(D, N, m=m, seed=0, deflate=Q, ctx=ctx)

    stage(f"graph and eigenvector ready, {npairs} pairs")
    run_e()  # warm-up: buffers, the basis allocations, the hub CSR
    run_d()
    redone0 = ctx.yform_redone()
    r, t_e, ts_e = best(run_e, a.repeat)
    out["guard_redos_per_call"] = (ctx.yform_redone() - redone0) / a.repeat
    d, t_d, ts_d = best(run_d, a.repeat)
    out.update({"entries_fun_s": t_e, "entries_fun_s_all": ts_e, "diag_fun_s": t_d, "diag_fun_s_all": ts_d,
                "pairs_cost_s": t_e - t_d, "entries_over_diag": t_e / t_d})

    stage(f"entries_fun {t_e:.4f} s, diag_fun {t_d:.4f} s")
    # one profiled call: slot 9 against the sweeps' passes (slot 3), byte rate
    _, slots, busy = profiled(ctx, run_e)
    nsw = (N + P - 1) // P
    # per sweep and pair: two Y rows (8 P each), two Q rows, the table entry, two sums read and written
    acc_bytes = nsw * npairs * (2 * 8.0 * P + 2 * 8.0 + 16.0 + 4 * 8.0)
    out.update({
        "pass_ms": slots[3][1], "pass_launches": slots[3][0], "pass_busy_ms": busy[3],
        "combine_ms": slots[7][1], "start_ms": slots[8][1],
        "pairs_ms": slots[9][1], "pairs_launches": slots[9][0], "pairs_busy_ms": busy[9],
        "pairs_share_of_pass_time": slots[9][1] / slots[3][1] if slots[3][1] else None,
        "pairs_GBps": acc_bytes / (slots[9][1] * 1e-3) / 1e9 if slots[9][1] else None,
        "pairs_gather_GB_per_sweep": npairs * 2 * 8.0 * P / 1e9,
    })

    stage("profiled; the sorted table")
    # the A/B of the pair table's order (same bits either way)
    os.environ["KT_ENTRIES_SORT"] = "1"
    run_e()
    rs, t_s, ts_s = best(run_e, a.repeat)
    _, slots_s, _ = profiled(ctx, run_e)
    del os.environ["KT_ENTRIES_SORT"]
    out.update({"sorted_entries_fun_s": t_s, "sorted_entries_fun_s_all": ts_s, "sorted_pairs_ms": slots_s[9][1],
                "sorted_over_given_pairs_ms": slots_s[9][1] / slots[9][1] if slots[9][1] else None,
                "sorted_same_bits": bool(np.array_equal(rs.esum, r.esum) and np.array_equal(rs.esum2, r.esum2)
                                         and np.array_equal(rs.e0, r.e0))})

    # what the run computed (no identity to hold these against)
    est = r.mean
    out.update({"sum_estimate_over_edges": float(est.sum()), "sum_e0_over_edges": float(r.e0.sum()),
                "sum_diag_estimate": float(d.mean.sum()), "median_stderr_over_abs_mean":
                float(np.median(r.stderr / np.abs(est))), "sum_q_equal_to_diag_fun": bool(r.sum_q == d.sum_q)})

    stage("function_multiple_entries on the sample")
    # the existing route on a sample of edges (1-based pairs), as measured
    rng = np.random.default_rng(0)
    pick = np.sort(rng.choice(npairs, min(a.sample, npairs), replace=False))
    out["fme_sample_edges"] = len(pick)
    try:
        t0 = time.perf_counter()
        X, itr = kra.function_multiple_entries(D, pairs[pick] + 1, "exp", 1e-12, ctx=ctx)
        t_fme = time.perf_counter() - t0
        out.update({"fme_sample_s": t_fme, "fme_iterations": itr,
                    "fme_vs_estimate_median_rel_diff": float(np.median(np.abs(est[pick] - X) / np.abs(X)))})
    except kra.KrylovError as e:  # e.g. its Arnoldi bases (n x 128 x (it + 1) doubles) do not fit
        out["fme_error"] = str(e)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

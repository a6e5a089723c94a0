"""The diag f(A) estimator (kt_diag_fun) on the benchmark graph
(graphs.chung_lu(), n = 1M, nnz = 10M): N = 256 probes, m = 30, deflation by
the device's leading eigenvector (k = 1).  A script, not a test; one JSON line.

  * wall time per call (best of --repeat, after a warm-up call) against the
    only earlier route to the same quantity, timed in the same run:
    kra.lanczos_fmv on two 128-column host Rademacher blocks and the numpy
    reduction rowsum(Z .* Y), undeflated;
  * the combine + accumulate kernels (profile slot 7) as a share of the
    sweep's pass time (slot 3) in one profiled call, their byte rate, and
    beside it k_update<16>'s (slot 1) from the same run's explicit-form call;
  * the A/B of the sweep form: the y-form with basis (default) against the
    explicit CGS2 sweep, selected by the hot path's existing KT_SLQ_YFORM=0
    on a second context;
  * sum_i (d0 + dsum / N) against the spectral trace of
    tests/golden/config4_values.json, and the count of guard redos."""
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
from conftest import GOLDEN  # noqa: E402
from oracle import krylov_oracle as ko  # noqa: E402


def best(fn, repeat):
    ts, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, min(ts), ts


def profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    out = fn()
    ctx.profile(False)
    slots = {s: ctx.profile_read(s) for s in (0, 1, 3, 7, 8)}
    busy = {s: ctx.profile_busy(s) for s in (0, 1, 3, 7, 8)}
    return out, slots, busy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--probes", type=int, default=256)
    ap.add_argument("--m", type=int, default=30)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--no-parent-route", action="store_true")
    a = ap.parse_args()
    N, m, P = a.probes, a.m, 16
    A = graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0)
    n = A.shape[0]
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    lam, u = kra.eigs_leading(D, ctx=ctx)
    Q = np.asfortranarray(u[:, None])
    out = {"workload": f"diag exp, chung_lu n={n} nnz={A.nnz}", "probes": N, "lanczos_m": m, "kdef": 1,
           "lambda1": lam, "source_digest": kra._lib.source_digest()}
    run = lambda c, d: kra.diag_fun(d, N, m=m, seed=0, deflate=Q, ctx=c)

    run(ctx, D)  # warm-up: buffers, the basis allocations, the hub CSR
    redone0 = ctx.yform_redone()
    r, t_new, ts = best(lambda: run(ctx, D), a.repeat)
    out.update({"diag_fun_s": t_new, "diag_fun_s_all": ts,
                "guard_redos_per_call": (ctx.yform_redone() - redone0) / a.repeat})

    # the estimate against the spectral trace
    est = r.mean
    out["sum_estimate"] = float(est.sum())
    out["sum_d0"] = float(r.d0.sum())
    # the deflated part alone: sum_i dsum_i / N against sum_q / N (equal in exact arithmetic)
    out["sum_q_over_N"] = r.sum_q / N
    out["sum_dsum_over_N"] = float(r.dsum.sum() / N)
    out["sum_abs_dsum_over_N"] = float(np.abs(r.dsum).sum() / N)
    out["median_stderr_over_mean"] = float(np.median(r.stderr / np.abs(est)))
    vp = os.path.join(GOLDEN, "config4_values.json")
    if os.path.exists(vp) and (a.n, a.nnz) == (1_000_000, 10_000_000):
        tr = json.load(open(vp))["spectrum"]["tr_exp_topk"]
        out["trace_spectral"] = tr
        out["sum_estimate_rel_err"] = abs(out["sum_estimate"] - tr) / tr
        out["sum_d0_rel_err"] = abs(out["sum_d0"] - tr) / tr

    # one profiled call: slot 7 against the sweep's passes (slot 3), byte rates
    _, slots, busy = profiled(ctx, lambda: run(ctx, D))
    nsw = (N + P - 1) // P
    basis_bytes = 8.0 * m * n * P * nsw
    # combine: the basis once, y stored; finish: y and Q read; both add into two n-vectors
    comb_bytes = basis_bytes + nsw * (2 * 8.0 * n * P + 2 * 8.0 * n + 4 * 8.0 * n)
    out.update({
        "pass_ms": slots[3][1], "pass_launches": slots[3][0], "pass_busy_ms": busy[3],
        "combine_ms": slots[7][1], "combine_launches": slots[7][0],
        "start_ms": slots[8][1], "start_launches": slots[8][0],
        "combine_share_of_pass_time": slots[7][1] / slots[3][1] if slots[3][1] else None,
        "combine_GBps": comb_bytes / (slots[7][1] * 1e-3) / 1e9 if slots[7][1] else None,
        "d0_and_redo_explicit_k1_ms": slots[0][1], "d0_and_redo_explicit_k2_ms": slots[1][1],
    })

    # the A/B of the sweep form: every sweep explicit (KT_SLQ_YFORM=0 is read at context creation)
    os.environ["KT_SLQ_YFORM"] = "0"
    ctx2 = kra.Context(0)
    del os.environ["KT_SLQ_YFORM"]
    D2 = kra.DeviceMatrix(A, ctx2)
    run(ctx2, D2)
    r2, t_ex, ts2 = best(lambda: run(ctx2, D2), a.repeat)
    _, slots2, _ = profiled(ctx2, lambda: run(ctx2, D2))
    k2_bytes = slots2[1][0] * 40.0 * n * P  # y, u_prev, u_cur read, u_next written twice (block + basis slot)
    out.update({
        "explicit_form_s": t_ex, "explicit_form_s_all": ts2, "yform_over_explicit": t_new / t_ex,
        "explicit_k1_ms": slots2[0][1], "explicit_k2_ms": slots2[1][1], "explicit_combine_ms": slots2[7][1],
        "k_update16_GBps": k2_bytes / (slots2[1][1] * 1e-3) / 1e9 if slots2[1][1] else None,
        "forms_max_rel_diff": float(np.abs(r2.mean - est).max() / np.abs(est).max()),
    })
    D2.close()
    ctx2.close()

    # the earlier route: lanczos_fmv on host Rademacher blocks + the numpy reduction (undeflated)
    if not a.no_parent_route:
        acc = np.zeros(n)
        t_old = 0.0
        kra.lanczos_fmv(D, ko.rademacher(n, range(N, N + 16), 0), m=m, ctx=ctx)  # warm-up
        for b0 in range(0, N, 128):
            Z = ko.rademacher(n, range(b0, min(N, b0 + 128)), 0)
            t0 = time.perf_counter()
            Y = kra.lanczos_fmv(D, Z, m=m, ctx=ctx)
            acc += (Z * Y).sum(axis=1)
            t_old += time.perf_counter() - t0
        out.update({"lanczos_fmv_route_s": t_old, "speedup_over_lanczos_fmv_route": t_old / t_new,
                    "lanczos_fmv_route_sum": float(acc.sum() / N)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""kt_eigs_topk on the benchmark graph (graphs.chung_lu(), n = 1M, nnz = 10M),
k = 16, default tol, best of --repeat after a warm-up.  A script, not a test;
one JSON line (also written to --out).

  * wall time, block products, thick restarts (context stat 9), nconv, the
    largest resid / |lambda_1|, and the top-16 eigenvalues against the golden
    spectrum tests/golden/config4_values.json was made from;
  * one profiled call: slot 10 (k_eig_start, k_eig_rotate, k_eig_resid).  The
    solver's block SpMM, Gram and combine launches are the block-Krylov paths'
    own, which are not event-timed, so the rest of the call is reported as
    wall time minus slot 10;
  * the parent's only route to the same Q, scipy.sparse.linalg.eigsh(A, 16,
    which="LA") on the host, once, outside every timed GPU region
    (--skip-eigsh leaves it out);
  * k = 1 against kra.eigs_leading on the same context;
  * the replicated-graph case: rome x 16 on the block diagonal under a fixed
    symmetric permutation, k = 16: the multiplicities found and spmm."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (torch's ROCm runtime first)
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import krylov_robustness_amd as kra  # noqa: E402
from krylov_robustness_amd import graphs  # noqa: E402
from conftest import load_graph  # noqa: E402


def stage(msg):
    print(f"[bench_eigs] {msg}", file=sys.stderr, flush=True)


def timed(fn, repeat):
    ts, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, min(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--skip-eigsh", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigs", "bench_eigs.json"))
    a = ap.parse_args()
    A = graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0)
    n = A.shape[0]
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    out = {"workload": f"eigs_topk k=16, chung_lu n={n} nnz={A.nnz}", "k": 16,
           "source_digest": kra._lib.source_digest()}
    run = lambda: kra.eigs_topk(D, 16, ctx=ctx, return_info=True)  # noqa: E731
    stage("graph ready; warm-up")
    run()
    r0 = ctx.stat(9)
    (lam, V, (resid, nconv, spmm)), t, ts = timed(run, a.repeat)
    out.update({"wall_s": t, "wall_s_all": ts, "spmm": spmm, "restarts": (ctx.stat(9) - r0) // a.repeat,
                "nconv": nconv, "max_resid_over_lambda1": float(resid.max() / abs(lam[0])),
                "lambda": [float(x) for x in lam]})
    if (a.n, a.nnz) == (1_000_000, 10_000_000):
        with open(os.path.join(ROOT, "tests", "golden", "config4_values.json")) as f:
            gold = np.array(json.load(f)["spectrum"]["lambda_desc"])
        out["max_abs_diff_vs_golden_over_lambda1"] = float(np.abs(lam - gold[:16]).max() / abs(gold[0]))
    stage(f"k=16: {t:.3f} s, spmm {spmm}, nconv {nconv}")
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    run()
    launches, ms = ctx.profile_read(10)
    tp = time.perf_counter() - t0
    ctx.profile(False)
    out.update({"slot10_launches": launches, "slot10_ms": ms, "profiled_call_s": tp,
                "rest_of_call_ms": tp * 1e3 - ms,
                "note_slots": "block SpMM, Gram and combine launches are not event-timed in this library"})

    run1 = lambda: kra.eigs_topk(D, 1, ctx=ctx, return_info=True)  # noqa: E731
    lead = lambda: kra.eigs_leading(D, ctx=ctx)  # noqa: E731
    run1()
    lead()
    (l1, _, (res1, _, sp1)), t1, _ = timed(run1, a.repeat)
    (ll, _), tl, _ = timed(lead, a.repeat)
    out.update({"k1_topk_s": t1, "k1_topk_spmm": sp1, "k1_leading_s": tl,
                "k1_lambda_rel_diff": float(abs(l1[0] - ll) / abs(ll)), "k1_resid": float(res1[0])})
    stage(f"k=1: topk {t1:.3f} s, eigs_leading {tl:.3f} s")

    if not a.skip_eigsh:
        t0 = time.perf_counter()
        w = np.sort(sla.eigsh(A.astype(np.float64), k=16, which="LA", return_eigenvectors=True)[0])[::-1]
        out.update({"host_eigsh_s": time.perf_counter() - t0,
                    "host_eigsh_max_abs_diff_over_lambda1": float(np.abs(w - lam).max() / abs(lam[0]))})
        stage(f"scipy eigsh {out['host_eigsh_s']:.1f} s")

    # the replicated graph: every eigenvalue of rome, sixteen times
    R = load_graph("rome")
    wr = np.linalg.eigvalsh(R.toarray())[::-1]
    nr = 16 * R.shape[0]
    perm = np.random.default_rng(0).permutation(nr)
    B = sp.block_diag([R] * 16, format="csr")[perm][:, perm].tocsr()
    DB = kra.DeviceMatrix(B, ctx)
    runb = lambda: kra.eigs_topk(DB, 16, ctx=ctx, return_info=True)  # noqa: E731
    runb()
    (lb, Vb, (rb, ncb, spb)), tb, _ = timed(runb, a.repeat)
    mult = {f"{wr[i]:.6f}": int((np.abs(lb - wr[i]) <= 1e-9 * wr[0]).sum()) for i in range(3)}
    out["replicated"] = {"graph": f"rome x 16, n={nr}", "wall_s": tb, "spmm": spb, "nconv": ncb,
                         "multiplicities_found": mult, "max_resid_over_lambda1": float(rb.max() / wr[0]),
                         "orth": float(np.abs(Vb.T @ Vb - np.eye(16)).max())}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

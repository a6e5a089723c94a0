"""kt_diag_fun_bracket on the benchmark graph (graphs.chung_lu(1e6, 1e7, 2.5,
seed=0): n = 1M, the graph of bench_miobi_node.py): the 64 highest-degree
nodes at rtol = 1e-10, lam_hi = lambda_upper(A), beside trace_fun_update_nodes
on the same nodes -- the same sweeps with the other check.  A script, not a
test; one JSON line (also written to --out).  For the record, not a gate.

Per entry: wall time per call (the median of --calls calls after a warm-up
call), the call's sweeps, the sweep steps it queued (one SpMM pass over A each:
kt_context_stat 13, 14), its deepest column (stat 15) and the depth histogram;
from the profile of one further call, the summed and busy time of the check
launches (id 14) beside the sweeps' K1 and K2 (ids 0, 1).  For the bracket also
lambda_upper's wall time and value against normest and ||A||_inf, the flags, and
the largest relative gap (hi - lo) / lo.  trace_fun_update_nodes runs at tol =
1e-10 times its own largest |Xm| of a first call, the counterpart of a relative
1e-10 (at bench_nodes.py's 1e-6 exp(normest) every column stops at depth 3)."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (torch's ROCm runtime first)
import numpy as np
import scipy.sparse as sp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

import krylov_robustness_amd as kra  # noqa: E402
from krylov_robustness_amd import graphs  # noqa: E402


def stage(msg):
    print(f"[bench_bracket] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--it", type=int, default=0, help="the depth cap of both entries (0: their default, min(100, n))")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bracket", "bench_bracket.json"))
    a = ap.parse_args()
    A = sp.csr_matrix(graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0), dtype=np.float64)
    n = A.shape[0]
    deg = np.diff(A.indptr)
    nodes = np.argsort(-deg, kind="stable")[:a.cands]
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    out = {"workload": f"diag_fun_bracket rtol={a.rtol:g} beside trace_fun_update_nodes, {a.cands} highest degrees, "
                       f"chung_lu n={n} nnz={A.nnz}",
           "source_digest": kra._lib.source_digest(), "max_degree": int(deg.max()),
           "min_degree_of_candidates": int(deg[nodes].min()), "it": a.it or min(100, n), "runs": 1}
    stage("lambda_upper")
    t0 = time.perf_counter()
    mu = kra.lambda_upper(D, ctx=ctx)
    out["lambda_upper"] = {"value": mu, "wall_s": time.perf_counter() - t0, "normest": kra.normest(D, ctx=ctx),
                           "norm_inf": float(abs(A).sum(axis=1).max())}

    def leg(label, call):
        stage(f"{label}: warm-up call")
        first = call()
        walls = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            again = call()
            walls.append(time.perf_counter() - t0)
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(first, again))
        rec = {"wall_s_per_call_median": float(np.median(walls)), "wall_s_per_call_all": walls,
               "sweeps": ctx.stat(13), "sweep_steps_queued_spmm_passes": ctx.stat(14), "deepest_column": ctx.stat(15)}
        stage(f"{label}: wall {rec['wall_s_per_call_median'] * 1e3:.2f} ms per call; profiled call")
        ctx.profile(True)
        ctx.profile_reset()
        call()
        prof = {}
        for name, slot in (("k1_spmm_dot", 0), ("k2_update", 1), ("check_and_start", 14)):
            launches, ms = ctx.profile_read(slot)
            prof[name] = {"intervals": launches, "summed_ms": ms, "busy_ms": ctx.profile_busy(slot)}
        ctx.profile(False)
        rec["profile_one_call"] = prof
        return rec, first

    rec, (lo, hi, it, fl) = leg("diag_fun_bracket",
                                lambda: kra.diag_fun_bracket(D, nodes + 1, rtol=a.rtol, it=a.it or None, lam_hi=mu,
                                                             ctx=ctx))
    ok = fl != 2
    rec.update({"depth_histogram": {str(d): int(c) for d, c in enumerate(np.bincount(it)) if c},
                "flags": {str(f): int(c) for f, c in enumerate(np.bincount(fl, minlength=4)) if c},
                "max_rel_gap": float(np.max((hi[ok] - lo[ok]) / lo[ok])) if ok.any() else None,
                "lo_min": float(lo.min()), "lo_max": float(lo.max())})
    out["diag_fun_bracket"] = rec
    xm0, _, _ = kra.trace_fun_update_nodes(D, nodes + 1, 1e-6 * float(np.exp(out["lambda_upper"]["normest"])), ctx=ctx)
    tol = a.rtol * float(np.max(np.abs(xm0)))
    rec, (xm, it, lk) = leg("trace_fun_update_nodes",
                            lambda: kra.trace_fun_update_nodes(D, nodes + 1, tol, it=a.it or None, ctx=ctx))
    rec.update({"tol": tol, "depth_histogram": {str(d): int(c) for d, c in enumerate(np.bincount(it)) if c},
                "lucky": int(lk.sum()), "reached_it_unstopped": int(np.sum(it >= (a.it or min(100, n))))})
    out["trace_fun_update_nodes"] = rec
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

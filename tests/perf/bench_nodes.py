"""kt_trace_fun_update_nodes on the benchmark graph (graphs.chung_lu(1e6, 1e7,
2.5, seed=0): n = 1M): the 256 highest-degree nodes, fun = exp, tol = 1e-6
exp(normest(A)).  A script, not a test; one JSON line (also written to --out).
On this graph that tol lies above every X_1 .. X_3 (the hubs' early iterates
are orders of magnitude below their limits), so the lag-2 rule stops every
column at its first test, depth 3.  --tol2-rel r > 0 adds a
second leg at tol = r times the first leg's largest |Xm| (the recorded run used
1e-9, which turned out below the converged values' rounding noise: 83 columns
ran to it = 100; its batched restatement takes minutes).  Per leg:

  * wall time per call (the median of --calls calls after a warm-up call);
  * the call's sweeps, the sweep steps it queued (one SpMM pass over A each:
    kt_context_stat 13, 14) and its deepest column (stat 15), with the depth
    histogram of the 256 columns;
  * from the profile of one further call: the summed and the busy time of the
    new launches (id 14: k_node_check and k_unit_start) beside the sweeps' K1 and
    K2 (ids 0, 1);
  * the only correct route the parent has, the NumPy restatement
    (tests/nodes_ref.py): --host-cands candidates timed on a pool of
    --host-threads threads; the figure for 256 candidates is labelled an
    extrapolation;
  * max |device - restatement| / |Xm| over all 256, the restatement run here
    in its batched form (the same three-term recurrence and stopping rule on
    --chunk columns at a time, one scipy SpMM per step)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import torch  # noqa: F401  (torch's ROCm runtime first)
import numpy as np
import scipy.sparse as sp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import krylov_robustness_amd as kra  # noqa: E402
from krylov_robustness_amd import graphs  # noqa: E402
import nodes_ref as nr  # noqa: E402


def stage(msg):
    print(f"[bench_nodes] {msg}", file=sys.stderr, flush=True)


def batched_restatement(A, nodes, tol, it, chunk):
    """nodes_ref.node_update for many nodes: independent three-term recurrences
    advanced together, each column stopped by its own lag-2 rule."""
    n = A.shape[0]
    xm = np.zeros(len(nodes))
    iters = np.zeros(len(nodes), dtype=int)
    for c0 in range(0, len(nodes), chunk):
        idx = nodes[c0:c0 + chunk]
        p = len(idx)
        V = np.zeros((n, p))
        V[idx, np.arange(p)] = 1.0
        Vp = np.zeros((n, p))
        beta = np.zeros(p)
        al = [[] for _ in range(p)]
        off = [[] for _ in range(p)]
        xstop = np.zeros((p, 2))
        live = np.ones(p, dtype=bool)
        for j in range(1, it + 1):
            W = A @ V - Vp * beta
            a = np.einsum("ij,ij->j", V, W)
            W -= V * a
            beta = np.linalg.norm(W, axis=0)
            for q in np.flatnonzero(live):
                al[q].append(a[q])
                x = nr.x_of_tridiag(np.array(al[q]), np.array(off[q]), "exp")
                stop = False
                if j <= 2:
                    xstop[q, j - 1] = x
                elif abs(x - xstop[q, 0]) < tol:
                    stop = True
                else:
                    xstop[q] = (xstop[q, 1], x)
                if stop or beta[q] < 1e-8 or j == it:
                    live[q] = False
                    xm[c0 + q], iters[c0 + q] = x, j
                else:
                    off[q].append(beta[q])
            if not live.any():
                break
            Vp = V
            V = W / np.where(beta > 0.0, beta, 1.0)
    return xm, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--cands", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-cands", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--tol2-rel", type=float, default=0.0,
                    help="a second leg at tol = this times the first leg's largest |Xm| (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nodes", "bench_nodes.json"))
    a = ap.parse_args()
    A = sp.csr_matrix(graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0), dtype=np.float64)
    n = A.shape[0]
    deg = np.diff(A.indptr)
    nodes = np.argsort(-deg, kind="stable")[:a.cands]
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    tol = 1e-6 * float(np.exp(kra.normest(D, ctx=ctx)))
    out = {"workload": f"trace_fun_update_nodes exp, {a.cands} highest degrees, chung_lu n={n} nnz={A.nnz}",
           "source_digest": kra._lib.source_digest(), "max_degree": int(deg.max()),
           "min_degree_of_candidates": int(deg[nodes].min())}

    def leg(tol, label):
        stage(f"{label}: tol {tol:.3e}; warm-up call")
        xm, it, lk = kra.trace_fun_update_nodes(D, nodes + 1, tol, ctx=ctx)
        walls = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            x2, _, _ = kra.trace_fun_update_nodes(D, nodes + 1, tol, ctx=ctx)
            walls.append(time.perf_counter() - t0)
            assert x2.tobytes() == xm.tobytes()
        hist = np.bincount(it)
        rec = {"tol": tol, "wall_s_per_call_median": float(np.median(walls)), "wall_s_per_call_all": walls,
               "sweeps": ctx.stat(13), "sweep_steps_queued_spmm_passes": ctx.stat(14), "deepest_column": ctx.stat(15),
               "steps_needed_sum_over_sweeps_of_max_depth": int(sum(it[s:s + 16].max() for s in range(0, len(it), 16))),
               "depth_histogram": {str(d): int(c) for d, c in enumerate(hist) if c}, "lucky": int(lk.sum()),
               "reached_it_unstopped": int(np.sum(it >= min(100, n)))}
        stage(f"{label}: wall {rec['wall_s_per_call_median'] * 1e3:.2f} ms per call; profiled call")
        ctx.profile(True)
        ctx.profile_reset()
        kra.trace_fun_update_nodes(D, nodes + 1, tol, ctx=ctx)
        prof = {}
        for name, slot in (("k1_spmm_dot", 0), ("k2_update", 1), ("node_check_and_start", 14)):
            launches, ms = ctx.profile_read(slot)
            prof[name] = {"intervals": launches, "summed_ms": ms, "busy_ms": ctx.profile_busy(slot)}
        ctx.profile(False)
        rec["profile_one_call"] = prof
        if a.host_cands > 0:
            stage(f"{label}: host restatement")
            with ThreadPoolExecutor(a.host_threads) as pool:
                t0 = time.perf_counter()
                res = list(pool.map(lambda i: nr.node_update(A, int(i), tol), nodes[:a.host_cands]))
                hs = time.perf_counter() - t0
            rec.update({"host_numpy_s_for_timed_candidates": hs, "host_numpy_candidates_timed": a.host_cands,
                        "host_numpy_threads": a.host_threads,
                        # the timed candidates ran side by side; all of them would take this many such rounds
                        # if 16 ran side by side as fast as these did (they share the memory bus: a lower bound)
                        "host_numpy_s_for_all_candidates_EXTRAPOLATED_LOWER_BOUND":
                            hs * -(-a.cands // a.host_threads) / -(-a.host_cands // a.host_threads),
                        "host_timed_vs_device_rel": [abs(r[0] - xm[q]) / abs(xm[q]) for q, r in enumerate(res)]})
        stage(f"{label}: batched restatement of all candidates")
        t0 = time.perf_counter()
        xr, itr = batched_restatement(A, nodes, tol, min(100, n), a.chunk)
        rec.update({"batched_restatement_s": time.perf_counter() - t0,
                    "max_abs_device_minus_restatement_over_abs_xm": float(np.max(np.abs(xm - xr) / np.abs(xm))),
                    "max_abs_device_minus_restatement_over_tol": float(np.max(np.abs(xm - xr)) / tol),
                    "tol_over_min_abs_xm": tol / float(np.min(np.abs(xm))),
                    "tol_over_max_abs_xm": tol / float(np.max(np.abs(xm))),
                    "iter_differs_in": int(np.sum(it != itr)), "xm_min": float(xm.min()), "xm_max": float(xm.max())})
        return rec, xm

    # the issue's setting; on this graph it is above every |Xm|, so every column stops at its first test
    out["tol_1e-6_exp_normest"], xm = leg(tol, "tol = 1e-6 exp(normest)")
    if a.tol2_rel > 0.0:
        # a tol that resolves the candidates a greedy step chooses among: relative to the largest |Xm|
        out[f"tol_{a.tol2_rel:g}_max_abs_xm"], _ = leg(a.tol2_rel * float(np.max(np.abs(xm))),
                                                       f"tol = {a.tol2_rel:g} max|Xm|")
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""kt_miobi_break on the benchmark graph (graphs.chung_lu(1e6, 1e7, 2.5, seed=0):
n = 1M, 5M edges), t = 25, k = 100, refresh = 50.  A script, not a test; one
JSON line (also written to --out).

  * wall time of the call and, from the id-11 profile (one interval per step:
    k_miobi_score + k_miobi_pick), milliseconds per step;
  * that figure against the step's gather bytes, 2 x 256 B per live edge (the
    pair list itself adds 9 B per edge), as GB/s;
  * the recomputation's share of the wall time.  A recomputation is the
    window's removals applied through the pair-edit path, the device copy
    rebuilt from the edited host CSR, and eigs_topk; each is timed standalone
    through the same entry points on a fresh copy (DeviceMatrix.set_pairs on
    the first window's edges, the first eigs_topk after it, a second one
    without a rebuild), and their sum is set against the call's wall time.
    The same call with refresh = 0 is reported beside it;
  * the host route: the NumPy restatement's step (tests/miobi_ref.py: scores,
    argmin, update) on the same eigenpairs, 2 steps timed, per step, and that
    figure times k labelled as an extrapolation;
  * the first selections of the two runs, which must agree up to the first
    recomputation."""
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
import miobi_ref as mr  # noqa: E402


def stage(msg):
    print(f"[bench_miobi] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--t", type=int, default=25)
    ap.add_argument("--refresh", type=int, default=50)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "miobi", "bench_miobi.json"))
    a = ap.parse_args()
    A = graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0)
    n, edges = A.shape[0], A.nnz // 2
    ctx = kra.Context(0)
    out = {"workload": f"miobi_break t={a.t} k={a.k} refresh={a.refresh}, chung_lu n={n} nnz={A.nnz}",
           "source_digest": kra._lib.source_digest(), "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
    stage("graph ready; warm-up (4 steps on a copy)")
    kra.miobi_break(kra.DeviceMatrix(A, ctx), 4, t=a.t, refresh=2, ctx=ctx)

    def run(refresh):
        D = kra.DeviceMatrix(A, ctx)
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        e, info = kra.miobi_break(D, a.k, t=a.t, refresh=refresh, ctx=ctx)
        wall = time.perf_counter() - t0
        launches, ms = ctx.profile_read(11)
        ctx.profile(False)
        return e, info, wall, launches, ms

    e50, i50, w50, l50, ms50 = run(a.refresh)
    stage(f"refresh={a.refresh}: {w50:.3f} s, {l50} steps, {ms50 / max(l50, 1):.3f} ms per step")
    e0, i0, w0, l0, ms0 = run(0)
    stage(f"refresh=0: {w0:.3f} s")
    step_ms = ms50 / max(l50, 1)
    gather = 2 * 256 * edges
    out.update({
        "edges": int(edges), "nsel": int(len(e50)), "refreshes": i50["refreshes"], "nconv_min": i50["nconv_min"],
        "rob_score": i50["rob_score"], "wall_s": w50, "steps_profiled": l50, "steps_ms_total": ms50,
        "ms_per_step": step_ms, "gather_bytes_per_step": gather, "gather_GBps": gather / (step_ms * 1e-3) / 1e9,
        "wall_s_refresh0": w0, "ms_per_step_refresh0": ms0 / max(l0, 1), "rob_score_refresh0": i0["rob_score"],
        "steps_share_of_wall": ms50 * 1e-3 / w50,
        "same_edges_before_first_recompute": bool((e50[:a.refresh] == e0[:a.refresh]).all()),
    })
    D = kra.DeviceMatrix(A, ctx)
    t0 = time.perf_counter()
    lam, V = kra.eigs_topk(D, a.t, ctx=ctx)
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    lam, V = kra.eigs_topk(D, a.t, ctx=ctx)
    solve = time.perf_counter() - t0
    window = e50[:a.refresh if a.refresh > 0 else len(e50)]
    t0 = time.perf_counter()
    D.set_pairs(window, 0.0)
    edit = time.perf_counter() - t0
    t0 = time.perf_counter()
    kra.eigs_topk(D, a.t, ctx=ctx)
    after_edit = time.perf_counter() - t0
    rec = edit + after_edit
    out.update({"eigs_topk_first_call_s": first, "eigs_topk_s": solve, "set_pairs_window_s": edit,
                "set_pairs_window_edges": int(len(window)), "eigs_topk_after_edit_s": after_edit,
                "recompute_s_standalone": rec, "recomputes_in_call": i50["refreshes"],
                "recompute_share_of_wall": rec * i50["refreshes"] / w50})

    if a.host_steps > 0:
        stage("host restatement steps")
        V = np.array(V)
        V[:, 0] = np.abs(V[:, 0])
        e = np.array(lam)
        p, r, w = mr.upper_edges(A)
        alive = np.ones(len(p), dtype=bool)
        host_edges = []
        t0 = time.perf_counter()
        for _ in range(a.host_steps):
            live = np.flatnonzero(alive)
            q = int(live[int(np.argmin(mr.scores(V, e, p[live], r[live])))])
            alive[q] = False
            host_edges.append([int(r[q]) + 1, int(p[q]) + 1])
            V, e, _ = mr.update(V, e, int(p[q]), int(r[q]), float(w[q]), "reference")
        hs = (time.perf_counter() - t0) / a.host_steps
        out.update({"host_numpy_s_per_step": hs, "host_numpy_steps_timed": a.host_steps,
                    "host_numpy_s_for_k_steps_EXTRAPOLATED": hs * a.k,
                    "host_edges_match_device": bool((np.array(host_edges) == e50[:a.host_steps]).all())})
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

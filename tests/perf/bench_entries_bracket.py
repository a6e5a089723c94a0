"""kt_entries_fun_bracket on the benchmark graph (graphs.chung_lu(1e6, 1e7, 2.5,
seed=0): n = 1M, the graph of bench_bracket.py): the 256 edges with the largest
degree product at rtol = 1e-10, it = 100, lam_hi = lambda_upper(A), beside
kt_diag_fun_bracket on their 512 endpoints (repeats included) for scale -- the
same sweeps, one column per node instead of two per pair.  A script, not a
test; one JSON line (also written to --out).  For the record, not a gate.

Per entry: wall time per call (the median of --calls calls after a warm-up
call), the call's sweeps, the sweep steps it queued (one SpMM pass over A each:
kt_context_stat 13, 14) and the steps needed (per sweep its deepest column,
summed), the depth histogram and the flags; from the profile of one further
call, the summed and busy time of the check and start launches (id 14) beside
the sweeps' K1 and K2 (ids 0, 1).  With --ordinary N also one call (not timed
more than once) on N edges spread evenly over the edge list by degree product,
whose entries are expected to lie below what the method resolves: their flags
and depths."""
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
    print(f"[bench_entries_bracket] {msg}", file=sys.stderr, flush=True)


def hist(v, minlength=0):
    return {str(d): int(c) for d, c in enumerate(np.bincount(v, minlength=minlength)) if c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--ftol", type=float, default=1e-12)
    ap.add_argument("--it", type=int, default=100)
    ap.add_argument("--ordinary", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entries_bracket", "bench_entries_bracket.json"))
    a = ap.parse_args()
    A = sp.csr_matrix(graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0), dtype=np.float64)
    n = A.shape[0]
    deg = np.diff(A.indptr)
    L = sp.tril(A, -1).tocoo()
    prod = deg[L.row].astype(np.float64) * deg[L.col]
    order = np.argsort(-prod, kind="stable")
    top = order[:a.pairs]
    pairs = np.stack([L.row[top], L.col[top]], axis=1).astype(np.int64)
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    out = {"workload": f"entries_fun_bracket rtol={a.rtol:g} ftol={a.ftol:g} it={a.it}, the {a.pairs} edges of largest "
                       f"degree product, beside diag_fun_bracket on their {2 * a.pairs} endpoints, chung_lu n={n} "
                       f"nnz={A.nnz}",
           "source_digest": kra._lib.source_digest(), "max_degree": int(deg.max()),
           "degree_product_min_max": [float(prod[top].min()), float(prod[top].max())], "runs": 1}
    stage("lambda_upper")
    t0 = time.perf_counter()
    mu = kra.lambda_upper(D, ctx=ctx)
    out["lambda_upper"] = {"value": mu, "wall_s": time.perf_counter() - t0}

    def leg(label, call, per_sweep, calls):
        stage(f"{label}: warm-up call")
        first = call()
        walls = []
        for _ in range(calls):
            t0 = time.perf_counter()
            again = call()
            walls.append(time.perf_counter() - t0)
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(first, again))
        it, fl = first[2], first[3]
        needed = int(sum(it[s:s + per_sweep].max() for s in range(0, len(it), per_sweep)))
        rec = {"wall_s_per_call_median": float(np.median(walls)) if walls else None, "wall_s_per_call_all": walls,
               "sweeps": ctx.stat(13), "sweep_steps_queued_spmm_passes": ctx.stat(14), "sweep_steps_needed": needed,
               "deepest_column": ctx.stat(15), "depth_histogram": hist(it), "flags": hist(fl, 5)}
        stage(f"{label}: {rec['wall_s_per_call_median']} s per call, flags {rec['flags']}; profiled call")
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        call()
        rec["wall_s_profiled_call"] = time.perf_counter() - t0
        prof = {}
        for name, slot in (("k1_spmm_dot", 0), ("k2_update", 1), ("check_and_start", 14)):
            launches, ms = ctx.profile_read(slot)
            prof[name] = {"intervals": launches, "summed_ms": ms, "busy_ms": ctx.profile_busy(slot)}
        ctx.profile(False)
        rec["profile_one_call"] = prof
        return rec, first

    rec, (lo, hi, it, fl) = leg("entries_fun_bracket", lambda: kra.entries_fun_bracket(
        D, pairs, rtol=a.rtol, ftol=a.ftol, it=a.it, lam_hi=mu, ctx=ctx), 8, a.calls)
    ok = fl == 0
    rec.update({"max_rel_gap_of_flag_0": float(np.max((hi[ok] - lo[ok]) / np.minimum(abs(lo[ok]), abs(hi[ok]))))
                if ok.any() else None, "lo_min": float(np.nanmin(lo)), "lo_max": float(np.nanmax(lo))})
    out["entries_fun_bracket"] = rec
    ends = pairs.ravel()
    rec, (dlo, dhi, dit, dfl) = leg("diag_fun_bracket", lambda: kra.diag_fun_bracket(
        D, ends + 1, rtol=a.rtol, it=a.it, lam_hi=mu, ctx=ctx), 16, a.calls)
    out["diag_fun_bracket_on_the_endpoints"] = rec
    # the pair values in their natural unit
    sc = 0.5 * (dlo[0::2] + dlo[1::2])
    out["entries_fun_bracket"]["lo_over_half_diag_sum_min_max"] = [float(np.nanmin(lo / sc)), float(np.nanmax(lo / sc))]
    if a.ordinary > 0:
        pick = order[np.linspace(a.pairs, len(order) - 1, a.ordinary).astype(np.int64)]
        opairs = np.stack([L.row[pick], L.col[pick]], axis=1).astype(np.int64)
        rec, (olo, ohi, oit, ofl) = leg("entries_fun_bracket, ordinary edges", lambda: kra.entries_fun_bracket(
            D, opairs, rtol=a.rtol, ftol=a.ftol, it=a.it, lam_hi=mu, ctx=ctx), 8, 0)
        rec["degree_product_min_max"] = [float(prod[pick].min()), float(prod[pick].max())]
        rec["timed_calls"] = "the warm-up call and the profiled call only"
        out["entries_fun_bracket_ordinary_edges"] = rec
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

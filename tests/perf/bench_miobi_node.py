"""kt_miobi_break_node on the benchmark graph (graphs.chung_lu(1e6, 1e7, 2.5,
seed=0) binarised: n = 1M, 5M edges), t = 25, k = 100, refresh = 50 and 0.  A
script, not a test; one JSON line (also written to --out).

  * from the id-13 profile (one interval per queued step: k_miobi_node_score +
    k_miobi_node_pick), milliseconds per step.  With refresh = 0 every queued
    step is a real one.  With refresh = 50 a window queues up to 25 steps and
    the device ends it as soon as the removed-entry count reaches 50 -- on this
    graph after one hub -- so most intervals are pairs of no-op launches: the
    figure per REAL step (total / nsel) contains them and is labelled so;
  * bytes per step by DESIGN.md §4.2g's formula -- the live entries of the
    step's matrix x (256 + 4 + 1) B plus n x (8 + 256) B -- and the implied
    TB/s (refresh = 0 only, where the intervals are clean);
  * the call's wall time and the share of it that is the steps, the
    eigensolver runs, the staging of V and the row lists, and the edits of A
    (kt_context_stat 10-12: host microseconds of the last call);
  * the score kernel's VGPR count and scratch bytes from the compiler's
    resource report (--resource-report: the text hipcc prints with
    -Rpass-analysis=kernel-resource-usage for kt_miobi.hip; without the option
    the script runs hipcc itself);
  * the host route: the restatement's step (tests/miobi_node_ref.py: scores of
    all nodes, first minimum) on the same eigenpairs, chunked over rows on
    --host-threads threads, --host-steps steps timed; the figure times k is
    labelled an extrapolation."""
import argparse
import json
import os
import re
import subprocess
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
import miobi_node_ref as nr  # noqa: E402


def stage(msg):
    print(f"[bench_miobi_node] {msg}", file=sys.stderr, flush=True)


def resource_report(path):
    """(VGPRs, scratch bytes per lane, LDS bytes) of k_miobi_node_score."""
    if path:
        text = open(path).read()
    else:
        src = os.path.join(ROOT, "krylov_robustness_amd", "csrc", "kt_miobi.hip")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                            "-munsafe-fp-atomics", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                           capture_output=True, text=True, timeout=600)
        text = r.stderr
    at = text.find("k_miobi_node_score")
    if at < 0:
        return None
    block = text[at:]
    nxt = block.find("Function Name", 10)
    block = block[:nxt] if nxt > 0 else block

    def num(label):
        m = re.search(re.escape(label) + r":\s*(\d+)", block)
        return int(m.group(1)) if m else None
    return {"vgprs": num("VGPRs"), "agprs": num("AGPRs"), "scratch_bytes_per_lane": num("ScratchSize [bytes/lane]"),
            "lds_bytes_per_block": num("LDS Size [bytes/block]"), "occupancy_waves_per_simd": num("Occupancy [waves/SIMD]")}


def host_step(S, V, e, pool, threads):
    """The restatement's scores of all nodes and their first minimum, chunked over rows."""
    n = S.shape[0]
    c = np.exp(e)
    bounds = np.linspace(0, n, 4 * threads + 1).astype(int)

    def chunk(q):
        lo, hi = bounds[q], bounds[q + 1]
        R = S[lo:hi]
        sc = np.sum(c[None, :] * np.exp(-2.0 * V[lo:hi] * (R @ V)), axis=1)
        sc[np.diff(R.indptr) == 0] = np.inf
        o = int(np.argmin(sc))
        return float(sc[o]), lo + o
    return min(pool.map(chunk, range(len(bounds) - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--t", type=int, default=25)
    ap.add_argument("--refresh", type=int, default=50)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--resource-report", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "miobi", "bench_miobi_node.json"))
    a = ap.parse_args()
    A = graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0)
    A = nr.binarise(A)
    A.setdiag(0.0)
    A.eliminate_zeros()
    n = A.shape[0]
    ctx = kra.Context(0)
    out = {"workload": f"miobi_break_node t={a.t} k={a.k} refresh={a.refresh} and 0, chung_lu n={n} nnz={A.nnz}",
           "source_digest": kra._lib.source_digest(), "max_degree": int(A.getnnz(axis=1).max()),
           "kernel_resources": resource_report(a.resource_report)}
    stage(f"graph ready, max degree {out['max_degree']}; warm-up (2 steps on a copy)")
    kra.miobi_break_node(kra.DeviceMatrix(A, ctx), 2, t=a.t, refresh=0, ctx=ctx)

    first = None
    for refresh in (a.refresh, 0):
        D = kra.DeviceMatrix(A, ctx)
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        nodes, info = kra.miobi_break_node(D, a.k, t=a.t, refresh=refresh, ctx=ctx)
        wall = time.perf_counter() - t0
        launches, ms = ctx.profile_read(13)
        ctx.profile(False)
        host = {"eig_s": ctx.stat(10) * 1e-6, "stage_upload_s": ctx.stat(11) * 1e-6, "edit_s": ctx.stat(12) * 1e-6}
        k = len(nodes)
        stage(f"refresh={refresh}: {wall:.3f} s, {k} steps in {launches} queued, {ms:.3f} ms in all")
        removed = np.concatenate([[0], np.cumsum(2 * info["degrees"])])[:k]
        live = A.nnz - removed                                  # the live entries every step's matrix holds
        bytes_step = live * (256 + 4 + 1) + n * (8 + 256)
        rec = {
            "nsel": int(k), "refreshes": info["refreshes"], "nconv_min": info["nconv_min"], "rob_score": info["rob_score"],
            "degrees_first5": info["degrees"][:5].tolist(), "degree_sum": int(info["degrees"].sum()), "wall_s": wall,
            "steps_queued": launches, "steps_ms_total": ms, "bytes_per_step_first": int(bytes_step[0]),
            "bytes_per_step_last": int(bytes_step[-1]), "steps_share_of_wall": ms * 1e-3 / wall,
            "eig_s_inside_call": host["eig_s"], "eig_share_of_wall": host["eig_s"] / wall,
            "stage_upload_s": host["stage_upload_s"], "edit_s": host["edit_s"],
            "rest_of_wall_s_incl_final_eigs_topk_for_R1": wall - ms * 1e-3 - sum(host.values()),
        }
        if launches == k:
            rec["ms_per_step"] = ms / max(k, 1)
            rec["tb_per_s_by_the_formula"] = float(bytes_step.sum()) / (ms * 1e-3) / 1e12 if ms > 0 else None
        else:
            rec["ms_per_real_step_INCLUDING_NOOP_LAUNCHES"] = ms / max(k, 1)
        out[f"refresh{refresh}"] = rec
        if refresh == a.refresh:
            first = nodes

    if a.host_steps > 0:
        stage("host restatement steps")
        lam, V = kra.eigs_topk(kra.DeviceMatrix(A, ctx), a.t, ctx=ctx)
        V = np.array(V)
        V[:, 0] = np.abs(V[:, 0])
        ev = np.array(lam)
        host_nodes = []
        live = np.ones(n, dtype=bool)
        S = sp.csr_matrix(A)
        with ThreadPoolExecutor(a.host_threads) as pool:
            t0 = time.perf_counter()
            for _ in range(a.host_steps):
                _, r = host_step(S, V, ev, pool, a.host_threads)
                host_nodes.append(r + 1)
                v = V[r]
                ev = ev - (2.0 * v * V.sum(axis=0) - v * v)
                live[r] = False
                S = nr.current(A, live)
            hs = (time.perf_counter() - t0) / a.host_steps
        # (with refresh = 50 the device recomputes after the first hub, the host loop here does not: only the
        # first node is comparable)
        out.update({"host_numpy_s_per_step": hs, "host_numpy_steps_timed": a.host_steps,
                    "host_numpy_threads": a.host_threads, "host_numpy_s_for_k_steps_EXTRAPOLATED": hs * a.k,
                    "host_first_node_matches_device": bool(host_nodes[0] == first[0])})
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""kt_miobi_make on the benchmark graph (graphs.chung_lu(1e6, 1e7, 2.5, seed=0):
n = 1M, 5M edges), t = 25, k = 100, refresh = 50 and 0.  A script, not a test;
one JSON line (also written to --out).

  * m and the number of scored pairs at the first and the last step, and the
    pair-terms (pairs x t) of all steps.  The device does not report pair
    counts; they are recounted here from the same eigenpairs (eigs_topk with
    the call's seed on a matrix with the same entries) and the call's own
    selections: m (m - 1) / 2 minus the adjacent pairs among the first m ranks;
  * from the id-12 profile (one interval per step: k_miobi_make_score +
    k_miobi_make_pick), milliseconds per step and pair-terms per second;
  * the call's wall time and the share of it that is the steps, the
    eigensolver runs, the ranking / mask / uploads and the edits of A
    (kt_context_stat 10-12: host microseconds of the last call);
  * the score kernel's VGPR count and scratch bytes from the compiler's
    resource report (--resource-report: the text hipcc prints with
    -Rpass-analysis=kernel-resource-usage for kt_miobi.hip; without the option
    the script runs hipcc itself);
  * the host route: the restatement's step (tests/miobi_make_ref.py: scores
    over all non-adjacent candidate pairs, first maximum) on the same
    eigenpairs, chunked over candidate rows so that it fits in memory, on
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
import miobi_make_ref as mk  # noqa: E402


def stage(msg):
    print(f"[bench_miobi_make] {msg}", file=sys.stderr, flush=True)


def resource_report(path):
    """(VGPRs, scratch bytes per lane, LDS bytes) of k_miobi_make_score."""
    if path:
        text = open(path).read()
    else:
        src = os.path.join(ROOT, "krylov_robustness_amd", "csrc", "kt_miobi.hip")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                            "-munsafe-fp-atomics", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                           capture_output=True, text=True, timeout=600)
        text = r.stderr
    at = text.find("k_miobi_make_score")
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


def with_edges(A, edges0):
    """A with the 0-based pairs set to 1 (they are non-adjacent in A)."""
    if len(edges0) == 0:
        return sp.csr_matrix(A)
    i, j = np.asarray(edges0)[:, 0], np.asarray(edges0)[:, 1]
    E = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=A.shape).tocsr()
    return sp.csr_matrix(A + E + E.T)


def pair_counts(A, edges0, ms, windows, eig, t):
    """Scored pairs of every step: windows = [(first step, last step + 1)], the
    ranking of a window from eig() of the matrix at its start.  before[b] = the
    ranks a < b adjacent to b, so the first m ranks hold sum(before[:m])
    adjacent pairs."""
    out = np.zeros(len(edges0), dtype=np.int64)
    for lo, hi in windows:
        S = with_edges(A, edges0[:lo])
        lam, V = eig(S, t)
        cand = mk.candidates(np.abs(np.array(V)[:, 0]), int(ms[lo:hi].max()))
        sub = S[cand][:, cand].toarray() != 0
        before = np.triu(sub, 1).sum(axis=0).astype(np.int64)
        pos = {int(v): a for a, v in enumerate(cand)}
        for s in range(lo, hi):
            m = int(ms[s])
            out[s] = m * (m - 1) // 2 - int(before[:m].sum())
            ra, rb = sorted((pos[int(edges0[s, 0])], pos[int(edges0[s, 1])]))
            before[rb] += 1
    return out


def host_step(V, e, cand, sub, pool, threads):
    """The restatement's scores and first maximum over the candidate block,
    chunked over rows a (pairs (a, b > a) with sub[a, b] clear)."""
    W = V[cand]
    c = np.exp(e)
    m = len(cand)
    bounds = np.linspace(0, m, 8 * threads + 1).astype(int)

    def chunk(q):
        best = (-np.inf, -1, -1)
        for a in range(bounds[q], bounds[q + 1]):
            b = np.flatnonzero(~sub[a, a + 1:]) + a + 1
            if len(b) == 0:
                continue
            sc = np.sum(c[None, :] * np.exp(2.0 * W[a][None, :] * W[b]), axis=1)
            o = int(np.argmax(sc))
            if sc[o] > best[0]:
                best = (float(sc[o]), a, int(b[o]))
        return best
    res = list(pool.map(chunk, range(len(bounds) - 1)))
    return max(res, key=lambda r: (r[0], -r[1], -r[2]))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "miobi", "bench_miobi_make.json"))
    a = ap.parse_args()
    A = graphs.chung_lu(a.n, a.nnz, gamma=2.5, seed=0)
    A = mk.binarise(A)
    n = A.shape[0]
    ctx = kra.Context(0)
    out = {"workload": f"miobi_make t={a.t} k={a.k} refresh={a.refresh} and 0, chung_lu n={n} nnz={A.nnz}",
           "source_digest": kra._lib.source_digest(), "max_degree": int(A.getnnz(axis=1).max()),
           "kernel_resources": resource_report(a.resource_report)}
    stage(f"graph ready, max degree {out['max_degree']}; warm-up (2 steps on a copy)")
    kra.miobi_make(kra.DeviceMatrix(A, ctx), 2, t=a.t, refresh=1, ctx=ctx)

    def eig(S, t):
        return kra.eigs_topk(kra.DeviceMatrix(S, ctx), t, ctx=ctx)

    def run(refresh):
        D = kra.DeviceMatrix(A, ctx)
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        e, info = kra.miobi_make(D, a.k, t=a.t, refresh=refresh, ctx=ctx)
        wall = time.perf_counter() - t0
        launches, ms = ctx.profile_read(12)
        ctx.profile(False)
        host = {"eig_s": ctx.stat(10) * 1e-6, "rank_mask_upload_s": ctx.stat(11) * 1e-6, "edit_s": ctx.stat(12) * 1e-6}
        return e, info, wall, launches, ms, host

    for refresh in (a.refresh, 0):
        e, info, wall, launches, ms, host = run(refresh)
        stage(f"refresh={refresh}: {wall:.3f} s, {launches} steps, {ms / max(launches, 1):.3f} ms per step")
        k = len(e)
        step = refresh if refresh > 0 else max(k, 1)
        windows = [(lo, min(lo + step, k)) for lo in range(0, k, step)]
        pairs = pair_counts(A, e - 1, info["m"], windows, eig, a.t)
        terms = int(pairs.sum()) * a.t
        tag = f"refresh{refresh}"
        out[tag] = {
            "nsel": int(k), "refreshes": info["refreshes"], "nconv_min": info["nconv_min"], "rob_score": info["rob_score"],
            "m_first": int(info["m"][0]), "m_last": int(info["m"][-1]), "pairs_first": int(pairs[0]),
            "pairs_last": int(pairs[-1]), "pair_terms_all_steps": terms, "wall_s": wall, "steps_profiled": launches,
            "steps_ms_total": ms, "ms_per_step": ms / max(launches, 1),
            "pair_terms_per_s": terms / (ms * 1e-3) if ms > 0 else None,
            "steps_share_of_wall": ms * 1e-3 / wall, "eig_s_inside_call": host["eig_s"],
            "eig_share_of_wall": host["eig_s"] / wall, "rank_mask_upload_s": host["rank_mask_upload_s"],
            "rank_mask_upload_share_of_wall": host["rank_mask_upload_s"] / wall, "edit_s": host["edit_s"],
            "edit_share_of_wall": host["edit_s"] / wall,
            "rest_of_wall_s_incl_final_eigs_topk_for_R1": wall - ms * 1e-3 - sum(host.values()),
        }
        if refresh == a.refresh:
            first = e

    if a.host_steps > 0:
        stage("host restatement steps")
        lam, V = eig(A, a.t)
        V = np.array(V)
        V[:, 0] = np.abs(V[:, 0])
        ev = np.array(lam)
        maxdeg = out["max_degree"]
        host_edges, added = [], []
        with ThreadPoolExecutor(a.host_threads) as pool:
            t0 = time.perf_counter()
            S = sp.csr_matrix(A)
            for _ in range(a.host_steps):
                m = min(maxdeg + a.k, n)
                cand = mk.candidates(V[:, 0], m)
                sub = S[cand][:, cand].toarray() != 0
                _, ra, rb = host_step(V, ev, cand, sub, pool, a.host_threads)
                i, j = int(cand[ra]), int(cand[rb])
                host_edges.append([max(i, j) + 1, min(i, j) + 1])
                added.append((i, j))
                S = with_edges(A, added)
                maxdeg = int(S.getnnz(axis=1).max())
                ev = ev + 2.0 * V[i] * V[j]
            hs = (time.perf_counter() - t0) / a.host_steps
        out.update({"host_numpy_s_per_step": hs, "host_numpy_steps_timed": a.host_steps,
                    "host_numpy_threads": a.host_threads, "host_numpy_s_for_k_steps_EXTRAPOLATED": hs * a.k,
                    "host_edges_match_device": bool((np.array(host_edges) == first[:a.host_steps]).all())})
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

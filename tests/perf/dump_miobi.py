"""Every array the five MIOBI entry points return on a fixed case list, in one
.npz: a script, not a test, for comparing two trees bit for bit (run it in
each, then `--compare a.npz b.npz`).  Only the public Python API is used, so
the same file runs in a tree from before a change of the drivers.

Cases (the golden graphs of the GPU tests, t = 25, k = 24):
  * miobi_break on anaheim, austria, oregon_A0, anaheim_weighted and path100,
    refresh 8 and 0, modes reference and paper, with return_V;
  * miobi_make on anaheim, austria, oregon_A0 (binarised) and star140, refresh
    8 and 0;
  * miobi_break_node on anaheim, austria, oregon_A0 (binarised), refresh 50 and
    0, both shifts;
  * the three loops with k = 0 on anaheim (miobi_break with return_V);
  * pairs_score_topk and nodes_score_topk on the three graphs' own eigenpairs.
Per loop case: the selections, scores, degrees or m, the whole track,
nconv_min, refreshes, R0, R1, rob_score and the edited matrix's CSR arrays.
An error is part of the record (its text as bytes).  --compare views floats
as 64-bit integers: equal means the same bits."""
import argparse
import json
import os
import sys
import warnings

import torch  # noqa: F401  (torch's ROCm runtime first)
import numpy as np
import scipy.sparse as sp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T, K = 25, 24
GOLDEN = ["anaheim", "austria", "oregon_A0"]


def golden(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "graphs.npz"))
    n = int(z[f"{name}__n"][0])
    return sp.csr_matrix((z[f"{name}__data"], z[f"{name}__indices"], z[f"{name}__indptr"]), shape=(n, n))


def binarise(A):
    B = sp.csr_matrix(A, copy=True)
    B.data[:] = 1.0
    return B


def weighted_copy(A, seed=0):
    U = sp.triu(sp.csr_matrix(A), 1).tocoo()
    w = np.random.default_rng(seed).uniform(0.5, 1.5, U.nnz)
    W = sp.coo_matrix((w, (U.row, U.col)), shape=A.shape).tocsr()
    return sp.csr_matrix(W + W.T)


def star(n):
    A = sp.lil_matrix((n, n))
    A[0, 1:] = 1.0
    A[1:, 0] = 1.0
    return sp.csr_matrix(A)


def path(n):
    return sp.csr_matrix(sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1]))


def record(out, tag, call):
    """call() -> (selections, info); every array of it under tag/..."""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            picked, info = call()
    except Exception as e:  # noqa: BLE001  (the text is the record)
        out[f"{tag}/error"] = np.frombuffer(f"{type(e).__name__}: {e}".encode(), dtype=np.uint8)
        return
    out[f"{tag}/selected"] = np.asarray(picked)
    out[f"{tag}/nsel"] = np.array([len(picked)])
    for key, val in info.items():
        if key == "D":
            S = sp.csr_matrix(val.to_scipy())
            S.sort_indices()
            out[f"{tag}/A_indptr"], out[f"{tag}/A_indices"], out[f"{tag}/A_data"] = S.indptr, S.indices, S.data
        else:
            out[f"{tag}/{key}"] = np.asarray(val)


def dump(path_out):
    import krylov_robustness_amd as kra
    ctx = kra.Context(0)
    out = {}
    cases = 0
    graphs = {g: golden(g) for g in GOLDEN}
    brk = dict(graphs, anaheim_weighted=weighted_copy(graphs["anaheim"]), path100=path(100))
    for name, A in brk.items():
        for refresh in (8, 0):
            for mode in ("reference", "paper"):
                record(out, f"break/{name}/r{refresh}/{mode}", lambda: kra.miobi_break(
                    kra.DeviceMatrix(A, ctx), K, t=T, refresh=refresh, mode=mode, seed=3, return_V=True, ctx=ctx))
                cases += 1
    # no step at all: the track's first row and, for the removal, the vectors as staged
    A = graphs["anaheim"]
    record(out, "break/anaheim/k0", lambda: kra.miobi_break(
        kra.DeviceMatrix(A, ctx), 0, t=T, refresh=8, seed=3, return_V=True, ctx=ctx))
    record(out, "make/anaheim/k0", lambda: kra.miobi_make(
        kra.DeviceMatrix(binarise(A), ctx), 0, t=T, refresh=8, seed=3, ctx=ctx))
    record(out, "node/anaheim/k0", lambda: kra.miobi_break_node(
        kra.DeviceMatrix(binarise(A), ctx), 0, t=T, refresh=50, seed=7, ctx=ctx))
    cases += 3
    mke = {g: binarise(A) for g, A in graphs.items()}
    mke["star140"] = star(140)
    for name, A in mke.items():
        for refresh in (8, 0):
            record(out, f"make/{name}/r{refresh}", lambda: kra.miobi_make(
                kra.DeviceMatrix(A, ctx), K, t=T, refresh=refresh, seed=3, ctx=ctx))
            cases += 1
    for name in GOLDEN:
        A = binarise(graphs[name])
        for refresh in (50, 0):
            for shift in ("reference", "first_order"):
                record(out, f"node/{name}/r{refresh}/{shift}", lambda: kra.miobi_break_node(
                    kra.DeviceMatrix(A, ctx), K, t=T, refresh=refresh, shift=shift, seed=7, ctx=ctx))
                cases += 1
        D = kra.DeviceMatrix(A, ctx)
        lam, V = kra.eigs_topk(D, T, seed=3, ctx=ctx)
        i, j = sp.triu(A, 1).nonzero()
        for sign in (-2.0, 2.0):
            out[f"pairs_score/{name}/{sign}"] = kra.pairs_score_topk(lam, V, np.stack([i, j], axis=1), sign=sign, ctx=ctx)
            cases += 1
        out[f"nodes_score/{name}"] = kra.nodes_score_topk(D, lam, V, ctx=ctx)
        cases += 1
    os.makedirs(os.path.dirname(os.path.abspath(path_out)), exist_ok=True)
    np.savez(path_out, **out)
    print(json.dumps({"cases": cases, "arrays": len(out), "errors": sorted(k for k in out if k.endswith("/error")),
                      "out": path_out}))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    differ = sorted(set(a.files) ^ set(b.files))
    for key in sorted(set(a.files) & set(b.files)):
        if a[key].dtype != b[key].dtype or a[key].shape != b[key].shape or not np.array_equal(bits(a[key]), bits(b[key])):
            differ.append(key)
    print(json.dumps({"arrays": len(a.files), "arrays_other": len(b.files), "differing": differ,
                      "errors": sorted(k for k in a.files if k.endswith("/error")), "equal": not differ}))
    return 0 if not differ else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    dump(a.out or os.path.join(ROOT, "dump", "miobi.npz"))

"""GPU tests of kt_eigs_topk (thick-restart block Lanczos) and
of deflate=k in the deflated estimators.  Every bound comes from the dense
numpy.linalg.eigh of the small graph, computed here: eigenvalues to 1e-9
|lambda_1|, orthonormality to 1e-12, the returned residuals against the host's
||A v - lambda v|| (scipy CSR) to 1e-6 resid + 1e-13 |lambda_1|, and each
vector against the exact one by Davis-Kahan from its own residual and the
exact gap."""
import functools
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, load_graph

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "tests", "native", "eig_check", "eig_check")
PARITY_GRAPHS = ["rome", "india", "austria", "oregon_A0", "anaheim"]
GAP_REL = 1e-6  # pairs whose exact gap is below this times |lambda_1| are compared as clusters


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


@functools.lru_cache(maxsize=None)
def _eig(name):
    w, V = np.linalg.eigh(load_graph(name).toarray())
    return w[::-1].copy(), V[:, ::-1].copy()  # descending


_DEV = {}


def _dev(kra, ctx, name):
    if name not in _DEV:
        _DEV[name] = kra.DeviceMatrix(load_graph(name), ctx)
    return _DEV[name]


def _host_resid(A, lam, V):
    return np.linalg.norm(A @ V - V * lam, axis=0)


def _check_resid(A, lam, V, resid, l1):
    host = _host_resid(sp.csr_matrix(A), lam, V)
    err = np.abs(resid - host)
    print("resid: device max", resid.max(), "worst |device - host|", err.max())
    assert (err <= 1e-6 * host + 1e-13 * abs(l1)).all(), (resid, host)


def _sums_nonnegative(V):
    """Column sums >= 0 up to the rounding of the sum itself (n eps ||v||_1):
    an eigenvector whose exact sum is zero may land on either side."""
    return (V.sum(axis=0) >= -V.shape[0] * 2.3e-16 * np.abs(V).sum(axis=0)).all()


def _orth_err(V):
    return np.abs(V.T @ V - np.eye(V.shape[1])).max()


def _clusters(w, k, thr):
    """Runs of consecutive exact eigenvalues closer than thr, as (lo, hi) index
    ranges (hi exclusive), for the runs that touch the first k."""
    out, lo = [], 0
    for i in range(1, len(w) + 1):
        if i == len(w) or w[i - 1] - w[i] > thr:
            if lo < k:
                out.append((lo, i))
            lo = i
            if lo >= k:
                break
    return out


@pytest.mark.parametrize("k", [1, 5, 16, 32])
@pytest.mark.parametrize("name", PARITY_GRAPHS)
def test_parity_with_dense_eigh(kra, gpu_ctx, name, k):
    A = load_graph(name)
    w, U = _eig(name)
    l1 = abs(w[0])
    D = _dev(kra, gpu_ctx, name)
    lam, V, (resid, nconv, spmm) = kra.eigs_topk(D, k, ctx=gpu_ctx, return_info=True)
    print(name, "k", k, "spmm", spmm, "nconv", nconv, "max |lam - exact| / l1", np.abs(lam - w[:k]).max() / l1,
          "orth", _orth_err(V))
    assert lam.shape == (k,) and V.shape == (A.shape[0], k) and resid.shape == (k,)
    assert (np.diff(lam) <= 0).all()
    assert np.abs(lam - w[:k]).max() <= 1e-9 * l1
    assert _orth_err(V) <= 1e-12
    _check_resid(A, lam, V, resid, l1)
    assert nconv == k and spmm > 0
    assert _sums_nonnegative(V)
    # Davis-Kahan per pair (cluster by cluster where the exact gap is tiny)
    thr = GAP_REL * l1
    singles = clustered = 0
    for lo, hi in _clusters(w, k, thr):
        if hi > k:  # the cluster leaves the computed set: nothing to compare it with
            clustered += k - lo
            continue
        gap = min(w[lo - 1] - w[lo] if lo else np.inf, w[hi - 1] - w[hi] if hi < len(w) else np.inf)
        Us, Vs = U[:, lo:hi], V[:, lo:hi]
        dist = np.linalg.norm(Vs - Us @ (Us.T @ Vs), axis=0)
        bound = 4 * resid[lo:hi].max() / gap + 1e-12
        assert (dist <= bound).all(), (name, k, lo, hi, dist, bound)
        if hi - lo == 1:
            singles += 1
        else:
            clustered += hi - lo
    assert singles + clustered == k
    assert clustered <= k / 4, (name, k, clustered)  # the exact spectra keep within this cap at GAP_REL
    if k == 1:
        lead = kra.eigs_leading(D, ctx=gpu_ctx)[0]
        assert abs(lam[0] - lead) <= 1e-12 * abs(lead)


@pytest.mark.parametrize("name", ["oregon_A0", "rome"])
def test_multiple_eigenvalues_are_all_found(kra, gpu_ctx, name):
    """Four copies on the block diagonal, rows symmetrically permuted: every
    eigenvalue is fourfold, the case a single-vector Krylov solver gets wrong.
    oregon_A0 (n = 2,532) is the case proper; rome (n = 13,412) is the same
    property above 8,192 rows, where the Gram and combine passes take the
    tall-skinny kernels instead of rocBLAS."""
    A1 = load_graph(name)
    w, _ = _eig(name)
    n4 = 4 * A1.shape[0]
    perm = np.random.default_rng(0).permutation(n4)
    A = sp.block_diag([A1] * 4, format="csr")[perm][:, perm].tocsr()
    lam, V, (resid, nconv, spmm) = kra.eigs_topk(kra.DeviceMatrix(A, gpu_ctx), 8, ctx=gpu_ctx, return_info=True)
    print(name, "x4: lam", lam, "spmm", spmm, "orth", _orth_err(V))
    assert np.abs(lam[:4] - w[0]).max() <= 1e-9 * w[0]
    assert np.abs(lam[4:] - w[1]).max() <= 1e-9 * w[0]
    assert _orth_err(V) <= 1e-12
    assert nconv == 8
    _check_resid(A, lam, V, resid, w[0])


def test_rank_loss_complete_bipartite(kra, gpu_ctx):
    """K_{100,100}: rank 2, so A V loses rank at the first product and the
    block is refilled from the counter RNG."""
    J = np.ones((100, 100))
    A = sp.csr_matrix(np.block([[np.zeros((100, 100)), J], [J, np.zeros((100, 100))]]))
    lam, V, (resid, nconv, spmm) = kra.eigs_topk(kra.DeviceMatrix(A, gpu_ctx), 4, ctx=gpu_ctx, return_info=True)
    print("lam", lam, "resid", resid, "nconv", nconv, "spmm", spmm)
    assert np.abs(lam - np.array([100.0, 0, 0, 0])).max() <= 1e-9 * 100
    assert np.isfinite(V).all() and _orth_err(V) <= 1e-12
    assert (resid <= 1e-8).all()
    _check_resid(A, lam, V, resid, 100.0)


def _path(n):
    return sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], format="csr")


@pytest.mark.parametrize("n", [20, 130, 131])
def test_dense_path_and_its_boundary(kra, gpu_ctx, n):
    A = _path(n)
    D = kra.DeviceMatrix(A, gpu_ctx)
    exact = 2 * np.cos(np.pi * np.arange(1, n + 1) / (n + 1))
    lam, V, (resid, nconv, spmm) = kra.eigs_topk(D, 4, ctx=gpu_ctx, return_info=True)
    assert np.abs(lam - exact[:4]).max() <= 1e-9 * exact[0]
    assert _orth_err(V) <= 1e-12 and nconv == 4 and _sums_nonnegative(V)
    _check_resid(A, lam, V, resid, exact[0])
    assert (spmm == 0) if n <= 130 else (spmm > 0)
    if n == 20:
        lam, V = kra.eigs_topk(D, 20, ctx=gpu_ctx)
        assert np.abs(lam - exact).max() <= 1e-9 * exact[0] and _orth_err(V) <= 1e-12
        for bad in (21, 0, 33):
            with pytest.raises(kra.KrylovError) as e:
                kra.eigs_topk(D, bad, ctx=gpu_ctx)
            assert "k must be in" in str(e.value)


def test_reaching_the_cap_is_reported_not_hidden(kra, gpu_ctx):
    A = load_graph("rome")
    w, _ = _eig("rome")
    lam, V, (resid, nconv, spmm) = kra.eigs_topk(_dev(kra, gpu_ctx, "rome"), 16, max_spmm=8, ctx=gpu_ctx,
                                                 return_info=True)
    print("nconv", nconv, "spmm", spmm, "resid", resid)
    assert nconv < 16 and 0 < spmm <= 8
    _check_resid(A, lam, V, resid, w[0])
    assert _orth_err(V) <= 1e-12


_CHILD = """
import sys
sys.path.insert(0, %r)
import conftest  # torch first, then the repository on the path
import numpy as np
import krylov_robustness_amd as kra
ctx = kra.Context(0)
lam, V, (resid, nconv, spmm) = kra.eigs_topk(kra.DeviceMatrix(conftest.load_graph("anaheim"), ctx), 5, ctx=ctx,
                                             return_info=True)
np.savez(sys.argv[1], lam=lam, V=V, resid=resid)
"""


def test_determinism_and_seed(kra, gpu_ctx, tmp_path):
    w, _ = _eig("anaheim")
    D = _dev(kra, gpu_ctx, "anaheim")
    a = kra.eigs_topk(D, 5, ctx=gpu_ctx, return_info=True)
    b = kra.eigs_topk(D, 5, ctx=gpu_ctx, return_info=True)
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[2][0], b[2][0])):
        assert x.tobytes() == y.tobytes()
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD % os.path.join(ROOT, "tests"), out], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, KT_SLQ_LANES="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    assert z["lam"].tobytes() == a[0].tobytes() and z["V"].tobytes() == np.asarray(a[1]).tobytes()
    assert z["resid"].tobytes() == a[2][0].tobytes()
    lam1 = kra.eigs_topk(D, 5, seed=1, ctx=gpu_ctx)[0]
    assert np.abs(lam1 - a[0]).max() <= 1e-9 * abs(w[0])
    assert np.abs(lam1 - w[:5]).max() <= 1e-9 * abs(w[0])


def _tril(A):
    L = sp.tril(sp.csc_matrix(A), -1).tocsc()
    L.sort_indices()
    J = np.repeat(np.arange(L.shape[1], dtype=np.int64), np.diff(L.indptr))
    return np.stack([L.indices.astype(np.int64), J], axis=1)


def _sigmas(E, Q, P, N):
    """The exact standard deviations of the deflated estimators with R = Pi E
    Pi, Pi = I - Q Q' (DESIGN.md §4.2b, §4.2c): node i, (sum_j R_ij^2 - R_ii^2)
    / N; edge (i, j), ((R_ii + R_jj)^2 + sum_{k != i, j} (R_ik^2 + R_jk^2)) / 4 / N."""
    EQ = E @ Q
    R = E - Q @ EQ.T - EQ @ Q.T + Q @ (Q.T @ EQ) @ Q.T
    rows = (R * R).sum(axis=1)
    dg = np.diag(R)
    I, J = P[:, 0], P[:, 1]
    cross = rows[I] - dg[I] ** 2 - R[I, J] ** 2 + rows[J] - dg[J] ** 2 - R[J, I] ** 2
    return np.sqrt((rows - dg ** 2) / N), np.sqrt(0.25 * ((dg[I] + dg[J]) ** 2 + cross) / N)


@pytest.mark.parametrize("name", ["oregon_A0", "rome"])
def test_deflation_end_to_end(kra, gpu_ctx, name):
    """deflate=16 is deflate=Q with the device's own Q, bit for bit; every
    estimate lies within 6 sigma of dense exp(A) with sigma the exact standard
    deviation for that Q; the reported stderr is within [0.7, 1.4] sigma at the
    median (test_statistics' bands); and the stderr falls from deflate=1 to
    deflate=16 by the factor exact arithmetic gives, within the same band."""
    N, m, seed = 256, 30, 7
    A = load_graph(name)
    w, U = _eig(name)
    E = (U * np.exp(w)) @ U.T
    D = _dev(kra, gpu_ctx, name)
    P = _tril(A)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # nconv == 16: no warning
        d16 = kra.diag_fun(D, N, m=m, seed=seed, deflate=16, ctx=gpu_ctx)
        e16 = kra.entries_fun(D, P, N, m=m, seed=seed, deflate=16, ctx=gpu_ctx)
    Q = kra.eigs_topk(D, 16, ctx=gpu_ctx)[1]
    dQ = kra.diag_fun(D, N, m=m, seed=seed, deflate=Q, ctx=gpu_ctx)
    eQ = kra.entries_fun(D, P, N, m=m, seed=seed, deflate=Q, ctx=gpu_ctx)
    for f in ("d0", "dsum", "dsum2"):
        assert getattr(d16, f).tobytes() == getattr(dQ, f).tobytes(), f
    for f in ("e0", "esum", "esum2"):
        assert getattr(e16, f).tobytes() == getattr(eQ, f).tobytes(), f
    s_node, s_edge = _sigmas(E, Q, P, N)
    zn = np.abs(d16.mean - np.diag(E)) / s_node
    ze = np.abs(e16.mean - E[P[:, 0], P[:, 1]]) / s_edge
    rn, re = np.median(d16.stderr / s_node), np.median(e16.stderr / s_edge)
    print(name, "worst |err| / sigma: nodes", zn.max(), "edges", ze.max(), "median stderr / sigma", rn, re)
    assert (zn <= 6.0).all() and (ze <= 6.0).all(), (zn.max(), ze.max())
    assert 0.7 <= rn <= 1.4 and 0.7 <= re <= 1.4, (rn, re)
    # deflate=16 against deflate=1: the ratio of median stderr, against the same ratio of exact sigmas
    u = kra.eigs_leading(D, ctx=gpu_ctx)[1]
    s1_node, s1_edge = _sigmas(E, u[:, None], P, N)
    d1 = kra.diag_fun(D, N, m=m, seed=seed, deflate=1, ctx=gpu_ctx)
    e1 = kra.entries_fun(D, P, N, m=m, seed=seed, deflate=1, ctx=gpu_ctx)
    for got, want, what in ((np.median(d16.stderr) / np.median(d1.stderr), np.median(s_node) / np.median(s1_node), "nodes"),
                            (np.median(e16.stderr) / np.median(e1.stderr), np.median(s_edge) / np.median(s1_edge), "edges")):
        print(name, what, "median stderr 16 / 1:", got, "exact sigma ratio:", want)
        assert 0.7 * want <= got <= 1.4 * want, (what, got, want)


def test_deflate_k_through_the_callers(kra, gpu_ctx):
    from krylov_robustness_amd.greedy import _stable_head
    A = load_graph("rome")
    n = A.shape[0]
    D = _dev(kra, gpu_ctx, "rome")
    c = kra.compute_centrality(D, "exp", deflate=8, ctx=gpu_ctx)
    assert c.shape == (n,) and np.isfinite(c).all()
    top = kra.find_top_edges_fun(D, 50, deflate=8, ctx=gpu_ctx)
    assert top.shape == (50, 2) and (top[:, 0] > top[:, 1]).all() and top.min() >= 1
    w, U = _eig("rome")
    E = (U * np.exp(w)) @ U.T
    P = _tril(A)
    as_set = lambda T: {(int(a), int(b)) for a, b in T}  # noqa: E731
    exact = as_set(P[_stable_head(-E[P[:, 0], P[:, 1]], 250)])
    ov = {}
    for k in (0, 8):
        t = kra.find_top_edges_fun(D, 250, nprobes=256, deflate=k, seed=7, ctx=gpu_ctx)
        ov[k] = len(as_set(t - 1) & exact)
    print("overlap with the exact top 250: deflate=0", ov[0], "deflate=8", ov[8])
    assert ov[8] >= ov[0]


@pytest.fixture(scope="module")
def kernel_run():
    assert os.path.exists(CHECK), "tests/native/eig_check/eig_check is not built (__graft_entry__.build())"
    h = subprocess.run([CHECK, "--host"], capture_output=True, text=True, timeout=120)
    assert h.returncode == 0, (h.returncode, h.stdout, h.stderr)
    counts = {g: v["cases"] for g, v in json.loads(h.stdout.strip().splitlines()[-1])["groups"].items()}
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    try:
        out = json.loads(r.stdout.strip().splitlines()[-1])
    except (IndexError, ValueError):
        out = None
    return r, out, counts


@pytest.mark.parametrize("group", ["rotate", "resid", "start"])
def test_kernels_match_exact_references(kernel_run, group):
    r, out, counts = kernel_run
    assert out is not None, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "hip_error" not in out and r.returncode in (0, 1), (r.returncode, out.get("hip_error"), r.stderr[-2000:])
    assert out["mode"] == "device"
    g = out["groups"][group]
    assert g["failed"] == [] and g["failed_count"] == 0, g["failed"]
    assert g["cases"] == counts[group] and g["cases"] > 0, (g["cases"], counts[group])

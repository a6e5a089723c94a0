"""Greedy edge selection over the device path: krylov_miobi.m / greedy_krylov.m.

``krylov_miobi`` scores every candidate edge of a greedy step with the batched
device evaluation (kt_trace_fun_update_pairs: one block-2 Lanczos run per
candidate, all candidates advanced by one SpMM per step) and edits A on the
device (kt_matrix_set_pairs).  ``greedy_krylov`` is the reference's outer loop
(greedy_krylov.m:64-93) with the search-space heuristics find_top_edges.m /
find_top_missing_edges.m restated on the host: they are ordering/combinatorics
on node centralities, not bandwidth work.

Indices follow the reference: edges are 1-based (i, j) rows with
E(:, 1) >= E(:, 2) for krylov_miobi's candidate lists.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional

import numpy as np

from . import _lib
from .core import Context, DeviceMatrix, _dev, _dptr, _fun_code, normest


def _i64(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int64))
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


def trace_fun_update_pairs(A, E, B, tol=1e-12, it=None, fun="exp", b_self=None,
                           ctx: Optional[Context] = None):
    """Xm[h] = trace_fun_update(A, U_h, B, tol, it, 0, fun) for every candidate
    edge h of E (q x 2, 1-based), U_h = [e_E(h,1), e_E(h,2)] as built in
    krylov_miobi.m:76-98 (a self-loop candidate uses U = e_i and B = b_self).
    Returns (Xm, iter, lucky) arrays."""
    D = _dev(A, ctx)
    E = np.asarray(E, dtype=np.int64).reshape(-1, 2)
    q = E.shape[0]
    ei, pi = _i64(E[:, 0] - 1)
    ej, pj = _i64(E[:, 1] - 1)
    Bm = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(2, 2))
    if b_self is None:
        b_self = float(Bm[0, 1])
    xm = np.zeros(q)
    itr = np.zeros(q, dtype=np.int32)
    lk = np.zeros(q, dtype=np.int32)
    _lib.check(_lib.load().kt_trace_fun_update_pairs(
        D.handle, q, pi, pj, _dptr(Bm), float(b_self), float(tol), int(it or 0), _fun_code(fun),
        _dptr(xm), itr.ctypes.data_as(C.POINTER(C.c_int)), lk.ctypes.data_as(C.POINTER(C.c_int))))
    return xm, itr, lk


def krylov_miobi(A, k, E=None, tol=1e-12, it=None, poles=np.inf, debug=0, miobi="break",
                 rescale=1.0, ctx: Optional[Context] = None):
    """[edges, rob, A_new] = krylov_miobi(A, k, E, tol, it, poles, debug, miobi, rescale)
    (krylov_miobi.m:1).  A may be a DeviceMatrix (edited in place and returned)
    or a matrix (uploaded; the returned DeviceMatrix holds A_new)."""
    if miobi not in ("break", "make"):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, "KRYLOV_MIOBI:: not supported option for miobi")
    D = _dev(A, ctx)
    if E is None or len(E) == 0:  # :42-46  all edges with E(:,1) >= E(:,2)
        S = D.to_scipy().tocoo()
        keep = S.row >= S.col
        E = np.stack([S.row[keep], S.col[keep]], axis=1) + 1
        E = E[np.lexsort((E[:, 0], E[:, 1]))]  # MATLAB find(): column-major order
    E = np.asarray(E, dtype=np.int64).reshape(-1, 2)
    nE = E.shape[0]
    ei, pi = _i64(E[:, 0] - 1)
    ej, pj = _i64(E[:, 1] - 1)
    cap = max(min(int(k), nE), 1)
    si = np.zeros(cap, dtype=np.int64)
    sj = np.zeros(cap, dtype=np.int64)
    rob = C.c_double()
    ns = C.c_int64()
    _lib.check(_lib.load().kt_krylov_miobi(
        D.handle, int(k), nE, pi, pj, float(tol), int(it or 0), 1 if miobi == "make" else 0,
        float(rescale), si.ctypes.data_as(C.POINTER(C.c_int64)),
        sj.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(rob), C.byref(ns)))
    m = int(ns.value)
    edges = np.stack([si[:m] + 1, sj[:m] + 1], axis=1)
    return edges, float(rob.value), D


def select_extreme(xm, make):
    """krylov_miobi.m:112-124: strict comparison, the first extreme wins.
    Returns (index, value); index -1 if no candidate compares (all NaN)."""
    best, bv = -1, (-np.inf if make else np.inf)
    for h, v in enumerate(np.asarray(xm, dtype=np.float64)):
        if (v > bv) if make else (v < bv):
            best, bv = h, float(v)
    return best, bv


def miobi_loop(k, E, make, score, edit):
    """Host loop of krylov_miobi.m:70-139 over injectable scoring / editing:
    score(E) -> the trace variation of every candidate row of E (1-based),
    edit(edge, value) applies A(i,j) = A(j,i) = value.  Returns (edges, rob)."""
    E = np.asarray(E, dtype=np.int64).reshape(-1, 2).copy()
    edges, rob = [], 0.0
    for _ in range(min(int(k), E.shape[0])):
        xm = score(E)
        best, bv = select_extreme(xm, make)
        if best < 0:
            raise _lib.KrylovError(_lib.KT_ERR_ARG, "KRYLOV_MIOBI:: no finite candidate score")
        chosen = E[best].copy()
        E = np.delete(E, best, axis=0)               # :127
        edit(chosen, 1.0 if make else 0.0)           # :129-135
        edges.append(chosen)
        rob += bv
    return np.array(edges, dtype=np.int64).reshape(-1, 2), rob


def krylov_miobi_sharded(A, k, E, tol=1e-12, it=None, poles=np.inf, debug=0, miobi="break",
                         rescale=1.0, group=None, ctx: Optional[Context] = None):
    """krylov_miobi with the candidate scoring sharded over the ranks of the
    process group: rank r scores its contiguous slice of E on
    its own GPU (kt_trace_fun_update_pairs), the scores are all-gathered in
    rank order, every rank picks the same extreme candidate and edits its own
    device copy of A.  Same result as krylov_miobi on one GPU."""
    import torch.distributed as dist
    from .dist import allgather_concat, probe_shard
    if miobi not in ("break", "make"):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, "KRYLOV_MIOBI:: not supported option for miobi")
    D = _dev(A, ctx)
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    make = miobi == "make"
    sg = 1.0 if make else -1.0
    B = sg * np.array([[0.0, 1.0], [1.0, 0.0]]) / rescale

    def score(Ecur):
        counts = [probe_shard(len(Ecur), r, world)[1] for r in range(world)]
        off, cnt = probe_shard(len(Ecur), rank, world)
        xm = (trace_fun_update_pairs(D, Ecur[off:off + cnt], B, tol, it, b_self=sg, ctx=ctx)[0]
              if cnt else np.zeros(0))
        return allgather_concat(xm, counts, group)

    def edit(e, value):
        D.set_pairs([e], value)

    edges, rob = miobi_loop(k, E, make, score, edit)
    return edges, rob, D


def _stable_head(key, num):
    """argsort(key, kind="stable")[:num] without sorting the whole key: every
    entry at or below the num-th smallest value, in index order, then a
    stable sort of those (same ties, same order)."""
    if num >= len(key):
        return np.argsort(key, kind="stable")
    th = np.partition(key, num - 1)[num - 1]
    if np.isnan(th):  # NaN keys sort last in argsort: take the full sort
        return np.argsort(key, kind="stable")[:num]
    cand = np.flatnonzero(key <= th)
    return cand[np.argsort(key[cand], kind="stable")][:num]


def _tril_edges(A):
    """[I, J] = find(tril(A, -1)), 0-based, in column-major order, read
    straight off the CSC arrays."""
    import scipy.sparse as sp
    L = A if sp.isspmatrix_csc(A) else sp.csc_matrix(A)
    if not L.has_canonical_format:  # duplicates summed (tril(A) sees sums), sorted
        L = L.copy()
        L.sum_duplicates()
    J = np.repeat(np.arange(L.shape[1], dtype=np.int64), np.diff(L.indptr))
    keep = (L.indices > J) & (L.data != 0)
    return L.indices[keep].astype(np.int64), J[keep]


def find_top_edges(A, centrality, num, order="mult"):
    """find_top_edges.m:1-40: the top `num` existing edges (1-based, i > j)."""
    I, J = _tril_edges(A)
    c = np.asarray(centrality, dtype=np.float64).ravel()
    if order == "mult":  # :22-25
        key = -(c[I] * c[J])
    elif order == "min":  # :26-37
        # find(sc == v, 1) with sc = sort(c, 'descend'): the first descending
        # position of v is n - (last ascending position of v), i.e.
        # n - searchsorted(ascending, v, 'right') + 1 (1-based), once per node
        nc = len(c)
        rank = (nc - np.searchsorted(np.sort(c), c, side="right") + 1).astype(np.float64)
        c1, c2 = rank[I], rank[J]
        mn, mx = np.minimum(c1, c2), np.maximum(c1, c2)
        key = mx * (mx - 1) / 2 + mn
    else:
        return np.stack([I + 1, J + 1], axis=1)
    # :19-21 warns when fewer than num edges exist; E(ind(1:num), :) then
    # indexes floor(num) of them and fails only if those are missing too
    if len(I) < num:
        warnings.warn("FIND_TOP_EDGES:: there are not enough edges in the graph")
    num = int(np.floor(num))
    if len(I) < num:
        raise IndexError("FIND_TOP_EDGES:: there are not enough edges in the graph")
    ind = _stable_head(key, num)
    return np.stack([I[ind] + 1, J[ind] + 1], axis=1)


def find_top_edges_fun(A, num, fun="exp", nprobes=256, deflate=1, m=30, seed=0, ctx: Optional[Context] = None):
    """The top `num` existing edges ranked by descending estimated f(A)[i, j]
    (entries_fun on every edge: one sweep set however many edges), returned as
    find_top_edges returns them: 1-based, i > j, enumerated in find(tril(A,
    -1)) order with ties kept in that order, and the same warning / error when
    fewer than `num` edges exist.  To first order, editing edge (i, j) changes
    tr f(A) by -/+ 2 f'(A)[i, j]: for f = exp the ranking is by that
    derivative; for a general f pass its derivative's code as `fun` (sinh to
    rank for cosh and the reverse).  Missing edges are O(n^2): score a
    candidate list of them with entries_fun."""
    from .core import _deflate_arg, entries_fun
    deflate = _deflate_arg("find_top_edges_fun", deflate, A)
    D = _dev(A, ctx)
    I, J = _tril_edges(D.to_scipy())
    if len(I) < num:
        warnings.warn("FIND_TOP_EDGES:: there are not enough edges in the graph")
    num = int(np.floor(num))
    if len(I) < num:
        raise IndexError("FIND_TOP_EDGES:: there are not enough edges in the graph")
    if len(I) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    est = entries_fun(D, np.stack([I, J], axis=1), nprobes, m=m, seed=seed, fun=fun, deflate=deflate, ctx=ctx)
    ind = _stable_head(-np.asarray(est.mean, dtype=np.float64), num)
    return np.stack([I[ind] + 1, J[ind] + 1], axis=1)


def find_top_missing_edges(A, centrality, num, order="min"):
    """find_top_missing_edges.m:1-67: the top `num` missing edges (1-based)."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    n = A.shape[0]
    c = np.asarray(centrality, dtype=np.float64).ravel()
    indC = np.argsort(-c, kind="stable")  # [sc, indC] = sort(centrality, 'descend')
    sc = c[indC]
    if order == "min":  # :52-64
        E = []
        j = 1
        while len(E) < num:
            if j >= n:
                raise IndexError("FIND_TOP_MISSING_EDGES:: not enough missing edges")
            col = A[indC[:j], :][:, [indC[j]]].toarray().ravel()
            for t in np.flatnonzero(col == 0):
                E.append((indC[t] + 1, indC[j] + 1))
            j += 1
        return np.array(E[:int(np.floor(num))], dtype=np.int64)  # E(1:num, :) with a fractional num
    if order == "mult":  # :22-51
        if (n * n - A.nnz - n) / 2 <= num:
            raise RuntimeError("FIND_TOP_MISSING_EDGES:: output E is not assigned on this branch "
                               "(find_top_missing_edges.m:23-30 returns before setting E)")
        min_N, ln = 2, 0
        while ln < num:
            ln += int(np.sum(A[indC[:min_N - 1], :][:, [indC[min_N - 1]]].toarray() == 0))
            min_N += 1
        min_N -= 1
        N = int(np.sum(sc[0] * sc > sc[min_N - 1] ** 2))
        S = np.triu(np.outer(c[indC[:N]], c[indC[:N]]))
        lin = np.argsort(-S.ravel(order="F"), kind="stable")
        I, J = lin % N, lin // N
        I, J = indC[I], indC[J]
        E = []
        for a, b in zip(I, J):
            if len(E) >= num:
                break
            if a != b and A[a, b] == 0:
                E.append((a + 1, b + 1))
        return np.array(E, dtype=np.int64).reshape(-1, 2)
    raise ValueError(f"unknown order {order!r}")


def edge2low_rank(E, n, value=-1.0):
    """[U, B] = edge2low_rank(E, n): the low-rank factors of an edge edit,
    A + U B U' (functions/edge2low_rank.m:1-13, value = -1: remove the edges;
    the make drivers' local copy, Tests/test_unweighted_make.m:171-183, uses
    +1: add them).  E: m x 2 1-based node pairs.  U: n x k sparse selector of
    the k distinct nodes (ascending, as unique()), B: k x k dense with
    B(a, b) = B(b, a) = value for every edge."""
    import scipy.sparse as sp
    E = np.asarray(E, dtype=np.int64).reshape(-1, 2)
    t1, t2 = E[:, 0], E[:, 1]
    ut = np.unique(np.concatenate([t1, t2]))
    if ut.size and (ut[0] < 1 or ut[-1] > n):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, "edge2low_rank: node index out of range")
    k = ut.size
    U = sp.csc_matrix((np.ones(k), (ut - 1, np.arange(k))), shape=(int(n), k))
    B = np.zeros((k, k))
    a = np.searchsorted(ut, t1)
    b = np.searchsorted(ut, t2)
    B[a, b] = value
    B[b, a] = value
    return U, B


def compute_centrality(A, kind="eig", ctx: Optional[Context] = None, **kw):
    """compute_centrality.m: 'eig' = abs(leading eigenvector) (:15-17), on the
    device when A is a DeviceMatrix (kt_eigs_leading), else scipy eigsh;
    'deg' = column sums (:18-19); 'exp' = diag(expm(A)), the subgraph
    centrality (:9-10): the dense expm for a host matrix, as the reference,
    and for a DeviceMatrix the deflated stochastic estimate diag_fun(A,
    nprobes=256, deflate=1).mean (kw: nprobes, deflate, m, seed, block;
    deflate = k in [2, 16] deflates the leading k eigenvectors of eigs_topk)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    if isinstance(A, DeviceMatrix):
        if kind == "deg":
            return np.asarray(A.to_scipy().sum(axis=0)).ravel()
        if kind == "exp":
            from .core import _deflate_arg, diag_fun
            _deflate_arg("compute_centrality", kw.get("deflate", 1))
            return diag_fun(A, kw.get("nprobes", 256), m=kw.get("m", 30), seed=kw.get("seed", 0),
                            block=kw.get("block", 0), deflate=kw.get("deflate", 1), ctx=ctx).mean
        from .core import eigs_leading
        return np.abs(eigs_leading(A, ctx=ctx)[1])
    A = sp.csr_matrix(A, dtype=np.float64)
    if kind == "deg":
        return np.asarray(A.sum(axis=0)).ravel()
    if kind == "exp":
        import scipy.linalg as sl
        return np.diag(sl.expm(A.toarray())).copy()
    _, u = sla.eigsh(A, k=1, which="LM")  # eigs(A, 1): largest magnitude
    return np.abs(u[:, 0])


def _is_symmetric(S):
    """issymmetric(A) for the sorted CSC the device exports: CSR of A equals
    its CSC exactly when A == A' entry for entry (the fast path); anything
    else falls back to the elementwise comparison."""
    R = S.tocsr()
    if (R.has_sorted_indices and np.array_equal(R.indptr, S.indptr)
            and np.array_equal(R.indices, S.indices) and np.array_equal(R.data, S.data)):
        return True
    return not (S != S.T).nnz


def greedy_krylov(A, k, Q=0, centrality=None, order="mult", tol=1e-12, it=None, poles=np.inf,
                  debug=0, miobi="break", rescale=1.0, ctx: Optional[Context] = None, top=None):
    """[edges, rob_variation, A_new] = greedy_krylov(A, k, Q, centrality, order, tol, it,
    poles, debug, miobi, rescale)  (greedy_krylov.m:1-100).  Returns A_new as
    the DeviceMatrix the edits were applied to (``.to_scipy()`` for the host copy).
    top: a ranked list of 1-based pairs (e.g. find_top_edges_fun's) used in
    place of the find_top_* call; centrality and order are then not read."""
    D = _dev(A, ctx)
    S = D.to_scipy()
    if not _is_symmetric(S):  # :27-29
        raise _lib.KrylovError(_lib.KT_ERR_NOT_HERMITIAN, "GREEDY_KRYLOV:: Adjacency matrix should be symmetric")
    if not Q:
        # :42-44 Q = max(sum(A, 1)); top_edges(1:Q, :) indexes floor(Q) rows, so
        # a weighted graph whose largest weighted degree is below 1 gives Q = 0,
        # an empty E, and krylov_miobi then scores every edge (krylov_miobi.m:43-46)
        Q = float(np.asarray(S.sum(axis=0)).max())
    # the ranking is asked for Q + k edges unfloored (find_top_edges.m:19 warns
    # against that count); every index use is 1:Q, i.e. floor(Q) rows
    Qn = Q + k
    Q = int(np.floor(Q))
    if miobi == "break" and S.nnz < 2 * k:  # :54-56
        raise _lib.KrylovError(_lib.KT_ERR_ARG, "GREEDY_KRYLOV:: edges to be removed are more than edges in the network")
    if top is not None:
        top = np.asarray(top, dtype=np.int64).reshape(-1, 2)
    else:
        if centrality is None:
            centrality = compute_centrality(D, "eig", ctx=ctx)
        top = (find_top_missing_edges(S, centrality, Qn, order) if miobi == "make"
               else find_top_edges(S, centrality, Qn, order))  # :82 (first step)
    if len(top) >= int(k) > 0 and int(Q) >= 1:
        # the step loop in the library (kt_greedy_krylov_steps): krylov_miobi(A, 1,
        # top(1:Q)) per step, the selected pair dropped from the ranking (:84-89)
        T = np.asarray(top, dtype=np.int64).reshape(-1, 2)
        ti, pi = _i64(T[:, 0] - 1)
        tj, pj = _i64(T[:, 1] - 1)
        si = np.zeros(int(k), dtype=np.int64)
        sj = np.zeros(int(k), dtype=np.int64)
        rb = C.c_double()
        ns = C.c_int64()
        _lib.check(_lib.load().kt_greedy_krylov_steps(
            D.handle, int(k), int(Q), len(T), pi, pj, float(tol), int(it or 0), 1 if miobi == "make" else 0,
            float(rescale), si.ctypes.data_as(C.POINTER(C.c_int64)), sj.ctypes.data_as(C.POINTER(C.c_int64)),
            C.byref(rb), C.byref(ns)))
        m = int(ns.value)
        return np.stack([si[:m] + 1, sj[:m] + 1], axis=1), float(rb.value), D
    edges = np.zeros((0, 2), dtype=np.int64)
    rob = 0.0
    last = None
    for j in range(int(k)):  # :64-93
        if j > 0:  # drop the previously selected edge from the search space
            hit = np.flatnonzero(np.all(top == last, axis=1))
            # :84-86; with no match [1 : ind-1, ind+1 : n] is empty and so is top_edges
            top = np.delete(top, hit[0], axis=0) if len(hit) else top[:0]
        E = top[:Q]
        tmp_edges, tmp_rob, D = krylov_miobi(D, 1, E, tol, it, poles, debug, miobi, rescale)
        edges = np.vstack([edges, tmp_edges])
        rob += tmp_rob
        last = tmp_edges[0] if len(tmp_edges) else None
    return edges, rob, D


def default_greedy_tol(A, rel=1e-6, ctx: Optional[Context] = None):
    """tol = 1e-6 * exp(normest(A)) as the greedy test drivers set it
    (Tests/test_unweighted_break.m:56,74: nrm = exp(normest(A, 1e-2)))."""
    return rel * float(np.exp(normest(A, 1e-2, ctx=ctx)))


def pairs_score_topk(lam, V, P, sign=-2.0, ctx: Optional[Context] = None):
    """The MIOBI score of every pair of P (npairs x 2, 0-based as entries_fun's
    pairs) from t <= 32 eigenpairs: sum_k exp(lam[k]) exp(sign V[i, k] V[j, k])
    (MIOBIBreakEdge2.m:60-68; sign = -2 scores removing the edge, +2 adding it,
    MIOBIMakeEdge.m).  On the device (kt_pairs_score_topk); the t terms are
    added in a fixed order."""
    from .core import _colmajor, default_context
    ctx = ctx or default_context()
    lam = np.ascontiguousarray(np.asarray(lam, dtype=np.float64).ravel())
    Vc = _colmajor(V)
    if Vc.shape[1] != lam.size:
        raise ValueError(f"pairs_score_topk: V has {Vc.shape[1]} columns, lam {lam.size} values")
    P = np.asarray(P, dtype=np.int64).reshape(-1, 2)
    _, pi = _i64(P[:, 0])
    _, pj = _i64(P[:, 1])
    score = np.zeros(max(P.shape[0], 1))
    _lib.check(_lib.load().kt_pairs_score_topk(ctx.handle, Vc.shape[0], lam.size, _dptr(lam), _dptr(Vc), P.shape[0],
                                               pi, pj, float(sign), _dptr(score)))
    return score[:P.shape[0]]


def _log_mean_exp(lam):
    """log(mean(exp(lam))) as natural_connectivity_topk forms it."""
    lam = np.asarray(lam, dtype=np.float64)
    return float(np.log(np.sum(np.exp(lam - lam[0]))) + lam[0] - np.log(lam.size))


def _miobi_run(name, A, k, t, lead, tol, max_spmm, seed, ctx, outputs, gain=False, empty_R1=True):
    """What miobi_break, miobi_make and miobi_break_node share: the call of the
    library's kt_<name>(A, k, t, *lead, tol, max_spmm, seed, <outputs>, nsel,
    nconv_min, refreshes) and what is made of its results.  outputs: the
    entry's output arguments in its order -- an int64 column of k rows each but
    "score" (float64), "m" (int32), "track" ((k + 1) x t) and "V" (n x t,
    column-major); None passes NULL.  gain: rob_score is (R1 - R0) 100 / R0, an
    addition's, and not (R0 - R1) 100 / R0.  empty_R1: R1 of a matrix left
    without an entry is that of t zero eigenvalues, with no eigs_topk run.
    Returns (the integer columns cut to nsel rows, info)."""
    from .core import eigs_topk
    D = _dev(A, ctx)
    n, _ = D.info()
    k, t = int(k), int(t)
    cap, tt = max(k, 1), max(t, 1)
    kinds = {"score": (cap, np.float64, "C"), "m": (cap, np.int32, "C"), "track": ((cap + 1, tt), np.float64, "C"),
             "V": ((max(n, 1), tt), np.float64, "F")}
    out = {o: np.zeros(*kinds.get(o, (cap, np.int64, "C"))) for o in outputs if o}
    ns, ncm, nrf = C.c_int64(), C.c_int(), C.c_int()
    _lib.check(getattr(_lib.load(), "kt_" + name)(
        D.handle, k, t, *lead, float(tol), int(max_spmm), int(seed) & 0xFFFFFFFFFFFFFFFF,
        *(out[o].ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(out[o].dtype))) if o else None for o in outputs),
        C.byref(ns), C.byref(ncm), C.byref(nrf)))
    D.n, D.nnz = D.info()
    m = int(ns.value)
    if ncm.value < t:
        warnings.warn(f"{name}: eigs_topk converged nconv = {ncm.value} of the {t} eigenpairs in at least one "
                      "run; the scores use the pairs as returned", RuntimeWarning, stacklevel=3)
    lam1 = (np.zeros(t) if empty_R1 and D.nnz == 0
            else eigs_topk(D, t, tol=tol, max_spmm=max_spmm, seed=seed, ctx=ctx)[0])
    R0, R1 = _log_mean_exp(out["track"][0]), _log_mean_exp(lam1)
    info = {"scores": out["score"][:m].copy(), "track": out["track"][:m + 1].copy(), "nconv_min": int(ncm.value),
            "refreshes": int(nrf.value), "R0": R0, "R1": R1,
            "rob_score": ((R1 - R0) if gain else (R0 - R1)) * 100.0 / R0 if R0 != 0.0 else 0.0, "D": D}
    if "V" in out:
        info["V"] = np.asarray(out["V"][:n])
    return {o: a[:m].copy() for o, a in out.items() if o not in ("score", "track", "V")}, info


def miobi_break(A, k, t=25, refresh=50, mode="reference", gap_rel=0.0, tol=0.0, max_spmm=0, seed=0,
                return_V=False, ctx: Optional[Context] = None):
    """MIOBI's top-t edge removal on the device (MIOBIBreakEdge2.m and
    MIOBIBreakEdge2_weighted.m; kt_miobi_break): k times, score every edge with
    the leading t eigenpairs, remove the lowest-scoring one and shift the
    eigenvalues to first order; the eigenpairs are recomputed (eigs_topk with
    tol, max_spmm, seed) after every refresh-th step, never with refresh <= 0
    (the reference's 'NoUpdate' run; 50 is its 'Update50' run).  mode
    "reference" keeps the vectors between recomputations, which is what the
    reference's code computes; "paper" applies the first-order vector update it
    meant to.  A DeviceMatrix is edited in place.

    Returns (edges, info): edges as krylov_miobi returns them (1-based rows
    (i, j), i >= j), fewer than k once no edge is left; info: "scores", "track"
    (nsel + 1 rows of t eigenvalues: row s scores step s + 1), "nconv_min",
    "refreshes", "R0" / "R1" = log(mean(exp(lam))) of eigs_topk(., t) before and
    after, "rob_score" = (R0 - R1) 100 / R0 (:40-42, :266-268), "D" the edited
    DeviceMatrix, and "V" (n x t, the vectors after the last step) with
    return_V."""
    if mode not in ("reference", "paper"):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, "miobi_break: mode must be 'reference' or 'paper'")
    cols, info = _miobi_run("miobi_break", A, k, t, (int(refresh), 1 if mode == "paper" else 0, float(gap_rel)),
                            tol, max_spmm, seed, ctx, ("i", "j", "score", "track", "V" if return_V else None))
    return np.stack([cols["i"] + 1, cols["j"] + 1], axis=1), info


def miobi_make(A, k, t=25, refresh=50, tol=0.0, max_spmm=0, seed=0, ctx: Optional[Context] = None):
    """MIOBI's top-t edge addition on the device (MIOBIMakeEdge.m with t a
    parameter; kt_miobi_make): k times, take the m = min(max degree + k, n)
    nodes with the largest |V(:, 1)| as candidates (k the whole budget, the
    degree of the current matrix), score every non-adjacent pair of them with
    the leading t eigenpairs, add the highest-scoring one and shift the
    eigenvalues to first order; the eigenpairs are recomputed (eigs_topk with
    tol, max_spmm, seed) after every refresh-th step, never with refresh <= 0
    (the reference's 'NoUpdate' run; 50 is its 'Update50' run).  The vectors
    stay as computed between recomputations, which is what the reference's
    code computes.  A must hold unit weights; a DeviceMatrix
    is edited in place.

    Returns (edges, info): edges as krylov_miobi returns them (1-based rows
    (i, j), i > j), fewer than k once no non-adjacent candidate pair is left;
    info: "scores", "track" (nsel + 1 rows of t eigenvalues: row s scores step
    s + 1), "m" (the candidate count of every step), "nconv_min", "refreshes",
    "R0" / "R1" = log(mean(exp(lam))) of eigs_topk(., t) before and after,
    "rob_score" = (R1 - R0) 100 / R0 (:44, :186-188), and "D" the edited
    DeviceMatrix."""
    cols, info = _miobi_run("miobi_make", A, k, t, (int(refresh),), tol, max_spmm, seed, ctx,
                            ("i", "j", "score", "track", "m"), gain=True, empty_R1=False)
    info = {"scores": info.pop("scores"), "track": info.pop("track"), "m": cols["m"].astype(np.int64), **info}
    return np.stack([cols["i"] + 1, cols["j"] + 1], axis=1), info


def nodes_score_topk(A, lam, V, ctx: Optional[Context] = None):
    """The MIOBI score of every node of A from t <= 32 eigenpairs: sum_k
    exp(lam[k]) exp(-2 V[r, k] W[r, k]) with W[r, :] the sum of V's rows over
    the neighbours of r, +Inf for a node without one (MIOBIBreakNode.m:186-202).
    On the device (kt_nodes_score_topk); the neighbours and the t terms are
    added in a fixed order.  A must hold unit weights and a zero diagonal; V is
    used as given."""
    from .core import _colmajor
    D = _dev(A, ctx)
    n, _ = D.info()
    lam = np.ascontiguousarray(np.asarray(lam, dtype=np.float64).ravel())
    Vc = _colmajor(V)
    if Vc.shape != (n, lam.size):
        raise ValueError(f"nodes_score_topk: V is {Vc.shape[0]} x {Vc.shape[1]}, expected {n} x {lam.size}")
    score = np.zeros(max(n, 1))
    _lib.check(_lib.load().kt_nodes_score_topk(D.handle, lam.size, _dptr(lam), _dptr(Vc), _dptr(score)))
    return score[:n]


def miobi_break_node(A, k, t=25, refresh=50, shift="reference", tol=0.0, max_spmm=0, seed=0,
                     ctx: Optional[Context] = None):
    """MIOBI's top-t node removal on the device (MIOBIBreakNode.m's second loop
    with t a parameter; kt_miobi_break_node): k times, score every node that
    still has a neighbour with the leading t eigenpairs, remove the
    lowest-scoring one (its row and column are cleared) and shift the
    eigenvalues.  shift "reference" is what the reference's code computes (its
    deltaA sets the node's WHOLE row and column to -1), "first_order" the shift
    for the entries actually removed.  Every step adds twice
    the removed node's degree to a count; once the count reaches `refresh` (the
    reference's 50) it is taken mod refresh and the eigenpairs are recomputed
    (eigs_topk with tol, max_spmm, seed); never with refresh <= 0 (the
    'NoUpdate' run).  The vectors stay as computed between recomputations.  A
    must hold unit weights and a zero diagonal; a DeviceMatrix is edited in
    place.

    Returns (nodes, info): nodes 1-based, fewer than k once no node has a
    neighbour; info: "scores", "degrees" (of each node when it was removed),
    "track" (nsel + 1 rows of t eigenvalues: row s scores step s + 1),
    "nconv_min", "refreshes", "R0" / "R1" = log(mean(exp(lam))) of
    eigs_topk(., t) before and after, "rob_score" = (R0 - R1) 100 / R0
    (:299-301), and "D" the edited DeviceMatrix."""
    if shift not in ("reference", "first_order"):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, "miobi_break_node: shift must be 'reference' or 'first_order'")
    cols, info = _miobi_run("miobi_break_node", A, k, t, (int(refresh), 1 if shift == "first_order" else 0),
                            tol, max_spmm, seed, ctx, ("node", "score", "degree", "track"))
    info = {"scores": info.pop("scores"), "degrees": cols["degree"], **info}
    return cols["node"] + 1, info


def _node_args(who, A, nodes, it, fun):
    """What the node entries reject before a device is touched; nodes 0-based."""
    code = _fun_code(fun)
    if code == _lib.FUN_CODES["log"]:
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: fun = log is not supported (f(0) of the isolated node "
                                                "is not finite)")
    if it is not None and int(it) > 256:
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: it must be at most 256")
    nodes = np.asarray(nodes, dtype=np.int64).ravel() - 1
    n = A.n if isinstance(A, DeviceMatrix) else A.shape[0]
    if nodes.size and (nodes.min() < 0 or nodes.max() >= n):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: node index out of range (1-based, 1..{n})")
    return code, nodes


def trace_fun_update_nodes(A, nodes, tol=1e-12, it=None, fun="exp", ctx: Optional[Context] = None):
    """Xm[c] ~= trace(f(A_{-i})) - trace(f(A)) for every node i of `nodes`
    (1-based, as miobi_break_node's; duplicates are legal), A_{-i} being A with
    row and column i zeroed -- the node stays as an isolated vertex.  From the
    single-vector Lanczos run started at e_i (kt_trace_fun_update_nodes;
    DESIGN.md §4.2h) with trace_fun_update's stopping rule: tol is absolute
    and means what it means to trace_fun_update_pairs.  A candidate's values do
    not depend on the other candidates of the call.  fun "log" is rejected.
    The rule's first test compares X_3 with X_1: a tol above both stops the
    column at depth 3 whatever its limit is, which happens to hubs of large
    graphs at tol ~ 1e-6 exp(normest(A)); check iter.
    Returns (Xm, iter, lucky) arrays."""
    code, nd = _node_args("trace_fun_update_nodes", A, nodes, it, fun)
    D = _dev(A, ctx)
    q = nd.size
    nd, pn = _i64(nd)
    xm = np.zeros(max(q, 1))
    itr = np.zeros(max(q, 1), dtype=np.int32)
    lk = np.zeros(max(q, 1), dtype=np.int32)
    _lib.check(_lib.load().kt_trace_fun_update_nodes(
        D.handle, q, pn, float(tol), int(it or 0), code, _dptr(xm),
        itr.ctypes.data_as(C.POINTER(C.c_int)), lk.ctypes.data_as(C.POINTER(C.c_int))))
    return xm[:q], itr[:q], lk[:q]


def krylov_break_node(A, k, nodes, tol=1e-12, it=None, fun="exp", ctx: Optional[Context] = None):
    """Greedy node removal scored by trace_fun_update_nodes: up to k times, score
    every remaining candidate of `nodes` (1-based; find_top_nodes_miobi or a
    degree ranking can feed it) on the current matrix, remove the one with the
    smallest Xm (the first on ties) -- its row and column are zeroed -- and drop
    it from the list (kt_krylov_break_node).  A DeviceMatrix is edited in place.

    Returns (nodes, rob, D, info): the removed nodes (1-based, fewer than k when
    the list ran out), rob = the summed Xm ~= trace(f(A_new)) - trace(f(A)), the
    edited DeviceMatrix, and info: "xm", the Xm of each removed node when it was
    removed."""
    code, nd = _node_args("krylov_break_node", A, nodes, it, fun)
    D = _dev(A, ctx)
    k = int(k)
    q = nd.size
    nd, pn = _i64(nd)
    cap = max(min(k, q), 1)
    sn = np.zeros(cap, dtype=np.int64)
    sx = np.zeros(cap)
    rob = C.c_double()
    ns = C.c_int64()
    _lib.check(_lib.load().kt_krylov_break_node(
        D.handle, k, q, pn, float(tol), int(it or 0), code, sn.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(sx),
        C.byref(rob), C.byref(ns)))
    D.n, D.nnz = D.info()
    m = int(ns.value)
    return sn[:m] + 1, float(rob.value), D, {"xm": sx[:m].copy()}


def lambda_upper(A, rounds=8, ctx: Optional[Context] = None, v=None):
    """An upper bound on lambda_max of symmetric A, what diag_fun_bracket's
    lam_hi=None uses.  For an entrywise non-negative A it is rigorous by
    Collatz-Wielandt: lambda_max <= max_i (A x)_i / x_i for any x > 0.  x starts
    at |v| + 1e-3 max|v| with v the leading eigenvector of eigs_leading (or the
    given v, and then no device is touched) and takes `rounds` steps x <- (A +
    I) x, normalised, none of which can raise the bound; the result is the
    smaller of that and ||A||_inf.  A matrix with a negative entry gets
    ||A||_inf.  Host numpy on the exported CSR; multiplied by 1 + 1e-12 so that
    rounding cannot put it below lambda_max."""
    import scipy.sparse as sp
    M = sp.csr_matrix(A.to_scipy() if isinstance(A, DeviceMatrix) else A, dtype=np.float64)
    n = M.shape[0]
    slack = 1.0 + 1e-12
    norm_inf = float(abs(M).sum(axis=1).max()) if M.nnz else 0.0
    if n == 0 or M.nnz == 0 or M.data.min() < 0.0:
        return norm_inf * slack
    if v is None:
        from .core import eigs_leading
        v = eigs_leading(A, ctx=ctx)[1]
    x = np.abs(np.asarray(v, dtype=np.float64).ravel())
    if x.size != n or not np.all(np.isfinite(x)) or x.max() <= 0.0:
        x = np.ones(n)
    x = x + 1e-3 * x.max()
    bound = norm_inf
    for r in range(int(rounds) + 1):
        y = M @ x
        bound = min(bound, float(np.max(y / x)))
        if r < int(rounds):
            x = y + x
            x /= x.max()
    return bound * slack


def diag_fun_bracket(A, nodes, rtol=1e-10, it=None, lam_hi=None, ctx: Optional[Context] = None):
    """Proved bounds lo[c] <= exp(A)_ii <= hi[c] on the subgraph centrality of
    every node i of `nodes` (1-based, as trace_fun_update_nodes'; duplicates are
    legal): the Gauss and Gauss-Radau rules of the Lanczos run started at e_i
    (kt_diag_fun_bracket), each column run until hi - lo <=
    rtol lo.  lam_hi must be an upper bound on lambda_max(A) (None:
    lambda_upper(A)); the upper bounds are proved only if it is one.  f = exp
    only.  A candidate's values do not depend on the other candidates of the
    call.  Returns (lo, hi, iter, flag) arrays; flag 0: the gap was reached, 1:
    the Krylov space ended, hi = lo is exact, 2: lam_hi is proved to be below
    lambda_max, lo holds and hi is NaN, 3: `it` steps (None: min(100, n); at
    most 256) did not reach the gap, the bracket is still valid."""
    who = "diag_fun_bracket"
    if it is not None and int(it) > 256:
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: it must be at most 256")
    nd = np.asarray(nodes, dtype=np.int64).ravel() - 1
    n = A.n if isinstance(A, DeviceMatrix) else A.shape[0]
    if nd.size and (nd.min() < 0 or nd.max() >= n):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: node index out of range (1-based, 1..{n})")
    if lam_hi is not None and not (np.isfinite(lam_hi) and float(lam_hi) <= 700.0):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: lam_hi must be finite and at most 700")
    D = _dev(A, ctx)
    if lam_hi is None:
        # n <= 130 takes the dense host path, which has no use for a Radau node
        lam_hi = lambda_upper(D, ctx=ctx) if n > 130 else 0.0
    q = nd.size
    nd, pn = _i64(nd)
    lo = np.zeros(max(q, 1))
    hi = np.zeros(max(q, 1))
    itr = np.zeros(max(q, 1), dtype=np.int32)
    fl = np.zeros(max(q, 1), dtype=np.int32)
    _lib.check(_lib.load().kt_diag_fun_bracket(
        D.handle, q, pn, float(lam_hi), float(rtol), int(it or 0), _dptr(lo), _dptr(hi),
        itr.ctypes.data_as(C.POINTER(C.c_int)), fl.ctypes.data_as(C.POINTER(C.c_int))))
    return lo[:q], hi[:q], itr[:q], fl[:q]


def find_top_nodes_fun(A, num, ncand=None, nprobes=256, deflate=1, rtol=1e-10, m=30, seed=0, it=None, lam_hi=None,
                       fun="exp", ctx: Optional[Context] = None):
    """The top `num` nodes by subgraph centrality exp(A)_ii with a proved order
    among the candidates: rank all nodes by the stochastic estimate
    diag_fun(A, nprobes, m, seed, deflate=deflate).mean, bracket the first
    `ncand` of that ranking (default 4 num) with diag_fun_bracket(rtol, it,
    lam_hi) and return the first `num` of them by descending lower bound, ties
    by index; 1-based.

    Returns (nodes, info): info "candidates" (1-based, in the bracketed order:
    descending lo, ties by index), "lo" and "hi" in that order, and "separated":
    True when every lo[r] > hi[r + 1] over all bracketed candidates, so their
    order is proved.  That proof covers the candidate set only: a node the
    stochastic ranking left out of it is bounded by nothing here, and may
    belong among the returned ones.  With the defaults that happens: 256 probes
    leave the estimate several per cent off per node, so where the top nodes
    are nearly tied (rome: the fifth is 0.05 % above the sixth) a true top node
    can be missing from the 4 num candidates; raise nprobes and ncand until the
    candidate set holds every node within a few standard errors
    (diag_fun(...).stderr) of the num-th value.  f = exp only: the bracket needs every
    derivative of f positive, which cosh, sinh and the other kt_fun codes do
    not give for a single Radau node."""
    if _fun_code(fun) != _lib.FUN_CODES["exp"]:
        raise _lib.KrylovError(_lib.KT_ERR_ARG, "find_top_nodes_fun: only fun = exp is supported (the Gauss / "
                                                "Gauss-Radau bracket needs every derivative of f positive)")
    from .core import diag_fun
    D = _dev(A, ctx)
    n, _ = D.info()
    num = int(np.floor(num))
    if n < num:
        raise IndexError("FIND_TOP_NODES:: there are not enough nodes in the graph")
    ncand = min(n, max(num, 4 * num if ncand is None else int(ncand)))
    est = diag_fun(D, nprobes, m=m, seed=seed, fun="exp", deflate=deflate, ctx=D.ctx).mean
    cand = _stable_head(-est, ncand)
    lo, hi, _, _ = diag_fun_bracket(D, cand + 1, rtol=rtol, it=it, lam_hi=lam_hi, ctx=D.ctx)
    order = np.lexsort((cand, -lo))
    cand, lo, hi = cand[order], lo[order], hi[order]
    separated = bool(np.all(lo[:-1] > hi[1:])) if ncand > 1 else True
    return cand[:num] + 1, {"lo": lo, "hi": hi, "candidates": cand + 1, "separated": separated}


def entries_fun_bracket(A, pairs, rtol=1e-10, ftol=1e-12, it=None, lam_hi=None, ctx: Optional[Context] = None):
    """Proved bounds lo[p] <= exp(A)[i, j] <= hi[p] on the communicability of
    every row (i, j) of `pairs` ((npairs, 2) integers, 0-BASED as entries_fun
    takes them; repeats and both orientations are legal, and (i, j) and (j, i)
    return the same bits): half the difference of the Gauss / Gauss-Radau
    brackets of the quadratic forms of exp at (e_i + e_j) / sqrt 2 and (e_i -
    e_j) / sqrt 2 (kt_entries_fun_bracket).  Rows with i == j
    are answered by diag_fun_bracket(rtol, it, lam_hi) and returned in place.
    lam_hi must be an upper bound on lambda_max(A) (None: lambda_upper(A)); the
    bounds are proved only if it is one.  f = exp only.  A row's values do not
    depend on the other rows of the call.  Returns (lo, hi, iter, flag) arrays;
    flag 0: lo and hi have one sign and hi - lo <= rtol min(|lo|, |hi|), 1:
    both Krylov spaces ended, hi = lo is exact, 2: lam_hi is proved to be below
    lambda_max, lo and hi are NaN (a diagonal row keeps its lo), 3: `it` steps
    (None: min(100, n); at most 256) reached neither, the bracket is still
    valid, 4: hi - lo <= ftol times the mean of the two quadratic forms, about
    (exp(A)[i, i] + exp(A)[j, j]) / 2 -- the bracket has closed to the rounding
    level of the method, the entry is smaller than that and all that is known
    of it; such a bracket can be inverted by a few ulps of that scale."""
    who = "entries_fun_bracket"
    P = np.asarray(pairs)
    if P.ndim != 2 or P.shape[1] != 2:
        raise ValueError(f"{who}: pairs must have shape (npairs, 2), got {P.shape}")
    if not np.issubdtype(P.dtype, np.integer):
        raise ValueError(f"{who}: pairs must be integers, got {P.dtype}")
    if it is not None and int(it) > 256:
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: it must be at most 256")
    n = A.n if isinstance(A, DeviceMatrix) else A.shape[0]
    if P.size and (P.min() < 0 or P.max() >= n):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: pair index out of range (0-based, 0..{n - 1})")
    if lam_hi is not None and not (np.isfinite(lam_hi) and float(lam_hi) <= 700.0):
        raise _lib.KrylovError(_lib.KT_ERR_ARG, f"{who}: lam_hi must be finite and at most 700")
    D = _dev(A, ctx)
    if lam_hi is None:
        # n <= 130 takes the dense host path, which has no use for a Radau node
        lam_hi = lambda_upper(D, ctx=ctx) if n > 130 else 0.0
    q = P.shape[0]
    lo = np.zeros(q)
    hi = np.zeros(q)
    itr = np.zeros(q, dtype=np.int32)
    fl = np.zeros(q, dtype=np.int32)
    diag = P[:, 0] == P[:, 1]
    off = np.flatnonzero(~diag)
    if off.size:
        ei, pi = _i64(P[off, 0])
        ej, pj = _i64(P[off, 1])
        olo, ohi = np.zeros(off.size), np.zeros(off.size)
        oit, ofl = np.zeros(off.size, dtype=np.int32), np.zeros(off.size, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        _lib.check(_lib.load().kt_entries_fun_bracket(
            D.handle, off.size, pi, pj, float(lam_hi), float(rtol), float(ftol), int(it or 0), _dptr(olo),
            _dptr(ohi), oit.ctypes.data_as(ip), ofl.ctypes.data_as(ip), None))
        lo[off], hi[off], itr[off], fl[off] = olo, ohi, oit, ofl
    if diag.any():
        lo[diag], hi[diag], itr[diag], fl[diag] = diag_fun_bracket(D, P[diag, 0] + 1, rtol=rtol, it=it,
                                                                   lam_hi=lam_hi, ctx=D.ctx)
    return lo, hi, itr, fl


def find_top_edges_bracket(A, num, ncand=None, nprobes=256, deflate=1, rtol=1e-10, ftol=1e-12, m=30, seed=0,
                           it=None, lam_hi=None, ctx: Optional[Context] = None):
    """The top `num` existing edges by communicability exp(A)[i, j] with a
    proved order among the candidates, the edge twin of find_top_nodes_fun:
    rank every edge of find(tril(A, -1)) by the stochastic estimate
    entries_fun(nprobes, m, seed, deflate=deflate).mean (find_top_edges_fun's
    ranking), bracket the first `ncand` of it (default 4 num) with
    entries_fun_bracket(rtol, ftol, it, lam_hi) and return the first `num` of
    them by descending lower bound, ties in find(tril(A, -1)) order; 1-based
    with i > j, as find_top_edges returns them, so the result serves as
    greedy_krylov(..., top=...).  The same warning / error when fewer than
    `num` edges exist.

    Returns (edges, info): info "candidates" ((ncand, 2), 1-based, i > j, in
    the bracketed order), "lo" and "hi" in that order, and "separated": True
    when every lo[r] > hi[r + 1] over all bracketed candidates, so their order
    is proved.  That proof covers the candidate set only: an edge the stochastic
    ranking left out of it is bounded by nothing here, and may belong among the
    returned ones; 256 probes leave the estimate several per cent off per
    entry, so where the top edges are nearly tied raise nprobes and ncand until
    the candidate set holds every edge within a few standard errors
    (entries_fun(...).stderr) of the num-th value.
    f = exp only."""
    from .core import _deflate_arg, entries_fun
    deflate = _deflate_arg("find_top_edges_bracket", deflate, A)
    D = _dev(A, ctx)
    I, J = _tril_edges(D.to_scipy())
    if len(I) < num:
        warnings.warn("FIND_TOP_EDGES:: there are not enough edges in the graph")
    num = int(np.floor(num))
    if len(I) < num:
        raise IndexError("FIND_TOP_EDGES:: there are not enough edges in the graph")
    if len(I) == 0:
        return np.zeros((0, 2), dtype=np.int64), {"lo": np.zeros(0), "hi": np.zeros(0),
                                                   "candidates": np.zeros((0, 2), dtype=np.int64), "separated": True}
    ncand = min(len(I), max(num, 4 * num if ncand is None else int(ncand)))
    est = entries_fun(D, np.stack([I, J], axis=1), nprobes, m=m, seed=seed, fun="exp", deflate=deflate, ctx=ctx)
    cand = _stable_head(-np.asarray(est.mean, dtype=np.float64), ncand)
    lo, hi, _, _ = entries_fun_bracket(D, np.stack([I[cand], J[cand]], axis=1), rtol=rtol, ftol=ftol, it=it,
                                       lam_hi=lam_hi, ctx=D.ctx)
    order = np.lexsort((cand, -lo))
    cand, lo, hi = cand[order], lo[order], hi[order]
    separated = bool(np.all(lo[:-1] > hi[1:])) if ncand > 1 else True
    E = np.stack([I[cand] + 1, J[cand] + 1], axis=1)
    return E[:num], {"lo": lo, "hi": hi, "candidates": E, "separated": separated}


def find_top_nodes_miobi(A, num, t=25, tol=0.0, max_spmm=0, seed=0, ctx: Optional[Context] = None):
    """The top `num` nodes ranked by ascending MIOBI node score (the node
    miobi_break_node would remove first comes first) from the leading t
    eigenpairs of eigs_topk, column 0 by absolute value (MIOBIBreakNode.m:
    176-204); 1-based, ties in node order.  Nodes without a neighbour score
    +Inf and come last."""
    from .core import eigs_topk
    D = _dev(A, ctx)
    n, _ = D.info()
    num = int(np.floor(num))
    if n < num:
        raise IndexError("FIND_TOP_NODES:: there are not enough nodes in the graph")
    lam, V = eigs_topk(D, t, tol=tol, max_spmm=max_spmm, seed=seed, ctx=ctx)
    V = np.array(V, order="F")
    V[:, 0] = np.abs(V[:, 0])
    score = nodes_score_topk(D, lam, V, ctx=D.ctx)
    return _stable_head(score, num) + 1


def find_top_edges_miobi(A, num, t=25, tol=0.0, max_spmm=0, seed=0, ctx: Optional[Context] = None):
    """The top `num` existing edges ranked by ascending MIOBI score (the edge
    MIOBI would remove first comes first) from the leading t eigenpairs of
    eigs_topk, column 0 by absolute value (MIOBIBreakEdge2.m:47-68), returned as
    find_top_edges returns them: 1-based, i > j, enumerated in find(tril(A, -1))
    order with ties kept in that order, and the same warning / error when fewer
    than `num` edges exist -- a ranking greedy_krylov(..., top=...) takes."""
    from .core import eigs_topk
    D = _dev(A, ctx)
    I, J = _tril_edges(D.to_scipy())
    if len(I) < num:
        warnings.warn("FIND_TOP_EDGES:: there are not enough edges in the graph")
    num = int(np.floor(num))
    if len(I) < num:
        raise IndexError("FIND_TOP_EDGES:: there are not enough edges in the graph")
    if len(I) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    lam, V = eigs_topk(D, t, tol=tol, max_spmm=max_spmm, seed=seed, ctx=ctx)
    V = np.array(V, order="F")
    V[:, 0] = np.abs(V[:, 0])
    score = pairs_score_topk(lam, V, np.stack([I, J], axis=1), sign=-2.0, ctx=D.ctx)
    ind = _stable_head(score, num)
    return np.stack([I[ind] + 1, J[ind] + 1], axis=1)

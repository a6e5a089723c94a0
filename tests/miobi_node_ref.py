"""NumPy restatement of the reference's MIOBI node removal, MIOBIBreakNode.m,
with t a parameter (the file hard-codes t = 50) and the recomputation
threshold as a parameter: its second ("Update50", :176-297) loop with refresh
= 50; refresh = 0 never recomputes.  Test infrastructure in the manner of
tests/miobi_ref.py and tests/miobi_make_ref.py: the eigensolver is a callback,
so the same code runs on numpy.linalg.eigh (tests/test_miobi_node_host.py) and
on the device's eigs_topk (tests/test_gpu_miobi_node.py).

Kept literally, per step:

  * the score of node n (:186-202): [p, r] = find(A) lists both triangles and
    indexP / indexR each pick the deg(n) entries of row / column n, so colSum_k
    = -2 V[n, k] (A V)[n, k] over the CURRENT matrix; a node without an entry
    scores +Inf (isolated="inf", the second loop) or sum(exp(e)) (isolated=
    "sum", the first loop, :70-79: the empty sum is 0 and exp(0) = 1); the
    FIRST minimum (:204);
  * the eigenvalue shift (:214-223): deltaA(remove, :) = -ep; deltaA(:, remove)
    = -ep assigns the WHOLE row and column, all N entries, so deltaE_k =
    -(2 V[r, k] s_k - V[r, k]^2) with s_k = sum_i V[i, k] over all N rows
    (shift="reference"); shift="first_order" is the shift for the entries
    actually removed, deltaE_k = -2 V[r, k] (A V)[r, k];
  * the vector update with [naR, naC] = find(isfinite(diffE)); diffE(naR, naC)
    = 0 (:232-233), which zeroes all of diffE (tests/miobi_ref.py inner_sum):
    the vectors are only divided by their norm, column 1 by absolute value;
  * the recomputation (:208, :283-295): edgesRM += sum(A(remove, :)) +
    sum(A(:, remove)) = 2 deg before the removal; at edgesRM >= refresh the
    eigenpairs are recomputed and edgesRM = mod(edgesRM, refresh).  As in the
    edge files the recomputation after the LAST step is never read and is
    skipped, as is one of a matrix without entries.
"""
import numpy as np
import scipy.sparse as sp

from miobi_make_ref import binarise
from miobi_ref import eigh_topk, inner_sum, log_mean_exp, rob_score  # noqa: F401  (the callers' helpers)


def current(S, live):
    """A with the removed nodes' rows and columns zeroed (:211-212)."""
    L = sp.diags(live.astype(np.float64))
    M = sp.csr_matrix(L @ S @ L)
    M.eliminate_zeros()
    M.sort_indices()
    return M


def node_scores(M, V, e, isolated="inf"):
    """:186-202 vectorised: score(n) = sum(c .* exp(-2 V(n, :) .* (M V)(n, :)))."""
    W = M @ V
    sc = np.sum(np.exp(e)[None, :] * np.exp(-2.0 * V * W), axis=1)
    if isolated == "inf":
        sc[np.diff(M.indptr) == 0] = np.inf                           # :199-201
    return sc


def node_score_literal(M, V, e, n, isolated="inf"):
    """:186-202 as written, for one node (0-based n)."""
    F = sp.csc_matrix(M).tocoo()                                      # find() runs down the columns
    p, r = F.row, F.col
    c = np.exp(e)
    indexP = np.flatnonzero(p == n)
    indexR = np.flatnonzero(r == n)
    if isolated == "inf" and not (len(indexP) and len(indexR)):
        return np.inf
    idx = np.concatenate([indexP, indexR])
    tnig = -1.0 * V[p[idx]] * V[r[idx]]
    return float(np.sum(c * np.exp(tnig.sum(axis=0))))


def delta_h(V, r, Wr=None):
    """deltaH = V' deltaA V.  Wr None: deltaA's whole row and column r at -1
    (:216-217; entry (r, r) once).  Wr = (A V)[r, :]: -1 on the entries removed."""
    v = V[r]
    if Wr is None:
        s = V.sum(axis=0)
        return -(np.outer(v, s) + np.outer(s, v) - np.outer(v, v))
    return -(np.outer(v, Wr) + np.outer(Wr, v))


def delta_h_dense(V, r):
    """:214-219 with the dense N x N deltaA, for small N."""
    n = V.shape[0]
    dA = np.zeros((n, n))
    dA[r, :] = -1.0
    dA[:, r] = -1.0
    return V.T @ dA @ V


def update(V, e, r, Wr, shift):
    """One step's eigenpair update (:214-281): returns (V_new, e_new, deltaV)."""
    dH = delta_h(V, r, None if shift == "reference" else Wr)
    e_new = e + np.diag(dH)                                           # :221-223
    dV = V @ inner_sum(dH, e, "reference")                            # :225-270
    Vn = V + dV                                                       # :272
    Vn = Vn / np.linalg.norm(Vn, axis=0)                              # :274-276
    Vn[:, 0] = np.abs(Vn[:, 0])                                       # :281
    return Vn, e_new, dV


def _eig(eig, M, t):
    e, V = eig(M, t)
    e, V = np.array(e, dtype=np.float64), np.array(V, dtype=np.float64)
    V[:, 0] = np.abs(V[:, 0])                                         # :177
    return e, V


def miobi_break_node_ref(A, k, t, eig, refresh=50, shift="reference", isolated="inf", forced=None):
    """Run k steps.  eig(S, t) -> (lam, V) is called on the binarised matrix at
    the start and whenever the removed-entry count reaches refresh (> 0), but
    not after the last step nor on an empty matrix.  forced: a sequence of
    0-based nodes to remove instead of the run's own argmin (the run still
    reports its own).  Returns a dict:
      nodes     (nsel,) 0-based, the nodes removed;  own  the run's own argmin
      score     the removed node's score;  smin  the run's own minimum
      gap       (second smallest - smallest) / |smallest| (inf with one candidate)
      excess    (removed node's score - smallest) / |smallest|
      alive     whether the forced node still had a neighbour
      degree    the removed node's degree before the removal
      acc       the removed-entry count after every step (after the mod)
      wend      whether the count reached refresh at that step
      track     (nsel + 1, t): row s = the eigenvalues that score step s + 1
      dv_max    max |deltaV| of every step
      A (the final matrix), refreshes, nsel"""
    if shift not in ("reference", "first_order") or isolated not in ("inf", "sum"):
        raise ValueError("shift is 'reference' or 'first_order', isolated 'inf' or 'sum'")
    S = binarise(A)
    assert S.diagonal().sum() == 0.0, "the restatement, as the device route, takes a zero diagonal"
    n = S.shape[0]
    live = np.ones(n, dtype=bool)
    M = current(S, live)
    e, V = _eig(eig, M, t)
    names = ("nodes", "own", "score", "smin", "gap", "excess", "alive", "degree", "acc", "wend", "dv_max")
    out = {k_: [] for k_ in names}
    track = [e.copy()]
    refreshes, acc = 0, 0
    for step in range(1, int(k) + 1):
        sc = node_scores(M, V, e, isolated)
        if not np.isfinite(sc).any():
            break
        o = int(np.argmin(sc))                                        # :204  the first minimum
        smin = float(sc[o])
        rest = np.delete(sc, o)
        with np.errstate(invalid="ignore"):
            gap = float((rest.min() - smin) / abs(smin)) if len(rest) else np.inf
        q = o
        if forced is not None:
            q = int(forced[step - 1])
            if not (0 <= q < n and np.isfinite(sc[q])):
                out["alive"].append(False)
                break
        deg = int(M.indptr[q + 1] - M.indptr[q])
        Wr = np.asarray(M[q] @ V).ravel()
        out["nodes"].append(q)
        out["own"].append(o)
        out["score"].append(float(sc[q]))
        out["smin"].append(smin)
        out["gap"].append(gap)
        out["excess"].append((float(sc[q]) - smin) / abs(smin))
        out["alive"].append(True)
        out["degree"].append(deg)
        acc += 2 * deg                                                # :208, :283
        V, e, dV = update(V, e, q, Wr, shift)
        out["dv_max"].append(float(np.max(np.abs(dV))) if dV.size else 0.0)
        live[q] = False                                               # :211-212
        M = current(S, live)
        wend = refresh > 0 and acc >= refresh                         # :286
        if wend:
            acc %= refresh                                            # :292
            if step < k and M.nnz > 0:
                e, V = _eig(eig, M, t)
                refreshes += 1
        out["acc"].append(acc)
        out["wend"].append(bool(wend))
        track.append(e.copy())
    res = {k_: np.array(v) for k_, v in out.items()}
    res["nodes"] = res["nodes"].astype(np.int64)
    res["own"] = res["own"].astype(np.int64)
    res.update(track=np.array(track), A=M, refreshes=refreshes, nsel=len(out["nodes"]))
    return res

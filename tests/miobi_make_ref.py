"""NumPy restatement of the reference's MIOBI edge addition, MIOBIMakeEdge.m,
with t a parameter (the file hard-codes t = 50) and the recomputation period
as a parameter: refresh = 0 is its first ("NoUpdate", :59-184) loop, refresh =
50 its second ("Update50", :201-334).  Test infrastructure in the manner of
tests/miobi_ref.py: the eigensolver is a callback, so the same code runs on
numpy.linalg.eigh (tests/test_miobi_make_host.py) and on the device's
eigs_topk (tests/test_gpu_miobi_make.py).

Kept literally, per step: the degrees of the CURRENT matrix and m = min(max
degree + k, N) with k the whole budget (:60-63); the stable descending sort of
V(:, 1) (:62); the a-then-b enumeration of the non-adjacent candidate pairs
(:72-80); score = sum(c .* exp(2 Up .* Ur), 2) and the FIRST maximum (:88-97);
the first-order eigenvalue shift (:109-118); and the vector update with

    [naR, naC] = find(isfinite(diffE));  diffE(naR, naC) = 0;          (:133-134)

through np.ix_, which zeroes all of diffE (tests/miobi_ref.py inner_sum): the
vectors are only divided by their norm, column 1 taken by absolute value.  As
in the break file, the recomputation after the LAST step (:326) is never read
and is skipped.
"""
import numpy as np
import scipy.sparse as sp

from miobi_ref import eigh_topk, inner_sum, log_mean_exp  # noqa: F401  (eigh_topk: the callers' callback)


def binarise(A):
    """:27-35  A = A + A'; A(find(A)) = 1 -- the pattern of A or A', all ones."""
    S = sp.csr_matrix(A, dtype=np.float64)
    S = sp.csr_matrix(abs(S) + abs(S.T))
    S.eliminate_zeros()
    S.data[:] = 1.0
    S.sort_indices()
    return S


def candidates(v0, m):
    """:62-63  the first m of [~, sortIndex] = sort(V(:, 1), 'descend'): stable,
    so equal values keep ascending index."""
    return np.argsort(-np.asarray(v0), kind="stable")[:m]


def enumerate_pairs(adj, cand):
    """:72-80 vectorised: rank positions a < b with adj[cand[a], cand[b]] == 0,
    a ascending, then b ascending."""
    sub = adj[np.ix_(cand, cand)]
    return np.nonzero(np.triu(~sub, 1))


def enumerate_pairs_loop(adj, cand):
    """:72-80 as written: the double loop."""
    ia, ib = [], []
    for a in range(len(cand)):
        for b in range(a + 1, len(cand)):
            if adj[cand[a], cand[b]] == 0:
                ia.append(a)
                ib.append(b)
    return np.array(ia, dtype=np.int64), np.array(ib, dtype=np.int64)


def scores(V, e, p, r):
    """:88-94  score = sum(c .* exp(2 Up .* Ur), 2), c = exp(e)'."""
    return np.sum(np.exp(e)[None, :] * np.exp(2.0 * V[p] * V[r]), axis=1)


def update(V, e, i, j):
    """One step's eigenpair update (:103-152) for deltaA(i, j) = deltaA(j, i) =
    1: returns (V_new, e_new, deltaV)."""
    u, v = V[i], V[j]
    dH = np.outer(u, v) + np.outer(v, u)                              # :107  V' deltaA V
    e_new = e + np.diag(dH)                                           # :109-111
    dV = V @ inner_sum(dH, e, "reference")                            # :113-166
    Vn = V + dV                                                       # :168
    Vn = Vn / np.linalg.norm(Vn, axis=0)                              # :170-172
    Vn[:, 0] = np.abs(Vn[:, 0])                                       # :177
    return Vn, e_new, dV


def _eig(eig, adj, t):
    e, V = eig(sp.csr_matrix(adj.astype(np.float64)), t)
    e, V = np.array(e, dtype=np.float64), np.array(V, dtype=np.float64)
    V[:, 0] = np.abs(V[:, 0])                                         # :49
    return e, V


def miobi_make_ref(A, k, t, eig, refresh=0, forced=None):
    """Run k steps.  eig(S, t) -> (lam, V) is called on the binarised matrix at
    the start and after every refresh-th step but the last.  forced: a
    sequence of 0-based pairs to add instead of the run's own argmax (the run
    still reports its own).  Returns a dict:
      edges     (nsel, 2) 0-based (larger, smaller) of the pairs added
      own       (nsel, 2) the run's own argmax at every step, same convention
      score     the added pair's score;  smax  the run's own maximum
      gap       (largest - second largest) / |largest| (inf with one pair)
      excess    (largest - added pair's score) / |largest|
      alive     whether the forced pair was a non-adjacent candidate pair
      m         the candidate count of every step;  npairs  its pairs
      track     (nsel + 1, t): row s = the eigenvalues that score step s + 1
      dv_max    max |deltaV| of every step
      A (the final matrix), refreshes, nsel"""
    S = binarise(A)
    n = S.shape[0]
    adj = S.toarray() != 0
    e, V = _eig(eig, adj, t)
    out = {k_: [] for k_ in ("edges", "own", "score", "smax", "gap", "excess", "alive", "m", "npairs", "dv_max")}
    track = [e.copy()]
    refreshes = 0
    for step in range(1, int(k) + 1):
        maxdeg = int(adj.sum(axis=1).max())                           # :60-61
        m = min(maxdeg + int(k), n)                                   # :63
        cand = candidates(V[:, 0], m)
        ia, ib = enumerate_pairs(adj, cand)
        if len(ia) == 0:
            break
        sc = scores(V, e, cand[ia], cand[ib])
        o = int(np.argmax(sc))                                        # :97  the first maximum
        smax = float(sc[o])
        rest = np.delete(sc, o)
        gap = float((smax - rest.max()) / abs(smax)) if len(rest) else np.inf
        q = o
        if forced is not None:
            pos = {int(v): a for a, v in enumerate(cand)}
            f = [pos.get(int(x), -1) for x in forced[step - 1]]
            hit = np.flatnonzero((ia == min(f)) & (ib == max(f))) if min(f) >= 0 else []
            if len(hit) != 1:
                out["alive"].append(False)
                break
            q = int(hit[0])
        i, j = int(cand[ia[q]]), int(cand[ib[q]])
        io, jo = int(cand[ia[o]]), int(cand[ib[o]])
        out["edges"].append((max(i, j), min(i, j)))
        out["own"].append((max(io, jo), min(io, jo)))
        out["score"].append(float(sc[q]))
        out["smax"].append(smax)
        out["gap"].append(gap)
        out["excess"].append((smax - float(sc[q])) / abs(smax))
        out["alive"].append(True)
        out["m"].append(m)
        out["npairs"].append(len(ia))
        adj[i, j] = adj[j, i] = True                                  # :100-101
        V, e, dV = update(V, e, i, j)
        out["dv_max"].append(float(np.max(np.abs(dV))) if dV.size else 0.0)
        if refresh > 0 and step % refresh == 0 and step < k:          # :326-331
            e, V = _eig(eig, adj, t)
            refreshes += 1
        track.append(e.copy())
    res = {k_: np.array(v) for k_, v in out.items()}
    res["edges"] = res["edges"].reshape(-1, 2).astype(np.int64)
    res["own"] = res["own"].reshape(-1, 2).astype(np.int64)
    final = sp.csr_matrix(adj.astype(np.float64))
    final.sort_indices()
    res.update(track=np.array(track), A=final, refreshes=refreshes, nsel=len(out["edges"]))
    return res


def rob_score(lam0, lam1):
    """(R(2) - R(1)) * 100 / R(1) (:44, :186-188): the gain, not the loss."""
    R0, R1 = log_mean_exp(lam0), log_mean_exp(lam1)
    return (R1 - R0) * 100.0 / R0

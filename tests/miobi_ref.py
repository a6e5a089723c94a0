"""NumPy restatement of the reference's MIOBI edge removal: MIOBIBreakEdge2.m
(unit weights) and MIOBIBreakEdge2_weighted.m, its second ("Update50") loop
with the recomputation period as a parameter; refresh = 0 is its first
("NoUpdate") loop.  Test infrastructure: the eigensolver is a callback, so the
same code runs on numpy.linalg.eigh (tests/test_miobi_host.py) and on the
device's eigs_topk (tests/test_gpu_miobi.py).

The literal index semantics of MIOBIBreakEdge2.m:99-100,

    [naR, naC] = find(isfinite(diffE));  diffE(naR, naC) = 0;

are kept with np.ix_: two index vectors assign the whole cross product rows x
columns, so diffE becomes all zero whenever every row and every column holds a
finite entry -- deltaV is then identically zero and the vectors are only
divided by their norm.  mode "paper" is the update equation (9) describes:
only the diagonal (and, with gap_rel, the near-degenerate pairs) of 1 / (e_c -
e_r) is zeroed.

Where the two files differ this follows the first loop of the weighted one:
deltaA = -A(i, j) read BEFORE the entry is zeroed (MIOBIBreakEdge2_weighted.m:
73-79; its second loop zeroes A(i, j) first, :184-190, and so shifts by 0).
The reference also recomputes after the LAST step when k is a multiple of the
period (:255); that result is never used and is skipped here.
"""
import numpy as np
import scipy.sparse as sp


def eigh_topk(S, t):
    """The eigensolver callback on dense eigh: (lam (t,) descending, V (n, t))."""
    w, U = np.linalg.eigh(S.toarray())
    return w[::-1][:t].copy(), U[:, ::-1][:, :t].copy()


def upper_edges(A):
    """[p, r] = find(triu(A, 1)) (:57, :168): column-major order, i.e. sorted by
    (larger index, smaller index); with the weights."""
    U = sp.triu(sp.csr_matrix(A), 1).tocoo()
    keep = U.data != 0
    p, r, w = U.row[keep].astype(np.int64), U.col[keep].astype(np.int64), U.data[keep].astype(np.float64)
    o = np.lexsort((p, r))
    return p[o], r[o], w[o]


def scores(V, e, p, r, sign=-2.0):
    """:60-68 / :171-179  score = sum(c .* exp(-2 Up .* Ur), 2), c = exp(e)'."""
    return np.sum(np.exp(e)[None, :] * np.exp(sign * V[p] * V[r]), axis=1)


def delta_h(V, i, j, a):
    """deltaH = V' deltaA V for deltaA(i, j) = deltaA(j, i) = -a (:81-86)."""
    u, v = V[i], V[j]
    return -a * (np.outer(u, v) + np.outer(v, u))


def inner_sum(dH, e, mode, gap_rel=0.0):
    """innerSum = deltaH .* diffE with the diagonal of deltaH zeroed (:92-102)."""
    t = len(e)
    dH = dH.copy()
    dH[np.eye(t, dtype=bool)] = 0.0                                   # :92
    with np.errstate(divide="ignore"):
        diffE = 1.0 / (e[None, :] - e[:, None])                       # :95-97  (r, c) = 1 / (e_c - e_r)
    if mode == "reference":
        naC, naR = np.nonzero(np.isfinite(diffE).T)                   # :99  find() runs down the columns
        diffE[np.ix_(naR, naC)] = 0.0                                 # :100 the whole cross product
    else:
        gap = np.abs(e[None, :] - e[:, None])
        diffE[~np.isfinite(diffE) | (gap <= gap_rel * abs(e[0]))] = 0.0
    with np.errstate(invalid="ignore"):
        S = dH * diffE                                                # :102 (0 * Inf = NaN, as MATLAB)
    return S


def update(V, e, i, j, a, mode, gap_rel=0.0, scale=1.0):
    """One step's eigenpair update (:81-142): returns (V_new, e_new, deltaV).
    scale multiplies deltaA (the second-order test)."""
    dH = scale * delta_h(V, i, j, a)
    e_new = e + np.diag(dH)                                           # :88-90
    dV = V @ inner_sum(dH, e, mode, gap_rel)                          # :124-132  deltaV(:, i) = V innerSum(:, i)
    Vn = V + dV                                                       # :134
    Vn = Vn / np.linalg.norm(Vn, axis=0)                              # :136-138
    Vn[:, 0] = np.abs(Vn[:, 0])                                       # :142
    return Vn, e_new, dV


def matrix_of(n, p, r, w, alive, diag=None):
    M = sp.coo_matrix((w[alive], (p[alive], r[alive])), shape=(n, n)).tocsr()
    M = M + M.T
    if diag is not None and np.any(diag):
        M = M + sp.diags(diag)
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def miobi_break_ref(A, k, t, eig, refresh=0, mode="reference", gap_rel=0.0, forced=None):
    """Run k steps.  eig(S, t) -> (lam, V) is called on the current matrix at
    the start and after every refresh-th step but the last.  forced: a
    sequence of 0-based pairs to remove instead of the run's own argmin (the
    run still reports its own).  Returns a dict:
      edges     (nsel, 2) 0-based (larger, smaller) of the pairs removed
      own       (nsel, 2) the run's own argmin at every step, same convention
      score     the removed pair's score;  smin  the run's own minimum
      gap       (second smallest - smallest) / |smallest| (inf with one edge)
      excess    (removed pair's score - smallest) / |smallest|
      alive     whether the forced pair was still an edge
      track     (nsel + 1, t): row s = the eigenvalues that score step s + 1
      dv_max    max |deltaV| of every step
      V, A, refreshes, nsel"""
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    p, r, w = upper_edges(A)
    diag = A.diagonal()
    alive = np.ones(len(p), dtype=bool)
    lookup = {(int(b), int(a)): q for q, (a, b) in enumerate(zip(p, r))}
    e, V = eig(matrix_of(n, p, r, w, alive, diag), t)                  # :47 / :159
    e, V = np.array(e, dtype=np.float64), np.array(V, dtype=np.float64)
    V[:, 0] = np.abs(V[:, 0])                                          # :48
    out = {k_: [] for k_ in ("edges", "own", "score", "smin", "gap", "excess", "alive", "dv_max")}
    track = [e.copy()]
    refreshes = 0
    for step in range(1, int(k) + 1):
        live = np.flatnonzero(alive)
        if len(live) == 0:
            break
        sc = scores(V, e, p[live], r[live])
        o = int(np.argmin(sc))                                         # :71  the first minimum in find() order
        smin = float(sc[o])
        rest = np.delete(sc, o)
        gap = float((rest.min() - smin) / abs(smin)) if len(rest) else np.inf
        q = int(live[o])
        ok = True
        if forced is not None:
            f = (int(max(forced[step - 1])), int(min(forced[step - 1])))
            ok = f in lookup and bool(alive[lookup[f]])
            if not ok:
                out["alive"].append(False)
                break
            q = lookup[f]
        sq = float(sc[np.searchsorted(live, q)])
        out["edges"].append((int(r[q]), int(p[q])))
        out["own"].append((int(r[live[o]]), int(p[live[o]])))
        out["score"].append(sq)
        out["smin"].append(smin)
        out["gap"].append(gap)
        out["excess"].append((sq - smin) / abs(smin))
        out["alive"].append(ok)
        alive[q] = False                                               # :78-79 / :189-190
        V, e, dV = update(V, e, int(p[q]), int(r[q]), float(w[q]), mode, gap_rel)
        out["dv_max"].append(float(np.max(np.abs(dV))) if dV.size else 0.0)
        if refresh > 0 and step % refresh == 0 and step < k and alive.any():   # :255-261
            e, V = eig(matrix_of(n, p, r, w, alive, diag), t)
            e, V = np.array(e, dtype=np.float64), np.array(V, dtype=np.float64)
            V[:, 0] = np.abs(V[:, 0])
            refreshes += 1
        track.append(e.copy())
    res = {k_: np.array(v) for k_, v in out.items()}
    res["edges"] = res["edges"].reshape(-1, 2).astype(np.int64)
    res["own"] = res["own"].reshape(-1, 2).astype(np.int64)
    res.update(track=np.array(track), V=V, A=matrix_of(n, p, r, w, alive, diag), refreshes=refreshes,
               nsel=len(out["edges"]))
    return res


def log_mean_exp(lam):
    """R = log((1 / t) sum(exp(lam))) (:40-42), formed stably."""
    lam = np.asarray(lam, dtype=np.float64)
    return float(np.log(np.sum(np.exp(lam - lam.max()))) + lam.max() - np.log(lam.size))


def rob_score(lam0, lam1):
    """(R(1) - R(2)) * 100 / R(1) (:266-268)."""
    R0, R1 = log_mean_exp(lam0), log_mean_exp(lam1)
    return (R0 - R1) * 100.0 / R0

"""NumPy restatement of the Gauss / Gauss-Radau bracket of exp(A)_ij, i != j
(DESIGN.md §4.2j), on tests/bracket_ref.py.

With z+- = e_i +- e_j and g+- = (z+- / sqrt 2)' exp(A) (z+- / sqrt 2),

    exp(A)_ij = (g+ - g-) / 2,

and each g is a quadratic form of exp: the Lanczos run started at z+- / sqrt 2
(full reorthogonalisation) gives its Gauss rule L and Gauss-Radau rule U with a
node at mu >= lambda_max(A) by bracket_ref.bracket, so

    lo = (L+ - U-) / 2 <= exp(A)_ij <= hi = (U+ - L-) / 2.

The stopping rule of kt_entries_fun_bracket at depth j, in this order: a column
whose own beta_j < 1e-8 is exact (U := L) and frozen at j; flag 2 when a running
column proves mu below lambda_max (lo = hi = NaN); 1 when both columns are
frozen; 0 when lo hi > 0 and 0 <= hi - lo <= rtol min(|lo|, |hi|); 4 when hi -
lo <= ftol (U+ + U-) / 2; 3 at j = it.  Pairs are 0-based and run as (min,
max)."""
import functools
import itertools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

import bracket_ref as br


def lanczos_full_vec(A, v, m):
    """bracket_ref.lanczos_full started at v / ||v||."""
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    V = np.zeros((n, m + 1))
    V[:, 0] = np.asarray(v, dtype=np.float64) / np.linalg.norm(v)
    alpha, beta = [], []
    for k in range(m):
        w = A @ V[:, k]
        a = float(V[:, k] @ w)
        for _ in range(2):
            w -= V[:, :k + 1] @ (V[:, :k + 1].T @ w)
        b = float(np.linalg.norm(w))
        alpha.append(a)
        beta.append(b)
        if b < 1e-8:
            break
        V[:, k + 1] = w / b
    return np.array(alpha), np.array(beta)


def pair_runs(A, i, j, m):
    """The (alpha, beta) records of the + and the - column of pair (i, j)."""
    i, j = min(i, j), max(i, j)
    n = A.shape[0]
    out = []
    for s in (1.0, -1.0):
        v = np.zeros(n)
        v[i], v[j] = 1.0, s
        out.append(lanczos_full_vec(A, v, m))
    return out


def column(run, d, mu):
    """(L, U, kind) of one column at depth d (scaled by exp(-mu)); a run that
    ended before d is taken at its end, where it is exact."""
    alpha, beta = run
    return br.bracket(alpha, beta, min(d, len(alpha)), mu)


def combine(cp, cm, rtol, ftol):
    """(lo, hi, flag) of a pair from its columns' (L, U, kind); flag 3: none of
    the others."""
    (Lp, Up, kp), (Lm, Um, km) = cp, cm
    if kp == 2 or km == 2:
        return float("nan"), float("nan"), 2
    lo, hi = 0.5 * (Lp - Um), 0.5 * (Up - Lm)
    gap = hi - lo
    if kp == 1 and km == 1:
        return lo, hi, 1
    if lo * hi > 0.0 and 0.0 <= gap <= rtol * min(abs(lo), abs(hi)):
        return lo, hi, 0
    if gap <= ftol * (0.5 * (Up + Um)):
        return lo, hi, 4
    return lo, hi, 3


def pair_at(runs, dp, dm, mu, rtol=1e-10, ftol=1e-12):
    """(lo, hi, flag), unscaled, of a pair whose columns are cut at dp and dm:
    what kt_entries_fun_bracket forms on the host from its col_iter."""
    s = float(np.exp(mu))
    cp, cm = column(runs[0], dp, mu), column(runs[1], dm, mu)
    return combine((cp[0] * s, cp[1] * s, cp[2]), (cm[0] * s, cm[1] * s, cm[2]), rtol, ftol)


def pair_run(A, i, j, mu, rtol=1e-10, ftol=1e-12, it=None, runs=None):
    """(lo, hi, iter, flag, (depth+, depth-)), unscaled, by the stopping rule of
    kt_entries_fun_bracket."""
    n = A.shape[0]
    if it is None or it <= 0:
        it = min(100, n)
    if runs is None:
        runs = pair_runs(A, i, j, it)
    frozen = [0, 0]
    for d in range(1, it + 1):
        for c in (0, 1):
            if not frozen[c] and column(runs[c], d, mu)[2] == 1:
                frozen[c] = d
        dp, dm = frozen[0] or d, frozen[1] or d
        lo, hi, flag = pair_at(runs, dp, dm, mu, rtol, ftol)
        if flag != 3 or d == it:
            return lo, hi, max(dp, dm), flag, (dp, dm)
    raise AssertionError("unreachable")


def exp_dense(A):
    """exp(A) and eigvalsh(A) by dense eigh."""
    w, V = np.linalg.eigh(sp.csr_matrix(A).toarray())
    return (V * np.exp(w)) @ V.T, w


def pair_set(A):
    """The tests' pairs of a graph, 0-based, as {kind: [(i, j), ...]}: "hub
    edges", two edges at each of the 4 highest-degree nodes (to their two
    highest-degree neighbours); "hubs", the 6 pairs among those nodes; "leaf
    edges", the first 4 leaves with their neighbours; "twins", the first two
    leaves that hang on one node (anaheim has none); "distant", three pairs:
    in a graph of several components its first isolated node (else the first
    node of the second largest component) with three hubs, an entry that is
    exactly 0; in a connected one the first hub with the three nodes farthest
    from it in hops (anaheim: below 2e-10 of (E_ii + E_jj) / 2, rome: below
    1e-15; oregon_A0 has diameter 6 and no entry below 2e-4 of that scale,
    which these reach).  Ties in node order."""
    M = sp.csr_matrix(A)
    n = M.shape[0]
    deg = np.diff(M.indptr)
    hubs = [int(h) for h in np.argsort(-deg, kind="stable")[:4]]
    out = {"hub edges": [], "hubs": list(itertools.combinations(hubs, 2)), "leaf edges": [], "twins": [],
           "distant": []}
    for h in hubs:
        nb = M.indices[M.indptr[h]:M.indptr[h + 1]]
        nb = nb[nb != h]
        for v in nb[np.argsort(-deg[nb], kind="stable")[:2]]:
            out["hub edges"].append((h, int(v)))
    leaves = np.flatnonzero(deg == 1)
    parent = {int(l): int(M.indices[M.indptr[l]]) for l in leaves}
    out["leaf edges"] = [(int(l), parent[int(l)]) for l in leaves[:4]]
    seen = {}
    for l in leaves:
        p = parent[int(l)]
        if p in seen:
            out["twins"] = [(seen[p], int(l))]
            break
        seen[p] = int(l)
    ncomp, lab = csgraph.connected_components(M, directed=False)
    if ncomp > 1:
        sizes = np.bincount(lab)
        other = [c for c in np.argsort(-sizes, kind="stable") if c != lab[hubs[0]]][0]
        iso = np.flatnonzero(deg == 0)
        far = int(iso[0]) if iso.size else int(np.flatnonzero(lab == other)[0])
        out["distant"] = [(h, far) for h in hubs[:3] if lab[h] != lab[far]]
    if len(out["distant"]) < 3:
        dist = csgraph.shortest_path(M, unweighted=True, indices=hubs[0])
        dist[~np.isfinite(dist)] = -1
        for v in np.argsort(-dist, kind="stable")[:3 - len(out["distant"])]:
            out["distant"].append((hubs[0], int(v)))
    return out


def flat(pairs):
    return [p for kind in ("hub edges", "hubs", "leaf edges", "twins", "distant") for p in pairs[kind]]


@functools.lru_cache(maxsize=None)
def graph_case(g, depth=40):
    """What the CPU and the GPU tests share of golden graph g, computed once:
    A, exp(A) and eigvalsh(A) by dense eigh, mu = lambda_upper from the vector
    of ones, the pair set and every pair's two Lanczos runs of `depth` steps."""
    from conftest import load_graph
    import krylov_robustness_amd as kra
    A = load_graph(g)
    E, w = exp_dense(A)
    pairs = pair_set(A)
    return {"A": A, "E": E, "w": w, "mu": kra.lambda_upper(A, v=np.ones(A.shape[0])), "pairs": pairs,
            "runs": {p: pair_runs(A, p[0], p[1], depth) for p in flat(pairs)}}


def scale_of(E, i, j):
    """(exp(A)_ii + exp(A)_jj) / 2: the unit of a pair bracket's rounding errors."""
    return 0.5 * (E[i, i] + E[j, j])


def violations(runs, mu, exact, scale, depths=range(1, 41)):
    """The largest violation of lo <= exact <= hi and of the bounds'
    monotonicity over the depths of one pair, both columns at one depth, in
    units of `scale`."""
    worst, plo, phi = 0.0, -np.inf, np.inf
    for d in depths:
        lo, hi, flag = pair_at(runs, d, d, mu)
        worst = max(worst, (lo - exact) / scale, (exact - hi) / scale, (plo - lo) / scale, (hi - phi) / scale)
        plo, phi = lo, hi
    return worst

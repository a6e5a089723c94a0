"""NumPy restatement of the node-removal trace update.

Removing node i from symmetric A -- row and column i zeroed, the node left as
an isolated vertex -- is the rank-2 update A + U B U' with U = [e_i, a_i].  Its
block Krylov space is the single-vector space K_{j+1}(A, e_i), and in the
Lanczos basis of e_i the update is minus the first row and column of T, so with
T_j the j x j Lanczos tridiagonal started at e_i

    X_j = f(0) + sum f(eig(T_j[2:j, 2:j])) - sum f(eig(T_j))  ->  tr f(A_{-i}) - tr f(A).

Plain three-term Lanczos without reorthogonalisation; the stop is
trace_fun_update.m:104-124 (X_1, X_2 stored; for j > 2 stop when
|X_j - X_{j-2}| < tol; lucky when beta_j < 1e-8); n <= 130 is dense.  Nodes are
0-based here."""
import numpy as np
import scipy.sparse as sp

FUNS = {"exp": np.exp, "sinh": np.sinh, "cosh": np.cosh, "sin": np.sin, "cos": np.cos, "sqrt": np.sqrt}


def trace_diff(d1, d2, fun):
    """trace_fun_update.m:85-89 on two ascending spectra of equal length."""
    if fun == "exp":
        return float(np.sum(np.exp(d1) * (1.0 - np.exp(d2 - d1))))
    f = FUNS[fun]
    return float(np.sum(f(d1) - f(d2)))


def tridiag(alpha, off):
    j = len(alpha)
    T = np.diag(np.asarray(alpha, dtype=np.float64))
    if j > 1:
        T += np.diag(off[:j - 1], 1) + np.diag(off[:j - 1], -1)
    return T


def x_of_tridiag(alpha, off, fun="exp"):
    """X_j from the tridiagonal (alpha[0..j-1], off[0..j-2])."""
    j = len(alpha)
    d2 = np.linalg.eigvalsh(tridiag(alpha, off))
    inner = np.linalg.eigvalsh(tridiag(alpha[1:], off[1:])) if j > 1 else np.zeros(0)
    d1 = np.sort(np.concatenate([[0.0], inner]))
    return trace_diff(d1, d2, fun)


def remove_node(A, i):
    """A with row and column i zeroed (CSR, explicit zeros dropped)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    keep = np.ones(A.shape[0])
    keep[i] = 0.0
    K = sp.diags(keep)
    M = (K @ A @ K).tocsr()
    M.eliminate_zeros()
    return M


def exact_update(A, i, fun="exp", w_full=None):
    """tr f(A_{-i}) - tr f(A) by dense eigvalsh (w_full: eigvalsh(A), reusable)."""
    w2 = np.linalg.eigvalsh(A.toarray()) if w_full is None else w_full
    w1 = np.linalg.eigvalsh(remove_node(A, i).toarray())
    return trace_diff(w1, w2, fun)


def node_update(A, i, tol=1e-12, it=None, fun="exp", keep=False):
    """(Xm, iter, lucky[, alpha, off, hist]) for node i (0-based)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    if it is None or it <= 0:
        it = min(100, n)
    if n <= 130:
        out = (exact_update(A, i, fun), 0, 0)
        return out + ([], [], []) if keep else out
    v = np.zeros(n)
    v[i] = 1.0
    vprev = np.zeros(n)
    beta = 0.0
    alpha, off, hist = [], [], []
    xstop = [0.0, 0.0]
    xm, lucky = 0.0, 0
    for j in range(1, it + 1):
        w = A @ v - beta * vprev
        a = float(v @ w)
        w -= a * v
        beta = float(np.linalg.norm(w))
        alpha.append(a)
        xm = x_of_tridiag(np.array(alpha), np.array(off), fun)
        lucky = int(beta < 1e-8)
        stop = False
        err = np.inf
        if j <= 2:
            xstop[j - 1] = xm
        else:
            err = abs(xm - xstop[0])
            if err < tol:
                stop = True
            else:
                xstop[0], xstop[1] = xstop[1], xm
        hist.append((j, err, xm))
        if stop or lucky or j == it:
            out = (xm, j, lucky)
            return out + (np.array(alpha), np.array(off), hist) if keep else out
        off.append(beta)
        vprev, v = v, w / beta
    raise AssertionError("unreachable")


def lanczos_tridiag(A, i, m):
    """alpha (m), off (m - 1) of the Lanczos run started at e_i (no stop test;
    a breakdown ends it early)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    v = np.zeros(n)
    v[i] = 1.0
    vprev = np.zeros(n)
    beta = 0.0
    alpha, off = [], []
    for _ in range(m):
        w = A @ v - beta * vprev
        a = float(v @ w)
        w -= a * v
        alpha.append(a)
        beta = float(np.linalg.norm(w))
        if beta < 1e-8 or len(alpha) == m:
            break
        off.append(beta)
        vprev, v = v, w / beta
    return np.array(alpha), np.array(off)


def node_set(A):
    """The tests' nodes of a graph: the four highest degrees, two leaves and,
    where there is one, an isolated node (0-based; ties in node order)."""
    deg = np.diff(sp.csr_matrix(A).indptr)
    order = np.argsort(-deg, kind="stable")
    nodes = [int(i) for i in order[:4]] + [int(i) for i in np.flatnonzero(deg == 1)[:2]]
    iso = np.flatnonzero(deg == 0)
    return nodes, (int(iso[0]) if iso.size else None)


def diag_copy(A, i, value=0.75):
    """A with a diagonal entry at node i."""
    A = sp.lil_matrix(A, dtype=np.float64)
    A[i, i] = value
    return sp.csr_matrix(A)


def krylov_break_node_ref(A, k, nodes, tol=1e-12, it=None, fun="exp", forced=None):
    """The greedy loop: per step score every remaining candidate, take the
    smallest Xm (the first on ties; forced[s] instead when given), zero its row
    and column, drop it.  Returns (selected, xm of each step's candidates as
    {node: xm} dicts, rob, A_new)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    cand = [int(c) for c in nodes]
    sel, steps, rob = [], [], 0.0
    for s in range(k):
        if not cand:
            break
        xm = [node_update(A, c, tol, it, fun)[0] for c in cand]
        steps.append(list(zip(cand, xm)))
        b = int(np.argmin(xm)) if forced is None else cand.index(int(forced[s]))
        sel.append(cand[b])
        rob += xm[b]
        A = remove_node(A, cand[b])
        del cand[b]
    return sel, steps, rob, A

"""NumPy restatement of the Gauss / Gauss-Radau bracket of exp(A)_ii (DESIGN.md
§4.2i; Golub & Meurant, Matrices, Moments and Quadrature).

Lanczos from e_i with full reorthogonalisation gives T_j (alpha_1..alpha_j,
beta_1..beta_{j-1}) and beta_j.  With mu >= lambda_max(A):

    L_j = sum z_k^2 exp(theta_k)        over the eigenpairs of T_j        (Gauss, lower)
    U_j = sum zh_k^2 exp(thetah_k)      over the eigenpairs of That_{j+1} (Gauss-Radau, upper)

That_{j+1} = T_j bordered by beta_j with last diagonal entry mu + beta_j^2 / d_j,
d the pivots of T_j - mu I (d_1 = alpha_1 - mu, d_k = alpha_k - mu -
beta_{k-1}^2 / d_{k-1}).  Both by numpy.linalg.eigh, both scaled by exp(-mu).
Flags: 0 the gap, 1 beta_j < 1e-8 (hi = lo), 2 mu proved below lambda_max (hi =
NaN), 3 the depth cap.  Nodes are 0-based here."""
import numpy as np
import scipy.sparse as sp


def lanczos_full(A, i, m):
    """alpha (k), beta (k) of the run started at e_i, k <= m: beta[k - 1] is
    beta_k, the off-diagonal after row k (full reorthogonalisation, twice; a
    beta < 1e-8 ends the run)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    V = np.zeros((n, m + 1))
    V[i, 0] = 1.0
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


def tridiag(alpha, off):
    j = len(alpha)
    T = np.diag(np.asarray(alpha, dtype=np.float64))
    if j > 1:
        T += np.diag(off[:j - 1], 1) + np.diag(off[:j - 1], -1)
    return T


def scaled_sum(alpha, off, mu):
    """sum z_k^2 exp(theta_k - mu) and theta_max of the tridiagonal."""
    w, Z = np.linalg.eigh(tridiag(alpha, off))
    return float(np.sum(Z[0] ** 2 * np.exp(w - mu))), float(w[-1])


def bracket(alpha, beta, j, mu):
    """(lo, hi, flag) at depth j, scaled by exp(-mu); flag 0, 1 or 2."""
    al, off, bj = np.asarray(alpha[:j], dtype=np.float64), np.asarray(beta[:j - 1], dtype=np.float64), float(beta[j - 1])
    lo, tmax = scaled_sum(al, off, mu)
    if bj < 1e-8:
        return lo, lo, 1
    d = al[0] - mu
    bad = not d < 0.0
    for k in range(1, j):
        d = al[k] - mu - off[k - 1] ** 2 / d
        bad = bad or not d < 0.0
    if bad or tmax > mu:
        return lo, float("nan"), 2
    hi, _ = scaled_sum(np.concatenate([al, [mu + bj * bj / d]]), np.concatenate([off, [bj]]), mu)
    return lo, hi, 0


def bracket_run(A, i, mu, rtol=1e-10, it=None):
    """(lo, hi, iter, flag), unscaled, by the stopping rule of kt_diag_fun_bracket."""
    n = A.shape[0]
    if it is None or it <= 0:
        it = min(100, n)
    alpha, beta = lanczos_full(A, i, it)
    scale = float(np.exp(mu))
    for j in range(1, len(alpha) + 1):
        lo, hi, flag = bracket(alpha, beta, j, mu)
        if flag == 0 and not hi - lo <= rtol * lo:
            flag = 3 if j == it else -1
        if flag >= 0:
            return lo * scale, hi * scale, j, flag
    raise AssertionError("unreachable")


def exp_diag(A):
    """diag(exp(A)) and eigvalsh(A) by dense eigh."""
    w, V = np.linalg.eigh(sp.csr_matrix(A).toarray())
    return (V * V) @ np.exp(w), w


def node_set(A):
    """The tests' nodes of a graph: the highest-degree node, a leaf and, where
    there is one, an isolated node (0-based; ties in node order), as
    nodes_ref.node_set picks them."""
    deg = np.diff(sp.csr_matrix(A).indptr)
    nodes = [int(np.argsort(-deg, kind="stable")[0]), int(np.flatnonzero(deg == 1)[0])]
    iso = np.flatnonzero(deg == 0)
    if iso.size:
        nodes.append(int(iso[0]))
    return nodes


def wide_node_set(A, k=8):
    """k hubs, k leaves and the isolated node if any (0-based)."""
    deg = np.diff(sp.csr_matrix(A).indptr)
    nodes = [int(i) for i in np.argsort(-deg, kind="stable")[:k]] + [int(i) for i in np.flatnonzero(deg == 1)[:k]]
    iso = np.flatnonzero(deg == 0)
    return nodes + ([int(iso[0])] if iso.size else [])


def violations(alpha, beta, mu, exact, rule=bracket, depths=None):
    """The largest relative violation of lo <= exact <= hi and of the bounds'
    monotonicity over the depths 1..len(alpha) of one run (exact unscaled)."""
    e = exact * np.exp(-mu)
    worst, plo, phi = 0.0, -np.inf, np.inf
    for j in depths or range(1, len(alpha) + 1):
        lo, hi, flag = rule(alpha, beta, j, mu)
        worst = max(worst, (lo - e) / e, (plo - lo) / e)
        if flag != 2:
            worst = max(worst, (e - hi) / e, (hi - phi) / e)
            phi = hi
        plo = lo
    return worst


def lambda_upper_ref(A):
    """max row sum of |A|: an upper bound on lambda_max whatever the signs."""
    return float(abs(sp.csr_matrix(A)).sum(axis=1).max())

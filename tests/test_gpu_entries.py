"""GPU tests of kt_entries_fun, the deflated stochastic estimator of entries of
f(A) on a pair list, against the numpy oracle on the same counter-RNG probes.

Expected values follow the estimator's definition literally: with
Z = ko.rademacher(n, probes, seed), Pi = I - Q Q', Y = ko.lanczos_fmv(A, Pi Z),
Yt = Pi Y and pair e = (i, j),
    t_p[e] = (Z[i, p] Yt[j, p] + Z[j, p] Yt[i, p]) / 2,
    esum = sum_p t_p,  esum2 = sum_p t_p^2,  q_p = z'_p' f(A) z'_p,
    e0[e] = sum_c (Q_ic G_jc + G_ic Q_jc) - (sum_c (QH)_ic Q_jc + (QH)_jc Q_ic) / 2,
    G = ko.lanczos_fmv(A, Q), H = Q'G.

Tolerances are test_gpu_diag.py's: a per-probe error delta = 1e-10 max|Yt| in
Yt carries into t unchanged (|z| = 1 and t is an average of two such terms),
so esum: rtol 1e-8, atol 1e-10 N max|Yt|; esum2: rtol 1e-8, atol 2e-10 N
max|Yt|^2; e0: rtol 1e-8, atol 4e-10 k max|G|; sum_q, sum_q2: 1e-8 relative."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph
from oracle import krylov_oracle as ko

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


@functools.lru_cache(maxsize=None)
def _eig(name):
    w, V = np.linalg.eigh(load_graph(name).toarray())
    return w, V


@functools.lru_cache(maxsize=None)
def _defl(name, k):
    """k = 1: the exact leading eigenvector; k = 4: the four leading
    eigenvectors perturbed by 1e-3 Gaussian noise and re-orthonormalised."""
    if k == 0:
        return None
    _, V = _eig(name)
    Q = V[:, ::-1][:, :k].copy()
    if k > 1:
        Q = Q + 1e-3 * np.random.default_rng(11).normal(size=Q.shape)
        Q, _ = np.linalg.qr(Q)
    return np.asfortranarray(Q)


def _tril(A):
    """find(tril(A, -1)), 0-based (npairs, 2) with i > j, column-major order."""
    L = sp.tril(sp.csc_matrix(A), -1).tocsc()
    L.sort_indices()
    J = np.repeat(np.arange(L.shape[1], dtype=np.int64), np.diff(L.indptr))
    return np.stack([L.indices.astype(np.int64), J], axis=1)


def _blocks(A, N, off, m, seed, fun, Q):
    """The pair-independent part of the oracle: Z, Yt = Pi f(A) Pi Z, q, Q, G, H."""
    n = A.shape[0]
    Z = ko.rademacher(n, range(off, off + N), seed)
    Zp = Z if Q is None else Z - Q @ (Q.T @ Z)
    Y = ko.lanczos_fmv(A, Zp, m, fun)
    Yt = Y if Q is None else Y - Q @ (Q.T @ Y)
    q = np.array([ko.lanczos_quadform(A, Zp[:, p], m, fun) for p in range(N)])
    out = {"Z": Z, "Yt": Yt, "q": q, "scale": np.abs(Yt).max(), "Q": Q, "gmax": 0.0}
    if Q is not None:
        out["G"] = ko.lanczos_fmv(A, Q, m, fun)
        out["H"] = Q.T @ out["G"]
        out["gmax"] = np.abs(out["G"]).max()
    return out


@functools.lru_cache(maxsize=None)
def _blocks_named(name, N, off, m, seed, fun, k):
    return _blocks(load_graph(name), N, off, m, seed, fun, _defl(name, k))


def _oracle(b, pairs):
    I, J = pairs[:, 0], pairs[:, 1]
    Z, Yt = b["Z"], b["Yt"]
    T = 0.5 * (Z[I] * Yt[J] + Z[J] * Yt[I])
    o = dict(b, T=T, esum=T.sum(axis=1), esum2=(T * T).sum(axis=1), e0=np.zeros(len(I)))
    if b["Q"] is not None:
        Q, G = b["Q"], b["G"]
        QH = Q @ b["H"]
        o["e0"] = ((Q[I] * G[J]).sum(axis=1) + (G[I] * Q[J]).sum(axis=1)
                   - 0.5 * ((QH[I] * Q[J]).sum(axis=1) + (QH[J] * Q[I]).sum(axis=1)))
    return o


def _check(r, o, N, k=0):
    print("max|esum err|", np.abs(r.esum - o["esum"]).max(), "atol", 1e-10 * N * o["scale"],
          "max|esum2 err|", np.abs(r.esum2 - o["esum2"]).max(), "max|e0 err|", np.abs(r.e0 - o["e0"]).max())
    np.testing.assert_allclose(r.esum, o["esum"], rtol=1e-8, atol=1e-10 * N * o["scale"])
    np.testing.assert_allclose(r.esum2, o["esum2"], rtol=1e-8, atol=2e-10 * N * o["scale"] ** 2)
    assert r.sum_q == pytest.approx(o["q"].sum(), rel=1e-8)
    assert r.sum_q2 == pytest.approx((o["q"] ** 2).sum(), rel=1e-8)
    if k:
        np.testing.assert_allclose(r.e0, o["e0"], rtol=1e-8, atol=4e-10 * k * o["gmax"])
    else:
        assert not r.e0.any()
    for a in (r.esum, r.esum2, r.e0, r.mean, r.stderr):
        assert np.isfinite(a).all()


def _mixed_pairs(A):
    """All tril edges, 64 diagonal pairs, 64 missing pairs, one pair twice,
    one pair in both orientations; the slots of the last two groups."""
    n = A.shape[0]
    rng = np.random.default_rng(5)
    E = _tril(A)
    d = rng.choice(n, 64, replace=False)
    miss = []
    D = sp.csr_matrix(A)
    while len(miss) < 64:
        i, j = rng.integers(0, n, 2)
        if i != j and D[i, j] == 0:
            miss.append((i, j))
    rep = E[len(E) // 2]
    P = np.vstack([E, np.stack([d, d], axis=1), np.array(miss, dtype=np.int64), rep[None], rep[None],
                   E[7][None], E[7][::-1][None]]).astype(np.int64)
    return P, len(P) - 4


def _bits_of_the_repeats(r, s):
    for f in ("esum", "esum2", "e0"):
        a = getattr(r, f)
        assert a[s] == a[s + 1], f
        assert a[s + 2] == a[s + 3], f


@pytest.mark.parametrize("name", ["anaheim", "oregon_A0", "india"])
def test_parity_without_deflation(kra, gpu_ctx, name):
    """N = 16 probes in one 16-wide sweep, m = 30: unit weights (anaheim), a
    206-entry row (oregon_A0), fp64 weights (india).  Edges, diagonal pairs,
    missing pairs; a repeated pair and the two orientations of a pair are
    equal bit for bit."""
    A = load_graph(name)
    P, s = _mixed_pairs(A)
    r = kra.entries_fun(kra.DeviceMatrix(A, gpu_ctx), P, 16, m=30, seed=3, block=16, ctx=gpu_ctx)
    _check(r, _oracle(_blocks_named(name, 16, 0, 30, 3, "exp", 0), P), 16)
    _bits_of_the_repeats(r, s)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("name", ["oregon_A0", "india"])
def test_parity_with_deflation(kra, gpu_ctx, name, k):
    """k = 1 with the exact leading eigenvector, k = 4 with an inexact
    orthonormal Q; e0 is checked.  On oregon_A0 max|y| is 3.6e7 before the
    output projection and 3.5e5 after it: a missing projection fails this."""
    A = load_graph(name)
    P, s = _mixed_pairs(A)
    r = kra.entries_fun(kra.DeviceMatrix(A, gpu_ctx), P, 16, m=30, seed=3, block=16, deflate=_defl(name, k),
                        ctx=gpu_ctx)
    _check(r, _oracle(_blocks_named(name, 16, 0, 30, 3, "exp", k), P), 16, k=k)
    _bits_of_the_repeats(r, s)


def test_diagonal_pairs_are_diag_fun(kra, gpu_ctx):
    """Pairs (i, i) for every i on oregon_A0, k = 1, 40 probes from offset 5,
    m = 12: the sums are diag_fun's from the same arguments (1e-12 of their
    largest entry, the tolerance test_gpu_diag.py uses for the same sums in
    another order), e0 is d0, sum_q agrees to 1e-12 relative."""
    A = load_graph("oregon_A0")
    n = A.shape[0]
    D = kra.DeviceMatrix(A, gpu_ctx)
    Q = _defl("oregon_A0", 1)
    kw = dict(m=12, seed=5, probe_offset=5, block=16, deflate=Q, ctx=gpu_ctx)
    d = kra.diag_fun(D, 40, **kw)
    i = np.arange(n, dtype=np.int64)
    r = kra.entries_fun(D, np.stack([i, i], axis=1), 40, **kw)
    print("max|esum - dsum|", np.abs(r.esum - d.dsum).max(), "max|dsum|", np.abs(d.dsum).max())
    np.testing.assert_allclose(r.esum, d.dsum, rtol=0, atol=1e-12 * np.abs(d.dsum).max())
    np.testing.assert_allclose(r.esum2, d.dsum2, rtol=0, atol=1e-12 * np.abs(d.dsum2).max())
    np.testing.assert_allclose(r.e0, d.d0, rtol=0, atol=1e-12 * np.abs(d.d0).max())
    assert r.sum_q == pytest.approx(d.sum_q, rel=1e-12)


def test_ranges_widths_and_bit_identity(kra, gpu_ctx, monkeypatch):
    """oregon_A0, m = 12, seed 5.  40 probes from offset 5 at block 16 (sweeps
    of 16, 16 and a remainder of 8) match the oracle; [5, 21) + [21, 45) add up
    to it; blocks 1, 2 and 4 with 5 probes, k = 1 and k = 0, match the oracle;
    two identical calls, and a call on one sweep lane, are bit-identical."""
    A = load_graph("oregon_A0")
    D = kra.DeviceMatrix(A, gpu_ctx)
    Q = _defl("oregon_A0", 1)
    P, _ = _mixed_pairs(A)
    call = lambda N, off, blk, q=Q: kra.entries_fun(D, P, N, m=12, seed=5, probe_offset=off, block=blk, deflate=q,
                                                    ctx=gpu_ctx)
    full = call(40, 5, 16)
    _check(full, _oracle(_blocks_named("oregon_A0", 40, 5, 12, 5, "exp", 1), P), 40, k=1)
    a, b = call(16, 5, 16), call(24, 21, 16)
    np.testing.assert_allclose(a.esum + b.esum, full.esum, rtol=0, atol=1e-12 * np.abs(full.esum).max())
    np.testing.assert_allclose(a.esum2 + b.esum2, full.esum2, rtol=0, atol=1e-12 * np.abs(full.esum2).max())
    assert a.sum_q + b.sum_q == pytest.approx(full.sum_q, rel=1e-12)
    for blk in (1, 2, 4):
        for q, k in ((Q, 1), (None, 0)):
            _check(call(5, 0, blk, q), _oracle(_blocks_named("oregon_A0", 5, 0, 12, 5, "exp", k), P), 5, k=k)
    again = call(40, 5, 16)
    monkeypatch.setenv("KT_SLQ_LANES", "1")
    one_lane = call(40, 5, 16)
    monkeypatch.delenv("KT_SLQ_LANES")
    for other in (again, one_lane):
        for f in ("esum", "esum2", "e0"):
            assert np.array_equal(getattr(full, f), getattr(other, f)), f
        assert (full.sum_q, full.sum_q2) == (other.sum_q, other.sum_q2)


def test_lucky_breakdown(kra, gpu_ctx):
    """32 disjoint edges: every Krylov space has dimension 2, every column
    breaks down at step 2 of 30.  exp(A) = cosh(1) I + sinh(1) A, so with
    y = cosh(1) z + sinh(1) A z the terms are exactly (z_i y_j + z_j y_i) / 2:
    16 sinh 1 + cosh 1 sum_p z_p[i] z_p[i^1] on an edge, cosh 1 sum_p z_p[i]
    z_p[j] + sinh 1 (...) across components."""
    n = 64
    i = np.arange(n)
    A = sp.csr_matrix((np.ones(n), (i, i ^ 1)), shape=(n, n))
    P = np.vstack([np.stack([i, i ^ 1], axis=1), np.stack([i, (i + 2) % n], axis=1), np.stack([i, i], axis=1)])
    r = kra.entries_fun(kra.DeviceMatrix(A, gpu_ctx), P, 16, m=30, seed=2, ctx=gpu_ctx)
    Z = ko.rademacher(n, range(16), 2)
    Y = np.cosh(1.0) * Z + np.sinh(1.0) * (A @ Z)
    T = 0.5 * (Z[P[:, 0]] * Y[P[:, 1]] + Z[P[:, 1]] * Y[P[:, 0]])
    np.testing.assert_allclose(r.esum, T.sum(axis=1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r.esum[:n], 16 * np.sinh(1.0) + np.cosh(1.0) * (Z * Z[i ^ 1]).sum(axis=1), rtol=0,
                               atol=1e-12)
    np.testing.assert_allclose(r.esum2, (T * T).sum(axis=1), rtol=0, atol=1e-12)
    for a in (r.esum, r.esum2, r.e0, r.mean, r.stderr, np.array([r.sum_q, r.sum_q2])):
        assert np.isfinite(a).all()


def test_larger_n_grid_stride_and_permutation(kra, gpu_ctx):
    """n = 50,000 with all 250k edges as pairs (several workgroups, the
    grid-stride loop over pairs, the inverse permutation), m = 10, k = 1 with
    the device's leading eigenvector passed as Q."""
    from krylov_robustness_amd import graphs
    A = graphs.erdos_renyi(50_000, 250_000, seed=1)
    D = kra.DeviceMatrix(A, gpu_ctx)
    _, u = kra.eigs_leading(D, ctx=gpu_ctx)
    Q = np.asfortranarray(u[:, None])
    P = _tril(A)
    r = kra.entries_fun(D, P, 16, m=10, seed=1, deflate=Q, ctx=gpu_ctx)
    _check(r, _oracle(_blocks(A, 16, 0, 10, 1, "exp", Q), P), 16, k=1)


@pytest.mark.parametrize("name,deflate", [("oregon_A0", 1), ("rome", None)])
def test_statistics(kra, gpu_ctx, name, deflate):
    """256 probes, seed 7, all tril edges.  With E = exp(A), R = Pi E Pi and
    i != j the exact variance of the estimate is
        sigma_ij^2 = ((R_ii + R_jj)^2 + sum_{k != i, j} (R_ik^2 + R_jk^2)) / 4 / 256
    (the cross terms are distinct Rademacher products, so uncorrelated).
    Every edge is within 6 sigma and the reported stderr within [0.7, 1.4]
    sigma, the bounds of test_subgraph_centrality_estimate (the numpy
    restatement: worst 3.53 sigma and [0.87, 1.10] on oregon_A0 with k = 1,
    3.54 sigma and [0.81, 1.15] on rome with k = 0)."""
    A = load_graph(name)
    n = A.shape[0]
    D = kra.DeviceMatrix(A, gpu_ctx)
    w, V = _eig(name)
    E = (V * np.exp(w)) @ V.T
    R = E
    if deflate:
        _, u = kra.eigs_leading(D, ctx=gpu_ctx)
        Pi = np.eye(n) - np.outer(u, u)
        R = Pi @ E @ Pi
    P = _tril(A)
    I, J = P[:, 0], P[:, 1]
    rows = (R * R).sum(axis=1)
    dg = np.diag(R)
    cross = rows[I] - dg[I] ** 2 - R[I, J] ** 2 + rows[J] - dg[J] ** 2 - R[J, I] ** 2
    sigma = np.sqrt(0.25 * ((dg[I] + dg[J]) ** 2 + cross) / 256)
    r = kra.entries_fun(D, P, 256, seed=7, deflate=deflate, ctx=gpu_ctx)
    z = np.abs(r.mean - E[I, J]) / sigma
    ratio = r.stderr / sigma
    print("worst |err| / sigma", z.max(), "stderr / sigma", ratio.min(), ratio.max(),
          "median rel err", np.median(np.abs(r.mean - E[I, J]) / E[I, J]))
    assert (z <= 6.0).all(), z.max()
    assert (ratio >= 0.7).all() and (ratio <= 1.4).all(), (ratio.min(), ratio.max())


def test_ranking_on_rome(kra, gpu_ctx):
    """find_top_edges_fun(rome, 250, 256 probes, no deflation, seed 7): the
    overlap with the exact top 250 edges by exp(A)_ij is at least the oracle
    restatement's (157 here; device and oracle values differ at the 1e-10
    level, so only near-ties at the cut can swap: 5 allowed) and strictly above
    that of the centrality product ranking find_top_edges(A, |u|, 250, "mult")
    (36 here).  Rows are 1-based with i > j."""
    from krylov_robustness_amd.greedy import _stable_head
    A = load_graph("rome")
    w, V = _eig("rome")
    E = (V * np.exp(w)) @ V.T
    P = _tril(A)
    exact = P[_stable_head(-E[P[:, 0], P[:, 1]], 250)]
    as_set = lambda T: {(int(a), int(b)) for a, b in T}
    o = _oracle(_blocks_named("rome", 256, 0, 30, 7, "exp", 0), P)
    ov_oracle = len(as_set(P[_stable_head(-o["esum"] / 256, 250)]) & as_set(exact))
    top = kra.find_top_edges_fun(kra.DeviceMatrix(A, gpu_ctx), 250, nprobes=256, deflate=None, seed=7, ctx=gpu_ctx)
    assert top.shape == (250, 2) and (top[:, 0] > top[:, 1]).all() and top.min() >= 1
    ov = len(as_set(top - 1) & as_set(exact))
    mult = kra.find_top_edges(A, np.abs(V[:, -1]), 250, "mult")
    ov_mult = len(as_set(mult - 1) & as_set(exact))
    print("overlap: device", ov, "oracle", ov_oracle, "c_i c_j", ov_mult)
    assert ov >= ov_oracle - 5
    assert ov > ov_mult


def test_greedy_krylov_takes_a_ranking(kra, gpu_ctx):
    """greedy_krylov(top=) with the ranking the default call computes, on india
    with the config-5 arguments at k = 5: the same edges, variation and
    exported matrix."""
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "config5_values.json")) as f:
        c5 = json.load(f)
    A = load_graph("india")
    c = np.array(c5["centrality"])
    k = 5
    args = (k, c5["Q"], c, c5["order"], c5["tol"], c5["it"], np.inf, 0, c5["miobi"])
    e1, r1, D1 = kra.greedy_krylov(kra.DeviceMatrix(A, gpu_ctx), *args, ctx=gpu_ctx)
    top = kra.find_top_edges(sp.csc_matrix(A), c, c5["Q"] + k, c5["order"])
    e2, r2, D2 = kra.greedy_krylov(kra.DeviceMatrix(A, gpu_ctx), *args, ctx=gpu_ctx, top=top)
    assert len(e1) == k
    np.testing.assert_array_equal(e1, e2)
    assert r1 == r2
    assert (D1.to_scipy() != D2.to_scipy()).nnz == 0


def _raw(D, npairs, ei, ej, block=0, kdef=0, Q=None):
    """kt_entries_fun called directly: (status, message)."""
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    ej = np.ascontiguousarray(ej, dtype=np.int64)
    out = np.zeros(max(len(ei), 1))
    i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    st = lib.kt_entries_fun(D.handle, 0, 30, 3, 0, 16, block, kdef, None if Q is None else Q.ctypes.data_as(dp),
                            npairs, ei.ctypes.data_as(i64p), ej.ctypes.data_as(i64p), out.ctypes.data_as(dp), None,
                            None, None, None)
    msg = lib.kt_last_error()
    return st, (msg.decode() if msg else "")


def test_other_function_and_argument_errors(kra, gpu_ctx):
    """fun = cosh matches the oracle; npairs = 0, an index equal to n, a
    negative index, block = 3, kdef = 17, a Q with a doubled column and a call
    while a slq_submit ticket is outstanding each return KT_ERR_ARG with a
    message and leave the context usable."""
    from krylov_robustness_amd import _lib
    A = load_graph("anaheim")
    n = A.shape[0]
    D = kra.DeviceMatrix(A, gpu_ctx)
    P, _ = _mixed_pairs(A)
    o = _oracle(_blocks_named("anaheim", 16, 0, 30, 3, "cosh", 0), P)
    _check(kra.entries_fun(D, P, 16, m=30, seed=3, fun="cosh", ctx=gpu_ctx), o, 16)
    Q17, _ = np.linalg.qr(np.random.default_rng(0).normal(size=(n, 17)))
    Q17 = np.asfortranarray(Q17)
    dup = np.asfortranarray(np.repeat(Q17[:, :1], 2, axis=1) / np.sqrt(2.0))
    raw = [dict(npairs=0, ei=[0], ej=[1]), dict(npairs=2, ei=[0, n], ej=[1, 1]), dict(npairs=2, ei=[0, 1], ej=[1, n]),
           dict(npairs=1, ei=[-1], ej=[1]), dict(npairs=1, ei=[0], ej=[1], block=3),
           dict(npairs=1, ei=[0], ej=[1], kdef=17, Q=Q17), dict(npairs=1, ei=[0], ej=[1], kdef=2, Q=dup)]
    for kw in raw:
        st, msg = _raw(D, **kw)
        assert st == _lib.KT_ERR_ARG and msg, kw
    for kw in (dict(block=3), dict(deflate=Q17), dict(deflate=dup), dict(nprobes=0), dict(m=0)):
        args = dict(nprobes=16, m=30, seed=3, ctx=gpu_ctx)
        args.update(kw)
        with pytest.raises(kra.KrylovError) as e:
            kra.entries_fun(D, P, **args)
        assert e.value.code == _lib.KT_ERR_ARG and str(e.value)
    pending = kra.slq_submit(D, 16, 30, 3, ctx=gpu_ctx)
    with pytest.raises(kra.KrylovError) as e:
        kra.entries_fun(D, P, 16, m=30, seed=3, ctx=gpu_ctx)
    assert e.value.code == _lib.KT_ERR_ARG and "outstanding" in str(e.value)
    kra.slq_collect(pending)
    _check(kra.entries_fun(D, P, 16, m=30, seed=3, fun="cosh", ctx=gpu_ctx), o, 16)

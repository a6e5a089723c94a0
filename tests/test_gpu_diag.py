"""GPU tests of kt_diag_fun, the deflated stochastic estimator of diag f(A)
(compute_centrality.m:9-10 with f = exp), against the numpy oracle on the same
counter-RNG probes.

Expected values follow the estimator's definition literally: with
Z = ko.rademacher(n, probes, seed), Pi = I - Q Q', Y = ko.lanczos_fmv(A, Pi Z),
    t = Z .* (Pi Y),  dsum = rowsum(t),  dsum2 = rowsum(t .* t),
    q_p = z'_p' f(A) z'_p by ko.lanczos_quadform,
    d0 = 2 rowsum(Q .* G) - rowsum((Q H) .* Q),  G = ko.lanczos_fmv(A, Q), H = Q'G.

Tolerances.  dsum: the project's own for Lanczos-f against the oracle
(test_lanczos_fmv_yform_basis_matches_oracle: 1e-10 max|y| per entry of y,
rtol 1e-8), summed over the N probes of a row: atol = 1e-10 N max|y - Q Q'y|.
dsum2: the same error delta of t carried through t^2 (2 |t| delta <= 2 max|y|
delta per probe): atol = 2e-10 N max|y|^2.  sum_q, sum_q2: 1e-8 relative, the
SLQ parity tolerance of test_gpu_slq.py.  d0: G within 1e-10 max|G| per entry
(the same Lanczos-f tolerance), |Q| <= 1, and 2 k + k^2-ish products per row
bounded by 4 k terms of size delta: atol = 4e-10 k max|G|, rtol 1e-8."""
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


def _oracle(A, N, off, m, seed, fun, Q):
    n = A.shape[0]
    Z = ko.rademacher(n, range(off, off + N), seed)
    Zp = Z if Q is None else Z - Q @ (Q.T @ Z)
    Y = ko.lanczos_fmv(A, Zp, m, fun)
    Yp = Y if Q is None else Y - Q @ (Q.T @ Y)
    T = Z * Yp
    q = np.array([ko.lanczos_quadform(A, Zp[:, p], m, fun) for p in range(N)])
    out = {"T": T, "dsum": T.sum(axis=1), "dsum2": (T * T).sum(axis=1), "q": q, "scale": np.abs(Yp).max(),
           "d0": np.zeros(n), "gmax": 0.0}
    if Q is not None:
        G = ko.lanczos_fmv(A, Q, m, fun)
        H = Q.T @ G
        out["d0"] = 2.0 * (Q * G).sum(axis=1) - ((Q @ H) * Q).sum(axis=1)
        out["gmax"] = np.abs(G).max()
    return out


@functools.lru_cache(maxsize=None)
def _oracle_named(name, N, off, m, seed, fun, k):
    return _oracle(load_graph(name), N, off, m, seed, fun, _defl(name, k))


def _check(r, o, N, k=0, sums=True):
    """Parity of a DiagEstimate with the oracle's sums, and the sum identity."""
    np.testing.assert_allclose(r.dsum, o["dsum"], rtol=1e-8, atol=1e-10 * N * o["scale"])
    np.testing.assert_allclose(r.dsum2, o["dsum2"], rtol=1e-8, atol=2e-10 * N * o["scale"] ** 2)
    if sums:
        assert r.sum_q == pytest.approx(o["q"].sum(), rel=1e-8)
        assert r.sum_q2 == pytest.approx((o["q"] ** 2).sum(), rel=1e-8)
    if k:
        np.testing.assert_allclose(r.d0, o["d0"], rtol=1e-8, atol=4e-10 * k * o["gmax"])
    else:
        assert not r.d0.any()
    # in exact arithmetic sum_i dsum_i = sum_q
    assert abs(r.dsum.sum() - r.sum_q) <= 1e-11 * np.abs(o["T"]).sum()
    for a in (r.dsum, r.dsum2, r.d0, r.mean, r.stderr):
        assert np.isfinite(a).all()


@pytest.mark.parametrize("name", ["anaheim", "oregon_A0", "india"])
def test_parity_without_deflation(kra, gpu_ctx, name):
    """N = 16 probes in one 16-wide sweep, m = 30: unit weights (anaheim), a
    206-entry row above long_thresh (oregon_A0), fp64 weights (india).  sum_q
    is also the sum kt_slq_trace forms from the same probes."""
    A = load_graph(name)
    D = kra.DeviceMatrix(A, gpu_ctx)
    r = kra.diag_fun(D, 16, m=30, seed=3, block=16, ctx=gpu_ctx)
    _check(r, _oracle_named(name, 16, 0, 30, 3, "exp", 0), 16)
    s1, _, _ = kra.slq_quadforms(D, 16, 30, 3, ctx=gpu_ctx)
    assert r.sum_q == pytest.approx(s1, rel=1e-10)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("name", ["oregon_A0", "india"])
def test_parity_with_deflation(kra, gpu_ctx, name, k):
    """k = 1 with the exact leading eigenvector, k = 4 with an inexact
    orthonormal Q.  On oregon_A0 max|y| is 3.6e7 before the output projection
    and 3.5e5 after it: a missing output projection fails this."""
    A = load_graph(name)
    Q = _defl(name, k)
    r = kra.diag_fun(kra.DeviceMatrix(A, gpu_ctx), 16, m=30, seed=3, block=16, deflate=Q, ctx=gpu_ctx)
    _check(r, _oracle_named(name, 16, 0, 30, 3, "exp", k), 16, k=k)


def test_ranges_widths_and_bit_identity(kra, gpu_ctx, monkeypatch):
    """oregon_A0, m = 12.  40 probes from offset 5 at block 16 (sweeps of 16,
    16 and a remainder of 8) match the oracle; the calls on [5, 21) and
    [21, 45) add up to it; blocks 1, 2 and 4 with 5 probes match the oracle;
    two identical calls, and a call on one sweep lane, are bit-identical."""
    A = load_graph("oregon_A0")
    D = kra.DeviceMatrix(A, gpu_ctx)
    Q = _defl("oregon_A0", 1)
    call = lambda N, off, blk, q=Q: kra.diag_fun(D, N, m=12, seed=5, probe_offset=off, block=blk, deflate=q,
                                                 ctx=gpu_ctx)
    full = call(40, 5, 16)
    _check(full, _oracle_named("oregon_A0", 40, 5, 12, 5, "exp", 1), 40, k=1)
    a, b = call(16, 5, 16), call(24, 21, 16)
    tol = 1e-12 * np.abs(full.dsum).max()
    np.testing.assert_allclose(a.dsum + b.dsum, full.dsum, rtol=0, atol=tol)
    np.testing.assert_allclose(a.dsum2 + b.dsum2, full.dsum2, rtol=0, atol=1e-12 * np.abs(full.dsum2).max())
    assert a.sum_q + b.sum_q == pytest.approx(full.sum_q, rel=1e-12)
    for blk in (1, 2, 4):
        for q, k in ((Q, 1), (None, 0)):
            _check(call(5, 0, blk, q), _oracle_named("oregon_A0", 5, 0, 12, 5, "exp", k), 5, k=k)
    again = call(40, 5, 16)
    monkeypatch.setenv("KT_SLQ_LANES", "1")
    one_lane = call(40, 5, 16)
    monkeypatch.delenv("KT_SLQ_LANES")
    for other in (again, one_lane):
        for f in ("dsum", "dsum2", "d0"):
            assert np.array_equal(getattr(full, f), getattr(other, f)), f
        assert (full.sum_q, full.sum_q2) == (other.sum_q, other.sum_q2)


def test_lucky_breakdown_cuts_the_basis(kra, gpu_ctx):
    """32 disjoint edges: every Krylov space has dimension 2, so every column
    breaks down at step 2 of 30 and the basis slots past the cut must not
    enter the sum.  exp(A) = cosh(1) I + sinh(1) A gives
    dsum_i = 16 cosh 1 + sinh 1 sum_p z_p[i] z_p[i xor 1]."""
    n = 64
    i = np.arange(n)
    A = sp.csr_matrix((np.ones(n), (i, i ^ 1)), shape=(n, n))
    r = kra.diag_fun(kra.DeviceMatrix(A, gpu_ctx), 16, m=30, seed=2, ctx=gpu_ctx)
    Z = ko.rademacher(n, range(16), 2)
    exact = 16 * np.cosh(1.0) + np.sinh(1.0) * (Z * Z[i ^ 1]).sum(axis=1)
    np.testing.assert_allclose(r.dsum, exact, rtol=0, atol=1e-12)
    assert r.sum_q == pytest.approx(exact.sum(), rel=1e-12)
    for a in (r.dsum, r.dsum2, r.d0, r.mean, r.stderr, np.array([r.sum_q, r.sum_q2])):
        assert np.isfinite(a).all()


def test_larger_n_grid_stride_and_permutation(kra, gpu_ctx):
    """n = 50,000 (several workgroups per kernel, the grid-stride loops, the
    permutation back to original numbering), m = 10, k = 1 with the device's
    leading eigenvector fetched to the host and passed as Q."""
    from krylov_robustness_amd import graphs
    A = graphs.erdos_renyi(50_000, 250_000, seed=1)
    D = kra.DeviceMatrix(A, gpu_ctx)
    _, u = kra.eigs_leading(D, ctx=gpu_ctx)
    Q = np.asfortranarray(u[:, None])
    r = kra.diag_fun(D, 16, m=10, seed=1, deflate=Q, ctx=gpu_ctx)
    _check(r, _oracle(A, 16, 0, 10, 1, "exp", Q), 16, k=1)


def test_subgraph_centrality_estimate(kra, gpu_ctx):
    """compute_centrality(D, 'exp') on oregon_A0: 256 probes, deflation by
    the device's leading eigenvector u.  With E = exp(A), R = (I - uu') E
    (I - uu') the exact standard deviation of node i's estimate is
    sigma_i = sqrt((sum_j R_ij^2 - R_ii^2) / 256).  Every node is within
    6 sigma (the oracle's worst is 3.83), the reported stderr within
    [0.7, 1.4] sigma (oracle: 0.95 to 1.09), the median relative error at most
    1e-2 (oracle 1.9e-3; 2.37 without deflation)."""
    name = "oregon_A0"
    A = load_graph(name)
    D = kra.DeviceMatrix(A, gpu_ctx)
    w, V = _eig(name)
    E = (V * np.exp(w)) @ V.T
    _, u = kra.eigs_leading(D, ctx=gpu_ctx)
    Pi = np.eye(A.shape[0]) - np.outer(u, u)
    R = Pi @ E @ Pi
    sigma = np.sqrt(((R * R).sum(axis=1) - np.diag(R) ** 2) / 256)
    est = kra.compute_centrality(D, "exp", ctx=gpu_ctx, nprobes=256, seed=7)
    exact = np.diag(E)
    z = np.abs(est - exact) / sigma
    print("worst |err| / sigma", z.max(), "median rel err", np.median(np.abs(est - exact) / exact))
    assert (z <= 6.0).all(), z.max()
    r = kra.diag_fun(D, 256, seed=7, deflate=1, ctx=gpu_ctx)
    np.testing.assert_allclose(r.mean, est, rtol=1e-9)
    ratio = r.stderr / sigma
    print("stderr / sigma", ratio.min(), ratio.max())
    assert (ratio >= 0.7).all() and (ratio <= 1.4).all(), (ratio.min(), ratio.max())
    assert np.median(np.abs(est - exact) / exact) <= 1e-2


def test_other_function_and_argument_errors(kra, gpu_ctx):
    """fun = cosh matches the oracle; block = 3, kdef = 17, a Q with a doubled
    column and a call while a slq_submit ticket is outstanding each return
    their status with a message and leave the context usable."""
    from krylov_robustness_amd import _lib
    A = load_graph("anaheim")
    n = A.shape[0]
    D = kra.DeviceMatrix(A, gpu_ctx)
    o = _oracle_named("anaheim", 16, 0, 30, 3, "cosh", 0)
    _check(kra.diag_fun(D, 16, m=30, seed=3, fun="cosh", ctx=gpu_ctx), o, 16)
    Q17, _ = np.linalg.qr(np.random.default_rng(0).normal(size=(n, 17)))
    dup = np.repeat(Q17[:, :1], 2, axis=1) / np.sqrt(2.0)
    bad = [dict(block=3), dict(deflate=Q17), dict(deflate=dup), dict(nprobes=0), dict(m=0)]
    for kw in bad:
        args = dict(nprobes=16, m=30, seed=3, ctx=gpu_ctx)
        args.update(kw)
        with pytest.raises(kra.KrylovError) as e:
            kra.diag_fun(D, **args)
        assert e.value.code == _lib.KT_ERR_ARG and str(e.value)
    pending = kra.slq_submit(D, 16, 30, 3, ctx=gpu_ctx)
    with pytest.raises(kra.KrylovError) as e:
        kra.diag_fun(D, 16, m=30, seed=3, ctx=gpu_ctx)
    assert e.value.code == _lib.KT_ERR_ARG and "outstanding" in str(e.value)
    kra.slq_collect(pending)
    _check(kra.diag_fun(D, 16, m=30, seed=3, fun="cosh", ctx=gpu_ctx), o, 16)

"""GPU tests of kt_miobi_break / kt_pairs_score_topk against
the NumPy restatement of the reference (tests/miobi_ref.py).

Parity: the restatement's eigensolver callback is kra.eigs_topk with the same
seed on a matrix with the same entries, so both sides start every window from
the same bits; the restatement is driven along the device's selections and
reports, per step, its own minimum, its runner-up gap and the relative excess
of the device's pair over its minimum.  Bounds: a score is t terms, each exp
carrying |x| eps argument error with |x| <= lambda_1 + 2 ~ 1e2 at most on these
graphs, ~3e-14 relative in all; 1e-12 leaves room.  The golden graphs must not
need the near-tie allowance (their smallest runner-up gap is asserted >= 1e-9);
the path graph, whose mirrored edges tie to rounding, is the case that does."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph

import miobi_ref as mr

pytestmark = pytest.mark.gpu

T, K, SEED = 25, 24, 3
GOLDEN = ["oregon_A0", "anaheim", "india", "austria"]


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


def weighted_copy(A, seed=0):
    U = sp.triu(sp.csr_matrix(A), 1).tocoo()
    w = np.random.default_rng(seed).uniform(0.5, 1.5, U.nnz)
    W = sp.coo_matrix((w, (U.row, U.col)), shape=A.shape).tocsr()
    return sp.csr_matrix(W + W.T)


def graph(name):
    if name == "path100":
        return sp.diags([np.ones(99), np.ones(99)], [-1, 1], format="csr"), 5
    if name == "anaheim_weighted":
        return weighted_copy(load_graph("anaheim")), T
    return sp.csr_matrix(load_graph(name)), T


def solver(kra, ctx):
    return lambda S, t: kra.eigs_topk(kra.DeviceMatrix(S, ctx), t, seed=SEED, ctx=ctx)


def minus_edges(A, edges0):
    """A with the 0-based pairs removed, entry for entry."""
    B = sp.lil_matrix(A)
    for i, j in edges0:
        B[i, j] = 0.0
        B[j, i] = 0.0
    B = sp.csr_matrix(B)
    B.eliminate_zeros()
    return B


def check_steps(name, edges, info, ref, k, golden):
    nsel = len(edges)
    assert nsel == k == ref["nsel"], (nsel, ref["nsel"])
    assert ref["alive"].all()
    e0 = edges - 1
    assert (e0[:, 0] > e0[:, 1]).all() and (ref["edges"] == e0).all()
    print(name, "smallest runner-up gap", ref["gap"].min(), "largest excess over the minimum", np.abs(ref["excess"]).max(),
          "score rel err", np.abs(info["scores"] - ref["score"]).max() / np.abs(ref["score"]).min())
    assert (np.abs(ref["excess"]) <= 1e-12).all(), ref["excess"]
    clear = ref["gap"] >= 1e-9
    assert (ref["own"][clear] == e0[clear]).all()
    if golden:
        assert ref["gap"].min() >= 1e-9, ref["gap"]
    assert (np.abs(info["scores"] - ref["score"]) <= 1e-12 * np.abs(ref["score"])).all()
    l1 = abs(ref["track"][0, 0])
    assert info["track"].shape == ref["track"].shape
    print(name, "track err / |lambda_1|", np.abs(info["track"] - ref["track"]).max() / l1)
    assert np.abs(info["track"] - ref["track"]).max() <= 1e-12 * l1


@pytest.mark.parametrize("refresh", [8, 0])
@pytest.mark.parametrize("name", GOLDEN + ["path100", "anaheim_weighted"])
def test_parity_with_the_restatement(kra, gpu_ctx, name, refresh):
    A, t = graph(name)
    D = kra.DeviceMatrix(A, gpu_ctx)
    edges, info = kra.miobi_break(D, K, t=t, refresh=refresh, seed=SEED, ctx=gpu_ctx)
    eig = solver(kra, gpu_ctx)
    ref = mr.miobi_break_ref(A, K, t, eig, refresh=refresh, forced=edges - 1)
    check_steps(name, edges, info, ref, K, name in GOLDEN or name == "anaheim_weighted")
    assert info["refreshes"] == ((K - 1) // refresh if refresh else 0) == ref["refreshes"]
    assert info["nconv_min"] == t
    want = minus_edges(A, edges - 1)
    got = sp.csr_matrix(D.to_scipy())
    assert got.nnz == want.nnz and abs(got - want).nnz == 0
    assert abs(got - ref["A"]).nnz == 0
    rob = mr.rob_score(ref["track"][0], eig(ref["A"], t)[0])
    print(name, "rob_score", info["rob_score"], "restatement", rob)
    assert abs(info["rob_score"] - rob) <= 1e-9 * abs(rob)
    assert info["R0"] == pytest.approx(mr.log_mean_exp(ref["track"][0]), rel=1e-13)


@pytest.mark.parametrize("name", ["anaheim", "oregon_A0"])
def test_paper_mode(kra, gpu_ctx, name):
    A, t = graph(name)
    k = 12
    D = kra.DeviceMatrix(A, gpu_ctx)
    edges, info = kra.miobi_break(D, k, t=t, refresh=0, mode="paper", seed=SEED, return_V=True, ctx=gpu_ctx)
    ref = mr.miobi_break_ref(A, k, t, solver(kra, gpu_ctx), refresh=0, mode="paper", forced=edges - 1)
    check_steps(name, edges, info, ref, k, True)
    V, Vr = info["V"], ref["V"]
    assert V.shape == Vr.shape == (A.shape[0], t)
    err = np.abs(V - Vr).max(axis=0)
    print(name, "paper: worst column error / max|V|", err.max() / np.abs(Vr).max(), "largest |deltaV|", ref["dv_max"].max())
    assert (err <= 1e-9 * np.abs(Vr).max()).all(), err
    assert np.abs(np.linalg.norm(V, axis=0) - 1.0).max() <= 1e-14
    assert (V[:, 0] >= 0.0).all()
    assert ref["dv_max"].max() > 0.0  # the vectors did move


def test_reference_mode_keeps_the_vectors(kra, gpu_ctx):
    A, t = graph("anaheim")
    _, info = kra.miobi_break(kra.DeviceMatrix(A, gpu_ctx), 6, t=t, refresh=0, seed=SEED, return_V=True, ctx=gpu_ctx)
    V0 = np.array(kra.eigs_topk(kra.DeviceMatrix(A, gpu_ctx), t, seed=SEED, ctx=gpu_ctx)[1])
    V0[:, 0] = np.abs(V0[:, 0])
    assert info["V"].tobytes() == V0.tobytes()


@pytest.mark.parametrize("sign", [-2.0, 2.0])
@pytest.mark.parametrize("t", [2, 16, 17, 32])
def test_pairs_score_topk(kra, gpu_ctx, t, sign):
    rng = np.random.default_rng(100 * t + int(sign))
    n = 301
    V = np.linalg.qr(rng.normal(size=(n, t)))[0]
    lam = np.sort(rng.uniform(-2.0, 12.0, t))[::-1]
    for npairs in (1, 63, 64, 65, 10000):
        P = rng.integers(0, n, size=(npairs, 2))
        got = kra.pairs_score_topk(lam, V, P, sign=sign, ctx=gpu_ctx)
        want = np.sum(np.exp(lam)[None, :] * np.exp(sign * V[P[:, 0]] * V[P[:, 1]]), axis=1)
        assert got.shape == (npairs,)
        err = np.abs(got - want).max() / np.abs(want).min()
        assert err <= 1e-12, (npairs, err)
        assert got.tobytes() == kra.pairs_score_topk(lam, V, P, sign=sign, ctx=gpu_ctx).tobytes()
    for bad in (np.array([[0, n]]), np.array([[-1, 0]])):
        with pytest.raises(kra.KrylovError):
            kra.pairs_score_topk(lam, V, bad, ctx=gpu_ctx)


def test_find_top_edges_miobi(kra, gpu_ctx):
    from krylov_robustness_amd.greedy import _tril_edges
    A, t = graph("oregon_A0")
    D = kra.DeviceMatrix(A, gpu_ctx)
    top = kra.find_top_edges_miobi(D, 50, t=t, seed=SEED, ctx=gpu_ctx)
    lam, V = kra.eigs_topk(D, t, seed=SEED, ctx=gpu_ctx)
    V = np.array(V)
    V[:, 0] = np.abs(V[:, 0])
    I, J = _tril_edges(sp.csc_matrix(A))
    score = kra.pairs_score_topk(lam, V, np.stack([I, J], axis=1), ctx=gpu_ctx)
    ind = np.argsort(score, kind="stable")[:50]
    assert top.shape == (50, 2) and (top[:, 0] > top[:, 1]).all()
    assert (top == np.stack([I[ind] + 1, J[ind] + 1], axis=1)).all()
    host = np.sum(np.exp(lam)[None, :] * np.exp(-2.0 * V[I] * V[J]), axis=1)
    assert np.abs(score - host).max() <= 1e-12 * np.abs(host).min()
    # the ranking feeds greedy_krylov
    edges, _, _ = kra.greedy_krylov(kra.DeviceMatrix(A, gpu_ctx), 2, Q=10, top=top, tol=1e-6, ctx=gpu_ctx)
    assert edges.shape == (2, 2) and {tuple(e) for e in edges} <= {tuple(e) for e in top}


def test_exhaustion(kra, gpu_ctx):
    n = 140
    A = sp.lil_matrix((n, n))
    A[0, 1:] = 1.0
    A[1:, 0] = 1.0
    D = kra.DeviceMatrix(sp.csr_matrix(A), gpu_ctx)
    edges, info = kra.miobi_break(D, 200, t=T, refresh=50, seed=SEED, ctx=gpu_ctx)
    assert len(edges) == 139 and len({tuple(e) for e in edges}) == 139
    assert info["scores"].shape == (139,) and info["track"].shape == (140, T)
    assert D.to_scipy().nnz == 0 and D.info()[1] == 0
    assert info["refreshes"] == 2


def test_determinism(kra, gpu_ctx):
    A, t = graph("anaheim")
    runs = [kra.miobi_break(kra.DeviceMatrix(A, gpu_ctx), K, t=t, refresh=8, seed=SEED, ctx=gpu_ctx) for _ in range(2)]
    (e1, i1), (e2, i2) = runs
    assert e1.tobytes() == e2.tobytes()
    assert i1["scores"].tobytes() == i2["scores"].tobytes() and i1["track"].tobytes() == i2["track"].tobytes()


def test_argument_errors_leave_the_matrix_usable(kra, gpu_ctx):
    A, _ = graph("austria")
    D = kra.DeviceMatrix(A, gpu_ctx)
    for bad in (1, 33):
        with pytest.raises(kra.KrylovError) as e:
            kra.miobi_break(D, 3, t=bad, ctx=gpu_ctx)
        assert "t must be in" in str(e.value)
    small = kra.DeviceMatrix(sp.csr_matrix(np.ones((10, 10)) - np.eye(10)), gpu_ctx)
    with pytest.raises(kra.KrylovError):
        kra.miobi_break(small, 3, t=11, ctx=gpu_ctx)
    with pytest.raises(kra.KrylovError):
        kra.miobi_break(D, 3, mode="other", ctx=gpu_ctx)
    N = sp.csr_matrix(A).tolil()
    i, j = sp.triu(A, 1).nonzero()
    N[i[0], j[0]] = 0.0
    ns = kra.DeviceMatrix(sp.csr_matrix(N), gpu_ctx)
    with pytest.raises(kra.KrylovError):
        kra.miobi_break(ns, 3, t=5, ctx=gpu_ctx)
    assert abs(ns.to_scipy() - sp.csr_matrix(N)).nnz == 0
    lam = kra.eigs_topk(D, 4, ctx=gpu_ctx)[0]
    edges, info = kra.miobi_break(D, 3, t=5, ctx=gpu_ctx)
    assert len(edges) == 3 and np.isfinite(lam).all() and np.isfinite(info["rob_score"])
    e10, _ = kra.miobi_break(small, 3, t=10, ctx=gpu_ctx)
    assert len(e10) == 3

"""GPU tests of kt_miobi_make against the NumPy restatement
of the reference (tests/miobi_make_ref.py).

Parity: the restatement's eigensolver callback is kra.eigs_topk with the same
seed on a matrix with the same entries, so both sides start every window from
the same bits; the restatement is driven along the device's selections and
reports, per step, its own maximum, its runner-up gap, the relative excess of
its maximum over the device's pair, and its m.  Bounds as for the removal
(tests/test_gpu_miobi.py): a score is t terms, each exp carrying |x| eps
argument error with |x| <= lambda_1 + 2 ~ 1e2 at most on these graphs, ~3e-14
relative in all; 1e-12 leaves room.  The clear-gap graphs must not need the
near-tie allowance (their smallest runner-up gap is asserted >= 1e-9); the
binarised weighted graphs, whose twin nodes tie exactly, and the star, whose
leaves tie to rounding, are the cases that do."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph

import miobi_make_ref as mk

pytestmark = pytest.mark.gpu

T, K, SEED = 25, 24, 3
CLEAR = ["oregon_A0", "anaheim", "rome"]
NEAR_TIE = ["austria", "denmark", "india"]


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


def star(n):
    A = sp.lil_matrix((n, n))
    A[0, 1:] = 1.0
    A[1:, 0] = 1.0
    return sp.csr_matrix(A)


def graph(name):
    if name == "star140":
        return star(140), 5
    return mk.binarise(load_graph(name)), K


def solver(kra, ctx):
    return lambda S, t: kra.eigs_topk(kra.DeviceMatrix(S, ctx), t, seed=SEED, ctx=ctx)


def plus_edges(A, edges0):
    """A with the 0-based pairs set to 1, entry for entry."""
    B = sp.lil_matrix(A)
    for i, j in edges0:
        B[i, j] = 1.0
        B[j, i] = 1.0
    return sp.csr_matrix(B)


def check_steps(name, edges, info, ref, k, clear):
    nsel = len(edges)
    assert nsel == k == ref["nsel"], (nsel, ref["nsel"], ref["alive"])
    assert ref["alive"].all()
    e0 = edges - 1
    assert (e0[:, 0] > e0[:, 1]).all() and (ref["edges"] == e0).all()
    print(name, "m", info["m"][0], "->", info["m"][-1], "pairs", ref["npairs"][0], "smallest runner-up gap",
          ref["gap"].min(), "largest excess of the maximum", np.abs(ref["excess"]).max(), "score rel err",
          (np.abs(info["scores"] - ref["score"]) / np.abs(ref["score"])).max())
    assert (np.abs(ref["excess"]) <= 1e-12).all(), ref["excess"]
    assert info["m"].shape == ref["m"].shape and (info["m"] == ref["m"]).all(), (info["m"], ref["m"])
    sure = ref["gap"] >= 1e-9
    assert (ref["own"][sure] == e0[sure]).all()
    if clear:
        assert ref["gap"].min() >= 1e-9, ref["gap"]
    assert (np.abs(info["scores"] - ref["score"]) <= 1e-12 * np.abs(ref["score"])).all()
    l1 = abs(ref["track"][0, 0])
    assert info["track"].shape == ref["track"].shape
    print(name, "track err / |lambda_1|", np.abs(info["track"] - ref["track"]).max() / l1)
    assert np.abs(info["track"] - ref["track"]).max() <= 1e-12 * l1


@pytest.mark.parametrize("refresh", [8, 0])
@pytest.mark.parametrize("name", CLEAR + NEAR_TIE + ["star140"])
def test_parity_with_the_restatement(kra, gpu_ctx, name, refresh):
    A, k = graph(name)
    D = kra.DeviceMatrix(A, gpu_ctx)
    edges, info = kra.miobi_make(D, k, t=T, refresh=refresh, seed=SEED, ctx=gpu_ctx)
    eig = solver(kra, gpu_ctx)
    ref = mk.miobi_make_ref(A, k, T, eig, refresh=refresh, forced=edges - 1)
    check_steps(name, edges, info, ref, k, name in CLEAR)
    if name == "star140":
        assert (info["m"] == 140).all()  # max degree + k is beyond n
    assert info["refreshes"] == ((k - 1) // refresh if refresh else 0) == ref["refreshes"]
    assert info["nconv_min"] == T
    want = plus_edges(A, edges - 1)
    got = sp.csr_matrix(D.to_scipy())
    assert got.nnz == want.nnz == A.nnz + 2 * len(edges) and abs(got - want).nnz == 0
    assert abs(got - ref["A"]).nnz == 0
    rob = mk.rob_score(ref["track"][0], eig(ref["A"], T)[0])
    print(name, "rob_score", info["rob_score"], "restatement", rob)
    assert abs(info["rob_score"] - rob) <= 1e-9 * abs(rob)
    assert info["R0"] == pytest.approx(mk.log_mean_exp(ref["track"][0]), rel=1e-13)


@pytest.mark.parametrize("t", [2, 17, 32])
def test_other_t(kra, gpu_ctx, t):
    A, _ = graph("oregon_A0")
    k = 6
    D = kra.DeviceMatrix(A, gpu_ctx)
    edges, info = kra.miobi_make(D, k, t=t, refresh=4, seed=SEED, ctx=gpu_ctx)
    ref = mk.miobi_make_ref(A, k, t, solver(kra, gpu_ctx), refresh=4, forced=edges - 1)
    check_steps(f"oregon_A0 t={t}", edges, info, ref, k, False)
    assert info["track"].shape == (k + 1, t) and info["refreshes"] == 1


def test_exhaustion(kra, gpu_ctx):
    """K_20 minus three edges: three steps, then no non-adjacent pair is left."""
    n = 20
    A = np.ones((n, n)) - np.eye(n)
    missing = [(3, 1), (11, 4), (19, 18)]
    for i, j in missing:
        A[i, j] = A[j, i] = 0.0
    D = kra.DeviceMatrix(sp.csr_matrix(A), gpu_ctx)
    edges, info = kra.miobi_make(D, 5, t=5, refresh=2, seed=SEED, ctx=gpu_ctx)
    assert len(edges) == 3 and {tuple(e) for e in edges - 1} == set(missing)
    assert info["scores"].shape == (3,) and info["track"].shape == (4, 5) and info["m"].shape == (3,)
    assert (info["m"] == n).all()
    got = sp.csr_matrix(D.to_scipy())
    assert got.nnz == n * (n - 1) and abs(got - sp.csr_matrix(np.ones((n, n)) - np.eye(n))).nnz == 0
    assert info["refreshes"] == 1


def test_determinism(kra, gpu_ctx):
    A, _ = graph("anaheim")
    runs = [kra.miobi_make(kra.DeviceMatrix(A, gpu_ctx), K, t=T, refresh=8, seed=SEED, ctx=gpu_ctx) for _ in range(2)]
    (e1, i1), (e2, i2) = runs
    assert e1.tobytes() == e2.tobytes() and i1["m"].tobytes() == i2["m"].tobytes()
    assert i1["scores"].tobytes() == i2["scores"].tobytes() and i1["track"].tobytes() == i2["track"].tobytes()


def test_argument_errors_leave_the_matrix_usable(kra, gpu_ctx):
    A, _ = graph("austria")
    D = kra.DeviceMatrix(A, gpu_ctx)
    for bad in (1, 33):
        with pytest.raises(kra.KrylovError) as e:
            kra.miobi_make(D, 3, t=bad, ctx=gpu_ctx)
        assert "t must be in" in str(e.value)
    small = kra.DeviceMatrix(star(10), gpu_ctx)
    with pytest.raises(kra.KrylovError):
        kra.miobi_make(small, 3, t=11, ctx=gpu_ctx)
    Wt = sp.csr_matrix(load_graph("austria"))  # the weighted original
    assert not (Wt.data == 1.0).all()
    wd = kra.DeviceMatrix(Wt, gpu_ctx)
    with pytest.raises(kra.KrylovError) as e:
        kra.miobi_make(wd, 3, t=5, ctx=gpu_ctx)
    assert "unit-weight" in str(e.value)
    assert abs(wd.to_scipy() - Wt).nnz == 0
    N = sp.csr_matrix(A).tolil()
    i, j = sp.triu(A, 1).nonzero()
    N[i[0], j[0]] = 0.0
    ns = kra.DeviceMatrix(sp.csr_matrix(N), gpu_ctx)
    with pytest.raises(kra.KrylovError):
        kra.miobi_make(ns, 3, t=5, ctx=gpu_ctx)
    assert abs(ns.to_scipy() - sp.csr_matrix(N)).nnz == 0
    assert abs(D.to_scipy() - A).nnz == 0
    lam = kra.eigs_topk(D, 4, ctx=gpu_ctx)[0]
    lw = kra.eigs_topk(wd, 4, ctx=gpu_ctx)[0]
    edges, info = kra.miobi_make(D, 3, t=5, ctx=gpu_ctx)
    assert len(edges) == 3 and np.isfinite(lam).all() and np.isfinite(lw).all() and np.isfinite(info["rob_score"])
    e10, _ = kra.miobi_make(small, 3, t=10, ctx=gpu_ctx)
    assert len(e10) == 3

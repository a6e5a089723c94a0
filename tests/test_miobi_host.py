"""CPU tests of the MIOBI restatement (tests/miobi_ref.py) on numpy.linalg.eigh:
the finding about the reference's eigenvector update, pinned; the weighted
shift; and the order of the `paper` update."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph

import miobi_ref as mr

T, K, REFRESH = 25, 24, 8


def weighted_copy(A, seed=0):
    """Seeded symmetric weights in [0.5, 1.5] on A's pattern."""
    U = sp.triu(sp.csr_matrix(A), 1).tocoo()
    w = np.random.default_rng(seed).uniform(0.5, 1.5, U.nnz)
    W = sp.coo_matrix((w, (U.row, U.col)), shape=A.shape).tocsr()
    return sp.csr_matrix(W + W.T)


@pytest.fixture(scope="module")
def anaheim():
    return load_graph("anaheim")


@pytest.fixture(scope="module")
def run(anaheim):
    return mr.miobi_break_ref(anaheim, K, T, mr.eigh_topk, refresh=REFRESH)


def test_literal_index_semantics_leave_deltav_zero(run):
    """MIOBIBreakEdge2.m:99-100 zeroes the whole of diffE: deltaV is identically
    zero at every step, with and between recomputations."""
    print("max |deltaV| per step:", run["dv_max"])
    assert len(run["dv_max"]) == K
    assert (run["dv_max"] == 0.0).all()
    assert run["refreshes"] == (K - 1) // REFRESH


def test_inner_sum_is_all_zero_for_distinct_eigenvalues():
    rng = np.random.default_rng(1)
    for t in (2, 3, 25):
        e = np.sort(rng.normal(size=t))[::-1]
        dH = rng.normal(size=(t, t))
        dH = dH + dH.T
        assert (mr.inner_sum(dH, e, "reference") == 0.0).all()
        S = mr.inner_sum(dH, e, "paper")
        off = ~np.eye(t, dtype=bool)
        assert (S[off] != 0.0).all() and (np.diag(S) == 0.0).all()
        assert np.allclose(S[off], (dH / (e[None, :] - e[:, None] + np.eye(t)))[off], rtol=1e-15)


def test_edges_are_distinct_and_complete(run, anaheim):
    assert run["nsel"] == K
    assert len({tuple(x) for x in run["edges"]}) == K
    assert (run["edges"][:, 0] > run["edges"][:, 1]).all()
    assert (run["edges"] == run["own"]).all() and (run["excess"] == 0.0).all()
    assert run["track"].shape == (K + 1, T)
    removed = sp.coo_matrix((np.ones(K), (run["edges"][:, 0], run["edges"][:, 1])), shape=anaheim.shape)
    assert (abs(anaheim - removed - removed.T - run["A"])).nnz == 0


def test_weighted_shift_uses_the_entry(anaheim):
    W = weighted_copy(anaheim)
    res = mr.miobi_break_ref(W, K, T, mr.eigh_topk, refresh=0)
    assert res["nsel"] == K
    e0, V0 = mr.eigh_topk(W, T)
    V0[:, 0] = np.abs(V0[:, 0])
    seen_weight_not_one = False
    e = e0.copy()
    for s, (i, j) in enumerate(res["edges"]):
        a = W[i, j]
        seen_weight_not_one |= abs(a - 1.0) > 1e-3
        e = e + -2.0 * a * V0[i] * V0[j]   # refresh = 0 and deltaV = 0: the vectors are V0 up to rounding
        assert np.abs(res["track"][s + 1] - e).max() <= 1e-13 * abs(e0[0]), s
        unit = res["track"][s] + -2.0 * V0[i] * V0[j]
        if abs(a - 1.0) > 1e-3 and np.abs(V0[i] * V0[j]).max() > 1e-6:
            assert np.abs(res["track"][s + 1] - unit).max() > 1e-10
    assert seen_weight_not_one


def _second_order_errors(A, t, full):
    """Errors of one `paper` update against eigh of A + s dA at s and s / 2 for
    the pair c with the largest exact gap: the eigenvalue, and the vector --
    with the full basis (t = n) the whole vector; with t < n its component in
    the span of the t vectors, because the sum of equation (9) over r <= t
    leaves out the first-order components along the other n - t vectors."""
    n = A.shape[0]
    w, U = np.linalg.eigh(A.toarray())
    w, U = w[::-1].copy(), U[:, ::-1].copy()
    tt = n if full else t
    gaps = np.array([np.min(np.abs(np.delete(w, c) - w[c])) for c in range(t)])
    c = int(np.argmax(gaps))
    assert gaps[c] >= 1e-3 * abs(w[0])
    p, r, wt = mr.upper_edges(A)
    q = int(np.argmax(np.abs(U[p, c] * U[r, c])))
    i, j, a = int(p[q]), int(r[q]), float(wt[q])
    V, e = U[:, :tt].copy(), w[:tt].copy()
    V[:, 0] = np.abs(V[:, 0])
    out = []
    for s in (0.02 * gaps[c], 0.01 * gaps[c]):
        Vn, en, _ = mr.update(V, e, i, j, a, "paper", scale=s)
        B = A.toarray()
        B[i, j] += -s * a
        B[j, i] += -s * a
        wx, Ux = np.linalg.eigh(B)
        wx, Ux = wx[::-1], Ux[:, ::-1]
        x = Ux[:, c] * np.sign(Ux[:, c] @ Vn[:, c])
        d = Vn[:, c] - x
        if not full:
            d = V.T @ d
        out.append((abs(en[c] - wx[c]), np.linalg.norm(d)))
    return c, gaps[c] / abs(w[0]), out


@pytest.mark.parametrize("full", [True, False])
def test_paper_update_is_second_order(anaheim, full):
    c, relgap, ((ev1, vec1), (ev2, vec2)) = _second_order_errors(anaheim, T, full)
    print("pair", c, "gap / |lambda_1|", relgap, "eigenvalue errors", ev1, ev2, "ratio", ev1 / ev2,
          "vector errors", vec1, vec2, "ratio", vec1 / vec2)
    assert 3.0 <= ev1 / ev2 <= 5.0
    assert 3.0 <= vec1 / vec2 <= 5.0


def test_reference_mode_update_leaves_the_vectors(anaheim):
    """The counterpart: with the literal semantics one update moves no vector
    beyond the division by its norm."""
    w, U = np.linalg.eigh(anaheim.toarray())
    w, U = w[::-1].copy(), U[:, ::-1].copy()
    V, e = U[:, :T].copy(), w[:T].copy()
    V[:, 0] = np.abs(V[:, 0])
    p, r, wt = mr.upper_edges(anaheim)
    q = int(np.argmax(np.abs(V[p, 0] * V[r, 0])))
    Vn, _, dV = mr.update(V, e, int(p[q]), int(r[q]), 1.0, "reference")
    assert (dV == 0.0).all() and np.abs(Vn - V).max() <= 4e-16


def test_abi_rejects_bad_arguments_before_the_device():
    import ctypes as C
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sig["kt_miobi_break"]) == 17 and len(sig["kt_pairs_score_topk"]) == 10
    ns = C.c_int64()
    for t in (1, 25, 33):  # a NULL matrix, whatever t
        assert lib.kt_miobi_break(None, 3, t, 50, 0, 0.0, 0.0, 0, 0, None, None, None, None, None, C.byref(ns),
                                  None, None) == _lib.KT_ERR_ARG
        assert b"kt_miobi_break" in lib.kt_last_error()
    lam = (C.c_double * 40)()
    assert lib.kt_pairs_score_topk(None, 10, 2, lam, lam, 0, None, None, -2.0, None) == _lib.KT_ERR_ARG
    assert b"kt_pairs_score_topk" in lib.kt_last_error()


def test_python_rejects_an_unknown_mode_without_a_device(monkeypatch, anaheim):
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import greedy

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(greedy, "_dev", no_device)
    with pytest.raises(kra.KrylovError):
        kra.miobi_break(anaheim, 3, mode="exact")


def test_kernel_check_host_enumeration():
    """tests/native/miobi_check --host: the cases the device run is held to."""
    import json
    import os
    import subprocess
    from conftest import ROOT
    check = os.path.join(ROOT, "tests", "native", "miobi_check", "miobi_check")
    assert os.path.exists(check), "tests/native/miobi_check/miobi_check is not built (__graft_entry__.build())"
    r = subprocess.run([check, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mode"] == "host" and out["max_score_rel_err"] <= 1e-12
    cases = {g: v["cases"] for g, v in out["groups"].items()}
    assert all(v["failed_count"] == 0 for v in out["groups"].values())
    assert cases["score"] == cases["pick"] >= 36 + 9 and cases["apply"] >= 36 and cases["norm"] == 6
    assert sum(cases.values()) <= 150  # a few dozen per group, not a sweep

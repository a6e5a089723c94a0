"""CPU tests of the MIOBI make-edge restatement (tests/miobi_make_ref.py) on
numpy.linalg.eigh: the finding about the reference's eigenvector update on
MIOBIMakeEdge.m's own lines, the enumeration order, the first-maximum rule,
the stability of the candidate ranking under the per-step normalisation, and
the new ABI entry's argument checks without a device."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph

import miobi_make_ref as mk

T, K, REFRESH = 25, 24, 8
GRAPHS = ["oregon_A0", "anaheim", "rome", "austria", "denmark", "india"]


@pytest.fixture(scope="module")
def run():
    return mk.miobi_make_ref(load_graph("anaheim"), K, T, mk.eigh_topk, refresh=REFRESH)


def test_literal_index_semantics_leave_deltav_zero(run):
    """MIOBIMakeEdge.m:133-134 zeroes the whole of diffE, as MIOBIBreakEdge2.m:
    99-100 does: deltaV is identically zero at every step."""
    print("max |deltaV| per step:", run["dv_max"])
    assert len(run["dv_max"]) == K == run["nsel"]
    assert (run["dv_max"] == 0.0).all()
    assert run["refreshes"] == (K - 1) // REFRESH


def test_run_is_complete(run):
    A = mk.binarise(load_graph("anaheim"))
    assert len({tuple(x) for x in run["edges"]}) == K
    assert (run["edges"][:, 0] > run["edges"][:, 1]).all()
    assert (run["edges"] == run["own"]).all() and (run["excess"] == 0.0).all()
    assert run["track"].shape == (K + 1, T) and run["m"].shape == (K,)
    assert all(A[i, j] == 0 for i, j in run["edges"])
    added = sp.coo_matrix((np.ones(K), (run["edges"][:, 0], run["edges"][:, 1])), shape=A.shape)
    assert abs(A + added + added.T - run["A"]).nnz == 0
    # m follows the running maximum degree with the WHOLE budget
    deg = np.asarray(A.sum(axis=1)).ravel()
    for s, (i, j) in enumerate(run["edges"]):
        assert run["m"][s] == min(int(deg.max()) + K, A.shape[0])
        deg[i] += 1
        deg[j] += 1
    assert (run["npairs"] <= run["m"] * (run["m"] - 1) // 2).all() and (run["npairs"] > 0).all()


def test_vectorised_enumeration_is_the_double_loop():
    rng = np.random.default_rng(5)
    n = 30
    U = np.triu(rng.random((n, n)) < 0.3, 1)
    adj = U | U.T
    for m in (2, 7, 30):
        cand = rng.permutation(n)[:m]
        ia, ib = mk.enumerate_pairs(adj, cand)
        la, lb = mk.enumerate_pairs_loop(adj, cand)
        assert (ia == la).all() and (ib == lb).all()
        assert (ia < ib).all() and ((np.diff(ia) > 0) | ((np.diff(ia) == 0) & (np.diff(ib) > 0))).all()


def test_an_exact_tie_goes_to_the_first_pair():
    """Nodes 0..3 of a 12-node graph share one row of V: the six pairs among
    them score the same bits, and the first in the a-then-b enumeration wins --
    ranks follow ascending index among equal values (the stable sort)."""
    n, t = 12, 3

    def eig(S, tt):
        V = np.zeros((n, tt))
        V[:, 0] = np.linspace(0.05, 0.01, n)
        V[:4, 0] = 0.5
        V[:4, 1] = 0.25
        V[:4, 2] = -0.125
        V[4:, 1] = np.linspace(0.01, 0.02, n - 4)
        return np.array([2.0, 1.0, 0.5]), V

    ring = sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], format="lil")
    ring[0, 1] = ring[1, 0] = 0.0                 # 0-1 is free, 1-2 and 2-3 are edges
    res = mk.miobi_make_ref(sp.csr_matrix(ring), 3, t, eig)
    assert res["gap"][0] == 0.0                   # an exact tie at the top
    assert [tuple(x) for x in res["edges"]] == [(1, 0), (2, 0), (3, 0)]
    assert (res["dv_max"] == 0.0).all()


@pytest.mark.parametrize("name", GRAPHS)
def test_the_normalisation_keeps_the_ranking(name):
    """The device ranks once per window and skips the per-step normalisation:
    dividing a column by its norm must not reorder it."""
    A = mk.binarise(load_graph(name))
    e, V = mk.eigh_topk(A, T)
    V[:, 0] = np.abs(V[:, 0])
    order0 = mk.candidates(V[:, 0], A.shape[0])
    v = V[:, 0].copy()
    for _ in range(50):
        v = np.abs(v / np.linalg.norm(v))
        assert (mk.candidates(v, A.shape[0]) == order0).all()
    print(name, "max |dV| after 50 normalisations", np.abs(v - V[:, 0]).max())
    # each pass rounds the norm and the quotient: two roundings of entries below 1 in magnitude
    assert np.abs(v - V[:, 0]).max() <= 50 * 2 * np.finfo(np.float64).eps


def test_rob_score_has_the_make_sign():
    lam0, lam1 = np.array([3.0, 1.0]), np.array([3.5, 1.0])
    assert mk.rob_score(lam0, lam1) > 0.0
    assert mk.rob_score(lam0, lam1) == pytest.approx(
        (mk.log_mean_exp(lam1) - mk.log_mean_exp(lam0)) * 100.0 / mk.log_mean_exp(lam0))


def test_abi_rejects_bad_arguments_before_the_device():
    import ctypes as C
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sig["kt_miobi_make"]) == 15
    ns = C.c_int64()
    for t in (1, 25, 33):  # a NULL matrix, whatever t
        assert lib.kt_miobi_make(None, 3, t, 50, 0.0, 0, 0, None, None, None, None, None, C.byref(ns),
                                 None, None) == _lib.KT_ERR_ARG
        assert b"kt_miobi_make" in lib.kt_last_error()


def test_kernel_check_host_enumeration():
    """tests/native/miobi_make_check --host: the cases the device run is held to."""
    import json
    import os
    import subprocess
    from conftest import ROOT
    check = os.path.join(ROOT, "tests", "native", "miobi_make_check", "miobi_make_check")
    assert os.path.exists(check), "tests/native/miobi_make_check/miobi_make_check is not built (__graft_entry__.build())"
    r = subprocess.run([check, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mode"] == "host" and out["max_score_rel_err"] <= 1e-12
    cases = {g: v["cases"] for g, v in out["groups"].items()}
    assert all(v["failed_count"] == 0 for v in out["groups"].values())
    assert cases["score"] == cases["pick"] >= 36 + 20 and cases["apply"] >= 36 + 17
    assert sum(cases.values()) <= 200  # a few dozen per group, not a sweep

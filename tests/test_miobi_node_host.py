"""CPU tests of the MIOBI node-removal restatement (tests/miobi_node_ref.py) on
numpy.linalg.eigh: the three findings about MIOBIBreakNode.m that DESIGN.md
§4.2g states (the vector update never happens; the eigenvalue shift is that of
a full -1 row and column; the recomputation counts removed entries, not steps),
the first loop's rule for a node without entries, the first-minimum rule, and
the new ABI entries' argument checks without a device."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph

import miobi_node_ref as nr

T, K = 25, 12


@pytest.fixture(scope="module")
def run():
    return nr.miobi_break_node_ref(load_graph("anaheim"), K, T, nr.eigh_topk, refresh=50)


def test_literal_index_semantics_leave_deltav_zero(run):
    """MIOBIBreakNode.m:232-233 zeroes the whole of diffE, as MIOBIBreakEdge2.m:
    99-100 does: deltaV is identically zero at every step."""
    print("max |deltaV| per step:", run["dv_max"])
    assert len(run["dv_max"]) == K == run["nsel"]
    assert (run["dv_max"] == 0.0).all()


def test_run_is_complete(run):
    A = nr.binarise(load_graph("anaheim"))
    assert len(set(run["nodes"].tolist())) == K
    assert (run["nodes"] == run["own"]).all() and (run["excess"] == 0.0).all()
    assert run["track"].shape == (K + 1, T)
    live = np.ones(A.shape[0], dtype=bool)
    acc, wends = 0, 0
    for s, r in enumerate(run["nodes"]):
        M = nr.current(A, live)
        assert run["degree"][s] == M.indptr[r + 1] - M.indptr[r] >= 1
        acc += 2 * run["degree"][s]
        assert run["wend"][s] == (acc >= 50)
        acc %= 50
        assert run["acc"][s] == acc
        wends += int(run["wend"][s] and s + 1 < K)
        live[r] = False
    assert run["refreshes"] == wends
    assert abs(nr.current(A, live) - run["A"]).nnz == 0


def test_the_shift_is_that_of_a_full_row_and_column():
    """:216-217 assign all N entries of row and column `remove`: the diagonal of
    the literal dense V' deltaA V is -(2 v s - v^2) with s the column sums over
    ALL rows, not the first-order shift of the entries removed."""
    A = nr.binarise(load_graph("austria"))
    e, V = nr._eig(nr.eigh_topk, A, T)
    r = int(np.argmin(nr.node_scores(A, V, e)))
    dense = nr.delta_h_dense(V, r)
    v, s = V[r], V.sum(axis=0)
    closed = -(2.0 * v * s - v * v)
    scale = np.abs(V).sum(axis=0).max()           # the dense product adds N terms of that size per entry
    print("dense diag vs closed form:", np.abs(np.diag(dense) - closed).max(), "scale", scale)
    assert np.abs(np.diag(dense) - closed).max() <= 64 * np.finfo(np.float64).eps * scale
    assert np.abs(dense - nr.delta_h(V, r)).max() <= 64 * np.finfo(np.float64).eps * scale
    first = np.diag(nr.delta_h(V, r, np.asarray(A[r] @ V).ravel()))
    print("reference shift", closed[:3], "first-order shift", first[:3])
    assert np.abs(closed - first).max() > 1e-3
    # and the restatement applies exactly those
    for shift, want in (("reference", closed), ("first_order", first)):
        _, e1, dV = nr.update(V, e, r, np.asarray(A[r] @ V).ravel(), shift)
        assert np.abs(e1 - (e + want)).max() <= 8 * np.finfo(np.float64).eps * (np.abs(e).max() + scale)
        assert np.max(np.abs(dV)) == 0.0


def two_stars_and_a_path():
    """Two stars of 30 leaves (hubs 0 and 31) and a path on nodes 62..69."""
    n = 70
    A = sp.lil_matrix((n, n))
    for hub in (0, 31):
        for leaf in range(hub + 1, hub + 31):
            A[hub, leaf] = A[leaf, hub] = 1.0
    for i in range(62, 69):
        A[i, i + 1] = A[i + 1, i] = 1.0
    return sp.csr_matrix(A)


def test_the_recomputation_counts_removed_entries():
    """:208, :283-292: edgesRM += 2 deg and a recomputation at >= 50 with
    edgesRM = mod(edgesRM, 50).  Degrees 30, 30: 60 -> recompute, carry 10; 70 ->
    recompute, carry 20; then path nodes of degree 2 and 1: 24, 26, no recomputation."""
    calls = []

    def eig(S, t):
        calls.append(S.nnz)
        return nr.eigh_topk(S, t)

    res = nr.miobi_break_node_ref(two_stars_and_a_path(), 4, 5, eig, refresh=50, forced=[0, 31, 65, 62])
    assert res["degree"].tolist() == [30, 30, 2, 1]
    assert res["wend"].tolist() == [True, True, False, False]
    assert res["acc"].tolist() == [10, 20, 24, 26]
    assert res["refreshes"] == 2 and calls == [134, 74, 14]
    # a step count would have recomputed never (4 < 50); refresh = 0 never does
    calls.clear()
    res0 = nr.miobi_break_node_ref(two_stars_and_a_path(), 4, 5, eig, refresh=0, forced=[0, 31, 65, 62])
    assert res0["refreshes"] == 0 and calls == [134] and not res0["wend"].any()
    # the recomputation after the last step is skipped: the count still wraps
    calls.clear()
    res1 = nr.miobi_break_node_ref(two_stars_and_a_path(), 1, 5, eig, refresh=50, forced=[0])
    assert res1["wend"].tolist() == [True] and res1["acc"].tolist() == [10] and res1["refreshes"] == 0
    assert calls == [134]


def test_isolated_nodes_inf_or_sum():
    """The second loop scores a node without entries +Inf (:199-201); the first
    loop's empty sum gives exp(0) = 1 per term: exactly sum(exp(e)) (:70-79)."""
    A = two_stars_and_a_path()
    live = np.ones(70, dtype=bool)
    live[0] = False                                # the hub gone: its 30 leaves and itself are isolated
    M = nr.current(A, live)
    e, V = nr._eig(nr.eigh_topk, A, 5)
    inf = nr.node_scores(M, V, e, "inf")
    tot = nr.node_scores(M, V, e, "sum")
    iso = np.diff(M.indptr) == 0
    assert iso.sum() == 31 and np.isinf(inf[iso]).all() and np.isfinite(inf[~iso]).all()
    ones = np.sum(np.exp(e)[None, :] * np.ones((70, 1)), axis=1)
    assert (tot[iso] == ones[iso]).all() and (tot[~iso] == inf[~iso]).all()
    for n in (0, 5, 31, 40, 64):
        for rule in ("inf", "sum"):
            lit = nr.node_score_literal(M, V, e, n, rule)
            vec = nr.node_scores(M, V, e, rule)[n]
            assert lit == vec or abs(lit - vec) <= 1e-14 * abs(vec), (n, rule, lit, vec)
    assert nr.node_score_literal(M, V, e, 0, "sum") == float(np.sum(np.exp(e)))
    # under "sum" an isolated node can be the minimum and is then removed with degree 0
    res = nr.miobi_break_node_ref(A, 3, 5, nr.eigh_topk, refresh=0, isolated="sum")
    assert res["nsel"] == 3 and (res["degree"] >= 0).all()


def test_an_exact_tie_goes_to_the_lower_node():
    """The two hubs carry the same rows in a hand-made V: min() takes node 0."""
    A = two_stars_and_a_path()

    def eig(S, t):
        V = np.full((70, t), 0.01)
        V[[0, 31]] = 0.5
        V[62:] = 0.001
        return np.array([3.0, 2.0, 1.0][:t]), V

    res = nr.miobi_break_node_ref(A, 2, 3, eig, refresh=0)
    assert res["gap"][0] == 0.0 and res["nodes"].tolist() == [0, 31]


def test_abi_rejects_bad_arguments_before_the_device():
    import ctypes as C
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sig["kt_miobi_break_node"]) == 15 and len(sig["kt_nodes_score_topk"]) == 5
    ns = C.c_int64()
    for t in (1, 25, 33):  # a NULL matrix, whatever t
        assert lib.kt_miobi_break_node(None, 3, t, 50, 0, 0.0, 0, 0, None, None, None, None, C.byref(ns),
                                       None, None) == _lib.KT_ERR_ARG
        assert b"kt_miobi_break_node" in lib.kt_last_error()
        assert lib.kt_nodes_score_topk(None, t, None, None, None) == _lib.KT_ERR_ARG
        assert b"kt_nodes_score_topk" in lib.kt_last_error()


def test_kernel_check_host_enumeration():
    """tests/native/miobi_node_check --host: the cases the device run is held to."""
    import json
    import os
    import subprocess
    from conftest import ROOT
    check = os.path.join(ROOT, "tests", "native", "miobi_node_check", "miobi_node_check")
    assert os.path.exists(check), "tests/native/miobi_node_check/miobi_node_check is not built (__graft_entry__.build())"
    r = subprocess.run([check, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mode"] == "host" and out["max_score_err_over_bound"] <= 1.0
    cases = {g: v["cases"] for g, v in out["groups"].items()}
    assert all(v["failed_count"] == 0 for v in out["groups"].values())
    assert cases["score"] >= 24 + 12 and cases["pick"] >= 24 and cases["apply"] >= 20 and cases["colsum"] >= 4
    assert sum(cases.values()) <= 300  # a few dozen per group, not a sweep

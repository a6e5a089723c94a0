"""kt_trace_fun_update_nodes / kt_krylov_break_node on the device (DESIGN.md
§4.2h) against the NumPy restatement (tests/nodes_ref.py) and exact dense
eigenvalue differences.

Bounds.  Against the restatement: rel 1e-7, abs tol, the oracle convention of
tests/test_gpu_greedy.py (the iterates may differ by a step where the stop
decision was marginal: conftest.iter_matches).  Against exact: 1e-8 relative at
tol = 1e-9 |exact|, the convention of tests/test_nodes_host.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import iter_matches, load_graph

import nodes_ref as nr
GRAPHS = ("anaheim", "india", "rome", "oregon_A0")


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


@pytest.fixture(scope="module")
def cases():
    """Per graph: A, eigvalsh(A), the node set (0-based), the exact differences."""
    out = {}
    for g in GRAPHS:
        A = load_graph(g)
        w = np.linalg.eigvalsh(A.toarray())
        nodes, iso = nr.node_set(A)
        out[g] = {"A": A, "w": w, "nodes": nodes, "iso": iso,
                  "exact": {i: nr.exact_update(A, i, "exp", w) for i in nodes}}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRAPHS)
def test_device_matches_restatement_and_exact(kra, gpu_ctx, cases, g):
    c = cases[g]
    D = kra.DeviceMatrix(c["A"], gpu_ctx)
    worst = 0.0
    for i in c["nodes"]:
        ex = c["exact"][i]
        tol = 1e-9 * abs(ex)
        xm, it, lk = kra.trace_fun_update_nodes(D, [i + 1], tol, fun="exp", ctx=gpu_ctx)
        xr, ir, lr, _, _, hist = nr.node_update(c["A"], i, tol, fun="exp", keep=True)
        print(g, "node", i, "device", xm[0], int(it[0]), int(lk[0]), "restatement", xr, ir, lr, "exact", ex)
        assert xm[0] == pytest.approx(xr, rel=1e-7, abs=tol)
        assert abs(xm[0] - ex) <= 1e-8 * abs(ex)
        worst = max(worst, abs(xm[0] - ex) / abs(ex))
        assert iter_matches(it[0], ir, hist, tol), (g, i, int(it[0]), ir, hist[-3:])
        assert lk[0] == lr == 0
    print(g, "worst relative error against exact", worst)
    if c["iso"] is not None:
        xm, it, lk = kra.trace_fun_update_nodes(D, [c["iso"] + 1], 1e-12, ctx=gpu_ctx)
        assert (xm[0], it[0], lk[0]) == (0.0, 1, 1)


@pytest.mark.gpu
def test_dense_branch(kra, gpu_ctx):
    A = load_graph("denmark")
    assert A.shape[0] == 96
    nodes, _ = nr.node_set(A)
    w = np.linalg.eigvalsh(A.toarray())
    xm, it, lk = kra.trace_fun_update_nodes(A, np.array(nodes) + 1, ctx=gpu_ctx)
    for h, i in enumerate(nodes):
        ex = nr.exact_update(A, i, "exp", w)
        assert xm[h] == pytest.approx(ex, rel=1e-10)
        assert it[h] == 0 and lk[h] == 0


@pytest.mark.gpu
def test_values_do_not_depend_on_the_call(kra, gpu_ctx, cases):
    """40 candidates: three sweeps, the last partial, one node twice."""
    c = cases["india"]
    A = c["A"]
    deg = np.diff(A.indptr)
    order = np.argsort(-deg, kind="stable")
    nodes = [int(i) for i in order[:37]] + [c["iso"], c["nodes"][4], int(order[3])]
    assert len(nodes) == 40 and len(set(nodes)) == 39
    tol = 1e-9
    D = kra.DeviceMatrix(A, gpu_ctx)
    one = np.array(nodes) + 1
    xm, it, lk = kra.trace_fun_update_nodes(D, one, tol, ctx=gpu_ctx)
    xm2, it2, lk2 = kra.trace_fun_update_nodes(D, one, tol, ctx=gpu_ctx)
    xr, itr, lkr = kra.trace_fun_update_nodes(D, one[::-1], tol, ctx=gpu_ctx)
    for a, b in ((xm, xm2), (it, it2), (lk, lk2), (xm, xr[::-1]), (it, itr[::-1]), (lk, lkr[::-1])):
        assert a.tobytes() == np.ascontiguousarray(b).tobytes()
    for h, i in enumerate(nodes):
        x1, i1, l1 = kra.trace_fun_update_nodes(D, [i + 1], tol, ctx=gpu_ctx)
        assert (x1[0].tobytes(), int(i1[0]), int(l1[0])) == (xm[h].tobytes(), int(it[h]), int(lk[h])), (h, i)
    assert xm[39] == xm[3] and lk[37] == 1 and xm[37] == 0.0
    assert gpu_ctx.stat(13) == 1 and gpu_ctx.stat(15) == int(it[39])  # the last call: one sweep


@pytest.mark.gpu
@pytest.mark.parametrize("fun", ["cosh", "sinh"])
def test_cosh_and_sinh(kra, gpu_ctx, cases, fun):
    c = cases["anaheim"]
    D = kra.DeviceMatrix(c["A"], gpu_ctx)
    for i in c["nodes"][:3]:
        ex = nr.exact_update(c["A"], i, fun, c["w"])
        xm, it, _ = kra.trace_fun_update_nodes(D, [i + 1], 1e-9 * abs(ex), fun=fun, ctx=gpu_ctx)
        print(fun, "node", i, "device", xm[0], int(it[0]), "exact", ex)
        assert abs(xm[0] - ex) <= 1e-8 * abs(ex)


@pytest.mark.gpu
def test_a_diagonal_entry_at_the_node(kra, gpu_ctx, cases):
    c = cases["anaheim"]
    i = c["nodes"][0]
    A = nr.diag_copy(c["A"], i)
    ex = nr.exact_update(A, i, "exp")
    xm, it, _ = kra.trace_fun_update_nodes(A, [i + 1], 1e-9 * abs(ex), ctx=gpu_ctx)
    print("diag copy node", i, "device", xm[0], int(it[0]), "exact", ex)
    assert abs(xm[0] - ex) <= 1e-8 * abs(ex)


@pytest.mark.gpu
def test_oregon_hubs_at_the_greedy_tolerance(kra, gpu_ctx, cases):
    """tol = 1e-6 exp(lambda_1), the scale of default_greedy_tol: the check's
    comparison runs at exp(-theta_max) and must neither overflow nor stall."""
    c = cases["oregon_A0"]
    A = c["A"]
    hubs = c["nodes"][:3]
    assert [int(d) for d in np.diff(A.indptr)[hubs]] == [206, 185, 157]
    tol = 1e-6 * float(np.exp(c["w"][-1]))
    xm, it, lk = kra.trace_fun_update_nodes(A, np.array(hubs) + 1, tol, ctx=gpu_ctx)
    for h, i in enumerate(hubs):
        print("hub", i, "device", xm[h], int(it[h]), "exact", c["exact"][i], "tol", tol)
        assert np.isfinite(xm[h]) and abs(xm[h] - c["exact"][i]) <= 10.0 * tol
        assert 3 <= it[h] < 100 and lk[h] == 0


@pytest.mark.gpu
def test_krylov_break_node(kra, gpu_ctx, cases):
    c = cases["anaheim"]
    A = c["A"]
    deg = np.diff(A.indptr)
    cand = [int(i) for i in np.argsort(-deg, kind="stable")[:40]]
    tol = 1e-10
    D = kra.DeviceMatrix(A, gpu_ctx)
    nnz0 = D.nnz
    nodes, rob, D2, info = kra.krylov_break_node(D, 3, np.array(cand) + 1, tol, ctx=gpu_ctx)
    assert D2 is D and len(nodes) == 3 and len(set(nodes.tolist())) == 3
    sel = [int(v) - 1 for v in nodes]
    # the restatement driven along the device's selections
    _, steps, rob_ref, A_ref = nr.krylov_break_node_ref(A, 3, cand, tol, forced=sel)
    removed = 0
    M = sp.csr_matrix(A)
    for s, step in enumerate(steps):
        xs = dict(step)
        assert info["xm"][s] == pytest.approx(xs[sel[s]], rel=1e-7, abs=tol)
        assert xs[sel[s]] <= min(xs.values()) + tol, (s, sel[s], xs[sel[s]], min(xs.values()))
        removed += int(np.diff(M.indptr)[sel[s]])
        M = nr.remove_node(M, sel[s])
    An = sp.csr_matrix(D.to_scipy())
    An.eliminate_zeros()
    assert abs(An - A_ref).nnz == 0 and abs(An - M).nnz == 0
    assert D.nnz == An.nnz == nnz0 - 2 * removed
    ex = float(np.sum(np.exp(np.linalg.eigvalsh(A_ref.toarray()))) - np.sum(np.exp(c["w"])))
    print("rob", rob, "restatement", rob_ref, "exact", ex, "selected", sel, "xm", info["xm"])
    assert rob == pytest.approx(float(np.sum(info["xm"])), rel=1e-14)
    assert abs(rob - ex) <= 1e-8 * abs(ex)
    # k larger than the list
    nodes2, rob2, _, info2 = kra.krylov_break_node(A, 5, np.array(cand[:2]) + 1, tol, ctx=gpu_ctx)
    assert len(nodes2) == 2 and sorted(nodes2.tolist()) == sorted(v + 1 for v in cand[:2]) and len(info2["xm"]) == 2
    nodes3, rob3, _, _ = kra.krylov_break_node(A, 0, np.array(cand[:2]) + 1, tol, ctx=gpu_ctx)
    assert len(nodes3) == 0 and rob3 == 0.0


@pytest.mark.gpu
def test_abi_rejects_a_node_index_equal_to_n(kra, gpu_ctx, cases):
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    A = cases["anaheim"]["A"]
    D = kra.DeviceMatrix(A, gpu_ctx)
    n = A.shape[0]
    nodes = (C.c_int64 * 2)(0, n)
    xm = (C.c_double * 2)()
    ns = C.c_int64()
    assert lib.kt_trace_fun_update_nodes(D.handle, 2, nodes, 1e-9, 0, 0, xm, None, None) == _lib.KT_ERR_ARG
    assert b"node index out of range" in lib.kt_last_error()
    assert lib.kt_krylov_break_node(D.handle, 1, 2, nodes, 1e-9, 0, 0, nodes, xm, None, C.byref(ns)) == _lib.KT_ERR_ARG
    assert lib.kt_trace_fun_update_nodes(D.handle, 2, None, 1e-9, 0, 0, xm, None, None) == _lib.KT_ERR_ARG
    nodes[1] = n - 1
    assert lib.kt_trace_fun_update_nodes(D.handle, 2, nodes, 1e-9, 0, 0, xm, None, None) == _lib.KT_OK
    assert D.nnz == A.nnz

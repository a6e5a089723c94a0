"""CPU tests of the node-removal trace update: the NumPy
restatement (tests/nodes_ref.py) against exact dense eigenvalue differences,
the host value function kt_host_node_update against NumPy, the finding that
the block route through trace_fun_update converges to a wrong value, and the
new ABI entries' argument checks without a device.

Bounds.  Restatement against exact: 1e-8 relative at tol = 1e-9 |exact| (the
exact-answer convention of the golden a5 row); worst measured 7.6e-12.
kt_host_node_update against NumPy: ten times "spread_max" of
tests/golden/adaptive_values.json (the host QL against numpy.linalg.eigh on
Lanczos tridiagonals), relative to sum |f(eig(T_j))|, as
tests/test_gpu_quad_check.py holds the device QL."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, load_graph

import nodes_ref as nr

GRAPHS = ("anaheim", "india", "rome", "oregon_A0")
with open(os.path.join(GOLDEN, "adaptive_values.json")) as _f:
    QL_TOL = 10.0 * json.load(_f)["spread_max"]


@pytest.fixture(scope="module")
def cases():
    """Per graph: A, eigvalsh(A), the node set and the exact differences."""
    out = {}
    for g in GRAPHS:
        A = load_graph(g)
        w = np.linalg.eigvalsh(A.toarray())
        nodes, iso = nr.node_set(A)
        out[g] = {"A": A, "w": w, "nodes": nodes, "iso": iso,
                  "exact": {i: nr.exact_update(A, i, "exp", w) for i in nodes}}
    return out


def test_india_has_an_isolated_node(cases):
    assert cases["india"]["iso"] is not None
    assert all(len(c["nodes"]) == 6 for c in cases.values())


@pytest.mark.parametrize("g", GRAPHS)
def test_restatement_matches_the_exact_difference(cases, g):
    c = cases[g]
    worst, deepest = 0.0, 0
    for i in c["nodes"]:
        ex = c["exact"][i]
        xm, it, lucky = nr.node_update(c["A"], i, tol=1e-9 * abs(ex), fun="exp")
        err = abs(xm - ex) / abs(ex)
        print(g, "node", i, "exact", ex, "restatement", xm, "iter", it, "lucky", lucky, "rel err", err)
        worst, deepest = max(worst, err), max(deepest, it)
        assert err <= 1e-8, (g, i, xm, ex, err)
        assert 3 <= it <= 40 and ex < 0.0
    print(g, "worst", worst, "deepest", deepest)


def test_an_isolated_node_stops_after_one_step(cases):
    c = cases["india"]
    xm, it, lucky = nr.node_update(c["A"], c["iso"], tol=1e-12)
    assert (xm, it, lucky) == (0.0, 1, 1)
    assert nr.exact_update(c["A"], c["iso"], "exp", c["w"]) == 0.0


@pytest.mark.parametrize("fun", ["cosh", "sinh"])
def test_cosh_and_sinh(cases, fun):
    """cosh(0) = 1: a missing f(0) term is an absolute error of 1."""
    c = cases["anaheim"]
    for i in c["nodes"][:3]:
        ex = nr.exact_update(c["A"], i, fun, c["w"])
        xm, it, _ = nr.node_update(c["A"], i, tol=1e-9 * abs(ex), fun=fun)
        print(fun, "node", i, "exact", ex, "restatement", xm, "iter", it)
        assert abs(xm - ex) <= 1e-8 * abs(ex)


def test_a_diagonal_entry_at_the_node(cases):
    """T_1 = [A_ii]; the update removes the diagonal entry with the row."""
    c = cases["anaheim"]
    i = c["nodes"][0]
    A = nr.diag_copy(c["A"], i)
    al, _ = nr.lanczos_tridiag(A, i, 1)
    assert al[0] == 0.75
    ex = nr.exact_update(A, i, "exp")
    xm, it, _ = nr.node_update(A, i, tol=1e-9 * abs(ex))
    print("diag copy node", i, "exact", ex, "restatement", xm, "iter", it)
    assert abs(xm - ex) <= 1e-8 * abs(ex)
    assert abs(ex - c["exact"][i]) > 1e-3 * abs(ex)  # the entry matters


def test_host_value_function_matches_numpy(cases):
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    worst, reached = 0.0, set()
    for g in GRAPHS:
        c = cases[g]
        for i in c["nodes"][:2] + c["nodes"][4:5]:
            al, off = nr.lanczos_tridiag(c["A"], i, 128)
            for j in (1, 2, 3, 8, 31, 32, 128):
                if j > len(al):
                    continue
                reached.add(j)
                a = np.ascontiguousarray(al[:j])
                o = np.ascontiguousarray(np.concatenate([off[:j - 1], [0.0]]))
                for fun in ("exp", "cosh"):
                    x = C.c_double()
                    assert lib.kt_host_node_update(j, a.ctypes.data_as(dp), o.ctypes.data_as(dp),
                                                   _lib.FUN_CODES[fun], C.byref(x)) == _lib.KT_OK
                    want = nr.x_of_tridiag(a, o[:j - 1], fun)
                    scale = float(np.sum(np.abs(nr.FUNS[fun](np.linalg.eigvalsh(nr.tridiag(a, o[:j - 1]))))))
                    err = abs(x.value - want) / scale
                    worst = max(worst, err)
                    assert err <= QL_TOL, (g, i, j, fun, x.value, want, err)
    print("worst |host - numpy| / sum|f(d2)|", worst, "tolerance", QL_TOL)
    assert reached == {1, 2, 3, 8, 31, 32, 128}
    x = C.c_double()
    a = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    assert lib.kt_host_node_update(1, a, None, _lib.FUN_CODES["exp"], C.byref(x)) == _lib.KT_OK and x.value == 0.0
    for bad in ((0, "exp"), (257, "exp"), (2, "log")):
        assert lib.kt_host_node_update(bad[0], a, a, _lib.FUN_CODES[bad[1]], C.byref(x)) == _lib.KT_ERR_ARG


@pytest.mark.parametrize("g,node,off_by", [("rome", 1754, 0.01), ("oregon_A0", 6, 1.0)])
def test_the_block_route_converges_to_a_wrong_value(cases, g, node, off_by):
    """trace_fun_update with U = [e_i, a_i], B = [[-A_ii, -1], [-1, 0]]: a_i =
    A e_i - A_ii e_i makes every block of the block Lanczos run rank-deficient;
    the qr completions bring non-Krylov directions in and the value it
    converges to is wrong.  The single-vector restatement is right."""
    from oracle import krylov_oracle as ko
    c = cases[g]
    A, n = c["A"], c["A"].shape[0]
    ai = np.asarray(A[:, node].todense()).ravel()
    aii = ai[node]
    ai[node] = 0.0
    e = np.zeros(n)
    e[node] = 1.0
    U = np.stack([e, ai], axis=1)
    B = np.array([[-aii, -1.0], [-1.0, 0.0]])
    hist = []
    xo, it, lucky = ko.trace_fun_update(A, U, B, tol=1e-12, it=30, fun="exp", hist=hist)
    ex = nr.exact_update(A, node, "exp", c["w"])
    rel = abs(xo - ex) / abs(ex)
    print(g, "node", node, "oracle", xo, "iter", it, "lucky", lucky, "exact", ex, "rel", rel)
    assert len(hist) >= 3 and abs(hist[-1][2] - hist[-2][2]) <= 1e-6 * abs(xo)  # it has settled
    assert rel > off_by
    xm, _, _ = nr.node_update(A, node, tol=1e-9 * abs(ex))
    assert abs(xm - ex) <= 1e-8 * abs(ex)


def test_greedy_restatement_on_a_small_graph():
    """Two stars and a path (n > 130): the bigger hub goes first, and rob is
    the exact trace difference."""
    n = 140
    A = sp.lil_matrix((n, n))
    for hub, leaves in ((0, 60), (61, 40)):
        for leaf in range(hub + 1, hub + 1 + leaves):
            A[hub, leaf] = A[leaf, hub] = 1.0
    for i in range(110, 139):
        A[i, i + 1] = A[i + 1, i] = 1.0
    A = sp.csr_matrix(A)
    sel, steps, rob, A1 = nr.krylov_break_node_ref(A, 5, [120, 61, 0], tol=1e-12)
    assert sel == [0, 61, 120] and len(steps) == 3
    ex = np.sum(np.exp(np.linalg.eigvalsh(A1.toarray()))) - np.sum(np.exp(np.linalg.eigvalsh(A.toarray())))
    assert abs(rob - ex) <= 1e-8 * abs(ex)
    assert A1.nnz == A.nnz - 2 * (60 + 40 + 2)


def test_abi_rejects_bad_arguments_before_the_device():
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sig["kt_trace_fun_update_nodes"]) == 9 and len(sig["kt_krylov_break_node"]) == 11
    assert len(sig["kt_host_node_update"]) == 5
    nodes = (C.c_int64 * 2)(0, 1)
    xm = (C.c_double * 2)()
    ns = C.c_int64()
    exp, log = _lib.FUN_CODES["exp"], _lib.FUN_CODES["log"]
    assert lib.kt_trace_fun_update_nodes(None, 2, nodes, 1e-9, 30, exp, xm, None, None) == _lib.KT_ERR_ARG
    assert b"kt_trace_fun_update_nodes: NULL" in lib.kt_last_error()
    assert lib.kt_trace_fun_update_nodes(None, 2, nodes, 1e-9, 30, log, xm, None, None) == _lib.KT_ERR_ARG
    assert b"log" in lib.kt_last_error()
    assert lib.kt_trace_fun_update_nodes(None, 2, nodes, 1e-9, 257, exp, xm, None, None) == _lib.KT_ERR_ARG
    assert b"256" in lib.kt_last_error()
    assert lib.kt_krylov_break_node(None, 1, 2, nodes, 1e-9, 30, exp, nodes, xm, None, C.byref(ns)) == _lib.KT_ERR_ARG
    assert b"kt_krylov_break_node: NULL" in lib.kt_last_error()
    assert lib.kt_krylov_break_node(None, 1, 2, nodes, 1e-9, 257, exp, nodes, xm, None, C.byref(ns)) == _lib.KT_ERR_ARG
    assert lib.kt_krylov_break_node(None, 1, 2, nodes, 1e-9, 30, log, nodes, xm, None, C.byref(ns)) == _lib.KT_ERR_ARG


def test_python_rejects_bad_arguments_without_a_device(monkeypatch):
    """fun = log, it = 257 and a node index equal to n (1-based: n + 1) never
    reach the device."""
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import greedy

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(greedy, "_dev", no_device)
    A = load_graph("anaheim")
    n = A.shape[0]
    for call in (lambda **kw: kra.trace_fun_update_nodes(A, kw.pop("nodes", [1, 2]), **kw),
                 lambda **kw: kra.krylov_break_node(A, 2, kw.pop("nodes", [1, 2]), **kw)):
        for kw in ({"fun": "log"}, {"it": 257}, {"nodes": [1, n + 1]}, {"nodes": [0]}):
            with pytest.raises(kra.KrylovError) as e:
                call(**kw)
            assert e.value.code == kra._lib.KT_ERR_ARG
        with pytest.raises(AssertionError, match="a device was touched"):
            call(nodes=[1, n])  # valid arguments go on to the device

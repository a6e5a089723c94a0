"""CPU: the adaptive Lanczos depth's stopping rule (kt_host_quad_converged,
pure host code) on the numpy oracle's tridiagonals."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, load_graph
from oracle import krylov_oracle as ko

with open(os.path.join(GOLDEN, "adaptive_values.json")) as _f:
    FIX = json.load(_f)
RTOL = FIX["rtol_default"]


def grid_graph(a, b):
    pa = sp.diags([np.ones(a - 1), np.ones(a - 1)], [-1, 1])
    pb = sp.diags([np.ones(b - 1), np.ones(b - 1)], [-1, 1])
    return sp.csr_matrix(sp.kron(sp.identity(b), pa) + sp.kron(pb, sp.identity(a)))


def rule(j, al, off, want=0, rtol=RTOL, fun=0):
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    cv, q = C.c_int(-1), C.c_double(np.nan)
    a = np.ascontiguousarray(al[:j], dtype=np.float64)
    o = np.ascontiguousarray(off[:j if want else j - 1], dtype=np.float64)
    st = lib.kt_host_quad_converged(j, a.ctypes.data_as(_lib._dp), o.ctypes.data_as(_lib._dp) if o.size else None,
                                    fun, want, rtol, C.byref(cv), C.byref(q))
    return st, cv.value, q.value


def test_default_rtol_is_the_measured_one():
    """Ten times the smallest power of ten at which every column of the
    fixture's graphs stops before depth 128 (profiles/adaptive/rtol_sweep.txt)."""
    assert FIX["rtol_default"] == pytest.approx(10.0 * FIX["rtol_smallest_all_stop"])
    k = FIX["rtols"].index(FIX["rtol_smallest_all_stop"])
    for g, sw in FIX["sweep"].items():
        assert sw["quad"][k] is not None and sw["fmv"][k] is not None and max(sw["quad"][k], sw["fmv"][k]) < 128, g
    assert any(sw["fmv"][k + 1] is None or sw["quad"][k + 1] is None for sw in FIX["sweep"].values())


@pytest.mark.parametrize("name", ["anaheim", "grid40_x16"])
@pytest.mark.parametrize("want", [0, 1])
def test_first_converged_depth_is_converged(name, want):
    """At the first depth j the rule holds, the oracle's quadrature differs
    from its value at depth 2j by at most 10 rtol (relative)."""
    A = load_graph("anaheim") if name == "anaheim" else grid_graph(40, 40) * 16.0
    Z = ko.rademacher(A.shape[0], np.arange(3), 0)
    for c in range(3):
        al, off, _, lucky = ko.lanczos_probe_tridiag(A, Z[:, c], 160)
        assert not lucky
        first = None
        for j in range(1, 80):
            st, cv, q = rule(j, al, off, want)
            assert st == 0 and np.isfinite(q)
            if j < 8:
                assert cv == 0
            if cv:
                first = j
                break
        assert first is not None and first >= 8, (name, c)
        if name == "grid40_x16":
            assert rule(8, al, off, want)[1] == 0 and first > 8
        qj = ko.tridiag_quadrature(al[:first], off[:first - 1])
        q2 = ko.tridiag_quadrature(al[:2 * first], off[:2 * first - 1])
        print(name, "column", c, "fe1" if want else "quad", "first depth", first, "rel diff to 2j", abs(qj / q2 - 1))
        assert abs(qj - q2) <= 10 * RTOL * abs(q2), (name, c, first, abs(qj / q2 - 1))


def test_lucky_breakdown_stops_at_depth_one():
    """Started from an eigenvector of a path graph, beta_1 ~ 0: the column
    stops at depth 1 with q = f(alpha_0) (exp: scaled by exp(-theta_max) = 1)."""
    n = 50
    A = sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1]).tocsr()
    w, V = np.linalg.eigh(A.toarray())
    v = V[:, -3]
    a0 = float(v @ (A @ v))
    b1 = float(np.linalg.norm(A @ v - a0 * v))
    assert b1 < 1e-8
    st, cv, q = rule(1, [a0], [b1], want=1)          # depth 1, the next off-diagonal known
    assert (st, cv) == (0, 1) and q == pytest.approx(1.0, abs=1e-15)
    st, cv, q = rule(2, [a0, 0.3], [b1])             # depth 2: T is cut back to depth 1
    assert (st, cv) == (0, 1) and q == pytest.approx(1.0, abs=1e-15)
    st, cv, q = rule(2, [a0, 0.3], [b1], fun=3)      # sin: unscaled
    assert (st, cv) == (0, 1) and q == pytest.approx(np.sin(a0), rel=1e-14)


def test_exp_scaling_keeps_a_large_spectrum_finite():
    k = np.arange(40)
    al = 600.0 + 20.0 * np.cos(0.9 * k)
    off = 150.0 + 10.0 * np.sin(0.4 * k)
    T = np.diag(al[:30]) + np.diag(off[:29], 1) + np.diag(off[:29], -1)
    assert np.linalg.eigvalsh(T).max() > 850
    for want in (0, 1):
        st, cv, q = rule(30, al, off, want)
        assert st == 0 and cv in (0, 1) and np.isfinite(q) and 0 < q <= 1.0
    w, V = np.linalg.eigh(T)
    assert q == pytest.approx(float(np.sum(V[0] ** 2 * np.exp(w - w.max()))), rel=1e-11)


def test_null_and_size_one_arguments_return_a_status():
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    cv, q = C.c_int(), C.c_double()
    one = (C.c_double * 1)(0.5)
    assert lib.kt_host_quad_converged(1, one, None, 0, 0, 1e-12, C.byref(cv), C.byref(q)) == _lib.KT_OK
    assert cv.value == 0 and q.value == pytest.approx(1.0)
    for args in ((1, None, None, 0, 0, 1e-12, C.byref(cv), C.byref(q)),
                 (1, one, None, 0, 1, 1e-12, C.byref(cv), C.byref(q)),     # fe1 needs beta_1
                 (2, one, None, 0, 0, 1e-12, C.byref(cv), C.byref(q)),
                 (0, one, one, 0, 0, 1e-12, C.byref(cv), C.byref(q)),
                 (257, one, one, 0, 0, 1e-12, C.byref(cv), C.byref(q)),
                 (1, one, one, 9, 0, 1e-12, C.byref(cv), C.byref(q)),
                 (1, one, one, 0, 0, 1e-12, None, C.byref(q)),
                 (1, one, one, 0, 0, 1e-12, C.byref(cv), None)):
        assert lib.kt_host_quad_converged(*args) == _lib.KT_ERR_ARG, args
        assert b"kt_host_quad_converged" in lib.kt_last_error()

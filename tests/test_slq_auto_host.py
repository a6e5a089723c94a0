"""Host side of the error-controlled probe sweeps (kt_slq_trace_auto): the
ctypes row, the argument errors that need no device, and the stopping depths
the GPU tests rely on, reproduced from the oracle's tridiagonals with the
host restatement of the rule (kt_host_quad_converged) at the default rtol.

Depth table (Rademacher probes 0..31 of seed 0; errors against depth 128,
the last graph against depth 256 with 8 probes).  The stopping depths are
pinned to what kt_host_quad_converged gives, which are the issue's figures
with ONE departure: rome_x16 stops at 32..34 where the issue's table, from a
numpy restatement of the rule (numpy.linalg.eigh where the library runs its
QL), has 32..33 -- one probe's decision at depth 33 is marginal.  The error
columns are held to the table's order of magnitude: at most ten times its
figure, and, where the figure is above the quadrature's own rounding
(1e-12), at least a tenth of it."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph
from oracle import krylov_oracle as ko

RTOL = 1e-12

# graph: (stopping depth min, max, probes, depth the error is measured against,
#         the table's max error at the stopping depth, its max error of a fixed m = 30 form
#         (None: not in the table), its min error of a fixed m = 30 form (None: not given))
TABLE = {
    "anaheim": (12, 12, 32, 128, 6e-15, 4e-15, None),
    "oregon_A0": (15, 17, 32, 128, 7e-14, 6e-14, None),
    "cl20k": (17, 22, 32, 128, 1.3e-13, 8e-14, None),
    "cl200k": (18, 22, 32, 128, 2.3e-13, 2e-13, None),
    "anaheim_x16": (30, 33, 32, 128, 3e-14, 5e-12, None),
    "rome_x16": (32, 34, 32, 128, 2e-13, 8e-12, None),  # the issue's table: 32..33 (see above)
    "grid40_x16": (34, 35, 32, 128, 4e-14, 4e-11, None),
    "rome_x40": (46, 51, 32, 128, 2e-13, 6.8e-4, 3e-6),
    "grid40_x40": (51, 53, 32, 128, 1.4e-13, 2.5e-4, 5e-5),
    "grid40_x150": (90, 94, 8, 256, 6e-13, None, None),
}


def grid_graph(a, b):
    pa = sp.diags([np.ones(a - 1), np.ones(a - 1)], [-1, 1])
    pb = sp.diags([np.ones(b - 1), np.ones(b - 1)], [-1, 1])
    return sp.csr_matrix(sp.kron(sp.identity(b), pa) + sp.kron(pb, sp.identity(a)))


def graph(name):
    if name in ("cl20k", "cl200k"):
        from krylov_robustness_amd import graphs
        n = 20_000 if name == "cl20k" else 200_000
        return sp.csr_matrix(graphs.chung_lu(n, 10 * n, seed=0))
    A = grid_graph(40, 40) if name.startswith("grid40") else load_graph(name.split("_x")[0])
    return sp.csr_matrix(A * float(name.split("_x")[1])) if "_x" in name else sp.csr_matrix(A)


def converged(j, al, off, rtol=RTOL):
    from krylov_robustness_amd import _lib
    cv, q = C.c_int(-1), C.c_double()
    a, o = np.ascontiguousarray(al[:j]), np.ascontiguousarray(off[:j - 1])
    st = _lib.load().kt_host_quad_converged(j, a.ctypes.data_as(_lib._dp), o.ctypes.data_as(_lib._dp), 0, 0, rtol,
                                            C.byref(cv), C.byref(q))
    assert st == 0
    return bool(cv.value)


@pytest.mark.parametrize("name", list(TABLE))
def test_stopping_depths_of_the_issue_table(name):
    dmin, dmax, nprobes, deep, e_stop, e30_max, e30_min = TABLE[name]
    A = graph(name)
    Z = ko.rademacher(A.shape[0], np.arange(nprobes), 0)
    depths, errs, errs30 = [], [], []
    for c in range(nprobes):
        al, off, _, lucky = ko.lanczos_probe_tridiag(A, Z[:, c], deep)
        assert not lucky
        d = next(j for j in range(8, deep + 1) if converged(j, al, off))
        depths.append(d)
        q_deep = ko.tridiag_quadrature(al, off)
        errs.append(abs(ko.tridiag_quadrature(al[:d], off[:d - 1]) / q_deep - 1.0))
        errs30.append(abs(ko.tridiag_quadrature(al[:30], off[:29]) / q_deep - 1.0))
    print(name, "depths", min(depths), max(depths), "err at the stop", max(errs), "err of m = 30", min(errs30),
          max(errs30))
    assert (min(depths), max(depths)) == (dmin, dmax)
    assert max(errs) <= 10 * e_stop, max(errs)
    if e30_max is not None:
        assert max(errs30) <= 10 * e30_max, max(errs30)
        if e30_max >= 1e-12:
            assert max(errs30) >= e30_max / 10, max(errs30)
    if e30_min is not None:  # where test_gpu_slq_auto.py wants the fixed m = 30 forms to drift
        assert e30_min / 10 <= min(errs30) and min(errs30) >= 3e-6, min(errs30)


def test_no_probe_stops_at_rtol_1e_17_on_grid40_x150():
    """The handover test's premise: at rtol = 1e-17 no probe of 0..15 stops at
    any depth 8..160."""
    A = graph("grid40_x150")
    Z = ko.rademacher(A.shape[0], np.arange(16), 0)
    for c in range(16):
        al, off, _, lucky = ko.lanczos_probe_tridiag(A, Z[:, c], 160)
        assert not lucky and len(al) == 160
        assert not any(converged(j, al, off, 1e-17) for j in range(8, 161)), c


def test_ctypes_row_and_deviceless_errors():
    from krylov_robustness_amd import _lib
    import krylov_robustness_amd as kra
    row = [r for r in _lib.SIGNATURES if r[0] == "kt_slq_trace_auto"]
    assert len(row) == 1
    _, res, args = row[0]
    assert res is C.c_int
    assert args == [_lib._mat_p, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_int64, C.c_int64, C.c_int,
                    _lib._dp, _lib._dp, _lib._dp, _lib._ip, _lib._i64p]
    lib = _lib.load()
    s = C.c_double()
    assert lib.kt_slq_trace_auto(None, 0, 128, 1e-12, 0, 0, 4, 0, C.byref(s), C.byref(s), None, None,
                                 None) == _lib.KT_ERR_ARG
    assert b"NULL" in lib.kt_last_error()
    assert _lib.load().kt_abi_version() == 3
    assert callable(kra.slq_quadforms_auto) and callable(kra.slq_trace_auto)

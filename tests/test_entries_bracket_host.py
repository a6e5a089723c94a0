"""CPU tests of the Gauss / Gauss-Radau bracket of exp(A)_ij:
the NumPy restatement (tests/entries_bracket_ref.py) against dense eigh, its
stopping rule on the tests' pair set, and the argument checks of
kt_entries_fun_bracket and its wrappers without a device.

Bracket slack.  lo <= exact <= hi and the monotonicity of both bounds hold up
to rounding, whose unit is (exp(A)_ii + exp(A)_jj) / 2 -- the size of the two
quadratic forms whose difference the entry is -- not exp(A)_ij.  MEASURED =
4.93e-14 is the largest violation in that unit of the restatement itself (full
reorthogonalisation, numpy.linalg.eigh) against dense eigh over depths 1..40 on
the four graphs, 21-22 pairs each (entries_bracket_ref.pair_set), with mu =
lambda_upper from the vector of ones and from the exact leading eigenvector
(per graph: anaheim 6.3e-15, india 5.0e-15, rome 5.8e-15, oregon_A0 4.93e-14);
SLACK is ten times that, because CGS2 records differ from full
reorthogonalisation in the last digits.  SLACK = 4.93e-13 lies below the 1e-12
default of ftol, which therefore stays."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_graph

import entries_bracket_ref as er

GRAPHS = ("anaheim", "india", "rome", "oregon_A0")
MEASURED = 4.93e-14
SLACK = 10.0 * MEASURED
FTOL_DEFAULT = 1e-12


def test_slack_lies_below_the_default_floor():
    assert SLACK <= FTOL_DEFAULT


def test_the_pair_set():
    for g in GRAPHS:
        ps = er.graph_case(g)["pairs"]
        count = {k: len(v) for k, v in ps.items()}
        assert count == {"hub edges": 8, "hubs": 6, "leaf edges": 4, "twins": 0 if g == "anaheim" else 1,
                         "distant": 3}, (g, count)
        A = er.graph_case(g)["A"]
        assert all(A[i, j] != 0 for i, j in ps["hub edges"] + ps["leaf edges"])
        assert all(i != j for i, j in er.flat(ps))


@pytest.mark.parametrize("g", GRAPHS)
def test_bracket_holds_and_tightens(g):
    """lo <= exact <= hi at every depth 1..40, lo rising and hi falling, up to
    SLACK (E_ii + E_jj) / 2, for mu from ones and from the exact leading vector."""
    import krylov_robustness_amd as kra
    c = er.graph_case(g)
    A, E = c["A"], c["E"]
    w, V = np.linalg.eigh(A.toarray())
    worst = 0.0
    for mu in (c["mu"], kra.lambda_upper(A, v=V[:, -1])):
        assert mu >= w[-1]
        for (i, j), runs in c["runs"].items():
            v = er.violations(runs, mu, E[i, j], er.scale_of(E, i, j))
            worst = max(worst, v)
            assert v <= SLACK, (g, i, j, mu, v)
    print(g, "largest violation in units of (E_ii + E_jj) / 2:", worst, "slack", SLACK)


@pytest.mark.parametrize("g", GRAPHS)
def test_stopping_rule_on_the_pair_set(g):
    """Every pair stops within 40 steps; edges with flag 0 at rtol 1e-8 in 5 to
    12 steps; the distant pairs with flag 4 at the defaults; every returned
    bracket holds the exact entry."""
    c = er.graph_case(g)
    A, E, mu, ps = c["A"], c["E"], c["mu"], c["pairs"]
    for kind, pairs in ps.items():
        for i, j in pairs:
            runs = c["runs"][(i, j)]
            sc = er.scale_of(E, i, j)
            for rtol in (1e-8, 1e-10):
                lo, hi, it, flag, dep = er.pair_run(A, i, j, mu, rtol=rtol, it=40, runs=runs)
                print(g, kind, (i, j), "rtol", rtol, "E_ij / scale %.3e" % (E[i, j] / sc), "iter", it, "flag", flag,
                      "depths", dep, "gap / scale %.3e" % ((hi - lo) / sc))
                assert flag in (0, 1, 4) and it <= 40, (g, kind, i, j, rtol, flag, it)
                assert lo - SLACK * sc <= E[i, j] <= hi + SLACK * sc
                if flag == 0:
                    assert lo * hi > 0 and 0 <= hi - lo <= rtol * min(abs(lo), abs(hi))
                if flag == 4:
                    assert hi - lo <= FTOL_DEFAULT * sc * (1.0 + 1e-6)
                if kind in ("hub edges", "leaf edges") and rtol == 1e-8:
                    assert flag == 0 and 5 <= it <= 12, (g, kind, i, j, flag, it)
                if kind == "distant" and rtol == 1e-10:
                    assert flag == 4, (g, i, j, flag)


@pytest.mark.parametrize("g", [g for g in GRAPHS if g != "anaheim"])
def test_twin_leaves(g):
    """Two leaves i, j on one node: e_i - e_j is an eigenvector of A to the
    eigenvalue 0, so the - column ends at depth 1 with g- = 1 and exp(A)_ij =
    exp(A)_ii - 1."""
    c = er.graph_case(g)
    (i, j), = c["pairs"]["twins"]
    E = c["E"]
    sc = er.scale_of(E, i, j)
    assert abs(E[i, j] - (E[i, i] - 1.0)) <= SLACK * sc
    lo, hi, it, flag, dep = er.pair_run(c["A"], i, j, c["mu"], it=40, runs=c["runs"][(i, j)])
    assert dep[1] == 1 and dep[0] == it > 1 and flag == 0
    assert lo - SLACK * sc <= E[i, i] - 1.0 <= hi + SLACK * sc
    Lm, Um, km = er.column(c["runs"][(i, j)][1], 1, c["mu"])
    assert km == 1 and Lm == Um and Lm * np.exp(c["mu"]) == pytest.approx(1.0, rel=1e-14)


def test_orientation_and_flags_of_the_rule():
    """(i, j) and (j, i) are one pair; a mu below lambda_max gives flag 2 and
    NaN; it = 3 gives flag 3 with a valid, wide bracket."""
    c = er.graph_case("anaheim")
    A, E, mu = c["A"], c["E"], c["mu"]
    i, j = c["pairs"]["hub edges"][0]
    assert er.pair_run(A, i, j, mu, it=40) == er.pair_run(A, j, i, mu, it=40)
    lo, hi, it, flag, _ = er.pair_run(A, i, j, 0.5 * c["w"][-1], it=40)
    assert flag == 2 and np.isnan(lo) and np.isnan(hi)
    lo, hi, it, flag, _ = er.pair_run(A, i, j, mu, it=3)
    assert flag == 3 and it == 3 and lo < E[i, j] < hi and hi - lo > 1e-3 * E[i, j]
    # both columns exact: a path of two nodes, exp(A)_01 = sinh(1)
    import scipy.sparse as sp
    P2 = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
    lo, hi, it, flag, dep = er.pair_run(P2, 0, 1, 1.0, it=2)
    assert flag == 1 and dep == (1, 1) and lo == hi == pytest.approx(np.sinh(1.0), rel=1e-15)


def test_abi_rejects_bad_arguments_before_the_device():
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sig["kt_entries_fun_bracket"]) == 13
    assert lib.kt_abi_version() == 3
    ei, ej = (C.c_int64 * 2)(0, 1), (C.c_int64 * 2)(1, 2)
    lo, hi = (C.c_double * 2)(), (C.c_double * 2)()

    def call(A=None, q=2, i=ei, j=ej, lam=4.0, it=30, lo=lo, hi=hi):
        return lib.kt_entries_fun_bracket(A, q, i, j, lam, 1e-10, 1e-12, it, lo, hi, None, None, None)
    assert call() == _lib.KT_ERR_ARG
    assert b"kt_entries_fun_bracket: NULL" in lib.kt_last_error()
    assert call(it=257) == _lib.KT_ERR_ARG
    assert b"256" in lib.kt_last_error()
    for bad in (float("inf"), float("nan"), 701.0):
        assert call(lam=bad) == _lib.KT_ERR_ARG
        assert b"lam_hi" in lib.kt_last_error()
    assert call(q=-1) == _lib.KT_ERR_ARG
    for kw in ({"i": None}, {"j": None}, {"lo": None}, {"hi": None}):
        assert call(**kw) == _lib.KT_ERR_ARG
        assert b"NULL" in lib.kt_last_error()
    same = (C.c_int64 * 2)(3, 2)
    assert call(i=same, j=(C.c_int64 * 2)(1, 2)) == _lib.KT_ERR_ARG
    assert b"i == j" in lib.kt_last_error() and b"kt_diag_fun_bracket" in lib.kt_last_error()


def test_python_rejects_bad_arguments_without_a_device(monkeypatch):
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import greedy

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(greedy, "_dev", no_device)
    A = load_graph("anaheim")
    n = A.shape[0]
    ok = np.array([[0, 1], [5, 2]])
    for kw in ({"it": 257}, {"pairs": np.array([[0, n]])}, {"pairs": np.array([[-1, 2]])}, {"lam_hi": 701.0},
               {"lam_hi": float("nan")}):
        with pytest.raises(kra.KrylovError) as e:
            kra.entries_fun_bracket(A, kw.pop("pairs", ok), **kw)
        assert e.value.code == kra._lib.KT_ERR_ARG
    for bad in (np.array([0, 1]), np.zeros((2, 3), dtype=np.int64), np.array([[0.0, 1.0]])):
        with pytest.raises(ValueError, match="entries_fun_bracket: pairs must"):
            kra.entries_fun_bracket(A, bad)
    with pytest.raises(AssertionError, match="a device was touched"):
        kra.entries_fun_bracket(A, ok, lam_hi=7.0)

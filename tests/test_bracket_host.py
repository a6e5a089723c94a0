"""CPU tests of the Gauss / Gauss-Radau bracket of exp(A)_ii:
the host rule kt_host_gauss_radau against the NumPy restatement
(tests/bracket_ref.py), the bracket property against dense eigh, the flags, the
argument checks of the new entries without a device, and lambda_upper.

Bounds.  Host rule against the restatement: ten times "spread_max" of
tests/golden/adaptive_values.json (the host QL against numpy.linalg.eigh on
Lanczos tridiagonals), relative on the scaled sums, what
tests/test_nodes_host.py holds kt_host_node_update to.

Bracket slack.  lo <= exact <= hi and the monotonicity of both bounds hold up
to rounding.  MEASURED = 7.83e-14 is the largest relative violation of the
restatement itself (full reorthogonalisation, numpy.linalg.eigh) against dense
eigh over depths 1..40 on the four graphs, 8 hubs, 8 leaves and the isolated
node each, with mu = lambda_upper from the vector of ones and from the exact
leading eigenvector (per graph: anaheim 9.0e-15, india 8.2e-15, rome 8.4e-15,
oregon_A0 7.8e-14); SLACK is ten times that, because CGS2 records differ from
full reorthogonalisation in the last digits."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import conftest
from conftest import GOLDEN, load_graph

import bracket_ref as br

GRAPHS = ("anaheim", "india", "rome", "oregon_A0")
DEPTHS = (1, 2, 3, 10, 30)
with open(os.path.join(GOLDEN, "adaptive_values.json")) as _f:
    QL_TOL = 10.0 * json.load(_f)["spread_max"]
MEASURED = 7.83e-14
SLACK = 10.0 * MEASURED
DP = C.POINTER(C.c_double)


def host_rule(alpha, beta, j, mu):
    """kt_host_gauss_radau as bracket_ref.bracket: (lo, hi, flag), scaled by exp(-mu)."""
    from krylov_robustness_amd import _lib
    a = np.ascontiguousarray(alpha[:j], dtype=np.float64)
    o = np.ascontiguousarray(np.concatenate([beta[:j - 1], [0.0]]), dtype=np.float64)
    lo, hi, flag = C.c_double(), C.c_double(), C.c_int()
    st = _lib.load().kt_host_gauss_radau(j, a.ctypes.data_as(DP), o.ctypes.data_as(DP), float(beta[j - 1]), float(mu),
                                         C.byref(lo), C.byref(hi), C.byref(flag))
    assert st == _lib.KT_OK
    s = float(np.exp(-mu))
    return lo.value * s, hi.value * s, flag.value


@pytest.fixture(scope="module")
def cases():
    """Per graph: A, diag exp(A) and eigvalsh(A) by dense eigh, mu, and the
    Lanczos runs (full reorthogonalisation, 40 steps) of the tests' nodes."""
    import krylov_robustness_amd as kra
    out = {}
    for g in GRAPHS:
        A = load_graph(g)
        ex, w = br.exp_diag(A)
        mu = kra.lambda_upper(A, v=np.ones(A.shape[0]))
        nodes = br.node_set(A)
        out[g] = {"A": A, "exact": ex, "w": w, "mu": mu, "nodes": nodes,
                  "runs": {i: br.lanczos_full(A, i, 40) for i in nodes}}
    return out


def test_india_has_an_isolated_node(cases):
    assert len(cases["india"]["nodes"]) == 3
    assert all(len(cases[g]["nodes"]) == 2 for g in GRAPHS if g != "india")


@pytest.mark.parametrize("g", GRAPHS)
def test_host_rule_matches_the_restatement(cases, g):
    c = cases[g]
    worst, reached = 0.0, set()
    for i in c["nodes"]:
        al, be = c["runs"][i]
        for j in DEPTHS:
            if j > len(al):
                continue
            reached.add(j)
            lo, hi, flag = br.bracket(al, be, j, c["mu"])
            hlo, hhi, hflag = host_rule(al, be, j, c["mu"])
            assert hflag == flag, (g, i, j, hflag, flag)
            err = abs(hlo - lo) / lo
            if flag == 0:
                err = max(err, abs(hhi - hi) / hi)
            else:
                assert flag == 1 and hhi == hlo
            worst = max(worst, err)
            assert err <= QL_TOL, (g, i, j, err)
    print(g, "worst |host - numpy| / value", worst, "tolerance", QL_TOL)
    assert reached == set(DEPTHS)


@pytest.mark.parametrize("g", GRAPHS)
@pytest.mark.parametrize("rule", ["restatement", "host"])
def test_bracket_holds_and_tightens(cases, g, rule):
    """lo <= exact <= hi at every depth, lo rising and hi falling, up to SLACK."""
    c = cases[g]
    fn = br.bracket if rule == "restatement" else host_rule
    worst = 0.0
    for i in c["nodes"]:
        al, be = c["runs"][i]
        v = br.violations(al, be, c["mu"], c["exact"][i], rule=fn)
        worst = max(worst, v)
        assert v <= SLACK, (g, i, rule, v)
        # and the bracket closes: the last depth's gap is at rounding level
        lo, hi, flag = fn(al, be, len(al), c["mu"])
        assert flag in (0, 1) and hi - lo <= 1e-10 * lo
    print(g, rule, "largest violation", worst, "slack", SLACK)


@pytest.mark.parametrize("g", GRAPHS)
def test_a_lam_hi_below_lambda_max_is_reported(cases, g):
    """mu = 0.5 lambda_max on the hub: some Ritz value passes mu within a few
    steps; flag 2, hi NaN, lo still a lower bound -- never a bracket."""
    c = cases[g]
    hub = c["nodes"][0]
    mu = 0.5 * float(c["w"][-1])
    lo, hi, it, flag = br.bracket_run(c["A"], hub, mu)
    print(g, "hub", hub, "mu", mu, "restatement", lo, hi, it, flag)
    al, be = c["runs"][hub]
    assert flag == 2 and np.isnan(hi) and it <= len(al)
    assert lo <= c["exact"][hub] * (1.0 + SLACK)
    hlo, hhi, hflag = host_rule(al, be, it, mu)
    assert hflag == 2 and np.isnan(hhi) and abs(hlo * np.exp(mu) - lo) <= QL_TOL * lo
    for j in range(it, len(al) + 1):  # theta_max only grows with the depth
        assert host_rule(al, be, j, mu)[2] == 2


def test_lucky_breakdowns(cases):
    """A path of two nodes: T_2 = [[0, 1], [1, 0]], beta_2 = 0, exp(A)_11 =
    cosh(1).  An isolated node: T_1 = [A_ii], beta_1 = 0."""
    lo, hi, flag = host_rule(np.array([0.0, 0.0]), np.array([1.0, 0.0]), 2, 1.0)
    assert flag == 1 and hi == lo and lo * np.e == pytest.approx(np.cosh(1.0), rel=1e-15)
    for aii in (0.0, 0.75):
        lo, hi, flag = host_rule(np.array([aii]), np.array([0.0]), 1, 2.0)
        assert flag == 1 and hi == lo and lo * np.exp(2.0) == pytest.approx(np.exp(aii), rel=1e-15)
    c = cases["india"]
    iso = c["nodes"][2]
    assert br.bracket_run(c["A"], iso, c["mu"]) == (pytest.approx(1.0, rel=1e-15), pytest.approx(1.0, rel=1e-15), 1, 1)
    # lucky wins over a mu that is too small: the Gauss rule is exact whatever mu is
    lo, hi, flag = host_rule(np.array([0.0, 0.0]), np.array([1.0, 0.0]), 2, 0.5)
    assert flag == 1 and hi == lo


def test_host_rule_rejects_bad_arguments():
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    a = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    lo, hi, flag = C.c_double(), C.c_double(), C.c_int()
    out = (C.byref(lo), C.byref(hi), C.byref(flag))
    assert lib.kt_host_gauss_radau(1, a, None, 1.0, 2.0, *out) == _lib.KT_OK
    for j, mu in ((0, 2.0), (257, 2.0), (2, float("inf")), (2, float("nan")), (2, 700.5)):
        assert lib.kt_host_gauss_radau(j, a, a, 1.0, mu, *out) == _lib.KT_ERR_ARG
        assert b"kt_host_gauss_radau" in lib.kt_last_error()
    assert lib.kt_host_gauss_radau(2, a, None, 1.0, 2.0, *out) == _lib.KT_ERR_ARG
    assert lib.kt_host_gauss_radau(2, a, a, 1.0, 2.0, None, C.byref(hi), C.byref(flag)) == _lib.KT_ERR_ARG


def test_abi_rejects_bad_arguments_before_the_device():
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sig["kt_diag_fun_bracket"]) == 10 and len(sig["kt_host_gauss_radau"]) == 8
    nodes = (C.c_int64 * 2)(0, 1)
    lo, hi = (C.c_double * 2)(), (C.c_double * 2)()
    assert lib.kt_diag_fun_bracket(None, 2, nodes, 4.0, 1e-10, 30, lo, hi, None, None) == _lib.KT_ERR_ARG
    assert b"kt_diag_fun_bracket: NULL" in lib.kt_last_error()
    assert lib.kt_diag_fun_bracket(None, 2, nodes, 4.0, 1e-10, 257, lo, hi, None, None) == _lib.KT_ERR_ARG
    assert b"256" in lib.kt_last_error()
    for bad in (float("inf"), float("nan"), 700.5):
        assert lib.kt_diag_fun_bracket(None, 2, nodes, bad, 1e-10, 30, lo, hi, None, None) == _lib.KT_ERR_ARG
        assert b"lam_hi" in lib.kt_last_error()
    assert lib.kt_diag_fun_bracket(None, -1, nodes, 4.0, 1e-10, 30, lo, hi, None, None) == _lib.KT_ERR_ARG


def test_python_rejects_bad_arguments_without_a_device(monkeypatch):
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import greedy

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(greedy, "_dev", no_device)
    A = load_graph("anaheim")
    n = A.shape[0]
    for kw in ({"it": 257}, {"nodes": [1, n + 1]}, {"nodes": [0]}, {"lam_hi": 701.0}, {"lam_hi": float("nan")}):
        with pytest.raises(kra.KrylovError) as e:
            kra.diag_fun_bracket(A, kw.pop("nodes", [1, 2]), **kw)
        assert e.value.code == kra._lib.KT_ERR_ARG
    with pytest.raises(AssertionError, match="a device was touched"):
        kra.diag_fun_bracket(A, [1, n], lam_hi=7.0)
    for fun in ("cosh", "sinh", "sqrt"):
        with pytest.raises(kra.KrylovError, match="only fun = exp") as e:
            kra.find_top_nodes_fun(A, 3, fun=fun)
        assert e.value.code == kra._lib.KT_ERR_ARG


def _two_components():
    """A star of 30 leaves and, joined to nothing of it, a triangle and an isolated node."""
    n = 35
    A = sp.lil_matrix((n, n))
    for leaf in range(1, 31):
        A[0, leaf] = A[leaf, 0] = 1.0
    for i, j in ((31, 32), (32, 33), (31, 33)):
        A[i, j] = A[j, i] = 1.0
    return sp.csr_matrix(A)


def _weighted(A, seed=3):
    rng = np.random.default_rng(seed)
    U = sp.triu(A, 1).tocoo()
    W = sp.coo_matrix((U.data * rng.uniform(0.25, 4.0, U.nnz), (U.row, U.col)), shape=A.shape)
    return sp.csr_matrix(W + W.T)


def test_lambda_upper_is_an_upper_bound():
    """On every golden graph, a weighted copy, a two-component graph and a
    signed copy, from a poor start (ones), the exact leading vector and a
    vector that vanishes on a component; rounds never raise it."""
    import krylov_robustness_amd as kra
    mats = [(g, load_graph(g)) for g in conftest.GRAPHS]
    mats += [("rome weighted", _weighted(load_graph("rome"))), ("two components", _two_components())]
    for name, A in mats:
        n = A.shape[0]
        w, V = np.linalg.eigh(A.toarray())
        lam, ninf = float(w[-1]), br.lambda_upper_ref(A)
        ratios = []
        for v in (np.ones(n), V[:, -1], np.where(np.arange(n) < n // 2, 1.0, 0.0)):
            prev = np.inf
            for rounds in (0, 1, 8):
                ub = kra.lambda_upper(A, rounds=rounds, v=v)
                assert lam <= ub <= ninf * (1.0 + 2e-12), (name, rounds, ub, lam, ninf)
                assert ub <= prev * (1.0 + 1e-14)
                prev = ub
            ratios.append(prev / lam)
        print(name, "n", n, "lambda_max", lam, "||A||_inf / lambda_max", ninf / lam,
              "lambda_upper / lambda_max from ones, exact v, half-zero v:", ratios)
    S = sp.lil_matrix(load_graph("anaheim"))
    i, j = S.nonzero()[0][0], S.nonzero()[1][0]
    S[i, j] = S[j, i] = -1.0
    S = sp.csr_matrix(S)
    assert kra.lambda_upper(S, v=np.ones(S.shape[0])) == br.lambda_upper_ref(S) * (1.0 + 1e-12)
    assert kra.lambda_upper(S, v=np.ones(S.shape[0])) >= np.linalg.eigvalsh(S.toarray())[-1]
    assert kra.lambda_upper(sp.csr_matrix((5, 5)), v=np.ones(5)) == 0.0

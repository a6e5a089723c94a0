"""kt_diag_fun_bracket on the device against dense eigh and
against the host rule on the NumPy restatement's tridiagonal
(tests/bracket_ref.py), and find_top_nodes_fun over it.

Bounds.  lo <= exact <= hi up to SLACK of tests/test_bracket_host.py (ten times
the restatement's own largest violation against dense eigh, 7.83e-14).  Device
values against kt_host_gauss_radau on the restatement's tridiagonal at the
device's depth: rel 1e-7, the convention of tests/test_gpu_nodes.py against
nodes_ref.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_graph

import bracket_ref as br

GRAPHS = ("anaheim", "india", "rome", "oregon_A0")
SLACK = 10.0 * 7.83e-14
RTOL = 1e-10
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


def cand_list(A, size):
    """8 (size 17) or 16 (size 33) hubs, as many leaves less one, the isolated
    node (a leaf where there is none) and hub 3 a second time; padded with the
    next hubs where the graph has too few leaves.  0-based."""
    deg = np.diff(A.indptr)
    k = (size - 1) // 2
    hubs = [int(i) for i in np.argsort(-deg, kind="stable")]
    leaves = [int(i) for i in np.flatnonzero(deg == 1)]
    iso = np.flatnonzero(deg == 0)
    lst = hubs[:k] + leaves[:k - 1]
    if iso.size or len(leaves) >= k:
        lst.append(int(iso[0]) if iso.size else leaves[k - 1])
    lst += [h for h in hubs[k:] if h not in lst][:size - 1 - len(lst)]
    lst.append(hubs[3])
    assert len(lst) == size and len(set(lst)) == size - 1
    return lst


@pytest.fixture(scope="module")
def cases(kra, gpu_ctx):
    """Per graph: A, its device copy, diag exp(A) by dense eigh, lam_hi =
    lambda_upper on the device's leading vector, and the 33-candidate call.
    The device copies are closed here, while the context is alive: a failure
    report that keeps this dict would otherwise leave them to the interpreter's
    shutdown, after the context."""
    out = {}
    for g in GRAPHS:
        A = load_graph(g)
        D = kra.DeviceMatrix(A, gpu_ctx)
        ex, w = br.exp_diag(A)
        mu = kra.lambda_upper(D, ctx=gpu_ctx)
        assert w[-1] <= mu <= br.lambda_upper_ref(A) * (1.0 + 2e-12)
        print(g, "lambda_upper / lambda_max", mu / w[-1])
        nodes = cand_list(A, 33)
        res = kra.diag_fun_bracket(D, np.array(nodes) + 1, rtol=RTOL, lam_hi=mu, ctx=gpu_ctx)
        out[g] = {"A": A, "D": D, "exact": ex, "w": w, "mu": mu, "nodes33": nodes, "res33": res, "runs": {}}
    yield out
    for c in out.values():
        c.pop("D").close()


def host_on_restatement(c, i, depth):
    """kt_host_gauss_radau at `depth` on the restatement's tridiagonal of node i."""
    from krylov_robustness_amd import _lib
    if i not in c["runs"]:
        c["runs"][i] = br.lanczos_full(c["A"], i, 40)
    al, be = c["runs"][i]
    assert depth <= len(al), (i, depth, len(al))
    a = np.ascontiguousarray(al[:depth])
    o = np.ascontiguousarray(np.concatenate([be[:depth - 1], [0.0]]))
    lo, hi, flag = C.c_double(), C.c_double(), C.c_int()
    assert _lib.load().kt_host_gauss_radau(depth, a.ctypes.data_as(DP), o.ctypes.data_as(DP), float(be[depth - 1]),
                                           float(c["mu"]), C.byref(lo), C.byref(hi), C.byref(flag)) == _lib.KT_OK
    return lo.value, hi.value, flag.value


def check_call(c, g, nodes, res, it_cap):
    lo, hi, it, fl = res
    worst = 0.0
    for h, i in enumerate(nodes):
        ex = c["exact"][i]
        print(g, "node", i, "lo", lo[h], "hi", hi[h], "iter", int(it[h]), "flag", int(fl[h]), "exact", ex)
        assert fl[h] in (0, 1), (g, i, int(fl[h]))
        assert 1 <= it[h] <= it_cap
        assert lo[h] <= ex * (1.0 + SLACK) and ex <= hi[h] * (1.0 + SLACK), (g, i, lo[h], ex, hi[h])
        worst = max(worst, (lo[h] - ex) / ex, (ex - hi[h]) / ex)
        if fl[h] == 0:
            assert hi[h] - lo[h] <= RTOL * lo[h], (g, i, lo[h], hi[h])
        else:
            assert hi[h] == lo[h]
        rlo, rhi, rflag = host_on_restatement(c, i, int(it[h]))
        assert lo[h] == pytest.approx(rlo, rel=1e-7) and hi[h] == pytest.approx(rhi, rel=1e-7)
        assert rflag == (1 if fl[h] == 1 else 0)
    print(g, len(nodes), "candidates: largest violation of the bracket", worst, "slack", SLACK)


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRAPHS)
def test_33_candidates_bracket_exact_and_match_the_host_rule(kra, gpu_ctx, cases, g):
    """Three sweeps on three lanes, the last with one column."""
    c = cases[g]
    check_call(c, g, c["nodes33"], c["res33"], min(100, c["A"].shape[0]))
    lo, hi, it, fl = c["res33"]
    assert (lo[32], hi[32], it[32], fl[32]) == (lo[3], hi[3], it[3], fl[3])  # the duplicate
    if g == "india":  # the isolated node: T_1 = [0], beta_1 = 0
        assert (lo[31], hi[31], it[31], fl[31]) == (1.0, 1.0, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRAPHS)
def test_17_candidates(kra, gpu_ctx, cases, g):
    """Two sweeps, the second with one column."""
    c = cases[g]
    nodes = cand_list(c["A"], 17)
    res = kra.diag_fun_bracket(c["D"], np.array(nodes) + 1, rtol=RTOL, lam_hi=c["mu"], ctx=gpu_ctx)
    check_call(c, g, nodes, res, min(100, c["A"].shape[0]))
    assert gpu_ctx.stat(13) == 2


@pytest.mark.gpu
def test_values_do_not_depend_on_the_call(kra, gpu_ctx, cases):
    """A node alone and inside the 33-candidate call: the same bits."""
    c = cases["india"]
    lo, hi, it, fl = c["res33"]
    for h in (0, 7, 15, 20, 31, 32):
        l1, h1, i1, f1 = kra.diag_fun_bracket(c["D"], [c["nodes33"][h] + 1], rtol=RTOL, lam_hi=c["mu"], ctx=gpu_ctx)
        assert (l1[0].tobytes(), h1[0].tobytes(), int(i1[0]), int(f1[0])) == \
            (lo[h].tobytes(), hi[h].tobytes(), int(it[h]), int(fl[h])), (h, c["nodes33"][h])
    again = kra.diag_fun_bracket(c["D"], np.array(c["nodes33"]) + 1, rtol=RTOL, lam_hi=c["mu"], ctx=gpu_ctx)
    rev = kra.diag_fun_bracket(c["D"], np.array(c["nodes33"][::-1]) + 1, rtol=RTOL, lam_hi=c["mu"], ctx=gpu_ctx)
    for a, b, r in zip(c["res33"], again, rev):
        assert a.tobytes() == b.tobytes() == np.ascontiguousarray(r[::-1]).tobytes()


@pytest.mark.gpu
def test_the_depth_cap_and_a_lam_hi_that_is_too_small(kra, gpu_ctx, cases):
    c = cases["rome"]
    hub = c["nodes33"][0]
    ex = c["exact"][hub]
    lo, hi, it, fl = kra.diag_fun_bracket(c["D"], [hub + 1], rtol=RTOL, it=3, lam_hi=c["mu"], ctx=gpu_ctx)
    print("it = 3:", lo[0], hi[0], int(it[0]), int(fl[0]), "exact", ex)
    assert (it[0], fl[0]) == (3, 3)
    assert lo[0] <= ex * (1.0 + SLACK) and ex <= hi[0] * (1.0 + SLACK) and hi[0] - lo[0] > RTOL * lo[0]
    rlo, rhi, _ = host_on_restatement(c, hub, 3)
    assert lo[0] == pytest.approx(rlo, rel=1e-7) and hi[0] == pytest.approx(rhi, rel=1e-7)
    lo, hi, it, fl = kra.diag_fun_bracket(c["D"], [hub + 1], rtol=RTOL, lam_hi=0.5 * float(c["w"][-1]), ctx=gpu_ctx)
    print("lam_hi = 0.5 lambda_max:", lo, hi, it, fl)
    assert fl[0] == 2 and np.isnan(hi[0]) and lo[0] <= ex * (1.0 + SLACK) and it[0] <= 40


@pytest.mark.gpu
def test_dense_branch(kra, gpu_ctx):
    A = load_graph("denmark")
    assert A.shape[0] == 96
    ex, _ = br.exp_diag(A)
    nodes = np.array([85, 0, 42, 85])
    lo, hi, it, fl = kra.diag_fun_bracket(A, nodes + 1, ctx=gpu_ctx)
    assert np.all(it == 0) and np.all(fl == 0) and np.array_equal(lo, hi)
    assert lo == pytest.approx(ex[nodes], rel=1e-10)


@pytest.mark.gpu
def test_find_top_nodes_fun(kra, gpu_ctx, cases):
    c = cases["rome"]
    want = np.argsort(-c["exact"], kind="stable")[:5] + 1
    # The ranking is diag_fun's.  Its error per probe is at most sqrt(exp(2A)_ii - exp(A)_ii^2), ~8 on
    # rome's top nodes (values ~7), so 256 probes leave ~7 % per node and the fifth node (0.05 % above the
    # sixth) can fall out of any small candidate set: it did, out of 20 and out of 128.  4096 probes leave
    # ~1.8 %, and 128 candidates hold every node within 20 % of the fifth value (85 nodes), 11 sigma.
    nodes, info = kra.find_top_nodes_fun(c["D"], 5, ncand=128, nprobes=4096, ctx=gpu_ctx)
    print("find_top_nodes_fun", nodes, "dense", want, "separated", info["separated"])
    assert nodes.tolist() == want.tolist()
    lo, hi, cand = info["lo"], info["hi"], info["candidates"]
    assert len(cand) == 128 and len(set(cand.tolist())) == 128 and cand[:5].tolist() == nodes.tolist()
    assert np.all(lo[:-1] >= lo[1:])
    assert info["separated"] == bool(np.all(lo[:-1] > hi[1:]))
    ex = c["exact"][cand - 1]
    assert np.all(lo <= ex * (1.0 + SLACK)) and np.all(ex <= hi * (1.0 + SLACK))
    if info["separated"]:  # then the order among the candidates is the exact one
        assert np.all(ex[:-1] > ex[1:])


@pytest.mark.gpu
def test_abi_rejects_an_index_equal_to_n_and_null_outputs(kra, gpu_ctx, cases):
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    c = cases["anaheim"]
    n = c["A"].shape[0]
    nodes = (C.c_int64 * 2)(0, n)
    lo, hi = (C.c_double * 2)(), (C.c_double * 2)()
    h = c["D"].handle
    assert lib.kt_diag_fun_bracket(h, 2, nodes, c["mu"], 0.0, 0, lo, hi, None, None) == _lib.KT_ERR_ARG
    assert b"node index out of range" in lib.kt_last_error()
    assert lib.kt_diag_fun_bracket(h, 2, nodes, c["mu"], 0.0, 0, lo, None, None, None) == _lib.KT_ERR_ARG
    nodes[1] = n - 1
    assert lib.kt_diag_fun_bracket(h, 2, nodes, c["mu"], 0.0, 0, lo, hi, None, None) == _lib.KT_OK  # rtol, it defaults
    assert lo[0] <= c["exact"][0] * (1.0 + SLACK) and c["exact"][0] <= hi[0] * (1.0 + SLACK)
    assert hi[0] - lo[0] <= 1e-10 * lo[0]

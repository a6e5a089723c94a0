"""The y-form sweep's last pass as a quadratic form over each row's
strictly-lower prefix and diagonal (k_spmm_quadform, DevCSR::lower), and the
neighbour-clustered row order of the relabelled copy (kt_order.h): per-probe
forms against the C oracle at tests/test_gpu_slq.py's tolerance (rtol 1e-8),
on small graphs built here that reach each branch of the prefix logic, with
m = 2 (the start pass plus only the new last pass) and m = 30, for every
probe-block width P up to 32; then the same forms and f(A) x through the
Lanczos-f Afun (permute in, permute out) on graphs of n = 20,000, and one
mc_trace round with the Lanczos Afun on a golden graph at its existing
tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph
from oracle import krylov_oracle as ko
from oracle import slq_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-8  # tests/test_gpu_slq.py
NPROBES = 37  # ragged against every P, more than the widest block


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


def _sym(n, i, j):
    i, j = np.asarray(i), np.asarray(j)
    A = sp.coo_matrix((np.ones(i.size), (i, j)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float64).tocsr()
    A.sort_indices()
    return A


def _path(n):
    return _sym(n, np.arange(n - 1), np.arange(1, n))


def _star(n):
    return _sym(n, np.zeros(n - 1, dtype=int), np.arange(1, n))


def _er(n, npairs, seed):
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, n, npairs), rng.integers(0, n, npairs)
    keep = i != j
    return _sym(n, i[keep], j[keep])


def _loops_weighted():
    """Self-loops on every third node and fp64 weights everywhere: the
    diagonal term and the 12 B/nnz (values read) path."""
    from krylov_robustness_amd import graphs
    n = 311
    W = graphs.symmetric_weights(_er(n, 900, 1), seed=2)
    d = np.zeros(n)
    d[::3] = np.random.default_rng(3).uniform(0.5, 1.5, d[::3].size)
    A = (W + sp.diags(d)).tocsr()
    A.sort_indices()
    assert (A.diagonal() != 0).sum() == d[::3].size and not np.all(A.data == 1.0)
    return A


def _empty_rows():
    """Rows 200.. have degree 0 (and some of the first 200 as well)."""
    n = 307
    A = sp.lil_matrix((n, n))
    A[:200, :200] = _er(200, 350, 4)
    A = A.tocsr()
    assert (np.diff(A.indptr) == 0).sum() > 100
    return A


def _long_rows():
    """Long rows of every kind of prefix.  Two star hubs of degree 71 and 301
    (> 64 and > 256: the whole-wave path), linked to each other: the larger
    takes label 0 with an empty prefix, the smaller a prefix of one entry.
    K_{100,120}: 120 rows of degree 100 whose neighbours all carry smaller
    labels (a full prefix, walked by a wave) and 100 rows of degree 120 whose
    neighbours all carry larger ones (an empty one).  Small stars (degree 5
    and 10): short rows whose neighbours all have larger labels.  A path joins
    the parts so that the spectrum is rich."""
    i, j = [], []
    n = 0

    def star(k):
        nonlocal n
        hub = n
        i.extend([hub] * k)
        j.extend(range(hub + 1, hub + 1 + k))
        n += k + 1
        return hub

    h1, h2 = star(300), star(70)
    i.append(h1)
    j.append(h2)
    left = np.arange(n, n + 100)
    right = np.arange(n + 100, n + 220)
    n += 220
    ii, jj = np.meshgrid(left, right, indexing="ij")
    i.extend(ii.ravel())
    j.extend(jj.ravel())
    s1, s2 = star(5), star(10)
    tail = np.arange(n, n + 60)
    n += 60
    i.extend(tail[:-1])
    j.extend(tail[1:])
    for a, b in ((h2 + 1, left[0]), (right[-1], s1 + 1), (s2 + 1, tail[0]), (s1 + 2, s2 + 2)):
        i.append(a)
        j.append(b)
    A = _sym(n, i, j)
    deg = np.diff(A.indptr)
    assert deg.max() > 256 and ((deg > 64) & (deg <= 256)).sum() >= 221
    return A


def _long_rows_weighted():
    from krylov_robustness_amd import graphs
    return graphs.symmetric_weights(_long_rows(), seed=5)


SMALL = {"path_300": lambda: _path(300), "star_300": lambda: _star(300), "loops_weighted": _loops_weighted,
         "empty_rows": _empty_rows, "long_rows": _long_rows, "long_rows_weighted": _long_rows_weighted}
_cache = {}


def _graph(name):
    if name not in _cache:
        _cache[name] = SMALL[name]()
    return _cache[name]


def _oracle(name, m):
    """The oracle's forms, once per (graph, m)."""
    key = (name, m)
    if key not in _cache:
        _cache[key] = slq_ref.slq_trace(_graph(name), NPROBES, m, seed=13, fun="exp")[1]
    return _cache[key]


@pytest.mark.parametrize("block", [1, 2, 4, 8, 16, 32])
@pytest.mark.parametrize("m", [2, 30])
@pytest.mark.parametrize("name", list(SMALL))
def test_last_pass_forms_match_oracle(kra, gpu_ctx, name, m, block):
    A = _graph(name)
    D = kra.DeviceMatrix(A, gpu_ctx)
    before = gpu_ctx.yform_redone()
    _, _, q = kra.slq_quadforms(D, NPROBES, m, seed=13, fun="exp", block=block, ctx=gpu_ctx)
    q_ref = _oracle(name, m)
    redone = gpu_ctx.yform_redone() - before
    print(f"{name} m={m} P={block}: max rel err {np.max(np.abs(q - q_ref) / np.abs(q_ref)):.3e}, redone {redone}")
    np.testing.assert_allclose(q, q_ref, rtol=RTOL)
    if m == 2:  # the forms above came from the new pass, not from the explicit sweep's redo
        assert redone == 0


@pytest.mark.parametrize("kind", ["erdos_renyi", "chung_lu"])
def test_clustered_order_forms_and_fmv(kra, gpu_ctx, kind):
    """n = 20,000 (more rows than the order's hub cut-off, so the neighbour key
    is in force): forms against the oracle, and f(A) x through the Lanczos-f
    Afun, whose columns are permuted into the relabelled order and back."""
    from krylov_robustness_amd import graphs
    A = graphs.erdos_renyi(20_000, 100_000, seed=6) if kind == "erdos_renyi" else \
        graphs.chung_lu(20_000, 200_000, seed=6)
    D = kra.DeviceMatrix(A, gpu_ctx)
    _, _, q = kra.slq_quadforms(D, 20, 30, seed=17, fun="exp", block=16, ctx=gpu_ctx)
    _, q_ref = slq_ref.slq_trace(A, 20, 30, seed=17, fun="exp")
    np.testing.assert_allclose(q, q_ref, rtol=RTOL)
    X = np.random.default_rng(8).normal(size=(A.shape[0], 5))
    Y = kra.lanczos_fmv(D, X, m=20, fun="exp", ctx=gpu_ctx)
    Yo = ko.lanczos_fmv(A, X, 20, "exp")
    np.testing.assert_allclose(Y, Yo, rtol=1e-8, atol=1e-10 * np.abs(Yo).max())  # tests/test_gpu_mctrace.py


def test_mc_trace_lanczos_afun_round(kra, gpu_ctx):
    """mc_trace's y-form quadrature columns end in the same last pass: one
    round on dt_oregon A6 against the oracle, at the tolerance of
    tests/test_gpu_mctrace.py::test_trace_exp_lanczos_config1."""
    A = load_graph("oregon_A6")
    D = kra.DeviceMatrix(A, gpu_ctx)
    tr, _, it = kra.mc_trace("lanczos", A.shape[0], 1e-4, 30, 1, seed=0, m=20, A=D, ctx=gpu_ctx)
    tro, _, ito = ko.trace_exp_lanczos(A, m=20, tol=1e-4, maxit=30, seed=0)
    assert it == ito == 1
    assert tr == pytest.approx(tro, rel=1e-10)

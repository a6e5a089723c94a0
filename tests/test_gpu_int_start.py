"""GPU: the compact start of a y-form sweep (y_0 kept as int16 row sums through
the first two steps) against the fp64 form, KT_SLQ_INT0=1 vs 0
in one process.  y_0 = s0 * (double)k is the product the fp64 start pass
stores and every sum keeps its order, so the per-probe forms are compared
BITWISE; kt_context_stat 7 counts the sweeps that took the compact form.
Against the C oracle the forms keep test_gpu_slq.py's tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import slq_ref
from test_gpu_slq import RTOL

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 4, 8, 16, 32]
DEPTHS = [2, 3, 4, 30]  # 2, 3: the first / second step is the sweep's last pass (k_spmm_quadform)


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


@pytest.fixture(scope="module")
def A3k():
    from krylov_robustness_amd import graphs
    A = graphs.chung_lu(3_000, 30_000, seed=4)
    assert A.nnz == 30_000 and np.all(A.data == 1.0)
    deg = np.diff(A.indptr)
    assert deg.max() > 64 and deg.min() <= 4  # long-row waves and short row groups both run
    return A


def nprobes_for(P):
    """Two full sweeps (one per lane) and a remainder sweep where P allows one."""
    return 2 * P + (P + 1) // 2


def both(kra, monkeypatch, ctx, D, nprobes, m, **kw):
    """(forms compact, forms fp64, sweeps that took the compact form); the
    fp64 run must not count any, and the guard redoes the same number of
    sweeps in both."""
    monkeypatch.setenv("KT_SLQ_INT0", "1")
    c0, r0 = ctx.stat(7), ctx.yform_redone()
    q1 = kra.slq_quadforms(D, nprobes, m, ctx=ctx, **kw)[2].copy()
    c1, r1 = ctx.stat(7), ctx.yform_redone()
    monkeypatch.setenv("KT_SLQ_INT0", "0")
    q0 = kra.slq_quadforms(D, nprobes, m, ctx=ctx, **kw)[2].copy()
    assert ctx.stat(7) == c1
    assert ctx.yform_redone() - r1 == r1 - r0
    return q1, q0, c1 - c0


@pytest.mark.parametrize("m", DEPTHS)
@pytest.mark.parametrize("P", WIDTHS)
def test_short_and_long_rows_bitwise(kra, gpu_ctx, monkeypatch, A3k, P, m):
    D = kra.DeviceMatrix(A3k, gpu_ctx)
    N = nprobes_for(P)
    q1, q0, engaged = both(kra, monkeypatch, gpu_ctx, D, N, m, seed=12, block=P)
    assert engaged == (-(-N // P) if m >= 3 else 0)
    assert np.all(np.isfinite(q1)) and np.array_equal(q1, q0)


@pytest.fixture(scope="module")
def oracle3k(A3k):
    """The oracle's forms per depth, for the widest probe count (the probes
    are keyed by global index: a narrower run's are a prefix)."""
    N = max(nprobes_for(P) for P in WIDTHS)
    return {m: slq_ref.slq_trace(A3k, N, m, seed=12)[1] for m in DEPTHS}


@pytest.mark.parametrize("m", DEPTHS)
@pytest.mark.parametrize("P", WIDTHS)
def test_forms_match_the_oracle(kra, gpu_ctx, monkeypatch, A3k, oracle3k, P, m):
    D = kra.DeviceMatrix(A3k, gpu_ctx)
    N = nprobes_for(P)
    monkeypatch.setenv("KT_SLQ_INT0", "1")
    q = kra.slq_quadforms(D, N, m, seed=12, block=P, ctx=gpu_ctx)[2]
    np.testing.assert_allclose(q, oracle3k[m][:N], rtol=RTOL)


def star(n, ring):
    """Node 0 joined to every other node (degree n - 1); `ring`: the other
    nodes also form a cycle, so the Krylov space is not exhausted after three
    steps as on the plain star (whose sweeps the guard redoes)."""
    leaves = np.arange(1, n)
    i, j = [np.zeros(n - 1, dtype=np.int64)], [leaves]
    if ring:
        i.append(leaves)
        j.append(np.roll(leaves, -1))
    i, j = np.concatenate(i), np.concatenate(j)
    A = sp.coo_matrix((np.ones(2 * i.size), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n))
    A = A.tocsr()
    assert np.all(A.data == 1.0)
    return A


@pytest.mark.parametrize("ring", [False, True])
def test_hub_of_degree_32767_engages(kra, monkeypatch, ring):
    A = star(32_768, ring)
    assert np.diff(A.indptr).max() == 32_767
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    q1, q0, engaged = both(kra, monkeypatch, ctx, D, 24, 5, seed=3, block=16)
    assert engaged == 2
    assert np.array_equal(q1, q0)


@pytest.mark.parametrize("ring", [False, True])
def test_hub_of_degree_32768_keeps_fp64(kra, monkeypatch, ring):
    A = star(32_769, ring)
    assert np.diff(A.indptr).max() == 32_768
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    q1, q0, engaged = both(kra, monkeypatch, ctx, D, 24, 5, seed=3, block=16)
    assert engaged == 0
    assert np.array_equal(q1, q0)


def test_unit_diagonal_entries(kra, gpu_ctx, monkeypatch):
    from krylov_robustness_amd import graphs
    A = graphs.chung_lu(500, 4_000, seed=9)
    loops = np.zeros(500)
    loops[::3] = 1.0
    A = sp.csr_matrix(A + sp.diags(loops))
    A.eliminate_zeros()
    assert np.all(A.data == 1.0) and A.diagonal().sum() == loops.sum()
    D = kra.DeviceMatrix(A, gpu_ctx)
    for m in (3, 20):
        q1, q0, engaged = both(kra, monkeypatch, gpu_ctx, D, 24, m, seed=5, block=16)
        assert engaged == 2
        assert np.array_equal(q1, q0)
        np.testing.assert_allclose(q1, slq_ref.slq_trace(A, 24, m, seed=5)[1], rtol=RTOL)


def test_weighted_graph_keeps_fp64(kra, gpu_ctx, monkeypatch, A3k):
    from krylov_robustness_amd import graphs
    W = graphs.symmetric_weights(A3k)
    D = kra.DeviceMatrix(W, gpu_ctx)
    q1, q0, engaged = both(kra, monkeypatch, gpu_ctx, D, 40, 30, seed=12, block=16)
    assert engaged == 0
    assert np.array_equal(q1, q0)


def test_guard_redo_is_the_same(kra, monkeypatch):
    """test_slq_yform_breakdown_falls_back's construction: K_50 exhausts the
    Krylov space after two steps, the guard trips and both sweeps are redone
    by the explicit sweep -- in the compact form as in the fp64 form."""
    A = sp.csr_matrix(np.ones((50, 50)) - np.eye(50))
    monkeypatch.setenv("KT_SLQ_YFORM", "1")
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    monkeypatch.setenv("KT_SLQ_INT0", "1")
    q1 = kra.slq_quadforms(D, 20, 30, seed=6, block=16, ctx=ctx)[2].copy()
    assert ctx.stat(7) == 2 and ctx.yform_redone() == 2  # both sweeps of 16 probes
    monkeypatch.setenv("KT_SLQ_INT0", "0")
    q0 = kra.slq_quadforms(D, 20, 30, seed=6, block=16, ctx=ctx)[2].copy()
    assert ctx.stat(7) == 2 and ctx.yform_redone() == 4
    assert np.array_equal(q1, q0)
    np.testing.assert_allclose(q1, slq_ref.slq_trace(A, 20, 30, seed=6)[1], rtol=1e-10)
    from oracle import krylov_oracle as ko
    Z = ko.rademacher(50, np.arange(20), 6)
    s = Z.sum(axis=0)
    exact = s ** 2 / 50 * np.exp(49.0) + (50 - s ** 2 / 50) * np.exp(-1.0)
    np.testing.assert_allclose(q1, exact, rtol=1e-10)

"""GPU: the probe sweep on the chained row order of the relabelled copy
(csrc/kt_order.h chain_order).  Small graphs that reach the order's branches
and the sweep's row kinds -- long rows owned by a wave, short row groups in
more than one block, a last ragged chunk, fewer rows than one grid, empty
rows, weights -- at m = 5 and 12 and P = 8, 16, 64: the per-probe forms
against the C oracle at tests/test_gpu_slq.py's tolerance, one sweep lane
against two bit for bit, the compact start against the fp64 start bit for
bit, two runs bit for bit, and the explicit sweep at the oracle's tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import slq_ref
from test_gpu_slq import RTOL

pytestmark = pytest.mark.gpu

WIDTHS = [8, 16, 64]
DEPTHS = [5, 12]
SEED = 21


def nprobes_for(P):
    """Two full sweeps (one per lane) and a remainder sweep."""
    return 2 * P + P // 2


def _sym(n, i, j):
    A = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float64).tocsr()
    A.sort_indices()
    return A


def _er(n, npairs, seed):
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, n, npairs), rng.integers(0, n, npairs)
    keep = i != j
    return _sym(n, i[keep], j[keep])


def _chung_lu_3k():
    from krylov_robustness_amd import graphs
    A = graphs.chung_lu(3_000, 30_000, seed=4)
    deg = np.diff(A.indptr)
    n_long = int((deg > 64).sum())
    # rows owned by a whole wave, eight to a block: a number of such blocks
    # that is no multiple of 8, so the short blocks do not start at label 0
    assert n_long > 0 and -(-n_long // 8) % 8 != 0
    return A


def _empty_rows():
    n = 700
    A = sp.lil_matrix((n, n))
    A[:500, :500] = _er(500, 1_200, 4)
    A = A.tocsr()
    assert (np.diff(A.indptr) == 0).sum() > 200
    return A


def _weighted():
    from krylov_robustness_amd import graphs
    return graphs.symmetric_weights(_er(1_100, 4_000, 8), seed=2)


GRAPHS = {
    "chung_lu_3k": _chung_lu_3k,
    "er_1535": lambda: _er(64 * 8 * 3 - 1, 6_000, 5),  # one row short of a whole number of chunks per label
    "er_1537": lambda: _er(64 * 8 * 3 + 1, 6_000, 6),  # one row past it
    "er_300": lambda: _er(300, 900, 7),  # fewer than eight 64-row chunks: a grid under eight blocks
    "empty_rows": _empty_rows,
    "weighted": _weighted,
}
_cache = {}


def _graph(name):
    if name not in _cache:
        _cache[name] = GRAPHS[name]()
    return _cache[name]


def _oracle(name, m):
    """The oracle's forms once per (graph, m), for the widest probe count (the
    probes are keyed by global index: a narrower run's are a prefix)."""
    if (name, m) not in _cache:
        _cache[(name, m)] = slq_ref.slq_trace(_graph(name), nprobes_for(max(WIDTHS)), m, seed=SEED)[1]
    return _cache[(name, m)]


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


@pytest.mark.parametrize("P", WIDTHS)
@pytest.mark.parametrize("m", DEPTHS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_sweep_forms_on_the_chained_order(kra, gpu_ctx, monkeypatch, name, m, P):
    A = _graph(name)
    N = nprobes_for(P)
    q_ref = _oracle(name, m)[:N]
    D = kra.DeviceMatrix(A, gpu_ctx)

    def forms(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return kra.slq_quadforms(D, N, m, seed=SEED, block=P, ctx=gpu_ctx)[2].copy()

    redone = gpu_ctx.yform_redone()
    q = forms(KT_SLQ_LANES="2", KT_SLQ_INT0="1")
    print(f"{name} m={m} P={P}: max rel err vs oracle {np.max(np.abs(q - q_ref) / np.abs(q_ref)):.3e}")
    np.testing.assert_allclose(q, q_ref, rtol=RTOL)
    assert np.array_equal(forms(), q), "two runs differ"
    assert np.array_equal(forms(KT_SLQ_LANES="1"), q), "one sweep lane differs from two"
    assert np.array_equal(forms(KT_SLQ_LANES="2", KT_SLQ_INT0="0"), q), "the fp64 start differs from the compact one"
    assert gpu_ctx.yform_redone() == redone  # every form above came from the y-form passes


@pytest.mark.parametrize("name", list(GRAPHS))
def test_explicit_sweep_agrees(kra, monkeypatch, name):
    """KT_SLQ_YFORM=0 (read at context creation): the explicit K1/K2 sweep
    runs on the same relabelled copy."""
    monkeypatch.setenv("KT_SLQ_YFORM", "0")
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(_graph(name), ctx)
    for m in DEPTHS:
        N = nprobes_for(16)
        q = kra.slq_quadforms(D, N, m, seed=SEED, block=16, ctx=ctx)[2]
        np.testing.assert_allclose(q, _oracle(name, m)[:N], rtol=RTOL)

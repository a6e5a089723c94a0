"""Host-side checks of the f(A) entries estimator's interface (no GPU): the
binding of kt_entries_fun, the argument checks of entries_fun that happen
before any device is touched, the ordering and tie rule of find_top_edges_fun
with entries_fun replaced by fixed means, and greedy_krylov's `top` argument."""
import inspect
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph


def test_kt_entries_fun_is_bound_with_17_arguments():
    from krylov_robustness_amd import _lib
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert "kt_entries_fun" in sig
    assert len(sig["kt_entries_fun"]) == 17


def test_entries_fun_rejects_bad_pairs_before_touching_a_device(monkeypatch):
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import core

    def no_device(*a, **k):
        raise AssertionError("a device was touched")

    monkeypatch.setattr(core, "_dev", no_device)
    monkeypatch.setattr(core, "eigs_leading", no_device)
    A = load_graph("denmark")
    n = A.shape[0]
    bad = [np.zeros((4, 3), dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros((0, 2), dtype=np.int64),
           np.array([[0, n]]), np.array([[-1, 0]]), np.array([[0.0, 1.0]])]
    for P in bad:
        with pytest.raises(ValueError):
            kra.entries_fun(A, P, 16)
    with pytest.raises(ValueError):
        kra.entries_fun(A, np.array([[0, 1]]), 16, deflate=2)
    # a good list gets as far as the device
    with pytest.raises(AssertionError, match="a device was touched"):
        kra.entries_fun(A, np.array([[0, n - 1]]), 16)


def _path_with_ties():
    """6 nodes, edges in find(tril(A, -1)) order: (1,0) (2,0) (3,1) (4,2) (5,3) (5,4)."""
    i = np.array([1, 2, 3, 4, 5, 5])
    j = np.array([0, 0, 1, 2, 3, 4])
    A = sp.csc_matrix((np.ones(6), (i, j)), shape=(6, 6))
    return (A + A.T).tocsc(), np.stack([i, j], axis=1)


def test_find_top_edges_fun_order_and_ties(monkeypatch):
    """entries_fun replaced by fixed means: rows are 1-based with i > j, ranked
    by descending mean, ties in find(tril(A, -1)) order -- the shape, the
    convention and the tie rule of find_top_edges on keys that tie the same way."""
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import core, greedy
    A, E = _path_with_ties()
    means = np.array([2.0, 5.0, 2.0, 7.0, 2.0, 5.0])
    seen = {}

    class Host:  # stands in for the DeviceMatrix
        def to_scipy(self):
            return A

    def fake_entries(D, pairs, nprobes, **kw):
        seen["pairs"], seen["nprobes"], seen["kw"] = np.array(pairs), nprobes, kw
        return core.EntryEstimate(np.zeros(len(means)), means * nprobes, np.zeros(len(means)), 0.0, 0.0, nprobes)

    monkeypatch.setattr(core, "entries_fun", fake_entries)
    monkeypatch.setattr(greedy, "_dev", lambda A, ctx=None: Host())
    top = kra.find_top_edges_fun(A, 5, fun="sinh", nprobes=32, deflate=None, m=20, seed=9)
    np.testing.assert_array_equal(seen["pairs"], E)  # 0-based, tril order, every edge
    assert seen["nprobes"] == 32 and seen["kw"]["fun"] == "sinh" and seen["kw"]["deflate"] is None
    assert seen["kw"]["m"] == 20 and seen["kw"]["seed"] == 9
    np.testing.assert_array_equal(top, np.array([[5, 3], [3, 1], [6, 5], [2, 1], [4, 2]]))
    assert top.dtype == np.int64 and (top[:, 0] > top[:, 1]).all()
    # find_top_edges with a centrality whose products tie the same way
    ref = kra.find_top_edges(A, np.ones(6), 6, "mult")
    np.testing.assert_array_equal(ref, E + 1)
    monkeypatch.setattr(core, "entries_fun", lambda D, pairs, nprobes, **kw: core.EntryEstimate(
        np.zeros(6), np.ones(6), np.zeros(6), 0.0, 0.0, nprobes))
    np.testing.assert_array_equal(kra.find_top_edges_fun(A, 6), ref)
    # fewer edges than asked for: the warning, then the error, of find_top_edges
    with warnings.catch_warnings(record=True) as wrn:
        warnings.simplefilter("always")
        np.testing.assert_array_equal(kra.find_top_edges_fun(A, 6.5), ref)
    assert any("not enough edges" in str(x.message) for x in wrn)
    with pytest.warns(UserWarning), pytest.raises(IndexError):
        kra.find_top_edges_fun(A, 7)


def test_entry_estimate_mean_and_stderr():
    from krylov_robustness_amd.core import DiagEstimate, EntryEstimate
    e0, s, s2 = np.array([1.0, 0.0]), np.array([8.0, -4.0]), np.array([20.0, 6.0])
    e, d = EntryEstimate(e0, s, s2, 3.0, 5.0, 4), DiagEstimate(e0, s, s2, 3.0, 5.0, 4)
    np.testing.assert_array_equal(e.mean, d.mean)
    np.testing.assert_array_equal(e.stderr, d.stderr)
    assert (e.sum_q, e.sum_q2, e.nprobes) == (3.0, 5.0, 4)
    assert np.isinf(EntryEstimate(e0, s, s2, 0.0, 0.0, 1).stderr).all()


def test_greedy_krylov_signature_accepts_top():
    import krylov_robustness_amd as kra
    p = inspect.signature(kra.greedy_krylov).parameters
    assert "top" in p and p["top"].default is None
    # the reference's positional order is untouched
    assert list(p)[:11] == ["A", "k", "Q", "centrality", "order", "tol", "it", "poles", "debug", "miobi", "rescale"]

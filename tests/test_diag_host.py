"""Host-side checks of the diag f(A) estimator's interface (no GPU): the 'exp'
branch of compute_centrality on a host matrix (compute_centrality.m:9-10,
c = diag(expm(A))), the binding of kt_diag_fun, and argument checks that
happen before any device is touched."""
import numpy as np
import pytest

from conftest import load_graph


def test_compute_centrality_exp_host_is_diag_expm():
    """The reference's subgraph centrality on the weighted `denmark` graph
    (n = 96) against a dense eigendecomposition's exp, to 1e-12 relative."""
    import krylov_robustness_amd as kra
    A = load_graph("denmark")
    c = kra.compute_centrality(A, "exp")
    w, V = np.linalg.eigh(A.toarray())
    ref = (V * V) @ np.exp(w)
    assert c.shape == ref.shape
    np.testing.assert_allclose(c, ref, rtol=1e-12)
    # the other kinds keep their behaviour, the fall-through to 'eig' included
    np.testing.assert_allclose(kra.compute_centrality(A, "deg"), np.asarray(A.sum(axis=0)).ravel())
    e = kra.compute_centrality(A, "eig")
    np.testing.assert_allclose(kra.compute_centrality(A, "no such kind"), e, rtol=1e-9, atol=1e-12)
    assert np.abs(c - e).max() > 0.1


def test_kt_diag_fun_is_bound_with_14_arguments():
    from krylov_robustness_amd import _lib
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert "kt_diag_fun" in sig
    assert len(sig["kt_diag_fun"]) == 14


def test_diag_fun_rejects_larger_int_deflate_before_touching_a_device(monkeypatch):
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import core

    def no_device(*a, **k):
        raise AssertionError("a device was touched")

    monkeypatch.setattr(core, "_dev", no_device)
    monkeypatch.setattr(core, "eigs_leading", no_device)
    A = load_graph("denmark")
    with pytest.raises(ValueError):
        kra.diag_fun(A, 16, deflate=2)

"""CPU: kt_eigs_topk's argument checks, the deflate=k argument of the deflated
estimators, natural_connectivity_topk's closed form, and the kernel-level
check program's host enumeration."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_graph

CHECK = os.path.join(ROOT, "tests", "native", "eig_check", "eig_check")


def test_kt_eigs_topk_rejects_bad_arguments_before_the_device():
    from krylov_robustness_amd import _lib
    lib = _lib.load()
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sig["kt_eigs_topk"]) == 10
    lam = (C.c_double * 40)()
    # a NULL matrix, whatever k
    for k in (0, 1, 33):
        assert lib.kt_eigs_topk(None, k, 0.0, 0, 0, lam, None, None, None, None) == _lib.KT_ERR_ARG
        assert b"kt_eigs_topk" in lib.kt_last_error()


def _no_device(*a, **k):
    raise AssertionError("a device was touched")


def test_deflate_int_up_to_16_is_accepted():
    from krylov_robustness_amd import core
    assert core._deflate_arg("diag_fun", 4) == 4
    assert core._deflate_arg("diag_fun", 16) == 16
    assert core._deflate_arg("diag_fun", np.int64(2)) == 2
    assert core._deflate_arg("diag_fun", 1) == 1
    assert core._deflate_arg("diag_fun", 0) is None
    assert core._deflate_arg("diag_fun", None) is None


@pytest.mark.parametrize("bad", [17, -1, True])
def test_deflate_out_of_range_raises_without_a_device(monkeypatch, bad):
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import core, greedy
    for mod in (core, greedy):
        monkeypatch.setattr(mod, "_dev", _no_device)
    monkeypatch.setattr(core, "eigs_leading", _no_device)
    monkeypatch.setattr(core, "eigs_topk", _no_device)
    A = load_graph("denmark")
    with pytest.raises(ValueError):
        kra.diag_fun(A, 16, deflate=bad)
    with pytest.raises(ValueError):
        kra.entries_fun(A, np.array([[0, 1]]), 16, deflate=bad)
    with pytest.raises(ValueError):
        kra.find_top_edges_fun(A, 5, deflate=bad)
    D = object.__new__(kra.DeviceMatrix)  # compute_centrality's device branch, no device behind it
    with pytest.raises(ValueError):
        kra.compute_centrality(D, "exp", deflate=bad)


def test_deflate_k_on_a_host_matrix_asks_for_a_device_matrix(monkeypatch):
    """An int k >= 2 deflates eigs_topk's vectors of a DeviceMatrix; a host
    matrix is refused before any device work (deflate=1 and arrays still go
    as far as the device)."""
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import core, greedy
    for mod in (core, greedy):
        monkeypatch.setattr(mod, "_dev", _no_device)
    A = load_graph("denmark")
    for call in (lambda: kra.diag_fun(A, 16, deflate=4),
                 lambda: kra.entries_fun(A, np.array([[0, 1]]), 16, deflate=16),
                 lambda: kra.find_top_edges_fun(A, 5, deflate=2)):
        with pytest.raises(ValueError, match="DeviceMatrix"):
            call()
    with pytest.raises(AssertionError, match="a device was touched"):
        kra.diag_fun(A, 16, deflate=1)
    D = object.__new__(kra.DeviceMatrix)  # no device behind it: the check passes, the next step needs one
    assert core._deflate_arg("diag_fun", 4, D) == 4


def test_deflate_k_takes_eigs_topk_and_warns_when_unconverged(monkeypatch):
    from krylov_robustness_amd import core
    n, k = 12, 3
    Q = np.linalg.qr(np.random.default_rng(0).normal(size=(n, k)))[0]
    calls = []

    def fake_topk(D, kk, ctx=None, return_info=False, **kw):
        calls.append(kk)
        return np.arange(kk, 0, -1.0), Q, (np.zeros(kk), fake_topk.nconv, 7)

    monkeypatch.setattr(core, "eigs_topk", fake_topk)
    monkeypatch.setattr(core, "eigs_leading", _no_device)
    fake_topk.nconv = k
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = core._deflation("diag_fun", None, n, k, None)
    np.testing.assert_array_equal(out, Q)
    assert out.flags.f_contiguous and calls == [k]
    fake_topk.nconv = 1
    with pytest.warns(RuntimeWarning, match="nconv = 1"):
        core._deflation("diag_fun", None, n, k, None)


def test_natural_connectivity_topk_closed_form(monkeypatch):
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import core
    lam = np.array([700.0, 699.5, 3.0, -1.0])  # exp(700) alone is near the overflow edge: the shifted form holds

    def fake_topk(A, k, **kw):
        return lam[:k].copy(), None

    monkeypatch.setattr(core, "eigs_topk", fake_topk)
    A = np.zeros((50, 50))
    for k in (1, 2, 4):
        want = 700.0 + np.log(np.sum(np.exp(lam[:k] - 700.0))) - np.log(50.0)
        assert kra.natural_connectivity_topk(A, k) == pytest.approx(want, rel=1e-15)
    small = np.array([2.0, 1.0, 0.5])
    monkeypatch.setattr(core, "eigs_topk", lambda A, k, **kw: (small[:k].copy(), None))
    assert kra.natural_connectivity_topk(A, 3) == pytest.approx(np.log(np.exp(small).sum() / 50.0), rel=1e-14)


def test_eig_check_host_enumeration():
    """The kernel-level check's cases pass on its host stand-ins (the cases and
    expectations themselves are sound) and every group has some."""
    assert os.path.exists(CHECK), "tests/native/eig_check/eig_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mode"] == "host" and "hip_error" not in out
    assert set(out["groups"]) == {"rotate", "resid", "start"}
    for g in out["groups"].values():
        assert g["cases"] > 0 and g["failed_count"] == 0 and g["failed"] == []

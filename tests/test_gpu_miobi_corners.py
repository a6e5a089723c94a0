"""GPU tests of the window loop the three MIOBI drivers share (kt_miobi.cpp,
DESIGN.md §4.2e): the corners of the window arithmetic that the parity tests'
K = 24 (12 for the node removal) with refresh 8 / 0 (50 / 0) do not reach --
one step, a recomputation after every step, a window longer than the run, and
no step at all.

Every case with a step runs the driver's own test_parity_with_the_restatement
(tests/test_gpu_miobi.py, test_gpu_miobi_make.py, test_gpu_miobi_node.py) on
anaheim with that module's K set to the case's k: the same helper, the same
bounds, and `refreshes` by the file's own formula (the restatement's count for
the node removal).  miobi_make's (k, refresh) = (5, 1) is not among the cases:
on anaheim its third step is a tie to rounding (the restatement's runner-up
gap is 3.7e-16), so it does not meet the clear-gap bound that parity test
holds anaheim to; the removal and the node removal cover refresh = 1."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_miobi as tb
import test_gpu_miobi_make as tm
import test_gpu_miobi_node as tn

pytestmark = pytest.mark.gpu

STEPS = [(1, 8), (5, 1), (5, 100)]


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


def no_step(kra, ctx, A, t, seed, picked, info, D, columns):
    """What a k = 0 call returns: nothing selected, the matrix as it was, one
    track row -- the eigenvalues of the input, bit for bit."""
    assert len(picked) == 0 and info["scores"].shape == (0,) and info["refreshes"] == 0
    assert picked.shape == ((0, 2) if columns == 2 else (0,))
    got = sp.csr_matrix(D.to_scipy())
    assert got.nnz == A.nnz and abs(got - A).nnz == 0
    lam = np.asarray(kra.eigs_topk(D, t, seed=seed, ctx=ctx)[0])
    assert info["track"].shape == (1, t) and info["track"][0].tobytes() == lam.tobytes()


@pytest.mark.parametrize("k,refresh", STEPS + [(0, 8)])
def test_break(kra, gpu_ctx, monkeypatch, k, refresh):
    """With k = 0 and return_V the vectors come back as staged.  After a call
    kt_context_stat 10-12 describe it: host microseconds of its
    eigensolver runs, its staging and its edits, within the call's wall time."""
    A, t = tb.graph("anaheim")
    D = kra.DeviceMatrix(A, gpu_ctx)
    t0 = time.perf_counter()
    edges, info = kra.miobi_break(D, k, t=t, refresh=refresh, seed=tb.SEED, return_V=True, ctx=gpu_ctx)
    wall_us = (time.perf_counter() - t0) * 1e6
    parts = [gpu_ctx.stat(s) for s in (10, 11, 12)]
    print("k", k, "refresh", refresh, "stats 10-12", parts, "wall us", wall_us)
    if k == 0:
        no_step(kra, gpu_ctx, A, t, tb.SEED, edges, info, D, 2)
        V0 = np.array(kra.eigs_topk(D, t, seed=tb.SEED, ctx=gpu_ctx)[1])
        V0[:, 0] = np.abs(V0[:, 0])  # the vectors as staged: column 0 by absolute value
        assert info["V"].shape == V0.shape and info["V"].tobytes() == V0.tobytes()
    else:
        monkeypatch.setattr(tb, "K", k)
        tb.test_parity_with_the_restatement(kra, gpu_ctx, "anaheim", refresh)
    assert parts[0] > 0 and sum(parts) <= wall_us


@pytest.mark.parametrize("k,refresh", [(1, 8), (5, 100), (0, 8)])
def test_make(kra, gpu_ctx, monkeypatch, k, refresh):
    if k == 0:
        A, _ = tm.graph("anaheim")
        D = kra.DeviceMatrix(A, gpu_ctx)
        edges, info = kra.miobi_make(D, 0, t=tm.T, refresh=refresh, seed=tm.SEED, ctx=gpu_ctx)
        assert info["m"].shape == (0,)
        no_step(kra, gpu_ctx, A, tm.T, tm.SEED, edges, info, D, 2)
    else:
        monkeypatch.setattr(tm, "K", k)
        tm.test_parity_with_the_restatement(kra, gpu_ctx, "anaheim", refresh)


@pytest.mark.parametrize("shift", ["reference", "first_order"])
@pytest.mark.parametrize("k,refresh", STEPS + [(0, 8)])
def test_break_node(kra, gpu_ctx, monkeypatch, k, refresh, shift):
    if k == 0:
        A, t = tn.graph("anaheim")
        D = kra.DeviceMatrix(A, gpu_ctx)
        nodes, info = kra.miobi_break_node(D, 0, t=t, refresh=refresh, shift=shift, seed=tn.SEED, ctx=gpu_ctx)
        assert info["degrees"].shape == (0,)
        no_step(kra, gpu_ctx, A, t, tn.SEED, nodes, info, D, 1)
    else:
        monkeypatch.setattr(tn, "K", k)
        tn.test_parity_with_the_restatement(kra, gpu_ctx, "anaheim", refresh, shift)
